"""The Newton-step (influence) unlearning contract on the CPU (ultrare_amd/influence.py): its Hessian-vector product and gradient ARE
torch float64 autograd's of the objective, its conjugate gradients solve the active system, the freeze rule holds, one and three
steps close the gap to the ALS fixed point of the remaining data, and every refusal of the new surface comes before any device work.
tests/test_gpu_influence.py holds the kernels to these functions bit for bit."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import influence_cases as C
from ultrare_amd import influence, lightgcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ------------------------------------------------------------------ 1. the contract is the objective's Hessian and gradient
def _objective_torch(c):
    u, i = torch.from_numpy(c.uid), torch.from_numpy(c.iid)
    r = torch.from_numpy(c.rating.astype(np.float64))
    nu = c.n_user * c.d

    def resid(theta):
        U, V = theta[:nu].view(c.n_user, c.d), theta[nu:].view(c.n_item, c.d)
        return (U[u] * V[i]).sum(dim=1) - r

    def F(theta):
        e = resid(theta)
        return (e * e).sum() + c.l2 * (theta * theta).sum()
    theta = torch.from_numpy(np.concatenate([c.U.reshape(-1), c.V.reshape(-1)]).astype(np.float64))
    return F, resid, theta


@pytest.fixture(scope='module')
def hessians():
    """Case A's explicit 48 x 48 Hessian (torch.autograd.functional.hessian of F in float64), its Gauss-Newton matrix 2 J^T J +
    2 l2 I from the Jacobian of the residuals, and the gradient."""
    c = C.case_a()
    F, resid, theta = _objective_torch(c)
    H = torch.autograd.functional.hessian(F, theta).numpy()
    J = torch.autograd.functional.jacobian(resid, theta).numpy()
    G = 2.0 * J.T @ J + 2.0 * c.l2 * np.eye(len(theta))
    t = theta.clone().requires_grad_(True)
    F(t).backward()
    assert H.shape == (48, 48)
    return {'full': H, 'gn': G, 'grad': t.grad.numpy()}


def _flat(a, b):
    return np.concatenate([np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)])


def _bound(c, mag):
    """(longest row + d + 4) 2^-52 sum|terms| per component.  With the unit roundoff u = 2^-53, a term of a component passes through
    at most: its coefficient's chain -- one product, 7 additions in the lane, log2(d / 4) in the tree: 8 + log2(d / 4) <= d + 4
    roundings -- then one product with the table entry, at most L additions of the walk (L the longest row), an exact doubling, and
    the closing addition: L + d + 6 roundings of at most u each, relative to the sum of the terms' magnitudes, to first order.
    (L + d + 6) 2^-53 <= (L + d + 4) 2^-52 / 2 + 2^-52: the stated bound is about twice the contract's own worst case, which leaves
    the other half to the autograd yardstick's float64 matrix-vector product."""
    L = int(max(np.diff(c.g.off_u).max(), np.diff(c.g.off_i).max()))
    return (L + c.d + 4) * EPS * mag


def _magnitude(c, P, Q, curvature, active=None):
    """sum |terms| of every component of matvec_ref: the same walk over absolute values (|e| <= |U| . |V| + |r|)."""
    aU, aV, aP, aQ = np.abs(c.U), np.abs(c.V), np.abs(P), np.abs(Q)
    e_abs = influence.coef_ref(c.g, aU, aV, -np.abs(c.r))
    return _flat(*influence.matvec_ref(c.g, aU, aV, c.r, aP, aQ, c.l2, 0.0, curvature, active, e_abs))


@pytest.mark.parametrize('curvature', influence.CURVATURES)
def test_matvec_is_the_explicit_hessian(hessians, curvature):
    c = C.case_a()
    has = _flat(np.repeat(np.diff(c.g.off_u) > 0, c.d), np.repeat(np.diff(c.g.off_i) > 0, c.d))
    for seed in (1, 2):
        P, Q = C.direction(c, seed)
        got = _flat(*influence.matvec_ref(c.g, c.U, c.V, c.r, P, Q, c.l2, 0.0, curvature))
        want = hessians[curvature] @ _flat(P, Q)
        bound = _bound(c, _magnitude(c, P, Q, curvature))
        assert (np.abs(got - want)[has] <= bound[has]).all(), np.max(np.abs(got - want)[has] / bound[has])
        assert (got[~has] == 0).all() and not np.signbit(got[~has]).any()          # emptied rows: +0.0, left out of the system
        # the active system: a direction that is zero off the active rows, the result on the active rows = H_aa v_a (+ 2 damping v_a)
        act = _flat(np.repeat(c.active[0], c.d), np.repeat(c.active[1], c.d))
        Pa, Qa = P * c.active[0][:, None], Q * c.active[1][:, None]
        got = _flat(*influence.matvec_ref(c.g, c.U, c.V, c.r, Pa, Qa, c.l2, 0.05, curvature, c.active))
        v = _flat(Pa, Qa)
        want = (hessians[curvature] + 2 * 0.05 * np.eye(48))[np.ix_(act, act)] @ v[act]
        bound = _bound(c, _flat(*influence.matvec_ref(c.g, np.abs(c.U), np.abs(c.V), c.r, np.abs(Pa), np.abs(Qa), c.l2, 0.05, curvature, c.active,
                                                      influence.coef_ref(c.g, np.abs(c.U), np.abs(c.V), -np.abs(c.r)))))
        assert (np.abs(got[act] - want) <= bound[act]).all()
        assert (got[~act] == 0).all() and not np.signbit(got[~act]).any()


def test_the_gauss_newton_matrix_differs_where_the_residuals_matter(hessians):
    c = C.case_a()
    P, Q = C.direction(c)
    full, gn = (_flat(*influence.matvec_ref(c.g, c.U, c.V, c.r, P, Q, c.l2, 0.0, cv)) for cv in influence.CURVATURES)
    assert np.abs(full - gn).max() > 1e-3                                      # a plant that drops the e term is told apart
    assert np.linalg.eigvalsh(hessians['gn']).min() > 0


def test_grad_is_autograd(hessians):
    c = C.case_a()
    got = _flat(*influence.grad_ref(c.g, c.U, c.V, c.r, c.l2))
    has = _flat(np.repeat(np.diff(c.g.off_u) > 0, c.d), np.repeat(np.diff(c.g.off_i) > 0, c.d))
    e_abs = influence.coef_ref(c.g, np.abs(c.U), np.abs(c.V), -np.abs(c.r))
    mag = _flat(*influence.grad_ref(c.g, np.abs(c.U), np.abs(c.V), c.r, c.l2, None, e_abs))
    assert (np.abs(got - hessians['grad'])[has] <= _bound(c, mag)[has]).all()
    assert (got[~has] == 0).all()
    masked = _flat(*influence.grad_ref(c.g, c.U, c.V, c.r, c.l2, c.active))
    act = _flat(np.repeat(c.active[0], c.d), np.repeat(c.active[1], c.d))
    assert masked[act].tobytes() == got[act].tobytes() and (masked[~act] == 0).all() and not np.signbit(masked[~act]).any()


@pytest.mark.parametrize('d', lightgcn.WIDTHS)
def test_coef_and_dot_orders_at_every_width(d):
    """The stated orders against plain float64 sums: within d (the coefficient) and 16 + 8 + 8 (the dot's chunk chain and two folds)
    roundings of the summed magnitudes."""
    c = C.case_b(d)
    u, i = c.g.row_u, c.g.col
    U, V = c.U.astype(np.float64), c.V.astype(np.float64)
    e = influence.coef_ref(c.g, c.U, c.V, c.r)
    assert (np.abs(e - ((U[u] * V[i]).sum(axis=1) - c.r)) <= (d + 1) * EPS * ((np.abs(U[u] * V[i])).sum(axis=1) + np.abs(c.r))).all()
    P, Q = C.direction(c)
    t = influence.coef_ref(c.g, c.U, c.V, c.r, P, Q)
    want = (P[u] * V[i]).sum(axis=1) + (U[u] * Q[i]).sum(axis=1)
    assert (np.abs(t - want) <= (2 * d + 1) * EPS * (np.abs(P[u] * V[i]).sum(axis=1) + np.abs(U[u] * Q[i]).sum(axis=1))).all()
    x, y = np.random.default_rng(d).normal(0, 1, (2, 3 * influence.DOT_CHUNK + 17))
    assert abs(influence.dot_ref(x, y) - float(np.sum(x * y))) <= 64 * EPS * np.abs(x * y).sum()
    assert influence.dot_ref(x[:5], y[:5]) == lightgcn.fold_256([lightgcn.fold_256(x[:5] * y[:5])])
    with pytest.raises(ValueError, match='both P and Q'):
        influence.coef_ref(c.g, c.U, c.V, c.r, P, None)


# ------------------------------------------------------------------ 2. the solve
@pytest.mark.parametrize('curvature,damping', (('full', 0.03), ('gn', 0.0)))
def test_cg_solves_the_active_system(hessians, curvature, damping):
    c = C.case_a()
    tol = 1e-8
    if curvature == 'full':
        # case A's tables are random, no minimiser: the full Hessian is indefinite there, and the damping that makes the active system
        # positive definite is read off the explicit matrix (half its most negative eigenvalue, and the margin above)
        act = _flat(np.repeat(c.active[0], c.d), np.repeat(c.active[1], c.d))
        lo = np.linalg.eigvalsh(hessians['full'][np.ix_(act, act)]).min()
        assert lo < 0
        damping = damping - lo / 2
    gU, gV = influence.grad_ref(c.g, c.U, c.V, c.r, c.l2, c.active)
    xU, xV, log = influence.solve_ref(c.g, c.U, c.V, c.r, -gU, -gV, c.l2, damping, curvature, c.active, None, 512, tol)
    act = _flat(np.repeat(c.active[0], c.d), np.repeat(c.active[1], c.d))
    A = (hessians[curvature] + 2 * damping * np.eye(48))[np.ix_(act, act)]
    b, x = -_flat(gU, gV)[act], _flat(xU, xV)
    want = np.linalg.solve(A, b)
    cond = np.linalg.cond(A)
    assert log['status'] == influence.CONVERGED and log['iters_run'] == len(log['rr']) <= 512 and log['flag'][-1] == 1 and not log['flag'][:-1].any()
    bb = influence.dot_ref(b, b)
    assert np.sqrt(log['rr'][-1] / bb) <= tol                                      # the recurrence's residual reaches tol ...
    assert np.linalg.norm(A @ x[act] - b) / np.linalg.norm(b) <= tol + cond * EPS   # ... and the true one, up to the recurrence's drift
    assert np.linalg.norm(x[act] - want) / np.linalg.norm(want) <= cond * tol
    assert (x[~act] == 0).all() and not np.signbit(x[~act]).any()


def test_cg_freezes_on_non_positive_curvature():
    """An indefinite matrix planted: status 2 is reported and x keeps the bytes of the last good iteration."""
    D = np.array([1.0, 2.0, 3.0, 4.0, -0.5])
    A = lambda p: D * p
    b = np.array([1.0, 1.0, 1.0, 1.0, 0.6])
    x, log = influence.cg_ref(A, b, 50, 1e-12)
    assert log['status'] == influence.NON_POSITIVE and log['flag'][-1] == 2 and not log['flag'][:-1].any()
    good = log['iters_run'] - 1
    assert good >= 1                                                               # the first direction is still one of positive curvature
    x_good, log_good = influence.cg_ref(A, b, good, 1e-12)
    assert log_good['status'] == influence.RUNNING and x.tobytes() == x_good.tobytes()
    assert log['rr'][-1] == log['rr'][-2] and log['rr'][:-1].tobytes() == log_good['rr'].tobytes()
    x0, log0 = influence.cg_ref(lambda p: -p, b, 50, 1e-12)                        # negative from the start: x stays 0
    assert log0['status'] == influence.NON_POSITIVE and log0['iters_run'] == 1 and not x0.any()
    xz, logz = influence.cg_ref(A, np.zeros(5), 50, 1e-12)                         # a zero right-hand side has converged
    assert logz['status'] == influence.CONVERGED and logz['iters_run'] == 1 and not xz.any()
    xs, logs = influence.cg_ref(lambda p: np.abs(D) * p, b, 2, 1e-12)              # out of iterations: status 0
    assert logs['status'] == influence.RUNNING and logs['iters_run'] == 2


# ------------------------------------------------------------------ 3. the whole update
def test_one_and_three_steps_close_the_gap_to_the_als_fixed_point():
    """Case C.  Gap to the yardstick (600 ALS sweeps on the remaining triples): emptied rows zeroed only -> one step -> three steps.
    Measured here: 7.6e-2 -> 8.4e-3 (9.0 x) -> 9.9e-4 (8.5 x more); the bound is 5 x each."""
    c = C.case_c()
    gap0 = c.F_zeroed - c.F_yard
    U1, V1, logs1 = C.case_c_steps(1)
    U3, V3, logs3 = C.case_c_steps(3)
    gap1, gap3 = c.objective(U1, V1) - c.F_yard, c.objective(U3, V3) - c.F_yard
    print(f'gaps {gap0:.3e} {gap1:.3e} {gap3:.3e} ratios {gap0 / gap1:.2f} {gap1 / gap3:.2f} iterations {[l["iters_run"] for l in logs3]}')
    assert gap0 > 0 and gap1 > 0 and gap3 > 0
    assert gap0 / gap1 >= 5 and gap1 / gap3 >= 5
    assert len(logs1) == 1 and len(logs3) == 3 and all(l['applied'] and l['status'] == influence.CONVERGED for l in logs3)
    assert all(l['F_after'] < l['F_before'] for l in logs3) and logs3[0]['rr'].tobytes() == logs1[0]['rr'].tobytes()
    assert U1.dtype == np.float32 and not U1[c.deleted].any() and not np.signbit(U1[c.deleted]).any()


def test_frozen_and_emptied_rows_and_rejected_steps():
    c = C.case_a()
    # (case A's tables are random, far from a minimiser: the undamped Gauss-Newton step overshoots there and is rejected -- below; a
    # damping of the order of the curvature shortens it to a descent step)
    U, V, logs = influence.newton_unlearn_ref(c.uid, c.iid, c.rating, c.U, c.V, c.l2, curvature='gn', damping=4.0, steps=2, scope=c.scope)
    assert U[5].tobytes() == c.U[5].tobytes() and V[4].tobytes() == c.V[4].tobytes()          # frozen
    assert U[3].tobytes() == bytes(16) and V[2].tobytes() == bytes(16)                        # emptied: +0.0 in every byte
    assert len(logs) == 2 and all(l['applied'] for l in logs) and (U[0] != c.U[0]).any()
    # case A's tables are random, no minimiser: the full Hessian is indefinite there at the default damping, the solve reports status 2,
    # the step is not applied and the second one is not tried -- only the emptied rows have changed
    U1, V1, logs1 = influence.newton_unlearn_ref(c.uid, c.iid, c.rating, c.U, c.V, c.l2, steps=2, scope=c.scope)
    assert len(logs1) == 1 and logs1[0]['status'] == influence.NON_POSITIVE and not logs1[0]['applied'] and 'curvature' in logs1[0]['reason']
    keep_u, keep_i = np.arange(7) != 3, np.arange(5) != 2
    assert U1[keep_u].tobytes() == c.U[keep_u].tobytes() and V1[keep_i].tobytes() == c.V[keep_i].tobytes() and not U1[3].any() and not V1[2].any()
    # a step that does not reduce F is not applied either and ends the update: the undamped Gauss-Newton step from these tables
    U2, V2, logs2 = influence.newton_unlearn_ref(c.uid, c.iid, c.rating, c.U, c.V, c.l2, curvature='gn', steps=3, scope=c.scope)
    assert len(logs2) == 1 and logs2[0]['status'] == influence.CONVERGED and not logs2[0]['applied'] and 'reduce' in logs2[0]['reason']
    assert logs2[0]['F_after'] >= logs2[0]['F_before'] and U2.tobytes() == U1.tobytes() and V2.tobytes() == V1.tobytes()
    # a solve that runs out of iterations (status 0) is applied exactly when it reduced F
    _, _, logs3 = influence.newton_unlearn_ref(c.uid, c.iid, c.rating, c.U, c.V, c.l2, curvature='gn', damping=4.0, steps=3, iters=1, tol=1e-8)
    assert all(l['status'] == influence.RUNNING for l in logs3)
    for l in logs3:
        assert l['applied'] == (l['F_after'] < l['F_before']) and (l['applied'] or l['reason'])


# ------------------------------------------------------------------ 4. refusals and wiring
def test_argument_checks():
    ok = dict(curvature='full', damping=None, steps=1, iters=512, tol=1e-8, l2=0.5)
    assert influence.check_args(**ok) == (0.5, 0.05) and influence.check_args(**{**ok, 'curvature': 'gn'}) == (0.5, 0.0)
    assert influence.check_args(**{**ok, 'curvature': 'gn', 'damping': 0.0}) == (0.5, 0.0)
    for kw, msg in ((dict(curvature='newton'), "'full' or 'gn'"), (dict(damping=-1e-9), 'damping'), (dict(damping=float('inf')), 'damping'),
                    (dict(damping=float('nan')), 'damping'), (dict(damping=0.0), 'rotation null space'), (dict(steps=0), 'steps'), (dict(steps=1.5), 'steps'),
                    (dict(steps=True), 'steps'), (dict(iters=0), 'iters'), (dict(tol=0.0), 'tol'), (dict(tol=1.0), 'tol'), (dict(tol=1), 'tol'),
                    (dict(l2=0.0), 'l2'), (dict(l2=-1.0), 'l2'), (dict(l2=float('nan')), 'l2')):
        with pytest.raises(ValueError, match=msg):
            influence.check_args(**{**ok, **kw})
    for args, msg in ((('lightgcn', 'mse'), "model='mf' only"), (('mf', 'bpr'), "loss='mse' only"), (('lightgcn', 'bpr'), "model='mf' only")):
        with pytest.raises(ValueError, match=msg):
            influence.check_model(*args)
    for scope in ('some', (None,), ([7], None), ([-1], None), (None, [5]), ([0.5], None)):
        with pytest.raises(ValueError, match='scope'):
            influence.check_scope(scope, 7, 5)
    for bad in (3, 6, 12, 512):
        with pytest.raises(ValueError, match='power of two'):
            influence.coef_ref(C.case_a().g, np.zeros((7, bad)), np.zeros((5, bad)), C.case_a().r)
    assert influence.WIDTHS is lightgcn.WIDTHS


def test_surface_refusals_come_before_any_device_work():
    from ultrare_amd import _native, engine, ops  # noqa: F401
    from ultrare_amd.config import InsParam
    from ultrare_amd.main import parser
    from ultrare_amd.method import sisa, utils
    data = os.path.join(ROOT, 'tests', 'golden')
    p = InsParam('toy', 2, data_dir=data)
    assert not hasattr(p, 'unlearn')                                            # the default leaves the saved param as it was
    assert InsParam('toy', 2, data_dir=data, unlearn='influence').unlearn == 'influence'
    for kw, msg in ((dict(unlearn='forget'), "'retrain' or 'influence'"), (dict(unlearn='influence', model='lightgcn'), "model='mf' only"),
                    (dict(unlearn='influence', model='lightgcn', loss='bpr'), "model='mf' only")):
        with pytest.raises(ValueError, match=msg):
            InsParam('toy', 2, data_dir=data, **kw)
    assert parser.parse_args([]).unlearn == 'retrain' and parser.parse_args(['--unlearn', 'influence']).unlearn == 'influence'
    with pytest.raises(SystemExit):
        parser.parse_args(['--unlearn', 'forget'])
    q = InsParam('toy', 2, data_dir=data, model='lightgcn')
    s = sisa.Sisa(q, 'lightgcn', 3, [])
    with pytest.raises(ValueError, match="model='mf' only"):
        s.unlearn_influence([], [], None, [], 0, '')
    for kw, msg in ((dict(), 'batch and lam'), (dict(l2=0.5, curvature='full', damping=0.0), 'rotation null space'), (dict(l2=0.5, tol=2.0), 'tol'),
                    (dict(batch=10, lam=0.0), 'l2'), (dict(l2=0.5, steps=0), 'steps')):
        with pytest.raises(ValueError, match=msg):
            utils.newton_unlearn(None, (np.zeros(3, np.int64), np.zeros(3, np.int64), np.ones(3, np.float32)), **kw)
    z = torch.zeros
    g = types.SimpleNamespace(n_user=2, n_item=2, nnz=2, N=2, device='cuda')
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.inf_matvec(g, z(2, 4), z(2, 4), z(2, 4, dtype=torch.float64), z(2, 4, dtype=torch.float64), 0.5)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.inf_grad(g, z(2, 4), z(2, 4), 0.5)
    with pytest.raises(ValueError, match='rotation null space'):
        engine.inf_solve(g, z(2, 4), z(2, 4), z(2, 4, dtype=torch.float64), z(2, 4, dtype=torch.float64), 0.5)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.inf_solve(g, z(2, 4), z(2, 4), z(2, 4, dtype=torch.float64), z(2, 4, dtype=torch.float64), 0.5, 0.1)
    i32, i64 = dict(dtype=torch.int32), dict(dtype=torch.int64)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        torch.ops.ultrare.inf_matvec(z(3, **i64), z(2, **i32), z(2, **i32), z(3, **i64), z(2, **i32), z(2, **i32), z(2), z(2, 4), z(2, 4),
                                     z(2, 4, dtype=torch.float64), z(2, 4, dtype=torch.float64), 0.5)


def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_influence.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.INF_EXPORTS)
    assert not declared & (set(nv.EXPORTS) | set(nv.CSR_PAIR_EXPORTS) | set(nv.GCN_EXPORTS) | set(nv.BPR_EXPORTS))
    assert '#include "ultrare_influence.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    L = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    from ultrare_amd import build
    assert 'influence.hip' in build.SOURCES and 'influence.hip' not in build.STEP_KERNEL_FILES
    import inspect
    assert "'ultrare_influence.h'" in inspect.getsource(build.source_hash)      # the header is part of the library's identity
    for name, (res, args) in nv._INF_PROTOTYPES.items():
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    sizer = nv.lib().ure_inf_dot_scratch
    assert [sizer(n) for n in (-1, 0, 1, 4096, 4097, 3 * 4096 + 17)] == [0, 0, 8, 8, 16, 32]
    assert nv.lib().ure_abi_version() == nv.ABI_VERSION


BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.addressof(BUF)


def _bad_calls():
    """(entry, arguments) that each entry must refuse: host addresses stand in for device memory -- nothing may touch them."""
    far, mid = P + 32768, P + 16384
    coef = lambda **kw: ('ure_inf_coef', [kw.get(k, v) for k, v in (('row', P), ('col', P), ('rating', P), ('nnz', 9), ('U', P), ('V', P), ('P', None), ('Q', None),
                                                                   ('n_user', 4), ('n_item', 4), ('d', 8), ('out', far), ('stream', None))])
    walk = lambda **kw: ('ure_inf_walk', [kw.get(k, v) for k, v in (('off', P), ('idx', P), ('map', None), ('a', P), ('T', P), ('b', None), ('D', None), ('reg', 0.5),
                                                                   ('X', P), ('active', None), ('n_dst', 4), ('n_src', 4), ('nnz', 9), ('d', 8), ('out', far),
                                                                   ('stream', None))])
    ws, res = P + 40960, P + 49152                                               # (x, y: 5000 float64 = 40,000 bytes at P)
    dot = lambda **kw: ('ure_inf_dot', [kw.get(k, v) for k, v in (('x', P), ('y', P), ('n', 5000), ('scratch', ws), ('bytes', 16), ('out', res), ('stream', None))])
    xr = lambda **kw: ('ure_inf_cg_xr', [kw.get(k, v) for k, v in (('state', P), ('x', P + 1024), ('r', P + 2048), ('p', P + 3072), ('Ap', P + 4096), ('n', 100),
                                                                  ('stream', None))])
    beta = lambda **kw: ('ure_inf_cg_beta', [kw.get(k, v) for k, v in (('state', P), ('log_rr', P + 1024), ('log_flag', P + 4096), ('it', 0), ('n_log', 100),
                                                                      ('stream', None))])
    pk = lambda **kw: ('ure_inf_cg_p', [kw.get(k, v) for k, v in (('state', P), ('p', P + 1024), ('r', P + 2048), ('n', 100), ('stream', None))])
    return [coef(d=6), coef(d=512), coef(nnz=0), coef(nnz=1 << 31), coef(out=None), coef(out=P + 8), coef(n_user=0), coef(n_item=0), coef(U=None),
            coef(P=P), coef(Q=P), coef(P=far, Q=P),
            walk(d=24), walk(nnz=0), walk(out=None), walk(out=P), walk(n_dst=0), walk(n_src=0), walk(b=P), walk(D=P), walk(reg=-1.0), walk(reg=float('nan')),
            walk(reg=float('inf')), walk(a=None), walk(X=None), walk(active=far + 8), walk(map=far),
            dot(n=0), dot(bytes=8), dot(scratch=None), dot(out=None), dot(scratch=P + 8), dot(out=P + 64), dot(out=ws + 8), dot(x=None),
            ('ure_inf_cg_start', [None, 1e-8, None]), ('ure_inf_cg_start', [P, 0.0, None]), ('ure_inf_cg_start', [P, 1.0, None]),
            ('ure_inf_cg_start', [P, float('nan'), None]),
            xr(n=0), xr(x=None), xr(r=P + 1024 + 8), xr(p=P + 1024), xr(Ap=P + 2048 + 792), xr(state=P + 1024), xr(state=None),
            beta(it=-1), beta(it=100), beta(n_log=0), beta(log_rr=None), beta(log_flag=P + 1024 + 8), beta(state=P + 1024), beta(log_flag=None),
            pk(n=0), pk(p=None), pk(r=P + 1024 + 8), pk(state=P + 1024 + 792), pk(r=None)]


@pytest.mark.parametrize('entry,args', _bad_calls(), ids=lambda v: v if isinstance(v, str) else '')
def test_entries_check_their_arguments_before_any_hip_call(nv, entry, args):
    """Through ctypes on a machine without a device: -1 and the check's own message, and the 'device' memory is untouched."""
    ctypes.memset(P, 0x5A, len(BUF))
    assert getattr(nv.lib(), entry)(*args) == -1
    assert b'argument check failed' in nv.lib().ure_last_error()
    assert BUF.raw == b'\x5a' * len(BUF)
