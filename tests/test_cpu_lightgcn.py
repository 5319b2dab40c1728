"""The LightGCN contract on the CPU (ultrare_amd/lightgcn.py): it IS LightGCN -- torch float64 autograd on the dense normalised
adjacency is the yardstick --, it is told apart from the near misses a wrong trainer would compute, its float32 stage contracts
stay within derived rounding bounds of their float64 versions, and every refusal of the new surface comes before any device work.
tests/test_gpu_lightgcn.py holds the kernels to these functions bit for bit."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import lightgcn_cases as C
import sgd_cases
from test_cpu_score_contract import tables as mixed_tables
from ultrare_amd import lightgcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u) for float32: the relative error of k successive roundings."""
    return k * U32 / (1 - k * U32)


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ------------------------------------------------------------------ 1. the contract is LightGCN
@pytest.mark.parametrize('case', C.SMALL_CASES, ids=repr)
def test_contract_equals_torch_autograd_in_float64(case):
    """train_ref(float64) against torch float64 autograd on the dense adjacency, MSELoss(sum), SGD(momentum, weight_decay): within
    1e-9 (the figure tests/test_cpu_adam.py holds its restatement to) over both final tables, both parameter tables and the epoch
    losses.  L = 1, 2, 3; a repeated pair; users and items without a rating."""
    ref, yard = case.train_ref(), C.torch_lightgcn(case, torch.float64)
    for k in ('U', 'V', 'P', 'Q', 'loss'):
        assert np.isfinite(ref[k]).all() and np.isfinite(yard[k]).all(), k
    assert C.distance(yard, ref) <= 1e-9
    assert (case.uid[0], case.iid[0]) == (case.uid[-1], case.iid[-1])
    assert set(range(case.no_u)).isdisjoint(case.uid) and set(range(case.no_i)).isdisjoint(case.iid)
    assert not np.array_equal(ref['U'][-1], ref['P'][-1])                    # the layers do something


def test_cases_cover_the_layer_counts():
    assert {c.layers for c in C.SMALL_CASES} == {1, 2, 3} == {c.layers for c in C.WHOLE_STEP_CASES}
    assert [c.d for c in C.WHOLE_STEP_CASES] == [8, 32, 64, 128, 256]
    assert all(c.N % c.B for c in C.WHOLE_STEP_CASES)                        # a partial last step


@pytest.mark.parametrize('case', C.SMALL_CASES[:2], ids=repr)
def test_zero_layers_is_the_sgd_restatement(case):
    got = case.train_ref(layers=0)
    U, V, loss = sgd_cases.sgd_train_ref(case.uid, case.iid, case.rating, case.U0, case.V0, case.orders, case.B, case.lr_host, case.lam, case.mu)
    assert C.distance(dict(U=U, V=V, P=U, Q=V, loss=loss), got) <= 1e-12
    assert np.array_equal(got['U'], got['P']) and np.array_equal(got['V'], got['Q'])


# ------------------------------------------------------------------ 2. told apart from near misses
@pytest.mark.parametrize('plant', lightgcn.PLANTS)
@pytest.mark.parametrize('case', C.SMALL_CASES, ids=repr)
def test_contract_is_told_apart_from_the_near_misses(case, plant):
    """Each plant is further from the torch float64 run than 100 x the distance the true contract has on the same case."""
    yard = C.torch_lightgcn(case, torch.float64)
    true = C.distance(yard, case.train_ref())
    planted = C.distance(yard, case.train_ref(plant=plant))
    assert planted > 100 * max(true, np.finfo(np.float64).eps), (plant, planted, true)


# ------------------------------------------------------------------ 3. float32 stages against their float64 versions
def test_propagate_float32_is_within_its_rounding_bound():
    """A chain of n terms: one rounding per product, at most n - 1 per addition chain, one for s_dst: |y32 - y64| <=
    gamma_(n + 1) s_dst sum |s_j x_j|; with add one more rounding of the whole: gamma_(n + 2) (|add| + s_dst sum |s_j x_j|).  The
    chain depth of a row is its length."""
    row, idx, lengths = C.prop_rows(67)
    g = lightgcn.Graph(row, idx, 67, C.N_SRC)
    off, idx, s_src, s_dst, n_dst, n_src = g.side('csr')
    (X, _), = mixed_tables(1, 8, 1, n_user=n_src, n_item=1)
    (add, _), = mixed_tables(2, 8, 1, n_user=n_dst, n_item=1)
    n = np.diff(off)[:, None]
    mag = lightgcn.propagate_ref(off, idx, s_src, s_dst, np.abs(X), dtype=np.float64)
    for a, extra in ((None, 1), (add, 2)):
        y32 = lightgcn.propagate_ref(off, idx, s_src, s_dst, X, add=a)
        y64 = lightgcn.propagate_ref(off, idx, s_src, s_dst, X, add=a, dtype=np.float64)
        assert y32.dtype == np.float32 and y64.dtype == np.float64
        bound = gamma(n + extra) * (mag + (0 if a is None else np.abs(a))) * (1 + 1e-6)
        err = np.abs(y32.astype(np.float64) - y64)
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
        assert err.max() > 0                                                 # (a float32 result: it does round)
    assert max(lengths) == C.LONG_ROW and np.array_equal(y32[[0, -1]], add[[0, -1]])              # an empty row gives add unchanged ...
    plain = lightgcn.propagate_ref(off, idx, s_src, s_dst, X)
    assert plain[[0, -1]].tobytes() == bytes(2 * 8 * 4)                                            # ... or +0.0
    acc = add.copy()
    y = lightgcn.propagate_ref(off, idx, s_src, s_dst, X, sum=acc)
    assert np.array_equal(acc, add + y)


def test_update_float32_is_within_its_rounding_bound():
    """w' = w - lr (mu m + (g + lam w)): six roundings between the inputs and w', four between them and m:
    |w32' - w64'| <= gamma_6 (|w| + lr (|mu m| + |g| + |lam w|)), |m32 - m64| <= gamma_4 (|mu m| + |g| + |lam w|)."""
    (w, _), (m, _), (g, _) = mixed_tables(3, 16, 3, n_user=129, n_item=1)
    for lam, mu, lr_decay, _ in (sgd_cases.DEFAULT, sgd_cases.NO_DECAY, sgd_cases.NO_MOMENTUM, sgd_cases.PLAIN, sgd_cases.MIXED, sgd_cases.LARGE):
        for first in (True, False):
            lr = sgd_cases.LR * lr_decay
            w32, m32 = lightgcn.sgd_update_ref(w, m, g, lr, lam, mu, first)
            w64, m64 = lightgcn.sgd_update_ref(w, m, g, lr, lam, mu, first, dtype=np.float64)
            assert w32.dtype == m32.dtype == np.float32
            lam_, mu_, lr_ = (float(np.float32(x)) for x in (lam, 0.0 if first else mu, lr))
            mag = np.abs(mu_ * m.astype(np.float64)) + np.abs(g) + np.abs(lam_ * w.astype(np.float64))
            assert (np.abs(m32 - m64) <= gamma(4) * mag).all()
            assert (np.abs(w32 - w64) <= gamma(6) * (np.abs(w) + lr_ * mag)).all()
    zero = np.zeros((3, 4), np.float32)
    w0, m0 = lightgcn.sgd_update_ref(zero, zero, zero, 1e-3, 0.1, 0.9, False)
    assert not w0.any() and not m0.any()                                     # padding columns stay exactly zero


@pytest.mark.parametrize('d', (4, 16, 64))
def test_loss_gradient_float32_is_within_its_rounding_bound(d):
    """pred: the score contract's depth 4 + log2(d / 4) (tests/test_cpu_score_contract.py, the strict count): dp = gamma_depth sum
    |u_c v_c|.  e = pred - r adds one rounding: de = dp + u (|e| + dp).  A row's chain of n_b batch entries: a rounding for 2 e v and
    at most n_b for the additions, on terms that carry de: |G32 - G64| <= sum 2 de |v| + gamma_(n_b + 1) sum 2 (|e| + de) |v|.
    The loss: |e32^2 - e64^2| <= de (2 |e| + de) per entry."""
    case = C.Case(37, 29, d, 300, 128, 1, 2, seed=77, no_u=5, no_i=4)
    g = lightgcn.Graph(case.uid, case.iid, case.n_user, case.n_item)
    (U, V), = mixed_tables(4 + d, d, 1, n_user=case.n_user, n_item=case.n_item)
    U, V = U * np.float32(0.25), V * np.float32(0.25)
    batch = case.orders[0][case.B:2 * case.B]
    Gu32, Gi32, loss32, pred32 = lightgcn.loss_grad_ref(g, U, V, case.rating, batch)
    Gu64, Gi64, loss64, pred64 = lightgcn.loss_grad_ref(g, U, V, case.rating, batch, dtype=np.float64)
    u, i = case.uid[batch].astype(np.int64), case.iid[batch].astype(np.int64)
    dp = gamma(4 + int(np.log2(d // 4))) * (np.abs(U[u].astype(np.float64) * V[i])).sum(axis=1)
    assert (np.abs(pred32[batch].astype(np.float64) - pred64[batch]) <= dp).all()
    e = np.abs(pred64[batch] - case.rating[batch])
    de = dp + U32 * (e + dp)
    for G32, G64, own, other, n_rows in ((Gu32, Gu64, u, np.abs(V[i]).astype(np.float64), case.n_user), (Gi32, Gi64, i, np.abs(U[u]).astype(np.float64), case.n_item)):
        n_b = np.bincount(own, minlength=n_rows)[:, None]
        carried, terms = np.zeros(G64.shape), np.zeros(G64.shape)
        np.add.at(carried, own, 2 * de[:, None] * other)
        np.add.at(terms, own, 2 * (e + de)[:, None] * other)
        bound = (carried + gamma(n_b + 1) * terms) * (1 + 1e-6)
        err = np.abs(G32.astype(np.float64) - G64)
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
        assert not G32[n_b[:, 0] == 0].any() and err.max() > 0
    assert abs(loss32 - loss64) <= (de * (2 * e + de)).sum() * (1 + 1e-6) + 1e-12 * loss64
    assert np.isnan(pred32).sum() == case.N - len(batch)


def test_fold_order_is_told_apart_from_a_plain_sum():
    rs = np.random.RandomState(9)
    x = rs.standard_normal(700) * np.exp(3 * rs.standard_normal(700))
    got = lightgcn.fold_256(x)
    assert abs(got - float(np.sum(x.astype(np.longdouble)))) <= 12 * 2.0 ** -53 * np.abs(x).sum()
    assert got != float(np.sum(x)) or got != sum(x.tolist())
    assert lightgcn.fold_256([]) == 0.0 and lightgcn.fold_256([1.5]) == 1.5


def test_the_fused_multiply_add_of_the_score_is_exact():
    """_fma32 rounds once: against exact rational arithmetic on values chosen to sit near float32 midpoints."""
    from fractions import Fraction
    rs = np.random.RandomState(11)
    a = rs.standard_normal(4000).astype(np.float32)
    b = rs.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * rs.choice([1, 1, 2 ** 12, 2 ** -12], 4000).astype(np.float32)
    got = lightgcn._fma32(a, b, c)
    for k in range(0, 4000, 7):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo, hi = np.nextafter(got[k], np.float32(-np.inf)), np.nextafter(got[k], np.float32(np.inf))
        assert abs(Fraction(float(got[k])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), k


# ------------------------------------------------------------------ 4. refusals and wiring
def test_graph_refusals_come_before_any_device_work():
    """No device is visible to this test: a ValueError (not the NativeError of a missing device) shows the order."""
    from ultrare_amd import engine
    ok = (np.array([0, 1]), np.array([0, 2]), np.array([1.0, 0.5]))
    for uid, iid, r, n_user, n_item, msg in ((np.array([0, 2]), ok[1], ok[2], 2, 3, 'user id'), (ok[0], np.array([0, 3]), ok[2], 2, 3, 'item id'),
                                             (np.array([-1, 0]), ok[1], ok[2], 2, 3, 'user id'), (ok[0], ok[1], ok[2][:1], 2, 3, 'rating has shape'),
                                             (ok[0][:0], ok[1][:0], ok[2][:0], 2, 3, 'at least one triple'), (ok[0], ok[1], ok[2], 0, 3, 'n_user')):
        with pytest.raises(ValueError, match=msg):
            engine.GcnGraph(uid, iid, r, n_user, n_item, device='cuda')
    for bad in (12, 2, 512, 0):
        with pytest.raises(ValueError, match='power of two'):
            lightgcn.check_width(bad)


def test_job_refusals_come_before_any_device_work():
    from ultrare_amd import engine
    g = types.SimpleNamespace(n_user=3, n_item=4, N=5, nnz=5, device='cuda')
    P, Q = np.zeros((3, 8), np.float32), np.zeros((4, 8), np.float32)
    orders = np.stack([np.arange(5), np.arange(5)[::-1]]).astype(np.int32)
    make = lambda **kw: engine.GcnJob(**{**dict(graph=g, init=(P, Q), orders=orders, k=8, layers=2, batch=2, epochs=2, lr=1e-3, lam=0.1, momentum=0.9), **kw})
    for kw, msg in ((dict(layers=9), 'layers'), (dict(layers=-1), 'layers'), (dict(layers=1.5), 'layers'), (dict(layers=True), 'layers'),
                    (dict(k=300), 'width'), (dict(batch=0), 'batch'), (dict(init=(P[:2], Q)), 'init tables'), (dict(orders=orders[:1]), 'orders must be'),
                    (dict(orders=orders.astype(np.float32)), 'orders must be'), (dict(orders=np.zeros((2, 5), np.int32)), 'not a permutation'),
                    (dict(orders=orders + 1), 'not a permutation')):
        with pytest.raises(ValueError, match=msg):
            make(**kw)


def test_surface_refusals_and_defaults(monkeypatch):
    from ultrare_amd.config import InsParam, Instance
    from ultrare_amd.main import parser
    from ultrare_amd.method import sisa
    from ultrare_amd.method.scratch import Scratch
    data = os.path.join(ROOT, 'tests', 'golden')
    p = InsParam('toy', 2, data_dir=data)
    assert (p.model, p.gcn_layers) == ('mf', 2)
    q = InsParam('toy', 2, data_dir=data, model='lightgcn', gcn_layers=3)
    assert (q.model, q.gcn_layers, q.layers) == ('lightgcn', 3, [32])
    for kw, msg in ((dict(model='dmf'), 'model'), (dict(model='lightgcn', optimizer='adam'), "optimizer='sgd' only"), (dict(gcn_layers=9), 'layers')):
        with pytest.raises(ValueError, match=msg):
            InsParam('toy', 2, data_dir=data, **kw)
    assert Scratch(q, 'lightgcn').gcn_layers == 3 and Scratch(p, 'lightgcn').gcn_layers == 2
    with pytest.raises(NotImplementedError):
        Scratch(p, 'dmf')
    q.optimizer = 'adam'
    with pytest.raises(ValueError, match="optimizer='sgd' only"):
        Scratch(q, 'lightgcn')
    q.optimizer = 'sgd'
    with pytest.raises(ValueError, match='given_model'):
        Scratch(q, 'lightgcn')._gcn_job(None, False, object())
    q.parallel = True
    with pytest.warns(UserWarning, match='one after the other'):
        s = sisa.Sisa(q, 'lightgcn', 3, [])
    assert s.parallel is False
    assert sisa.Sisa(q, 'mf', 3, []).parallel is True
    two = types.SimpleNamespace(get_world_size=lambda: 2)
    monkeypatch.setattr(sisa, '_dist', lambda: two)
    with pytest.raises(ValueError, match='one rank, not 2'):
        sisa.Sisa(q, 'lightgcn', 3, [])
    with pytest.raises(ValueError, match='one rank, not 2'):
        s.learn([None] * 3, [None] * 3, None, 0, '')
    with pytest.raises(ValueError, match='one rank, not 2'):
        s.unlearn([], [None] * 3, [None] * 3, None, [], 0, '')
    sisa.Sisa(q, 'mf', 3, [])                                               # (MF is not refused)
    args = parser.parse_args(['--model', 'lightgcn', '--gcn-layers', '3', '--layer', '64', '32'])
    assert (args.model, args.gcn_layers, args.layer) == ('lightgcn', 3, ['64', '32'])
    assert parser.parse_args([]).model == 'mf' and parser.parse_args([]).gcn_layers == 2
    ins = Instance.__new__(Instance)
    ins.param = q
    assert ins._model() == ('lightgcn', 'LightGCN_')
    ins.param = p
    assert ins._model() == ('mf', 'MF_')


def test_ops_refuse_cpu_tensors():
    from ultrare_amd import _native, engine, ops  # noqa: F401
    z = torch.zeros
    with pytest.raises(_native.NativeError, match='HIP device only'):
        torch.ops.ultrare.gcn_propagate(z(3, dtype=torch.int64), z(1, dtype=torch.int32), z(2), z(2), z(2, 4), None)
    g = types.SimpleNamespace(side=lambda side: (None, None, None, None, 2, 2), device='cuda')
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.gcn_propagate(g, 'csr', z(2, 4))
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.gcn_sgd_step(z(4), z(4), z(4), 1e-3, 0.1, 0.9, True)


def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_gcn.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.GCN_EXPORTS) and not declared & set(nv.EXPORTS) and not declared & set(nv.CSR_PAIR_EXPORTS)
    assert '#include "ultrare_gcn.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    L = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    from ultrare_amd import build
    assert 'gcn.hip' in build.SOURCES and not {'gcn.hip', 'csr_lanes.h', 'score_dot.h'} & set(build.STEP_KERNEL_FILES)
    for name, (res, args) in nv._GCN_PROTOTYPES.items():
        proto = re.search(r'int\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name


BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.addressof(BUF)


def _bad_calls():
    """(entry, arguments) that each entry must refuse: host addresses stand in for device memory -- nothing may touch them."""
    far = P + 32768
    prop = lambda **kw: ('ure_gcn_propagate', [kw.get(k, v) for k, v in (('off', P), ('idx', P), ('n_dst', 4), ('n_src', 4), ('s_src', P), ('s_dst', P), ('X', P),
                                                                        ('d', 8), ('add', None), ('sum', None), ('out', far), ('stream', None))])
    grad = lambda **kw: ('ure_gcn_grad', [kw.get(k, v) for k, v in (('off', P), ('idx', P), ('map', None), ('tag', P), ('err', P), ('n_dst', 4), ('n_src', 4),
                                                                   ('nnz', 9), ('step', 0), ('T', P), ('d', 8), ('G', far), ('row_loss', None), ('stream', None))])
    res = lambda **kw: ('ure_gcn_residual', [kw.get(k, v) for k, v in (('row', P), ('col', P), ('rating', P), ('tag', P), ('nnz', 9), ('step', 0), ('U', P), ('V', P),
                                                                      ('n_user', 4), ('n_item', 4), ('d', 8), ('err', far), ('pred', None), ('stream', None))])
    return [prop(d=12), prop(d=2), prop(d=512), prop(d=0), prop(n_dst=0), prop(n_src=1 << 31), prop(n_dst=1 << 31), prop(X=None), prop(out=None),
            prop(out=P + 64), prop(add=far + 16), prop(sum=far), prop(sum=P), prop(off=None),
            grad(d=24), grad(nnz=0), grad(nnz=1 << 31), grad(step=-1), grad(G=P), grad(T=None), grad(n_dst=0),
            res(d=6), res(nnz=0), res(err=None), res(n_user=0), res(step=-1),
            ('ure_gcn_scale', [P, 6, 0.5, far, None]), ('ure_gcn_scale', [P, 0, 0.5, far, None]), ('ure_gcn_scale', [P, 64, 0.5, P + 16, None]),
            ('ure_gcn_scale', [None, 64, 0.5, far, None]),
            ('ure_gcn_gather_tags', [P, P, 0, far, None]), ('ure_gcn_gather_tags', [P, P, 1 << 31, far, None]), ('ure_gcn_gather_tags', [P, far, 16, P, None]),
            ('ure_gcn_step_loss', [P, 0, 1, far, None]), ('ure_gcn_step_loss', [P, 16, 1, P + 8, None]), ('ure_gcn_step_loss', [None, 16, 1, far, None]),
            ('ure_gcn_sgd_step', [P, far, P + 4096, 6, 1.0, 1e-3, 0.1, 0.9, 1, None]), ('ure_gcn_sgd_step', [P, P + 16, far, 64, 1.0, 1e-3, 0.1, 0.9, 1, None]),
            ('ure_gcn_sgd_step', [P, far, None, 64, 1.0, 1e-3, 0.1, 0.9, 1, None])]


@pytest.mark.parametrize('entry,args', _bad_calls(), ids=lambda v: v if isinstance(v, str) else '')
def test_entries_check_their_arguments_before_any_hip_call(nv, entry, args):
    """Through ctypes on a machine without a device: -1 and the check's own message, and the 'device' memory is untouched."""
    ctypes.memset(P, 0x5A, len(BUF))
    assert getattr(nv.lib(), entry)(*args) == -1
    assert b'argument check failed' in nv.lib().ure_last_error()
    assert BUF.raw == b'\x5a' * len(BUF)
