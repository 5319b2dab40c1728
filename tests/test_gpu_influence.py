"""Newton-step (influence) unlearning on the device (csrc/influence.hip, engine.inf_coef / inf_matvec / inf_grad / inf_dot / inf_solve,
utils.newton_unlearn, Sisa.unlearn_influence) against its numpy contract (ultrare_amd/influence.py): every kernel bit for bit, the
whole solve with the same log and the same bytes, the whole update row for row, reproducibility, the memory contract of every new
entry, and the Sisa / Instance surface."""
import copy
import os

import numpy as np
import pytest
import torch

import influence_cases as C
from abi_arena import Arena, run_prefills, verdict
from ultrare_amd import influence, lightgcn

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
WIDTHS = lightgcn.WIDTHS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _same(got, want):
    got = got.detach().cpu().numpy()
    want = np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _engine():
    from ultrare_amd import engine
    return engine


def _graph(c):
    return _engine().GcnGraph(c.uid, c.iid, c.rating, c.n_user, c.n_item)


# ------------------------------------------------------------------ 1. the kernels, bit for bit
def _check_kernels(c):
    E = _engine()
    g = _graph(c)
    U, V = _dev(c.U), _dev(c.V)
    P, Q = C.direction(c)
    Pd, Qd = _dev(P), _dev(Q)
    e = influence.coef_ref(c.g, c.U, c.V, c.r)
    ed = E.inf_coef(g, U, V)
    assert _same(ed, e)
    assert _same(E.inf_coef(g, U, V, Pd, Qd), influence.coef_ref(c.g, c.U, c.V, c.r, P, Q))
    for active in (None, c.active):
        gU, gV = E.inf_grad(g, U, V, c.l2, active)
        wU, wV = influence.grad_ref(c.g, c.U, c.V, c.r, c.l2, active)
        assert _same(gU, wU) and _same(gV, wV)
        for curvature, damping in (('full', 0.0), ('full', 0.07), ('gn', 0.0)):
            HU, HV = E.inf_matvec(g, U, V, Pd, Qd, c.l2, damping, curvature, active, ed if active is None else None)
            wU, wV = influence.matvec_ref(c.g, c.U, c.V, c.r, P, Q, c.l2, damping, curvature, active)
            assert _same(HU, wU) and _same(HV, wV), (curvature, damping, active is None)
    x, y = P.reshape(-1), np.random.default_rng(5).normal(0, 1, P.size)
    assert float(E.inf_dot(_dev(x), _dev(y)).cpu()[0]) == influence.dot_ref(x, y)
    assert float(E.inf_dot(ed, ed).cpu()[0]) == influence.dot_ref(e, e)


def test_kernels_equal_the_contract_on_case_a():
    """Repeated pairs, a user and an item without triples (+0.0 in every byte), a frozen row on each side."""
    _check_kernels(C.case_a())


@pytest.mark.parametrize('d', WIDTHS)
def test_kernels_equal_the_contract_at_every_width(d):
    """Case B: a row of 130 entries -- two tiles of the widest lane group and a tail of 2 -- beside rows of 3 and 7."""
    _check_kernels(C.case_b(d))


def test_dot_crosses_chunks_and_the_second_level():
    """1, 255, 256, 257 values; one chunk less, exactly and more; 300 chunks (the second level folds more than 256 partials)."""
    E = _engine()
    rng = np.random.default_rng(11)
    for n in (1, 255, 256, 257, influence.DOT_CHUNK - 1, influence.DOT_CHUNK, influence.DOT_CHUNK + 1, 300 * influence.DOT_CHUNK + 5):
        x, y = rng.normal(0, 1, (2, n))
        assert float(E.inf_dot(_dev(x), _dev(y)).cpu()[0]) == influence.dot_ref(x, y), n


# ------------------------------------------------------------------ 2. the whole solve
def _solve_both(c, curvature, damping, iters=512, tol=1e-8, stream=None):
    E = _engine()
    g = _graph(c)
    U, V = _dev(c.U), _dev(c.V)
    gU, gV = influence.grad_ref(c.g, c.U, c.V, c.r, c.l2, c.active)
    want = influence.solve_ref(c.g, c.U, c.V, c.r, -gU, -gV, c.l2, damping, curvature, c.active, None, iters, tol)
    got = E.inf_solve(g, U, V, _dev(-gU), _dev(-gV), c.l2, damping, curvature, c.active, None, iters, tol, stream=stream)
    return got, want


@pytest.mark.parametrize('curvature,damping,iters,status', (('gn', 0.0, 512, 1), ('full', 3.0, 512, 1), ('full', 0.01, 512, 2), ('gn', 0.0, 5, 0),
                                                             ('gn', 0.0, 16, 0), ('gn', 0.0, 17, 0)))
def test_solve_equals_cg_ref(curvature, damping, iters, status):
    """Case A: the same log, the same iters_run and the same x bytes -- converged, frozen on non-positive curvature (case A's random
    tables are no minimiser: the lightly damped full Hessian is indefinite there) and out of iterations inside, at and past a block
    of the log."""
    (xU, xV, log), (wU, wV, wlog) = _solve_both(C.case_a(), curvature, damping, iters)
    assert wlog['status'] == status
    assert (log['iters_run'], log['status']) == (wlog['iters_run'], wlog['status'])
    assert log['rr'].tobytes() == wlog['rr'].tobytes() and log['flag'].tobytes() == wlog['flag'].tobytes()
    assert _same(xU, wU) and _same(xV, wV)


# ------------------------------------------------------------------ 3. the whole update
def _model(c):
    from ultrare_amd.method.utils import MF
    return MF.from_tables(_dev(c.U), _dev(c.V))


def test_newton_unlearn_equals_the_contract_on_case_c():
    """utils.newton_unlearn on the device = newton_unlearn_ref rounded to float32, row for row; the deleted users' rows are +0.0."""
    from ultrare_amd.method import utils
    c = C.case_c()
    wU, wV, wlogs = C.case_c_steps(1)
    m = _model(c)
    logs = utils.newton_unlearn(m, (c.uid, c.iid, c.rating), l2=c.l2)
    assert _same(m.user_mat.weight, wU) and _same(m.item_mat.weight, wV)
    assert _bytes(m.user_mat.weight[_dev(c.deleted)]) == bytes(4 * c.d * len(c.deleted))
    assert len(logs) == 1 and logs[0]['applied'] and logs[0]['iters_run'] == wlogs[0]['iters_run']
    assert logs[0]['rr'].tobytes() == wlogs[0]['rr'].tobytes() and (logs[0]['F_before'], logs[0]['F_after']) == (wlogs[0]['F_before'], wlogs[0]['F_after'])


def test_newton_unlearn_keeps_frozen_rows_and_rejects_bad_steps():
    from ultrare_amd.method import utils
    c = C.case_a()
    applied = []
    for kw in (dict(curvature='gn', damping=4.0, steps=2), dict(curvature='gn', steps=2), dict(steps=2), dict(curvature='gn', damping=4.0, steps=3, iters=1)):
        wU, wV, wlogs = influence.newton_unlearn_ref(c.uid, c.iid, c.rating, c.U, c.V, c.l2, scope=c.scope, **kw)
        m = _model(c)
        logs = utils.newton_unlearn(m, (c.uid, c.iid, c.rating), l2=c.l2, scope=c.scope, **kw)
        assert _same(m.user_mat.weight, wU) and _same(m.item_mat.weight, wV), kw
        assert [(l['applied'], l['status'], l['reason'], l['F_after']) for l in logs] == [(l['applied'], l['status'], l['reason'], l['F_after']) for l in wlogs]
        assert _bytes(m.user_mat.weight[5]) == c.U[5].tobytes() and _bytes(m.item_mat.weight[4]) == c.V[4].tobytes()       # frozen
        assert _bytes(m.user_mat.weight[3]) == bytes(16) and _bytes(m.item_mat.weight[2]) == bytes(16)                    # emptied
        applied.append([l['applied'] for l in logs])
    # two damped steps applied; the undamped Gauss-Newton step overshoots from these random tables; the lightly damped full Hessian is
    # indefinite there (status 2)
    assert applied[0] == [True, True] and applied[1] == [False] and applied[2] == [False] and logs[0]['status'] == influence.RUNNING


# ------------------------------------------------------------------ 4. reproducibility
def test_equal_bytes_on_a_second_stream_and_interleaved():
    E = _engine()
    a, b = C.case_a(), C.case_b(64)
    (xU, xV, log), (wU, wV, wlog) = _solve_both(a, 'gn', 0.0, stream=torch.cuda.Stream())
    torch.cuda.synchronize()
    assert _same(xU, wU) and _same(xV, wV) and log['rr'].tobytes() == wlog['rr'].tobytes()
    # the calls of two shards interleaved, one on a stream of its own
    s2 = torch.cuda.Stream()
    shards = []
    for c, st in ((a, None), (b, s2)):
        P, Q = C.direction(c, 3)
        shards.append((c, _graph(c), _dev(c.U), _dev(c.V), _dev(P), _dev(Q), P, Q, st))
    torch.cuda.synchronize()
    outs = [[], []]
    for _ in range(3):
        for k, (c, g, U, V, Pd, Qd, P, Q, st) in enumerate(shards):
            outs[k].append(E.inf_matvec(g, U, V, Pd, Qd, c.l2, 0.05, 'full', c.active, stream=st))
    torch.cuda.synchronize()
    for k, (c, g, U, V, Pd, Qd, P, Q, st) in enumerate(shards):
        wU, wV = influence.matvec_ref(c.g, c.U, c.V, c.r, P, Q, c.l2, 0.05, 'full', c.active)
        for HU, HV in outs[k]:
            assert _same(HU, wU) and _same(HV, wV)


# ------------------------------------------------------------------ 5. memory contract of every new entry
ENTRIES = [n for n in __import__('ultrare_amd._native', fromlist=['INF_EXPORTS']).INF_EXPORTS if not n.endswith('_scratch')]
ARENA_CASES = [('ure_inf_coef', 'e'), ('ure_inf_coef', 't'), ('ure_inf_walk', 'grad'), ('ure_inf_walk', 'full_csc'), ('ure_inf_dot', ''),
               ('ure_inf_cg_start', ''), ('ure_inf_cg_xr', 'run'), ('ure_inf_cg_xr', 'frozen'), ('ure_inf_cg_beta', ''), ('ure_inf_cg_p', 'run'),
               ('ure_inf_cg_p', 'frozen')]


def _arena_case(entry, mode):
    from ultrare_amd import _native as nv
    L, c = nv.lib(), C.case_b(16)
    g, d = c.g, c.d
    P, Q = C.direction(c)
    e = influence.coef_ref(g, c.U, c.V, c.r)
    t = influence.coef_ref(g, c.U, c.V, c.r, P, Q)
    A = Arena('cuda')
    st = nv.stream_handle()
    rng = np.random.default_rng(2)
    n = 5000
    x, r, p, Ap = rng.normal(0, 1, (4, n))
    state = np.array([3.0, 2.0, 1.5, 1e-16 * 3.0, 0.0, 0.0, 0.25, 0.0])
    if mode == 'frozen':
        state[4] = 1.0
    if entry == 'ure_inf_coef':
        for name, a in (('row', g.row_u), ('col', g.col), ('rating', c.r), ('U', c.U), ('V', c.V), ('P', P), ('Q', Q)):
            A.input(name, a)
        A.output('out', 8 * g.N)
        dirs = ('P', 'Q') if mode == 't' else (None, None)
        call = lambda A: nv.check(L.ure_inf_coef(A.addr('row'), A.addr('col'), A.addr('rating'), g.N, A.addr('U'), A.addr('V'), A.addr(dirs[0]),
                                                 A.addr(dirs[1]), g.n_user, g.n_item, d, A.addr('out'), st), entry)
        want = dict(out=t if mode == 't' else e)
    elif entry == 'ure_inf_walk' and mode == 'grad':
        for name, a in (('off', g.off_u), ('idx', g.col), ('a', e), ('T', c.V), ('X', c.U.astype(np.float64)), ('active', np.array([1, 1, 0], np.uint8))):
            A.input(name, a)
        A.output('out', 8 * c.U.size)
        call = lambda A: nv.check(L.ure_inf_walk(A.addr('off'), A.addr('idx'), None, A.addr('a'), A.addr('T'), None, None, c.l2, A.addr('X'),
                                                 A.addr('active'), g.n_user, g.n_item, g.N, d, A.addr('out'), st), entry)
        want = dict(out=influence.walk_ref(g.off_u, g.col, None, e, c.V, None, None, c.l2, c.U, np.array([1, 1, 0])))
    elif entry == 'ure_inf_walk':
        for name, a in (('off', g.off_i), ('idx', g.row), ('map', g.to_csr), ('a', t), ('T', c.U), ('b', e), ('D', P), ('X', Q)):
            A.input(name, a)
        A.output('out', 8 * c.V.size)
        call = lambda A: nv.check(L.ure_inf_walk(A.addr('off'), A.addr('idx'), A.addr('map'), A.addr('a'), A.addr('T'), A.addr('b'), A.addr('D'), c.l2 + 0.05,
                                                 A.addr('X'), None, g.n_item, g.n_user, g.N, d, A.addr('out'), st), entry)
        want = dict(out=influence.walk_ref(g.off_i, g.row, g.to_csr, t, c.U, e, P, c.l2 + 0.05, Q, None))
    elif entry == 'ure_inf_dot':
        A.input('x', x)
        A.input('y', y := r)
        A.scratch('ws', L.ure_inf_dot_scratch(n))
        A.output('out', 8)
        call = lambda A: nv.check(L.ure_inf_dot(A.addr('x'), A.addr('y'), n, A.addr('ws'), A.size('ws'), A.addr('out'), st), entry)
        want = dict(out=np.array([influence.dot_ref(x, y)]))
    elif entry == 'ure_inf_cg_start':
        A.input('rr', np.array([3.0]))
        A.output('state', 64)                                  # (in place: the call works on a copy of rr made inside the arena)

        def call(A):
            A.view('state')[:8].copy_(A.view('rr'))
            nv.check(L.ure_inf_cg_start(A.addr('state'), 1e-8, st), entry)
        want = dict(state=np.array([3.0, 0.0, 0.0, (1e-8 * 1e-8) * 3.0, 0.0, 0.0, 0.0, 0.0]))
    elif entry == 'ure_inf_cg_xr':
        for name, a in (('state', state), ('x0', x), ('r0', r), ('p', p), ('Ap', Ap)):
            A.input(name, a)
        A.output('x', 8 * n)
        A.output('r', 8 * n)

        def call(A):
            A.view('x').copy_(A.view('x0'))
            A.view('r').copy_(A.view('r0'))
            nv.check(L.ure_inf_cg_xr(A.addr('state'), A.addr('x'), A.addr('r'), A.addr('p'), A.addr('Ap'), n, st), entry)
        alpha = state[0] / state[1]
        want = dict(x=x, r=r) if mode == 'frozen' else dict(x=x + alpha * p, r=r - alpha * Ap)
    elif entry == 'ure_inf_cg_beta':
        A.input('state0', state)
        A.output('state', 64)
        A.output('log_rr', 8)
        A.output('log_flag', 4)

        def call(A):
            A.view('state').copy_(A.view('state0'))
            nv.check(L.ure_inf_cg_beta(A.addr('state'), A.addr('log_rr'), A.addr('log_flag'), 0, 1, st), entry)
        after = state.copy()
        after[[0, 5, 6]] = state[2], state[0] / state[1], state[2] / state[0]
        want = dict(state=after, log_rr=np.array([state[2]]), log_flag=np.array([0], np.int32))
    else:
        assert entry == 'ure_inf_cg_p'
        for name, a in (('state', state), ('p0', p), ('r', r)):
            A.input(name, a)
        A.output('p', 8 * n)

        def call(A):
            A.view('p').copy_(A.view('p0'))
            nv.check(L.ure_inf_cg_p(A.addr('state'), A.addr('p'), A.addr('r'), n, st), entry)
        want = dict(p=p if mode == 'frozen' else r + state[6] * p)
    return A, call, want


@pytest.mark.parametrize('entry,mode', ARENA_CASES)
def test_every_entry_keeps_the_memory_contract_on_dirty_memory(entry, mode):
    """Every new entry through the raw ABI inside guard zones, at exactly its sizer's scratch, its outputs prefilled with 0x00, 0xFF and
    0x5A: no guard byte and no input byte changes, every output byte is written and none depends on the prefill, and the outputs are
    the contract's."""
    assert {e for e, _ in ARENA_CASES} == set(ENTRIES)
    A, call, want = _arena_case(entry, mode)
    reports = run_prefills(A, call, sync=torch.cuda.synchronize)
    assert not verdict(reports)
    for name, w in want.items():
        assert reports[0].outputs[name] == np.ascontiguousarray(w).tobytes(), (entry, mode, name)


# ------------------------------------------------------------------ 6. the surface
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071


class Param:
    """The InsParam fields Scratch / Sisa read."""

    def __init__(self, epochs, k=16, batch=3000, parallel=False):
        self.k, self.lam, self.seed, self.batch = k, 0.1, 42, batch
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, parallel
        self.optimizer = 'sgd'


def _loaders(S, del_user=()):
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, list(del_user), [], S, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], S, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    return idx, trd, ted, loadData(RatingData(np.hstack(te)), 3000, 24, False)


def test_sisa_unlearn_influence_on_the_toy_set(tmp_path):
    from ultrare_amd.method import utils
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import MF, baseTest
    idx, trd, ted, tot = _loaders(3)
    s = Sisa(Param(2), 'mf', 3, idx)
    torch.manual_seed(42)
    ml = s.learn(trd, ted, tot, 0, '')
    del_user = [int(u) for u in idx[1][:5]]
    idx2, trd2, ted2, tot2 = _loaders(3, del_user)
    items = lambda models: [_bytes(m.item_mat.weight) for m in models]
    rows = lambda m, ids: _bytes(m.user_mat.weight.detach()[torch.as_tensor(np.asarray(ids, dtype=np.int64)).cuda()])
    before_items = items(ml)
    s2 = Sisa(Param(2), 'mf', 3, idx2)
    s2.combiner = object()
    ml2 = s2.unlearn_influence([copy.deepcopy(m) for m in ml], trd2, tot2, del_user, 0, str(tmp_path), curvature='gn', steps=1, iters=32)
    assert s2.influenced == [1] and s2.retrained == [] and s2.combiner is None and list(s2.influence_logs) == [1]
    after_items = items(ml2)
    assert after_items[0] == before_items[0] and after_items[2] == before_items[2] and after_items[1] != before_items[1]
    for g in (0, 2):                                        # the merged rows of the unaffected shards' users
        assert rows(ml2[0], idx2[g]) == rows(ml[0], idx2[g])
    assert rows(ml2[0], del_user) == bytes(4 * 16 * len(del_user))                       # the deleted users' merged rows are zero
    kept = [u for u in idx2[1] if u not in del_user]
    assert rows(ml2[0], kept) != rows(ml[0], kept)
    assert all(m.user_mat.weight.data_ptr() == ml2[0].user_mat.weight.data_ptr() for m in ml2)
    # ... and they are the shard's own update: newton_unlearn on (a copy of the merged table, the shard's item table)
    own = MF.from_tables(ml[0].user_mat.weight.detach().clone(), ml[1].item_mat.weight.detach().clone())
    log = utils.newton_unlearn(own, trd2[1], batch=3000, lam=0.1, curvature='gn', steps=1, iters=32)
    assert rows(own, idx2[1]) == rows(ml2[0], idx2[1]) and _bytes(own.item_mat.weight) == after_items[1]
    assert log[0]['rr'].tobytes() == s2.influence_logs[1][0]['rr'].tobytes()
    assert os.path.exists(tmp_path / 'log0.npy')
    again = baseTest(tot2, [MF.from_tables(m.user_mat.weight.detach().clone(), m.item_mat.weight.detach().clone()) for m in ml2])
    assert (s2.log0['total_rmse'], s2.log0['total_ndcg'], s2.log0['total_hr']) == tuple(again)
    # unlearn afterwards still retrains correctly from that state: the same bytes as retraining from the learned state
    s3 = Sisa(Param(2), 'mf', 3, idx2)
    torch.manual_seed(42)
    want = s3.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, '')
    torch.manual_seed(42)
    got = s2.unlearn(ml2, trd2, ted2, tot2, del_user, 0, '')
    assert s2.retrained == [1] and items(got) == items(want) and _bytes(got[0].user_mat.weight) == _bytes(want[0].user_mat.weight)
    assert s2.log0 == s3.log0


def test_the_op_equals_the_engine_path_and_raises_on_cpu_tensors():
    from ultrare_amd import _native as nv, ops  # noqa: F401
    E = _engine()
    c = C.case_b(32)
    g = _graph(c)
    U, V = _dev(c.U), _dev(c.V)
    Pd, Qd = (_dev(a) for a in C.direction(c, 4))
    halves = (g.off_u, g.col, g.row_u, g.off_i, g.row, g.to_csr, g.rating)
    for full, curvature in ((True, 'full'), (False, 'gn')):
        HU, HV = torch.ops.ultrare.inf_matvec(*halves, U, V, Pd, Qd, c.l2, 0.05, full)
        wU, wV = E.inf_matvec(g, U, V, Pd, Qd, c.l2, 0.05, curvature)
        assert _bytes(HU) == _bytes(wU) and _bytes(HV) == _bytes(wV)
    with pytest.raises(nv.NativeError, match='HIP device only'):
        torch.ops.ultrare.inf_matvec(*(t.cpu() for t in halves), U.cpu(), V.cpu(), Pd.cpu(), Qd.cpu(), c.l2)
    with pytest.raises(ValueError, match='int64 off_u'):
        torch.ops.ultrare.inf_matvec(g.off_u.int(), *halves[1:], U, V, Pd, Qd, c.l2)


def _run_main(tmp_path, name, extra):
    import shutil
    from ultrare_amd.main import main
    data = tmp_path / 'data'
    if not data.exists():
        (data / 'toy').mkdir(parents=True)
        shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
        shutil.copy(TEST, data / 'toy' / '0_test.csv')
    save = tmp_path / name
    main(['--dataset', 'toy', '--epoch', '1', '--group', '2', '--group-type', 'uniform', '--verbose', '0', '--data-dir', str(data), '--save-dir', str(save)] + extra)
    base = save / '2' / 'rand' / 'toy_g2'
    out = {}
    for f in sorted(base.rglob('*')):
        if f.is_file():
            key, raw = str(f.relative_to(base)), f.read_bytes()
            if os.path.basename(key).startswith('log') and not os.path.basename(key).startswith('log0'):
                log = np.load(f, allow_pickle=True).item()                       # a shard's epoch log: everything but the wall times
                raw = repr(sorted((k, v) for k, v in log.items() if k != 'time')).encode()
            out[key] = raw
    return out


def test_main_runs_influence_end_to_end_and_the_default_is_unchanged(tmp_path):
    plain = _run_main(tmp_path, 'plain', [])
    retrain = _run_main(tmp_path, 'retrain', ['--unlearn', 'retrain'])
    assert plain.keys() == retrain.keys() and not [k for k in plain if plain[k] != retrain[k]]
    assert b'unlearn' not in plain['param.pkl']                                # the saved parameters of a plain run name no new field
    inf = _run_main(tmp_path, 'influence', ['--unlearn', 'influence'])
    assert 'MF_uniform_sisa_unlearn/log0.npy' in inf and inf.keys() >= {k for k in plain if 'sisa_learn' in k}
    for k in plain:
        if 'sisa_learn' in k:
            assert inf[k] == plain[k], k                                        # learning is the same run
    assert inf['MF_uniform_sisa_unlearn/log0.npy'] != plain['MF_uniform_sisa_unlearn/log0.npy']
    log0 = np.load(tmp_path / 'influence' / '2' / 'rand' / 'toy_g2' / 'MF_uniform_sisa_unlearn' / 'log0.npy', allow_pickle=True).item()
    assert np.isfinite([log0['total_rmse'], log0['total_ndcg'], log0['total_hr']]).all()
