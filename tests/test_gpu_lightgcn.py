"""The LightGCN backbone on the device (csrc/gcn.hip, engine.GcnGraph / gcn_propagate / GcnJob) against its numpy contract
(ultrare_amd/lightgcn.py): every stage bit for bit, whole training against the float64 restatement with two float32 CPU executions
as the yardstick, reproducibility, the memory contract of every new entry, and the Scratch / Sisa / Instance surface."""
import os

import numpy as np
import pytest
import torch

import lightgcn_cases as C
import sgd_cases
from abi_arena import Arena, run_prefills, verdict
from test_cpu_score_contract import tables as mixed_tables
from ultrare_amd import lightgcn

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
WIDTHS = lightgcn.WIDTHS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def _engine():
    from ultrare_amd import engine
    return engine


# ------------------------------------------------------------------ 5. propagate, bit for bit
_PROP = {}


def _prop_graph(n_rows, side):
    """The matrix of lightgcn_cases.prop_rows as the `side` half of a GcnGraph (for 'csc' the triples are transposed, so that
    the items' rows have the lengths under test), made once per process."""
    if (n_rows, side) not in _PROP:
        row, idx, lengths = C.prop_rows(n_rows)
        uid, iid, n_user, n_item = (row, idx, n_rows, C.N_SRC) if side == 'csr' else (idx, row, C.N_SRC, n_rows)
        g = _engine().GcnGraph(uid, iid, np.ones(len(row), np.float32), n_user, n_item)
        off = g.host.side(side)[0]
        assert list(np.diff(off)) == list(lengths)
        _PROP[n_rows, side] = g
    return _PROP[n_rows, side]


@pytest.mark.parametrize('n_rows', C.ROW_COUNTS)
@pytest.mark.parametrize('d', WIDTHS)
def test_propagate_equals_the_contract_bit_for_bit(d, n_rows):
    """Row lengths 0 .. 300 and one of 1,500, the first and the last row empty, indices 0 and n_src - 1, 1 / 67 / 257 rows (a
    partial last workgroup at every group width), both sides, with and without add and sum, and out being add; tables of mixed
    magnitudes."""
    E = _engine()
    for side in ('csr', 'csc'):
        g = _prop_graph(n_rows, side)
        off, idx, s_src, s_dst, n_dst, n_src = g.host.side(side)
        (X, _), = mixed_tables(500 + d + n_rows, d, 1, n_user=n_src, n_item=1)
        (add, _), (acc, _) = mixed_tables(600 + d + n_rows, d, 2, n_user=n_dst, n_item=1)
        Xd = _dev(X)
        want = lightgcn.propagate_ref(off, idx, s_src, s_dst, X)
        assert _same(E.gcn_propagate(g, side, Xd), want), (side, 'plain')
        want_add = lightgcn.propagate_ref(off, idx, s_src, s_dst, X, add=add)
        assert _same(E.gcn_propagate(g, side, Xd, add=_dev(add)), want_add), (side, 'add')
        assert not np.array_equal(want, want_add) or n_dst == 0
        acc_ref = acc.copy()
        want_sum = lightgcn.propagate_ref(off, idx, s_src, s_dst, X, sum=acc_ref)
        acc_d = _dev(acc)
        assert _same(E.gcn_propagate(g, side, Xd, sum=acc_d), want_sum) and _same(acc_d, acc_ref), (side, 'sum')
        acc_ref = acc.copy()
        lightgcn.propagate_ref(off, idx, s_src, s_dst, X, add=add, sum=acc_ref)
        acc_d, io = _dev(acc), _dev(add)
        out = E.gcn_propagate(g, side, Xd, add=io, sum=acc_d, out=io)                # out IS add
        assert out is io and _same(io, want_add) and _same(acc_d, acc_ref), (side, 'in place')
        empty = np.flatnonzero(np.diff(off) == 0)
        if len(empty):
            got = E.gcn_propagate(g, side, Xd).cpu().numpy()
            assert got[empty].tobytes() == np.zeros((len(empty), d), np.float32).tobytes()       # +0.0 in every byte


def test_propagate_refusals_on_the_device():
    E = _engine()
    g = _prop_graph(67, 'csr')
    X = torch.zeros(C.N_SRC, 8, device='cuda')
    with pytest.raises(E.nv.NativeError, match='HIP device only'):
        E.gcn_propagate(g, 'csr', X.cpu())
    with pytest.raises(ValueError, match='X must be'):
        E.gcn_propagate(g, 'csc', X)
    with pytest.raises(ValueError, match='power of two'):
        E.gcn_propagate(g, 'csr', torch.zeros(C.N_SRC, 12, device='cuda'))
    with pytest.raises(ValueError, match='side'):
        E.gcn_propagate(g, 'rows', X)
    both = torch.zeros(C.N_SRC + 67, 8, device='cuda')
    with pytest.raises(E.nv.NativeError, match='argument check'):                  # out overlaps X
        E.gcn_propagate(g, 'csr', both[:C.N_SRC], out=both[C.N_SRC - 67:C.N_SRC])


# ------------------------------------------------------------------ 6. loss gradient
GRAD_CASE = C.Case(37, 29, 4, 300, 128, 1, 2, seed=77, no_u=5, no_i=4)        # 3 steps, the last of 44 triples; a repeated pair


@pytest.mark.parametrize('d', WIDTHS)
def test_loss_gradient_equals_the_contract_bit_for_bit(d):
    """pred is ure_score's bytes, G_u and G_i are loss_grad_ref's at every width; the last step is partial (44 of 128) and leaves
    rows without an entry; the loss is within 1e-12 relative of the contract and has equal bytes run to run."""
    E, case = _engine(), GRAD_CASE
    g = case.graph()
    (U, V), = mixed_tables(700 + d, d, 1, n_user=case.n_user, n_item=case.n_item)
    U, V = (U * np.float32(0.25)).astype(np.float32), (V * np.float32(0.25)).astype(np.float32)
    Ud, Vd = _dev(U), _dev(V)
    tag = E.gcn_step_tags(g, case.orders[0], case.B)
    from ultrare_amd import ops  # noqa: F401
    for step in range(case.steps):
        batch = case.orders[0][step * case.B:(step + 1) * case.B]
        Gu, Gi, loss, pred = lightgcn.loss_grad_ref(g.host, U, V, case.rating, batch)
        got_u, got_i, got_loss, err, got_pred = E.gcn_loss_grad(g, tag, step, Ud, Vd, want_pred=True)
        assert _same(got_u, Gu) and _same(got_i, Gi), (d, step)
        in_csr = ~np.isnan(pred[g.host.pos])
        assert in_csr.sum() == len(batch)
        score = torch.ops.ultrare.mf_score(Ud, Vd, g.row_u[_dev(in_csr)], g.col[_dev(in_csr)]).cpu().numpy()
        got_pred = got_pred.cpu().numpy()
        assert got_pred[in_csr].tobytes() == score.tobytes() == pred[g.host.pos][in_csr].tobytes()
        assert not got_pred[~in_csr].any() and not err.cpu().numpy()[~in_csr].any()
        got_loss = float(got_loss.cpu()[0])
        assert abs(got_loss - loss) <= 1e-12 * abs(loss), (got_loss, loss)
        again = E.gcn_loss_grad(g, tag, step, Ud, Vd)
        assert _same(again[0], Gu) and _same(again[1], Gi) and float(again[2].cpu()[0]).hex() == got_loss.hex()
    last = case.orders[0][2 * case.B:]
    assert len(last) == 44 and len(np.unique(case.uid[last])) < case.n_user - case.no_u      # a step in which some rows have no entry
    Gu = lightgcn.loss_grad_ref(g.host, U, V, case.rating, last)[0]
    assert (np.abs(Gu).max(axis=1) == 0).sum() > case.no_u
    assert case.uid[0] == case.uid[-1] and case.iid[0] == case.iid[-1]


# ------------------------------------------------------------------ 7. update
SCHEDULES = (sgd_cases.DEFAULT, sgd_cases.NO_DECAY, sgd_cases.NO_MOMENTUM, sgd_cases.PLAIN, sgd_cases.MIXED, sgd_cases.LARGE)


@pytest.mark.parametrize('schedule', SCHEDULES, ids=sgd_cases.sid)
def test_update_equals_the_contract_bit_for_bit(schedule):
    """The first step of a job (m is written, whatever it held) and a later one, with and without the backward's scale."""
    E = _engine()
    lam, mu, lr_decay, lr_step = schedule
    (w, _), (m, _), (g, _) = mixed_tables(800, 32, 3, n_user=129, n_item=1)
    for first, gscale, lr in ((True, 1.0, sgd_cases.LR), (False, 1.0, sgd_cases.LR * lr_decay), (False, float(lightgcn.layer_scale(2)), sgd_cases.LR)):
        gs = (g * np.float32(gscale)).astype(np.float32)
        want_w, want_m = lightgcn.sgd_update_ref(w, m, gs, lr, lam, mu, first)
        wd, md = _dev(w), _dev(m)
        E.gcn_sgd_step(wd, md, _dev(g), lr, lam, mu, first, gscale=gscale)
        assert _same(wd, want_w) and _same(md, want_m), (first, gscale)


@pytest.mark.parametrize('k', (5, 20, 33))
def test_padding_columns_stay_zero_and_training_is_the_float32_contract(k):
    """k = 5, 20, 33 train at the widths 8, 32, 64: the padding columns of the parameters, the momentum and the final tables are
    zero after training, and every table is train_ref(float32)'s bit for bit."""
    case = C.Case(23, 31, k, 260, 100, 2, 2, seed=30 + k)
    job = case.job()
    job.run()
    assert job.d == {5: 8, 20: 32, 33: 64}[k]
    for name in ('W', 'M', 'Star', 'G'):
        assert not job._t[name][:, k:].cpu().numpy().any(), name
    ref = case.train_ref(dtype=np.float32)
    U, V = job.tables(0)
    P, Q = job.base_tables()
    for got, want in ((U, ref['U'][-1]), (V, ref['V'][-1]), (P, ref['P'][-1]), (Q, ref['Q'][-1])):
        assert _same(got.contiguous(), want)
    assert job.epoch_sse(0).tobytes() == ref['sse'].tobytes()
    job.close()


# ------------------------------------------------------------------ 8. whole training against float64
def _run(job):
    job.run()
    U, V = job.tables(0)
    P, Q = job.base_tables()
    sse = job.epoch_sse(0)
    return dict(U=[U.cpu().numpy()], V=[V.cpu().numpy()], P=[P.cpu().numpy()], Q=[Q.cpu().numpy()], loss=np.sqrt(sse / job.graph.N))


@pytest.mark.parametrize('case', C.WHOLE_STEP_CASES, ids=repr)
def test_whole_training_is_as_close_to_float64_as_the_float32_executions(case):
    """E_k = distance of the job from train_ref(float64): the maximum absolute difference over both final tables and both parameter
    tables plus the maximum relative difference over the epoch losses, nothing left out.  E_y = the larger such distance of two
    float32 CPU executions, train_ref(float32) and torch float32 autograd on the dense adjacency.  E_k <= 4 max(E_y, ulp32(max |w|))."""
    ref = C.reference(case)
    job = case.job()
    E_k = C.distance(ref['f64'], _run(job))
    job.close()
    print(f'{case!r}: E_k {E_k:.3g} E_y {ref["E_y"]:.3g} ratio {E_k / ref["E_y"]:.3g} bound {ref["bound"]:.3g}')
    assert ref['E_y'] > 0
    assert E_k <= ref['bound'], (E_k, ref['E_y'], ref['bound'])


def test_zero_layers_is_matrix_factorisation():
    """The L = 0 job against sgd_cases.sgd_train_ref in float64, under the same bound."""
    case = C.WHOLE_STEP_CASES[1]
    ref = C.reference(case, 0)
    U64, V64, loss64 = sgd_cases.sgd_train_ref(case.uid, case.iid, case.rating, case.U0, case.V0, case.orders, case.B, case.lr_host, case.lam, case.mu)
    mf = dict(U=U64, V=V64, P=U64, Q=V64, loss=loss64)
    job = case.job(layers=0)
    E_k = C.distance(mf, _run(job))
    job.close()
    print(f'{case!r} L = 0: E_k {E_k:.3g} E_y {ref["E_y"]:.3g} bound {ref["bound"]:.3g}')
    assert ref['E_y'] > 0 and E_k <= ref['bound'], (E_k, ref['bound'])


# ------------------------------------------------------------------ 9. reproducibility
def _job_bytes(job):
    return [t.cpu().numpy().tobytes() for t in (*job.padded_tables(0), *job.base_tables(padded=True), job._t['M'])] + [job.epoch_sse(0).tobytes()]


def test_a_job_gives_equal_bytes_twice_and_on_a_side_stream_beside_another_job():
    case, other = C.WHOLE_STEP_CASES[1], C.WHOLE_STEP_CASES[2]
    graph = case.graph()
    first = case.job(graph)
    first.run()
    want = _job_bytes(first)
    first.close()
    again = case.job(graph)
    again.run()
    assert _job_bytes(again) == want
    again.close()
    side, beside = case.job(graph), other.job()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(case.epochs):                                    # the two jobs' epochs interleaved on two streams
        side.run_epochs(1, stream=s1)
        if beside.done < beside.ticks:
            beside.run_epochs(1, stream=s2)
    torch.cuda.current_stream().wait_stream(s1)
    torch.cuda.current_stream().wait_stream(s2)
    torch.cuda.synchronize()
    assert _job_bytes(side) == want
    side.close()
    beside.close()


# ------------------------------------------------------------------ 10. memory contract of every new entry
def _arena_case(entry, d=16):
    """-> (arena, call(A), want {output: numpy}, keep {output: mask}) of one entry on GRAD_CASE's graph."""
    from ultrare_amd import _native as nv
    L, case = nv.lib(), GRAD_CASE
    g = lightgcn.Graph(case.uid, case.iid, case.n_user, case.n_item)
    (U, V), (add_u, _) = mixed_tables(900 + d, d, 2, n_user=case.n_user, n_item=case.n_item)
    step, B = 1, case.B
    file_tag = np.empty(g.N, np.int32)
    file_tag[case.orders[0]] = np.arange(g.N) // B
    tag = file_tag[g.pos]
    batch = case.orders[0][step * B:(step + 1) * B]
    Gu, Gi, loss, pred = lightgcn.loss_grad_ref(g, U, V, case.rating, batch)
    pred_csr = np.nan_to_num(pred[g.pos], nan=0.0).astype(np.float32)
    in_csr = tag == step
    err = np.where(in_csr, pred_csr - case.rating.astype(np.float32)[g.pos], np.float32(0)).astype(np.float32)
    A = Arena('cuda')
    st = nv.stream_handle()
    keep = {}
    if entry == 'ure_gcn_propagate':
        acc = add_u.copy()
        for n, a in (('off', g.off_u), ('idx', g.col), ('s_src', g.s_i), ('s_dst', g.s_u), ('X', V), ('add', add_u)):
            A.input(n, a)
        A.output('out', U.nbytes)
        call = lambda A: nv.check(L.ure_gcn_propagate(A.addr('off'), A.addr('idx'), g.n_user, g.n_item, A.addr('s_src'), A.addr('s_dst'), A.addr('X'), d,
                                                      A.addr('add'), None, A.addr('out'), st), entry)
        want = dict(out=lightgcn.propagate_ref(g.off_u, g.col, g.s_i, g.s_u, V, add=add_u))
    elif entry == 'ure_gcn_scale':
        A.input('X', U)
        A.output('out', U.nbytes)
        call = lambda A: nv.check(L.ure_gcn_scale(A.addr('X'), U.size, float(lightgcn.layer_scale(2)), A.addr('out'), st), entry)
        want = dict(out=U * lightgcn.layer_scale(2))
    elif entry == 'ure_gcn_gather_tags':
        A.input('file_tag', file_tag)
        A.input('pos', g.pos)
        A.output('tag', tag.nbytes)
        call = lambda A: nv.check(L.ure_gcn_gather_tags(A.addr('file_tag'), A.addr('pos'), g.N, A.addr('tag'), st), entry)
        want = dict(tag=tag)
    elif entry == 'ure_gcn_residual':
        for n, a in (('row', g.row_u), ('col', g.col), ('rating', case.rating.astype(np.float32)[g.pos]), ('tag', tag), ('U', U), ('V', V)):
            A.input(n, a)
        A.output('err', err.nbytes)
        A.output('pred', err.nbytes)
        call = lambda A: nv.check(L.ure_gcn_residual(A.addr('row'), A.addr('col'), A.addr('rating'), A.addr('tag'), g.N, step, A.addr('U'), A.addr('V'),
                                                     g.n_user, g.n_item, d, A.addr('err'), A.addr('pred'), st), entry)
        want = dict(err=err, pred=pred_csr)
    elif entry == 'ure_gcn_grad':
        for n, a in (('off', g.off_i), ('idx', g.row), ('map', g.to_csr), ('tag', tag), ('err', err), ('T', U)):
            A.input(n, a)
        A.output('G', V.nbytes)
        A.output('row_loss', 8 * g.n_item)
        call = lambda A: nv.check(L.ure_gcn_grad(A.addr('off'), A.addr('idx'), A.addr('map'), A.addr('tag'), A.addr('err'), g.n_item, g.n_user, g.N, step,
                                                 A.addr('T'), d, A.addr('G'), A.addr('row_loss'), st), entry)
        want = dict(G=Gi)
    elif entry == 'ure_gcn_step_loss':
        rs = np.random.RandomState(3)
        row_loss = rs.random_sample(700)
        A.input('row_loss', row_loss)
        A.output('loss', 8)
        call = lambda A: nv.check(L.ure_gcn_step_loss(A.addr('row_loss'), 700, 1, A.addr('loss'), st), entry)
        want = dict(loss=np.array([lightgcn.fold_256(row_loss)]))
    else:
        assert entry == 'ure_gcn_sgd_step'
        A.input('w0', U)                                            # (w is in place: the call works on a copy made inside the arena)
        A.input('g', add_u)
        A.output('w', U.nbytes)
        A.output('m', U.nbytes)

        def call(A):
            A.view('w').copy_(A.view('w0'))
            nv.check(L.ure_gcn_sgd_step(A.addr('w'), A.addr('m'), A.addr('g'), U.size, 1.0, 1e-3, 0.1, 0.9, 1, st), entry)
        want_w, want_m = lightgcn.sgd_update_ref(U, np.zeros_like(U), add_u, 1e-3, 0.1, 0.9, True)
        want = dict(w=want_w, m=want_m)
    return A, call, want, keep


@pytest.mark.parametrize('entry', __import__('ultrare_amd._native', fromlist=['GCN_EXPORTS']).GCN_EXPORTS)
def test_every_entry_keeps_the_memory_contract_on_dirty_memory(entry):
    """Every new stateless entry inside guard zones, its outputs prefilled with 0x00, 0xFF and 0x5A (none takes scratch): no guard
    byte and no input byte changes, every output byte is written and none depends on the prefill, and the outputs are the
    contract's."""
    A, call, want, keep = _arena_case(entry)
    reports = run_prefills(A, call, sync=torch.cuda.synchronize)
    assert not verdict(reports, keep=keep)
    for name, w in want.items():
        assert reports[0].outputs[name] == np.ascontiguousarray(w).tobytes(), (entry, name)


# ------------------------------------------------------------------ 11. the surface
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071


class Param:
    """The InsParam fields Scratch / Sisa read, with the LightGCN options."""

    def __init__(self, epochs, k=16, batch=3000, parallel=False, gcn_layers=2):
        self.k, self.lam, self.seed, self.batch = k, 0.1, 42, batch
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, parallel
        self.optimizer, self.gcn_layers = 'sgd', gcn_layers


def _loaders(S, del_user=()):
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, list(del_user), [], S, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], S, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    return idx, trd, ted, loadData(RatingData(np.hstack(te)), 3000, 24, False)


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def test_scratch_train_gives_the_tables_of_a_direct_job():
    from ultrare_amd import engine, rng
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.utils import seed_all
    _, trd, ted, _ = _loaders(1)
    p = Param(2, k=20)
    sc = Scratch(p, 'lightgcn')
    torch.manual_seed(42)
    model = sc.train(trd[0], ted[0], [], 0, '')
    torch.manual_seed(42)                                   # (the CPU generator feeds the inits and the epochs' seeds; seed_all leaves it alone)
    seed_all(p.seed)
    init = rng.mf_init(N_USER, N_ITEM, p.k)                 # the RNG stream of the MF request
    n = len(trd[0].dataset)
    orders = rng.epoch_perms(rng.epoch_seeds(p.epochs, False), n)
    graph = engine.GcnGraph(*trd[0].dataset.triples(), N_USER, N_ITEM)
    job = engine.GcnJob(graph, init, orders, p.k, 2, 3000, p.epochs, p.lr, p.lam, p.momentum, p.lr_decay)
    job.run()
    U, V = job.tables(0)
    P, Q = job.base_tables()
    assert _bytes(model.user_mat.weight) == _bytes(U.contiguous()) and _bytes(model.item_mat.weight) == _bytes(V.contiguous())
    assert _bytes(model.base[0]) == _bytes(P.contiguous()) and _bytes(model.base[1]) == _bytes(Q.contiguous())
    assert _bytes(P.contiguous()) != _bytes(U.contiguous())
    loss = np.sqrt(job.epoch_sse(0) / n)
    job.close()
    assert sc.log['train_loss'] == [float(x) for x in loss]
    for key in ('train_loss', 'test_rmse', 'test_ndcg', 'test_hr'):
        assert len(sc.log[key]) == p.epochs and np.isfinite(sc.log[key]).all(), key
    assert sc.log['train_loss'][1] < sc.log['train_loss'][0]
    with pytest.raises(ValueError, match='given_model'):
        sc.train(trd[0], ted[0], [], 0, '', given_model=model)


def test_sisa_learns_and_unlearns_one_shard():
    import copy
    import warnings
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import MF, baseTest
    idx, trd, ted, tot = _loaders(3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        s = Sisa(Param(2, parallel=True), 'lightgcn', 3, idx)
    assert s.parallel is False and sum('one after the other' in str(w.message) for w in caught) == 1
    torch.manual_seed(42)
    ml = s.learn(trd, ted, tot, 0, '')
    assert len(ml) == 3 and all(np.isfinite(v).all() for k, v in s.log.items() if k != 'time')
    again = baseTest(tot, [MF.from_tables(m.user_mat.weight.detach().clone(), m.item_mat.weight.detach().clone()) for m in ml])
    assert (s.log0['total_rmse'], s.log0['total_ndcg'], s.log0['total_hr']) == tuple(again)
    # deleting users of shard 1 retrains that shard only, on its post-deletion graph
    del_user = [int(u) for u in idx[1][:5]]
    idx2, trd2, ted2, tot2 = _loaders(3, del_user)
    before = [(_bytes(m.item_mat.weight), _bytes(m.base[0]), _bytes(m.base[1])) for m in ml]
    s2 = Sisa(Param(2), 'lightgcn', 3, idx2)
    torch.manual_seed(42)
    ml2 = s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, '')
    assert s2.retrained == [1]
    after = [(_bytes(m.item_mat.weight), _bytes(m.base[0]), _bytes(m.base[1])) for m in ml2]
    assert after[0] == before[0] and after[2] == before[2] and all(a != b for a, b in zip(after[1], before[1]))
    rows = lambda m, g: _bytes(m.user_mat.weight.detach()[torch.as_tensor(np.asarray(g, dtype=np.int64)).cuda()])
    for g in (0, 2):                                        # the merged rows of the unaffected shards' users
        assert rows(ml2[0], idx2[g]) == rows(ml[0], idx2[g])
    assert np.isfinite([s2.log0['total_rmse'], s2.log0['total_ndcg'], s2.log0['total_hr']]).all()
    again = baseTest(tot2, [MF.from_tables(m.user_mat.weight.detach().clone(), m.item_mat.weight.detach().clone()) for m in ml2])
    assert (s2.log0['total_rmse'], s2.log0['total_ndcg'], s2.log0['total_hr']) == tuple(again)


def test_instance_writes_the_lightgcn_artifacts(tmp_path):
    import shutil
    from ultrare_amd.config import InsParam, Instance
    data = tmp_path / 'data'
    (data / 'toy').mkdir(parents=True)
    shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
    shutil.copy(TEST, data / 'toy' / '0_test.csv')
    save = tmp_path / 'result'
    torch.manual_seed(42)
    p = InsParam('toy', 1, 24, [32], 2, 2, 'rand', data_dir=str(data), model='lightgcn', gcn_layers=1)
    models = Instance(p, save_dir=str(save)).runGroup(is_save=True, learn_type='sisa', group_type='uniform', n_group=2, verbose=0)
    assert len(models) == 2 and all(len(m.base) == 2 for m in models)
    base = save / '2' / 'rand' / 'toy_g2'
    for f in ('LightGCN_uniform_sisa_learn/log0.npy', 'LightGCN_uniform_sisa_learn/user_mat2.npy', 'LightGCN_uniform_sisa_learn/base_user_mat1.npy',
              'LightGCN_uniform_sisa_learn/base_item_mat2.npy', 'LightGCN_uniform_sisa_unlearn/log0.npy'):
        assert (base / f).exists(), f
    assert not list(base.glob('MF_*'))
    P = np.load(base / 'LightGCN_uniform_sisa_learn' / 'base_user_mat1.npy')
    assert P.shape == (N_USER, 16) and np.isfinite(P).all()


def test_the_op_equals_the_ctypes_path_and_raises_on_cpu_tensors():
    from ultrare_amd import _native as nv, ops  # noqa: F401
    E = _engine()
    g = _prop_graph(67, 'csr')
    (X, _), = mixed_tables(950, 32, 1, n_user=C.N_SRC, n_item=1)
    (add, _), = mixed_tables(951, 32, 1, n_user=67, n_item=1)
    Xd, addd = _dev(X), _dev(add)
    got = torch.ops.ultrare.gcn_propagate(g.off_u, g.col, g.s_i, g.s_u, Xd, addd)
    assert _bytes(got) == _bytes(E.gcn_propagate(g, 'csr', Xd, add=addd))
    assert _bytes(torch.ops.ultrare.gcn_propagate(g.off_u, g.col, g.s_i, g.s_u, Xd, None)) == _bytes(E.gcn_propagate(g, 'csr', Xd))
    with pytest.raises(nv.NativeError, match='HIP device only'):
        torch.ops.ultrare.gcn_propagate(g.off_u.cpu(), g.col.cpu(), g.s_i.cpu(), g.s_u.cpu(), torch.from_numpy(X), None)
