"""BPR training on the device (csrc/bpr.hip, engine.bpr_negatives / bpr_neg_index / bpr_loss_grad / GcnJob(loss='bpr')) against its
numpy contract (ultrare_amd/bpr.py): the sampler and the negative index as equal integers, the coefficient pass and both walks bit
for bit (w to one ulp), whole training against the float64 restatement with two float32 CPU executions as the yardstick,
reproducibility, the memory contract of every new entry, the MSE job unchanged, and the Scratch / Sisa / Instance surface."""
import os

import numpy as np
import pytest
import torch

import bpr_cases as B
import lightgcn_cases as C
from abi_arena import Arena, run_prefills, verdict
from test_cpu_score_contract import tables as mixed_tables
from ultrare_amd import bpr, lightgcn

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
WIDTHS = lightgcn.WIDTHS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want):
    got = _np(got) if torch.is_tensor(got) else got
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _engine():
    from ultrare_amd import engine
    return engine


# ------------------------------------------------------------------ 1. the sampler and the negative index
def _check_sampler_and_index(uid, iid, n_user, n_item, draws):
    E = _engine()
    g = E.GcnGraph(uid, iid, np.ones(len(uid), np.float32), n_user, n_item)
    off_d, col_d = bpr.distinct_csr(g.host)
    out = []
    for key, epoch in draws:
        want = bpr.sample_ref(g.host, off_d, col_d, key, epoch)
        neg = E.bpr_negatives(g, key, epoch)
        assert _same(neg, want), (key, epoch)
        w_off, w_map, w_usr = bpr.neg_index_ref(want, g.host.row_u, n_item)
        off_n, map_n, usr_n = E.bpr_neg_index(g, neg)
        assert _same(off_n, w_off) and _same(map_n, w_map) and _same(usr_n, w_usr), (key, epoch)
        out.append((g.host, want, w_off))
    return out


@pytest.mark.parametrize('nnz', (1, 255, 256, 257, 10_007))
@pytest.mark.parametrize('n_item', (2, 255, 256, 257, 65_537))
def test_sampler_and_index_equal_the_contract(n_item, nnz):
    """Equal integers: one, two and three digit passes of the 8-bit radix (n_item up to 256, 257, 65,537), one entry, one tile less
    and more than a wave / a workgroup's round, ten tiles; rows of lightgcn_cases.ROW_LENGTHS, repeated pairs, a user without a triple;
    keys 0 and 2^63 + 5, epochs 0 and 49.  With two items, item 1 is every entry's negative and item 0 nobody's."""
    uid, iid, n_user = B.sampler_triples(n_item, nnz)
    assert len(uid) == nnz
    for host, neg, off_n in _check_sampler_and_index(uid, iid, n_user, n_item, ((0, 0), (2 ** 63 + 5, 49))):
        assert not set(zip(host.row_u.tolist(), neg.tolist())) & set(zip(uid.tolist(), iid.tolist()))
        if n_item == 2:
            assert off_n.tolist() == [0, 0, nnz]
        if n_item == 65_537:
            assert (np.diff(off_n) == 0).sum() > 50_000          # items that are nobody's negative
    if nnz > 1000:
        assert len(bpr.distinct_csr(host)[1]) < nnz               # repeated pairs: the distinct-item CSR is not the graph's


def test_sampler_and_index_on_a_long_row():
    """One user with 1,500 entries over 2,000 items (drawn with repeats) beside rows of 0 .. 300: the binary search runs over about
    a thousand distinct items."""
    uid, iid, n_user, n_item = B.long_row_triples()
    (host, neg, off_n), = _check_sampler_and_index(uid, iid, n_user, n_item, ((20240608, 1),))
    assert np.diff(host.off_u).max() == C.LONG_ROW and 900 < np.diff(bpr.distinct_csr(host)[0]).max() < C.LONG_ROW
    assert np.diff(off_n).max() >= 4                               # an item that is several entries' negative


# ------------------------------------------------------------------ 2. the coefficient pass and the walks
GRAD_CASE = B.Case(37, 29, 4, 300, 128, 1, 2, seed=77, no_u=5, no_i=4)        # 3 steps, the last of 44 triples; a repeated pair
_GRAD = {}


def _grad_setup():
    """GRAD_CASE's graph on the device, the negatives of epoch 0 and their index -- the contract's, made once per process."""
    if not _GRAD:
        E, case = _engine(), GRAD_CASE
        g = case.graph()
        off_d, col_d = bpr.distinct_csr(g.host)
        neg = bpr.sample_ref(g.host, off_d, col_d, case.key, 0)
        index = bpr.neg_index_ref(neg, g.host.row_u, case.n_item)
        _GRAD.update(g=g, neg=neg, index=index, neg_d=_dev(neg), index_d=tuple(_dev(a) for a in index), tag=E.gcn_step_tags(g, case.orders[0], case.B))
    return _GRAD


def _ulp_of(w64):
    """One float32 ulp at the float64 value w64 (the spacing of the float32 numbers around it)."""
    return np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize('d', WIDTHS)
def test_coefficients_and_walks_equal_the_contract(d):
    """Every step of GRAD_CASE at every width: x and both scores are coef_ref's bytes, w is within one float32 ulp of its float64
    value, entries outside the batch are +0.0; G_u and G_i are walks_ref's bytes on the device's own w and x.  The last step is
    partial (44 of 128) and leaves rows without an entry (+0.0 in every byte); items are positive and negative in one batch, others
    negative only.  The loss is within 1e-12 relative of the contract's on the same x and has equal bytes run to run."""
    E, case, S = _engine(), GRAD_CASE, _grad_setup()
    g, neg, index = S['g'], S['neg'], S['index']
    (U, V), = mixed_tables(700 + d, d, 1, n_user=case.n_user, n_item=case.n_item)
    U, V = (U * np.float32(0.25)).astype(np.float32), (V * np.float32(0.25)).astype(np.float32)
    Ud, Vd = _dev(U), _dev(V)
    for step in range(case.steps):
        batch = case.orders[0][step * case.B:(step + 1) * case.B]
        in_csr = bpr.in_batch_csr(g.host, batch)
        w_ref, x_ref, sp_ref, sn_ref = bpr.coef_ref(g.host, U, V, neg, in_csr)
        Gu, Gi, loss, w, x, sp, sn = E.bpr_loss_grad(g, S['tag'], step, Ud, Vd, S['neg_d'], S['index_d'])
        assert _same(x, x_ref) and _same(sp, sp_ref) and _same(sn, sn_ref), (d, step)
        w, x = _np(w), _np(x)
        w64 = -1.0 / (1.0 + np.exp(x[in_csr].astype(np.float64)))
        assert (np.abs(w[in_csr].astype(np.float64) - w64) <= _ulp_of(w64)).all() and (w[in_csr] <= 0).all()
        assert w[~in_csr].tobytes() == bytes(4 * int((~in_csr).sum())) == x[~in_csr].tobytes()
        want_u, want_i, row_loss = bpr.walks_ref(g.host, index, U, V, neg, w, x, in_csr)
        assert _same(Gu, want_u) and _same(Gi, want_i), (d, step)
        got_loss, want_loss = float(loss.cpu()[0]), lightgcn.fold_256(row_loss)
        assert abs(got_loss - want_loss) <= 1e-12 * want_loss, (got_loss, want_loss)
        # the walks alone, on GIVEN arrays: the contract's own w
        again = E.bpr_loss_grad(g, S['tag'], step, Ud, Vd, S['neg_d'], S['index_d'], coef=(_dev(w_ref), _dev(x_ref)))
        ref_u, ref_i, _ = bpr.walks_ref(g.host, index, U, V, neg, w_ref, x_ref, in_csr)
        assert _same(again[0], ref_u) and _same(again[1], ref_i) and again[5] is None
        twice = E.bpr_loss_grad(g, S['tag'], step, Ud, Vd, S['neg_d'])                     # (the index made on the device)
        assert _same(twice[0], want_u) and _same(twice[1], want_i) and float(twice[2].cpu()[0]).hex() == got_loss.hex()
        pos_items, neg_items = set(g.host.col[in_csr].tolist()), set(neg[in_csr].tolist())
        assert pos_items & neg_items and neg_items - pos_items
        idle_u = np.setdiff1d(np.arange(case.n_user), g.host.row_u[in_csr])
        idle_i = np.setdiff1d(np.arange(case.n_item), list(pos_items | neg_items))
        assert len(idle_u) >= case.no_u and _np(Gu)[idle_u].tobytes() == bytes(4 * d * len(idle_u))
        assert _np(Gi)[idle_i].tobytes() == bytes(4 * d * len(idle_i))
        only_neg = sorted(neg_items - pos_items)
        assert np.abs(_np(Gi)[only_neg]).max() > 0
    assert len(batch) == 44 and len(idle_u) > case.no_u and len(idle_i) > 0


@pytest.mark.parametrize('d', WIDTHS)
def test_the_coefficient_at_zero_and_at_both_ends(d):
    """Tables whose scores are 0 or +-100 exactly: x = 0 gives w = -0.5 exactly, x = 100 and x = -100 give finite values (no NaN) in
    w, in both gradients and in the loss."""
    E, case, S = _engine(), GRAD_CASE, _grad_setup()
    g, neg = S['g'], S['neg']
    U, V = np.zeros((case.n_user, d), np.float32), np.zeros((case.n_item, d), np.float32)
    U[:, 0], V[:, 0] = 10.0, 10.0 * (np.arange(case.n_item) % 3 - 1)             # s(u, i) = -100, 0 or 100
    in_csr = bpr.in_batch_csr(g.host, case.orders[0][:case.B])
    want_x = (100.0 * ((g.host.col % 3) - (neg % 3))).astype(np.float32)
    assert {-100.0, 0.0, 100.0} <= set(want_x[in_csr].tolist())
    Gu, Gi, loss, w, x, sp, sn = E.bpr_loss_grad(g, S['tag'], 0, _dev(U), _dev(V), S['neg_d'], S['index_d'])
    w, x = _np(w), _np(x)
    assert np.array_equal(x[in_csr], want_x[in_csr])
    assert (w[in_csr][x[in_csr] == 0] == np.float32(-0.5)).all()
    assert np.isfinite(w).all() and (w[in_csr][x[in_csr] <= -100] == -1).all() and (np.abs(w[in_csr][x[in_csr] >= 100]) < 1e-40).all()
    w64 = -1.0 / (1.0 + np.exp(x[in_csr].astype(np.float64)))
    assert (np.abs(w[in_csr].astype(np.float64) - w64) <= _ulp_of(w64)).all()
    assert np.isfinite(_np(Gu)).all() and np.isfinite(_np(Gi)).all() and np.isfinite(float(loss.cpu()[0]))
    want_u, want_i, row_loss = bpr.walks_ref(g.host, S['index'], U, V, neg, w, x, in_csr)
    assert _same(Gu, want_u) and _same(Gi, want_i)
    assert abs(float(loss.cpu()[0]) - lightgcn.fold_256(row_loss)) <= 1e-12 * lightgcn.fold_256(row_loss)


# ------------------------------------------------------------------ 3. whole training against float64
def _run(job):
    job.run()
    U, V = job.tables(0)
    P, Q = job.base_tables()
    return dict(U=[_np(U)], V=[_np(V)], P=[_np(P)], Q=[_np(Q)], loss=job.epoch_loss(0) / job.graph.N)


@pytest.mark.parametrize('case', B.WHOLE_STEP_CASES, ids=repr)
def test_whole_training_is_as_close_to_float64_as_the_float32_executions(case):
    """E_k = distance of the job from bpr.train_ref(float64) (lightgcn_cases.distance: both final tables, both parameter tables, the
    epoch losses).  E_y = the larger such distance of two float32 CPU executions, train_ref(float32) and torch float32 autograd.
    E_k <= 4 max(E_y, ulp32(max |w|)); every plant lies outside that bound; the last epoch's negatives are the contract's."""
    ref = B.reference(case)
    job = case.job()
    E_k = B.distance(ref['f64'], _run(job))
    neg = _np(job._bpr['neg'])
    with pytest.raises(ValueError, match='epoch_loss'):
        job.epoch_sse(0)
    job.close()
    print(f'{case!r}: E_k {E_k:.3g} E_y {ref["E_y"]:.3g} ratio {E_k / ref["E_y"]:.3g} bound {ref["bound"]:.3g}')
    assert ref['E_y'] > 0
    assert E_k <= ref['bound'], (E_k, ref['E_y'], ref['bound'])
    assert _same(neg, ref['f64']['neg'][-1])
    for plant in bpr.PLANTS:
        assert B.plant_distance(case, plant) > ref['bound'], plant


# ------------------------------------------------------------------ 4. reproducibility, and the MSE job unchanged
def _job_bytes(job):
    return [_np(t).tobytes() for t in (*job.padded_tables(0), *job.base_tables(padded=True), job._t['M'])] + [job.epoch_loss(0).tobytes()]


def test_a_job_gives_equal_bytes_twice_and_on_a_side_stream_beside_another_job():
    case, other = B.WHOLE_STEP_CASES[1], B.WHOLE_STEP_CASES[2]
    graph = case.graph()
    first = case.job(graph)
    first.run()
    want = _job_bytes(first)
    first.close()
    again = case.job(graph)
    again.run()
    assert _job_bytes(again) == want
    again.close()
    moved = case.job(graph, key=case.key + 1)
    moved.run()
    assert _job_bytes(moved) != want                                  # (the key matters)
    moved.close()
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


def test_the_mse_job_is_unchanged_by_the_argument():
    """GcnJob(loss='mse') and the default give the bytes of a job made without the argument, and those are train_ref(float32)'s."""
    case = C.WHOLE_STEP_CASES[1]
    graph = case.graph()
    got = []
    for kw in ({}, dict(loss='mse'), dict(loss='mse', key=7)):
        job = case.job(graph, **kw)
        job.run()
        assert job._bpr is None and job.loss == 'mse'
        got.append(_job_bytes(job) + [job.epoch_sse(0).tobytes()])
        job.close()
    assert got[0] == got[1] == got[2]
    ref = case.train_ref(dtype=np.float32)
    assert got[0][0] == ref['U'][-1].tobytes() and got[0][-1] == ref['sse'].tobytes()


# ------------------------------------------------------------------ 5. memory contract of every new entry
def _arena_case(entry, d=16):
    """-> (arena, call(A), want {output: numpy}) of one entry on GRAD_CASE's graph."""
    from ultrare_amd import _native as nv
    L, case = nv.lib(), GRAD_CASE
    g = lightgcn.Graph(case.uid, case.iid, case.n_user, case.n_item)
    off_d, col_d = bpr.distinct_csr(g)
    neg = bpr.sample_ref(g, off_d, col_d, case.key, 3)
    off_n, map_n, usr_n = bpr.neg_index_ref(neg, g.row_u, g.n_item)
    (U, V), = mixed_tables(900 + d, d, 1, n_user=case.n_user, n_item=case.n_item)
    step, Bsz = 1, case.B
    file_tag = np.empty(g.N, np.int32)
    file_tag[case.orders[0]] = np.arange(g.N) // Bsz
    tag = file_tag[g.pos]
    in_csr = tag == step
    w, x, sp, sn = bpr.coef_ref(g, U, V, neg, in_csr)
    Gu, Gi, row_loss = bpr.walks_ref(g, (off_n, map_n, usr_n), U, V, neg, w, x, in_csr)
    A = Arena('cuda')
    st = nv.stream_handle()
    if entry == 'ure_bpr_sample':
        for n, a in (('off_d', off_d), ('col_d', col_d), ('row_u', g.row_u), ('pos', g.pos)):
            A.input(n, a)
        A.output('neg', neg.nbytes)
        call = lambda A: nv.check(L.ure_bpr_sample(A.addr('off_d'), A.addr('col_d'), len(col_d), A.addr('row_u'), A.addr('pos'), g.N, g.n_user, g.n_item,
                                                   case.key, 3, A.addr('neg'), st), entry)
        want = dict(neg=neg)
    elif entry == 'ure_bpr_index':
        A.input('neg', neg)
        A.input('row_u', g.row_u)
        A.output('off_n', off_n.nbytes)
        A.output('map_n', map_n.nbytes)
        A.output('usr_n', usr_n.nbytes)
        A.scratch('ws', L.ure_bpr_index_scratch(g.N, g.n_item))                  # exactly the sizer's size
        call = lambda A: nv.check(L.ure_bpr_index(A.addr('neg'), A.addr('row_u'), g.N, g.n_item, A.addr('off_n'), A.addr('map_n'), A.addr('usr_n'),
                                                  A.addr('ws'), A.size('ws'), st), entry)
        want = dict(off_n=off_n, map_n=map_n, usr_n=usr_n)
    elif entry == 'ure_bpr_coef':
        for n, a in (('row', g.row_u), ('col', g.col), ('neg', neg), ('tag', tag), ('U', U), ('V', V)):
            A.input(n, a)
        for n in ('w', 'x', 'sp', 'sn'):
            A.output(n, x.nbytes)
        call = lambda A: nv.check(L.ure_bpr_coef(A.addr('row'), A.addr('col'), A.addr('neg'), A.addr('tag'), g.N, step, A.addr('U'), A.addr('V'),
                                                 g.n_user, g.n_item, d, A.addr('w'), A.addr('x'), A.addr('sp'), A.addr('sn'), st), entry)
        want = dict(x=x, sp=sp, sn=sn)                                           # (w: to one ulp, below)
    elif entry == 'ure_bpr_grad_user':
        for n, a in (('off', g.off_u), ('col', g.col), ('neg', neg), ('tag', tag), ('w', w), ('x', x), ('V', V)):
            A.input(n, a)
        A.output('G', U.nbytes)
        A.output('row_loss', 8 * g.n_user)
        call = lambda A: nv.check(L.ure_bpr_grad_user(A.addr('off'), A.addr('col'), A.addr('neg'), A.addr('tag'), A.addr('w'), A.addr('x'), g.n_user,
                                                      g.n_item, g.N, step, A.addr('V'), d, A.addr('G'), A.addr('row_loss'), st), entry)
        want = dict(G=Gu)
    else:
        assert entry == 'ure_bpr_grad_item'
        for n, a in (('off_i', g.off_i), ('row', g.row), ('to_csr', g.to_csr), ('off_n', off_n), ('map_n', map_n), ('usr_n', usr_n), ('tag', tag), ('w', w),
                     ('U', U)):
            A.input(n, a)
        A.output('G', V.nbytes)
        call = lambda A: nv.check(L.ure_bpr_grad_item(A.addr('off_i'), A.addr('row'), A.addr('to_csr'), A.addr('off_n'), A.addr('map_n'), A.addr('usr_n'),
                                                      A.addr('tag'), A.addr('w'), g.n_item, g.n_user, g.N, step, A.addr('U'), d, A.addr('G'), st), entry)
        want = dict(G=Gi)
    return A, call, want, w, row_loss


ENTRIES = [n for n in __import__('ultrare_amd._native', fromlist=['BPR_EXPORTS']).BPR_EXPORTS if not n.endswith('_scratch')]


@pytest.mark.parametrize('entry', ENTRIES)
def test_every_entry_keeps_the_memory_contract_on_dirty_memory(entry):
    """Every new stateless entry inside guard zones, its outputs and scratch prefilled with 0x00, 0xFF and 0x5A, the scratch exactly
    the sizer's size: no guard byte and no input byte changes, every output byte is written and none depends on the prefill, and
    the outputs are the contract's."""
    A, call, want, w, row_loss = _arena_case(entry)
    reports = run_prefills(A, call, sync=torch.cuda.synchronize)
    assert not verdict(reports)
    for name, a in want.items():
        assert reports[0].outputs[name] == np.ascontiguousarray(a).tobytes(), (entry, name)
    if entry == 'ure_bpr_coef':
        got = np.frombuffer(reports[0].outputs['w'], np.float32)
        x64 = np.frombuffer(reports[0].outputs['x'], np.float32).astype(np.float64)
        with np.errstate(over='ignore'):
            w64 = np.where(w != 0, -1.0 / (1.0 + np.exp(x64)), 0.0)
        assert (np.abs(got.astype(np.float64) - w64) <= _ulp_of(w64)).all() and not got[w == 0].any()
    if entry == 'ure_bpr_grad_user':
        got = np.frombuffer(reports[0].outputs['row_loss'], np.float64)
        assert np.allclose(got, row_loss, rtol=1e-12, atol=0)


def test_the_sizer_is_an_export_and_every_other_export_has_an_arena_case():
    from ultrare_amd import _native as nv
    assert set(nv.BPR_EXPORTS) - set(ENTRIES) == {'ure_bpr_index_scratch'} and len(ENTRIES) == 5


# ------------------------------------------------------------------ 6. the surface
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071


class Param:
    """The InsParam fields Scratch / Sisa read, with the LightGCN and BPR options."""

    def __init__(self, epochs, k=16, batch=3000, parallel=False, gcn_layers=2, loss='bpr'):
        self.k, self.lam, self.seed, self.batch = k, 0.1, 42, batch
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, parallel
        self.optimizer, self.gcn_layers, self.loss = 'sgd', gcn_layers, loss


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
    model = sc.train(trd[0], ted[0], [], 0, '', id=3)
    torch.manual_seed(42)
    seed_all(p.seed)
    init = rng.mf_init(N_USER, N_ITEM, p.k)
    n = len(trd[0].dataset)
    orders = rng.epoch_perms(rng.epoch_seeds(p.epochs, False), n)
    graph = engine.GcnGraph(*trd[0].dataset.triples(), N_USER, N_ITEM)
    job = engine.GcnJob(graph, init, orders, p.k, 2, 3000, p.epochs, p.lr, p.lam, p.momentum, p.lr_decay, loss='bpr', key=bpr.stream_key(p.seed, 3))
    job.run()
    U, V = job.tables(0)
    P, Q = job.base_tables()
    assert _bytes(model.user_mat.weight) == _bytes(U.contiguous()) and _bytes(model.item_mat.weight) == _bytes(V.contiguous())
    assert _bytes(model.base[0]) == _bytes(P.contiguous()) and _bytes(model.base[1]) == _bytes(Q.contiguous())
    loss = job.epoch_loss(0) / n
    job.close()
    assert sc.log['train_loss'] == [float(x) for x in loss]
    for key in ('train_loss', 'test_rmse', 'test_ndcg', 'test_hr'):
        assert len(sc.log[key]) == p.epochs and np.isfinite(sc.log[key]).all(), key
    torch.manual_seed(42)
    other = Scratch(p, 'lightgcn').train(trd[0], ted[0], [], 0, '', id=4)         # another shard number: another key
    assert _bytes(other.user_mat.weight) != _bytes(model.user_mat.weight)
    torch.manual_seed(42)
    mse = Scratch(Param(2, k=20, loss='mse'), 'lightgcn').train(trd[0], ted[0], [], 0, '', id=3)
    assert _bytes(mse.user_mat.weight) != _bytes(model.user_mat.weight)
    with pytest.raises(ValueError, match='given_model'):
        sc.train(trd[0], ted[0], [], 0, '', given_model=model)


def test_sisa_learns_unlearns_one_shard_ranks_and_recommends():
    import copy
    from ultrare_amd.method.sisa import Sisa
    idx, trd, ted, tot = _loaders(3)
    s = Sisa(Param(2), 'lightgcn', 3, idx)
    torch.manual_seed(42)
    ml = s.learn(trd, ted, tot, 0, '')
    assert len(ml) == 3 and all(np.isfinite(v).all() for k, v in s.log.items() if k != 'time')
    metrics = s.rank_eval(tot)
    assert metrics and all(np.isfinite(v) for v in metrics.values())
    scores, items = s.recommend(np.arange(8), 10)
    assert np.isfinite(np.asarray(scores.cpu() if torch.is_tensor(scores) else scores)).all()
    assert np.asarray(items.cpu() if torch.is_tensor(items) else items).shape == (8, 10)
    # deleting users of shard 1 retrains that shard only, under its own key, on its post-deletion graph
    del_user = [int(u) for u in idx[1][:5]]
    idx2, trd2, ted2, tot2 = _loaders(3, del_user)
    before = [(_bytes(m.item_mat.weight), _bytes(m.base[0]), _bytes(m.base[1])) for m in ml]
    s2 = Sisa(Param(2), 'lightgcn', 3, idx2)
    torch.manual_seed(42)
    ml2 = s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, '')
    assert s2.retrained == [1]
    after = [(_bytes(m.item_mat.weight), _bytes(m.base[0]), _bytes(m.base[1])) for m in ml2]
    assert after[0] == before[0] and after[2] == before[2] and all(a != b for a, b in zip(after[1], before[1]))
    assert all(np.isfinite(v) for v in s2.rank_eval(tot2).values())


def test_instance_writes_the_bpr_artifacts(tmp_path):
    import shutil
    from ultrare_amd.config import InsParam, Instance
    data = tmp_path / 'data'
    (data / 'toy').mkdir(parents=True)
    shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
    shutil.copy(TEST, data / 'toy' / '0_test.csv')
    save = tmp_path / 'result'
    torch.manual_seed(42)
    p = InsParam('toy', 1, 24, [32], 2, 2, 'rand', data_dir=str(data), model='lightgcn', gcn_layers=0, loss='bpr')
    models = Instance(p, save_dir=str(save)).runGroup(is_save=True, learn_type='sisa', group_type='uniform', n_group=2, verbose=0)
    assert len(models) == 2 and all(len(m.base) == 2 for m in models)
    base = save / '2' / 'rand' / 'toy_g2'
    for f in ('LightGCN_bpr_uniform_sisa_learn/log0.npy', 'LightGCN_bpr_uniform_sisa_learn/user_mat2.npy', 'LightGCN_bpr_uniform_sisa_learn/base_user_mat1.npy',
              'LightGCN_bpr_uniform_sisa_learn/base_item_mat2.npy', 'LightGCN_bpr_uniform_sisa_unlearn/log0.npy'):
        assert (base / f).exists(), f
    assert not list(base.glob('MF_*')) and not list(base.glob('LightGCN_uniform*'))
    P = np.load(base / 'LightGCN_bpr_uniform_sisa_learn' / 'base_user_mat1.npy')
    assert P.shape == (N_USER, 16) and np.isfinite(P).all()
    Q, V = (np.load(base / 'LightGCN_bpr_uniform_sisa_learn' / f) for f in ('base_item_mat1.npy', 'item_mat1.npy'))
    assert np.array_equal(Q, V)                                                      # L = 0 is BPR-MF: the item table is the parameters


def test_the_op_equals_the_ctypes_path_and_raises_on_cpu_tensors():
    from ultrare_amd import _native as nv, ops  # noqa: F401
    E, S = _engine(), _grad_setup()
    g = S['g']
    E.bpr_prepare(g)
    for key, epoch in ((5, 0), (2 ** 63 + 5, 49)):
        got = torch.ops.ultrare.bpr_negatives(g.off_d, g.col_d, g.row_u, g.pos, g.n_item, key - 2 ** 64 if key >= 2 ** 63 else key, epoch)
        assert _bytes(got) == _bytes(E.bpr_negatives(g, key, epoch))
    with pytest.raises(nv.NativeError, match='HIP device only'):
        torch.ops.ultrare.bpr_negatives(g.off_d.cpu(), g.col_d.cpu(), g.row_u.cpu(), g.pos.cpu(), g.n_item, 5, 0)
    with pytest.raises(ValueError, match='do not fit'):
        torch.ops.ultrare.bpr_negatives(g.off_d, g.col_d, g.row_u, g.pos[:-1], g.n_item, 5, 0)
    with pytest.raises(nv.NativeError, match='HIP device'):
        E.bpr_neg_index(g, S['neg_d'].cpu())
    with pytest.raises(ValueError, match='neg must be'):
        E.bpr_neg_index(g, S['neg_d'][:-1])
    with pytest.raises(ValueError, match='no negative to draw'):
        E.bpr_negatives(E.GcnGraph([0, 0, 1], [0, 1, 1], np.ones(3, np.float32), 2, 2), 0, 0)
