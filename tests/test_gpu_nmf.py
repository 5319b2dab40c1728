"""The NeuMF backbone on the device (csrc/nmf.hip through the raw ABI, engine.NmfJob, Scratch / Sisa): every kernel against its
numpy contract (ultrare_amd/nmf.py in float32) bit for bit, whole training against train_ref bit for bit and against float64
within the bound of nmf_cases.reference, and every new entry on dirty memory inside guard zones (tests/abi_arena.py; DESIGN
4.20).  tests/test_cpu_nmf.py holds the contract itself to torch autograd."""
import os

import numpy as np
import pytest
import torch

import nmf_cases as C
import poison
from abi_arena import PREFILLS, Arena, run_prefills, verdict
from lightgcn_cases import ROW_COUNTS, prop_rows
from ultrare_amd import lightgcn, nmf

pytestmark = pytest.mark.gpu

SLOT_COUNTS = (1, 63, 64, 65, 300)
SCORE_PARTIALS = 2048


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import _native
    _native.lib()
    torch.cuda.set_device(0)
    return _native


def lay_of(layers):
    return np.ascontiguousarray(layers, dtype=np.int32)


def f32(raw, shape):
    return np.frombuffer(raw, dtype=np.float32).reshape(shape)


def clean(report):
    return not report.guards and not report.inputs


# ------------------------------------------------------------------ 5a. forward / backward, and scoring against it
STAGE_CASE = {}


def stage_case(k, layers):
    """One graph per shape (37 x 29, 420 ratings, 5 users and 4 items without one, a repeated pair), its model and one epoch's ranks."""
    key = (k, tuple(layers))
    if key not in STAGE_CASE:
        case = C.Case(37, 29, k, layers, 420, 300, 1, seed=40 + k + len(layers), no_u=5, no_i=4)
        g = lightgcn.Graph(case.uid, case.iid, case.n_user, case.n_item)
        U, V, dense = C.stage_model(k, layers, case.n_user, case.n_item, seed=k)
        STAGE_CASE[key] = (case, g, U, V, dense, nmf.epoch_rank(g, case.orders[0]), case.rating[g.pos])
    return STAGE_CASE[key]


@pytest.mark.parametrize('k,layers', C.STAGE_SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_forward_backward_equals_the_contract(nv, k, layers):
    """err, pred, act, dlt and emb of every slot, bit for bit, for batches of 1, 63, 64, 65 and 300 slots at different places of
    the epoch (a prefill each); two units of the first layer sit at a pre-activation of exactly zero (their delta is +0.0); the
    repeated pair, and users and items without a rating, are in the graph.  ure_nmf_score on the batch's pairs gives pred's bytes."""
    case, g, U, V, dense, rank, r_csr = stage_case(k, layers)
    S, lay, st = nmf.Shape(k, layers), lay_of(layers), nv.stream_handle()
    assert (case.uid[0], case.iid[0]) == (case.uid[-1], case.iid[-1])
    for n, (n_slots, prefill) in enumerate(zip(SLOT_COUNTS, PREFILLS + PREFILLS)):
        lo = (0, 17, 120, 355, 100)[n]
        A = Arena('cuda')
        for name, a in (('row', g.row_u), ('col', g.col), ('rating', r_csr), ('rank', rank), ('U', U), ('V', V), ('dense', dense)):
            A.input(name, a)
        for name, width in (('err', 1), ('pred', 1), ('act', S.A), ('dlt', S.Dw), ('emb', 2 * S.wd)):
            A.output(name, n_slots * width * 4)
        A.load(prefill)
        nv.check(nv.lib().ure_nmf_forward_backward(A.addr('row'), A.addr('col'), A.addr('rating'), A.addr('rank'), g.N, lo, n_slots, A.addr('U'),
                                                   A.addr('V'), case.n_user, case.n_item, A.addr('dense'), k, nv.ptr(lay), len(lay), A.addr('err'),
                                                   A.addr('pred'), A.addr('act'), A.addr('dlt'), A.addr('emb'), st), 'ure_nmf_forward_backward')
        torch.cuda.synchronize()
        rep = A.collect()
        assert clean(rep), (rep.guards, rep.inputs)
        q = nmf.batch_entries(rank, lo, n_slots)
        uid, iid = g.row_u[q].astype(np.int64), g.col[q].astype(np.int64)
        pred, act = nmf.forward_ref(U, V, dense, k, layers, uid, iid)
        err = pred - r_csr[q]
        dlt, emb = nmf.backward_ref(U, V, dense, k, layers, uid, iid, act, err)
        for name, want in (('pred', pred), ('err', err), ('act', act), ('dlt', dlt), ('emb', emb)):
            assert rep.outputs[name] == np.ascontiguousarray(want).tobytes(), (name, n_slots)
        a1 = act[:, S.a_at[1]:S.a_at[1] + 2]
        assert a1.tobytes() == bytes(a1.nbytes) and dlt[:, :2].tobytes() == bytes(8 * n_slots)      # the planted units: +0.0, and no gradient
        assert n_slots == 1 or ((act[:, S.a_at[1] + 2:] > 0).any() and (act[:, S.a_at[1] + 2:] == 0).any())      # relu on both sides
        from ultrare_amd import engine
        dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dtype=t)
        got = engine.nmf_score(dev(U, torch.float32), dev(V, torch.float32), dev(dense, torch.float32), k, layers, dev(uid, torch.int32), dev(iid, torch.int32))
        assert got.cpu().numpy().tobytes() == rep.outputs['pred']


# ------------------------------------------------------------------ 5b. the weight gradient
@pytest.mark.parametrize('k,layers', [(16, [64, 32, 16, 8]), (4, [8, 4]), (16, [32, 128, 4])], ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('n_slots', (1, 255, 256, 257, 515))
def test_weight_gradient_equals_the_contract_on_any_grid(nv, k, layers, n_slots):
    """g_dense against weight_grad_ref, bit for bit, at the chunk's edges (255, 256, 257: one slot past it; 515: three chunks),
    launched with a workgroup per chunk, with ONE workgroup for all chunks and with two (257: 2 against 1; 515: 3, 1 and 2 -- the loop over
    chunks is walked more than once): equal bytes; at exactly the sizer's scratch."""
    S, lay, st = nmf.Shape(k, layers), lay_of(layers), nv.stream_handle()
    rs = np.random.RandomState(n_slots + k)
    err = rs.standard_normal(n_slots).astype(np.float32)
    act = rs.standard_normal((n_slots, S.A)).astype(np.float32)
    dlt = (rs.standard_normal((n_slots, S.Dw)) * (rs.rand(n_slots, S.Dw) < 0.6)).astype(np.float32)          # zeros, as relu leaves them
    want = nmf.weight_grad_ref(err, act, dlt, k, layers)
    assert want.shape == (S.n_dense,) and want[S.n_real:].tobytes() == bytes(4 * (S.n_dense - S.n_real))
    L = nv.lib()
    ws = L.ure_nmf_weight_grad_scratch(n_slots, k, nv.ptr(lay), len(lay))
    assert ws == -(-n_slots // nmf.CHUNK) * S.n_dense * 4
    got = []
    for blocks in (0, 1, 2):
        A = Arena('cuda')
        A.input('err', err), A.input('act', act), A.input('dlt', dlt)
        A.output('g', S.n_dense * 4)
        A.scratch('ws', ws)
        call = lambda A: nv.check(L.ure_nmf_weight_grad(A.addr('err'), A.addr('act'), A.addr('dlt'), n_slots, k, nv.ptr(lay), len(lay), A.addr('g'),
                                                        A.addr('ws'), A.size('ws'), blocks, st), 'ure_nmf_weight_grad')
        reports = run_prefills(A, call, sync=torch.cuda.synchronize)
        assert not verdict(reports)
        got.append(reports[0].outputs['g'])
    assert got[0] == got[1] == got[2] == want.tobytes()


# ------------------------------------------------------------------ 5c. the masked row sums
@pytest.mark.parametrize('n_rows', ROW_COUNTS)
@pytest.mark.parametrize('width', (8, 48, 192))
def test_row_sums_equal_the_contract(nv, n_rows, width):
    """Rows of 0 .. 300 entries and one of 1,500 (a single row: 300), widths that are and are not a power of two, a column
    window inside wider slot rows, on the CSR side (with the float64 loss chain) and through a map on the CSC side: bit for
    bit; a row without an entry in the batch is +0.0 in every byte."""
    row, _, lengths = prop_rows(n_rows)
    nnz = len(row)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rs = np.random.RandomState(n_rows + width)
    rank = rs.permutation(nnz).astype(np.int32)
    to_csr = rs.permutation(nnz).astype(np.int32)
    n_slots, lo = max(nnz // 3, 1), nnz // 4
    col0, ld = 12, width + 20
    E = rs.standard_normal((n_slots, ld)).astype(np.float32)
    err = rs.standard_normal(n_slots).astype(np.float32)
    L, st = nv.lib(), nv.stream_handle()
    for mapped in (False, True):
        m = to_csr if mapped else None
        G, row_loss = nmf.row_sum_ref(off, m, rank, lo, n_slots, E, col0, width, err=None if mapped else err)
        A = Arena('cuda')
        A.input('off', off), A.input('rank', rank), A.input('E', E), A.input('err', err), A.input('map', to_csr)
        A.output('G', n_rows * width * 4)
        if not mapped:
            A.output('row_loss', n_rows * 8)
        call = lambda A: nv.check(L.ure_nmf_row_sum(A.addr('off'), A.addr('map' if mapped else None), A.addr('rank'), n_rows, nnz, lo, n_slots, A.addr('E'),
                                                    ld, col0, width, A.addr(None if mapped else 'err'), A.addr('G'), A.addr(None if mapped else 'row_loss'),
                                                    st), 'ure_nmf_row_sum')
        reports = run_prefills(A, call, sync=torch.cuda.synchronize)
        assert not verdict(reports)
        assert reports[0].outputs['G'] == G.tobytes(), mapped
        if not mapped:
            assert reports[0].outputs['row_loss'] == row_loss.tobytes()
        q = np.arange(nnz) if m is None else m
        s = rank[q].astype(np.int64) - lo
        hit = np.zeros(n_rows, dtype=bool)
        hit[row[(s >= 0) & (s < n_slots)]] = True
        got = f32(reports[0].outputs['G'], (n_rows, width))
        assert got[~hit].tobytes() == bytes(int((~hit).sum()) * width * 4) and hit.any()
        assert n_rows < 3 or (~hit).sum() >= 2


# ------------------------------------------------------------------ 5d. scoring
@pytest.mark.parametrize('n', (1, 255, 257, 1000))
@pytest.mark.parametrize('n_models', (1, 3))
def test_scoring_equals_the_contract(nv, n, n_models):
    """pred of an ensemble of 1 and 3 models scored one call per model: the additions and the division of ure_score's protocol
    restated in numpy (nmf.score_ref), bit for bit; the squared-error partials are one per workgroup, zeros behind them, and sum
    to the squared error; nothing outside pred and sse is written."""
    k, layers = 16, [64, 32, 16, 8]
    S, lay, st, L = nmf.Shape(k, layers), lay_of(layers), nv.stream_handle(), nv.lib()
    n_user, n_item = 23, 31
    rs = np.random.RandomState(n + n_models)
    models = [C.stage_model(k, layers, n_user, n_item, seed=7 * s + n) for s in range(n_models)]
    uid, iid = rs.randint(0, n_user, n).astype(np.int32), rs.randint(0, n_item, n).astype(np.int32)
    uid[0], iid[0], uid[-1], iid[-1] = 0, 0, n_user - 1, n_item - 1
    rating = (rs.randint(1, 6, n) / 5).astype(np.float32)
    want = nmf.score_ref(models, k, layers, uid, iid)
    A = Arena('cuda')
    A.input('uid', uid), A.input('iid', iid), A.input('rating', rating)
    for s, (U, V, dense) in enumerate(models):
        A.input(f'U{s}', U), A.input(f'V{s}', V), A.input(f'dense{s}', dense)
    A.output('pred', n * 4)
    A.output('sse', SCORE_PARTIALS * 8)

    def call(A):
        for s in range(n_models):
            nv.check(L.ure_nmf_score(A.addr(f'U{s}'), A.addr(f'V{s}'), A.addr(f'dense{s}'), k, nv.ptr(lay), len(lay), n_user, n_item, n_models,
                                     int(s == 0), int(s == n_models - 1), A.addr('uid'), A.addr('iid'), A.addr('rating'), n, A.addr('pred'),
                                     A.addr('sse'), st), 'ure_nmf_score')
    reports = run_prefills(A, call, sync=torch.cuda.synchronize)
    assert not verdict(reports)
    assert reports[0].outputs['pred'] == want.tobytes()
    assert reports[0].outputs['sse'] == nmf.sse_ref(want, rating).tobytes()
    sse = np.frombuffer(reports[0].outputs['sse'], dtype=np.float64)
    exact = float(((want.astype(np.float64) - rating) ** 2).sum())
    assert not sse[min(-(-n // 4), SCORE_PARTIALS):].any() and abs(sse.sum() - exact) <= 1e-5 * exact      # (the chain IS the squared error)


def test_grid_stride_loops_take_more_than_one_trip(nv):
    """Both kernels that cap their grid, past the cap: ure_nmf_forward_backward over 600,000 entries (2,048 workgroups of 256: the
    list of a workgroup is rebuilt on its second trip) with a batch of 300 slots spread over both trips, and ure_nmf_score over
    10,000 pairs (2,048 workgroups of four waves); every slot and every pair, pred and sse, bit for bit; the smallest stack."""
    k, layers, n_user, n_item, N = 4, [8, 4], 1500, 1100, 600000
    S, lay, st, L = nmf.Shape(k, layers), lay_of(layers), nv.stream_handle(), nv.lib()
    rs = np.random.RandomState(12)
    uid, iid = rs.randint(0, n_user, N).astype(np.int32), rs.randint(0, n_item, N).astype(np.int32)
    rating = (rs.randint(1, 6, N) / 5).astype(np.float32)
    g = lightgcn.Graph(uid, iid, n_user, n_item)
    U, V, dense = C.stage_model(k, layers, n_user, n_item, seed=12)
    rank, r_csr = nmf.epoch_rank(g, rs.permutation(N)), rating[g.pos]
    lo, n_slots = 123456, 300
    q = nmf.batch_entries(rank, lo, n_slots)
    assert N > 2048 * 256 and (q < 2048 * 256).sum() > 50 and (q >= 2048 * 256).sum() > 20          # slots of both trips
    A = Arena('cuda')
    for name, a in (('row', g.row_u), ('col', g.col), ('rating', r_csr), ('rank', rank), ('U', U), ('V', V), ('dense', dense)):
        A.input(name, a)
    for name, width in (('err', 1), ('pred', 1), ('act', S.A), ('dlt', S.Dw), ('emb', 2 * S.wd)):
        A.output(name, n_slots * width * 4)
    A.load(0x5A)
    nv.check(L.ure_nmf_forward_backward(A.addr('row'), A.addr('col'), A.addr('rating'), A.addr('rank'), N, lo, n_slots, A.addr('U'), A.addr('V'), n_user,
                                        n_item, A.addr('dense'), k, nv.ptr(lay), len(lay), A.addr('err'), A.addr('pred'), A.addr('act'), A.addr('dlt'),
                                        A.addr('emb'), st), 'ure_nmf_forward_backward')
    torch.cuda.synchronize()
    rep = A.collect()
    assert clean(rep), (rep.guards, rep.inputs)
    u, i = g.row_u[q].astype(np.int64), g.col[q].astype(np.int64)
    pred, act = nmf.forward_ref(U, V, dense, k, layers, u, i)
    err = pred - r_csr[q]
    dlt, emb = nmf.backward_ref(U, V, dense, k, layers, u, i, act, err)
    for name, want in (('pred', pred), ('err', err), ('act', act), ('dlt', dlt), ('emb', emb)):
        assert rep.outputs[name] == np.ascontiguousarray(want).tobytes(), name
    # scoring: the first 10,000 triples as pairs
    n = 10000
    assert n > SCORE_PARTIALS * 4
    want = nmf.score_ref([(U, V, dense)], k, layers, uid[:n].astype(np.int64), iid[:n].astype(np.int64))
    B = Arena('cuda')
    B.input('uid', uid[:n]), B.input('iid', iid[:n]), B.input('rating', rating[:n]), B.input('U', U), B.input('V', V), B.input('dense', dense)
    B.output('pred', n * 4)
    B.output('sse', SCORE_PARTIALS * 8)
    B.load(0xFF)
    nv.check(L.ure_nmf_score(B.addr('U'), B.addr('V'), B.addr('dense'), k, nv.ptr(lay), len(lay), n_user, n_item, 1, 1, 1, B.addr('uid'), B.addr('iid'),
                             B.addr('rating'), n, B.addr('pred'), B.addr('sse'), st), 'ure_nmf_score')
    torch.cuda.synchronize()
    rep = B.collect()
    assert clean(rep), (rep.guards, rep.inputs)
    assert rep.outputs['pred'] == want.tobytes() and rep.outputs['sse'] == nmf.sse_ref(want, rating[:n]).tobytes()


# ------------------------------------------------------------------ 6. whole training
def job_bytes(job):
    torch.cuda.synchronize()
    return b''.join(t.cpu().numpy().tobytes() for t in job.params()) + job.epoch_sse().tobytes()


@pytest.mark.parametrize('case', C.WHOLE_CASES, ids=repr)
def test_whole_training_equals_the_contract(nv, case):
    """NmfJob against train_ref(float32): every parameter and every epoch's loss sum bit for bit; and within
    bound = 4 max(E_y, ulp32(largest |w|)) of train_ref(float64) (nmf_cases.reference)."""
    ref = C.reference(case)
    job = case.job()
    job.run()
    U, V, dense = (t.cpu().numpy() for t in job.params())
    sse = job.epoch_sse()
    job.close()
    f32_ref = ref['f32']
    for name, got in (('U', U), ('V', V), ('dense', dense)):
        assert got.tobytes() == f32_ref[name][-1].tobytes(), name
    assert sse.tobytes() == f32_ref['sse'].tobytes()
    run = dict(U=[U], V=[V], dense=[dense], loss=np.sqrt(sse / case.N))
    dist = C.distance(ref['f64'], run)
    print(f'{case!r}: distance {dist:.3g}, E_y {ref["E_y"]:.3g}, bound {ref["bound"]:.3g}')
    assert np.isfinite(U).all() and np.isfinite(dense).all() and 3e-8 <= ref['E_y'] <= 3e-6
    assert dist <= ref['bound']
    assert case.N % case.B and len(set(case.lr_host.tolist())) == case.epochs


def test_two_streams_give_equal_bytes(nv):
    case = C.WHOLE_CASES[2]
    one = case.job()
    one.run()
    want = job_bytes(one)
    one.close()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    side, beside = case.job(), C.WHOLE_CASES[0].job()
    for _ in range(case.epochs):
        side.run_epochs(1, stream=s1)
        beside.run_epochs(1, stream=s2)
    torch.cuda.current_stream().wait_stream(s1)
    torch.cuda.current_stream().wait_stream(s2)
    assert job_bytes(side) == want
    side.close()
    beside.close()


# ------------------------------------------------------------------ 7. memory
def test_job_on_poisoned_memory(nv, monkeypatch):
    """A whole NmfJob with every torch.empty buffer filled with 0x00, 0xFF and 0x5A: equal bytes (the job writes before it reads)."""
    case, got = C.WHOLE_CASES[1], []
    graph = case.graph()
    for fill in poison.FILLS:
        with poison.active(monkeypatch, fill):
            job = case.job(graph)
            job.run()
            got.append(job_bytes(job))
            job.close()
    assert got[0] == got[1] == got[2] == b''.join(C.reference(case)['f32'][name][-1].tobytes() for name in ('U', 'V', 'dense')) + C.reference(case)['f32']['sse'].tobytes()


def test_sisa_request_on_poisoned_memory(nv, monkeypatch):
    """A 3-shard Sisa('nmf') learn + unlearn under the three fills: equal models and equal logs."""
    got = []
    for fill in poison.FILLS:
        with poison.active(monkeypatch, fill):
            ml, ml2, s, s2 = sisa_request()
            torch.cuda.synchronize()
            got.append(b''.join(model_bytes(m) for m in ml + ml2) + repr((s.log0, s2.log0, s.log['train_loss'], s2.log['test_rmse'])).encode())
    assert got[0] == got[1] == got[2]


# ------------------------------------------------------------------ 8. the surface
G = os.path.join(os.path.dirname(__file__), 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071
SYN_USER, SYN_ITEM = 90, 60


class Param:
    """The InsParam fields Scratch / Sisa read, with the NeuMF options."""

    def __init__(self, epochs, k, layers, n_user=N_USER, n_item=N_ITEM, batch=3000, parallel=False):
        self.k, self.layers, self.lam, self.seed, self.batch = k, layers, 0.1, 42, batch
        # (lr: at the default 0.001 and batches of 3,000 the summed loss diverges in the first epoch, in torch as here -- README)
        self.lr, self.lr_decay, self.momentum, self.epochs = 1e-4, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = n_user, n_item, parallel
        self.optimizer, self.loss, self.model = 'sgd', 'mse', 'nmf'


def model_bytes(m):
    return b''.join(t.detach().cpu().numpy().tobytes() for t in m.tables())


def shard_bytes(m):
    """What stays per shard: the item tables, the MLP and the head."""
    U, V, dense = m.tables()
    return V.cpu().numpy().tobytes() + dense.cpu().numpy().tobytes()


def synthetic_loaders(del_user=()):
    """Three shards of 30 users each over 60 items: 500 training and 120 test ratings per shard, batch 200 (a partial last step)."""
    from ultrare_amd.read import RatingData, loadData
    rs = np.random.RandomState(77)
    idx = [list(range(30 * g, 30 * (g + 1))) for g in range(3)]
    tr, te = [], []
    for g in range(3):
        for n, out in ((500, tr), (120, te)):
            a = np.stack([rs.randint(30 * g, 30 * (g + 1), n), rs.randint(0, SYN_ITEM, n), rs.randint(1, 6, n) / 5.0])
            out.append(a)
    tr = [a[:, ~np.isin(a[0], list(del_user))] for a in tr]
    trd = [loadData(RatingData(a), 200, 24) for a in tr]
    ted = [loadData(RatingData(a), 200, 24, False) for a in te]
    return idx, trd, ted, loadData(RatingData(np.hstack(te)), 200, 24, False)


def sisa_request():
    """learn on the three synthetic shards, then unlearn five users of shard 1 -> (models, models after, the two Sisa objects)."""
    import copy
    from ultrare_amd.method.sisa import Sisa
    idx, trd, ted, tot = synthetic_loaders()
    s = Sisa(Param(2, 8, [16, 8], SYN_USER, SYN_ITEM, batch=200), 'nmf', 3, idx)
    torch.manual_seed(42)
    ml = list(s.learn(trd, ted, tot, 0, ''))
    kept = [copy.deepcopy(m) for m in ml]
    del_user = idx[1][:5]
    _, trd2, ted2, tot2 = synthetic_loaders(del_user)
    s2 = Sisa(Param(2, 8, [16, 8], SYN_USER, SYN_ITEM, batch=200), 'nmf', 3, idx)
    torch.manual_seed(42)
    ml2 = list(s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, ''))
    return kept, ml2, s, s2


def toy_loaders():
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, [], [], 1, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], 1, idx)
    return loadData(RatingData(tr[0]), 3000, 24), loadData(RatingData(te[0]), 3000, 24, False)


def test_scratch_on_the_toy_set_logs_what_basetest_recomputes(nv, tmp_path):
    """Scratch('nmf') on the toy golden data: the artifacts carry the reference's attribute names; every epoch's log entry equals
    baseTest of that epoch's model rebuilt by a direct NmfJob on the same RNG stream, and the last one equals baseTest of the model
    loaded back from the saved artifacts."""
    from ultrare_amd import engine, rng
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.utils import NMF, baseTest, seed_all
    trd, ted = toy_loaders()
    p = Param(2, 16, [32, 16])
    sc = Scratch(p, 'nmf')
    torch.manual_seed(42)
    model = sc.train(trd, ted, [], 0, str(tmp_path))
    names = ('user_mat_mf', 'user_mat_mlp', 'item_mat_mf', 'item_mat_mlp')
    assert sorted(os.listdir(tmp_path)) == sorted(['model0.pth', 'log0.npy'] + [n + '0.npy' for n in names])
    for key in ('train_loss', 'test_rmse', 'test_ndcg', 'test_hr'):
        assert len(sc.log[key]) == p.epochs and np.isfinite(sc.log[key]).all(), key
    assert sc.log['train_loss'][1] < sc.log['train_loss'][0]
    # from the artifacts
    back = NMF(N_USER, N_ITEM, p.k, p.layers)
    back.load_state_dict(torch.load(os.path.join(tmp_path, 'model0.pth')))
    back = back.to('cuda')
    for n in names:
        assert np.load(os.path.join(tmp_path, n + '0.npy')).tobytes() == getattr(back, n).weight.detach().cpu().numpy().tobytes() == \
            getattr(model, n).weight.detach().cpu().numpy().tobytes()
    assert (sc.log['test_rmse'][-1], sc.log['test_ndcg'][-1], sc.log['test_hr'][-1]) == tuple(baseTest(ted, [back]))
    saved = np.load(os.path.join(tmp_path, 'log0.npy'), allow_pickle=True).item()
    assert saved['test_rmse'] == sc.log['test_rmse']
    # epoch by epoch, from a direct job on the same stream
    torch.manual_seed(42)
    seed_all(p.seed)
    init = tuple(t.numpy() for t in NMF(N_USER, N_ITEM, p.k, p.layers).tables())
    n = len(trd.dataset)
    orders = rng.epoch_perms(rng.epoch_seeds(p.epochs, False), n)
    job = engine.NmfJob(engine.GcnGraph(*trd.dataset.triples(), N_USER, N_ITEM), init, orders, p.k, p.layers, 3000, p.epochs, p.lr, p.lam, p.momentum,
                        p.lr_decay)
    for t in range(p.epochs):
        job.run_epochs(1)
        m = NMF.from_tables(*(x.clone() for x in job.params()), p.k, p.layers)
        assert (sc.log['test_rmse'][t], sc.log['test_ndcg'][t], sc.log['test_hr'][t]) == tuple(baseTest(ted, [m])), t
    assert sc.log['train_loss'] == [float(x) for x in np.sqrt(job.epoch_sse(0) / n)]
    assert model_bytes(m) == model_bytes(model)
    job.close()
    with pytest.raises(ValueError, match='given_model'):
        sc.train(trd, ted, [], 0, '', given_model=model)


def test_sisa_learns_merges_both_user_tables_and_unlearns_one_shard(nv):
    from ultrare_amd.method.utils import baseTest
    ml, ml2, s, s2 = sisa_request()
    idx = s.group_index
    assert len(ml) == len(ml2) == 3 and all(np.isfinite(v).all() for k, v in s.log.items() if k != 'time')
    # learn: every model shares the merged user tables; a shard's own users' rows come from that shard's training
    for name in ('user_mat_mf', 'user_mat_mlp'):
        tabs = [getattr(m, name).weight.detach().cpu().numpy() for m in ml]
        assert all(np.array_equal(tabs[0], t) for t in tabs[1:]) and np.isfinite(tabs[0]).all()
    solo = sisa_shard_alone(1)
    for name in ('user_mat_mf', 'user_mat_mlp'):
        merged, own = getattr(ml[1], name).weight.detach().cpu().numpy(), getattr(solo, name).weight.detach().cpu().numpy()
        assert np.array_equal(merged[idx[1]], own[idx[1]]) and not np.array_equal(merged[idx[0]], own[idx[0]])
    assert shard_bytes(solo) == shard_bytes(ml[1])
    assert len({shard_bytes(m) for m in ml}) == 3                                    # item tables, MLP and head stay per shard
    assert (s.log0['total_rmse'], s.log0['total_ndcg'], s.log0['total_hr']) == tuple(baseTest(synthetic_loaders()[3], ml))
    # unlearn: the deleted users' shard is retrained, the others keep their bytes
    assert s2.retrained == [1]
    assert shard_bytes(ml2[0]) == shard_bytes(ml[0]) and shard_bytes(ml2[2]) == shard_bytes(ml[2]) and shard_bytes(ml2[1]) != shard_bytes(ml[1])
    for name in ('user_mat_mf', 'user_mat_mlp'):
        old, new = getattr(ml[0], name).weight.detach().cpu().numpy(), getattr(ml2[0], name).weight.detach().cpu().numpy()
        assert np.array_equal(old[idx[0]], new[idx[0]]) and np.array_equal(old[idx[2]], new[idx[2]]) and not np.array_equal(old[idx[1]], new[idx[1]])
        assert all(np.array_equal(new, getattr(m, name).weight.detach().cpu().numpy()) for m in ml2)
    tot2 = synthetic_loaders(idx[1][:5])[3]
    assert (s2.log0['total_rmse'], s2.log0['total_ndcg'], s2.log0['total_hr']) == tuple(baseTest(tot2, ml2))
    # the refusals, on trained models
    from ultrare_amd.method import utils
    for who, call in (('recommend', lambda: s2.recommend([0, 1])), ('rank_eval', lambda: s2.rank_eval(tot2)), ('fit_combiner', lambda: s2.fit_combiner([None] * 3)),
                      ('test_combined', lambda: s2.test_combined(tot2, 0, '')), ('fold_in', lambda: s2.fold_in(tot2, 0.1)),
                      ('attribute_unlearn', lambda: s2.attribute_unlearn([0], [1])), ('als_sweeps', lambda: utils.als_sweeps(ml2[0], tot2, 0.1)),
                      ('padded_tables', lambda: utils.padded_tables(ml2[0])), ('recommend', lambda: utils.recommend(ml2, [0]))):
        with pytest.raises(ValueError, match=who + ".*'nmf' backbone"):
            call()
    with pytest.raises(ValueError, match="not 'nmf'"):
        s2.unlearn_influence(ml2, [None] * 3, tot2, [0], 0, '')
    with pytest.raises(ValueError, match='one backbone'):
        baseTest(tot2, [ml2[0], utils.MF(SYN_USER, SYN_ITEM, 8).to('cuda')])


def sisa_shard_alone(i):
    """Shard i of the synthetic request trained by a plain Scratch under the stream Sisa.learn gives it (the shards before it draw first)."""
    from ultrare_amd.method.scratch import Scratch
    idx, trd, ted, tot = synthetic_loaders()
    torch.manual_seed(42)
    sc = Scratch(Param(2, 8, [16, 8], SYN_USER, SYN_ITEM, batch=200), 'nmf')
    for j in range(i + 1):
        model = sc.train(trd[j], ted[j], tot, 0, '', j + 1)
    return model


def test_forward_equals_the_op(nv):
    from ultrare_amd import ops  # noqa: F401
    from ultrare_amd.method.utils import NMF
    torch.manual_seed(3)
    m = NMF(23, 31, 16, [64, 32, 16, 8]).to('cuda')
    rs = np.random.RandomState(4)
    uid, iid = torch.from_numpy(rs.randint(0, 23, 300)).cuda(), torch.from_numpy(rs.randint(0, 31, 300)).cuda()
    U, V, dense = m.tables()
    got = m(uid, iid)
    assert got.cpu().numpy().tobytes() == torch.ops.ultrare.nmf_score(U, V, dense, 16, [64, 32, 16, 8], uid, iid).cpu().numpy().tobytes()
    want = nmf.forward_ref(U.cpu().numpy(), V.cpu().numpy(), dense.cpu().numpy(), 16, [64, 32, 16, 8], uid.cpu().numpy(), iid.cpu().numpy())[0]
    assert got.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(nv.NativeError, match='HIP device only'):
        torch.ops.ultrare.nmf_score(U.cpu(), V.cpu(), dense.cpu(), 16, [64, 32, 16, 8], uid.cpu(), iid.cpu())


def test_instance_writes_the_nmf_artifacts(nv, tmp_path):
    import shutil
    from ultrare_amd.config import InsParam, Instance
    data = tmp_path / 'data'
    (data / 'toy').mkdir(parents=True)
    shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
    shutil.copy(TEST, data / 'toy' / '0_test.csv')
    save = tmp_path / 'result'
    torch.manual_seed(42)
    p = InsParam('toy', 1, 24, [32, 16], 2, 2, 'rand', data_dir=str(data), model='nmf', lr=1e-4)
    models = Instance(p, save_dir=str(save)).runGroup(is_save=True, learn_type='sisa', group_type='uniform', n_group=2, verbose=0)
    assert len(models) == 2
    base = save / '2' / 'rand' / 'toy_g2'
    for f in ('NMF_uniform_sisa_learn/log0.npy', 'NMF_uniform_sisa_learn/user_mat_mf2.npy', 'NMF_uniform_sisa_learn/user_mat_mlp1.npy',
              'NMF_uniform_sisa_learn/item_mat_mlp2.npy', 'NMF_uniform_sisa_learn/model1.pth', 'NMF_uniform_sisa_unlearn/log0.npy'):
        assert (base / f).exists(), f
    assert not list(base.glob('MF_*')) and not list(base.glob('LightGCN_*'))
    P = np.load(base / 'NMF_uniform_sisa_learn' / 'user_mat_mlp1.npy')
    assert P.shape == (N_USER, 16) and np.isfinite(P).all()


@pytest.mark.parametrize('model,group', C.ARTIFACT_RUNS, ids=lambda v: str(v))
def test_the_other_backbones_write_the_artifacts_they_wrote_before(nv, tmp_path, model, group):
    """`--model mf` (a 2-shard request and the full-train / retrain pair) and `--model lightgcn` through main on the toy set: every
    file -- param, deletion, model, user_mat, item_mat, base_*, log, log0 -- has the digest recorded from the commit before this
    backbone existed (tests/golden/backbone_artifacts.json; nmf_cases.artifact_digests says what of a file is hashed)."""
    import json
    import shutil
    from ultrare_amd.main import main
    data = tmp_path / 'data'
    (data / 'toy').mkdir(parents=True)
    shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
    shutil.copy(TEST, data / 'toy' / '0_test.csv')
    main(C.artifact_args(model, group, str(data), str(tmp_path / 'result')))
    with open(os.path.join(G, 'backbone_artifacts.json')) as f:
        want = json.load(f)[f'{model}_g{group}']
    got = C.artifact_digests(str(tmp_path / 'result'))
    assert sorted(got) == sorted(want) and len(want) >= 10
    assert {name: got[name] for name in want if got[name] != want[name]} == {}
    assert any('user_mat' in n for n in want) and any(n.endswith('.pth') for n in want) and any('log0' in n for n in want)
