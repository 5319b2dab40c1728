"""Weighted matrix factorisation for implicit feedback on the device (csrc/wmf.hip), held to the numpy contract of
ultrare_amd/wmf.py: ure_gram to the bit at every width and around every chunk edge, on two streams and on dirty memory inside
guard zones; ure_wridge_rows to ure_ridge_rows's bytes where the two coincide, to the float64 contract under a derived bound
where they do not, its independence of stream / order / company, its failure path, the torch ops and the raw ABI; then
utils.wmf_sweeps / wmf_fold_in and the 'wmf' backbone through Scratch, Sisa and Instance on the reference's toy set."""
import copy
import os

import numpy as np
import pytest
import torch

import wmf_cases as C
from abi_arena import Arena, run_prefills, verdict
from ultrare_amd import ridge
from ultrare_amd import wmf as W

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071
WIDTHS = [(4, 4), (8, 8), (5, 8), (16, 16), (32, 32), (64, 64), (128, 128), (100, 128)]          # (k, d)
ROWS = [1, 255, 256, 257, 513, 76801]          # one chunk, the chunk edges, a few chunks, 301 chunks


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import _native
    return _native


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_TABLES = {}


def _gram_case(n, d, k):
    """(F, gram_ref(F, k)) of one shape, made once: tables of equal (n, d) share their values."""
    if (n, d) not in _TABLES:
        _TABLES[n, d] = C.normal_table(n, d, seed=1000 * d + n % 997)
    F = _TABLES[n, d]
    return F, W.gram_ref(F, k)


# ---- 1. ure_gram ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('k,d', WIDTHS)
def test_gram_is_the_contract_to_the_bit(nv, k, d, n):
    """Through the raw ABI on dirty memory inside guard zones at exactly the sizer's scratch (three prefills: the bytes must not
    depend on what the memory held), and through engine.gram on the current and on a side stream."""
    from ultrare_amd import engine
    F, want = _gram_case(n, d, k)
    L = nv.lib()
    tri = k * (k + 1) // 2
    ar = Arena('cuda')
    ar.input('F', F)
    ar.output('G0', 8 * tri)
    ar.scratch('ws', L.ure_gram_scratch(n, k))
    assert ar.size('ws') == -(-n // 256) * tri * 8
    st = nv.stream_handle(None)
    call = lambda a: nv.check(L.ure_gram(a.addr('F'), n, d, k, a.addr('G0'), a.addr('ws'), a.size('ws'), st), 'ure_gram')
    reports = run_prefills(ar, call, sync=torch.cuda.synchronize)
    assert verdict(reports) == []
    assert reports[0].outputs['G0'] == want.tobytes()
    Fd = _dev(F)
    here = engine.gram(Fd, d, k)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = engine.gram(Fd, d, k, stream=side)
    torch.cuda.synchronize()
    assert here.dtype == torch.float64 and here.shape == (tri,)
    assert _bytes(here) == want.tobytes() and _bytes(there) == want.tobytes()


def test_gram_refusals_and_the_op(nv):
    from ultrare_amd import engine, ops  # noqa: F401  (registers torch.ops.ultrare.*)
    F = _dev(C.normal_table(300, 16, 1))
    assert _bytes(torch.ops.ultrare.gram(F, 12)) == _bytes(engine.gram(F, 16, 12)) == W.gram_ref(F.cpu().numpy(), 12).tobytes()
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fake = torch.ops.ultrare.gram(mode.from_tensor(F), 12)
    assert tuple(fake.shape) == (78,) and fake.dtype == torch.float64
    with pytest.raises(nv.NativeError, match='HIP device only'):
        torch.ops.ultrare.gram(F.cpu(), 12)
    with pytest.raises(ValueError, match='does not fit in LDS'):
        engine.gram(torch.zeros(4, 256, device='cuda'), 256, 200)
    with pytest.raises(ValueError, match='1 <= k <= d'):
        engine.gram(F, 16, 17)


# ---- 2. ure_wridge_rows -----------------------------------------------------------------------------------------------------------
def _edge_lens(d):
    T = C.tile_rows(d)
    return [0, 1, T - 1, T, T + 1, 3 * T + 1]


@pytest.mark.parametrize('k,d', WIDTHS + [(3, 4), (20, 64)])
def test_unit_confidence_without_a_gram_matrix_gives_ridge_rows_bytes(k, d):
    """(a) wg = 1, wb = val, G0 = None: the weighted kernel's accumulate multiplies by exactly 1.0 and adds nothing at the store."""
    from ultrare_amd import engine
    lens = _edge_lens(d) + [k, 2 * k + 1, 500]
    F = _dev(C.normal_table(300, d, seed=k))
    seg, idx, val = C.segments_of(lens, 300, seed=k + 1)
    segs = engine.SegmentSet(seg, idx, val, len(lens))
    for l2, l2_n in ((0.5, 0.0), (1e-2, 0.05)):
        want = engine.ridge_rows(F, d, k, segs, l2, l2_n)
        got = engine.wridge_rows(F, d, k, segs, torch.ones_like(segs.val), segs.val, None, l2, l2_n)
        assert got.shape == (len(lens), d) and got.dtype == torch.float32
        assert _bytes(got) == _bytes(want)


@pytest.mark.parametrize('alpha,l2,l2_n', [(40.0, 0.1, 0.0), (3.0, 0.5, 0.05)])
@pytest.mark.parametrize('k,d', WIDTHS)
def test_rows_match_the_float64_contract(k, d, alpha, l2, l2_n):
    """(b) with G0 from ure_gram.  l2 = 0.1 (the backbone's default) and 0.5: the Gram matrix of 400 normal rows has eigenvalues
    of the order of 400 in every direction and the confidences add at most alpha n_s |f|^2, so cond stays below a few hundred and
    (n_fixed + n_s + k) cond far inside 2^26 by the contract alone; check_rows asserts that per segment before it compares."""
    from ultrare_amd import engine
    lens = _edge_lens(d) * 2 + [0, 2, k, 2 * k + 1]
    Fh = C.normal_table(400, d, seed=10 + k)                # the padding columns are NOT zero: they must not enter
    F = _dev(Fh)
    seg, idx, val = C.segments_of(lens, 400, seed=k + 2)
    segs = engine.SegmentSet(seg, idx, val, len(lens))
    wg, wb = engine.confidence(segs.val, alpha)
    wg_h, wb_h = W.confidence_ref(val, alpha)
    assert _bytes(wg) == wg_h.tobytes() and _bytes(wb) == wb_h.tobytes()
    G0 = engine.gram(F, d, k)
    X = engine.wridge_rows(F, d, k, segs, wg, wb, G0, l2, l2_n).cpu().numpy()
    assert X.shape == (len(lens), d) and X.dtype == np.float32
    off = np.concatenate([[0], np.cumsum(lens)])
    C.check_rows(X, Fh, k, off, idx, wg_h, wb_h, G0.cpu().numpy(), l2, l2_n, what=f'k={k} d={d} alpha={alpha} l2={l2} l2_n={l2_n}')


@pytest.mark.parametrize('k', [5, 32, 128, 64, 3])
def test_bytes_do_not_depend_on_stream_order_or_company(k):
    """(c)"""
    from ultrare_amd import engine
    d = engine.pad_dim(k)
    rs = np.random.RandomState(k)
    lens = rs.choice([0, 1, 3, k, 2 * k + 1, 77, 300], 60)
    F = _dev(C.normal_table(300, d, seed=2))
    seg, idx, val = C.segments_of(lens, 300, seed=3)
    segs = engine.SegmentSet(seg, idx, val, len(lens))
    wg, wb = engine.confidence(segs.val, 40.0)
    G0 = engine.gram(F, d, k)
    run = lambda **kw: engine.wridge_rows(F, d, k, segs, wg, wb, G0, 0.1, 0.01, **kw)
    base = run(order=None)
    torch.cuda.synchronize()
    longest = segs.order.cpu().numpy()
    variants = [run(), run(order=longest[::-1].copy()), run(order=rs.permutation(len(lens)))]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        variants.append(run(stream=side))
    torch.cuda.synchronize()
    for v in variants:
        assert _bytes(v) == _bytes(base)
    off = np.concatenate([[0], np.cumsum(lens)])
    for s in (int(longest[0]), int(longest[20]), int(np.flatnonzero(lens == 1)[0])):          # a segment solved alone
        a, b = off[s], off[s + 1]
        alone = engine.wridge_rows(F, d, k, engine.SegmentSet(np.zeros(b - a, int), idx[a:b], val[a:b], 1), wg[a:b].contiguous(), wb[a:b].contiguous(),
                                   G0, 0.1, 0.01)
        assert _bytes(alone[0]) == _bytes(base[s]), s


def test_a_rank_deficient_segment_is_reported_and_spoils_no_other_row():
    """(d) k = 16, l2 = 0, G0 from a 3-row table, one entry in the segment.  The table's columns 3 .. 15 are zero, so every entry
    of G outside its leading 3 x 3 block is exactly 0.0 and the fourth pivot is exactly zero -- a fact of the inputs, not of
    rounding.  The kernel marks the segment in a status word; nothing faults.  The fixed table holds the 3 rows first and 200
    full-width rows behind them: the other segments draw from those and are full rank through their own entries."""
    from ultrare_amd import engine
    k = d = 16
    small = np.zeros((3, d), dtype=np.float32)
    small[:, :3] = C.normal_table(3, 3, 5)
    G0 = engine.gram(_dev(small), d, k)                     # rank 3
    Fh = np.vstack([small, C.normal_table(200, d, seed=6)])          # rows 0 .. 2: the small table; the others: full width
    F = _dev(Fh)
    lens = np.array([60, 48, 1, 100, 0, 55])
    seg, idx, val = C.segments_of(lens, 200, seed=7)
    idx = idx + 3
    idx[seg == 2] = 1                                       # the one-entry segment points into the small table
    wg_h, wb_h = W.confidence_ref(val, 40.0)
    full = engine.SegmentSet(seg, idx, val, len(lens))
    wg, wb = engine.confidence(full.val, 40.0)
    with pytest.raises(ValueError, match=r'first segment 2 .*l2 = 0') as info:
        engine.wridge_rows(F, d, k, full, wg, wb, G0, 0.0, 0.0)
    err = info.value
    assert err.failed == 1 and err.segment == 2
    X = err.X
    assert torch.isnan(X[2]).all() and torch.isfinite(X[[0, 1, 3, 4, 5]]).all() and not X[4].any()
    off = np.concatenate([[0], np.cumsum(lens)])
    assert W.wridge_rows_ref(Fh, k, off, idx, wg_h, wb_h, G0.cpu().numpy(), 0.0, 0.0)[1] == [2]          # the contract lists it too
    keep = seg != 2
    rest = engine.SegmentSet(seg[keep], idx[keep], val[keep], len(lens))
    good = engine.wridge_rows(F, d, k, rest, *engine.confidence(rest.val, 40.0), G0, 0.0, 0.0)
    assert not good[2].any()                                # (now an empty segment)
    for s in (0, 1, 3, 4, 5):
        assert _bytes(X[s]) == _bytes(good[s]), s
    assert torch.isfinite(engine.wridge_rows(F, d, k, full, wg, wb, G0, 1e-3, 0.0)).all()
    with pytest.raises(ValueError, match='outside the fixed table'):
        engine.wridge_rows(F, d, k, engine.SegmentSet(seg, idx + 203, val, len(lens)), wg, wb, G0, 0.5)
    with pytest.raises(ValueError, match='one per entry'):
        engine.wridge_rows(F, d, k, full, wg[:-1].contiguous(), wb, G0, 0.5)
    with pytest.raises(ValueError, match='packed triangle'):
        engine.wridge_rows(F, d, k, full, wg, wb, G0[:-1].contiguous(), 0.5)


def test_torch_op_equals_the_engine_call(nv):
    """(e)"""
    from ultrare_amd import engine, ops  # noqa: F401
    k, d = 12, 16
    lens = np.array([30, 0, 14, 200, 5])
    F = _dev(C.normal_table(100, d, seed=7))
    seg, idx, val = C.segments_of(lens, 100, seed=8)
    segs = engine.SegmentSet(seg, idx, val, len(lens))
    wg, wb = engine.confidence(segs.val, 40.0)
    G0 = engine.gram(F, d, k)
    for g in (G0, None):
        want = engine.wridge_rows(F, d, k, segs, wg, wb, g, 0.3, 0.02)
        got = torch.ops.ultrare.wridge_rows(F, segs.off, segs.idx, wg, wb, g, k, 0.3, 0.02)
        assert got.dtype == torch.float32 and _bytes(got) == _bytes(want)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        f = mode.from_tensor
        fake = torch.ops.ultrare.wridge_rows(f(F), f(segs.off), f(segs.idx), f(wg), f(wb), f(G0), k, 0.3, 0.02)
    assert tuple(fake.shape) == (5, 16) and fake.dtype == torch.float32
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.wridge_rows(F.cpu(), segs.off, segs.idx, wg, wb, G0, k, 0.3, 0.02)


@pytest.mark.parametrize('with_g0', [True, False])
@pytest.mark.parametrize('k,d', [(5, 8), (32, 32), (100, 128)])
def test_wridge_rows_on_dirty_memory_inside_guard_zones(nv, k, d, with_g0):
    """(f) the raw ABI, `order` given, scratch of exactly the sizer's 0 bytes (fenced by guards all the same)."""
    from ultrare_amd import engine
    L = nv.lib()
    lens = _edge_lens(d) + [2 * k + 1]
    m = len(lens)
    Fh = C.normal_table(150, d, seed=k)
    seg, idx, val = C.segments_of(lens, 150, seed=k + 1)
    off, idx_c, val_c, order = ridge.segment_csr(seg, idx, val, m)
    wg, wb = W.confidence_ref(val_c, 40.0)
    G0 = W.gram_ref(Fh, k)
    ar = Arena('cuda')
    ar.input('F', Fh), ar.input('off', off), ar.input('idx', idx_c), ar.input('wg', wg), ar.input('wb', wb), ar.input('order', order), ar.input('G0', G0)
    ar.output('X', 4 * m * d), ar.output('status', 8)
    ar.scratch('ws', L.ure_wridge_rows_scratch(m, k))
    assert ar.size('ws') == 0
    st = nv.stream_handle(None)
    call = lambda a: nv.check(L.ure_wridge_rows(a.addr('F'), 150, d, k, a.addr('off'), a.addr('idx'), a.addr('wg'), a.addr('wb'), m, a.addr('order'),
                                                a.addr('G0') if with_g0 else None, 0.1, 0.01, a.addr('X'), a.addr('status'), a.addr('ws'), 0, st),
                              'ure_wridge_rows')
    reports = run_prefills(ar, call, sync=torch.cuda.synchronize)
    assert verdict(reports) == []
    assert np.frombuffer(reports[0].outputs['status'], dtype=np.int32).tolist() == [0, -1]
    segs = engine.SegmentSet(seg, idx, val, m)
    want = engine.wridge_rows(_dev(Fh), d, k, segs, _dev(wg), _dev(wb), _dev(G0) if with_g0 else None, 0.1, 0.01)
    assert reports[0].outputs['X'] == _bytes(want)


# ---- 3. utils.wmf_sweeps, wmf_fold_in ---------------------------------------------------------------------------------------------
def _synthetic():
    uid, iid, r = C.rating_set(300, 200, 6000, seed=11, skip_user=7, skip_item=3)
    return uid, iid, r, C.normal_table(300, 8, 12), C.normal_table(200, 8, 13)


def test_wmf_sweeps_objectives_and_first_half_sweep():
    """The objectives against wmf_sweeps_ref's own, at the relative tolerance tests/test_gpu_ridge.py uses for als_sweeps (1e-12:
    float64 sums of the same terms in another order).  The reference's tables are its own float32 roundings of float64 rows the
    device matches to ~1e-13, so the two runs hold the same tables unless a value straddles a float32 rounding boundary."""
    from ultrare_amd.method.utils import MF, wmf_sweeps
    uid, iid, r, U0, V0 = _synthetic()
    k, alpha, l2 = 8, 40.0, 0.1
    model = MF.from_tables(_dev(U0), _dev(V0))
    torch_state, numpy_state = torch.get_rng_state(), np.random.get_state()[1].copy()
    for l2_n in (0.0, 0.02):
        out, obj = wmf_sweeps(model, (uid, iid, r), alpha, l2, l2_n, sweeps=1)
        U1, V1 = out.user_mat.weight.detach().cpu().numpy(), out.item_mat.weight.detach().cpu().numpy()
        assert obj.dtype == np.float64 and obj.shape == (3,) and U1.shape == U0.shape and V1.shape == V0.shape
        _, _, want = W.wmf_sweeps_ref(U0, V0, uid, iid, r, alpha, l2, l2_n, sweeps=1)
        print(f'l2_n={l2_n}: objectives {obj.tolist()}, relative error {[abs(a - b) / b for a, b in zip(obj, want)]}')
        assert all(abs(a - b) <= 1e-12 * b for a, b in zip(obj, want))
        assert obj[2] <= obj[1] <= obj[0]
        assert not U1[7].any() and not V1[3].any()          # no observations: the zero row
        # the first half sweep is the contract's U against V0 and the Gram matrix of ALL of V0
        off, idx, val, _ = ridge.segment_csr(uid, iid, r, 300)
        wg, wb = W.confidence_ref(val, alpha)
        C.check_rows(U1, V0, k, off, idx, wg, wb, W.gram_ref(V0, k), l2, l2_n, what=f'wmf first half, l2_n={l2_n}')
    assert torch.equal(torch.get_rng_state(), torch_state) and np.array_equal(np.random.get_state()[1], numpy_state)      # no RNG drawn
    same, obj0 = wmf_sweeps(model, (uid, iid, r), alpha, l2, 0.02, sweeps=0)
    assert obj0.shape == (1,) and abs(obj0[0] - want[0]) <= 1e-12 * want[0]          # (want: the last case's, l2_n = 0.02)
    assert torch.equal(same.user_mat.weight.detach(), model.user_mat.weight.detach()) and torch.equal(same.item_mat.weight.detach(), model.item_mat.weight.detach())
    out3, obj3 = wmf_sweeps(model, (uid, iid, r), alpha, l2, sweeps=3)
    print('three sweeps:', obj3.tolist())
    assert len(obj3) == 7 and all(b <= a * (1 + 1e-6) for a, b in zip(obj3[:-1], obj3[1:]))
    with pytest.raises(ValueError, match='l2'):
        wmf_sweeps(model, (uid, iid, r), alpha, 0.0)


def test_wmf_fold_in_equals_a_user_half_sweep_on_those_users():
    from ultrare_amd.method.utils import MF, wmf_fold_in, wmf_sweeps
    uid, iid, r, U0, V0 = _synthetic()
    model = MF.from_tables(_dev(U0), _dev(V0))
    out, _ = wmf_sweeps(model, (uid, iid, r), 40.0, 0.1, 0.02, sweeps=1)
    pick = np.isin(uid, [4, 5, 250, 299])
    users, rows = wmf_fold_in([model], (uid[pick], iid[pick], r[pick]), 40.0, 0.1, 0.02, item_table=0)
    assert users.tolist() == [4, 5, 250, 299] and rows.shape == (4, 8) and rows.dtype == torch.float32 and rows.is_cuda
    assert _bytes(rows) == _bytes(out.user_mat.weight.detach()[_dev(users)])
    users2, rows2 = wmf_fold_in([model, model], (uid[pick], iid[pick], r[pick]), 40.0, 0.1, 0.02)          # the mean of two equal tables
    assert users2.tolist() == users.tolist() and _bytes(rows2) == _bytes(rows)
    with pytest.raises(ValueError, match='item_table'):
        wmf_fold_in([model], (uid, iid, r), 40.0, 0.1, item_table=1)
    with pytest.raises(ValueError, match='alpha'):
        wmf_fold_in([model], (uid, iid, r), -1.0, 0.1)


# ---- 4. the backbone on the toy set -----------------------------------------------------------------------------------------------
class Param:
    def __init__(self, epochs, parallel=False):
        self.k, self.lam, self.seed, self.batch = 16, 0.1, 42, 3000
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, parallel


def _loaders(S, del_user=(), groups=()):
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, list(del_user), [], S, list(groups))
    te, _ = readRating(TEST, N_USER, 5, [], [], S, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    return idx, trd, ted, loadData(RatingData(np.hstack(te)), 3000, 24, False)


def _tables(m):
    return _bytes(m.user_mat.weight), _bytes(m.item_mat.weight)


def test_scratch_trains_and_writes_the_artifacts(tmp_path):
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.utils import MF, wmf_sweeps
    from ultrare_amd import rng
    from ultrare_amd.method.utils import seed_all
    _, trd, ted, _ = _loaders(1)
    runs = []
    for out in ('a', 'b'):
        (tmp_path / out).mkdir()
        sc = Scratch(Param(2), 'wmf')
        torch.manual_seed(42)
        model = sc.train(trd[0], ted[0], [], 0, str(tmp_path / out))
        assert sorted(os.listdir(tmp_path / out)) == ['item_mat0.npy', 'log0.npy', 'model0.pth', 'user_mat0.npy']
        log = np.load(tmp_path / out / 'log0.npy', allow_pickle=True).item()
        for key in ('train_loss', 'test_rmse', 'test_ndcg', 'test_hr', 'time'):
            assert len(log[key]) == 2 and len(sc.log[key]) == 2, key
        assert np.isfinite([log[key] for key in ('train_loss', 'test_rmse', 'test_ndcg', 'test_hr')]).all()
        assert log['train_loss'][1] < log['train_loss'][0]
        assert np.load(tmp_path / out / 'user_mat0.npy').tobytes() == _tables(model)[0] and np.load(tmp_path / out / 'item_mat0.npy').tobytes() == _tables(model)[1]
        runs.append(_tables(model) + (log['train_loss'],))
    assert runs[0] == runs[1]                               # two runs of the same request give equal bytes
    # ... and they are utils.wmf_sweeps from the MF request's own draws, with the untuned defaults
    torch.manual_seed(42)
    seed_all(42)
    U0, V0 = rng.mf_init(N_USER, N_ITEM, 16)
    direct, obj = wmf_sweeps(MF.from_tables(U0.cuda(), V0.cuda()), trd[0], 40.0, 0.1, sweeps=2)
    assert _tables(direct) == runs[0][:2] and [obj[2], obj[4]] == runs[0][2]


def test_sisa_learns_unlearns_and_serves(tmp_path):
    import warnings
    from ultrare_amd.method import utils
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.sisa import Sisa
    idx, trd, ted, tot = _loaders(3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        s = Sisa(Param(2, parallel=True), 'wmf', 3, idx)
    assert s.parallel is False and sum('one after the other' in str(w.message) for w in caught) == 1
    torch.manual_seed(42)
    ml = s.learn(trd, ted, tot, 0, '')
    assert len(ml) == 3 and all(np.isfinite(v).all() for key, v in s.log.items() if key != 'time') and len(s.log['train_loss']) == 6
    merged = ml[0].user_mat.weight.detach()
    before = [(_bytes(m.item_mat.weight), _bytes(merged[_dev(np.asarray(g, dtype=np.int64))])) for m, g in zip(ml, idx)]
    # the ensemble is two dot-product tables per shard: the rest of the surface takes it unchanged
    scores, items = utils.recommend(ml, np.arange(20), top_k=10)
    assert torch.isfinite(scores).all() and int(items.min()) >= 0
    metrics = utils.rank_eval(ml, tot, ks=(10,))
    print('rank_eval of the WMF ensemble (2 sweeps, untuned defaults):', metrics)
    assert all(np.isfinite(v) for v in metrics.values())
    # deleting users of shard 1 retrains that shard only, from scratch, by the same sweeps
    del_user = [int(u) for u in idx[1][:5]]
    idx2, trd2, ted2, tot2 = _loaders(3, del_user, idx)
    s2 = Sisa(Param(2), 'wmf', 3, idx2)
    torch.manual_seed(42)
    ml2 = s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, str(tmp_path))
    assert s2.retrained == [1]
    assert sorted(os.listdir(tmp_path)) == ['item_mat2.npy', 'log0.npy', 'log2.npy', 'model2.pth', 'user_mat2.npy']
    merged2 = ml2[0].user_mat.weight.detach()
    after = [(_bytes(m.item_mat.weight), _bytes(merged2[_dev(np.asarray(g, dtype=np.int64))])) for m, g in zip(ml2, idx)]
    assert after[0] == before[0] and after[2] == before[2]                  # untouched shards: byte-identical tables and rows
    assert after[1][0] != before[1][0] and after[1][1] != before[1][1]
    # the retrained shard is a fresh Scratch run on its remaining data, bit for bit
    torch.manual_seed(42)
    fresh = Scratch(Param(2), 'wmf').train(trd2[1], ted2[1], tot2, 0, '')
    own = _dev(np.asarray(idx2[1], dtype=np.int64))
    assert _bytes(ml2[1].item_mat.weight) == _bytes(fresh.item_mat.weight)
    assert _bytes(merged2[own]) == _bytes(fresh.user_mat.weight.detach()[own])
    assert not fresh.user_mat.weight.detach()[_dev(np.asarray(del_user))].any()          # a deleted user has no observation: the zero row
    assert np.isfinite([s2.log0['total_rmse'], s2.log0['total_ndcg'], s2.log0['total_hr']]).all()
    with pytest.raises(ValueError, match="model='mf' only"):
        s2.unlearn_influence(ml2, trd2, tot2, del_user, 0, '')


def test_instance_runs_the_group_stage_and_writes_wmf_artifacts(tmp_path):
    import shutil
    from ultrare_amd.config import InsParam, Instance
    data = tmp_path / 'data'
    (data / 'toy').mkdir(parents=True)
    shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
    shutil.copy(TEST, data / 'toy' / '0_test.csv')
    save = tmp_path / 'result'
    torch.manual_seed(42)
    p = InsParam('toy', 2, 24, [32], 2, 2, 'rand', data_dir=str(data), model='wmf')
    models = Instance(p, save_dir=str(save)).runGroup(is_save=True, learn_type='sisa', group_type='uniform', n_group=2, verbose=0)
    assert len(models) == 2
    base = save / '2' / 'rand' / 'toy_g2'
    for f in ('log0.npy', 'user_mat1.npy', 'item_mat2.npy', 'model1.pth', 'log2.npy'):
        assert (base / 'WMF_uniform_sisa_learn' / f).exists(), f
    assert (base / 'WMF_uniform_sisa_unlearn' / 'log0.npy').exists()
    assert not list(base.glob('MF_*')) and not list(base.glob('LightGCN_*'))
    log = np.load(base / 'WMF_uniform_sisa_learn' / 'log1.npy', allow_pickle=True).item()
    assert len(log['train_loss']) == 2 and np.isfinite(log['train_loss']).all()
    U = np.load(base / 'WMF_uniform_sisa_learn' / 'user_mat1.npy')
    assert U.shape == (N_USER, 16) and np.isfinite(U).all()
