"""The batched ridge solves on the device (csrc/mf_ridge.hip), held to the numpy contract ridge.ridge_rows_ref: accuracy
at every served kind of width and segment length, bitwise independence of stream / order / company, the failure path (an
arithmetic status word, never a device fault), the torch op, utils.fold_in on the reference's toy ensembles, Sisa.fold_in /
forget_folded end to end, utils.als_sweeps, and the configs[3] shapes (each in a child process under its own time limit)."""
import copy
import os
import time

import numpy as np
import pytest
import torch

if __name__ == '__main__':          # the scale tests' child process: what conftest.py does for a pytest run
    import sys
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071
COND_LIMIT = 2.0 ** 26            # the input condition of the small cases: (n_s + k) * cond(G_s) <= 2^26
BOUND = 2.0 ** -23                # ... under which |x_dev - x_64| <= 2^-23 max |x_64| per row


def segments_of(lens, n_fixed, seed):
    """A CSR with the given segment lengths, ids drawn with replacement (repeats inside a segment), ratings in {0.2 .. 1}."""
    rs = np.random.RandomState(seed)
    seg = np.repeat(np.arange(len(lens)), lens)
    return seg, rs.randint(0, n_fixed, len(seg)), (rs.randint(1, 6, len(seg)) / 5.0).astype(np.float32)


def normal_table(n, d, seed):
    return np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)


def check_against_contract(X, F, k, off, idx, val, l2, l2_n, rows=None, widened=False, what=''):
    """Every row (or `rows`) of the device's X against the float64 contract.  Small cases: asserts the input condition
    (n_s + k) cond_s <= 2^26, then |x_dev - x_64| <= 2^-23 max |x_64|.  widened: the bound is computed per row from its own
    cond, (2^-24 + 4 (n_s + k) 2^-53 cond_s) max |x_64|.  Prints the worst figures before it asserts."""
    from ultrare_amd import ridge
    rows = range(len(off) - 1) if rows is None else rows
    worst, worst_cond = 0.0, 0.0
    fails = []
    for s in rows:
        a, b = int(off[s]), int(off[s + 1])
        got = X[s].astype(np.float64)
        if a == b:
            assert not got.any(), f'{what}: empty segment {s} is not the zero row'
            continue
        want = ridge.ridge_rows_ref(F, k, [0, b - a], idx[a:b], val[a:b], l2, l2_n)[0][0]
        cond = np.linalg.cond(ridge.ridge_system(F, k, idx[a:b], val[a:b], l2, l2_n)[0])
        n_s = b - a
        if widened:
            bound = 2.0 ** -24 + 4 * (n_s + k) * 2.0 ** -53 * cond
        else:
            assert (n_s + k) * cond <= COND_LIMIT, f'{what}: segment {s} (n_s = {n_s}) has cond {cond:.3g}: raise l2'
            bound = BOUND
        err = np.abs(got[:k] - want).max() / np.abs(want).max()
        worst, worst_cond = max(worst, err / bound), max(worst_cond, cond)
        if not err <= bound:
            fails.append((s, n_s, err, bound))
    print(f'{what}: worst error / bound = {worst:.3f}, largest cond = {worst_cond:.3g}')
    assert not fails, fails[:5]


# ---- 1. accuracy against the contract ---------------------------------------------------------------------------------------
# (k, d): every width the kernel is instantiated for -- 4 (one float4 per row, 1 x 1 register blocks), 8, 16, 32, 64 (the only
# width whose packed triangle, 2080 doubles, is larger than its tile of 32 rows) and 128 -- with k below, at and between the
# widths as pad_dim gives them, then k <= d / 2: a narrow system in a wide table, which pad_dim never produces but
# engine.ridge_rows accepts
KD = [pytest.param(k, d, id=str(k)) for k, d in [(5, 8), (16, 16), (32, 32), (100, 128), (128, 128)]] + \
     [pytest.param(k, d, id=f'{k}-{d}') for k, d in [(1, 4), (2, 4), (3, 4), (4, 4), (33, 64), (48, 64), (64, 64),
                                                     (3, 16), (20, 64), (40, 128)]]


def tile_rows(d):
    """Rows of one LDS tile of csrc/mf_ridge.hip (RrShape<D>::T)."""
    return 64 if d <= 32 else 2048 // d


@pytest.mark.parametrize('l2_n', [0.0, 0.05])
@pytest.mark.parametrize('l2', [0.5, 1e-2])
@pytest.mark.parametrize('k,d', KD)
def test_rows_match_the_float64_contract(k, d, l2, l2_n):
    from ultrare_amd import engine
    assert d == engine.pad_dim(d) and (d == engine.pad_dim(k) or 2 * k <= d)
    T = tile_rows(d)
    lens = [0, 1, 2, k - 1, k, k + 1, 2 * k, 500, 3000] * 2 + [0] + [T - 1, T, T + 1, 2 * T, 2 * T + 1]
    F = normal_table(400, d, seed=k)                        # the padding columns are NOT zero: they must not enter
    seg, idx, val = segments_of(lens, 400, seed=k + 1)
    segs = engine.SegmentSet(seg, idx, val, len(lens))
    X = engine.ridge_rows(torch.from_numpy(F).cuda(), d, k, segs, l2, l2_n).cpu().numpy()
    assert X.shape == (len(lens), d) and X.dtype == np.float32
    assert not X[:, k:].any()                               # padding columns are exactly zero
    off = np.concatenate([[0], np.cumsum(lens)])
    check_against_contract(X, F, k, off, idx, val, l2, l2_n, what=f'k={k} d={d} l2={l2} l2_n={l2_n}')


# ---- 2. determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [5, 32, 128, 64, 3])
def test_bytes_do_not_depend_on_stream_order_or_company(k):
    from ultrare_amd import engine
    d = engine.pad_dim(k)                                   # 8, 32, 128, 64, 4
    rs = np.random.RandomState(k)
    lens = rs.choice([0, 1, 3, k, 2 * k + 1, 77, 700], 150)
    F = torch.from_numpy(normal_table(300, d, seed=2)).cuda()
    seg, idx, val = segments_of(lens, 300, seed=3)
    segs = engine.SegmentSet(seg, idx, val, len(lens))
    longest = segs.order.cpu().numpy()
    assert (np.diff(lens[longest]) <= 0).all()
    base = engine.ridge_rows(F, d, k, segs, 0.1, 0.01, order=None)
    torch.cuda.synchronize()
    variants = [engine.ridge_rows(F, d, k, segs, 0.1, 0.01), engine.ridge_rows(F, d, k, segs, 0.1, 0.01, order=longest[::-1].copy()),
                engine.ridge_rows(F, d, k, segs, 0.1, 0.01, order=rs.permutation(len(lens)))]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        variants.append(engine.ridge_rows(F, d, k, segs, 0.1, 0.01, stream=side))
    torch.cuda.synchronize()
    for v in variants:
        assert torch.equal(v.view(torch.int32), base.view(torch.int32))
    off = np.concatenate([[0], np.cumsum(lens)])
    for s in (int(longest[0]), int(longest[40]), int(np.flatnonzero(lens == 1)[0])):          # a segment solved alone
        a, b = off[s], off[s + 1]
        alone = engine.ridge_rows(F, d, k, engine.SegmentSet(np.zeros(b - a, int), idx[a:b], val[a:b], 1), 0.1, 0.01)
        assert torch.equal(alone[0].view(torch.int32), base[s].view(torch.int32)), s


# ---- 3. the failure path --------------------------------------------------------------------------------------------------------
def test_a_rank_deficient_segment_is_reported_and_spoils_no_other_row():
    """One rating cannot fix 16 unknowns: with l2 = l2_n = 0 its second pivot is exactly zero (products of float32 values are
    exact in float64).  The kernel marks it in a status word; nothing faults."""
    from ultrare_amd import engine
    k = d = 16
    lens = np.array([60, 48, 1, 100, 0, 55])
    F = torch.from_numpy(normal_table(200, d, seed=5)).cuda()
    seg, idx, val = segments_of(lens, 200, seed=6)
    with pytest.raises(ValueError, match=r'first segment 2 .*l2 = 0') as info:
        engine.ridge_rows(F, d, k, engine.SegmentSet(seg, idx, val, len(lens)), 0.0, 0.0)
    err = info.value
    assert 'l2' in str(err) and err.failed == 1 and err.segment == 2
    X = err.X
    assert torch.isnan(X[2]).all() and torch.isfinite(X[[0, 1, 3, 4, 5]]).all() and not X[4].any()
    keep = seg != 2
    good = engine.ridge_rows(F, d, k, engine.SegmentSet(seg[keep], idx[keep], val[keep], len(lens)), 0.0, 0.0)
    assert not good[2].any()                                # (now an empty segment)
    for s in (0, 1, 3, 4, 5):
        assert torch.equal(X[s].view(torch.int32), good[s].view(torch.int32)), s
    fixed = engine.ridge_rows(F, d, k, engine.SegmentSet(seg, idx, val, len(lens)), 1e-3, 0.0)
    assert torch.isfinite(fixed).all()
    with pytest.raises(ValueError, match='outside the fixed table'):
        engine.ridge_rows(F, d, k, engine.SegmentSet(seg, idx + 200, val, len(lens)), 0.5)
    with pytest.raises(ValueError, match='does not fit in LDS'):
        engine.ridge_rows(torch.zeros(4, 256, device='cuda'), 256, 200, engine.SegmentSet([0], [0], [0.2], 1), 0.5)


# ---- 4. the torch op ------------------------------------------------------------------------------------------------------------
def test_torch_op_equals_the_engine_call():
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    from ultrare_amd import ops  # noqa: F401  (registers torch.ops.ultrare.*)
    k, d = 12, 16
    lens = np.array([30, 0, 14, 200, 5])
    F = torch.from_numpy(normal_table(100, d, seed=7)).cuda()
    seg, idx, val = segments_of(lens, 100, seed=8)
    segs = engine.SegmentSet(seg, idx, val, len(lens))
    want = engine.ridge_rows(F, d, k, segs, 0.3, 0.02)
    got = torch.ops.ultrare.ridge_rows(F, segs.off, segs.idx, segs.val, k, 0.3, 0.02)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fake = torch.ops.ultrare.ridge_rows(mode.from_tensor(F), mode.from_tensor(segs.off), mode.from_tensor(segs.idx), mode.from_tensor(segs.val),
                                            k, 0.3, 0.02)
    assert tuple(fake.shape) == (5, 16) and fake.dtype == torch.float32
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.ridge_rows(F.cpu(), segs.off, segs.idx, segs.val, k, 0.3, 0.02)


# ---- 5. utils.fold_in on the reference's toy ensembles ----------------------------------------------------------------------------
def _toy_models(tag='S3'):
    from ultrare_amd.method.utils import MF
    g = np.load(os.path.join(G, 'sisa_toy.npz'))
    S = int(tag[1:])
    U = torch.from_numpy(g[f'{tag}_learn_Umerged']).cuda()
    models = [MF.from_tables(U, torch.from_numpy(g[f'{tag}_learn_V{i}']).cuda()) for i in range(S)]
    return models, [g[f'{tag}_index{i}'].tolist() for i in range(S)], [g[f'{tag}_learn_V{i}'] for i in range(S)]


def _csv_triple(path, users=None):
    from ultrare_amd import _native as nv
    uid, iid, raw = nv.read_csv(path)
    keep = np.ones(len(uid), dtype=bool) if users is None else np.isin(uid, np.asarray(users))
    return uid[keep].astype(np.int64), iid[keep].astype(np.int64), (raw[keep] / 5).astype(np.float32)


@pytest.mark.parametrize('tag', ['S3', 'S4'])
def test_fold_in_against_one_table_and_against_the_mean(tag):
    from ultrare_amd.method.utils import fold_in
    from ultrare_amd.read import RatingData, loadData
    models, groups, Vs = _toy_models(tag)
    S, k, l2, l2_n = len(models), 16, 0.5, 0.01
    uid, iid, r = _csv_triple(TRAIN, groups[1][:200])
    shuffle = np.random.RandomState(0).permutation(len(uid))            # users arrive in any order; ids come back ascending
    uid, iid, r = uid[shuffle], iid[shuffle], r[shuffle]
    users_want = np.unique(uid)
    perm = np.argsort(uid, kind='stable')
    off = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(users_want, uid), minlength=len(users_want)))])
    mean64 = Vs[0].astype(np.float64)
    for V in Vs[1:]:
        mean64 = mean64 + V.astype(np.float64)
    tables = {s: Vs[s] for s in range(S)}
    tables['mean'] = (mean64 / S).astype(np.float32)
    for which, V in tables.items():
        users, rows = fold_in(models, (uid, iid, r), l2, l2_n, item_table=which)
        assert users.dtype == np.int64 and np.array_equal(users, users_want) and (np.diff(users) > 0).all()
        assert rows.shape == (len(users), k) and rows.dtype == torch.float32 and rows.is_cuda
        check_against_contract(rows.cpu().numpy(), V, k, off, iid[perm], r[perm], l2, l2_n, what=f'{tag} item_table={which}')
    loader = loadData(RatingData(np.vstack([uid, iid, r.astype(np.float64)])), 3000, 0, False)
    users2, rows2 = fold_in(models, loader, l2, l2_n, item_table='mean')            # a loader gives the same bytes as its triple
    assert np.array_equal(users2, users) and torch.equal(rows2, rows)
    with pytest.raises(ValueError, match='outside the fixed table'):
        fold_in(models, (uid, iid + N_ITEM, r), l2)


# ---- 6. Sisa end to end ---------------------------------------------------------------------------------------------------------
class Param:
    def __init__(self, epochs, parallel):
        self.k, self.lam, self.seed, self.batch = 16, 0.1, 42, 3000
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, parallel


def _loaders(groups, del_user=()):
    from ultrare_amd.read import RatingData, loadData, readRating
    S = len(groups)
    tr, _ = readRating(TRAIN, N_USER, 5, list(del_user), [], S, groups)
    te, _ = readRating(TEST, N_USER, 5, [], [], S, groups)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    return trd, ted, loadData(RatingData(np.hstack(te)), 3000, 24, False)


@pytest.mark.parametrize('parallel', [False, True])
def test_sisa_fold_in_forget_folded_and_unlearn(parallel, tmp_path):
    from ultrare_amd.method import utils
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.read import RatingData, loadData, readRating
    _, full = readRating(TRAIN, N_USER, 5, [], [], 3, [])
    all_uid, all_iid, all_r = _csv_triple(TRAIN)
    t_uid, _, _ = _csv_triple(TEST)
    rated = set(np.unique(all_uid).tolist()) & set(np.unique(t_uid).tolist())
    new = sorted([u for u in full[1] if u in rated][-3:])               # group 1's last users with train and test ratings ...
    groups = [[u for u in g if u not in new] for g in full]             # ... are in no list and no loader
    assert [len(g) for g in groups] == [503, 500, 502]
    trd, ted, tot = _loaders(groups)
    assert not any(set(new) & set(l.dataset.users.tolist()) for l in trd + ted + [tot])
    sisa = Sisa(Param(3, parallel), 'mf', 3, [list(g) for g in groups])
    torch.manual_seed(42)
    sisa.learn(trd, ted, tot, 0, str(tmp_path))
    assert sisa.folded == {}
    l2 = utils.trainer_l2(len(trd[1].dataset), 3000, 0.1)
    merged = sisa.model_list[0].user_mat.weight.detach()
    U_before = merged.clone()
    V_before = [m.item_mat.weight.detach().clone() for m in sisa.model_list]
    assert not U_before[new].any()                                      # nobody's row yet
    pick = np.isin(all_uid, new)
    triple = (all_uid[pick], all_iid[pick], all_r[pick])
    sisa.fit_combiner(trd)
    assert sisa.combiner is not None

    users, home = sisa.fold_in(triple, l2)
    assert users.tolist() == new and home.tolist() == [1, 1, 1]          # 500 -> 503: the smallest group every time (a tie at 502: lowest id)
    assert sisa.group_index[1] == groups[1] + new and sisa.group_index[0] == groups[0] and sisa.group_index[2] == groups[2]
    assert sisa.folded == {u: 1 for u in new} and sisa.combiner is None
    want_users, want_rows = utils.fold_in(sisa.model_list, triple, l2, item_table=1)
    for m in sisa.model_list:                                           # the one merged table every model shares
        assert m.user_mat.weight.data_ptr() == merged.data_ptr()
    assert torch.equal(merged[new].view(torch.int32), want_rows.view(torch.int32)) and merged[new].abs().sum() > 0
    rest = np.setdiff1d(np.arange(N_USER), new)
    assert torch.equal(merged[rest], U_before[rest])
    # they are served like anybody else
    te_uid, te_iid, te_r = _csv_triple(TEST, new)
    theirs = loadData(RatingData(np.vstack([te_uid, te_iid, te_r.astype(np.float64)])), 3000, 0, False)
    res = utils.baseTest(theirs, sisa.model_list)
    print(f'parallel={parallel}: folded users (rmse, ndcg, hr) = {res}')
    assert np.isfinite(res).all()
    scores, items = sisa.recommend(new, top_k=10)
    assert torch.isfinite(scores).all() and int(items.min()) >= 0
    assert all(np.isfinite(v) for v in sisa.rank_eval(theirs).values())

    sisa.fit_combiner(trd)
    sisa.forget_folded(new)
    assert sisa.folded == {} and sisa.combiner is None and sisa.group_index == groups
    assert torch.equal(merged.view(torch.int32), U_before.view(torch.int32)) and not merged[new].any()
    for m, V in zip(sisa.model_list, V_before):
        assert torch.equal(m.item_mat.weight.detach().view(torch.int32), V.view(torch.int32))
    with pytest.raises(ValueError, match='were not folded in'):
        sisa.forget_folded(new[:1])

    # against='ensemble' and explicit groups; then unlearn of a TRAINED user of group 1 drops group 1's folded users only
    users, home = sisa.fold_in(triple, l2, groups=[0, 1, 2], against='ensemble')
    assert home.tolist() == [0, 1, 2] and sisa.folded == dict(zip(new, [0, 1, 2]))
    _, ens_rows = utils.fold_in(sisa.model_list, triple, l2, item_table='mean')
    assert torch.equal(merged[new].view(torch.int32), ens_rows.view(torch.int32))
    with pytest.raises(ValueError, match='already in a group'):
        sisa.fold_in(triple, l2)
    victim = groups[1][0]
    trd2, ted2, tot2 = _loaders(sisa.group_index, del_user=[victim])
    torch.manual_seed(42)
    sisa.unlearn([copy.deepcopy(m) for m in sisa.model_list], trd2, ted2, tot2, [victim], 0, '')
    assert sisa.retrained == [1] and sisa.folded == {new[0]: 0, new[2]: 2}
    now = sisa.model_list[0].user_mat.weight.detach()
    assert torch.equal(now[[new[0], new[2]]].view(torch.int32), ens_rows[[0, 2]].view(torch.int32))      # the others' rows stay


# ---- 7. utils.als_sweeps ----------------------------------------------------------------------------------------------------------
def test_als_sweeps_objectives_and_first_half_sweep():
    from ultrare_amd import ridge
    from ultrare_amd.method.utils import MF, als_sweeps
    n_user, n_item, n, k, l2 = 2000, 500, 50000, 16, 0.5
    rs = np.random.RandomState(11)
    uid, iid = rs.randint(0, n_user, n), rs.randint(0, n_item, n)
    uid[uid == 7] = 8                                                   # a user and an item without ratings
    iid[iid == 3] = 4
    r = (rs.randint(1, 6, n) / 5.0).astype(np.float32)
    U0, V0 = normal_table(n_user, k, 12), normal_table(n_item, k, 13)
    model = MF.from_tables(torch.from_numpy(U0).cuda(), torch.from_numpy(V0).cuda())
    torch_state, numpy_state = torch.get_rng_state(), np.random.get_state()[1].copy()
    for l2_n in (0.0, 0.02):
        out, obj = als_sweeps(model, (uid, iid, r), l2, l2_n, sweeps=1)
        U1, V1 = out.user_mat.weight.detach().cpu().numpy(), out.item_mat.weight.detach().cpu().numpy()
        assert obj.dtype == np.float64 and obj.shape == (3,) and U1.shape == U0.shape and V1.shape == V0.shape
        want = [ridge.ridge_objective(U0, V0, uid, iid, r, l2, l2_n), None, ridge.ridge_objective(U1, V1, uid, iid, r, l2, l2_n)]
        want[1] = ridge.ridge_objective(U1, V0, uid, iid, r, l2, l2_n)
        print(f'l2_n={l2_n}: objectives {obj.tolist()}, relative error {[abs(a - b) / b for a, b in zip(obj, want)]}')
        assert all(abs(a - b) <= 1e-12 * b for a, b in zip(obj, want))
        assert not U1[7].any() and not V1[3].any()                      # no ratings: the zero row
        # the first half sweep is the contract's U against V0
        off, idx, val, _ = ridge.segment_csr(uid, iid, r, n_user)
        check_against_contract(U1, V0, k, off, idx, val, l2, l2_n, what=f'als first half, l2_n={l2_n}')
    assert torch.equal(torch.get_rng_state(), torch_state) and np.array_equal(np.random.get_state()[1], numpy_state)      # no RNG drawn
    out, obj = als_sweeps(model, (uid, iid, r), l2, sweeps=3)
    print('three sweeps:', obj.tolist())
    assert len(obj) == 7 and all(b <= a * (1 + 1e-8) for a, b in zip(obj[:-1], obj[1:]))
    assert obj[-1] < 0.5 * obj[0]
    U3, V3 = out.user_mat.weight.detach().cpu().numpy(), out.item_mat.weight.detach().cpu().numpy()
    assert abs(obj[-1] - ridge.ridge_objective(U3, V3, uid, iid, r, l2)) <= 1e-12 * obj[-1]
    same, obj0 = als_sweeps(model, (uid, iid, r), l2, sweeps=0)
    assert obj0.shape == (1,) and obj0[0] == obj[0] and torch.equal(same.user_mat.weight.detach(), model.user_mat.weight.detach())


# ---- 8. scale -----------------------------------------------------------------------------------------------------------------------
SCALE_TIME_LIMIT_S = 600


@pytest.mark.parametrize('side', ['user', 'item'])
def test_configs3_shape_within_memory_bound_and_against_numpy(side):
    """162,000 user segments (or 60,000 item segments with a long tail: the longest has about 80,000 entries or more) over 22.5 M entries
    at k = 128.  Runs in a child process under a time limit of its own (_scale_body below), so that a pass that does not come
    back ends there."""
    import subprocess
    import sys
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), 'scale', side]
    out = subprocess.run(cmd, timeout=SCALE_TIME_LIMIT_S, capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0 and 'scale ok' in out.stdout


def scale_lengths(side, nnz=22500000, seed=0):
    """Segment lengths of the configs[3] shape: users between 20 and a few thousand ratings, items on a power law whose top
    item has about 80,000; both sum to nnz exactly."""
    rs = np.random.RandomState(seed)
    m = 162000 if side == 'user' else 60000
    if side == 'user':
        w = rs.lognormal(0.0, 1.0, m)
        lo = 20
    else:
        w = (1.0 + np.arange(m)) ** -0.54
        rs.shuffle(w)
        lo = 1
    lens = lo + np.floor(w / w.sum() * (nnz - lo * m)).astype(np.int64)
    lens[np.argmax(lens)] += nnz - lens.sum()
    assert lens.sum() == nnz and lens.min() >= lo
    return lens


def _scale_body(side):
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    k = d = 128
    l2, l2_n = 0.5, 0.05
    lens = scale_lengths(side)
    m, n_fixed = len(lens), 60000 if side == 'user' else 162000
    seg, idx, val = segments_of(lens, n_fixed, seed=1)
    F = normal_table(n_fixed, d, seed=2)
    Fd = torch.from_numpy(F).cuda()
    segs = engine.SegmentSet(seg, idx, val, m)
    del seg
    assert nv.lib().ure_ridge_rows_scratch(m, k) == 0
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    X = engine.ridge_rows(Fd, d, k, segs, l2, l2_n)              # (reads the status words: zero, or this raises)
    t1 = time.perf_counter()
    grown = torch.cuda.max_memory_allocated() - base
    print(f'{side} side: {m} segments, longest {lens.max()}, {1e3 * (t1 - t0):.1f} ms (host clock, first call), grew {grown / 2**20:.1f} MiB')
    # the scratch formula (0) plus X, plus the status words and the caching allocator's block rounding
    assert grown <= m * d * 4 + (4 << 20), grown
    assert torch.isfinite(X).all()
    off = np.concatenate([[0], np.cumsum(lens)])
    rs = np.random.RandomState(3)
    rows = rs.choice(m, 256, replace=False)                      # 256 segments, the longest among them
    if int(np.argmax(lens)) not in rows:
        rows[0] = int(np.argmax(lens))
    rows = np.sort(rows)
    check_against_contract(X[torch.from_numpy(rows).cuda()].cpu().numpy(), F, k, np.concatenate([[0], np.cumsum(lens[rows])]),
                           np.concatenate([idx[off[s]:off[s + 1]] for s in rows]), np.concatenate([val[off[s]:off[s + 1]] for s in rows]),
                           l2, l2_n, widened=True, what=f'{side} side sample')
    print('scale ok')


if __name__ == '__main__':
    import sys
    assert sys.argv[1] == 'scale' and sys.argv[2] in ('user', 'item')
    _scale_body(sys.argv[2])
