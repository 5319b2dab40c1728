"""Catalogue sweeps under the learned shard combiner on the device (csrc/mf_combine_rank.hip): ure_recommend_topk_weighted and
ure_rank_pairs_weighted against engine.score_weighted over all (query user, item) pairs of the case, ordered on the host by the
documented key (nmf.rank_keys, held to a brute-force lexsort by tests/test_cpu_nmf_rank.py).  Every comparison is bitwise: int32
views of scores, equal integers for items and ranks."""
import ctypes

import numpy as np
import pytest
import torch

from abi_arena import Arena, run_prefills, verdict
from test_gpu_nmf_rank import bits, csr, ints, oracle_topk, random_excl, same_topk
from ultrare_amd import combine, nmf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import _native
    _native.lib()
    torch.cuda.set_device(0)
    return _native


def make_tables(S, d, n_user, n_item, seed):
    """S models of width d as numpy (U, V) pairs, scores of unit scale (every model its own tables)."""
    rs = np.random.RandomState(seed)
    scale = d ** -0.25
    return [((rs.standard_normal((n_user, d)) * scale).astype(np.float32), (rs.standard_normal((n_item, d)) * scale).astype(np.float32))
            for _ in range(S)]


def on_device(tabs):
    return [(torch.from_numpy(U).cuda(), torch.from_numpy(V).cuda()) for U, V in tabs]


def make_weights(S, G, link, seed, scale=1.0):
    """W [G, S + 1]: the mean weights disturbed, each group its own row."""
    rs = np.random.RandomState(seed)
    W = combine.mean_weights(S)[None, :] + 0.5 * rs.standard_normal((G, S + 1)) / S
    if link == 1:
        W = W * 3.0                                                                      # sigmoid(z) over its bend, not its middle
    return np.ascontiguousarray(W * scale, dtype=np.float64)


def weights_on_device(link, W, gou):
    return link, torch.from_numpy(W).cuda(), None if gou is None else torch.from_numpy(np.asarray(gou, dtype=np.int32)).cuda()


def yardstick(dev, d, users, n_item, weights):
    """[n, n_item] float32: what engine.score_weighted writes for every (query user, item) pair under the same weights."""
    from ultrare_amd import engine
    link, W, gou = weights
    uid = torch.from_numpy(np.repeat(np.asarray(users, dtype=np.int32), n_item)).cuda()
    iid = torch.from_numpy(np.tile(np.arange(n_item, dtype=np.int32), len(users))).cuda()
    pred, _ = engine.score_weighted(dev, d, uid, iid, None, link, W, gou)
    return pred.cpu().numpy().reshape(len(users), n_item)


def ranks_of(sc, targets, excl):
    return nmf.rank_ref(None, None, None, None, targets, excl, scores=sc, n_item=sc.shape[1])


# (link, d, S, n_item, n_query, top_k): every axis of the issue crossed against the base case (0, 32, 5, 65, 33, 10) -- every
# lane-group width under both links (QW changes at d = 256), S in {1, 5, 32}, n_item in {1, 63, 64, 65, 1500} (1,500 items are
# two item splits and their merge), n_query around the workgroup's QT users (32; 16 at d = 256), top_k in {1, 10, 128}
BASE = (0, 32, 5, 65, 33, 10)
CASES = sorted(set(
    [(link, d, 5, 65, 33, 10) for link in (0, 1) for d in (4, 8, 16, 32, 64, 128, 256)] +
    [(link, 32, S, 65, 33, 10) for link in (0, 1) for S in (1, 32)] +
    [(1, 256, 32, 65, 17, 10)] +
    [(link, 32, 5, n_item, 33, 10) for link in (0, 1) for n_item in (1, 63, 64, 1500)] +
    [(0, 32, 5, 65, n_query, 10) for n_query in (1, 31, 32)] + [(1, 256, 5, 65, n_query, 10) for n_query in (15, 16, 17)] +
    [(link, 32, 5, 1500 if top_k == 1 else 300, 33, top_k) for link in (0, 1) for top_k in (1, 128)]))


def case_inputs(link, d, S, n_item, n_query, seed_extra=0):
    n_user = n_query + 5
    tabs = make_tables(S, d, n_user, n_item, seed=d + 3 * S + n_item + n_query + seed_extra)
    rs = np.random.RandomState(n_item + n_query)
    users = rs.permutation(n_user)[:n_query]                                             # unsorted
    gou = np.arange(n_user) % 3                                                          # the users of one wave differ in their row
    return tabs, users, weights_on_device(link, make_weights(S, 3, link, seed=S + d), gou), rs


# ------------------------------------------------------------------ 1. top-k
@pytest.mark.parametrize('link,d,S,n_item,n_query,top_k', CASES, ids=lambda v: str(v))
def test_topk_equals_the_weighted_scores_sorted(nv, link, d, S, n_item, n_query, top_k):
    from ultrare_amd import engine
    tabs, users, weights, rs = case_inputs(link, d, S, n_item, n_query)
    dev = on_device(tabs)
    sc = yardstick(dev, d, users, n_item, weights)
    assert np.isfinite(sc).all()
    excl = random_excl(rs, n_query, n_item, 0.05)
    if n_item == 1:
        excl = (np.concatenate([np.zeros(n_query, np.int64), [1]]), np.array([0], dtype=np.int32))   # the last user's one item excluded: padding
    for ex in (None, excl):
        got = engine.recommend(dev, d, users, top_k, ex, weights=weights)
        assert got[0].shape == got[1].shape == (n_query, top_k) and got[0].dtype == torch.float32 and got[1].dtype == torch.int64
        same_topk(got, oracle_topk(sc, top_k, ex), (link, d, ex is not None))
    if (link, d, S, n_item, n_query, top_k) == BASE:                                     # per-group rows matter: the mean orders otherwise
        assert not np.array_equal(ints(engine.recommend(dev, d, users, top_k)[1]), ints(engine.recommend(dev, d, users, top_k, weights=weights)[1]))
        # ... and the numpy contract gives the same order from the per-model scores (the linear link: no exp)
        uid, iid = np.repeat(users, n_item), np.tile(np.arange(n_item), n_query)
        P = np.stack([np.einsum('ij,ij->i', U[uid].astype(np.float64), V[iid].astype(np.float64)) for U, V in tabs], axis=1).astype(np.float32)
        rows, outside = combine.weight_rows(weights[1].cpu().numpy(), uid, weights[2].cpu().numpy())
        ref = combine.weighted_scores_ref(P, link, rows, outside).reshape(n_query, n_item)
        assert np.abs(ref - sc).max() <= 1e-5 * np.abs(sc).max()                          # (P here is float64-rounded, not the kernel's tree)


# ------------------------------------------------------------------ 2. the group map
def test_group_maps_null_and_users_in_no_group(nv):
    from ultrare_amd import engine
    link, d, S, n_item, n_query = 0, 32, 5, 130, 37
    tabs, users, (_, W, gou), rs = case_inputs(link, d, S, n_item, n_query)
    users[20] = users[3]                                                                 # a user queried twice
    dev = on_device(tabs)
    targets = csr([rs.randint(0, n_item, 5) for _ in users])
    # NULL map: row 0 for everybody, whatever else W holds
    for lk in (0, 1):
        w0 = (lk, W, None)
        sc = yardstick(dev, d, users, n_item, w0)
        same_topk(engine.recommend(dev, d, users, 10, weights=w0), oracle_topk(sc, 10, None))
        assert np.array_equal(ints(engine.rank_pairs(dev, d, users, targets, weights=w0)), ranks_of(sc, targets, None))
        one = (lk, W[:1].contiguous(), None)
        assert np.array_equal(bits(engine.recommend(dev, d, users, 10, weights=one)[0]), bits(engine.recommend(dev, d, users, 10, weights=w0)[0]))
    # users with entry -1 (and one past the map's end, one with a group that does not exist) take the mean weights under link 0
    m = gou.cpu().numpy().copy()
    m[users[::4]] = -1
    m[users[1]] = 7
    short = torch.from_numpy(m[:-1].copy()).cuda()                                       # the last user id lies outside the map
    w1 = (0, W, short)
    sc = yardstick(dev, d, users, n_item, w1)
    got = engine.recommend(dev, d, users, 10, weights=w1)
    same_topk(got, oracle_topk(sc, 10, None))
    assert np.array_equal(ints(engine.rank_pairs(dev, d, users, targets, weights=w1)), ranks_of(sc, targets, None))
    lost = np.flatnonzero((m[users] < 0) | (m[users] >= 3) | (users >= len(m) - 1))
    assert len(lost) >= 9
    assert np.array_equal(bits(got[0][20]), bits(got[0][3])) and np.array_equal(ints(got[1][20]), ints(got[1][3]))
    # under link 1 such a user scores NaN everywhere: every item ties below -inf, in id order
    w2 = (1, W, short)
    sc = yardstick(dev, d, users, n_item, w2)
    assert np.isnan(sc[lost]).all() and np.isfinite(np.delete(sc, lost, axis=0)).all()
    got = engine.recommend(dev, d, users, 10, weights=w2)
    same_topk(got, oracle_topk(sc, 10, None))
    assert ints(got[1])[lost[0]].tolist() == list(range(10)) and np.isnan(got[0].cpu().numpy()[lost[0]]).all()
    assert np.array_equal(ints(engine.rank_pairs(dev, d, users, targets, weights=w2)), ranks_of(sc, targets, None))


# ------------------------------------------------------------------ 3. special values, saturation, padding
def test_special_values_ties_and_padding(nv):
    from ultrare_amd import engine
    d, S, n_user, n_item = 16, 3, 9, 1100
    tabs = make_tables(S, d, n_user, n_item, seed=5)
    for U, V in tabs:
        V[[63, 64, 575, 576]] = V[10]                                                    # equal rows across a tile and a split boundary
        V[20] = np.inf
        V[21] = np.nan
        V[22] = 0.0
        V[23] = -0.0
        U[5] = 0.0
    dev = on_device(tabs)
    users = np.array([0, 1, 2, 3, 4, 5, 6])
    gou = np.arange(n_user) % 3
    rows = [[], [10, 64], [21], np.setdiff1d(np.arange(n_item), [63, 576, 21]), np.arange(n_item), [20], [5, 6]]
    excl = csr(rows)
    targets = csr([[10, 63, 64, 575, 576, 20, 21, 22, 23, 7, 7]] * len(users))
    for link in (0, 1):
        weights = weights_on_device(link, make_weights(S, 3, link, seed=2), gou)
        sc = yardstick(dev, d, users, n_item, weights)
        assert np.isnan(sc[:, 21]).all() and np.isnan(sc[5, 20])                         # inf * 0 for the zero user
        for t in (63, 64, 575, 576):
            assert np.array_equal(bits(sc[:, t]), bits(sc[:, 10]))
        assert np.array_equal(bits(sc[:, 22]), bits(sc[:, 23]))                           # p = 0.f + dot: the -0.0 row scores as the zero row
        for ex in (None, excl):
            for top_k in (10, 128):
                same_topk(engine.recommend(dev, d, users, top_k, ex, weights=weights), oracle_topk(sc, top_k, ex), (link, top_k, ex is not None))
            assert np.array_equal(ints(engine.rank_pairs(dev, d, users, targets, ex, weights=weights)), ranks_of(sc, targets, ex))
        s, it = engine.recommend(dev, d, users, 10, excl, weights=weights)
        it = ints(it)
        assert it[4].tolist() == [-1] * 10 and np.isnan(s[4].cpu().numpy()).all()       # everything excluded
        assert it[3, :3].tolist() == [63, 576, 21] and it[3, 3:].tolist() == [-1] * 7     # the tie by id, the NaN last, then padding
        assert np.isnan(s[3, 2].item())


def test_saturated_logistic_scores_tie_by_item_id(nv):
    """Weights scaled until most items of a user share (float)mu == 1.0f and others a common tiny value: ranking is by that float,
    so the order among them is the item id's, whatever z says."""
    from ultrare_amd import engine
    d, S, n_user, n_item = 32, 5, 12, 700
    tabs = make_tables(S, d, n_user, n_item, seed=8)
    dev = on_device(tabs)
    users = np.arange(n_user)
    W = make_weights(S, 3, 1, seed=4, scale=400.0)
    W[:, :S] = np.abs(W[:, :S])
    weights = weights_on_device(1, W, np.arange(n_user) % 3)
    sc = yardstick(dev, d, users, n_item, weights)
    ones, zeros = (sc == 1.0).sum(axis=1), (sc == 0.0).sum(axis=1)
    assert (ones > 150).all() and (zeros > 150).all() and len(np.unique(sc[0])) < 200
    rs = np.random.RandomState(1)
    excl = random_excl(rs, n_user, n_item, 0.05)
    targets = csr([rs.randint(0, n_item, 8) for _ in users])
    for ex in (None, excl):
        got = engine.recommend(dev, d, users, 128, ex, weights=weights)
        same_topk(got, oracle_topk(sc, 128, ex))
        assert np.array_equal(ints(engine.rank_pairs(dev, d, users, targets, ex, weights=weights)), ranks_of(sc, targets, ex))
    it, s = ints(got[1]), got[0].cpu().numpy()
    assert (s == 1.0).all() and (np.diff(it, axis=1) > 0).all()                          # 128 of the saturated items, ascending ids
    # top_k beyond the eligible items pads with (NaN, -1)
    few = csr([np.arange(5, n_item)] * n_user)
    s, it = engine.recommend(dev, d, users, 10, few, weights=weights)
    same_topk((s, it), oracle_topk(sc, 10, few))
    assert (ints(it)[:, 5:] == -1).all() and np.isnan(s.cpu().numpy()[:, 5:]).all() and (ints(it)[:, :5] >= 0).all()


# ------------------------------------------------------------------ 4. ranks
@pytest.mark.parametrize('d', [4, 8, 16, 32, 64, 128, 256])
@pytest.mark.parametrize('link', [0, 1])
def test_ranks_equal_counting_over_the_weighted_scores(nv, link, d):
    from ultrare_amd import engine
    S, n_item, n_query = 3, 600, 5
    tabs, _, weights, rs = case_inputs(link, d, S, n_item, 8)
    for U, V in tabs:
        V[[70, 300]] = V[7]                                                              # equal scores, told apart by the id
    dev = on_device(tabs)
    users = np.array([5, 0, 3, 7, 3])
    long_row = rs.randint(0, n_item, 4097 if d == 32 else 40)                            # > 4,096 targets: the row counts in global memory
    rows = [rs.permutation(n_item)[:50].tolist() + [7, 70, 300, 7], [], long_row, [4, 9, 9, 250], np.arange(n_item)]
    targets = csr(rows)
    excl = csr([[1, 2, 3], [5], np.unique(rs.randint(0, n_item, 40)), [9, 100], []])
    sc = yardstick(dev, d, users, n_item, weights)
    for ex in (None, excl):
        got = engine.rank_pairs(dev, d, users, targets, ex, weights=weights)
        assert got.dtype == torch.int32 and got.shape == (len(targets[1]),)
        got = ints(got)
        assert np.array_equal(got, ranks_of(sc, targets, ex))
        # every rank r < top_k is position r of recommend under the same weights and exclusion
        items = ints(engine.recommend(dev, d, users, 128, ex, weights=weights)[1])
        row = np.repeat(np.arange(len(users)), np.diff(targets[0]))
        low = (got >= 0) & (got < 128)
        assert low.sum() > 100 and np.array_equal(items[row[low], got[low]], targets[1][low])
    assert got[targets[0][3] + 1] == -1 and got[targets[0][3] + 2] == -1               # item 9 is in its own row's exclusion list
    assert engine.rank_pairs(dev, d, users, csr([[], [], [], [], []]), weights=weights).numel() == 0


# ------------------------------------------------------------------ 5. reproducibility
def test_rows_do_not_depend_on_the_batch_or_the_stream(nv):
    from ultrare_amd import engine
    link, d, S, n_item, n_query = 1, 64, 4, 700, 37
    tabs, users, weights, rs = case_inputs(link, d, S, n_item, n_query)
    dev = on_device(tabs)
    excl = random_excl(rs, n_query, n_item, 0.05)
    targets = csr([rs.randint(0, n_item, 6) for _ in users])
    s, it = engine.recommend(dev, d, users, 10, weights=weights)
    r = engine.rank_pairs(dev, d, users, targets, weights=weights)
    for q in (3, 36):                                                                    # alone: another tile, another grid
        s1, it1 = engine.recommend(dev, d, users[q:q + 1], 10, weights=weights)
        assert np.array_equal(bits(s1[0]), bits(s[q])) and np.array_equal(ints(it1[0]), ints(it[q]))
        t1 = (np.array([0, 6]), targets[1][6 * q:6 * q + 6])
        assert np.array_equal(ints(engine.rank_pairs(dev, d, users[q:q + 1], t1, weights=weights)), ints(r[6 * q:6 * q + 6]))
    s0, it0 = engine.recommend(dev, d, users, 10, excl, weights=weights)
    r0 = engine.rank_pairs(dev, d, users, targets, excl, weights=weights)
    torch.cuda.synchronize()
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            s2, it2 = engine.recommend(dev, d, users, 10, excl, stream=stream, weights=weights)
            r2 = engine.rank_pairs(dev, d, users, targets, excl, stream=stream, weights=weights)
        stream.synchronize()
        assert np.array_equal(bits(s2), bits(s0)) and np.array_equal(ints(it2), ints(it0)) and np.array_equal(ints(r2), ints(r0))


# ------------------------------------------------------------------ 6. the raw ABI on dirty memory inside guard zones
def test_raw_abi_in_guard_zones(nv):
    """Both entries at exactly the sizer's scratch under the three prefills (0x00, 0xFF, 0x5A): guards and inputs intact, every
    output byte written and equal under every prefill, and equal to the engine's clean run."""
    from ultrare_amd import engine
    link, d, S, n_user, n_item, top_k = 1, 16, 3, 12, 1100, 10
    tabs = make_tables(S, d, n_user, n_item, seed=33)
    rs = np.random.RandomState(8)
    users = np.array([4, 0, 11, 7, 4], dtype=np.int32)
    excl = random_excl(rs, len(users), n_item, 0.05)
    targets = csr([rs.randint(0, n_item, 5) for _ in users[:-1]] + [[]])
    W, gou = make_weights(S, 3, link, seed=1), (np.arange(n_user) % 3).astype(np.int32)
    L = nv.lib()
    n, n_t = len(users), len(targets[1])
    dev = on_device(tabs)
    weights = weights_on_device(link, W, gou)
    want_s, want_i = engine.recommend(dev, d, users, top_k, excl, weights=weights)
    want_r = engine.rank_pairs(dev, d, users, targets, excl, weights=weights)

    def arena(outputs, scratch_bytes):
        A = Arena('cuda')
        for m, (U, V) in enumerate(tabs):
            A.input(f'U{m}', U), A.input(f'V{m}', V)
        A.input('users', users), A.input('excl_off', excl[0]), A.input('excl_items', excl[1])
        A.input('tgt_off', targets[0]), A.input('tgt_items', targets[1]), A.input('W', W), A.input('gou', gou)
        for name, nbytes in outputs:
            A.output(name, nbytes)
        A.scratch('ws', scratch_bytes)
        return A

    ptrs = lambda A: [(ctypes.c_void_p * S)(*[A.addr(f'{c}{m}') for m in range(S)]) for c in 'UV']
    need = L.ure_recommend_weighted_scratch(n, n_item, top_k, d, S, link, 3)
    assert need == n * 2 * top_k * 12 == L.ure_recommend_scratch(n, n_item, top_k)     # two splits: the merge runs
    A = arena([('scores', n * top_k * 4), ('items', n * top_k * 4)], need)

    def call_rec(A):
        Up, Vp = ptrs(A)
        nv.check(L.ure_recommend_topk_weighted(Up, Vp, S, A.addr('users'), n, n_item, d, A.addr('excl_off'), A.addr('excl_items'), top_k,
                                               A.addr('scores'), A.addr('items'), A.addr('ws'), A.size('ws'), nv.stream_handle(), link, A.addr('W'), 3,
                                               A.addr('gou'), n_user), 'ure_recommend_topk_weighted')
    reports = run_prefills(A, call_rec, sync=torch.cuda.synchronize)
    assert verdict(reports) == []
    assert np.array_equal(np.frombuffer(reports[0].outputs['scores'], np.int32), bits(want_s).reshape(-1))
    assert np.array_equal(np.frombuffer(reports[0].outputs['items'], np.int32), ints(want_i).reshape(-1))

    need = L.ure_rank_pairs_weighted_scratch(n, n_t, n_item, d, S, link, 3)
    assert need == n_t * 24
    A = arena([('ranks', n_t * 4)], need)

    def call_rank(A):
        Up, Vp = ptrs(A)
        nv.check(L.ure_rank_pairs_weighted(Up, Vp, S, A.addr('users'), n, n_item, d, A.addr('tgt_off'), A.addr('tgt_items'), A.addr('excl_off'),
                                           A.addr('excl_items'), A.addr('ranks'), A.addr('ws'), A.size('ws'), nv.stream_handle(), link, A.addr('W'), 3,
                                           A.addr('gou'), n_user), 'ure_rank_pairs_weighted')
    reports = run_prefills(A, call_rank, sync=torch.cuda.synchronize)
    assert verdict(reports) == []
    assert np.array_equal(np.frombuffer(reports[0].outputs['ranks'], np.int32), ints(want_r))


# ------------------------------------------------------------------ 7. the operators
def test_ops_match_the_engine(nv):
    from ultrare_amd import engine, ops  # noqa: F401
    d, S, n_user, n_item = 16, 3, 20, 150
    dev = on_device(make_tables(S, d, n_user, n_item, seed=2))
    rs = np.random.RandomState(6)
    users = np.arange(0, 20, 2)
    excl = random_excl(rs, len(users), n_item, 0.05)
    targets = csr([rs.randint(0, n_item, 4) for _ in users])
    Us, Vs = [U for U, _ in dev], [V for _, V in dev]
    t = lambda a: torch.from_numpy(np.asarray(a)).cuda()
    for link in (0, 1):
        _, W, gou = weights = weights_on_device(link, make_weights(S, 3, link, seed=3), np.arange(n_user) % 3)
        for ex in (None, excl):
            for g in (gou, None):
                e_off, e_items = (None, None) if ex is None else (t(ex[0]), t(ex[1]))
                s, it = torch.ops.ultrare.recommend_topk_weighted(Us, Vs, t(users), e_off, e_items, 7, link, W, g)
                ws, wi = engine.recommend(dev, d, users, 7, ex, weights=(link, W, g))
                assert np.array_equal(bits(s), bits(ws)) and np.array_equal(ints(it), ints(wi)) and it.dtype == torch.int64
                r = torch.ops.ultrare.rank_pairs_weighted(Us, Vs, t(users), t(targets[0]), t(targets[1]), e_off, e_items, link, W, g)
                assert np.array_equal(ints(r), ints(engine.rank_pairs(dev, d, users, targets, ex, weights=(link, W, g)))) and r.dtype == torch.int32
    # the existing ops and the default route do not see the new argument
    s, it = torch.ops.ultrare.recommend_topk(Us, Vs, t(users), None, None, 7)
    ws, wi = engine.recommend(dev, d, users, 7)
    assert np.array_equal(bits(s), bits(ws)) and np.array_equal(ints(it), ints(wi))


# ------------------------------------------------------------------ 8. Sisa
class Param:
    """The InsParam fields Sisa reads for the 'mf' and 'lightgcn' backbones on the synthetic three-shard set."""

    def __init__(self, epochs):
        import test_gpu_nmf as T
        self.k, self.lam, self.seed, self.batch = 16, 0.1, 42, 200
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = T.SYN_USER, T.SYN_ITEM, False
        self.optimizer, self.gcn_layers = 'sgd', 2


def _train_csr(loaders, n_user, n_item):
    import scipy.sparse as sp
    u = np.concatenate([np.asarray(d.dataset.users, dtype=np.int64) for d in loaders])
    i = np.concatenate([np.asarray(d.dataset.items, dtype=np.int64) for d in loaders])
    return sp.csr_matrix((np.ones(len(u), np.float32), (u, i)), shape=(n_user, n_item))


def _sisa_yardstick(sisa, users, n_item):
    """score_weighted over all pairs under the combiner Sisa holds -> [n, n_item]."""
    from ultrare_amd.method.utils import padded_tables
    tabs = [padded_tables(m) for m in sisa.model_list]
    c = sisa.combiner
    W, gou = c.on_device(tabs[0][0].device, int(tabs[0][0].shape[0]))
    return yardstick([(U, V) for U, V, _ in tabs], tabs[0][2], users, n_item, (c.link_code, W, gou))


@pytest.mark.parametrize('backbone', ['mf', 'lightgcn'])
def test_sisa_recommends_and_ranks_under_its_combiner(nv, backbone):
    import copy
    import test_gpu_nmf as T
    from ultrare_amd import engine
    from ultrare_amd.method import utils
    from ultrare_amd.method.sisa import Sisa
    idx, trd, ted, tot = T.synthetic_loaders()
    sisa = Sisa(Param(3), backbone, 3, idx)
    torch.manual_seed(42)
    ml = sisa.learn(trd, ted, tot, 0, '')
    users = np.arange(T.SYN_USER)
    excl = _train_csr(trd, T.SYN_USER, T.SYN_ITEM)
    with pytest.raises(ValueError, match='no combiner'):
        sisa.recommend(users, 10, excl, combined=True)
    with pytest.raises(ValueError, match='no combiner'):
        sisa.rank_eval(tot, excl, combined=True)
    mean = sisa.recommend(users, 10, excl)
    for link in ('linear', 'logistic'):
        sisa.fit_combiner(trd, link=link, l2=1e-3)
        assert sisa.combiner.W.shape == (3, 4)
        got = sisa.recommend(users, 10, excl, combined=True)
        sc = _sisa_yardstick(sisa, users, T.SYN_ITEM)
        same_topk(got, oracle_topk(sc, 10, engine.exclusion_rows(excl, users)))
        assert (ints(got[1]) != ints(mean[1])).any(axis=1).sum() >= 1                     # per-group weights re-order somebody's catalogue
        q_users, off, items = utils.relevant_pairs(tot, T.SYN_ITEM)
        ex = engine.exclusion_rows(excl, q_users)
        want = utils.rank_metrics(off, ranks_of(sc[q_users], (off, items), ex))
        assert sisa.rank_eval(tot, excl, combined=True) == want
        assert sisa.rank_eval(tot, excl) == utils.rank_eval(sisa.model_list, tot, excl)   # the default is the mean's, as before
        again = sisa.recommend(users, 10, excl)
        assert np.array_equal(bits(again[0]), bits(mean[0])) and np.array_equal(ints(again[1]), ints(mean[1]))
    if backbone == 'mf':
        del_user = idx[1][:5]
        _, trd2, ted2, tot2 = T.synthetic_loaders(del_user)
        s2 = Sisa(Param(3), backbone, 3, idx)
        s2.combiner = sisa.combiner
        torch.manual_seed(42)
        s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, '')
        with pytest.raises(ValueError, match='no combiner'):
            s2.recommend(users, 10, combined=True)
        with pytest.raises(ValueError, match='no combiner'):
            s2.rank_eval(tot2, combined=True)
        s2.fit_combiner(trd2)
        got = s2.recommend(users, 10, combined=True)
        same_topk(got, oracle_topk(_sisa_yardstick(s2, users, T.SYN_ITEM), 10, None))
