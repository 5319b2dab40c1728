"""Exact full-catalogue ranks (ure_rank_pairs, csrc/mf_rank.hip) on the MI355X.

The oracle is the existing scoring entry point: ure_score over the query rows' full [n_query, n_item] score matrix, in model
chunks with first / last as EvalSet.evaluate calls it, then numpy counts the eligible items whose (score, id) key beats each
target's.  Ranks must be equal as integers; an excluded target is -1."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from ultrare_amd import _native as nv
from ultrare_amd import engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071
LDS_TARGETS = 4096          # kRankLdsTargets of csrc/mf_rank.hip


def oracle_scores(tables, d, users):
    """[n_query, n_item] scores exactly as ure_score writes them for the ensemble `tables`."""
    users = np.asarray(users, dtype=np.int64)
    n_item, S = tables[0][1].shape[0], len(tables)
    dev = tables[0][0].device
    uid = torch.from_numpy(np.repeat(users, n_item).astype(np.int32)).to(dev)
    iid = torch.from_numpy(np.tile(np.arange(n_item, dtype=np.int32), len(users))).to(dev)
    pred = torch.empty(uid.numel(), dtype=torch.float32, device=dev)
    for c0 in range(0, S, nv.MAX_MODELS_PER_CALL):
        chunk = tables[c0:c0 + nv.MAX_MODELS_PER_CALL]
        Up = (ctypes.c_void_p * len(chunk))(*[U.data_ptr() for U, _ in chunk])
        Vp = (ctypes.c_void_p * len(chunk))(*[V.data_ptr() for _, V in chunk])
        nv.check(nv.lib().ure_score(Up, Vp, len(chunk), S, int(c0 == 0), int(c0 + len(chunk) >= S), nv.ptr(uid), nv.ptr(iid), None,
                                    uid.numel(), d, nv.ptr(pred), None, nv.stream_handle()), 'ure_score')
    return pred.cpu().numpy().reshape(len(users), n_item)


def keys(s, ids):
    """rec_key of csrc/rec_score.h in numpy: order bits of the score (NaN lowest, -0.0 == +0.0) above ~id."""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).copy()
    b[(b << np.uint32(1)) == 0] = 0
    b = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    b[np.isnan(s)] = 0
    return (b.astype(np.uint64) << np.uint64(32)) | (~np.asarray(ids, dtype=np.uint32)).astype(np.uint64)


def oracle_ranks(P, targets, excl=None):
    off, items = targets
    n_item = P.shape[1]
    out = np.empty(len(items), dtype=np.int64)
    for q in range(P.shape[0]):
        ids = np.arange(n_item)
        ex = excl[1][excl[0][q]:excl[0][q + 1]] if excl is not None else np.zeros(0, dtype=np.int64)
        ids = np.setdiff1d(ids, ex)
        ek = np.sort(keys(P[q, ids], ids))
        t = items[off[q]:off[q + 1]]
        tk = keys(P[q, t], t)
        r = len(ek) - np.searchsorted(ek, tk, side='right')
        r[np.isin(t, ex)] = -1
        out[off[q]:off[q + 1]] = r
    return out


def random_tables(S, n_user, n_item, d, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return [(torch.randn(n_user, d, device='cuda', generator=g), torch.randn(n_item, d, device='cuda', generator=g)) for _ in range(S)]


def rows(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return off, (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int32)


def random_csr(n_query, n_item, rate, seed):
    r = np.random.default_rng(seed)
    return rows([np.flatnonzero(r.random(n_item) < rate) for _ in range(n_query)])


def random_targets(n_query, n_item, mean, seed, excl=None):
    """Unsorted targets with duplicates, empty rows and (when excl is given) some excluded items."""
    r = np.random.default_rng(seed)
    out = []
    for q in range(n_query):
        n = 0 if q % 5 == 3 else int(r.integers(1, 2 * mean + 1))
        t = r.integers(0, n_item, n)
        if n > 2:
            t[-1] = t[0]                                 # a duplicate
        if excl is not None and excl[0][q + 1] > excl[0][q] and n > 0:
            t[0] = excl[1][excl[0][q]]                   # an excluded target
        out.append(t)
    return rows(out)


def ranks_of(tabs, d, users, targets, excl=None):
    got = engine.rank_pairs(tabs, d, users, targets, excl)
    assert got.dtype == torch.int32 and got.is_cuda and got.numel() == len(targets[1])
    return got.cpu().numpy().astype(np.int64)


# (d, S, n_item, n_query): every d and S of the contract, n_item from 1 to 60,013
CASES = [
    (4, 1, 1, 3),
    (4, 5, 63, 7),
    (8, 33, 65, 9),
    (16, 5, 3416, 40),
    (32, 5, 3416, 300),
    (64, 1, 60013, 5),
    (128, 33, 3416, 7),
    (128, 128, 1000, 7),
    (256, 5, 60013, 2),
    (256, 1, 700, 9),
]


@pytest.mark.parametrize('d,S,n_item,n_query', CASES)
def test_ranks_equal_ure_score_and_numpy(d, S, n_item, n_query):
    tabs = random_tables(S, 1200, n_item, d, seed=d * 1000 + S)
    users = np.random.default_rng(S).integers(0, 1200, n_query)
    P = oracle_scores(tabs, d, users)
    excl = random_csr(n_query, n_item, 0.05, seed=d) if n_item > 1 else None
    tg = random_targets(n_query, n_item, 20, seed=n_item, excl=excl)
    got = ranks_of(tabs, d, users, tg, excl)
    np.testing.assert_array_equal(got, oracle_ranks(P, tg, excl))
    if excl is not None:
        assert (got == -1).any()
    np.testing.assert_array_equal(ranks_of(tabs, d, users, tg), oracle_ranks(P, tg))


def test_independent_of_batching_and_reproducible():
    d, S, n_item = 32, 6, 5000
    tabs = random_tables(S, 3000, n_item, d, seed=11)
    users = np.random.default_rng(1).integers(0, 3000, 200)
    excl = random_csr(200, n_item, 0.02, seed=2)
    tg = random_targets(200, n_item, 30, seed=3, excl=excl)
    a = ranks_of(tabs, d, users, tg, excl)
    np.testing.assert_array_equal(a, ranks_of(tabs, d, users, tg, excl))
    for q in range(200):
        one_t = (np.array([0, tg[0][q + 1] - tg[0][q]]), tg[1][tg[0][q]:tg[0][q + 1]])
        one_e = (np.array([0, excl[0][q + 1] - excl[0][q]]), excl[1][excl[0][q]:excl[0][q + 1]])
        if len(one_t[1]) == 0:
            assert engine.rank_pairs(tabs, d, users[q:q + 1], one_t, one_e).numel() == 0
            continue
        np.testing.assert_array_equal(ranks_of(tabs, d, users[q:q + 1], one_t, one_e), a[tg[0][q]:tg[0][q + 1]])
    np.testing.assert_array_equal(a, oracle_ranks(oracle_scores(tabs, d, users), tg, excl))


def test_ties_and_special_values():
    d, S, n_item = 16, 3, 700
    tabs = random_tables(S, 50, n_item, d, seed=7)
    for U, V in tabs:
        V[10] = V[300]
        V[20] = V[300]
        V[650] = V[300]
        V[5] = float('nan')
        V[6, 0], V[7, 0] = float('inf'), float('-inf')
        U[0] = 0.0                         # user 0: every finite score +-0: the order is the ids'
        U[1, 0] = 1.0
        U[2, 0] = -1.0
    zeros = [(torch.zeros(50, d, device='cuda'), torch.zeros(n_item, d, device='cuda'))]
    users = np.array([0, 1, 2, 3, 4])
    P = oracle_scores(tabs, d, users)
    assert np.isnan(P[:, 5]).all() and P[1, 6] == np.inf and P[1, 7] == -np.inf
    pick = np.array([5, 6, 7, 10, 20, 300, 650, 0, 699, 300])
    tg = rows([pick] * 5)
    got = ranks_of(tabs, d, users, tg)
    np.testing.assert_array_equal(got, oracle_ranks(P, tg))
    r0 = got[:len(pick)]
    np.testing.assert_array_equal(r0[[3, 4, 5, 6, 7, 8]], [7, 17, 297, 647, 0, 696])    # user 0: ids in order, NaN (5, 6, 7) last
    assert r0[5] == r0[9]
    r1 = got[len(pick):2 * len(pick)]
    assert r1[1] == 0 and r1[0] == n_item - 1 and r1[2] == n_item - 2                   # +inf first, NaN below -inf
    assert list(r1[[3, 4, 5, 6]]) == sorted(r1[[3, 4, 5, 6]])                           # equal scores by ascending id
    zt = rows([np.arange(n_item)[::-1]])
    np.testing.assert_array_equal(ranks_of(zeros, d, [3], zt), np.arange(n_item)[::-1])


def test_whole_catalogue_user_is_the_lexsort_permutation():
    d, S, n_item = 64, 4, 6000
    tabs = random_tables(S, 100, n_item, d, seed=21)
    users = np.array([42])
    P = oracle_scores(tabs, d, users)[0]
    perm = np.random.default_rng(0).permutation(n_item)
    got = ranks_of(tabs, d, users, rows([perm]))
    order = np.lexsort((np.arange(n_item), -P))          # (score descending, id ascending); finite scores here
    want = np.empty(n_item, dtype=np.int64)
    want[order] = np.arange(n_item)
    np.testing.assert_array_equal(got, want[perm])


def test_rows_beyond_the_lds_budget():
    """A tile whose rows do not all fit the workgroup's LDS: heavy rows search and count in global memory."""
    d, S, n_item = 32, 3, 9000
    tabs = random_tables(S, 400, n_item, d, seed=31)
    users = np.arange(0, 400, 10)
    r = np.random.default_rng(5)
    lists = [r.integers(0, n_item, 30) for _ in users]
    lists[1] = r.integers(0, n_item, LDS_TARGETS + 500)          # more targets than one workgroup's LDS holds
    lists[2] = r.permutation(n_item)[:3000]                       # fits beside the light rows
    lists[7] = np.arange(n_item)
    tg = rows(lists)
    excl = random_csr(len(users), n_item, 0.03, seed=6)
    P = oracle_scores(tabs, d, users)
    np.testing.assert_array_equal(ranks_of(tabs, d, users, tg, excl), oracle_ranks(P, tg, excl))
    np.testing.assert_array_equal(ranks_of(tabs, d, users, tg), oracle_ranks(P, tg))


def test_ranks_agree_with_recommend_topk():
    d, S, n_item, k = 32, 5, 3416, 50
    tabs = random_tables(S, 1000, n_item, d, seed=41)
    users = np.random.default_rng(2).integers(0, 1000, 120)
    excl = random_csr(len(users), n_item, 0.05, seed=4)
    tg = random_targets(len(users), n_item, 200, seed=8, excl=excl)
    ranks = ranks_of(tabs, d, users, tg, excl)
    _, items = engine.recommend(tabs, d, users, k, excl)
    items = items.cpu().numpy()
    hits = 0
    for q in range(len(users)):
        t, rq = tg[1][tg[0][q]:tg[0][q + 1]], ranks[tg[0][q]:tg[0][q + 1]]
        for ti, ri in zip(t, rq):
            if 0 <= ri < k:
                assert items[q, ri] == ti
        top = np.intersect1d(items[q], t)
        assert len(np.unique(t[(rq >= 0) & (rq < k)])) == len(top)
        hits += len(top)
    assert hits > 0


class Param:
    def __init__(self, epochs, k=16, batch=3000, parallel=False):
        self.k, self.lam, self.seed, self.batch = k, 0.1, 42, batch
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, parallel


def _sisa_inputs(S, del_user=()):
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, list(del_user), [], S, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], S, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    tot = loadData(RatingData(np.hstack(te)), 3000, 24, False)
    return idx, trd, ted, tot


def _train_csr():
    """The toy training set as a CSR with user ids as rows (float32 values: only the pattern matters for exclusion)."""
    from scipy.sparse import coo_matrix
    from ultrare_amd.read import _read_csv
    u, i, r = _read_csv(TRAIN)
    return coo_matrix(((r / 5).astype(np.float32), (u, i)), shape=(N_USER, N_ITEM)).tocsr()


def _numpy_metrics(off, ranks, ks):
    out = {f'{m}@{K}': [] for K in ks for m in ('hr', 'recall', 'ndcg')}
    out['mrr'] = []
    n_pairs = 0
    for q in range(len(off) - 1):
        r = ranks[off[q]:off[q + 1]]
        r = r[r >= 0]
        if r.size == 0:
            continue
        n_pairs += r.size
        for K in ks:
            out[f'hr@{K}'].append(float(r.min() < K))
            out[f'recall@{K}'].append(np.sum(r < K) / r.size)
            out[f'ndcg@{K}'].append(np.sum(1 / np.log2(r[r < K] + 2.0)) / np.sum(1 / np.log2(np.arange(min(r.size, K)) + 2.0)))
        out['mrr'].append(1 / (1 + r.min()))
    res = {k: float(np.mean(v)) for k, v in out.items()}
    res.update(n_users=len(out['mrr']), n_pairs=n_pairs)
    return res


def _oracle_eval(models, test_loader, train, ks):
    from ultrare_amd.method.utils import padded_tables, relevant_pairs
    tabs = [padded_tables(m) for m in models]
    users, off, items = relevant_pairs(test_loader, N_ITEM)
    excl = engine.exclusion_rows(train, users) if train is not None else None
    ranks = oracle_ranks(oracle_scores([(U, V) for U, V, _ in tabs], tabs[0][2], users), (off, items), excl)
    return _numpy_metrics(off, ranks, ks)


def _assert_metrics(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])


def test_rank_eval_on_the_toy_split(tmp_path):
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.utils import rank_eval, relevant_pairs
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, [], [], 1, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], 1, idx)
    train, test = loadData(RatingData(tr[0]), 3000, 24), loadData(RatingData(te[0]), 3000, 24, False)
    users, off, items = relevant_pairs(test, N_ITEM)
    assert off[-1] == 7133
    torch.manual_seed(42)
    model = Scratch(Param(2), 'mf').train(train, test, [], 0, str(tmp_path))
    csr = _train_csr()
    got = rank_eval([model], test, exclude=csr, ks=(1, 10, 20, 100))
    want = _oracle_eval([model], test, csr, (1, 10, 20, 100))
    _assert_metrics(got, want)
    assert got['n_pairs'] == 7133 and got['n_users'] == len(users)        # disjoint from training: no test pair excluded
    assert 0 < got['hr@100'] <= 1 and got['hr@10'] <= got['hr@20'] and got['recall@10'] <= got['recall@20']
    _assert_metrics(rank_eval([model], test), _oracle_eval([model], test, None, (10, 20)))


@pytest.mark.parametrize('parallel', [False, True])
def test_sisa_rank_eval_before_and_after_unlearn(parallel, tmp_path):
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import padded_tables
    S, E = 3, 2
    train = _train_csr()
    idx, trd, ted, tot = _sisa_inputs(S)
    sisa = Sisa(Param(E, parallel=parallel), 'mf', S, idx)
    torch.manual_seed(42)
    ml = sisa.learn(trd, ted, tot, 0, str(tmp_path))
    before = sisa.rank_eval(tot, exclude=train)
    _assert_metrics(before, _oracle_eval(sisa.model_list, tot, train, (10, 20)))

    del_user = [int(idx[0][0]), int(idx[0][1]), int(idx[1][0])]
    idx2, trd2, ted2, tot2 = _sisa_inputs(S, del_user)
    s2 = Sisa(Param(E, parallel=parallel), 'mf', S, idx2)
    out = tmp_path / 'un'
    out.mkdir()
    torch.manual_seed(42)
    s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, str(out))
    after = s2.rank_eval(tot2, exclude=train)
    _assert_metrics(after, _oracle_eval(s2.model_list, tot2, train, (10, 20)))
    assert after != before

    # forgetting check: the deleted users' former training pairs, ranked by the unlearned ensemble
    forgot = rows([train.indices[train.indptr[u]:train.indptr[u + 1]] for u in del_user])
    tabs = [padded_tables(m) for m in s2.model_list]
    tables, d = [(U, V) for U, V, _ in tabs], tabs[0][2]
    got = ranks_of(tables, d, del_user, forgot)
    np.testing.assert_array_equal(got, oracle_ranks(oracle_scores(tables, d, del_user), forgot))
    assert got.min() >= 0 and len(got) > 0


def test_custom_op_matches_engine_and_refuses_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ultrare_amd import ops  # noqa: F401
    d, S, n_item = 32, 3, 900
    tabs = random_tables(S, 60, n_item, d, seed=5)
    users = np.array([3, 1, 4, 1, 5])
    excl = random_csr(len(users), n_item, 0.1, seed=9)
    tg = random_targets(len(users), n_item, 40, seed=10, excl=excl)
    Us, Vs = [U for U, _ in tabs], [V for _, V in tabs]
    dev = [torch.from_numpy(x).cuda() for x in (users, tg[0], tg[1], excl[0], excl[1])]
    got = torch.ops.ultrare.rank_pairs(Us, Vs, *dev)
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), ranks_of(tabs, d, users, tg, excl))
    got = torch.ops.ultrare.rank_pairs(Us, Vs, *dev[:3], None, None)
    np.testing.assert_array_equal(got.cpu().numpy(), oracle_ranks(oracle_scores(tabs, d, users), tg))
    with FakeTensorMode() as mode:
        f = torch.ops.ultrare.rank_pairs([mode.from_tensor(U) for U in Us], [mode.from_tensor(V) for V in Vs],
                                         *[mode.from_tensor(t) for t in dev[:3]], None, None)
    assert tuple(f.shape) == (len(tg[1]),) and f.dtype == torch.int32
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.rank_pairs([U.cpu() for U in Us], [V.cpu() for V in Vs], *[t.cpu() for t in dev[:3]], None, None)
