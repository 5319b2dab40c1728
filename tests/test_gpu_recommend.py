"""Full-catalogue top-k recommendation (ure_recommend_topk, csrc/mf_recommend.hip) on the MI355X.

The oracle is the existing scoring entry point: ure_score over every (user, item) pair of the query, in model chunks with
first / last as EvalSet.evaluate calls it, then numpy's lexsort with exclusion and padding.  Items and scores must be equal
to the bit; padding is item -1 with a NaN score."""
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


def oracle_topk(P, k, excl=None):
    n_query, n_item = P.shape
    scores = np.full((n_query, k), np.nan, dtype=np.float32)
    items = np.full((n_query, k), -1, dtype=np.int64)
    for q in range(n_query):
        ids = np.arange(n_item)
        if excl is not None:
            ids = np.setdiff1d(ids, excl[1][excl[0][q]:excl[0][q + 1]])
        s = P[q, ids]
        top = ids[np.lexsort((ids, -s))][:k]
        items[q, :len(top)] = top
        scores[q, :len(top)] = P[q, top]
    return scores, items


def assert_same(got, want):
    gs, gi = (t.cpu().numpy() for t in got)
    ws, wi = want
    assert gi.dtype == np.int64 and gs.dtype == np.float32
    np.testing.assert_array_equal(gi, wi)
    pad = wi < 0
    assert np.isnan(gs[pad]).all()
    np.testing.assert_array_equal(gs[~pad].view(np.int32), ws[~pad].view(np.int32))


def random_tables(S, n_user, n_item, d, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return [(torch.randn(n_user, d, device='cuda', generator=g), torch.randn(n_item, d, device='cuda', generator=g)) for _ in range(S)]


def random_csr(n_query, n_item, rate, seed):
    r = np.random.default_rng(seed)
    rows = [np.flatnonzero(r.random(n_item) < rate).astype(np.int32) for _ in range(n_query)]
    off = np.zeros(n_query + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=off[1:])
    return off, np.concatenate(rows).astype(np.int32)


# (d, S, n_item, k, n_query): every d and S of the contract, n_item from 1 to 60,013, k from 1 to 128 and k = n_item
CASES = [
    (4, 1, 1, 1, 1),
    (4, 5, 63, 10, 7),
    (8, 32, 65, 65, 7),
    (16, 33, 3416, 128, 7),
    (32, 5, 3416, 10, 1000),
    (64, 1, 60013, 100, 7),
    (128, 33, 3416, 100, 7),
    (128, 128, 1000, 10, 7),
    (256, 5, 60013, 128, 1),
    (256, 32, 63, 100, 7),
]


@pytest.mark.parametrize('d,S,n_item,k,n_query', CASES)
def test_topk_equals_ure_score_and_lexsort(d, S, n_item, k, n_query):
    n_user = 1200
    tabs = random_tables(S, n_user, n_item, d, seed=d * 1000 + S)
    users = np.random.default_rng(S).integers(0, n_user, n_query)
    excl = random_csr(n_query, n_item, 0.05, seed=k) if n_item > 1 else None
    got = engine.recommend(tabs, d, users, k, excl)
    torch.cuda.synchronize()
    assert_same(got, oracle_topk(oracle_scores(tabs, d, users), k, excl))
    if excl is not None:
        assert_same(engine.recommend(tabs, d, users, k), oracle_topk(oracle_scores(tabs, d, users), k))


def test_constructed_ties_and_special_values():
    d, S, n_item, k = 16, 3, 700, 40
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
    users = np.array([0, 1, 2, 3, 4])
    P = oracle_scores(tabs, d, users)
    assert np.isnan(P[:, 5]).all() and P[1, 6] == np.inf and P[1, 7] == -np.inf
    got = engine.recommend(tabs, d, users, k)
    assert_same(got, oracle_topk(P, k))
    items = got[1].cpu().numpy()
    np.testing.assert_array_equal(items[0], np.setdiff1d(np.arange(k + 3), [5, 6, 7]))   # 0 * NaN, 0 * inf: NaN, last
    assert items[1, 0] == 6 and 7 not in items[1] and 5 not in items[1]
    for q in range(1, 5):                  # equal scores come in ascending id
        pos = [list(items[q]).index(i) for i in (10, 20, 300, 650) if i in items[q]]
        assert pos == sorted(pos)
    # NaN below -inf: with everything but items 5 (NaN) and 7 (-inf for user 1) excluded, -inf comes first
    off = np.array([0, n_item - 2], dtype=np.int64)
    rest = np.setdiff1d(np.arange(n_item), [5, 7]).astype(np.int32)
    s, it = engine.recommend(tabs, d, [1], 3, (off, rest))
    assert it.cpu().tolist() == [[7, 5, -1]]
    assert s[0, 0].item() == -np.inf and np.isnan(s[0, 1:].cpu().numpy()).all()


def test_exclusion_and_padding():
    d, S, n_item, k = 32, 4, 3416, 10
    tabs = random_tables(S, 100, n_item, d, seed=3)
    users = np.array([5, 6, 7, 5])
    keep3 = np.array([17, 1000, 3415])
    rows = [np.arange(0, n_item, 3), np.setdiff1d(np.arange(n_item), keep3), np.arange(n_item), np.zeros(0, dtype=np.int64)]
    off = np.zeros(5, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    excl = (off, np.concatenate(rows).astype(np.int32))
    s, it = engine.recommend(tabs, d, users, k, excl)
    assert_same((s, it), oracle_topk(oracle_scores(tabs, d, users), k, excl))
    it = it.cpu().numpy()
    assert not np.isin(it[0], rows[0]).any()
    assert sorted(it[1, :3]) == sorted(keep3) and (it[1, 3:] == -1).all() and np.isnan(s[1, 3:].cpu().numpy()).all()
    assert (it[2] == -1).all() and np.isnan(s[2].cpu().numpy()).all()


def test_deterministic_and_independent_of_batching():
    d, S, n_item, k = 64, 6, 5000, 50
    tabs = random_tables(S, 3000, n_item, d, seed=11)
    users = np.random.default_rng(1).integers(0, 3000, 1000)
    excl = random_csr(1000, n_item, 0.02, seed=2)
    a = engine.recommend(tabs, d, users, k, excl)
    b = engine.recommend(tabs, d, users, k, excl)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    for q in (0, 1, 499, 999):
        one = engine.recommend(tabs, d, users[q:q + 1], k, (np.array([0, excl[0][q + 1] - excl[0][q]]), excl[1][excl[0][q]:excl[0][q + 1]]))
        assert torch.equal(one[1][0], a[1][q]) and torch.equal(one[0][0].view(torch.int32), a[0][q].view(torch.int32))
    sub = engine.recommend(tabs, d, users[:37], k, (excl[0][:38], excl[1][:excl[0][37]]))
    assert torch.equal(sub[1], a[1][:37]) and torch.equal(sub[0].view(torch.int32), a[0][:37].view(torch.int32))


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
    """The toy training set as a CSR with user ids as rows: read.readSparseMat's matrix, held as float32 (its float16 values
    are refused by some SciPy releases; only the sparsity pattern matters for exclusion)."""
    from scipy.sparse import coo_matrix
    from ultrare_amd.read import _read_csv
    u, i, r = _read_csv(TRAIN)
    return coo_matrix(((r / 5).astype(np.float32), (u, i)), shape=(N_USER, N_ITEM)).tocsr()


def _oracle_models(models, users, k, train):
    from ultrare_amd.method.utils import padded_tables
    tabs = [padded_tables(m) for m in models]
    excl = engine.exclusion_rows(train, users)
    return oracle_topk(oracle_scores([(U, V) for U, V, _ in tabs], tabs[0][2], users), k, excl)


@pytest.mark.parametrize('parallel', [False, True])
def test_sisa_recommend_before_and_after_unlearn(parallel, tmp_path):
    from ultrare_amd.method.sisa import Sisa
    S, E = 3, 2
    train = _train_csr()
    users = np.arange(0, N_USER, 7)
    idx, trd, ted, tot = _sisa_inputs(S)
    sisa = Sisa(Param(E, parallel=parallel), 'mf', S, idx)
    torch.manual_seed(42)
    ml = sisa.learn(trd, ted, tot, 0, str(tmp_path))
    before = sisa.recommend(users, 10, exclude=train)
    assert_same(before, _oracle_models(sisa.model_list, users, 10, train))
    items = before[1].cpu().numpy()
    for q, u in enumerate(users):
        assert not np.isin(items[q], train.indices[train.indptr[u]:train.indptr[u + 1]]).any()

    del_user = [int(idx[0][0]), int(idx[0][1])]
    idx2, trd2, ted2, tot2 = _sisa_inputs(S, del_user)
    s2 = Sisa(Param(E, parallel=parallel), 'mf', S, idx2)
    out = tmp_path / 'un'
    out.mkdir()
    torch.manual_seed(42)
    s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, str(out))
    after = s2.recommend(users, 10, exclude=train)
    assert_same(after, _oracle_models(s2.model_list, users, 10, train))
    assert not torch.equal(after[0].view(torch.int32), before[0].view(torch.int32))


def test_scratch_full_model_recommend(tmp_path):
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.utils import recommend
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, [], [], 1, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], 1, idx)
    train, test = loadData(RatingData(tr[0]), 3000, 24), loadData(RatingData(te[0]), 3000, 24, False)
    torch.manual_seed(42)
    model = Scratch(Param(2), 'mf').train(train, test, [], 0, str(tmp_path))
    csr = _train_csr()
    users = np.array([0, 1, 2, 1507, 700])
    assert_same(recommend([model], users, 20, exclude=csr), _oracle_models([model], users, 20, csr))
    from ultrare_amd.method.utils import padded_tables
    U, V, d = padded_tables(model)
    assert_same(recommend([model], users, 20), oracle_topk(oracle_scores([(U, V)], d, users), 20))


def test_custom_op_matches_engine_and_refuses_cpu():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ultrare_amd import ops  # noqa: F401
    d, S, n_item, k = 32, 3, 900, 12
    tabs = random_tables(S, 60, n_item, d, seed=5)
    users = np.array([3, 1, 4, 1, 5])
    excl = random_csr(len(users), n_item, 0.1, seed=9)
    Us, Vs = [U for U, _ in tabs], [V for _, V in tabs]
    u_dev = torch.from_numpy(users).cuda()
    got = torch.ops.ultrare.recommend_topk(Us, Vs, u_dev, torch.from_numpy(excl[0]).cuda(), torch.from_numpy(excl[1]).cuda(), k)
    want = engine.recommend(tabs, d, users, k, excl)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    got = torch.ops.ultrare.recommend_topk(Us, Vs, u_dev, None, None, k)
    assert_same(got, oracle_topk(oracle_scores(tabs, d, users), k))
    with FakeTensorMode() as mode:
        fs, fi = torch.ops.ultrare.recommend_topk([mode.from_tensor(U) for U in Us], [mode.from_tensor(V) for V in Vs],
                                                  mode.from_tensor(u_dev), None, None, k)
    assert tuple(fs.shape) == (5, k) and fs.dtype == torch.float32 and tuple(fi.shape) == (5, k) and fi.dtype == torch.int64
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.recommend_topk([U.cpu() for U in Us], [V.cpu() for V in Vs], torch.from_numpy(users), None, None, k)
