"""User-by-user distance clusterers on the device (-m gpu): k-medoids and LPA on the reference's own n x n array against
the goldens of tests/golden/make_golden_cluster.py, findNeighbor against the reference's kNN lists for three metrics, the
streamed reductions pinned bit for bit to the same reductions over the device's own materialised distances, Group.grouping
with the new clusterers, and the configs[3] shape with no n x n buffer."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
METRICS = ('euclidean', 'cosine', 'manhattan')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'cluster_toy.npz'))


@pytest.fixture(scope='module')
def toy_D(gold):
    """The given array the goldens were made on.  It is not stored: make_golden_cluster.toy_distances builds it from X in
    float64 (IEEE operations, numpy's fixed pairwise order over d = 16) with one rounding to float32, restated here and
    checked against the digest the generator recorded."""
    X64 = gold['X'].astype(np.float64)
    D = np.empty((len(X64), len(X64)), dtype=np.float32)
    for i in range(0, len(X64), 128):
        D[i:i + 128] = np.sqrt(((X64[i:i + 128, None, :] - X64[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    assert hashlib.sha256(D.tobytes()).hexdigest() == str(gold['D_sha256'])
    return D


def _d64(X, rows, metric):
    """float64 distances of X[rows] to every row of X."""
    X = X.astype(np.float64)
    A = X[np.asarray(rows)]
    if metric == 'euclidean':
        return np.sqrt(((A[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    if metric == 'manhattan':
        return np.abs(A[:, None, :] - X[None, :, :]).sum(-1)
    na, nx = np.linalg.norm(A, axis=1), np.linalg.norm(X, axis=1)
    den = na[:, None] * nx[None, :]
    out = np.where(den == 0, 1.0, 1.0 - (A @ X.T) / np.where(den == 0, 1.0, den))
    out = np.clip(out, 0.0, 2.0)
    out[np.arange(len(rows)), np.asarray(rows)] = 0.0
    return out


def _w64(D_iu, label, k):
    """W[u, g] = sum over i labelled g of float32 exp(-D[i, u]), in float64."""
    E = np.exp(-D_iu).astype(np.float64)
    return np.stack([E[label == g].sum(0) for g in range(k)], axis=1)


# ---- the given array against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize('k', [4, 5])
@pytest.mark.parametrize('balanced', [False, True])
def test_kmedoids_given_matches_reference(gold, toy_D, k, balanced):
    from ultrare_amd import engine
    from ultrare_amd.method import utils as U
    D = toy_D
    n = D.shape[0]
    R = engine.pair_rowsum(D).cpu().numpy()
    assert R.view(np.uint32).tolist() == np.sum(D, axis=1).view(np.uint32).tolist()
    tag = f'km_k{k}_{"bal" if balanced else "plain"}'
    np.random.seed(11)
    for r in range(3):
        label, inertia, medoids = U.singleKmedoids(k, n, D, balanced, 10, return_medoids=True)
        np.testing.assert_array_equal(label, gold[tag + '_labels'][r])
        assert np.float32(inertia) == gold[tag + '_inertia'][r]
        np.testing.assert_array_equal(medoids, gold[tag + '_medoids'][r])
    np.random.seed(11)
    np.testing.assert_array_equal(U.kmedoids(k, n, D, balanced=balanced, n_init=3, max_iter=10), gold[tag + '_label'])


@pytest.mark.parametrize('balanced', [False, True])
def test_lpa_given_matches_reference(gold, toy_D, balanced):
    from ultrare_amd import engine
    from ultrare_amd.method import utils as U
    D = toy_D
    n, k = D.shape[0], 4
    tag = f'lpa_{"bal" if balanced else "plain"}'
    np.random.seed(13)
    for r in range(3):
        label, inertia = U.singleLPA(k, n, D, balanced, 10, max_iter=10)
        want, margin = gold[tag + '_labels'][r], gold[tag + '_margin'][r]
        differ = np.flatnonzero(label != want)
        assert np.all(margin[differ] < 1e-5), (differ[:10], margin[differ][:10])
        W = engine.pair_label_expsum(D, want, k).cpu().numpy()
        ref = _w64(D, want, k)
        assert np.max(np.abs(W - ref) / np.maximum(np.abs(ref), 1e-300)) < 1e-6
        assert abs(inertia - gold[tag + '_inertia'][r]) <= 1e-6 * abs(gold[tag + '_inertia'][r])


@pytest.mark.parametrize('metric', METRICS)
def test_find_neighbor_matches_reference(gold, metric, tmp_path):
    from ultrare_amd.method import utils as U
    from ultrare_amd import engine
    X = gold['X']
    n = X.shape[0]
    idx, val = U.findNeighbor(str(tmp_path) + '/', X, n, var=metric, n_neighbor=10)
    assert os.path.exists(str(tmp_path) + '/' + metric + '.npy')
    g_idx, g_val = gold[f'nn_{metric}_idx'], gold[f'nn_{metric}_val']
    dist = engine.pair_knn(X, 10, metric)[0].cpu().numpy()
    for u in range(n):
        ref = _d64(X, [u], metric)[0]
        np.testing.assert_allclose(dist[u], ref[idx[u]], rtol=1e-5, atol=1e-5)
        assert np.all(np.diff(dist[u]) >= 0)
        for p in np.flatnonzero(idx[u] != g_idx[u]):
            a, b = ref[idx[u, p]], ref[g_idx[u, p]]
            assert abs(a - b) <= 1e-5 * max(abs(a), abs(b), 1e-6), (u, p, a, b)
    # one float16 ulp; near zero the reference's own cosine self-distance is sklearn's rounding noise (about -1e-7), where
    # the kernel writes 0 exactly
    spacing = np.spacing(np.abs(g_val).astype(np.float16)).astype(np.float32)
    assert np.all(np.abs(val.astype(np.float32) - g_val.astype(np.float32)) <= spacing + 1e-6)


# ---- the streamed path pinned to the given path --------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 2071, 1), (63, 7, 10), (63, 128, 10), (1000, 32, 128), (1000, 2071, 10), (4099, 1, 10), (4099, 128, 128)]


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    if n > 4:                                     # duplicated rows: exact ties of whole lists
        X[n // 2:n // 2 + n // 8 + 1] = X[:n // 8 + 1]
    if n > 2:
        X[1] = 0.0                                # a zero row (cosine distance 1 to everything)
    return X


@pytest.mark.parametrize('n,d,n_nb', SHAPES)
@pytest.mark.parametrize('metric', METRICS)
def test_streamed_equals_given_on_own_distances(n, d, n_nb, metric):
    from ultrare_amd import engine
    X = _data(n, d, n * 7 + d)
    Xd = torch.from_numpy(X).cuda()
    G = engine.pair_cols(Xd, np.arange(n), metric)
    Gh = G.cpu().numpy()
    assert np.array_equal(Gh.view(np.uint32), np.ascontiguousarray(Gh.T).view(np.uint32))
    assert np.all(np.diag(Gh).view(np.uint32) == 0)
    ref = _d64(X, np.arange(n), metric) if n * n * d <= 1 << 26 else None
    if ref is not None:
        np.testing.assert_allclose(Gh, ref, rtol=1e-4, atol=1e-4)
    # kNN: streamed == given == numpy lexsort of the device's own distances; batching and splits change nothing
    dist, idx = engine.pair_knn(Xd, n_nb, metric)
    gd, gi = engine.pair_knn(G, n_nb, None)
    assert torch.equal(dist, gd) and torch.equal(idx, gi)
    order = np.lexsort((np.broadcast_to(np.arange(n), Gh.shape), Gh), axis=1)[:, :n_nb]
    np.testing.assert_array_equal(idx.cpu().numpy(), order)
    np.testing.assert_array_equal(dist.cpu().numpy(), np.take_along_axis(Gh, order, axis=1))
    perm = np.random.default_rng(n).permutation(n)
    half = max(1, n // 2)
    for splits in (1, 3):
        parts = [engine.pair_knn(Xd, n_nb, metric, query=q, splits=splits) for q in (perm[:half], perm[half:]) if len(q)]
        bd = torch.cat([p[0] for p in parts])
        bi = torch.cat([p[1] for p in parts])
        assert torch.equal(bd, dist[torch.from_numpy(perm).cuda()]) and torch.equal(bi, idx[torch.from_numpy(perm).cuda()])
    from ultrare_amd import ops  # noqa: F401  (registers torch.ops.ultrare)
    od, oi = torch.ops.ultrare.pair_knn(Xd, None, n_nb, metric)
    assert torch.equal(od, dist) and torch.equal(oi, idx)
    # row sums: streamed == given == np.sum(D, axis=1)
    R = engine.pair_rowsum(Xd, metric).cpu().numpy()
    assert np.array_equal(R.view(np.uint32), engine.pair_rowsum(G).cpu().numpy().view(np.uint32))
    assert np.array_equal(R.view(np.uint32), np.sum(Gh, axis=1).view(np.uint32))
    # columns
    cols = np.random.default_rng(d).integers(0, n, size=min(n, 70))
    C = engine.pair_cols(Xd, cols, metric).cpu().numpy()
    assert np.array_equal(C.view(np.uint32), Gh[:, cols].view(np.uint32))
    assert np.array_equal(C.view(np.uint32), engine.pair_cols(G, cols).cpu().numpy().view(np.uint32))
    # label-grouped exp sums
    k = 5 if n > 1 else 1
    label = np.random.default_rng(n + d).integers(0, k, size=n)
    W = engine.pair_label_expsum(Xd, label, k, metric).cpu().numpy()
    assert np.array_equal(W.view(np.uint64), engine.pair_label_expsum(G, label, k).cpu().numpy().view(np.uint64))
    # (1e-6 relative; terms below float32's normal range -- exp(-D) for D > 87, e.g. manhattan at d = 128 -- may differ
    # between numpy's exp and the device's, hence the absolute floor of one smallest normal per term)
    ref_w = _w64(Gh, label, k)
    assert np.all(np.abs(W - ref_w) <= 1e-6 * np.abs(ref_w) + n * np.finfo(np.float32).tiny)


# ---- row sums past one numpy buffer ---------------------------------------------------------------------------------
# np.sum(A, axis=1) sums a row in buffers of 8192 values; above that the kernel switches to the last buffer's leaf table and
# adds the buffer sums in order.  8193: a last buffer of one value; 8261: of 69 (one leaf, a tail of 5); 16391: two full
# buffers and 7 values (a leaf below one group of 8); 20000: two full buffers and 3616 values (a tree of its own).
ROWSUM_NS = [8193, 8261, 16391, 20000]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('n', ROWSUM_NS)
@pytest.mark.parametrize('metric', METRICS)
def test_rowsum_beyond_one_buffer_equals_numpy(n, metric):
    """256 rows of D -- the first 64, the last 70 (the ragged tile) and 122 random ones -- fetched as columns (D is symmetric bit
    for bit: test_streamed_equals_given_on_own_distances) and summed by numpy against the streamed row sums."""
    from ultrare_amd import engine
    X = _data(n, 3, n)
    Xd = torch.from_numpy(X).cuda()
    R = engine.pair_rowsum(Xd, metric).cpu().numpy()
    rows = np.concatenate([np.arange(64), np.arange(n - 70, n), np.random.default_rng(n).choice(np.arange(64, n - 70), 122, replace=False)])
    Dt = np.ascontiguousarray(engine.pair_cols(Xd, rows, metric).cpu().numpy().T)
    assert Dt.shape == (256, n) and Dt.flags['C_CONTIGUOUS']
    want = np.sum(Dt, axis=1)
    print(f'n={n} {metric}: {int((_bits(R[rows]) != _bits(want)).sum())} of 256 row sums differ from numpy')
    assert np.array_equal(_bits(R[rows]), _bits(want))


def test_rowsum_beyond_one_buffer_given_source():
    """Once, the whole 8261 x 8261 array (273 MB): the given source takes the same walk as the streamed one, and numpy agrees
    on every row."""
    from ultrare_amd import engine
    n = 8261
    Xd = torch.from_numpy(_data(n, 3, n)).cuda()
    G = engine.pair_cols(Xd, np.arange(n), 'euclidean')
    R = engine.pair_rowsum(Xd, 'euclidean').cpu().numpy()
    assert np.array_equal(_bits(engine.pair_rowsum(G).cpu().numpy()), _bits(R))
    assert np.array_equal(_bits(np.sum(G.cpu().numpy(), axis=1)), _bits(R))


# ---- exp-sums at the limit of k ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [77, 128])
@pytest.mark.parametrize('metric', METRICS)
def test_label_expsum_at_the_group_limit(k, metric):
    """k = 77 is the first whose dynamic LDS (the tile + k x 64 doubles) passes 64 KiB, 128 is the limit; some groups have
    no member."""
    from ultrare_amd import engine
    n, d = 300, 10
    X = _data(n, d, n * 7 + d)
    Xd = torch.from_numpy(X).cuda()
    label = np.random.default_rng(k).integers(0, k, size=n)
    label[label % 5 == 3] = 0                                  # every fifth group stays empty
    label[label == k - 1] = 1                                  # and the last one
    empty = np.setdiff1d(np.arange(k), label)
    assert len(empty) >= k // 5 and k - 1 in empty and len(np.unique(label)) > k // 2
    G = engine.pair_cols(Xd, np.arange(n), metric)
    Gh = G.cpu().numpy()
    W = engine.pair_label_expsum(Xd, label, k, metric).cpu().numpy()
    assert W.shape == (n, k) and W.dtype == np.float64
    assert np.array_equal(W.view(np.uint64), engine.pair_label_expsum(G, label, k).cpu().numpy().view(np.uint64))
    ref_w = _w64(Gh, label, k)
    assert np.all(np.abs(W - ref_w) <= 1e-6 * np.abs(ref_w) + n * np.finfo(np.float32).tiny)
    assert not W[:, empty].any() and W[:, np.unique(label)].all()


# ---- kNN at the split limit -----------------------------------------------------------------------------------------------
def test_knn_at_the_split_limit_and_given_with_query():
    """n = 4090 is 64 column tiles, the last one ragged: splits = 64 gives every tile a workgroup of its own (fewer columns
    than n_nb = 128 in each), splits = 1000 is clamped to 64.  Both sources, 70 query rows with repeats: every call returns
    the bytes of splits = 1, which are the lexsort of the device's own distances."""
    from ultrare_amd import engine
    n, d, n_nb = 4090, 10, 128
    Xd = torch.from_numpy(_data(n, d, n * 7 + d)).cuda()
    query = np.random.default_rng(3).integers(0, n, size=64)
    query = np.concatenate([query, query[:5], [n - 1]])
    assert len(query) == 70 and len(np.unique(query)) < 70
    Dq = np.ascontiguousarray(engine.pair_cols(Xd, query, 'euclidean').cpu().numpy().T)        # rows `query` of D (symmetric)
    G = engine.pair_cols(Xd, np.arange(n), 'euclidean')
    assert np.array_equal(_bits(G[torch.from_numpy(query).cuda()].cpu().numpy()), _bits(Dq))
    dist, idx = engine.pair_knn(Xd, n_nb, 'euclidean', query=query, splits=1)
    for src, met in ((Xd, 'euclidean'), (G, None)):
        for splits in (1, 64, 1000):
            d2, i2 = engine.pair_knn(src, n_nb, met, query=query, splits=splits)
            assert torch.equal(d2.view(torch.int32), dist.view(torch.int32)) and torch.equal(i2, idx), (met, splits)
    order = np.lexsort((np.broadcast_to(np.arange(n), Dq.shape), Dq), axis=1)[:, :n_nb]
    np.testing.assert_array_equal(idx.cpu().numpy(), order)
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(np.take_along_axis(Dq, order, axis=1)))


# ---- Group.grouping ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('var', ['emb-bkmedoids', 'emb-blpa'])
def test_group_grouping_new_clusterers(gold, var, tmp_path):
    from ultrare_amd.group import Group
    X = gold['X']
    n, k = X.shape[0], 4
    np.random.seed(3)
    res = Group(None, 'toy', user_mat=X).grouping('toy', k, var, verbose=False, data_dir=str(tmp_path))
    assert sorted(i for g in res for i in g) == list(range(n))
    assert max(len(g) for g in res) <= int(np.ceil(n / k))
    path = os.path.join(str(tmp_path), 'toy', 'val', var + str(k) + '.npy')
    assert os.path.exists(path)
    again = Group(None, 'toy', user_mat=X).grouping('toy', k, var, verbose=False, data_dir=str(tmp_path))
    assert again == res


# ---- the configs[3] shape: no n x n buffer --------------------------------------------------------------------------
def test_scale_162k_no_dense_matrix():
    from ultrare_amd import engine
    n, d = 162000, 128
    X = np.random.default_rng(5).standard_normal((n, d)).astype(np.float32)
    Xd = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    dist, idx = engine.pair_knn(Xd, 10, 'euclidean')
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 1 << 30
    rows = np.random.default_rng(6).choice(n, 64, replace=False)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    for r in rows:
        ref = np.sqrt(((X[r].astype(np.float64) - X.astype(np.float64)) ** 2).sum(1))
        want = np.sort(ref)[:10]
        np.testing.assert_allclose(dist[r], want, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(ref[idx[r]], want, rtol=1e-5, atol=1e-5)
        assert idx[r, 0] == r
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    label = np.random.default_rng(7).integers(0, 8, size=n)
    W = engine.pair_label_expsum(Xd, label, 8, 'euclidean')
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 1 << 30
    W = W.cpu().numpy()
    for r in rows[:4]:
        ref = np.sqrt(((X[r].astype(np.float64) - X.astype(np.float64)) ** 2).sum(1)).astype(np.float32)
        want = np.bincount(label, weights=np.exp(-ref).astype(np.float64), minlength=8)
        assert np.max(np.abs(W[r] - want) / want) < 1e-5
