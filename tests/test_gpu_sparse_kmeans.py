"""k-means / balanced k-means on the sparse rating matrix, device side: ure_csr_kmeans_cost and ure_csr_kmeans_centroids
against the numpy contract (ultrare_amd/sparse_kmeans.py) BIT FOR BIT, ure_balanced_fill against ure_host_kmeans_assign of
the same library label for label -- at the lane-group and chunk boundaries, on long rows and columns, on tied, signed-zero
and NaN keys; order and company; whole singleKmeans runs against the dense route; the Group.grouping and command-line
surface; no dense array; the torch ops.  The fill's round counts are recorded (ROUNDS, printed), never bounded by k."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, 'tests', 'golden', 'toy', '0_train.csv')
N_USER, N_ITEM = 1508, 2071
# a single lane, one lane group narrower than a wavefront (2, 5, 16), one below / at / above a full wavefront (63, 64, 65:
# the second chunk of 64 holds one centroid) and the limit
KS = [1, 2, 5, 16, 63, 64, 65, 256]
ROUNDS = {}                                               # (what, n, k, capacity) -> rounds of the fill, for the record


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def crafted():
    """203 users x 97 items at density 0.1, values on the float16 grid of the ratings: rows 0 and 202 empty, row 2 full,
    25 explicit stored zeros."""
    from scipy import sparse
    from ultrare_amd import sparse_group as sg
    rs = np.random.RandomState(5)
    mat = sparse.random(203, 97, density=0.1, random_state=rs, format='coo', dtype=np.float32)
    keep = (mat.row != 0) & (mat.row != 202) & (mat.row != 2)
    rows = np.concatenate([mat.row[keep], np.full(97, 2)])
    cols = np.concatenate([mat.col[keep], np.arange(97)])
    vals = (rs.randint(1, 11, len(rows)) / 10.0).astype(np.float16).astype(np.float32)
    vals[rs.choice(len(vals), 25, replace=False)] = 0.0
    halves = sg.canonical_csr(sparse.coo_matrix((vals, (rows, cols)), shape=(203, 97)))
    lens = np.diff(halves[0].off)
    assert lens[0] == 0 == lens[202] and lens[2] == 97 and (halves[0].val == 0).sum() == 25
    return halves


@pytest.fixture(scope='module')
def small():
    from ultrare_amd import engine
    halves = crafted()
    return halves, engine.CsrSet(halves)


@pytest.fixture(scope='module')
def toy():
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    from ultrare_amd.read import readSparseMat
    mat = readSparseMat(TRAIN, N_USER, N_ITEM)
    halves = sg.canonical_csr(mat)
    return mat, halves, engine.CsrSet(halves)


def centroids_for(halves, k, seed):
    """k float32 centroids: sampled rows while there are enough of them, random values beyond."""
    from ultrare_amd import sparse_group as sg
    rs = np.random.RandomState(seed)
    n, n_item = halves[0].shape
    C = rs.standard_normal((k, n_item)).astype(np.float32)
    m = min(k, n) // 2
    C[:m] = sg.dense_rows(halves[0], rs.choice(n, m, replace=False))
    return C


def transposed(C):
    return torch.from_numpy(np.ascontiguousarray(C.T)).cuda()


def labels_for(n, k, seed):
    """Random labels; for k >= 3 cluster k - 1 has exactly one member (user 7) and cluster k - 2 none."""
    lab = np.random.RandomState(seed).randint(0, max(k - 2, 1), n)
    if k >= 3:
        lab[7] = k - 1
    return lab


# ---- 1. cost, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_cost_equals_the_contract_bit_for_bit(small, k):
    from ultrare_amd import engine
    from ultrare_amd import sparse_kmeans as sk
    halves, S = small
    C = centroids_for(halves, k, seed=k)
    got = engine.csr_kmeans_cost(S, transposed(C), k)
    assert got.shape == (203, k) and got.dtype == torch.float32
    assert np.array_equal(bits(got), bits(sk.kmeans_cost_csr_ref(halves[0], C))), k


@pytest.mark.parametrize('k', [4, 5])
def test_cost_on_the_toy_ratings_bit_for_bit(toy, k):
    from oracle import cpu_ref as O
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    from ultrare_amd import sparse_kmeans as sk
    mat, halves, S = toy
    C = sg.dense_rows(halves[0], np.random.RandomState(k).choice(N_USER, k, replace=False))
    got = engine.csr_kmeans_cost(S, transposed(C), k)
    assert np.array_equal(bits(got), bits(sk.kmeans_cost_csr_ref(halves[0], C)))
    assert np.array_equal(bits(got), bits(O.kmeans_dist(np.asarray(mat.todense(), dtype=np.float32), C)))      # and the dense oracle's


def test_cost_on_a_5000_entry_row_bit_for_bit():
    """9 users x 6,000 items: user 4 rated 5,000 of them (78 full tiles of 64 and a tail), the others 30 each; 6,000 items are
    one tile of the squared-norm pass and a half at k = 3 (4,095 floats a tile), many at k = 65."""
    from scipy import sparse
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    from ultrare_amd import sparse_kmeans as sk
    rs = np.random.RandomState(3)
    rows = np.concatenate([np.repeat(np.delete(np.arange(9), 4), 30), np.full(5000, 4)])
    cols = np.concatenate([rs.choice(6000, 30, replace=False) for _ in range(8)] + [rs.choice(6000, 5000, replace=False)])
    vals = (rs.randint(1, 11, len(rows)) / 10.0).astype(np.float16).astype(np.float32)
    halves = sg.canonical_csr(sparse.coo_matrix((vals, (rows, cols)), shape=(9, 6000)))
    assert np.diff(halves[0].off)[4] == 5000
    S = engine.CsrSet(halves)
    for k in (3, 65):
        C = centroids_for(halves, k, seed=k)
        got = engine.csr_kmeans_cost(S, transposed(C), k)
        assert np.array_equal(bits(got), bits(sk.kmeans_cost_csr_ref(halves[0], C))), k


# ---- 2. centroids, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_centroids_equal_the_contract_bit_for_bit(small, k):
    from ultrare_amd import engine
    from ultrare_amd import sparse_kmeans as sk
    halves, S = small
    label = labels_for(203, k, seed=100 + k)
    want, want_counts = sk.kmeans_centroids_csc_ref(halves[1], label, k)
    if k >= 3:
        assert want_counts[k - 1] == 1 and want_counts[k - 2] == 0
    Ct, counts = engine.csr_kmeans_centroids(S, label, k)
    assert Ct.shape == (97, k) and Ct.dtype == torch.float32 and counts.dtype == torch.int32
    assert np.array_equal(counts.cpu().numpy(), want_counts), k
    assert np.array_equal(bits(Ct.T), bits(want)), k
    if k >= 3:
        assert not Ct[:, k - 2].any() and Ct[:, k - 1].any()        # the cluster without members: a zero row, count 0
    Ct2, counts2 = engine.csr_kmeans_centroids(S, torch.from_numpy(label.astype(np.int32)).cuda(), k)      # device labels: the same path
    assert torch.equal(Ct2.view(torch.int32), Ct.view(torch.int32)) and torch.equal(counts2, counts)


@pytest.mark.parametrize('k', [4, 5])
def test_centroids_on_the_toy_ratings_bit_for_bit(toy, k):
    from oracle import cpu_ref as O
    from ultrare_amd import engine
    from ultrare_amd import sparse_kmeans as sk
    mat, halves, S = toy
    label = np.random.RandomState(k).randint(0, k, N_USER)
    want, want_counts = sk.kmeans_centroids_csc_ref(halves[1], label, k)
    Ct, counts = engine.csr_kmeans_centroids(S, label, k)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(bits(Ct.T), bits(want))
    assert np.array_equal(bits(Ct.T), bits(O.kmeans_centroids(np.asarray(mat.todense(), dtype=np.float32), label, k)))


def test_centroids_on_a_70000_entry_column_bit_for_bit():
    """70,000 users x 40 items, 3 draws per user and one item rated by everyone: a column one past any 16-bit count, walked
    by its one owner.  Cluster 3 of 4 has no member."""
    from scipy import sparse
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    from ultrare_amd import sparse_kmeans as sk
    n, n_item, k = 70000, 40, 4
    rs = np.random.RandomState(11)
    rows = np.concatenate([np.repeat(np.arange(n), 3), np.arange(n)])
    cols = np.concatenate([rs.randint(0, n_item - 1, 3 * n), np.full(n, n_item - 1)])
    vals = (rs.randint(1, 11, len(rows)) / 10.0).astype(np.float16).astype(np.float32)
    halves = sg.canonical_csr(sparse.coo_matrix((vals, (rows, cols)), shape=(n, n_item)))
    assert np.diff(halves[1].off)[n_item - 1] == n > 65536
    label = rs.randint(0, 3, n)
    want, want_counts = sk.kmeans_centroids_csc_ref(halves[1], label, k)
    Ct, counts = engine.csr_kmeans_centroids(engine.CsrSet(halves), label, k)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and want_counts[3] == 0
    got = Ct.cpu().numpy().T
    assert np.array_equal(bits(got), bits(want)) and not got[3].any()
    # the long column once more, independently of the contract's own vectorisation: a plain float32 loop
    a, b = halves[1].off[n_item - 1], halves[1].off[n_item]
    users, x = halves[1].idx[a:b], halves[1].val[a:b]
    for c in range(3):
        inv = np.float32(1.0 / np.float64(want_counts[c]))
        s = np.float32(0.0)
        for t in (x[label[users] == c] * inv):
            s = np.float32(s + t)
        assert got[c, n_item - 1] == s


# ---- 3. the fill against the host function of the same library -------------------------------------------------------------------
def host_assign(dist, capacity):
    from ultrare_amd import _native as nv
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n, k = dist.shape
    label = np.empty(n, dtype=np.int32)
    nv.check(nv.lib().ure_host_kmeans_assign(dist.ctypes.data, n, k, capacity, label.ctypes.data, None), 'ure_host_kmeans_assign')
    return label


def check_fill(what, dist, capacity):
    from ultrare_amd import engine
    n, k = dist.shape
    label, rounds = engine.balanced_fill(torch.from_numpy(dist).cuda(), capacity)
    ROUNDS[(what, n, k, capacity)] = rounds
    print(f'balanced_fill {what}: n = {n}, k = {k}, capacity = {capacity}: {rounds} rounds')
    assert label.dtype == torch.int32 and label.shape == (n,)
    assert 1 <= rounds <= n * k + 1
    got = label.cpu().numpy()
    assert np.array_equal(got, host_assign(dist, capacity)), (what, n, k, capacity)
    if capacity > 0:
        assert np.bincount(got, minlength=k).max() <= capacity
    return rounds


@pytest.mark.parametrize('n,k', [(1, 1), (37, 5), (320, 5), (999, 7), (4097, 32), (1000, 256), (70001, 3)])
def test_fill_equals_the_host_fill_at_every_shape(n, k):
    dist = np.random.RandomState(n + k).rand(n, k).astype(np.float32)
    check_fill('uniform', dist, int(np.ceil(n / k)))
    if (n, k) == (37, 5):
        assert check_fill('uniform, nothing binds', dist, n) == 1
    if (n, k) == (320, 5):
        assert int(np.ceil(n / k)) * k == n                 # capacity exactly n / k: every group ends full


def fill_patterns(n, k):
    rs = np.random.RandomState(n * k)
    base = rs.rand(k).astype(np.float32)
    return {
        'three levels': rs.randint(0, 3, (n, k)).astype(np.float32),
        'all zero': np.zeros((n, k), dtype=np.float32),
        'signed zeros': np.where(rs.rand(n, k) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32),
        'skewed columns': (np.arange(k)[None, :] * 1e3 + np.arange(n)[:, None]).astype(np.float32),
        'last bits': (base.view(np.uint32)[None, :] + rs.randint(0, 4, (n, k)).astype(np.uint32)).view(np.float32),
    }


@pytest.mark.parametrize('what', ['three levels', 'all zero', 'signed zeros', 'skewed columns', 'last bits'])
def test_fill_equals_the_host_fill_on_every_distance_pattern(what):
    for n, k in [(320, 5), (999, 7)]:
        dist = fill_patterns(n, k)[what]
        if what == 'signed zeros':
            assert np.signbit(dist).any() and not np.signbit(dist).all()
        check_fill(what, dist, int(np.ceil(n / k)))


def test_argmin_follows_the_first_nan_rule():
    rs = np.random.RandomState(0)
    dist = rs.standard_normal((517, 6)).astype(np.float32)
    dist[::3, 4] = np.nan
    dist[::6, 1] = np.nan                                    # two NaNs in a row: the first wins
    dist[5] = [2.0, 1.0, 1.0, 5.0, 1.0, 3.0]                 # the first minimum
    dist[7] = [0.0, -0.0, 1.0, 2.0, 3.0, 4.0]                # -0.0 == +0.0 here
    assert check_fill('argmin with NaN', dist, 0) == 1
    want = host_assign(dist, 0)
    assert want[0] == 1 and want[3] == 4 and want[5] == 1 and want[7] == 0
    # and a NaN key in the balanced fill sorts by its bits, as on the host
    check_fill('balanced with NaN', dist, int(np.ceil(517 / 6)))


def test_the_fill_refuses_what_the_host_refuses():
    from ultrare_amd import engine
    dist = torch.zeros(10, 4, device='cuda')
    with pytest.raises(ValueError, match='capacity 2 x 4 groups < 10 users'):
        engine.balanced_fill(dist, 2)
    with pytest.raises(ValueError, match='contiguous float32'):
        engine.balanced_fill(dist.double(), 3)
    with pytest.raises(ValueError, match='k must'):
        engine.balanced_fill(torch.zeros(2, 257, device='cuda'), 1)


# ---- 4. order and company -------------------------------------------------------------------------------------------------------
def test_a_second_stream_and_other_company_change_no_byte(small, toy):
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    halves, S = small
    k = 5
    Ct = transposed(centroids_for(halves, k, seed=9))
    label = labels_for(203, k, seed=9)
    fill_in = torch.from_numpy(np.random.RandomState(9).randint(0, 3, (999, 7)).astype(np.float32)).cuda()
    dist_a = engine.csr_kmeans_cost(S, Ct, k)
    cent_a, counts_a = engine.csr_kmeans_centroids(S, label, k)
    fill_a, rounds_a = engine.balanced_fill(fill_in, 143)
    torch.cuda.synchronize()
    _, toy_halves, toy_S = toy
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    toy_Ct = transposed(sg.dense_rows(toy_halves[0], np.arange(7)))
    label_d = torch.from_numpy(label.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        engine.csr_kmeans_cost(toy_S, toy_Ct, 7)                                 # unrelated work in flight on the default stream ...
        engine.csr_kmeans_cost(toy_S, toy_Ct, 7, stream=side)                    # ... and ahead on the side stream
        dist_b = engine.csr_kmeans_cost(S, Ct, k, stream=side)
        cent_b, counts_b = engine.csr_kmeans_centroids(S, label_d, k, stream=side)
        fill_b, rounds_b = engine.balanced_fill(fill_in, 143, stream=side)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(dist_a.view(torch.int32), dist_b.view(torch.int32))
    assert torch.equal(cent_a.view(torch.int32), cent_b.view(torch.int32)) and torch.equal(counts_a, counts_b)
    assert torch.equal(fill_a, fill_b) and rounds_a == rounds_b


# ---- 5. whole runs against the dense route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('balanced', [False, True])
@pytest.mark.parametrize('k', [4, 5])
def test_single_kmeans_on_the_csr_equals_the_dense_route(toy, k, balanced):
    from ultrare_amd.method.utils import singleKmeans
    mat, halves, _ = toy
    dense = np.asarray(mat.todense(), dtype=np.float32)
    for seed in (0, 1):
        np.random.seed(seed)
        label, inertia = singleKmeans(k, N_USER, halves, balanced, 10)
        np.random.seed(seed)
        want_label, want_inertia = singleKmeans(k, N_USER, dense, balanced, 10)
        assert label.dtype == np.int64 and np.array_equal(label, want_label), (seed, k, balanced)
        assert inertia == want_inertia, (seed, k, balanced)
        if balanced:
            assert np.bincount(label, minlength=k).max() <= int(np.ceil(N_USER / k))
    np.random.seed(0)
    again, _ = singleKmeans(k, N_USER, mat, balanced, 10)    # the SciPy matrix (wider than DENSE_MAX_ITEMS) takes the same route
    np.random.seed(0)
    assert np.array_equal(again, singleKmeans(k, N_USER, halves, balanced, 10)[0])


def test_the_fill_rounds_of_a_run_are_recorded(toy):
    from ultrare_amd.method import utils
    _, _, S = toy
    np.random.seed(0)
    rounds = []
    utils._single_kmeans_csr(5, N_USER, S, True, 10, rounds=rounds)
    print('balanced_fill rounds per k-means round on the toy ratings at k = 5:', rounds)
    ROUNDS[('toy run', N_USER, 5, 302)] = rounds
    assert 1 <= len(rounds) <= 10 and all(1 <= r <= N_USER * 5 + 1 for r in rounds)


# ---- 6. the surface ------------------------------------------------------------------------------------------------------------
def test_group_grouping_rating_bkmeans_partitions_the_users_and_caches(toy, tmp_path):
    from ultrare_amd.group import Group
    mat = toy[0]
    np.random.seed(0)
    res = Group(mat, 'toy').grouping('toy', 5, 'rating-bkmeans', verbose=False, data_dir=str(tmp_path))
    assert len(res) == 5 and sorted(u for g in res for u in g) == list(range(N_USER))
    assert all(g == sorted(g) for g in res)
    assert max(map(len, res)) <= int(np.ceil(N_USER / 5))
    path = tmp_path / 'toy' / 'val' / 'rating-bkmeans5.npy'
    assert path.exists()
    again = Group(None, 'toy', None).grouping('toy', 5, 'rating-bkmeans', verbose=False, data_dir=str(tmp_path))     # no matrix: only the cache can answer
    assert again == res


def test_the_command_line_groups_by_balanced_kmeans_in_a_fresh_process(tmp_path):
    """main.py --group 5 --group-type rating-bkmeans on the toy set in a child process, with no user_mat0.npy anywhere:
    Instance.runGroup reads the ratings, groups them through the CSR k-means kernels and trains the shards."""
    import shutil
    data, save = tmp_path / 'data', tmp_path / 'result'
    (data / 'toy').mkdir(parents=True)
    shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
    shutil.copy(os.path.join(ROOT, 'tests', 'golden', 'toy', '0_test.csv'), data / 'toy' / '0_test.csv')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'main.py'), '--dataset', 'toy', '--group', '5', '--group-type', 'rating-bkmeans',
                        '--epoch', '1', '--verbose', '0', '--data-dir', str(data), '--save-dir', str(save)], env=env, cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    assert not list(save.rglob('*_g0'))                               # no full-MF stage ran, before or during
    g5 = save / '2' / 'rand' / 'toy_g5'
    for f in ('MF_rating-bkmeans_sisa_learn/log0.npy', 'MF_rating-bkmeans_sisa_learn/user_mat5.npy'):
        assert (g5 / f).exists(), f
    groups = np.load(data / 'toy' / 'val' / 'rating-bkmeans5.npy', allow_pickle=True)
    assert sorted(u for g in groups for u in g) == list(range(N_USER)) and max(len(g) for g in groups) <= int(np.ceil(N_USER / 5))


# ---- 7. no dense array -----------------------------------------------------------------------------------------------------------
def test_a_balanced_run_on_two_million_items_forms_no_dense_array():
    """300 users x 2,000,000 items with about 30,000 ratings, k = 4, one balanced run.  The dense float32 matrix would take
    2.4 GB; the run may hold the CSR and the CSC (12 bytes a rating each and their offsets), two [n_item][k] centroid tables
    (the round's and the next), the [n][k] distances with the labels and gathered values beside them, and the workspaces --
    nothing that grows with n * n_item."""
    from scipy import sparse
    from ultrare_amd import sparse_group as sg
    from ultrare_amd.method.utils import singleKmeans
    n, n_item, k = 300, 2_000_000, 4
    rs = np.random.RandomState(2)
    rows, cols = np.repeat(np.arange(n), 100), rs.randint(0, n_item, 100 * n)
    vals = (rs.randint(1, 11, len(rows)) / 10.0).astype(np.float16).astype(np.float32)
    halves = sg.canonical_csr(sparse.coo_matrix((vals, (rows, cols)), shape=(n, n_item)))
    nnz = halves[0].nnz
    assert 29000 < nnz <= 30000
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    np.random.seed(0)
    label, inertia = singleKmeans(k, n, halves, True, 10)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    csr_csc = 2 * 12 * nnz + 8 * (n + 1) + 8 * (n_item + 1)
    tables = 2 * n_item * k * 4
    per_user = 2 * (n * k * 4 + n * (4 + 8 + 4 + 8))        # distances; int32 and int64 labels, gathered float, fill keys -- a round's
                                                            # arrays live until the next round rebinds their names
    workspace = 4 * k + 4096 + 4 * k
    slack = 64 * 512                                        # the caching allocator rounds every block up to 512 bytes
    bound = csr_csc + tables + per_user + workspace + slack
    print(f'peak device memory {peak} bytes, bound {bound}, dense array {n * n_item * 4}')
    assert peak <= bound < n * n_item * 4 / 20
    assert np.bincount(label, minlength=k).max() <= 75 and np.isfinite(inertia)


# ---- 8. the torch ops ------------------------------------------------------------------------------------------------------------
def test_torch_ops_equal_the_engine_calls(small):
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    from ultrare_amd import ops  # noqa: F401  (registers torch.ops.ultrare.*)
    halves, S = small
    k = 5
    Ct = transposed(centroids_for(halves, k, seed=2))
    label = torch.from_numpy(labels_for(203, k, seed=2).astype(np.int32)).cuda()
    want = engine.csr_kmeans_cost(S, Ct, k)
    got = torch.ops.ultrare.csr_kmeans_cost(S.row_off, S.col, S.val, Ct, k)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    want_C, want_counts = engine.csr_kmeans_centroids(S, label, k)
    got_C, got_counts = torch.ops.ultrare.csr_kmeans_centroids(S.col_off, S.row, S.cval, label, k)
    assert torch.equal(got_C.view(torch.int32), want_C.view(torch.int32)) and torch.equal(got_counts, want_counts)
    for capacity in (0, 41):
        want_label, want_rounds = engine.balanced_fill(want, capacity)
        got_label, got_rounds = torch.ops.ultrare.balanced_fill(want, capacity)
        assert torch.equal(got_label, want_label) and got_rounds.tolist() == [want_rounds] and not got_rounds.is_cuda
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        f = mode.from_tensor
        fake = torch.ops.ultrare.csr_kmeans_cost(f(S.row_off), f(S.col), f(S.val), f(Ct), k)
        fake_C, fake_counts = torch.ops.ultrare.csr_kmeans_centroids(f(S.col_off), f(S.row), f(S.cval), f(label), k)
        fake_label, fake_rounds = torch.ops.ultrare.balanced_fill(f(want), 41)
    assert tuple(fake.shape) == (203, k) and fake.dtype == torch.float32
    assert tuple(fake_C.shape) == (97, k) and fake_C.dtype == torch.float32
    assert tuple(fake_counts.shape) == (k,) and fake_counts.dtype == torch.int32
    assert tuple(fake_label.shape) == (203,) and fake_label.dtype == torch.int32 and fake_rounds.dtype == torch.int64
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.csr_kmeans_cost(S.row_off.cpu(), S.col, S.val, Ct, k)
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.csr_kmeans_centroids(S.col_off, S.row, S.cval, label.cpu(), k)
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.balanced_fill(want.cpu(), 41)
    with pytest.raises(nv.NativeError):
        engine.csr_kmeans_cost(S, Ct.cpu(), k)
