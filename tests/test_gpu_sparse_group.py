"""Rating-based OT grouping on the sparse matrix, device side: ure_csr_cost and ure_csr_centroids against the numpy contract
(ultrare_amd/sparse_group.py) BIT FOR BIT -- never against themselves -- at the lane-group, chunk and padding boundaries;
order and company; a 70,000-entry column without any dense array; whole ot_cluster rounds against a host replay; the
Group.grouping surface for 'rating-ot' and 'rating-sinkhorn'; the torch ops."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, 'tests', 'golden', 'toy', '0_train.csv')
N_USER, N_ITEM = 1508, 2071
# every lane-group width of csr_group.hip's group_width -- 1, 2 (the only width without the unrolled full-tile branch), 4, 8,
# 16, 32 (the usual shard count) and 64 -- with k at, just below and just above a width, then two chunks of 64 (65, 128),
# one past them (129) and the limit
KS = [1, 2, 3, 4, 5, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256]


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def crafted(variant):
    """130 users x 257 items (one past the 256 lanes of the cc reduction), values on the float16 grid of the ratings.
    'rows':    row 0 empty, row 1 one entry, row 2 all 257 entries, the others 7 .. 40 entries, some stored zeros.
    'columns': column 100 empty (row 2 holds the other 256), column 256 holds every user (so no row is empty)."""
    from scipy import sparse
    from ultrare_amd import sparse_group as sg
    rs = np.random.RandomState(5)
    rows, cols = [], []
    for i in range(130):
        if i == 0:
            c = np.zeros(0, dtype=np.int64)
        elif i == 1:
            c = np.array([200])
        elif i == 2:
            c = np.arange(257)
        else:
            c = rs.choice(256, size=7 + (i * 5) % 34, replace=False)
        if variant == 'columns':
            c = np.union1d(c[c != 100], [256])
        rows.append(np.full(len(c), i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = (rs.randint(1, 11, len(rows)) / 10.0).astype(np.float16).astype(np.float32)
    vals[rs.choice(len(vals), 25, replace=False)] = 0.0            # explicit stored zeros
    halves = sg.canonical_csr(sparse.coo_matrix((vals, (rows, cols)), shape=(130, 257)))
    lens, clens = np.diff(halves[0].off), np.diff(halves[1].off)
    assert halves[0].nnz == len(rows) and (halves[0].val == 0).sum() == 25
    if variant == 'rows':
        assert lens[0] == 0 and lens[1] == 1 and lens[2] == 257 and lens[3:].min() >= 7 and lens[3:].max() <= 40
    else:
        assert clens[100] == 0 and clens[256] == 130 and lens.min() >= 1
    return halves


@pytest.fixture(scope='module')
def mats():
    from ultrare_amd import engine
    out = {}
    for v in ('rows', 'columns'):
        halves = crafted(v)
        out[v] = (halves, engine.CsrSet(halves))
    return out


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


def transposed(C, ldc):
    """Ct [n_item, ldc] on the device; the padding columns hold NaN: the kernel must not read them."""
    k, n_item = C.shape
    Ct = np.full((n_item, ldc), np.nan, dtype=np.float32)
    Ct[:, :k] = C.T
    return torch.from_numpy(Ct).cuda()


# ---- 1. cost, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_cost_equals_the_contract_bit_for_bit(mats, k):
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    for v in ('rows', 'columns'):
        halves, S = mats[v]
        assert (S.n, S.n_item, S.nnz) == (130, 257, halves[0].nnz)
        C = centroids_for(halves, k, seed=k)
        want = sg.csr_cost_ref(halves[0], C)
        for ldc in (k, k + 3):
            got = engine.csr_cost(S, transposed(C, ldc), k)
            assert got.shape == (k, 130) and got.dtype == torch.float32
            assert np.array_equal(bits(got), bits(want)), (v, k, ldc)


def test_cost_on_the_toy_ratings_bit_for_bit(toy):
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    _, halves, S = toy
    C = sg.dense_rows(halves[0], np.random.RandomState(0).choice(N_USER, 5, replace=False))
    got = engine.csr_cost(S, transposed(C, 5), 5)
    assert np.array_equal(bits(got), bits(sg.csr_cost_ref(halves[0], C)))


# ---- 2. centroids, bit for bit ----------------------------------------------------------------------------------------------
def labels_for(n, k, seed):
    """Random labels; for k >= 2 cluster k - 1 has exactly one member (user 7)."""
    lab = np.random.RandomState(seed).randint(0, max(k - 1, 1), n)
    if k >= 2:
        lab[7] = k - 1
    return lab


@pytest.mark.parametrize('k', KS)
def test_centroids_equal_the_contract_bit_for_bit(mats, k):
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    for v in ('rows', 'columns'):
        halves, S = mats[v]
        label = labels_for(130, k, seed=100 + k)
        want, want_counts = sg.csr_centroids_ref(halves[1], label, k)
        if k >= 2:
            assert want_counts[k - 1] == 1
        for ldc in (k, k + 3):
            Ct, counts = engine.csr_centroids(S, label, k, ldc=ldc)
            assert Ct.shape == (257, ldc) and Ct.dtype == torch.float32 and counts.dtype == torch.int32
            assert np.array_equal(counts.cpu().numpy(), want_counts), (v, k)
            assert np.array_equal(bits(Ct[:, :k].T), bits(want)), (v, k, ldc)
            assert not Ct[:, k:].any()
        if v == 'columns':
            assert not Ct[100].any()                                # the empty column
        # device labels take the same path
        Ct2, counts2 = engine.csr_centroids(S, torch.from_numpy(label.astype(np.int32)).cuda(), k)
        assert torch.equal(Ct2, Ct[:, :k]) and torch.equal(counts2, counts)


def test_a_cluster_without_members_gives_the_zero_row_and_count_zero(mats):
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    halves, S = mats['columns']
    label = np.random.RandomState(1).randint(0, 4, 130)
    label[label == 2] = 3
    want, want_counts = sg.csr_centroids_ref(halves[1], label, 5)
    Ct, counts = engine.csr_centroids(S, label, 5)
    assert counts.cpu().numpy().tolist() == want_counts.tolist() and want_counts[2] == 0 == want_counts[4]
    assert np.array_equal(bits(Ct.T), bits(want)) and not Ct[:, 2].any() and not Ct[:, 4].any() and Ct[:, 3].any()


# ---- 3. order and company -----------------------------------------------------------------------------------------------------
def test_a_second_stream_and_other_company_change_no_byte(mats, toy):
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    halves, S = mats['rows']
    k = 5
    Ct = transposed(centroids_for(halves, k, seed=9), k)
    label = labels_for(130, k, seed=9)
    dist_a = engine.csr_cost(S, Ct, k)
    cent_a, counts_a = engine.csr_centroids(S, label, k)
    torch.cuda.synchronize()
    _, toy_halves, toy_S = toy
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        engine.csr_cost(toy_S, transposed(sg.dense_rows(toy_halves[0], np.arange(7)), 7), 7, stream=side)      # unrelated work first
        label_d = torch.from_numpy(label.astype(np.int32)).cuda()
        dist_b = engine.csr_cost(S, Ct, k, stream=side)
        cent_b, counts_b = engine.csr_centroids(S, label_d, k, stream=side)
    side.synchronize()
    assert torch.equal(dist_a.view(torch.int32), dist_b.view(torch.int32))
    assert torch.equal(cent_a.view(torch.int32), cent_b.view(torch.int32)) and torch.equal(counts_a, counts_b)


# ---- 4. a long column and no dense array ----------------------------------------------------------------------------------------
def test_a_70000_entry_column_and_no_dense_array():
    """70,000 users x 3,000 items, 20 draws per user and one item rated by everyone: a column one past any 16-bit count.  The
    dense float32 matrix would take 840 MB; the kernel path must stay below a quarter of that."""
    from scipy import sparse
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    n, n_item, k = 70000, 3000, 3
    rs = np.random.RandomState(11)
    rows = np.concatenate([np.repeat(np.arange(n), 20), np.arange(n)])
    cols = np.concatenate([rs.randint(0, n_item - 1, 20 * n), np.full(n, n_item - 1)])
    vals = (rs.randint(1, 11, len(rows)) / 10.0).astype(np.float16).astype(np.float32)
    halves = sg.canonical_csr(sparse.coo_matrix((vals, (rows, cols)), shape=(n, n_item)))
    csr, csc = halves
    assert np.diff(csc.off)[n_item - 1] == n > 65536
    C = sg.dense_rows(csr, rs.choice(n, k, replace=False))
    label = rs.randint(0, k, n)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    S = engine.CsrSet(halves)
    dist = engine.csr_cost(S, torch.from_numpy(np.ascontiguousarray(C.T)).cuda(), k)
    Ct, counts = engine.csr_centroids(S, label, k)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < n * n_item * 4 / 4
    want_C, want_counts = sg.csr_centroids_ref(csc, label, k)
    assert np.array_equal(bits(dist), bits(sg.csr_cost_ref(csr, C)))
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    got_C = Ct.cpu().numpy().T
    assert np.array_equal(bits(got_C), bits(want_C))
    # the long column once more, independently of the reference's own vectorisation: one cumsum per cluster
    a, b = csc.off[n_item - 1], csc.off[n_item]
    users, x = csc.idx[a:b], csc.val[a:b].astype(np.float64)
    assert np.array_equal(users, np.arange(n))
    for c in range(k):
        seq = np.cumsum(x[label[users] == c])[-1]
        assert got_C[c, n_item - 1] == np.float32(seq / np.float64(want_counts[c]))


# ---- 5. whole rounds ---------------------------------------------------------------------------------------------------------
def replay(halves, k, solve, max_iters=10):
    """ot_cluster's rounds on the host from the contract functions, with the draws of numpy's global generator."""
    from ultrare_amd import sparse_group as sg
    csr, csc = halves
    centroid = sg.dense_rows(csr, np.random.choice(csr.shape[0], size=k, replace=False))
    for _ in range(max_iters):
        dist = sg.csr_cost_ref(csr, centroid)
        label = solve(dist)
        inertia = np.min(dist, axis=0).sum()
        new_centroid, counts = sg.csr_centroids_ref(csc, label, k)
        assert counts.min() > 0
        if np.allclose(centroid, new_centroid):
            break
        centroid = new_centroid
    return inertia, label.astype(np.int64)


def warm_exact_solver(n, k):
    """The exact LP on the REFERENCE costs from the start ot_cluster gives it: ure_ot_potentials on the uploaded matrix, the
    potentials carried from round to round.  The start matters here.  The solver reaches the optimum from any potentials, but
    the labels are determined by the costs alone only where the optimum is unique (test_parity_pins.py compares labels only
    without tight cycles), and the ratings do not make it so: the 19 users without a rating, and users with the same ratings,
    have the same cost column (158 users have such a twin in the first round at k = 4, 148 at k = 5), and two of them on
    either side of a cluster boundary may change places at no cost.  On the first round's reference costs the cold start
    (pi = None) and starts a fraction of the cost's spread apart reach the same objective with 2 (k = 4) and up to 136
    (k = 5) different labels; a replay from the cold start differed from ot_cluster at k = 4."""
    from ultrare_amd import _native as nv
    from ultrare_amd.method.utils import ot_warm_iters
    pi = np.zeros(k, dtype=np.float64)

    def solve(dist):
        dist_d = torch.from_numpy(dist).cuda()
        nv.check(nv.lib().ure_ot_potentials(nv.ptr(dist_d), n, k, ot_warm_iters(n), pi.ctypes.data, None, nv.stream_handle()),
                 'ure_ot_potentials')
        return nv.ot_assign_warm(dist, pi, want_plan=False)[0]
    return solve


@pytest.mark.parametrize('k', [4, 5])
def test_ot_cluster_on_the_toy_csr_equals_the_host_replay(toy, k):
    from ultrare_amd.method.utils import ot_cluster
    mat, halves, _ = toy
    np.random.seed(0)
    inertia, label = ot_cluster(mat, k)
    np.random.seed(0)
    want_inertia, want_label = replay(halves, k, warm_exact_solver(N_USER, k))
    assert label.dtype == np.int64 and np.array_equal(label, want_label)
    assert float(inertia) == float(want_inertia)
    sizes = np.bincount(label, minlength=k)
    assert sizes.sum() == N_USER and sizes.max() - sizes.min() <= 1


# ---- 6. the surface ------------------------------------------------------------------------------------------------------------
def test_group_grouping_rating_ot_partitions_the_users_and_caches(toy, tmp_path):
    from ultrare_amd.group import Group
    from ultrare_amd.read import readSparseMat
    np.random.seed(0)
    res = Group(readSparseMat(TRAIN, N_USER, N_ITEM), 'toy', None).grouping('toy', 4, 'rating-ot', verbose=False, data_dir=str(tmp_path))
    assert len(res) == 4 and sorted(u for g in res for u in g) == list(range(N_USER))
    assert all(g == sorted(g) for g in res)
    assert max(map(len, res)) - min(map(len, res)) <= 1
    path = tmp_path / 'toy' / 'val' / 'rating-ot4.npy'
    assert path.exists()
    again = Group(None, 'toy', None).grouping('toy', 4, 'rating-ot', verbose=False, data_dir=str(tmp_path))     # no matrix: only the cache can answer
    assert again == res


def test_group_grouping_rating_sinkhorn_equals_the_solver_on_the_reference_costs(toy, tmp_path):
    """reg = the median of the first round's reference cost matrix: a large regulariser -- this is a test of the wiring,
    not of grouping quality."""
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    from ultrare_amd.group import Group
    mat, halves, _ = toy
    k = 4
    np.random.seed(0)
    first = sg.dense_rows(halves[0], np.random.choice(N_USER, size=k, replace=False))
    reg = float(np.median(sg.csr_cost_ref(halves[0], first)))
    np.random.seed(0)
    res = Group(mat, 'toy', None).grouping('toy', k, 'rating-sinkhorn', verbose=False, data_dir=str(tmp_path), reg=reg)
    assert sorted(u for g in res for u in g) == list(range(N_USER)) and all(g == sorted(g) for g in res)
    assert (tmp_path / 'toy' / 'val' / 'rating-sinkhorn4.npy').exists()

    def solve(dist):
        r = engine.ot_sinkhorn(torch.from_numpy(dist).cuda(), reg, 1000, 1e-9, want_u=False)
        return r['label'].cpu().numpy()
    np.random.seed(0)
    _, want_label = replay(halves, k, solve)
    assert res == [np.flatnonzero(want_label == c).tolist() for c in range(k)]


def test_the_command_line_groups_on_the_ratings_without_a_full_mf_run(tmp_path):
    """main --group 3 --group-type rating-ot on the toy set with no user_mat0.npy anywhere: Instance.runGroup reads the
    ratings, groups them through the CSR kernels and trains the shards."""
    import shutil
    from ultrare_amd import main as cli
    data, save = tmp_path / 'data', tmp_path / 'result'
    (data / 'toy').mkdir(parents=True)
    shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
    shutil.copy(os.path.join(ROOT, 'tests', 'golden', 'toy', '0_test.csv'), data / 'toy' / '0_test.csv')
    cli.main(['--dataset', 'toy', '--group', '3', '--group-type', 'rating-ot', '--epoch', '1', '--verbose', '0',
              '--data-dir', str(data), '--save-dir', str(save)])
    assert not list(save.rglob('*_g0'))                               # no full-MF stage ran, before or during
    g3 = save / '2' / 'rand' / 'toy_g3'
    for f in ('MF_rating-ot_sisa_learn/log0.npy', 'MF_rating-ot_sisa_learn/user_mat3.npy'):
        assert (g3 / f).exists(), f
    groups = np.load(data / 'toy' / 'val' / 'rating-ot3.npy', allow_pickle=True)
    sizes = sorted(len(g) for g in groups)
    assert sorted(u for g in groups for u in g) == list(range(N_USER)) and sizes[-1] - sizes[0] <= 1


def test_timing_is_served_for_sparse_input(toy):
    from ultrare_amd.method.utils import ot_cluster
    mat = toy[0]
    np.random.seed(0)
    exact, sink = [], []
    ot_cluster(mat, 4, max_iters=2, timing=exact)
    assert 1 <= len(exact) <= 2
    assert list(exact[0]) == ['cost_kernel_ms', 'device_potentials_ms', 'cost_to_host_ms', 'host_solver_ms', 'centroids_ms']
    ot_cluster(mat, 4, max_iters=1, timing=sink, solver='sinkhorn', reg=50.0)
    assert len(sink) == 1 and list(sink[0]) == ['cost_kernel_ms', 'device_sinkhorn_ms', 'centroids_ms']
    assert all(v >= 0 for t in exact + sink for v in t.values())


DENSE_EXACT_PARTS = ['centroid_upload_ms', 'cost_kernel_ms', 'device_potentials_ms', 'cost_to_host_ms', 'host_solver_ms', 'centroids_ms']
DENSE_SINKHORN_PARTS = ['centroid_upload_ms', 'cost_kernel_ms', 'device_sinkhorn_ms', 'centroids_ms']


def small_dense():
    return np.random.RandomState(0).standard_normal((96, 5)).astype(np.float32)


def test_timing_is_served_for_dense_input():
    """The parts bench.py's OT leg reads, in order, and the same list with the Sinkhorn part in place of the exact solver's
    three.  reg = the median of the first round's cost matrix, as in the wiring test above."""
    from ultrare_amd.method.utils import ot_cluster
    X, k = small_dense(), 3
    exact, sink = [], []
    np.random.seed(0)
    ot_cluster(X, k, max_iters=2, timing=exact)
    assert 1 <= len(exact) <= 2
    assert all(list(t) == DENSE_EXACT_PARTS for t in exact)
    np.random.seed(0)
    first = X[np.random.choice(len(X), size=k, replace=False)]
    reg = float(np.median(((X - first[:, np.newaxis]) ** 2).sum(axis=2)))
    np.random.seed(0)
    ot_cluster(X, k, max_iters=1, timing=sink, solver='sinkhorn', reg=reg)
    assert len(sink) == 1 and list(sink[0]) == DENSE_SINKHORN_PARTS
    assert all(v >= 0 for t in exact + sink for v in t.values())


@pytest.mark.parametrize('rows', ['dense', 'csr'])
def test_timing_does_not_change_the_answer(rows):
    from scipy import sparse
    from ultrare_amd.method.utils import ot_cluster
    X = small_dense()
    if rows == 'csr':
        X = sparse.csr_matrix(X * (X > 0.5))
    np.random.seed(0)
    inertia, label = ot_cluster(X, 3)
    np.random.seed(0)
    timed_inertia, timed_label = ot_cluster(X, 3, timing=[])
    assert np.array_equal(label, timed_label) and float(inertia) == float(timed_inertia)


# ---- 7. the torch ops ------------------------------------------------------------------------------------------------------------
def test_torch_ops_equal_the_engine_calls(mats):
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    from ultrare_amd import ops  # noqa: F401  (registers torch.ops.ultrare.*)
    halves, S = mats['rows']
    k = 5
    Ct = transposed(centroids_for(halves, k, seed=2), k + 3)
    label = torch.from_numpy(labels_for(130, k, seed=2).astype(np.int32)).cuda()
    want = engine.csr_cost(S, Ct, k)
    got = torch.ops.ultrare.csr_cost(S.row_off, S.col, S.val, Ct, k)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    want_C, want_counts = engine.csr_centroids(S, label, k)
    got_C, got_counts = torch.ops.ultrare.csr_centroids(S.col_off, S.row, S.cval, label, k)
    assert torch.equal(got_C.view(torch.int32), want_C.view(torch.int32)) and torch.equal(got_counts, want_counts)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        f = mode.from_tensor
        fake = torch.ops.ultrare.csr_cost(f(S.row_off), f(S.col), f(S.val), f(Ct), k)
        fake_C, fake_counts = torch.ops.ultrare.csr_centroids(f(S.col_off), f(S.row), f(S.cval), f(label), k)
    assert tuple(fake.shape) == (k, 130) and fake.dtype == torch.float32
    assert tuple(fake_C.shape) == (257, k) and fake_C.dtype == torch.float32
    assert tuple(fake_counts.shape) == (k,) and fake_counts.dtype == torch.int32
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.csr_cost(S.row_off.cpu(), S.col, S.val, Ct, k)
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.csr_centroids(S.col_off, S.row, S.cval, label.cpu(), k)
    with pytest.raises(nv.NativeError):
        engine.csr_cost(S, Ct.cpu(), k)
