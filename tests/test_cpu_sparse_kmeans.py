"""k-means / balanced k-means on the sparse rating matrix, host side (-m "not gpu"): the numpy contract of the CSR kernels
(ultrare_amd/sparse_kmeans.py), which the GPU tests hold the device to bit for bit, against the oracle of the dense route on
the densified matrix; the fill contract against ure_host_kmeans_assign (the authority on bit patterns) and against the oracle;
the threshold iteration the device runs against the same walk; the refusals before any device work; the C entry points'
argument checks; the Group.grouping and command-line surface.  Nothing here initialises HIP."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, 'tests', 'golden', 'toy', '0_train.csv')
N_USER, N_ITEM = 1508, 2071


@pytest.fixture(scope='session')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_matrix(seed, n=61, n_item=45):
    """A random matrix with two empty rows, an empty column and explicit stored zeros, values on the float16 grid."""
    from scipy import sparse
    from ultrare_amd import sparse_group as sg
    rs = np.random.RandomState(seed)
    mat = sparse.random(n, n_item, density=0.2, random_state=rs, format='coo', dtype=np.float32)
    keep = (mat.row != 3) & (mat.row != n - 1) & (mat.col != 7)
    rows, cols = mat.row[keep], mat.col[keep]
    vals = (rs.randint(1, 11, len(rows)) / 10.0).astype(np.float16).astype(np.float32)
    vals[rs.choice(len(vals), 9, replace=False)] = 0.0
    halves = sg.canonical_csr(sparse.coo_matrix((vals, (rows, cols)), shape=(n, n_item)))
    csr, csc = halves
    assert np.diff(csr.off)[3] == 0 and np.diff(csc.off)[7] == 0 and (csr.val == 0).sum() == 9
    return halves, sg.dense_rows(csr, np.arange(n))


@pytest.fixture(scope='module')
def toy():
    from ultrare_amd import sparse_group as sg
    from ultrare_amd.read import readSparseMat
    mat = readSparseMat(TRAIN, N_USER, N_ITEM)
    return sg.canonical_csr(mat), np.asarray(mat.todense(), dtype=np.float32)


# ---- 1. the contract against the oracle of the dense route --------------------------------------------------------------------
@pytest.mark.parametrize('seed,k', [(0, 1), (1, 4), (2, 7)])
def test_cost_and_centroids_equal_the_dense_oracle_on_random_matrices(seed, k):
    from oracle import cpu_ref as O
    from ultrare_amd import sparse_kmeans as sk
    (csr, csc), dense = random_matrix(seed)
    rs = np.random.RandomState(100 + seed)
    C = rs.standard_normal((k, dense.shape[1])).astype(np.float32)
    C[0] = dense[5]
    assert np.array_equal(bits(sk.kmeans_cost_csr_ref(csr, C)), bits(O.kmeans_dist(dense, C)))
    label = rs.randint(0, k, dense.shape[0])
    label[:k] = np.arange(k)                                 # the oracle divides by every cluster's size
    got, counts = sk.kmeans_centroids_csc_ref(csc, label, k)
    assert np.array_equal(bits(got), bits(O.kmeans_centroids(dense, label, k)))
    assert np.array_equal(counts, np.bincount(label, minlength=k))


@pytest.mark.parametrize('k', [4, 5])
def test_cost_and_centroids_equal_the_dense_oracle_on_the_toy_ratings(toy, k):
    from oracle import cpu_ref as O
    from ultrare_amd import sparse_kmeans as sk
    (csr, csc), dense = toy
    rs = np.random.RandomState(k)
    C = dense[rs.choice(N_USER, k, replace=False)]
    dist = sk.kmeans_cost_csr_ref(csr, C)
    assert dist.shape == (N_USER, k) and dist.dtype == np.float32
    assert np.array_equal(bits(dist), bits(O.kmeans_dist(dense, C)))
    label = dist.argmin(axis=1)
    if np.bincount(label, minlength=k).min() == 0:
        label[:k] = np.arange(k)
    got, counts = sk.kmeans_centroids_csc_ref(csc, label, k)
    assert np.array_equal(bits(got), bits(O.kmeans_centroids(dense, label, k)))
    # and a second round from centroids that are means, not rows
    assert np.array_equal(bits(sk.kmeans_cost_csr_ref(csr, got)), bits(O.kmeans_dist(dense, got)))


def test_a_cluster_without_members_gives_a_zero_row():
    from ultrare_amd import sparse_kmeans as sk
    (csr, csc), dense = random_matrix(3)
    label = np.random.RandomState(0).randint(0, 3, dense.shape[0])
    label[label == 1] = 2
    C, counts = sk.kmeans_centroids_csc_ref(csc, label, 4)
    assert counts[1] == 0 == counts[3] and not C[1].any() and not C[3].any() and C[2].any()
    with pytest.raises(ValueError, match='label must'):
        sk.kmeans_centroids_csc_ref(csc, np.full(dense.shape[0], 4), 4)


# ---- 2. the fill contract -------------------------------------------------------------------------------------------------------
def host_assign(nv, dist, capacity):
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n, k = dist.shape
    label = np.empty(n, dtype=np.int32)
    nv.check(nv.lib().ure_host_kmeans_assign(dist.ctypes.data, n, k, capacity, label.ctypes.data, None), 'ure_host_kmeans_assign')
    return label


def fill_cases():
    rs = np.random.RandomState(7)
    out = []
    for n, k in [(1, 1), (7, 7), (37, 5), (59, 6), (200, 3)]:
        out.append((f'random {n}x{k}', rs.standard_normal((n, k)).astype(np.float32), False))
        out.append((f'tied {n}x{k}', rs.randint(0, 3, (n, k)).astype(np.float32), False))
        out.append((f'equal {n}x{k}', np.full((n, k), 2.5, dtype=np.float32), False))
        out.append((f'skewed {n}x{k}', (np.arange(k)[None, :] * 1e3 + np.arange(n)[:, None]).astype(np.float32), False))
        z = np.where(rs.rand(n, k) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        out.append((f'signed zeros {n}x{k}', z, True))
    return out


@pytest.mark.parametrize('name,dist,signed_zero', fill_cases(), ids=[c[0] for c in fill_cases()])
def test_the_fill_contract_equals_the_host_function_and_the_oracle(nv, name, dist, signed_zero):
    from oracle import cpu_ref as O
    from ultrare_amd import sparse_kmeans as sk
    n, k = dist.shape
    cap = int(np.ceil(n / k))
    for capacity in (cap, n):
        want = host_assign(nv, dist, capacity)
        assert np.array_equal(sk.balanced_fill_ref(dist, capacity), want), (name, capacity)
        got, rounds = sk.threshold_fill_ref(dist, capacity)   # the iteration the device runs reaches the same labels
        assert np.array_equal(got, want) and 1 <= rounds <= n * k + 1, (name, capacity, rounds)
    assert np.bincount(sk.balanced_fill_ref(dist, cap), minlength=k).max() <= cap
    assert np.array_equal(sk.balanced_fill_ref(dist, 0), host_assign(nv, dist, 0))
    if not signed_zero:
        assert np.array_equal(sk.balanced_fill_ref(dist, cap), O.kmeans_assign(dist, True))
        assert np.array_equal(sk.balanced_fill_ref(dist, 0), O.kmeans_assign(dist, False))


def test_the_fill_ranks_minus_zero_before_plus_zero_and_nan_by_its_bits(nv):
    from ultrare_amd import sparse_kmeans as sk
    dist = np.array([[0.0, -0.0], [0.0, -0.0], [-0.0, 0.0]], dtype=np.float32)
    want = host_assign(nv, dist, 2)
    assert want.tolist() == [1, 1, 0]                        # every user's -0.0 comes first; a stable float sort would give [0, 0, 1]
    assert sk.balanced_fill_ref(dist, 2).tolist() == want.tolist()
    assert sk.threshold_fill_ref(dist, 2)[0].tolist() == want.tolist()
    keys = sk.fill_keys(np.array([[-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan]], dtype=np.float32))
    assert (np.diff((keys >> np.uint64(32)).astype(np.int64)) > 0).all()
    # argmin: the first NaN wins, otherwise the first minimum (and -0.0 == +0.0 there)
    rows = np.array([[3.0, np.nan, 1.0, np.nan], [2.0, 1.0, 1.0, 5.0], [0.0, -0.0, 1.0, 2.0]], dtype=np.float32)
    assert sk.balanced_fill_ref(rows, 0).tolist() == host_assign(nv, rows, 0).tolist() == [1, 1, 0]
    nan = np.random.RandomState(0).standard_normal((30, 4)).astype(np.float32)
    nan[::3, 2] = np.nan
    for capacity in (8, 30):
        want = host_assign(nv, nan, capacity)
        assert np.array_equal(sk.balanced_fill_ref(nan, capacity), want)
        assert np.array_equal(sk.threshold_fill_ref(nan, capacity)[0], want)
    with pytest.raises(ValueError, match='capacity'):
        sk.balanced_fill_ref(nan, 7)


# ---- 3. refusals before any device work ----------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from ultrare_amd import engine

    def no_device(*a, **kw):
        raise AssertionError('device work started')
    for name in ('_device', 'CsrSet', 'csr_kmeans_cost', 'csr_kmeans_centroids', 'balanced_fill'):
        monkeypatch.setattr(engine, name, no_device)


def _bad_inputs():
    from scipy import sparse
    from ultrare_amd import sparse_group as sg
    ok = sparse.random(300, 400, density=0.05, random_state=np.random.RandomState(0), format='csr', dtype=np.float32)
    nan = ok.copy()
    nan.data[7] = np.nan
    one = lambda shape: sg.Compressed(np.zeros(1), np.zeros(0), np.zeros(0), shape)
    wide = (one((2 ** 24, 3)), one((3, 2 ** 24)))            # n k = 2^32 at k = 256; only the shape is read before the refusal
    return [('k < 1', ok, 0, 'k <= n'), ('k > n', ok, 301, 'k <= n'), ('k > 256', ok, 257, 'at most 256'),
            ('n k >= 2^32', wide, 256, '2\\^32'), ('1-D', sparse.coo_array(np.ones(300)), 4, '2-D'), ('NaN', nan, 4, 'non-finite'),
            ('not an integer', ok, 2.0, 'integer')]


@pytest.mark.parametrize('case', range(7))
def test_bad_input_is_refused_before_device_work(nv, monkeypatch, tmp_path, case):
    from ultrare_amd import sparse_kmeans as sk
    from ultrare_amd.group import Group
    from ultrare_amd.method import utils
    _no_device(monkeypatch)
    name, X, k, word = _bad_inputs()[case]
    with pytest.raises(ValueError, match=word):
        sk.check_kmeans_args(X, k)
    state = np.random.get_state()[1].copy()
    for balanced in (False, True):
        with pytest.raises(ValueError):
            utils.kmeans(k, 300, X, balanced=balanced)
        with pytest.raises(ValueError):
            utils.singleKmeans(k, 300, X, balanced, 10)
    assert np.array_equal(np.random.get_state()[1], state)    # and before any draw from the global generator
    if not isinstance(X, tuple) and isinstance(k, int) and k > 1:
        for var in ('rating-kmeans', 'rating-bkmeans'):
            with pytest.raises(ValueError):
                Group(X, 'bad', None).grouping('bad', k, var, verbose=False, data_dir=str(tmp_path))
            assert not os.path.exists(tmp_path / 'bad' / 'val' / f'{var}{k}.npy')


def test_the_largest_admitted_product_passes_the_check():
    from ultrare_amd import sparse_group as sg
    from ultrare_amd import sparse_kmeans as sk
    half = lambda shape: sg.Compressed(np.zeros(1), np.zeros(0), np.zeros(0), shape)
    halves = (half((2 ** 24, 3)), half((3, 2 ** 24)))
    assert sk.check_kmeans_args(halves, 255) is halves


def test_engine_calls_refuse_cpu_tensors(nv):
    import types

    import torch
    from ultrare_amd import engine
    S = types.SimpleNamespace(n=4, n_item=6, device='cpu')
    with pytest.raises(nv.NativeError, match='HIP device only'):
        engine.csr_kmeans_cost(S, torch.zeros(6, 2), 2)
    with pytest.raises(nv.NativeError, match='HIP device only'):
        engine.csr_kmeans_centroids(S, torch.zeros(4, dtype=torch.int32), 2)
    with pytest.raises(nv.NativeError, match='HIP device only'):
        engine.balanced_fill(torch.zeros(4, 2), 2)
    with pytest.raises(nv.NativeError, match='HIP device only'):
        engine.balanced_fill(np.zeros((4, 2), dtype=np.float32), 2)
    with pytest.raises(ValueError, match='k must'):
        engine.csr_kmeans_cost(S, torch.zeros(6, 2), 257)
    with pytest.raises(ValueError, match='k must'):
        engine.csr_kmeans_centroids(S, np.zeros(4, dtype=np.int64), 0)
    with pytest.raises(ValueError, match='label must'):
        engine.csr_kmeans_centroids(S, np.array([0, 1, 2, 0]), 2)


# ---- 4. the C entry points ------------------------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(0x1000)                         # never dereferenced: every check fails before the device is touched


def test_the_c_entry_points_reject_bad_arguments(nv):
    L = nv.lib()

    def refused(rc, word):
        msg = L.ure_last_error().decode()
        return rc == -1 and word in msg

    cost = lambda n=10, n_item=20, k=8, ws=FAKE, nbytes=32, Ct=FAKE: L.ure_csr_kmeans_cost(FAKE, FAKE, FAKE, n, n_item, Ct, k, FAKE, ws, nbytes, None)
    assert refused(cost(Ct=None), 'row_off && col') and refused(cost(k=0), 'k >= 1') and refused(cost(k=257, nbytes=4096), 'k <= kCsrMaxK')
    assert refused(cost(n=0), 'n >= 1') and refused(cost(n_item=1 << 31), 'n_item <= INT32_MAX')
    assert refused(cost(ws=None), 'workspace != nullptr') and refused(cost(nbytes=31), 'workspace_bytes')
    cent = lambda n=10, n_item=20, k=8, label=FAKE: L.ure_csr_kmeans_centroids(FAKE, FAKE, FAKE, n_item, n, label, k, FAKE, FAKE, None)
    assert refused(cent(label=None), 'col_off && row') and refused(cent(k=0), 'k >= 1') and refused(cent(k=257), 'k <= kCsrMaxK')
    assert refused(cent(n=1 << 31), 'n <= INT32_MAX') and refused(cent(n_item=0), 'n_item >= 1')
    fill = lambda n=10, k=4, cap=3, ws=FAKE, nbytes=1 << 20, label=FAKE: L.ure_balanced_fill(FAKE, n, k, cap, label, None, ws, nbytes, None)
    assert refused(fill(label=None), 'dist_nk && label') and refused(fill(k=0), 'k >= 1') and refused(fill(k=257), 'k <= kCsrMaxK')
    assert refused(fill(n=1 << 24, k=256), '<< 32') and refused(fill(cap=2), 'capacity 2 x 4 groups < 10 users')
    assert refused(fill(ws=None), 'workspace != nullptr') and refused(fill(nbytes=4096 + 79), 'workspace_bytes')
    for k in (1, 5, 256):
        assert L.ure_csr_kmeans_cost_scratch(k) == 4 * k
    assert L.ure_csr_kmeans_cost_scratch(0) == -1 == L.ure_csr_kmeans_cost_scratch(257)
    assert L.ure_balanced_fill_scratch(10, 4) == 4096 + 80
    assert L.ure_balanced_fill_scratch(1 << 24, 256) == -1 == L.ure_balanced_fill_scratch(0, 4)
    assert L.ure_balanced_fill_scratch((1 << 24) - 1, 256) > 0


def test_no_kmeans_kernel_spills(nv):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = [r for r in isa_report.kernels(nv.LIB_PATH) if r['name'].startswith(('km_', 'fill_', 'csr_row_walk<KmCost,', 'csr_col_walk<KmMean,'))]
    assert len([r for r in rows if r['name'].startswith('csr_row_walk<KmCost,')]) == 7
    assert len([r for r in rows if r['name'].startswith('csr_col_walk<KmMean,')]) == 7
    assert {'km_csq_kernel', 'fill_argmin_kernel', 'fill_choose_kernel', 'fill_select_kernel'} <= {r['name'].split('(')[0] for r in rows}
    for r in rows:
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, r


# ---- 5. the surface ---------------------------------------------------------------------------------------------------------------
def test_grouping_admits_the_kmeans_variants_and_sends_the_csr_through(monkeypatch, tmp_path, toy):
    """Group.grouping('rating-kmeans' / 'rating-bkmeans') on a matrix wider than DENSE_MAX_ITEMS hands kmeans the (csr, csc)
    pair, never a dense array; narrower matrices and the embedding keep the dense route."""
    from scipy import sparse
    from ultrare_amd import group as G
    from ultrare_amd.sparse_group import Compressed
    seen = []

    def fake_kmeans(n_group, n_user, X, balanced=False):
        seen.append((n_group, n_user, X, balanced))
        return np.arange(n_user) % n_group
    monkeypatch.setattr(G, 'kmeans', fake_kmeans)
    mat = sparse.csr_matrix(toy[1])
    for var, balanced in (('rating-kmeans', False), ('rating-bkmeans', True)):
        res = G.Group(mat, 'toy', None).grouping('toy', 5, var, verbose=False, data_dir=str(tmp_path))
        n_group, n_user, X, bal = seen[-1]
        assert (n_group, n_user, bal) == (5, N_USER, balanced)
        assert isinstance(X, tuple) and all(isinstance(h, Compressed) for h in X) and X[0].shape == (N_USER, N_ITEM)
        assert sorted(u for g in res for u in g) == list(range(N_USER))
        assert (tmp_path / 'toy' / 'val' / f'{var}5.npy').exists()
    narrow = sparse.csr_matrix(toy[1][:, :G.DENSE_MAX_ITEMS])
    G.Group(narrow, 'narrow', None).grouping('narrow', 5, 'rating-bkmeans', verbose=False, data_dir=str(tmp_path))
    assert isinstance(seen[-1][2], np.ndarray) and seen[-1][2].shape == (N_USER, G.DENSE_MAX_ITEMS)


def test_kmeans_routes_by_input_type(monkeypatch, toy):
    from scipy import sparse
    from ultrare_amd.group import DENSE_MAX_ITEMS
    from ultrare_amd.method import utils
    assert utils._kmeans_takes_csr(toy[0])
    assert utils._kmeans_takes_csr(sparse.csr_matrix((4, DENSE_MAX_ITEMS + 1)))
    assert not utils._kmeans_takes_csr(sparse.csr_matrix((4, DENSE_MAX_ITEMS)))
    assert not utils._kmeans_takes_csr(np.zeros((4, 1000), dtype=np.float32))


def test_the_command_line_admits_rating_bkmeans(tmp_path):
    """--group-type: 'rating-bkmeans' is in the help and passes main's check: the run gets as far as the rating file, which is
    not there.  Plain 'rating-kmeans' stays refused by that check (tests/test_cpu_sparse_group.py pins it)."""
    from ultrare_amd import main as cli
    assert cli.parser.parse_args(['--group-type', 'rating-bkmeans']).group_type == 'rating-bkmeans'
    assert 'rating-bkmeans' in cli.parser.format_help()
    with pytest.raises(Exception, match='cannot open') as e:
        cli.main(['--dataset', 'toy', '--group', '5', '--group-type', 'rating-bkmeans', '--data-dir', str(tmp_path / 'data'),
                  '--save-dir', str(tmp_path / 'result')])
    assert not isinstance(e.value, AssertionError)
