"""Rating-based OT grouping on the sparse matrix, host side (-m "not gpu"): readSparseMat on a SciPy that refuses float16; the
numpy contract of the CSR kernels (sparse_group.py), which the GPU tests hold the device to bit for bit, against plain-Python
restatements and against the dense float64 forms with derived bounds; canonical_csr; the refusals of ot_cluster /
Group.grouping before any device work; the C entry points' argument checks.  Nothing here initialises HIP.

A note on a figure: the toy file holds 28,361 rating rows, three of which repeat a (user, item) pair of user 307.  The
reference's coo_matrix(...).tocsr() sums repeats, so the CSR stores 28,358 entries; both numbers are asserted."""
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


@pytest.fixture(scope='module')
def toy(nv):
    from ultrare_amd import sparse_group as sg
    from ultrare_amd.read import readSparseMat
    mat = readSparseMat(TRAIN, N_USER, N_ITEM)
    csr, csc = sg.canonical_csr(mat)
    return mat, csr, csc, np.asarray(mat.todense(), dtype=np.float64)


# ---- 1. readSparseMat ---------------------------------------------------------------------------------------------------
def test_read_sparse_mat_returns_the_float16_rounded_ratings(nv, toy):
    mat = toy[0]
    uid, iid, raw = nv.read_csv(TRAIN)
    assert len(uid) == 28361
    pairs, inverse, times = np.unique(uid.astype(np.int64) * N_ITEM + iid, return_inverse=True, return_counts=True)
    assert mat.shape == (N_USER, N_ITEM) and mat.format == 'csr'
    assert mat.nnz == len(pairs) == 28358                           # 28,361 rows, three repeated pairs summed (the reference's tocsr)
    assert np.array_equal(mat.data.astype(np.float16).astype(mat.data.dtype), mat.data)      # every value is its own float16 rounding
    single = np.flatnonzero(times[inverse] == 1)
    got = np.asarray(mat[uid[single], iid[single]]).reshape(-1).astype(np.float64)
    assert np.array_equal(got, (raw[single] / 5).astype(np.float16).astype(np.float64))
    # the repeated pairs: the float16 sum of their float16 values
    assert np.float64(mat[307, 206]) == np.float64(np.float16(3.5 / 5) + np.float16(3 / 5))
    assert np.float64(mat[307, 11]) == np.float64(np.float16(4 / 5) + np.float16(4 / 5))


# ---- 2. the contract against plain Python and against the dense float64 forms ----------------------------------------------
def _cost_plain(csr, C):
    """sparse_group.csr_cost_ref restated as loops over Python floats (IEEE doubles)."""
    k, n_item = C.shape
    cc = []
    for c in range(k):
        lanes = [0.0] * 256
        for j in range(n_item):
            lanes[j % 256] += float(C[c, j]) * float(C[c, j])
        t = 0.0
        for l in range(256):
            t += lanes[l]
        cc.append(t)
    out = np.empty((k, csr.shape[0]), dtype=np.float32)
    off, idx, val = csr.off.tolist(), csr.idx.tolist(), [float(v) for v in csr.val]
    Cl = [[float(v) for v in row] for row in C]
    for i in range(csr.shape[0]):
        xx = 0.0
        for p in range(off[i], off[i + 1]):
            xx += val[p] * val[p]
        for c in range(k):
            dot, row = 0.0, Cl[c]
            for p in range(off[i], off[i + 1]):
                dot += val[p] * row[idx[p]]
            out[c, i] = np.float32(max((xx - 2.0 * dot) + cc[c], 0.0))
    return out


def _centroids_plain(csc, label, k):
    n_item = csc.shape[0]
    S = [[0.0] * n_item for _ in range(k)]
    off, idx, val = csc.off.tolist(), csc.idx.tolist(), [float(v) for v in csc.val]
    lab = [int(v) for v in label]
    for j in range(n_item):
        for p in range(off[j], off[j + 1]):
            S[lab[idx[p]]][j] += val[p]
    counts = [lab.count(c) for c in range(k)]
    C = np.zeros((k, n_item), dtype=np.float32)
    for c in range(k):
        if counts[c]:
            C[c] = [np.float32(s / float(counts[c])) for s in S[c]]
    return C, counts


@pytest.mark.parametrize('k', [4, 5])
def test_cost_ref_equals_plain_python_and_the_dense_form_within_one_float32_rounding(toy, k):
    from ultrare_amd import sparse_group as sg
    mat, csr, csc, X = toy
    C = sg.dense_rows(csr, np.random.RandomState(k).choice(N_USER, k, replace=False))
    assert np.array_equal(C.astype(np.float64), X[np.random.RandomState(k).choice(N_USER, k, replace=False)])
    got = sg.csr_cost_ref(csr, C)
    assert got.dtype == np.float32 and got.shape == (k, N_USER)
    assert np.array_equal(got.view(np.uint32), _cost_plain(csr, C).view(np.uint32))
    assert np.array_equal(got, sg.csr_cost_ref(mat, C))              # a SciPy matrix is canonicalised on the way in
    Cd = C.astype(np.float64)
    dense = ((X[None, :, :] - Cd[:, None, :]) ** 2).sum(axis=2)
    xx, cc = (X ** 2).sum(axis=1), (Cd ** 2).sum(axis=1)
    # one float32 rounding of a result that is at most xx + cc, doubled; the float64 terms are orders of magnitude smaller
    assert (np.abs(got.astype(np.float64) - dense) <= 2.0 ** -23 * (xx[None, :] + cc[:, None])).all()
    empty = np.flatnonzero(np.diff(csr.off) == 0)
    assert len(empty) == 19
    assert np.array_equal(got[:, empty], np.repeat(sg.cc_ref(C).astype(np.float32)[:, None], len(empty), axis=1))


def test_cc_ref_follows_its_lane_order():
    from ultrare_amd import sparse_group as sg
    rs = np.random.RandomState(3)
    for n_item in (1, 255, 256, 257, 700):
        C = rs.standard_normal((3, n_item)).astype(np.float32)
        want = []
        for c in range(3):
            lanes = [0.0] * 256
            for j in range(n_item):
                lanes[j % 256] += float(C[c, j]) ** 2
            t = 0.0
            for v in lanes:
                t += v
            want.append(t)
        assert np.array_equal(sg.cc_ref(C), np.array(want))


@pytest.mark.parametrize('k', [4, 5])
def test_centroids_ref_equals_plain_python_and_the_dense_mean(toy, k):
    from ultrare_amd import sparse_group as sg
    mat, csr, csc, X = toy
    label = np.random.RandomState(10 + k).randint(0, k, N_USER)
    C, counts = sg.csr_centroids_ref(csc, label, k)
    assert C.dtype == np.float32 and C.shape == (k, N_ITEM) and counts.dtype == np.int64
    Cp, cp = _centroids_plain(csc, label, k)
    assert np.array_equal(C.view(np.uint32), Cp.view(np.uint32)) and counts.tolist() == cp == np.bincount(label, minlength=k).tolist()
    want = np.stack([X[label == c].mean(axis=0) for c in range(k)])
    assert (np.abs(C.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(X).max()).all()
    assert (np.diff(csc.off) == 0).sum() == 160 and not C[:, np.diff(csc.off) == 0].any()
    # a cluster without members: the zero row and count 0
    label2 = np.where(label == 2, 0, label)
    C2, counts2 = sg.csr_centroids_ref(csc, label2, k)
    assert counts2[2] == 0 and not C2[2].any() and counts2.sum() == N_USER and C2[1].any()
    assert np.array_equal(C2[1], C[1])
    with pytest.raises(ValueError, match='label must'):
        sg.csr_centroids_ref(csc, np.full(N_USER, k), k)
    with pytest.raises(ValueError, match='label must'):
        sg.csr_centroids_ref(csc, label[:-1], k)


# ---- 3. canonical_csr -------------------------------------------------------------------------------------------------
def test_canonical_csr_sums_duplicates_sorts_and_keeps_stored_zeros():
    from scipy import sparse
    from ultrare_amd import sparse_group as sg
    rows = np.array([2, 0, 2, 2, 1, 0, 2])
    cols = np.array([3, 1, 0, 3, 2, 0, 1])
    vals = np.array([0.5, 1.0, 0.25, 0.125, 0.0, 2.0, 4.0])        # (2, 3) twice; (1, 2) a stored zero; row 2 out of order
    csr, csc = sg.canonical_csr(sparse.coo_matrix((vals, (rows, cols)), shape=(4, 5)))
    assert csr.shape == (4, 5) and csc.shape == (5, 4) and csr.nnz == csc.nnz == 6
    assert (csr.off.dtype, csr.idx.dtype, csr.val.dtype) == (np.int64, np.int32, np.float32) == (csc.off.dtype, csc.idx.dtype, csc.val.dtype)
    assert csr.off.tolist() == [0, 2, 3, 6, 6] and csr.idx.tolist() == [0, 1, 2, 0, 1, 3]
    assert csr.val.tolist() == [2.0, 1.0, 0.0, 0.25, 4.0, 0.625]
    assert csc.off.tolist() == [0, 2, 4, 5, 6, 6] and csc.idx.tolist() == [0, 2, 0, 2, 1, 2]
    assert csc.val.tolist() == [2.0, 0.25, 1.0, 4.0, 0.0, 0.625]
    # an unsorted csr_matrix with a repeat, built behind SciPy's back
    raw = sparse.csr_matrix((np.array([1.0, 2.0, 3.0], dtype=np.float64), np.array([4, 1, 4]), np.array([0, 3])), shape=(1, 5))
    csr, csc = sg.canonical_csr(raw)
    assert csr.idx.tolist() == [1, 4] and csr.val.tolist() == [2.0, 4.0]
    assert raw.nnz == 3                                             # the input is left as it was
    assert sg.canonical_csr((csr, csc)) == (csr, csc)
    assert sg.dense_rows(csr, [0]).tolist() == [[0.0, 2.0, 0.0, 0.0, 4.0]]


def test_canonical_csr_refusals():
    from scipy import sparse
    from ultrare_amd import sparse_group as sg
    with pytest.raises(ValueError, match='2-D'):
        sg.canonical_csr(sparse.coo_array(np.array([1.0, 0.0, 2.0])))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match='non-finite'):
            sg.canonical_csr(sparse.csr_matrix(np.array([[1.0, bad], [0.0, 1.0]])))
    with pytest.raises(ValueError, match='2\\^31'):
        sg.canonical_csr(sparse.coo_matrix((2 ** 31, 3)))
    with pytest.raises(ValueError, match='2\\^31'):
        sg.canonical_csr(sparse.coo_matrix((3, 2 ** 31)))

    huge = sparse.coo_matrix((3, 3))                                # 2^31 stored entries cannot be allocated here: the count alone is faked
    huge.__class__ = type('Huge', (sparse.coo_matrix,), {'nnz': property(lambda self: 2 ** 31)})
    with pytest.raises(ValueError, match='2\\^31'):
        sg.canonical_csr(huge)
    with pytest.raises(ValueError, match='SciPy sparse'):
        sg.canonical_csr(np.eye(3))


# ---- 4. refusals before any device work -----------------------------------------------------------------------------------
def _no_device(monkeypatch):
    from ultrare_amd import engine

    def no_device(*a, **kw):
        raise AssertionError('device work started')
    for name in ('_device', 'CsrSet', 'csr_cost', 'csr_centroids', 'ot_sinkhorn'):
        monkeypatch.setattr(engine, name, no_device)


def _bad_inputs():
    from scipy import sparse
    rs = np.random.RandomState(0)
    ok = sparse.random(300, 400, density=0.05, random_state=rs, format='csr', dtype=np.float32)
    nan = ok.copy()
    nan.data[7] = np.nan
    return [('k > n', ok, 301), ('k > 256', ok, 257), ('1-D', sparse.coo_array(np.ones(300)), 4), ('NaN', nan, 4)]


@pytest.mark.parametrize('case', range(4))
@pytest.mark.parametrize('solver', ['exact', 'sinkhorn'])
def test_ot_cluster_refuses_bad_sparse_input_before_device_work(nv, monkeypatch, case, solver):
    from ultrare_amd.method import utils
    _no_device(monkeypatch)
    _, X, k = _bad_inputs()[case]
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):
        utils.ot_cluster(X, k, solver=solver, reg=1.0)
    assert np.array_equal(np.random.get_state()[1], state)          # and before any draw from the global generator


@pytest.mark.parametrize('case', range(4))
@pytest.mark.parametrize('var', ['rating-ot', 'rating-sinkhorn'])
def test_grouping_refuses_bad_sparse_input_before_device_work(nv, monkeypatch, tmp_path, case, var):
    from ultrare_amd.group import Group
    _no_device(monkeypatch)
    _, X, k = _bad_inputs()[case]
    with pytest.raises(ValueError):
        Group(X, 'bad', None).grouping('bad', k, var, verbose=False, data_dir=str(tmp_path))
    assert not os.path.exists(tmp_path / 'bad' / 'val' / f'{var}{k}.npy')


# ---- 5. the C entry points ------------------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(0x1000)                         # never dereferenced: every check fails before the device is touched


def _cost(nv, n=10, n_item=20, ldc=8, k=8, scratch_bytes=64, row_off=True, col=True, val=True, Ct=True, dist=True, scratch=True):
    f = lambda on: FAKE if on else None
    return nv.lib().ure_csr_cost(f(row_off), f(col), f(val), n, n_item, f(Ct), ldc, k, f(dist), f(scratch), scratch_bytes, None)


def _cent(nv, n=10, n_item=20, ldc=8, k=8, col_off=True, row=True, val=True, label=True, Ct=True, counts=True):
    f = lambda on: FAKE if on else None
    return nv.lib().ure_csr_centroids(f(col_off), f(row), f(val), f(label), n, n_item, k, f(Ct), ldc, f(counts), None)


@pytest.mark.parametrize('kw,word', [({'row_off': False}, 'row_off && col'), ({'col': False}, 'row_off && col'), ({'val': False}, 'row_off && col'),
                                     ({'Ct': False}, 'row_off && col'), ({'dist': False}, 'row_off && col'), ({'scratch': False}, 'scratch != nullptr'),
                                     ({'k': 0}, 'k >= 1'), ({'k': 257, 'ldc': 300, 'scratch_bytes': 4096}, 'k <= kCsrMaxK'),
                                     ({'ldc': 7}, 'ldc >= k'), ({'scratch_bytes': 63}, 'scratch_bytes >= need'), ({'scratch_bytes': 0}, 'scratch_bytes >= need'),
                                     ({'n': 0}, 'n >= 1'), ({'n': 1 << 31}, 'n <= INT32_MAX'), ({'n_item': 0}, 'n_item >= 1'),
                                     ({'n_item': 1 << 31}, 'n_item <= INT32_MAX')])
def test_csr_cost_rejects_bad_arguments(nv, kw, word):
    assert _cost(nv, **kw) == -1
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


@pytest.mark.parametrize('kw,word', [({'col_off': False}, 'col_off && row'), ({'row': False}, 'col_off && row'), ({'val': False}, 'col_off && row'),
                                     ({'label': False}, 'col_off && row'), ({'Ct': False}, 'col_off && row'), ({'counts': False}, 'col_off && row'),
                                     ({'k': 0}, 'k >= 1'), ({'k': 257, 'ldc': 300}, 'k <= kCsrMaxK'), ({'ldc': 7}, 'ldc >= k'),
                                     ({'n': 0}, 'n >= 1'), ({'n': 1 << 31}, 'n <= INT32_MAX'), ({'n_item': 0}, 'n_item >= 1'),
                                     ({'n_item': 1 << 31}, 'n_item <= INT32_MAX')])
def test_csr_centroids_rejects_bad_arguments(nv, kw, word):
    assert _cent(nv, **kw) == -1
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


def test_scratch_sizer_and_the_abi_number(nv):
    L = nv.lib()
    assert L.ure_abi_version() == 15 == nv.ABI_VERSION
    for k in (1, 5, 64, 65, 256):
        assert L.ure_csr_cost_scratch(k) == 8 * k
    for k in (0, -1, 257):
        assert L.ure_csr_cost_scratch(k) == -1


def test_engine_calls_refuse_cpu_tensors(nv):
    import types

    import torch
    from ultrare_amd import engine
    S = types.SimpleNamespace(n=4, n_item=6, device='cpu')
    with pytest.raises(nv.NativeError, match='HIP device only'):
        engine.csr_cost(S, torch.zeros(6, 2), 2)
    with pytest.raises(nv.NativeError, match='HIP device only'):
        engine.csr_centroids(S, torch.zeros(4, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match='k must'):
        engine.csr_cost(S, torch.zeros(6, 2), 257)
    with pytest.raises(ValueError, match='k must'):
        engine.csr_centroids(S, np.zeros(4, dtype=np.int64), 0)
    with pytest.raises(ValueError, match='label must'):
        engine.csr_centroids(S, np.array([0, 1, 2, 0]), 2)


def test_no_csr_kernel_spills(nv):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = [r for r in isa_report.kernels(nv.LIB_PATH) if r['name'].startswith('csr_')]
    assert len([r for r in rows if r['name'].startswith('csr_row_walk<OtCost,')]) == 7
    assert len([r for r in rows if r['name'].startswith('csr_col_walk<OtMean,')]) == 7
    for r in rows:
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, r


def test_the_command_line_admits_rating_ot_and_refuses_other_rating_variants():
    """--group-type: 'rating-ot' is in the help and passes the check; 'rating-sinkhorn' (needs a reg the command line cannot
    give) and 'rating-kmeans' are refused by the assertion before anything is imported or read."""
    from ultrare_amd import main as cli
    assert cli.parser.parse_args(['--group-type', 'rating-ot']).group_type == 'rating-ot'
    assert 'rating-ot' in cli.parser.format_help()
    for var in ('rating-sinkhorn', 'rating-kmeans'):
        with pytest.raises(AssertionError):
            cli.main(['--dataset', 'toy', '--group', '3', '--group-type', var])
