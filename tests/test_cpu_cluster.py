"""User-by-user distance clusterers, host side (-m "not gpu"): every new C ABI entry rejects bad arguments before any HIP
call, the kNN scratch follows its formula, the balanced descending assignment equals a numpy restatement of utils.py:484-497
(ties included), and the Python wrappers refuse malformed input before device work.  Nothing here initialises HIP."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope='session')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


FAKE = ctypes.c_void_p(0x1000)                         # never dereferenced: every check fails before the device is touched


def _fails(nv, rc, word):
    assert rc == -1
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


def _knn(nv, n=100, d=8, metric=1, n_query=10, n_nb=5, splits=0, dist=True, idx=True, scratch_bytes=None, src=True):
    L = nv.lib()
    if scratch_bytes is None:
        scratch_bytes = max(L.ure_pair_knn_scratch(n_query, n, n_nb, splits), 0)
    return L.ure_pair_knn(FAKE if src else None, n, d, metric, None, n_query, n_nb, splits, FAKE if dist else None, FAKE if idx else None,
                          FAKE, scratch_bytes, None)


@pytest.mark.parametrize('kw,word', [({'metric': 4}, 'metric_ok(metric)'), ({'metric': -1}, 'metric_ok(metric)'), ({'src': False}, 'src'),
                                     ({'n': 0}, 'n >= 1'), ({'n': 1 << 31}, 'n <= INT32_MAX'), ({'d': 0}, 'd >= 1'),
                                     ({'metric': 0, 'n': 1518500250, 'n_nb': 5, 'scratch_bytes': 1 << 40}, 'n <= kGivenMaxN'),
                                     ({'n_query': 0, 'scratch_bytes': 0}, 'n_query >= 1'), ({'n_nb': 0, 'scratch_bytes': 0}, 'n_nb >= 1'),
                                     ({'n_nb': 129, 'scratch_bytes': 1 << 30}, 'n_nb <= kPairMaxNb'),
                                     ({'n': 4, 'n_nb': 5, 'scratch_bytes': 1 << 20}, 'n_nb <= n'),
                                     ({'splits': -1, 'scratch_bytes': 1 << 20}, 'splits >= 0'),
                                     ({'dist': False}, 'dist && idx'), ({'idx': False}, 'dist && idx'),
                                     ({'scratch_bytes': 10 * 5 * 8 - 1, 'splits': 1}, 'scratch_bytes >= ure_pair_knn_scratch')])
def test_pair_knn_rejects_bad_arguments(nv, kw, word):
    _fails(nv, _knn(nv, **kw), word)


def test_given_path_takes_any_d(nv):
    # d is ignored for a given array: the call fails only on the missing output, not on d
    _fails(nv, _knn(nv, metric=0, d=0, dist=False), 'dist && idx')


def test_pair_reductions_reject_bad_arguments(nv):
    L = nv.lib()
    _fails(nv, L.ure_pair_rowsum(FAKE, 100, 8, 7, FAKE, None), 'metric_ok(metric)')
    _fails(nv, L.ure_pair_rowsum(FAKE, 100, 8, 1, None, None), 'R')
    _fails(nv, L.ure_pair_rowsum(FAKE, 0, 8, 1, FAKE, None), 'n >= 1')
    _fails(nv, L.ure_pair_rowsum(FAKE, 1518500250, 8, 0, FAKE, None), 'n <= kGivenMaxN')
    _fails(nv, L.ure_pair_cols(FAKE, 100, 8, 2, FAKE, 0, FAKE, None), 'cols && m >= 1')
    _fails(nv, L.ure_pair_cols(FAKE, 100, 8, 2, None, 3, FAKE, None), 'cols && m >= 1')
    _fails(nv, L.ure_pair_cols(FAKE, 100, 8, 2, FAKE, 3, None, None), 'out')
    _fails(nv, L.ure_pair_cols(FAKE, 100, 0, 3, FAKE, 3, FAKE, None), 'd >= 1')
    _fails(nv, L.ure_pair_label_expsum(FAKE, 100, 8, 1, FAKE, 0, FAKE, None), 'k >= 1')
    _fails(nv, L.ure_pair_label_expsum(FAKE, 100, 8, 1, FAKE, 129, FAKE, None), 'k <= kPairMaxGroups')
    _fails(nv, L.ure_pair_label_expsum(FAKE, 100, 8, 1, None, 4, FAKE, None), 'label')
    _fails(nv, L.ure_pair_label_expsum(FAKE, 100, 8, 1, FAKE, 4, None, None), 'W')
    _fails(nv, L.ure_pair_label_expsum(FAKE, 100, 8, 5, FAKE, 4, FAKE, None), 'metric_ok(metric)')


def _splits(n_query, n, want):
    col_tiles, row_tiles = -(-n // 64), -(-n_query // 64)
    s = want if want > 0 else -(-1024 // row_tiles)
    s = max(1, min(s, col_tiles, 64))
    per = -(-col_tiles // s)
    return -(-col_tiles // per)


def test_knn_scratch_formula(nv):
    L = nv.lib()
    for nq, n, nb, sp in [(1, 1, 1, 0), (10, 100, 5, 0), (10, 100, 5, 1), (10, 100, 5, 3), (64, 6040, 10, 0), (162000, 162000, 10, 0),
                          (5, 162000, 128, 0), (5, 162000, 128, 7), (1000, 4099, 128, 2), (3, 4099, 128, 1000)]:
        want = nq * nb * 8 * _splits(nq, n, sp)
        assert L.ure_pair_knn_scratch(nq, n, nb, sp) == want, (nq, n, nb, sp)
    assert L.ure_pair_knn_scratch(162000, 162000, 10, 0) == 162000 * 10 * 8          # enough rows: one split, never n * n
    assert L.ure_pair_knn_scratch(1, 162000, 10, 0) == 10 * 8 * 64                   # one query: at most 64 splits
    for args in [(0, 10, 5, 0), (10, 0, 1, 0), (10, 10, 0, 0), (10, 10, 129, 0), (10, 4, 5, 0), (10, 10, 5, -1), (10, 1 << 31, 5, 0)]:
        assert L.ure_pair_knn_scratch(*args) == -1, args


def _assign_desc_numpy(W, cap):
    """utils.py:484-497 restated: pairs in np.argsort(W, axis=None)[::-1] order (stable ascending: ties by ascending flat index,
    reversed), each user its first group with room."""
    n, k = W.shape
    order = np.argsort(W, axis=None, kind='stable')[::-1]
    label, left, done = np.zeros(n, dtype=np.int64), [cap] * k, np.zeros(n, dtype=bool)
    for t in order:
        u, g = divmod(int(t), k)
        if done[u] or left[g] <= 0:
            continue
        label[u], done[u] = g, True
        left[g] -= 1
    return label, np.sum(W[np.arange(n), label])


@pytest.mark.parametrize('n,k,ties', [(1, 1, False), (7, 3, True), (100, 4, True), (1508, 5, False), (1508, 4, True), (9001, 3, True),
                                      (20000, 7, False)])
def test_assign_desc_matches_numpy(nv, n, k, ties):
    rng = np.random.default_rng(n * 31 + k)
    W = rng.random((n, k)) * 100
    if ties:                                             # exact ties inside rows, across rows and whole duplicated rows
        W = np.round(W / 10) * 10
        W[n // 2:n // 2 + n // 4] = W[:n // 4]
    W = np.ascontiguousarray(W)
    cap = int(np.ceil(n / k))
    want_label, want_inertia = _assign_desc_numpy(W, cap)
    label, inertia = np.empty(n, dtype=np.int32), ctypes.c_double(0.0)
    assert nv.lib().ure_host_assign_desc_f64(W.ctypes.data, n, k, cap, label.ctypes.data, ctypes.byref(inertia)) == 0
    np.testing.assert_array_equal(label, want_label)
    assert inertia.value == want_inertia                 # np.sum's float64 order, bit for bit (n > 8192: its buffers)
    assert np.bincount(label, minlength=k).max() <= cap


def test_assign_desc_rejects_bad_arguments(nv):
    L = nv.lib()
    W, lab = np.zeros((4, 2)), np.zeros(4, dtype=np.int32)
    _fails(nv, L.ure_host_assign_desc_f64(None, 4, 2, 2, lab.ctypes.data, None), 'w && label')
    _fails(nv, L.ure_host_assign_desc_f64(W.ctypes.data, 0, 2, 2, lab.ctypes.data, None), 'n >= 1 && k >= 1')
    _fails(nv, L.ure_host_assign_desc_f64(W.ctypes.data, 4, 0, 2, lab.ctypes.data, None), 'n >= 1 && k >= 1')
    _fails(nv, L.ure_host_assign_desc_f64(W.ctypes.data, 4, 2, 1, lab.ctypes.data, None), 'capacity * k >= n')


def test_wrappers_check_input_before_device_work(tmp_path):
    from ultrare_amd.method import utils as U
    D = np.zeros((6, 6), dtype=np.float32)
    with pytest.raises(TypeError):
        U.kmedoids(2, 6, D.astype(np.float64))
    with pytest.raises(TypeError):
        U.lpa(2, 6, D.astype(np.float16))
    with pytest.raises(ValueError):
        U.kmedoids(2, 6, np.zeros((6, 5), dtype=np.float32))            # not square
    with pytest.raises(ValueError):
        U.singleKmedoids(7, 6, D, False, 10)                            # k > n
    with pytest.raises(ValueError):
        U.singleLPA(0, 6, D, False, 10)
    with pytest.raises(ValueError):
        U.lpa(2, 5, D)                                                  # n_user does not match
    with pytest.raises(ValueError):
        U.lpa(129, 200, np.zeros((200, 3), dtype=np.float32), metric='euclidean')   # more groups than the kernel keeps
    with pytest.raises(ValueError):
        U.kmedoids(2, 6, np.zeros((6, 3), dtype=np.float32), metric='chebyshev')
    with pytest.raises(ValueError):
        U.kmedoids(2, 6, np.zeros(6, dtype=np.float32), metric='euclidean')       # X must be 2-D
    with pytest.raises(ValueError):
        U.findNeighbor(str(tmp_path) + '/', np.zeros((6, 3), dtype=np.float32), 6, var='chebyshev')
    with pytest.raises(ValueError):
        U.findNeighbor(str(tmp_path) + '/', np.zeros((6, 3), dtype=np.float32), 7)


def test_kmedoids_empty_cluster_raises(monkeypatch):
    """The host logic of singleKmedoids with the device reductions restated in numpy: users 0 and 1 coincide, so when both
    are medoids the later one's cluster is empty after the first assignment -- ValueError, where the reference fails on
    argmin of an empty array."""
    from ultrare_amd import engine
    from ultrare_amd.method import utils as U
    x = np.array([0., 0., 10., 20.], dtype=np.float32)
    D = np.abs(x[:, None] - x[None, :]).astype(np.float32)
    monkeypatch.setattr(engine, 'pair_source', lambda src, metric=None: (src, src.shape[0], src.shape[1], 0))
    monkeypatch.setattr(engine, 'pair_rowsum', lambda src, metric=None: _Host(np.sum(src, axis=1)))
    monkeypatch.setattr(engine, 'pair_cols', lambda src, cols, metric=None: _Host(src[:, np.asarray(cols)]))
    seed = next(s for s in range(1000) if set(np.random.RandomState(s).choice(4, 3, replace=False)) == {0, 1, 2})
    np.random.seed(seed)
    with pytest.raises(ValueError, match='lost all its members'):
        U.singleKmedoids(3, 4, D, False, 10)


class _Host:
    """Stands in for a device tensor in the monkeypatched test: .cpu().numpy() gives the array back."""
    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


# ---- the shapes of the GPU bit tests can tell numpy's summation rules apart (on the numpy installed here) -------------------
def _np_leaf(a):
    """numpy's pairwise_sum of at most 128 float32 values: below 8 one after the other from 0, else eight accumulators."""
    if len(a) < 8:
        res = np.float32(0)
        for v in a:
            res = res + v
        return res
    r = a[:8].copy()
    full = len(a) - len(a) % 8
    for i in range(8, full, 8):
        r = r + a[i:i + 8]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[full:]:
        res = res + v
    return res


def _np_pairwise(a):
    """One pairwise sum over the whole run: halves (the first a multiple of 8) down to leaves of at most 128."""
    if len(a) <= 128:
        return _np_leaf(a)
    h = len(a) // 2
    h -= h % 8
    return _np_pairwise(a[:h]) + _np_pairwise(a[h:])


def _one_split(a):
    """The rule ure_ot_cost had before: a row longer than 128 split once, both halves taken as leaves."""
    if len(a) <= 128:
        return _np_leaf(a)
    h = len(a) // 2
    h -= h % 8
    return _np_leaf(a[:h]) + _np_leaf(a[h:])


@pytest.mark.parametrize('n', [8193, 8261, 16391, 20000])
def test_numpy_row_sums_past_8192_are_not_one_pairwise_sum(n):
    """np.sum(A, axis=1) of float32 rows longer than 8192 adds the pairwise sums of buffers of 8192 values in order; a single
    pairwise sum over the row gives other bits somewhere in a few rows, so tests/test_gpu_cluster.py's row-sum shapes would
    catch a kernel that ignored the buffers."""
    A = np.abs(np.random.default_rng(n).standard_normal((6, n))).astype(np.float32)
    got = np.sum(A, axis=1)
    buffered = np.array([sum((_np_pairwise(row[i:i + 8192]) for i in range(0, n, 8192)), np.float32(0)) for row in A])
    single = np.array([_np_pairwise(row) for row in A])
    assert buffered.dtype == np.float32 and single.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), buffered.view(np.uint32))
    assert (got.view(np.uint32) != single.view(np.uint32)).any()


@pytest.mark.parametrize('d,differs', [(248, False), (249, True), (255, True), (256, False)])
def test_numpy_cost_rows_of_249_to_255_split_twice(d, differs):
    """utils.py:637's row sums follow numpy's full rule; for d = 249 .. 255 the second half (129 .. 135 terms) is split again,
    so the one-split rule gives other bits there and the same bits at 248 and 256."""
    rs = np.random.RandomState(d)
    X = rs.standard_normal((300, d)).astype(np.float32)
    C = rs.standard_normal((4, d)).astype(np.float32)
    T = (X - C[:, np.newaxis]) ** 2
    got = T.sum(axis=2)
    full = np.array([[_np_pairwise(row) for row in block] for block in T])
    once = np.array([[_one_split(row) for row in block] for block in T])
    assert np.array_equal(got.view(np.uint32), full.view(np.uint32))
    assert (got.view(np.uint32) != once.view(np.uint32)).any() == differs
