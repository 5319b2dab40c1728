"""The pair-distance clusterers on the sparse rating matrix, host side: the union walk of ultrare_amd/sparse_pair.py against
float64 distances of the densified matrix, the refusals that come before any device work, how _pair_input and findNeighbor
route their input, the command line's group types, and the classification of the new C entries."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ('euclidean', 'cosine', 'manhattan')


def crafted():
    """41 users x 90 items: rows 0 and 40 empty, row 1 holds one entry, row 2 every item, rows 5 and 6 identical, rows 7 and
    8 on disjoint columns, row 9 only stored zeros, and a dozen stored zeros (one of them -0.0) elsewhere."""
    from scipy import sparse
    rs = np.random.RandomState(11)
    n, n_item = 41, 90
    X = np.where(rs.rand(n, n_item) < 0.15, rs.randint(1, 11, (n, n_item)) / 2.0, 0.0).astype(np.float32)
    X[0] = X[40] = X[9] = 0
    X[1] = 0
    X[1, 17] = 3.5
    X[2] = rs.randint(1, 11, n_item) / 2.0
    X[6] = X[5]
    X[7, 45:] = 0
    X[8, :45] = 0
    mask = X != 0
    zr, zc = rs.randint(10, 40, 12), rs.randint(0, n_item, 12)          # stored zeros
    mask[zr, zc] = True
    mask[9, [3, 50]] = True
    r, c = np.nonzero(mask)
    v = X[r, c].copy()
    v[np.flatnonzero(v == 0)[:1]] = -0.0
    mat = sparse.csr_matrix((v, (r, c)), shape=(n, n_item))
    assert mat.nnz == mask.sum() and (mat.data == 0).sum() >= 3
    return mat, X


def dense_f64(X, metric):
    X = X.astype(np.float64)
    t = X[:, None, :] - X[None, :, :]
    if metric == 'euclidean':
        return np.sqrt((t * t).sum(-1))
    if metric == 'manhattan':
        return np.abs(t).sum(-1)
    nrm = np.sqrt((X * X).sum(-1))
    den = nrm[:, None] * nrm[None, :]
    with np.errstate(invalid='ignore', divide='ignore'):
        D = np.where(den == 0, 1.0, np.clip(1.0 - (X @ X.T) / den, 0.0, 2.0))
    D[np.arange(len(X)), np.arange(len(X))] = 0.0
    return D


@pytest.mark.parametrize('metric', METRICS)
def test_the_union_walk_equals_float64_distances_of_the_densified_matrix(metric):
    from ultrare_amd import sparse_pair as sp
    mat, X = crafted()
    rows = np.arange(X.shape[0])
    D = sp.pair_dist_csr_ref(mat, rows, rows, metric)
    want = dense_f64(X, metric)
    # both are float64 sums of the same non-zero terms in another order (numpy's pairwise sum against the walk's sequential
    # one): at most 90 terms, so 90 ulp of the largest partial sum is a generous bound; identical and zero terms are exact
    np.testing.assert_allclose(D, want, rtol=90 * 2.3e-16, atol=90 * 2.3e-16 * np.abs(want).max())
    assert (np.diag(D) == 0).all() and (D == D.T).all()
    assert D[5, 6] == 0 or metric == 'cosine' and D[5, 6] <= 2.3e-16            # identical rows
    if metric == 'cosine':
        assert (D[0, 1:] == 1).all() and (D[9, 10:] == 1).all() and D[0, 40] == 1 and D[7, 8] == 1    # empty, all-zero, disjoint rows
    halves = __import__('ultrare_amd.sparse_group', fromlist=['x']).canonical_csr(mat)
    sub = sp.pair_dist_csr_ref(halves, [2, 40, 7], [8, 2], metric)              # the (csr, csc) pair; a rectangle
    assert (sub == D[np.ix_([2, 40, 7], [8, 2])]).all()


def test_refusals_come_before_any_device_work(monkeypatch):
    from scipy import sparse
    from ultrare_amd import engine
    from ultrare_amd import sparse_pair as sp
    from ultrare_amd.group import Group
    from ultrare_amd.method import utils
    monkeypatch.setattr(engine, '_device', lambda: pytest.fail('device work before the refusal'))
    monkeypatch.setattr(engine, 'CsrSet', lambda *a, **k: pytest.fail('an upload before the refusal'))
    mat, _ = crafted()
    wide = sparse.csr_matrix((np.ones(3, np.float32), ([0, 1, 2], [0, 5, 299])), shape=(41, 300))
    halves = sp.check_pair_args(wide, 'euclidean', 41, 5, 128)
    assert halves[0].shape == (41, 300)
    with pytest.raises(ValueError, match='no CSR form'):
        sp.check_pair_args(wide, None)
    for call in (lambda: utils.kmedoids(3, 41, wide, metric=None), lambda: utils.lpa(3, 41, wide, metric=None),
                 lambda: utils.singleKmedoids(3, 41, halves, False, 3, metric=None)):
        with pytest.raises(ValueError, match='no CSR form'):
            call()
    with pytest.raises(ValueError, match="'euclidean' / 'cosine' / 'manhattan'"):
        sp.check_pair_args(wide, 'chebyshev')
    bad = wide.copy()
    bad.data[1] = np.inf
    with pytest.raises(ValueError, match='non-finite'):
        utils.kmedoids(3, 41, bad, metric='euclidean')
    with pytest.raises(ValueError, match='non-finite'):
        utils.findNeighbor('unused', bad, 41, 'cosine')
    with pytest.raises(ValueError, match='2-D'):
        utils.lpa(3, 41, sparse.coo_array(np.ones(300, np.float32)), metric='euclidean')
    with pytest.raises(ValueError, match='n_user = 40'):
        utils.kmedoids(3, 40, wide, metric='euclidean')
    with pytest.raises(ValueError, match='n_user = 40'):
        utils.findNeighbor('unused', halves, 40, 'euclidean')
    with pytest.raises(ValueError, match='1 <= k <= n'):
        utils.kmedoids(42, 41, wide, metric='manhattan')
    with pytest.raises(ValueError, match='at most 128'):
        utils.lpa(129, 200, sparse.csr_matrix((200, 300), dtype=np.float32), metric='euclidean')
    with pytest.raises(ValueError, match='non-finite'):
        Group(bad, 'toy').grouping('toy', 3, 'rating-bkmedoids', verbose=False, data_dir=os.path.join(ROOT, 'tests', 'no-such-dir'))


def test_pair_input_routes_by_width_and_by_input_type(monkeypatch):
    from scipy import sparse
    from ultrare_amd import engine
    from ultrare_amd import sparse_group as sg
    from ultrare_amd.group import DENSE_MAX_ITEMS
    from ultrare_amd.method import utils
    seen = []
    monkeypatch.setattr(engine, 'CsrSet', lambda halves: seen.append(('csr', halves[0].shape)) or 'a CsrSet')
    monkeypatch.setattr(engine, 'pair_source', lambda arr, metric: (seen.append(('dense', type(arr).__name__, tuple(arr.shape))) or 'a tensor',))
    rs = np.random.RandomState(0)
    wide = sparse.random(30, DENSE_MAX_ITEMS + 1, density=0.05, random_state=rs, format='csr', dtype=np.float32)
    edge = sparse.random(30, DENSE_MAX_ITEMS, density=0.05, random_state=rs, format='csr', dtype=np.float32)
    assert utils._pair_input(3, 30, wide, 'euclidean') == 'a CsrSet' and seen.pop() == ('csr', (30, DENSE_MAX_ITEMS + 1))
    assert utils._pair_input(3, 30, wide.tocoo(), 'cosine') == 'a CsrSet' and seen.pop() == ('csr', (30, DENSE_MAX_ITEMS + 1))
    assert utils._pair_input(3, 30, edge, 'euclidean') == 'a tensor' and seen.pop() == ('dense', 'ndarray', (30, DENSE_MAX_ITEMS))
    assert utils._pair_input(3, 30, sg.canonical_csr(edge), 'manhattan') == 'a CsrSet' and seen.pop() == ('csr', (30, DENSE_MAX_ITEMS))   # a pair: always
    X = np.zeros((30, 1000), dtype=np.float32)
    assert utils._pair_input(3, 30, X, 'euclidean') == 'a tensor' and seen.pop() == ('dense', 'ndarray', (30, 1000))                  # an array: never
    G = np.zeros((30, 30), dtype=np.float32)
    assert utils._pair_input(3, 30, G, None) == 'a tensor' and seen.pop() == ('dense', 'ndarray', (30, 30))
    assert not seen


def test_the_window_constant_mirrors_the_kernel_and_the_new_entries_are_declared_and_classified():
    from ultrare_amd import _native as nv
    from ultrare_amd import sparse_pair as sp
    L = nv.lib()
    assert L.ure_csr_pair_window() == sp.WINDOW
    src = open(os.path.join(ROOT, 'ultrare_amd', 'csrc', 'pair_dist.hip')).read()
    assert re.search(r'constexpr int kCsrPairWindow = (\d+);', src).group(1) == str(sp.WINDOW)
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ultrare_csr_pair.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.CSR_PAIR_EXPORTS) and not declared & set(nv.EXPORTS)
    raw = ctypes.CDLL(nv.LIB_PATH)
    assert all(hasattr(raw, name) for name in declared)
    assert '#include "ultrare_csr_pair.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    # every name has a memory class in tests/test_gpu_sparse_pair.py, and every 'arena' name a guard-zone case there
    import test_gpu_sparse_pair as G
    assert set(G.INVENTORY) == declared
    assert {e for e, klass in G.INVENTORY.items() if klass == 'arena'} == {c[1] for c in G.ARENA_CASES}
    assert {e for e, klass in G.INVENTORY.items() if klass == 'sizer'} == {'ure_csr_pair_knn_scratch'}
    # the sizer refuses what the entry refuses, and is linear in n_query * n_nb * splits
    assert L.ure_csr_pair_knn_scratch(130, 130, 0, 0) == -1 and L.ure_csr_pair_knn_scratch(130, 130, 129, 0) == -1
    assert L.ure_csr_pair_knn_scratch(5, 4, 5, 0) == -1 and L.ure_csr_pair_knn_scratch(0, 4, 1, 0) == -1
    assert L.ure_csr_pair_knn_scratch(64, 20000, 10, 1) == 64 * 10 * 8
    assert L.ure_csr_pair_knn_scratch(64, 20000, 10, 10 ** 6) == 64 * 10 * 8 * 63       # 313 column tiles, 5 a split at the cap of 64: 63 splits
    assert L.ure_csr_pair_knn_scratch(64, 20000, 10, 7) == L.ure_pair_knn_scratch(64, 20000, 10, 7)


def test_the_command_line_accepts_the_two_balanced_group_types():
    from ultrare_amd import main as cli
    text = open(cli.__file__).read()
    for name in ('rating-bkmedoids', 'rating-blpa'):
        assert cli.parser.parse_args(['--group-type', name]).group_type == name
        assert name in re.sub(r'\s+', '', cli.parser.format_help())           # (argparse wraps at hyphens)
        assert re.search(r"assert args\.group_type in \[[^\]]*'" + name + "'", text)
