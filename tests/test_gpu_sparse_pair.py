"""The pair-distance reductions on the sparse rating matrix, device side.  The bit contract is the dense device route on the
densified matrix: kNN, row sums, columns and label-grouped exp sums from an engine.CsrSet equal those from the array BIT
FOR BIT, for the three streamed metrics, at the tile edges, with item ids beyond 16 bits, on empty, one-entry, identical,
disjoint and full rows and rows longer than the staging window, on grid and arbitrary values with stored +-0.0.  Then the
clusterers end to end against the dense route, peak memory, the raw entries inside guard zones, refusals and the torch op."""
import os

import numpy as np
import pytest
import torch

from abi_arena import Arena, run_prefills, verdict

pytestmark = pytest.mark.gpu

METRICS = ('euclidean', 'cosine', 'manhattan')
NS = (1, 63, 65, 130)                       # one row; a ragged tile; a tile and one row; two tiles and two rows
N_ITEMS = (300, 70000)                      # one window's worth of ids; ids beyond 16 bits

# memory classes of the names of include/ultrare_csr_pair.h (tests/test_cpu_sparse_pair.py holds this table to the binding)
INVENTORY = {
    'ure_csr_pair_window': 'host', 'ure_csr_pair_knn_scratch': 'sizer',
    'ure_csr_pair_knn': 'arena', 'ure_csr_pair_rowsum': 'arena', 'ure_csr_pair_cols': 'arena', 'ure_csr_pair_label_expsum': 'arena',
}
_CASES = {}


def build_case(n, n_item, values):
    """(scipy csr, dense float32 [n, n_item]) from one seed.  Row 0 stores column 0 and column n_item - 1; row 1 is empty;
    row 2 holds one entry; row 3 is 3 windows and 5 entries long; row 4 stores every item at n_item = 300 (7 windows
    otherwise); rows 5 and 6 are identical; rows 7 and 8 live on disjoint halves of the items; the others hold 1 .. 40
    entries.  values 'grid': half stars 0.5 .. 5; 'float': arbitrary float32 with stored 0.0 and -0.0."""
    key = (n, n_item, values)
    if key in _CASES:
        return _CASES[key]
    from scipy import sparse
    from ultrare_amd.sparse_pair import WINDOW
    rs = np.random.RandomState(20240 + n_item % 7)
    rows, cols = [], []
    for u in range(n):
        m = int(rs.randint(1, 41))
        pool = n_item
        if u == 1:
            m = 0
        elif u == 2:
            m = 1
        elif u == 3:
            m = 3 * WINDOW + 5
        elif u == 4:
            m = n_item if n_item == 300 else 7 * WINDOW
        c = np.sort(rs.choice(pool, m, replace=False))
        if u == 0:
            c = np.unique(np.concatenate([[0, n_item - 1], c]))
        if u == 7:
            c = np.unique(c // 2)
        if u == 8:
            c = np.unique(n_item // 2 + c // 2)
        if u == 6:
            c = cols[5]
        rows.append(np.full(len(c), u))
        cols.append(c)
    r, c = np.concatenate(rows), np.concatenate(cols)
    if values == 'grid':
        v = (rs.randint(1, 11, len(r)) / 2.0).astype(np.float32)
    else:
        v = (rs.standard_normal(len(r)) * np.exp(rs.uniform(-3, 3, len(r)))).astype(np.float32)
        z = rs.choice(len(v), max(len(v) // 20, min(2, len(v))), replace=False)
        v[z[::2]] = 0.0
        v[z[1::2]] = -0.0
    if n > 6:
        v[r == 6] = v[r == 5]
    mat = sparse.csr_matrix((v, (r, c)), shape=(n, n_item))
    mat.sort_indices()
    assert mat.nnz == len(v)                                                    # stored zeros stay stored
    X = np.zeros((n, n_item), dtype=np.float32)
    X[r, c] = v                                                                  # (-0.0 densifies to -0.0: the dense route sees it too)
    lens = np.diff(mat.indptr)
    assert X[0, 0] == mat[0, 0] and mat.indices[0] == 0 and mat.indices[mat.indptr[1] - 1] == n_item - 1
    if n > 8:
        assert lens[1] == 0 and lens[2] == 1 and lens[3] > 3 * WINDOW and lens[4] > WINDOW and (n_item != 300 or lens[4] == 300)
        assert (X[5] == X[6]).all() and lens[5] > 0 and not ((X[7] != 0) & (X[8] != 0)).any()
    if values == 'float' and n > 8:
        assert (mat.data == 0).sum() >= 2 and np.signbit(mat.data[mat.data == 0]).any()
    _CASES[key] = (mat, X)
    return mat, X


def same(a, b):
    """Equal shape, dtype and bytes (floats compared as integers: -0.0 and NaN by pattern)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    as_int = {torch.float32: torch.int32, torch.float64: torch.int64}.get(a.dtype)
    return torch.equal(a.view(as_int), b.view(as_int)) if as_int else torch.equal(a, b)


@pytest.fixture(scope='module')
def sources():
    """(n, n_item, values) -> (CsrSet, dense device tensor), uploaded once per module."""
    from ultrare_amd import engine
    made = {}

    def get(n, n_item, values):
        key = (n, n_item, values)
        if key not in made:
            mat, X = build_case(n, n_item, values)
            made.clear()                                                         # one 36 MB array at a time
            made[key] = (engine.CsrSet(mat), torch.from_numpy(X).cuda())
        return made[key]
    return get


# ---- 1. the four reductions, bit for bit against the dense route --------------------------------------------------------------
@pytest.mark.parametrize('values', ('grid', 'float'))
@pytest.mark.parametrize('n_item', N_ITEMS)
@pytest.mark.parametrize('n', NS)
def test_every_reduction_equals_the_dense_route_bit_for_bit(sources, n, n_item, values):
    from ultrare_amd import engine
    S, Xd = sources(n, n_item, values)
    query = np.array([n - 1, 0, n // 2, 5 % n, 5 % n, 6 % n, 64 % n])
    cols = np.array([n - 1, 0, n // 2, 0])                                       # a repeated column
    for metric in METRICS:
        # kNN: every row with automatic splits; a query list at 1 split and at the maximum; the widest list
        for q, n_nb, splits in ((None, min(n, 10), 0), (query, min(n, 10), 1), (query, min(n, 10), 64), (None, min(n, 128), 1)):
            got, want = engine.pair_knn(S, n_nb, metric, q, splits), engine.pair_knn(Xd, n_nb, metric, q, splits)
            assert same(got[0], want[0]) and same(got[1], want[1]), (metric, n_nb, splits)
        assert same(engine.pair_rowsum(S, metric), engine.pair_rowsum(Xd, metric)), metric
        assert same(engine.pair_cols(S, cols, metric), engine.pair_cols(Xd, cols, metric)), metric
        for k in (1, 128):
            label = (np.arange(n) * 7 + 3) % k
            assert same(engine.pair_label_expsum(S, label, k, metric), engine.pair_label_expsum(Xd, label, k, metric)), (metric, k)


@pytest.mark.parametrize('metric', METRICS)
def test_symmetry_zero_diagonal_ties_and_the_float64_yardstick(sources, metric):
    """The whole D of the 130 x 300 case: symmetric and zero on the diagonal to the bit, the identical rows 5 and 6 at
    distance 0 with the tie broken by id, and within rounding of the union walk in float64 (sparse_pair.pair_dist_csr_ref).
    A float32 accumulator over m <= 300 terms: each fmaf / add rounds once (relative 2^-24 of a partial sum that the sum of
    the absolute terms bounds), the difference x - y once more (doubled by the square), sqrt / divide / the norms a few
    more: (2 m + 8) 2^-24, relative to the distance for the sums of non-negative terms, to 1 for the cosine, whose
    dot product is bounded by the product of the norms."""
    from ultrare_amd import engine
    from ultrare_amd.sparse_pair import pair_dist_csr_ref
    n, n_item = 130, 300
    for values in ('grid', 'float'):
        S, _ = sources(n, n_item, values)
        D = engine.pair_cols(S, np.arange(n), metric)
        assert same(D, D.T.contiguous()) and (torch.diagonal(D) == 0).all()
        dist, idx = engine.pair_knn(S, 3, metric, [5, 6])
        if metric != 'cosine':
            assert D[5, 6] == 0 and idx[:, :2].tolist() == [[5, 6], [5, 6]] and (dist[:, :2] == 0).all()
        else:
            assert (D[1, 2:] == 1).all() and D[7, 8] == 1                       # the empty row, disjoint rows
        rows = np.array([0, 1, 2, 3, 4, 5, 7, 8, 64, 129])
        ref = pair_dist_csr_ref(S.csr, rows, np.arange(n), metric)
        got = D.cpu().numpy().astype(np.float64)[rows]
        bound = (2 * n_item + 8) * 2.0 ** -24 * (np.ones_like(ref) if metric == 'cosine' else ref)
        assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) - bound).max())


# ---- 2. the clusterers end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ratings():
    """200 users x 400 items (wider than group.DENSE_MAX_ITEMS), about 25 half-star ratings a user."""
    from scipy import sparse
    rs = np.random.RandomState(77)
    mat = sparse.random(200, 400, density=0.06, random_state=rs, format='csr', dtype=np.float32)
    mat.data[:] = rs.randint(1, 11, mat.nnz) / 2.0
    return mat, np.ascontiguousarray(mat.toarray(), dtype=np.float32)


@pytest.mark.parametrize('balanced', (False, True))
def test_kmedoids_and_lpa_on_the_csr_return_the_dense_routes_labels(ratings, balanced):
    from ultrare_amd.method import utils
    mat, X = ratings
    for fn, metric in ((utils.kmedoids, 'euclidean'), (utils.kmedoids, 'cosine'), (utils.lpa, 'euclidean'), (utils.lpa, 'manhattan')):
        out = []
        for src in (mat, X):
            np.random.seed(1234)
            out.append(fn(4, 200, src, balanced=balanced, n_init=2, max_iter=6, metric=metric))
        assert out[0] is not None and (out[0] == out[1]).all(), (fn.__name__, metric)
        if balanced:
            assert np.bincount(out[0], minlength=4).max() <= 50


def test_find_neighbor_writes_the_same_cache_file(ratings, tmp_path):
    from ultrare_amd.method import utils
    mat, X = ratings
    for var in METRICS:
        a = utils.findNeighbor(str(tmp_path) + '/csr_', mat, 200, var, 10)
        b = utils.findNeighbor(str(tmp_path) + '/dense_', X, 200, var, 10)
        assert (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()
        with open(f'{tmp_path}/csr_{var}.npy', 'rb') as f, open(f'{tmp_path}/dense_{var}.npy', 'rb') as g:
            assert f.read() == g.read()


@pytest.mark.parametrize('var', ('rating-bkmedoids', 'rating-blpa'))
def test_group_grouping_streams_the_sparse_rows(ratings, tmp_path, var, monkeypatch):
    from ultrare_amd import group
    from ultrare_amd.method import utils
    mat, X = ratings
    monkeypatch.setattr(group, '_dense_f32', lambda *_: pytest.fail('the rating matrix was densified'))
    np.random.seed(99)
    res = group.Group(mat, 'toy').grouping('toy', 4, var, verbose=False, data_dir=str(tmp_path))
    assert sorted(u for g in res for u in g) == list(range(200)) and [len(g) for g in res] == [50] * 4
    np.random.seed(99)
    fn = utils.kmedoids if var == 'rating-bkmedoids' else utils.lpa
    want = fn(4, 200, X, balanced=True, metric='euclidean')
    assert res == [np.flatnonzero(want == g).tolist() for g in range(4)]
    assert os.path.exists(f'{tmp_path}/toy/val/{var}4.npy')


# ---- 3. memory -------------------------------------------------------------------------------------------------------------------
def test_knn_at_20000_users_by_60000_items_allocates_no_dense_array():
    """64 query rows against 20,000 users over 60,000 items, 40 ratings a user: the peak over upload and call stays within the
    CSR's bytes, the outputs, the sizer's scratch and 1 MiB; the dense input alone would be 4.8 GB."""
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    n, n_item, per, nq, n_nb = 20000, 60000, 40, 64, 10
    rs = np.random.RandomState(3)
    col = np.sort(rs.randint(0, n_item // per, (n, per)) + np.arange(per) * (n_item // per), axis=1).astype(np.int32).reshape(-1)
    val = (rs.randint(1, 11, n * per) / 2.0).astype(np.float32)
    off = np.arange(n + 1, dtype=np.int64) * per
    query = rs.choice(n, nq, replace=False)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    S = engine.CsrSet.from_device(n, n_item, torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda())
    dist, idx = engine.pair_knn(S, n_nb, 'euclidean', query)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    scratch = int(nv.lib().ure_csr_pair_knn_scratch(nq, n, n_nb, 0))
    outputs = nq * n_nb * (4 + 4 + 8) + nq * 4                                   # dist, idx (int32 and the int64 copy), the query ids
    assert 0 < scratch <= nq * n_nb * 8 * 64
    assert peak <= off.nbytes + col.nbytes + val.nbytes + outputs + scratch + (1 << 20), peak
    assert n * n_item * 4 == 4.8e9
    assert idx[:, 0].cpu().tolist() == query.tolist() and (dist[:, 0] == 0).all() and (dist[:, 1] > 0).all()


# ---- 4. the raw entries on dirty memory inside guard zones -----------------------------------------------------------------
def _arena_inputs(A):
    mat, _ = build_case(130, 300, 'float')
    A.input('row_off', mat.indptr.astype(np.int64))
    A.input('col', mat.indices.astype(np.int32))
    A.input('val', mat.data.astype(np.float32))
    return mat, 130, 300


def _head(A, n, n_item, code):
    return (A.addr('row_off'), A.addr('col'), A.addr('val'), n, n_item, code)


def case_knn(A, metric, splits, with_query):
    from ultrare_amd import _native as nv, engine
    mat, n, n_item = _arena_inputs(A)
    n_nb = 10
    query = np.array([129, 0, 64, 63, 5, 5], dtype=np.int32) if with_query else None
    nq = n if query is None else len(query)
    if with_query:
        A.input('query', query)
    A.output('dist', nq * n_nb * 4)
    A.output('idx', nq * n_nb * 4)
    nbytes = int(nv.lib().ure_csr_pair_knn_scratch(nq, n, n_nb, splits))
    assert nbytes > 0
    A.scratch('ws', nbytes)                                                      # exactly the sizer's bytes
    code = engine.PAIR_METRICS[metric]

    def call(A):
        nv.check(nv.lib().ure_csr_pair_knn(*_head(A, n, n_item, code), A.addr('query' if with_query else None), nq, n_nb, splits, A.addr('dist'),
                                           A.addr('idx'), A.addr('ws'), A.size('ws'), nv.stream_handle()), 'ure_csr_pair_knn')

    def want():
        dist, idx = engine.pair_knn(engine.CsrSet(mat), n_nb, metric, query, splits)
        return {'dist': dist.cpu().numpy(), 'idx': idx.cpu().numpy().astype(np.int32)}
    return call, want


def case_rowsum(A, metric):
    from ultrare_amd import _native as nv, engine
    mat, n, n_item = _arena_inputs(A)
    A.output('R', n * 4)
    code = engine.PAIR_METRICS[metric]

    def call(A):
        nv.check(nv.lib().ure_csr_pair_rowsum(*_head(A, n, n_item, code), A.addr('R'), nv.stream_handle()), 'ure_csr_pair_rowsum')
    return call, lambda: {'R': engine.pair_rowsum(engine.CsrSet(mat), metric).cpu().numpy()}


def case_cols(A, metric):
    from ultrare_amd import _native as nv, engine
    mat, n, n_item = _arena_inputs(A)
    cols = np.array([129, 0, 64], dtype=np.int32)
    A.input('cols', cols)
    A.output('out', n * 3 * 4)
    code = engine.PAIR_METRICS[metric]

    def call(A):
        nv.check(nv.lib().ure_csr_pair_cols(*_head(A, n, n_item, code), A.addr('cols'), 3, A.addr('out'), nv.stream_handle()), 'ure_csr_pair_cols')
    return call, lambda: {'out': engine.pair_cols(engine.CsrSet(mat), cols, metric).cpu().numpy()}


def case_label_expsum(A, metric):
    from ultrare_amd import _native as nv, engine
    mat, n, n_item = _arena_inputs(A)
    k = 3
    label = (np.arange(n) % k).astype(np.int32)
    A.input('label', label)
    A.output('W', n * k * 8)
    code = engine.PAIR_METRICS[metric]

    def call(A):
        nv.check(nv.lib().ure_csr_pair_label_expsum(*_head(A, n, n_item, code), A.addr('label'), k, A.addr('W'), nv.stream_handle()),
                 'ure_csr_pair_label_expsum')
    return call, lambda: {'W': engine.pair_label_expsum(engine.CsrSet(mat), label, k, metric).cpu().numpy()}


ARENA_CASES = [
    ('knn-euclidean-s0-all', 'ure_csr_pair_knn', lambda A: case_knn(A, 'euclidean', 0, False)),
    ('knn-cosine-s3-query', 'ure_csr_pair_knn', lambda A: case_knn(A, 'cosine', 3, True)),
    ('rowsum-manhattan', 'ure_csr_pair_rowsum', lambda A: case_rowsum(A, 'manhattan')),
    ('cols-cosine', 'ure_csr_pair_cols', lambda A: case_cols(A, 'cosine')),
    ('label_expsum-euclidean', 'ure_csr_pair_label_expsum', lambda A: case_label_expsum(A, 'euclidean')),
]


@pytest.mark.parametrize('case', ARENA_CASES, ids=[c[0] for c in ARENA_CASES])
def test_entry_keeps_the_memory_contract(case):
    """tests/test_gpu_abi_memory.py's check for the entries of include/ultrare_csr_pair.h: outputs and scratch prefilled with
    three byte values, no guard or input byte changed, equal outputs whatever the prefill, and the wrapper's bytes."""
    _, entry, build = case
    A = Arena('cuda:0')
    call, want = build(A)
    reports = run_prefills(A, call, sync=torch.cuda.synchronize)
    found = verdict(reports)
    assert not found, f'{entry}:\n  ' + '\n  '.join(found)
    ref = want()
    assert set(ref) == set(reports[0].outputs)
    for name, arr in ref.items():
        assert reports[0].outputs[name] == np.ascontiguousarray(arr).tobytes(), (entry, name)


# ---- 5. refusals and the torch op ------------------------------------------------------------------------------------------------
def test_the_engine_refuses_a_given_matrix_a_missing_half_and_the_host():
    from ultrare_amd import _native as nv, engine
    mat, _ = build_case(65, 300, 'grid')
    S = engine.CsrSet(mat)
    for call in (lambda m: engine.pair_knn(S, 3, m), lambda m: engine.pair_rowsum(S, m), lambda m: engine.pair_cols(S, [0], m),
                 lambda m: engine.pair_label_expsum(S, np.zeros(65, int), 1, m)):
        for m in (None, 'given'):
            with pytest.raises(ValueError, match='no CSR form'):
                call(m)
    half = engine.CsrSet.from_device(65, 300, col_off=S.col_off, row=S.row, cval=S.cval)
    with pytest.raises(ValueError, match='without the CSR half'):
        engine.pair_rowsum(half, 'euclidean')
    host = engine.CsrSet.from_device(65, 300, S.row_off.cpu(), S.col.cpu(), S.val.cpu())
    with pytest.raises(nv.NativeError, match='HIP device only'):
        engine.pair_rowsum(host, 'euclidean')
    mixed = engine.CsrSet.from_device(65, 300, S.row_off, S.col.cpu(), S.val)
    with pytest.raises(ValueError, match='is on cpu'):
        engine.pair_rowsum(mixed, 'euclidean')
    with pytest.raises(ValueError, match='n_nb'):
        engine.pair_knn(S, 66, 'euclidean')
    L = nv.lib()
    rc = L.ure_csr_pair_rowsum(nv.ptr(S.row_off), nv.ptr(S.col), nv.ptr(S.val), 65, 300, engine.PAIR_METRICS['given'], nv.ptr(S.val), None)
    assert rc == -1                                                              # refused before any launch


def test_the_torch_op_equals_the_engine_call():
    from ultrare_amd import engine
    import ultrare_amd.ops  # noqa: F401
    mat, X = build_case(130, 300, 'grid')
    S = engine.CsrSet(mat)
    query = torch.tensor([129, 5, 5, 0], dtype=torch.int32, device='cuda')
    for metric in METRICS:
        for q in (None, query):
            got = torch.ops.ultrare.csr_pair_knn(S.row_off, S.col, S.val, 300, q, 7, metric)
            want = engine.pair_knn(torch.from_numpy(X).cuda(), 7, metric, q)
            assert same(got[0], want[0]) and same(got[1], want[1])
    with pytest.raises(ValueError, match='outside'):
        torch.ops.ultrare.csr_pair_knn(S.row_off, S.col, S.val, 299, None, 7, 'euclidean')
