"""Host side of rating-based OT grouping on the sparse matrix (csrc/csr_group.hip): the contract of ure_csr_cost
and ure_csr_centroids restated in numpy, and the canonical CSR / CSC both read.  The reference's own 'rating-ot' branch raises
(utils.py:637 on a csr_matrix), so the arithmetic is this project's: float64 accumulators, a fixed order of additions, one
rounding to float32 at the end.  The device is held to these functions bit for bit.  Nothing here touches the device."""
import numpy as np

MAX_K = 256          # kCsrMaxK of csrc/csr_group.hip
CC_LANES = 256       # lanes of the squared-norm reduction (cc_ref)


class Compressed:
    """One compressed orientation of a matrix: off int64 [n_major + 1], idx int32 [nnz] (ascending inside a segment, no
    repeats), val float32 [nnz]; shape = (n_major, n_minor).  (A scipy matrix forces one dtype on both index arrays.)"""
    __slots__ = ('off', 'idx', 'val', 'shape')

    def __init__(self, off, idx, val, shape):
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        self.idx = np.ascontiguousarray(idx, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float32)
        self.shape = (int(shape[0]), int(shape[1]))

    @property
    def nnz(self):
        return len(self.idx)

    def segment_of_entry(self):
        """int64 [nnz]: the segment every stored entry belongs to."""
        return np.repeat(np.arange(self.shape[0], dtype=np.int64), np.diff(self.off))


def canonical_csr(sp_mat):
    """(csr, csc) of a SciPy sparse matrix as Compressed float32 copies: duplicates summed, indices sorted, explicit zeros
    kept.  ValueError for an input that is not 2-D, for non-finite values and for nnz, n or n_item at or above 2^31."""
    from scipy import sparse
    if isinstance(sp_mat, tuple) and len(sp_mat) == 2 and all(isinstance(h, Compressed) for h in sp_mat):
        return sp_mat
    if not sparse.issparse(sp_mat):
        raise ValueError(f'expected a SciPy sparse matrix, not {type(sp_mat).__name__}')
    if len(sp_mat.shape) != 2:
        raise ValueError(f'the rating matrix must be 2-D, not of shape {tuple(sp_mat.shape)}')
    n, n_item = (int(v) for v in sp_mat.shape)
    if n >= 2 ** 31 or n_item >= 2 ** 31 or sp_mat.nnz >= 2 ** 31:
        raise ValueError(f'shape {n} x {n_item} with {sp_mat.nnz} entries: n, n_item and nnz must stay below 2^31')
    if n < 1 or n_item < 1:
        raise ValueError(f'an empty rating matrix ({n} x {n_item})')
    csr = sparse.csr_matrix(sp_mat, dtype=np.float32, copy=True)
    csr.sum_duplicates()                                    # sorts the indices as well; stored zeros stay
    if not np.isfinite(csr.data).all():
        raise ValueError('the rating matrix holds non-finite values')
    csc = csr.tocsc()                                       # ascending row inside a column
    return (Compressed(csr.indptr, csr.indices, csr.data, (n, n_item)),
            Compressed(csc.indptr, csc.indices, csc.data, (n_item, n)))


def check_cluster_args(sp_mat, k):
    """canonical_csr plus the range of k, before any device work -> (csr, csc)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f'k must be an integer, not {k!r}')
    halves = canonical_csr(sp_mat)
    n = halves[0].shape[0]
    if k < 1 or k > n:
        raise ValueError('need 1 <= k <= n clusters')
    if k > MAX_K:
        raise ValueError(f'the CSR cost and centroid kernels take at most {MAX_K} clusters, not {k}')
    return halves


def dense_rows(csr, rows):
    """float32 [len(rows), n_item]: the given rows of a Compressed CSR, densified (the initial centroids)."""
    out = np.zeros((len(rows), csr.shape[1]), dtype=np.float32)
    for r, i in enumerate(rows):
        a, b = csr.off[i], csr.off[i + 1]
        out[r, csr.idx[a:b]] = csr.val[a:b]
    return out


def cc_ref(C):
    """float64 [k]: the squared norms of the float32 centroids C [k, n_item] in the kernel's order.  Lane l of 256 adds
    C[c][j]^2 for j = l, l + 256, ... in ascending j from +0.0; the 256 lane sums are then added in ascending l.  (A square
    of a float32 is exact in float64: only the order matters.)"""
    C = np.asarray(C, dtype=np.float32)
    k, n_item = C.shape
    m = -(-n_item // CC_LANES)
    sq = np.zeros((k, m * CC_LANES), dtype=np.float64)      # the tail adds +0.0, which changes no sum
    sq[:, :n_item] = C.astype(np.float64) ** 2
    lanes = np.cumsum(sq.reshape(k, m, CC_LANES), axis=1)[:, -1, :]       # cumsum adds one after the other
    return np.cumsum(lanes, axis=1)[:, -1]


def _seq_sums(seg, weights, n_seg):
    """Per segment the sequential float64 sum of its weights in the order given, from +0.0 (np.bincount's loop)."""
    return np.bincount(seg, weights=weights, minlength=n_seg)


def csr_cost_ref(csr, C):
    """The contract of ure_csr_cost -> float32 [k, n] (ure_ot_cost's layout).  For row i and centroid c, over the row's stored
    entries in ascending column, sequentially in float64 from +0.0: dot = sum x_ij C[c][j], xx = sum x_ij^2; then
    dist[c][i] = float32(max((xx - 2 dot) + cc_c, 0.0)), cc = cc_ref(C).  An empty row gives float32(cc_c)."""
    if not isinstance(csr, Compressed):
        csr = canonical_csr(csr)[0]
    C = np.asarray(C, dtype=np.float32)
    n = csr.shape[0]
    k = C.shape[0]
    assert C.shape[1] == csr.shape[1]
    seg = csr.segment_of_entry()
    x = csr.val.astype(np.float64)
    xx = _seq_sums(seg, x * x, n)
    cc = cc_ref(C)
    out = np.empty((k, n), dtype=np.float32)
    for c in range(k):
        dot = _seq_sums(seg, x * C[c, csr.idx].astype(np.float64), n)      # each product is exact in float64
        out[c] = np.maximum((xx - 2.0 * dot) + cc[c], 0.0).astype(np.float32)
    return out


def csr_centroids_ref(csc, label, k):
    """The contract of ure_csr_centroids -> (C float32 [k, n_item], counts int64 [k]).  S[c][j] = the sequential float64 sum,
    in ascending user id from +0.0, of the entries of column j whose user has label c; C[c][j] = float32(S[c][j] /
    float64(counts[c])).  A cluster with no member gives a zero row (counts says so; the callers raise)."""
    if not isinstance(csc, Compressed):
        csc = canonical_csr(csc)[1]
    label = np.asarray(label, dtype=np.int64)
    n_item, n = csc.shape
    if label.shape != (n,) or (n and (label.min() < 0 or label.max() >= k)):
        raise ValueError(f'label must be n = {n} values in [0, {k})')
    counts = np.bincount(label, minlength=k).astype(np.int64)
    key = label[csc.idx] * n_item + csc.segment_of_entry()
    S = _seq_sums(key, csc.val.astype(np.float64), k * n_item).reshape(k, n_item)
    C = np.zeros((k, n_item), dtype=np.float32)
    has = counts > 0
    C[has] = (S[has] / counts[has].astype(np.float64)[:, None]).astype(np.float32)
    return C, counts
