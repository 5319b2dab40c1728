"""Host side of the pair-distance clusterers on the sparse rating matrix (the CSR tile producer of csrc/pair_dist.hip; DESIGN
4.22): the argument checks that run before any device work, and the union walk stated in numpy.

The BIT contract of the device route is the dense device route on the densified matrix (engine.pair_* on an array): the CSR
producer walks the union of the stored columns of two rows in ascending column with the dense producer's own float32
operation per term, and a dense term of two implicit zeros changes no accumulator.  pair_dist_csr_ref below is the same walk
in float64, one pair at a time: a yardstick for tolerances, not a bit contract.  Nothing here touches the device."""
import numpy as np

from .sparse_group import Compressed, canonical_csr

WINDOW = 32          # kCsrPairWindow of csrc/pair_dist.hip: the entries of a row staged in LDS per item-id window
METRICS = ('euclidean', 'cosine', 'manhattan')


def check_pair_metric(metric):
    """The streamed metric of a CSR source, or ValueError: a given n x n matrix (metric None / 'given') has no CSR form."""
    if metric is None or metric == 'given':
        raise ValueError("a sparse matrix needs metric 'euclidean', 'cosine' or 'manhattan': a given distance matrix (metric None) has no CSR form")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of 'euclidean' / 'cosine' / 'manhattan', not {metric!r}")
    return metric


def check_pair_args(sp_mat, metric, n_user=None, k=None, k_max=None):
    """check_pair_metric, canonical_csr (2-D, finite, sizes below 2^31) and, where given, the row count against n_user and the
    range of k, before any device work -> (csr, csc)."""
    check_pair_metric(metric)
    halves = canonical_csr(sp_mat)
    n = halves[0].shape[0]
    if n_user is not None and n != n_user:
        raise ValueError(f'n_user = {n_user} but the input has {n} rows')
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f'k must be an integer, not {k!r}')
        if not 1 <= k <= n:
            raise ValueError(f'need 1 <= k <= n clusters, not k = {k}, n = {n}')
        if k_max is not None and k > k_max:
            raise ValueError(f'at most {k_max} groups, not {k}')
    return halves


def pair_dist_csr_ref(csr, rows, cols, metric):
    """float64 [len(rows), len(cols)]: D[rows[a], cols[b]] by the union walk, one pair at a time.  The stored columns of the
    two rows are merged in ascending column; a column stored in one row only pairs with 0.  euclidean: sqrt(sum t^2);
    manhattan: sum |t|; cosine: 1 - x.y / (|x| |y|) clamped to [0, 2], 1 when either row has no non-zero entry, 0 when both
    ids are equal.  csr: a Compressed CSR, the (csr, csc) pair, or a SciPy sparse matrix."""
    check_pair_metric(metric)
    if not isinstance(csr, Compressed):
        csr = canonical_csr(csr)[0]
    off, idx, val = csr.off, csr.idx, csr.val.astype(np.float64)
    out = np.empty((len(rows), len(cols)), dtype=np.float64)
    for a, u in enumerate(rows):
        ua, ub = off[u], off[u + 1]
        for b, v in enumerate(cols):
            va, vb = off[v], off[v + 1]
            p, q = ua, va
            acc = nx = ny = 0.0
            while p < ub or q < vb:
                iu = idx[p] if p < ub else np.iinfo(np.int64).max
                iv = idx[q] if q < vb else np.iinfo(np.int64).max
                m = min(iu, iv)
                x = y = 0.0
                if iu == m:
                    x = val[p]
                    p += 1
                if iv == m:
                    y = val[q]
                    q += 1
                if metric == 'euclidean':
                    acc += (x - y) * (x - y)
                elif metric == 'manhattan':
                    acc += abs(x - y)
                else:
                    acc += x * y
                    nx += x * x
                    ny += y * y
            if metric == 'euclidean':
                acc = np.sqrt(acc)
            elif metric == 'cosine':
                den = np.sqrt(nx) * np.sqrt(ny)
                acc = 1.0 if den == 0.0 else min(max(1.0 - acc / den, 0.0), 2.0)
                if u == v:
                    acc = 0.0
            out[a, b] = acc
    return out
