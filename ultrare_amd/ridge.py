"""Host side of the batched ridge solves (csrc/mf_ridge.hip): the contract of ure_ridge_rows restated in
numpy, the CSR builder of engine.SegmentSet and the argument checks that run before any device work.  Nothing here
touches the device."""
import numpy as np

MAX_D = 128          # kRrMaxD of csrc/mf_ridge.hip: the widest padded table the kernel serves


def check_ridge_args(l2, l2_n=0.0):
    """ValueError unless l2 and l2_n are finite real numbers >= 0."""
    for name, v in (('l2', l2), ('l2_n', l2_n)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
            raise ValueError(f'{name} must be a finite number >= 0, not {v!r}')
    return float(l2), float(l2_n)


def segment_csr(seg_ids, other_ids, rating, n_seg):
    """(off int64 [n_seg + 1], idx int32 [nnz], val float32 [nnz], order int32 [n_seg]) of entries (segment, other id,
    rating / 5): a STABLE sort by segment, so a segment keeps its entries in the order given, and `order` lists the
    segments longest first (equal lengths by ascending id).  ValueError for arrays of different lengths and for ids out
    of range."""
    seg = np.ascontiguousarray(seg_ids).reshape(-1)
    other = np.ascontiguousarray(other_ids).reshape(-1)
    val = np.ascontiguousarray(rating, dtype=np.float32).reshape(-1)
    if not len(seg) == len(other) == len(val):
        raise ValueError('segment ids, other ids and ratings differ in length')
    n_seg = int(n_seg)
    if n_seg < 0 or n_seg >= 2 ** 31:
        raise ValueError(f'n_seg = {n_seg} outside [0, 2^31)')
    if len(seg) and (seg.min() < 0 or seg.max() >= n_seg):
        raise ValueError(f'segment ids outside [0, {n_seg})')
    if len(other) and (other.min() < 0 or other.max() >= 2 ** 31):
        raise ValueError('other ids outside [0, 2^31)')
    # numpy's stable sort of 16-bit keys is a radix sort; wider keys take the merge sort
    keys = seg.astype(np.uint16 if n_seg <= 65536 else np.int32)
    perm = np.argsort(keys, kind='stable')
    counts = np.bincount(seg, minlength=n_seg).astype(np.int64) if len(seg) else np.zeros(n_seg, dtype=np.int64)
    off = np.zeros(n_seg + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    order = np.argsort(-counts, kind='stable').astype(np.int32)
    return off, other[perm].astype(np.int32), val[perm], order


def ridge_system(F, k, idx, val, l2, l2_n=0.0):
    """(G, b) of one segment in float64: G = sum_j f_j f_j^T + (l2 + l2_n n) I, b = sum_j r_j f_j, f_j = F[idx[j]][0:k]."""
    f = np.asarray(F)[np.asarray(idx, dtype=np.int64), :k].astype(np.float64)
    r = np.asarray(val).astype(np.float64)
    return f.T @ f + (l2 + l2_n * len(r)) * np.eye(k), f.T @ r


def ridge_rows_ref(F, k, off, idx, val, l2, l2_n=0.0):
    """The contract of ure_ridge_rows in numpy float64 -> (X float64 [m, k], failed: the list of failed segments).  Per segment:
    the system of ridge_system, x = G^-1 b by Cholesky (G = L L^T) and two triangular solves; an empty segment gives the zero
    row; a segment whose Cholesky meets a pivot that is not positive and finite gives a NaN row and is listed.  The order of
    the additions inside a segment is numpy's, not the kernel's: the two agree to float64 rounding, not to the bit."""
    from numpy.linalg import LinAlgError
    off = np.asarray(off, dtype=np.int64)
    m = len(off) - 1
    X = np.zeros((m, k), dtype=np.float64)
    failed = []
    for s in range(m):
        a, b = int(off[s]), int(off[s + 1])
        if b <= a:
            continue
        G, rhs = ridge_system(F, k, idx[a:b], val[a:b], l2, l2_n)
        try:
            if not np.isfinite(G).all():
                raise LinAlgError('non-finite system')
            L = np.linalg.cholesky(G)
            if not (np.isfinite(L).all() and (np.diag(L) > 0).all()):
                raise LinAlgError('non-finite factor')
            y = _forward(L, rhs)
            X[s] = _forward(L.T[::-1, ::-1], y[::-1])[::-1]
        except LinAlgError:
            X[s] = np.nan
            failed.append(s)
    return X, failed


def _forward(L, b):
    """Solve L y = b for lower-triangular L, column by column."""
    y = np.array(b, dtype=np.float64)
    for j in range(len(y)):
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    return y


def ridge_objective(U, V, uid, iid, val, l2, l2_n=0.0):
    """sum_j (u_j . v_j - r_j)^2 + sum over the rows of U and of V of (l2 + l2_n n_row) |x|^2 in float64 on the host; the
    ratings are the float32 values the kernel reads.  What als_sweeps reports, for tests."""
    U, V = np.asarray(U).astype(np.float64), np.asarray(V).astype(np.float64)
    uid, iid = np.asarray(uid, dtype=np.int64), np.asarray(iid, dtype=np.int64)
    e = np.einsum('ij,ij->i', U[uid], V[iid]) - np.asarray(val, dtype=np.float32).astype(np.float64)
    nu = np.bincount(uid, minlength=len(U)).astype(np.float64)
    ni = np.bincount(iid, minlength=len(V)).astype(np.float64)
    return float(e @ e + ((l2 + l2_n * nu) * (U * U).sum(axis=1)).sum() + ((l2 + l2_n * ni) * (V * V).sum(axis=1)).sum())
