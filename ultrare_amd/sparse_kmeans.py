"""Host side of k-means / balanced k-means on the sparse rating matrix (csrc/csr_kmeans.hip): the contract of
ure_csr_kmeans_cost, ure_csr_kmeans_centroids and ure_balanced_fill restated in numpy.  The arithmetic is the dense route's
(kmeans_cost_kernel / kmeans_centroid_kernel of csrc/ot.hip, scipy's csr order: oracle/cpu_ref.py) restricted to the stored
entries: float32 chains, sequential in ascending index from +0.0, one rounded multiply and one rounded add per term.  An entry
that is not stored would add +-0 to such a chain and change no bit, so for finite centroids these functions equal the dense
ones on the densified matrix bit for bit.  The device is held to them bit for bit.  Nothing here touches the device."""
import numpy as np

from .sparse_group import MAX_K, Compressed, canonical_csr


def check_kmeans_args(sp_mat, k):
    """canonical_csr (2-D, finite, sizes below 2^31) plus the range of k and the fill's n k < 2^32, before any device work
    -> (csr, csc)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f'k must be an integer, not {k!r}')
    halves = canonical_csr(sp_mat)
    n = halves[0].shape[0]
    if k < 1 or k > n:
        raise ValueError('need 1 <= k <= n clusters')
    if k > MAX_K:
        raise ValueError(f'the CSR k-means kernels take at most {MAX_K} clusters, not {k}')
    if n * int(k) >= 2 ** 32:
        raise ValueError(f'n * k = {n} * {k} must stay below 2^32 (the fill keys carry the flat index in 32 bits)')
    return halves


def _seq_f32(seg, terms, n_seg):
    """Per segment the sequential float32 sum of its float32 terms in the order given, from +0.0.  Step t adds the t-th term of
    every segment that has one: each segment sees its own terms one after the other, every add rounded to float32."""
    seg = np.asarray(seg, dtype=np.int64)
    terms = np.asarray(terms, dtype=np.float32)
    out = np.zeros(n_seg, dtype=np.float32)
    if len(seg) == 0:
        return out
    order = np.argsort(seg, kind='stable')
    seg, terms = seg[order], terms[order]
    start = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
    length = np.diff(np.r_[start, len(seg)])
    ids = seg[start]
    by_len = np.argsort(-length, kind='stable')             # segments with a t-th term are a prefix of this order
    start, length, ids = start[by_len], length[by_len], ids[by_len]
    acc = np.zeros(len(ids), dtype=np.float32)
    for t in range(int(length[0])):
        m = int(np.searchsorted(-length, -t, side='left'))  # segments with length > t
        acc[:m] = acc[:m] + terms[start[:m] + t]
    out[ids] = acc
    return out


def csq_ref(C):
    """float32 [k]: the sequential float32 sum of C[c][j]^2 over all items in ascending j from +0.0."""
    C = np.asarray(C, dtype=np.float32)
    s = np.zeros(C.shape[0], dtype=np.float32)
    for j in range(C.shape[1]):
        s = s + C[:, j] * C[:, j]
    return s


def kmeans_cost_csr_ref(csr, C):
    """The contract of ure_csr_kmeans_cost -> float32 [n, k] (ure_kmeans_cost's layout).  For row i and centroid c, over the
    row's stored entries in ascending column, in float32 from +0.0: dot += x * C[c][j], esq += x * x; csq = csq_ref(C);
    dist[i][c] = ((-2 * dot) + esq) + csq[c], every operation rounded to float32.  An empty row gives csq[c]."""
    if not isinstance(csr, Compressed):
        csr = canonical_csr(csr)[0]
    C = np.asarray(C, dtype=np.float32)
    n = csr.shape[0]
    k = C.shape[0]
    assert C.shape[1] == csr.shape[1]
    seg = csr.segment_of_entry()
    x = csr.val
    esq = _seq_f32(seg, x * x, n)
    csq = csq_ref(C)
    out = np.empty((n, k), dtype=np.float32)
    for c in range(k):
        dot = _seq_f32(seg, x * C[c, csr.idx], n)
        out[:, c] = ((np.float32(-2.0) * dot) + esq) + csq[c]
    return out


def kmeans_centroids_csc_ref(csc, label, k):
    """The contract of ure_csr_kmeans_centroids -> (C float32 [k, n_item], counts int64 [k]).  inv_c = float32(1.0 /
    float64(counts[c])); C[c][j] = the sequential float32 sum, in ascending user id from +0.0, of float32(x * inv_c) over the
    entries of column j whose user has label c.  A cluster with no member gives a zero row (counts says so; the callers
    raise)."""
    if not isinstance(csc, Compressed):
        csc = canonical_csr(csc)[1]
    label = np.asarray(label, dtype=np.int64)
    n_item, n = csc.shape
    if label.shape != (n,) or (n and (label.min() < 0 or label.max() >= k)):
        raise ValueError(f'label must be n = {n} values in [0, {k})')
    counts = np.bincount(label, minlength=k).astype(np.int64)
    with np.errstate(divide='ignore'):
        inv = (1.0 / counts.astype(np.float64)).astype(np.float32)
    lab = label[csc.idx]
    key = lab * n_item + csc.segment_of_entry()
    C = _seq_f32(key, csc.val * inv[lab], k * n_item).reshape(k, n_item)
    return C, counts


def fill_keys(dist):
    """uint64 [n * k]: ure_host_kmeans_assign's sort keys of a float32 [n, k] matrix -- the order-preserving map of the float's
    bit pattern (negative: all bits flipped, otherwise the sign bit set: -0.0 sorts before +0.0, NaN patterns by their bits)
    above the flat index u * k + c."""
    b = np.ascontiguousarray(dist, dtype=np.float32).reshape(-1).view(np.uint32)
    b = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return (b.astype(np.uint64) << np.uint64(32)) | np.arange(b.size, dtype=np.uint64)


def balanced_fill_ref(dist, capacity):
    """The contract of ure_balanced_fill (ure_host_kmeans_assign's rule) -> int32 [n].  capacity <= 0: the argmin of every row,
    first minimum, the first NaN winning.  capacity > 0: walk the (user, group) pairs in ascending fill_keys order; a user
    takes its first group that still has room for one of `capacity` users."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    if dist.ndim != 2 or dist.size == 0 or dist.size >= 2 ** 32:
        raise ValueError(f'dist must be a float32 [n, k] matrix with 0 < n k < 2^32, not of shape {dist.shape}')
    n, k = dist.shape
    if capacity <= 0:
        return dist.argmin(axis=1).astype(np.int32)          # numpy's argmin: the first minimum, the first NaN wins
    if capacity * k < n:
        raise ValueError(f'capacity {capacity} x {k} groups < {n} users')
    label = np.zeros(n, dtype=np.int32)
    left = [int(capacity)] * k
    done = np.zeros(n, dtype=bool)
    n_done = 0
    for f in np.argsort(fill_keys(dist)).tolist():            # (the keys are distinct: any sort gives this order)
        u, c = divmod(f, k)
        if done[u] or left[c] <= 0:
            continue
        label[u], done[u] = c, True
        left[c] -= 1
        n_done += 1
        if n_done == n:
            break
    return label


def threshold_fill_ref(dist, capacity):
    """The device's iteration on the host -> (label int32 [n], rounds): thresholds start at UINT64_MAX; every user picks the
    group with its smallest key <= that group's threshold; every group with more than `capacity` choosers lowers its threshold
    to its capacity-th smallest chooser key; the first round that moves no threshold holds the labels."""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n, k = dist.shape
    capacity = min(int(capacity), n)
    if capacity * k < n:
        raise ValueError(f'capacity {capacity} x {k} groups < {n} users')
    key = fill_keys(dist).reshape(n, k)
    big = np.uint64(0xFFFFFFFFFFFFFFFF)
    thr = np.full(k, big, dtype=np.uint64)
    for rounds in range(1, n * k + 2):
        masked = np.where(key <= thr[None, :], key, big)
        choice = masked.argmin(axis=1)
        chosen = masked[np.arange(n), choice]
        moved = False
        for g in range(k):
            mine = chosen[choice == g]
            if len(mine) > capacity:
                thr[g] = np.partition(mine, capacity - 1)[capacity - 1]
                moved = True
        if not moved:
            return choice.astype(np.int32), rounds
    raise RuntimeError(f'no fixed point after {n * k + 1} rounds')
