"""Inputs and the comparison the WMF tests share (tests/test_cpu_wmf.py, tests/test_gpu_wmf.py): small rating sets without a
repeated pair, normal tables, CSR segments of chosen lengths, and the per-row bound of the weighted ridge solve against its float64
contract.  No test here; nothing touches the device."""
import numpy as np

COND_LIMIT = 2.0 ** 26            # the input condition: (n_fixed + n_s + k) * cond(G_s) <= 2^26


def normal_table(n, d, seed):
    return np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)


def rating_set(n_user, n_item, n, seed, skip_user=None, skip_item=None):
    """n distinct (user, item) pairs in random order with ratings in {0.2 .. 1.0} as float32; skip_user / skip_item have none."""
    rs = np.random.RandomState(seed)
    flat = rs.permutation(n_user * n_item)
    uid, iid = flat // n_item, flat % n_item
    keep = np.ones(len(flat), dtype=bool)
    if skip_user is not None:
        keep &= uid != skip_user
    if skip_item is not None:
        keep &= iid != skip_item
    uid, iid = uid[keep][:n].astype(np.int64), iid[keep][:n].astype(np.int64)
    assert len(uid) == n
    return uid, iid, (rs.randint(1, 6, n) / 5.0).astype(np.float32)


def tiny():
    """7 users x 11 items, k = 3: 30 observations, user 5 and item 9 without any."""
    uid, iid, r = rating_set(7, 11, 30, seed=1, skip_user=5, skip_item=9)
    return uid, iid, r, normal_table(7, 3, 2), normal_table(11, 3, 3)


def segments_of(lens, n_fixed, seed):
    """A CSR with the given segment lengths, ids drawn with replacement (repeats inside a segment), ratings in {0.2 .. 1}."""
    rs = np.random.RandomState(seed)
    seg = np.repeat(np.arange(len(lens)), lens)
    return seg, rs.randint(0, n_fixed, len(seg)), (rs.randint(1, 6, len(seg)) / 5.0).astype(np.float32)


def tile_rows(d):
    """Rows of one LDS tile of the ridge kernels (csrc/ridge_solve.h: RrShape<D>::T)."""
    return 64 if d <= 32 else 2048 // d


def check_rows(X, F, k, off, idx, wg, wb, G0, l2, l2_n=0.0, rows=None, what=''):
    """Every row (or `rows`) of the device's X against wmf.wridge_rows_ref.  The bound is the one tests/test_gpu_ridge.py derives
    for the plain solve -- one float32 rounding at the store plus the float64 accumulation and Cholesky, 4 (depth + k) 2^-53 cond --
    with the Gram matrix's depth n_fixed added to the segment's: |x_dev - x_64| <= (2^-24 + 4 (n_fixed + n_s + k) 2^-53 cond(G_s))
    max |x_64| per row.  Asserts the input condition (n_fixed + n_s + k) cond <= 2^26 from the contract first; prints the worst
    figures before it asserts."""
    from ultrare_amd import wmf
    n_fixed = len(F)
    full = None if G0 is None else wmf.tri_unpack(G0, k)
    rows = range(len(off) - 1) if rows is None else rows
    worst, worst_cond, fails = 0.0, 0.0, []
    for s in rows:
        a, b = int(off[s]), int(off[s + 1])
        got = np.asarray(X[s], dtype=np.float64)
        assert not got[k:].any(), f'{what}: padding columns of row {s} are not zero'
        if a == b:
            assert not got.any(), f'{what}: empty segment {s} is not the zero row'
            continue
        want = wmf.wridge_rows_ref(F, k, [0, b - a], idx[a:b], wg[a:b], wb[a:b], full, l2, l2_n)[0][0]
        cond = np.linalg.cond(wmf.wridge_system(F, k, idx[a:b], wg[a:b], wb[a:b], full, l2, l2_n)[0])
        depth = n_fixed + (b - a) + k
        assert depth * cond <= COND_LIMIT, f'{what}: segment {s} (n_s = {b - a}) has cond {cond:.3g}: raise l2'
        bound = 2.0 ** -24 + 4 * depth * 2.0 ** -53 * cond
        err = np.abs(got[:k] - want).max() / np.abs(want).max()
        worst, worst_cond = max(worst, err / bound), max(worst_cond, cond)
        if not err <= bound:
            fails.append((s, b - a, err, bound))
    print(f'{what}: worst error / bound = {worst:.3f}, largest cond = {worst_cond:.3g}')
    assert not fails, fails[:5]
