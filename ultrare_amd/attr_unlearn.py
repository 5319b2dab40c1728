"""Host side of attribute unlearning (csrc/mmd.hip): the contract of ure_mmd_bandwidth, ure_mmd_loss_grad and
ure_u2u_loss_grad restated in numpy float64, the fine-tune loop of utils.attribute_unlearn in float64, and the argument
checks that run before any device work.  Nothing here touches the device.

The losses are the reference's rbk / mmd_loss / buildLap (utils.py:223-279) on m = n1 + n2 selected rows of a table, the
first n1 the source group S, the rest the target group T:

  bandwidth   fix_sigma, or sum_ij L_ij / (m^2 - m), L_ij = |x_i - x_j|^2, by its closed form on centred rows
              (2 m sum |c_i|^2 - 2 |sum c_i|^2) / (m^2 - m), c_i = x_i - mean.  bw_q = bw / kernel_mul^(kernel_num // 2) *
              kernel_mul^q.  No gradient flows through it (the reference's .data).
  value       K_ij = sum_q exp(-L_ij / bw_q); loss = mean(K_SS) + mean(K_TT) - mean(K_ST) - mean(K_TS), diagonals included.
  gradient    g_i = sum_j c_ij w_ij (x_i - x_j), w_ij = sum_q (-2 / bw_q) exp(-L_ij / bw_q), c_ij = 2 / n1^2 inside S,
              2 / n2^2 inside T and -2 / (n1 n2) across.
  u2u         trace(U^T Lap U) of the complete bipartite graph S - T = sum_{i in S, j in T} L_ij, gradient
              2 (n2 x_i - sum_T x_j) for i in S and the mirror image for T.

How far the float32 kernel may stray from these (u = 2^-24), returned beside the values so that a test never tunes them:

  loss      4 kernel_num ((d + 3) / e + 4) u.  L_ij is a float32 sum of d squares of float32 differences (relative error
            (d + 2) u), times the rounded 1 / bw_q (one more u): the argument t = L / bw_q of exp(-t) is off by (d + 3) u t and
            exp(-t) by (d + 3) u t e^-t <= (d + 3) u / e.  expf adds at most 4 u (its value is <= 1).  K_ij has kernel_num such
            terms, the sums over a block are float64, and the loss is four means.
  gradient  ((d + 3) / e + 80) u (sum_q 2 / bw_q) sum_j |c_ij| |x_if - x_jf| plus one float32 denormal, elementwise.  Each term
            (2 / bw_q) exp(-t) carries the error above relative to 2 / bw_q; the 80 u are the 64 float32 additions of one
            partial sum (no float32 sum is longer before it enters a float64 accumulator) and 16 u for the products c w,
            c w (x_i - x_j), the difference, the rounded coefficients and expf.
  u2u       float64 sums of float32 data: (m + d + 8) 2^-53 of the sum of the magnitudes added, plus for the float32
            gradient one rounding u |g|.
"""
import numpy as np

MAX_D = 128            # kMmdMaxD of csrc/mmd.hip
MAX_KERNELS = 16       # kMmdMaxKernels
RBK_MAX_M = 8192       # the widest kernel matrix utils.rbk writes
U32 = 2.0 ** -24
U64 = 2.0 ** -53
DENORMAL32 = 2.0 ** -149
_CHUNK = 256           # rows of the m x m temporaries held at a time


def _real(name, v, positive=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or (positive and v <= 0):
        raise ValueError(f'{name} must be a finite number' + (' > 0' if positive else '') + f', not {v!r}')
    return float(v)


def check_mmd_args(kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """ValueError unless kernel_mul > 0, 1 <= kernel_num <= 16 (an integer) and fix_sigma is None or > 0 -> the three values."""
    kernel_mul = _real('kernel_mul', kernel_mul, positive=True)
    if isinstance(kernel_num, bool) or not isinstance(kernel_num, (int, np.integer)) or not 1 <= kernel_num <= MAX_KERNELS:
        raise ValueError(f'kernel_num must be an integer in 1 .. {MAX_KERNELS}, not {kernel_num!r}')
    if fix_sigma is not None:
        fix_sigma = _real('fix_sigma', fix_sigma, positive=True)
    return kernel_mul, int(kernel_num), fix_sigma


def check_width(d, ld=None):
    """ValueError unless 1 <= d <= 128 (and ld >= d)."""
    if not 1 <= int(d) <= MAX_D:
        raise ValueError(f'the embedding width must be in 1 .. {MAX_D}, not {d}')
    if ld is not None and int(ld) < int(d):
        raise ValueError(f'row stride {ld} < width {d}')
    return int(d)


def check_groups(id1, id2, n_rows):
    """(rows int32 [n1 + n2], n1, n2) of two groups of row ids, or ValueError: each non-empty, integers in [0, n_rows),
    distinct, and the two disjoint."""
    out = []
    for name, ids in (('id1', id1), ('id2', id2)):
        a = np.asarray(ids.detach().cpu().numpy() if hasattr(ids, 'detach') else ids).reshape(-1)
        if a.size == 0:
            raise ValueError(f'{name} is empty: both groups need at least one row')
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f'{name} must hold integer row ids, not {a.dtype}')
        a = a.astype(np.int64)
        if a.min() < 0 or a.max() >= n_rows:
            raise ValueError(f'{name} holds ids outside [0, {n_rows})')
        if len(np.unique(a)) != len(a):
            raise ValueError(f'{name} lists a row more than once')
        out.append(a)
    if len(np.intersect1d(out[0], out[1])):
        raise ValueError(f'id1 and id2 share rows {np.intersect1d(out[0], out[1])[:8].tolist()}: the groups must be disjoint')
    if n_rows >= 2 ** 31:
        raise ValueError(f'{n_rows} rows: ids must stay below 2^31')
    return np.concatenate(out).astype(np.int32), len(out[0]), len(out[1])


def check_var(var):
    if var not in ('d2d', 'u2u'):
        raise ValueError(f"var must be 'd2d' or 'u2u', not {var!r}")
    return var


def check_loop_args(eta, alpha, lr, steps):
    eta, lr = _real('eta', eta), _real('lr', lr)
    alpha = _real('alpha', alpha)
    if alpha < 0:
        raise ValueError(f'alpha must be >= 0, not {alpha!r}')
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
        raise ValueError(f'steps must be an integer >= 0, not {steps!r}')
    return eta, alpha, lr, int(steps)


def check_bandwidth(bw):
    """ValueError for a bandwidth that is not positive and finite (all selected rows equal; the reference returns NaN)."""
    if not (np.isfinite(bw) and bw > 0):
        raise ValueError(f'the bandwidth is {bw!r}: it must be positive and finite (the selected rows are all equal, or not finite); '
                         'pass fix_sigma')
    return float(bw)


def _selected(X, rows, n1):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n1 = int(n1)
    if not 1 <= n1 < len(rows):
        raise ValueError(f'n1 = {n1} must leave both groups non-empty ({len(rows)} rows)')
    x = np.asarray(X)[rows].astype(np.float64)
    check_width(x.shape[1])
    return x, n1, len(rows) - n1


def bandwidth_ref(x):
    """sum_ij |x_i - x_j|^2 / (m^2 - m) of the rows of x (float64 [m, d], m >= 2) by the closed form on centred rows."""
    m = len(x)
    c = x - x.mean(axis=0)
    return float((2.0 * m * (c * c).sum() - 2.0 * (c.sum(axis=0) ** 2).sum()) / (float(m) * m - m))


def bandwidths(bw, kernel_mul, kernel_num):
    return np.array([bw / kernel_mul ** (kernel_num // 2) * kernel_mul ** q for q in range(kernel_num)], dtype=np.float64)


def kernel_matrix_ref(x, bw, kernel_mul, kernel_num):
    """K float64 [m, m] of the rows of x (small m only)."""
    L = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return sum(np.exp(-L / b) for b in bandwidths(bw, kernel_mul, kernel_num))


def _abs_dev_sums(x, ref):
    """out[i, f] = sum_j |x[i, f] - ref[j, f]| by sorting every column of ref: O((m + n) log n) per feature."""
    out = np.empty_like(x)
    n = len(ref)
    for f in range(x.shape[1]):
        v = np.sort(ref[:, f])
        P = np.concatenate([[0.0], np.cumsum(v)])
        k = np.searchsorted(v, x[:, f])
        out[:, f] = x[:, f] * k - P[k] + (P[n] - P[k]) - x[:, f] * (n - k)
    return out


def mmd_ref(X, rows, n1, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """The contract of ure_mmd_bandwidth + ure_mmd_loss_grad in float64 on the rows `rows` of X (the first n1 the source
    group) -> (loss, grad float64 [m, d], bandwidth, bound_loss, bound_grad float64 [m, d]); the bounds are the module
    docstring's.  ValueError for a bandwidth that is not positive and finite."""
    kernel_mul, kernel_num, fix_sigma = check_mmd_args(kernel_mul, kernel_num, fix_sigma)
    x, n1, n2 = _selected(X, rows, n1)
    m, d = x.shape
    bw = check_bandwidth(fix_sigma if fix_sigma is not None else bandwidth_ref(x))
    bws = bandwidths(bw, kernel_mul, kernel_num)
    in_s = np.arange(m) < n1
    sums = np.zeros((2, 2))
    grad = np.zeros((m, d))
    # L from the Gram matrix of the centred rows (L is invariant under the shift): its rounding, a few 2^-53 |c|^2, is nine
    # orders of magnitude below the bounds
    xc = x - x.mean(axis=0)
    sq = (xc * xc).sum(axis=1)
    for a in range(0, m, _CHUNK):
        L = np.maximum(sq[a:a + _CHUNK, None] + sq[None, :] - 2.0 * (xc[a:a + _CHUNK] @ xc.T), 0.0)
        L[np.arange(len(L)), np.arange(a, a + len(L))] = 0.0
        K, w = np.zeros_like(L), np.zeros_like(L)
        for b in bws:
            e = np.exp(-L / b)
            K += e
            w += (-2.0 / b) * e
        rs = in_s[a:a + _CHUNK]
        c = np.where(rs[:, None] == in_s[None, :], np.where(rs[:, None], 2.0 / (n1 * n1), 2.0 / (n2 * n2)), -2.0 / (n1 * n2))
        for g_r in (0, 1):
            for g_c in (0, 1):
                sums[g_r, g_c] += K[rs == (g_r == 0)][:, in_s == (g_c == 0)].sum()
        cw = c * w
        grad[a:a + _CHUNK] = cw.sum(axis=1)[:, None] * x[a:a + _CHUNK] - cw @ x      # sum_j cw_ij (x_i - x_j), in float64
    # sum_j |c_ij| |x_if - x_jf|: |c| takes one value per (group of i, group of j)
    to_s, to_t = _abs_dev_sums(x, x[:n1]), _abs_dev_sums(x, x[n1:])
    spread = np.where(in_s[:, None], 2.0 / (n1 * n1) * to_s + 2.0 / (n1 * n2) * to_t, 2.0 / (n1 * n2) * to_s + 2.0 / (n2 * n2) * to_t)
    loss = sums[0, 0] / (n1 * n1) + sums[1, 1] / (n2 * n2) - sums[0, 1] / (n1 * n2) - sums[1, 0] / (n1 * n2)
    bound_loss = 4.0 * kernel_num * ((d + 3) / np.e + 4.0) * U32
    bound_grad = ((d + 3) / np.e + 80.0) * U32 * (2.0 / bws).sum() * spread + DENORMAL32
    return float(loss), grad, bw, bound_loss, bound_grad


def u2u_ref(X, rows, n1):
    """The contract of ure_u2u_loss_grad in float64 -> (value, grad float64 [m, d], bound_value, bound_grad float64 [m, d])."""
    x, n1, n2 = _selected(X, rows, n1)
    m, d = x.shape
    c = x - x.mean(axis=0)
    cs, ct = c[:n1], c[n1:]
    vs, vt = cs.sum(axis=0), ct.sum(axis=0)
    qs, qt = (cs * cs).sum(), (ct * ct).sum()
    value = n2 * qs + n1 * qt - 2.0 * (vs @ vt)
    grad = np.concatenate([2.0 * (n2 * cs - vt), 2.0 * (n1 * ct - vs)])
    slack = (m + d + 8) * U64
    bound_value = slack * (n2 * qs + n1 * qt + 2.0 * np.abs(vs * vt).sum())
    scale = np.concatenate([2.0 * (n2 * np.abs(cs) + np.abs(ct).sum(axis=0)), 2.0 * (n1 * np.abs(ct) + np.abs(cs).sum(axis=0))])
    bound_grad = U32 * np.abs(grad) + slack * scale + DENORMAL32
    return float(value), grad, float(bound_value), bound_grad


def attribute_unlearn_ref(U, id1, id2, var='d2d', eta=1.0, alpha=0.0, lr=0.1, steps=1, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """The loop of utils.attribute_unlearn in float64 throughout -> (table float64, log): `steps` gradient steps
    U_i -= lr grad_i J on the rows id1 + id2 of a copy of U, J = eta dis(U[id1], U[id2]) + alpha sum_i |U_i - U*_i|^2 with U*
    the table at entry; the bandwidth is recomputed from the current rows every step unless fix_sigma is given.  log = dict
    of dis, reg, bandwidth (u2u: NaN), each steps + 1 values: before every step and after the last."""
    check_var(var)
    eta, alpha, lr, steps = check_loop_args(eta, alpha, lr, steps)
    T = np.array(U, dtype=np.float64)
    rows, n1, n2 = check_groups(id1, id2, len(T))
    rows = rows.astype(np.int64)
    start = T[rows].copy()
    log = {'dis': [], 'reg': [], 'bandwidth': []}
    for t in range(steps + 1):
        if var == 'd2d':
            dis, g, bw = mmd_ref(T, rows, n1, kernel_mul, kernel_num, fix_sigma)[:3]
        else:
            dis, g = u2u_ref(T, rows, n1)[:2]
            bw = float('nan')
        delta = T[rows] - start
        log['dis'].append(dis)
        log['reg'].append(float((delta * delta).sum()))
        log['bandwidth'].append(bw)
        if t < steps:
            T[rows] -= lr * (eta * g + 2.0 * alpha * delta)
    return T, log
