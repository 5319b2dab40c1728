"""Host side of weighted matrix factorisation for implicit feedback (csrc/wmf.hip, include/ultrare_wmf.h): the
contract of ure_gram and ure_wridge_rows restated in numpy, the objective in closed form, a whole sweep, and the argument checks
that run before any device work.  Nothing here touches the device.

The model (Hu, Koren, Volinsky 2008).  Every training triple (u, i, r) is an observation with preference p = 1 and confidence
c = 1 + alpha r; every other pair of the n_user x n_item universe has p = 0 and c = 1.  The ratings are the float32 rating / 5
the loaders give.  The trainer minimises

    sum over ALL pairs of c (p - x_u . y_i)^2  +  sum over rows of (l2 + l2_n n_row) |x|^2

by alternating least squares: with the item table Y fixed, user u's row solves

    (Y^T Y + sum_j (c_j - 1) y_j y_j^T + (l2 + l2_n n_u) I) x = sum_j c_j p_j y_j          (j over u's observations)

and Y^T Y -- the Gram matrix of the WHOLE fixed table, one k x k matrix for every user -- is what turns the sum over all
n_user x n_item pairs into O(nnz k^2 + rows k^3) work.

Confidence.  Entry j carries two float32 weights, as the kernel reads them: wg_j = fl32(alpha32 * r_j), which is c - 1, and
wb_j = fl32(1 + wg_j), which is c p with p = 1 (confidence_ref).

Gram (a BIT contract).  For a table F [n][d] float32 and a width k <= d, G0[a][b] = sum_i F[i][a] F[i][b] in float64 as a two-level
chain: within a chunk of CHUNK = 256 consecutive rows in ascending row order from 0.0, then the chunk sums in ascending chunk
order, starting from the first.  A product of two float32 values is exact in float64, so every step rounds once, here as on the
device: gram_ref gives the kernel's bytes.  Stored as the packed upper triangle, row-major, k (k + 1) / 2 doubles.

Weighted ridge row.  Segment s with entries j in CSR order, n_s of them, f_j = (double)F[idx[j]][0:k]:
    G = G0 + sum_j wg_j f_j f_j^T + (l2 + l2_n n_s) I,   b = sum_j wb_j f_j,   x = G^-1 b
by Cholesky and two substitutions in float64; x is rounded to float32 once, at the store.  G0 None adds nothing.  An empty segment
gives the zero row; a pivot that is not positive and finite gives a NaN row and is listed.  The kernel's order of additions
(fma(wg_j f_a, f_b, acc) in CSR order, then acc + G0[a][b], then + ridge on the diagonal) is not numpy's: wridge_rows_ref agrees
with the device to float64 rounding, not to the bit -- except that with wg = 1, wb = val and no G0 the device's bytes are
ure_ridge_rows's.

A sweep.  User half: F = V, segments by user, G0 = the Gram of ALL rows of V.  Item half: F = the new U, segments by item, G0 =
the Gram of all rows of the new U.  A user without observations gets the zero row in the first user half, so a shard's universe
is its own users x all items; an item nobody in the shard rated gets the zero row.

Objective (a diagnostic, float64).  With s_j = x_u . y_i of observation j, G_U = U^T U and G_V = V^T V:

    J = sum_ab G_U[a][b] G_V[a][b]                                  = sum over all pairs of (x_u . y_i)^2
      + sum_j (wg_j s_j^2 - 2 wb_j s_j + wb_j)                      the observations' share beyond confidence 1, preference 0
      + sum_u (l2 + l2_n n_u) |x_u|^2 + sum_i (l2 + l2_n n_i) |y_i|^2

The two weights enter as the solves read them, so every half sweep minimises J over its block exactly.  Where wb = 1 + wg holds
exactly the middle line is sum_j (wb_j (1 - s_j)^2 - s_j^2) and J is the objective above; in float32 the two differ by one
rounding of wb.  objective_dense evaluates the same J pair by pair over the dense n_user x n_item matrix (tests, tiny shapes).
"""
import numpy as np

from .ridge import MAX_D, _forward, segment_csr

CHUNK = 256          # URE_GRAM_CHUNK of include/ultrare_wmf.h: rows per inner chain of the Gram matrix
DEFAULT_ALPHA = 40.0     # Hu et al.'s value for their data; untuned here
DEFAULT_L2 = 0.1         # untuned


def _real(name, v, positive=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0 or (positive and v == 0):
        raise ValueError(f"{name} must be a finite number {'> 0' if positive else '>= 0'}, not {v!r}")
    return float(v)


def check_wmf_args(alpha, l2, l2_n=0.0, sweeps=1):
    """ValueError unless alpha is finite >= 0, l2 finite > 0 (the Gram matrix of a table with fewer rows than columns is
    singular: only the ridge makes every system definite), l2_n finite >= 0 and sweeps an integer >= 0.
    -> (alpha, l2, l2_n, sweeps)."""
    alpha, l2, l2_n = _real('alpha', alpha), _real('l2', l2, positive=True), _real('l2_n', l2_n)
    if alpha > float(np.finfo(np.float32).max):
        raise ValueError(f'alpha = {alpha!r} is not a finite float32')
    if isinstance(sweeps, bool) or not isinstance(sweeps, (int, np.integer)) or sweeps < 0:
        raise ValueError(f'sweeps must be an integer >= 0, not {sweeps!r}')
    return alpha, l2, l2_n, int(sweeps)


def confidence_ref(r, alpha):
    """(wg, wb) float32 of ratings r (rating / 5, read as float32): wg = fl32(alpha32 * r) = c - 1, wb = fl32(1 + wg) = c p."""
    r = np.ascontiguousarray(r, dtype=np.float32)
    wg = (np.float32(alpha) * r).astype(np.float32)
    wb = (np.float32(1.0) + wg).astype(np.float32)
    return wg, wb


def tri_size(k):
    return k * (k + 1) // 2


def tri_pack(G):
    """The packed upper triangle, row-major, of a square matrix."""
    G = np.asarray(G)
    return np.ascontiguousarray(G[np.triu_indices(G.shape[0])])


def tri_unpack(packed, k):
    """The symmetric k x k matrix of a packed upper triangle."""
    packed = np.asarray(packed, dtype=np.float64).reshape(-1)
    if packed.shape != (tri_size(k),):
        raise ValueError(f'a packed triangle of width {k} holds {tri_size(k)} values, not {packed.shape}')
    G = np.zeros((k, k), dtype=np.float64)
    G[np.triu_indices(k)] = packed
    return G + np.triu(G, 1).T


def gram_ref(F, k=None):
    """The contract of ure_gram, to the bit: the packed upper triangle (float64 [k (k + 1) / 2]) of F[:, :k]^T F[:, :k] summed as
    the two-level chain of the module's docstring.  Rows behind the table's end are padded with zeros, which changes no sum
    (x + 0.0 = x, and no partial sum is -0.0: every chain starts from +0.0)."""
    F = np.asarray(F)
    if F.ndim != 2 or F.shape[0] < 1 or F.dtype != np.float32:
        raise ValueError('F must be a float32 [n >= 1, d] array')
    k = F.shape[1] if k is None else int(k)
    if not 1 <= k <= F.shape[1]:
        raise ValueError(f'need 1 <= k <= {F.shape[1]}, not {k}')
    n = F.shape[0]
    chunks = -(-n // CHUNK)
    f = np.zeros((chunks * CHUNK, k), dtype=np.float64)
    f[:n] = F[:, :k]
    f = f.reshape(chunks, CHUNK, k)
    part = np.zeros((chunks, k, k), dtype=np.float64)
    for t in range(CHUNK):                                  # ascending row order inside every chunk; one rounding per step
        part += f[:, t, :, None] * f[:, t, None, :]
    G = part[0].copy()
    for c in range(1, chunks):                              # ascending chunk order, starting from the first
        G += part[c]
    return tri_pack(G)


def wridge_system(F, k, idx, wg, wb, G0=None, l2=0.0, l2_n=0.0):
    """(G, b) of one segment in float64: G = G0 + sum_j wg_j f_j f_j^T + (l2 + l2_n n) I, b = sum_j wb_j f_j, f_j = F[idx[j]][0:k];
    G0: a packed triangle (gram_ref), a k x k matrix, or None."""
    f = np.asarray(F)[np.asarray(idx, dtype=np.int64), :k].astype(np.float64)
    wg = np.asarray(wg, dtype=np.float32).astype(np.float64)
    wb = np.asarray(wb, dtype=np.float32).astype(np.float64)
    G = f.T @ (wg[:, None] * f) + (l2 + l2_n * len(wg)) * np.eye(k)
    if G0 is not None:
        G0 = np.asarray(G0, dtype=np.float64)
        G = G + (G0 if G0.ndim == 2 else tri_unpack(G0, k))
    return G, f.T @ wb


def wridge_rows_ref(F, k, off, idx, wg, wb, G0=None, l2=0.0, l2_n=0.0):
    """The contract of ure_wridge_rows in numpy float64 -> (X float64 [m, k], failed: the list of failed segments), as
    ridge.ridge_rows_ref states ure_ridge_rows: the system of wridge_system, Cholesky and two triangular solves; an empty segment
    gives the zero row; a pivot that is not positive and finite gives a NaN row and is listed.  The order of the additions is
    numpy's, not the kernel's."""
    from numpy.linalg import LinAlgError
    off = np.asarray(off, dtype=np.int64)
    m = len(off) - 1
    X = np.zeros((m, k), dtype=np.float64)
    full = None if G0 is None else (np.asarray(G0, dtype=np.float64) if np.ndim(G0) == 2 else tri_unpack(G0, k))
    failed = []
    for s in range(m):
        a, b = int(off[s]), int(off[s + 1])
        if b <= a:
            continue
        G, rhs = wridge_system(F, k, idx[a:b], wg[a:b], wb[a:b], full, l2, l2_n)
        try:
            if not np.isfinite(G).all():
                raise LinAlgError('non-finite system')
            L = np.linalg.cholesky(G)
            if not (np.isfinite(L).all() and (np.diag(L) > 0).all()):
                raise LinAlgError('non-finite factor')
            y = _forward(L, rhs)
            X[s] = _forward(L.T[::-1, ::-1], y[::-1])[::-1]
            if not np.isfinite(X[s]).all():
                raise LinAlgError('non-finite solution')
        except LinAlgError:
            X[s] = np.nan
            failed.append(s)
    return X, failed


def objective_ref(U, V, uid, iid, wg, wb, l2, l2_n=0.0):
    """J of the module's docstring in float64 on the host, without the dense matrix; the tables are read as the float32 values the
    kernels read (all their columns)."""
    U, V = np.asarray(U, dtype=np.float32).astype(np.float64), np.asarray(V, dtype=np.float32).astype(np.float64)
    uid, iid = np.asarray(uid, dtype=np.int64), np.asarray(iid, dtype=np.int64)
    wg, wb = np.asarray(wg, dtype=np.float32).astype(np.float64), np.asarray(wb, dtype=np.float32).astype(np.float64)
    s = np.einsum('ij,ij->i', U[uid], V[iid])
    nu = np.bincount(uid, minlength=len(U)).astype(np.float64)
    ni = np.bincount(iid, minlength=len(V)).astype(np.float64)
    cross = float(((U.T @ U) * (V.T @ V)).sum())
    obs = float((wg * s * s - 2.0 * wb * s + wb).sum())
    reg = float(((l2 + l2_n * nu) * (U * U).sum(axis=1)).sum() + ((l2 + l2_n * ni) * (V * V).sum(axis=1)).sum())
    return cross + obs + reg


def objective_dense(U, V, uid, iid, wg, wb, l2, l2_n=0.0):
    """The same J pair by pair over the dense n_user x n_item matrix: S = U V^T, the quadratic weight 1 + wg on an observed pair and
    1 elsewhere, the linear weight wb on an observed pair and 0 elsewhere (several observations of one pair add up).  Tiny shapes."""
    U, V = np.asarray(U, dtype=np.float32).astype(np.float64), np.asarray(V, dtype=np.float32).astype(np.float64)
    uid, iid = np.asarray(uid, dtype=np.int64), np.asarray(iid, dtype=np.int64)
    Cq, Cl = np.ones((len(U), len(V))), np.zeros((len(U), len(V)))
    np.add.at(Cq, (uid, iid), np.asarray(wg, dtype=np.float32).astype(np.float64))
    np.add.at(Cl, (uid, iid), np.asarray(wb, dtype=np.float32).astype(np.float64))
    S = U @ V.T
    nu = np.bincount(uid, minlength=len(U)).astype(np.float64)
    ni = np.bincount(iid, minlength=len(V)).astype(np.float64)
    reg = ((l2 + l2_n * nu) * (U * U).sum(axis=1)).sum() + ((l2 + l2_n * ni) * (V * V).sum(axis=1)).sum()
    return float((Cq * S * S - 2.0 * Cl * S + Cl).sum() + reg)


def wmf_sweeps_ref(U0, V0, uid, iid, rating, alpha, l2, l2_n=0.0, sweeps=1):
    """`sweeps` sweeps of implicit ALS from the float32 tables (U0 [n_user, k], V0 [n_item, k]) by the contract's calls ->
    (U, V float32, objectives float64 [1 + 2 sweeps]: J before the first and after every half sweep).  Every row is rounded to
    float32 once, as the kernel stores it."""
    alpha, l2, l2_n, sweeps = check_wmf_args(alpha, l2, l2_n, sweeps)
    U, V = np.ascontiguousarray(U0, dtype=np.float32), np.ascontiguousarray(V0, dtype=np.float32)
    k = U.shape[1]
    r = np.ascontiguousarray(rating, dtype=np.float32)
    wg, wb = confidence_ref(r, alpha)
    off_u, idx_u, r_u, _ = segment_csr(uid, iid, r, len(U))
    off_i, idx_i, r_i, _ = segment_csr(iid, uid, r, len(V))
    wg_u, wb_u = confidence_ref(r_u, alpha)
    wg_i, wb_i = confidence_ref(r_i, alpha)
    objectives = [objective_ref(U, V, uid, iid, wg, wb, l2, l2_n)]
    for _ in range(sweeps):
        X, failed = wridge_rows_ref(V, k, off_u, idx_u, wg_u, wb_u, gram_ref(V, k), l2, l2_n)
        assert not failed
        U = X.astype(np.float32)
        objectives.append(objective_ref(U, V, uid, iid, wg, wb, l2, l2_n))
        X, failed = wridge_rows_ref(U, k, off_i, idx_i, wg_i, wb_i, gram_ref(U, k), l2, l2_n)
        assert not failed
        V = X.astype(np.float32)
        objectives.append(objective_ref(U, V, uid, iid, wg, wb, l2, l2_n))
    return U, V, np.asarray(objectives, dtype=np.float64)


def check_backbone(optimizer='sgd', loss='mse', unlearn='retrain', dis_type='nor'):
    """What model='wmf' refuses by name (config.InsParam, method.scratch.Scratch): its trainer is alternating least squares on the
    implicit-feedback objective -- no optimizer to choose, no other loss, no Newton step on the MSE objective, no per-batch term."""
    if optimizer != 'sgd':
        raise ValueError(f"model='wmf' trains by alternating least squares: optimizer={optimizer!r} is not supported with it (leave the default)")
    if loss != 'mse':
        raise ValueError(f"model='wmf' minimises its own implicit-feedback objective: loss={loss!r} is not supported with it")
    if unlearn != 'retrain':
        raise ValueError(f"model='wmf' unlearns by retraining the affected shards (a few ALS sweeps): unlearn={unlearn!r} is not supported with it")
    if dis_type != 'nor':
        raise ValueError(f"model='wmf' has no per-batch step to add a term to: dis_type={dis_type!r} is not supported with it")
