"""Newton-step (influence) unlearning of an MF shard with the MSE loss, stated in numpy float64: the contract of csrc/influence.hip
(include/ultrare_influence.h), of engine.inf_matvec / inf_grad / inf_solve and of utils.newton_unlearn.  DESIGN 4.25.

For a shard's tables theta = (U, V) -- float32, widened to float64 once -- and its REMAINING triples D (a lightgcn.Graph of them and
their ratings r in CSR order, r = rating[graph.pos]):

    F(theta) = sum_D e_k^2 + l2 (|U|^2 + |V|^2),   e_k = U[u_k] . V[i_k] - r_k.

A row without an entry in D is EMPTIED: the minimiser of what remains is 0, the row is set to +0.0 and left out of the system.
Every other row is ACTIVE unless the caller freezes it (scope); a frozen row keeps its bytes and has a zero direction.  One step
solves (H + 2 damping I) x = -grad F on the active rows by conjugate gradients and sets theta <- float32(theta + x).  With the
tangent t_k = P[u_k] . V[i_k] + U[u_k] . Q[i_k] of a direction (P, Q),

    (H (P, Q))_U[u] = 2 sum_{k in row u} (t_k V[i_k] + [full] e_k Q[i_k]) + 2 l2 P[u]

and the item rows are the mirror image over the CSC; curvature 'gn' (Gauss-Newton) drops the e_k term; the gradient is the same
walk with t := e, no second term and P := U.

THE CHAINS (every operation is one float64 operation rounded on its own, never fused):
  coefficient pass   a lane holds four consecutive columns c = 4 l .. 4 l + 3 of the d / 4 lanes of a width d and runs
                     p = a_0 b_0; p = p + a_k b_k (k = 1, 2, 3) over them -- for t the four P V products and then, in the same
                     chain, the four U Q products; the d / 4 lane values are added as a balanced tree of adjacent pairs (width 4:
                     one lane, no tree; width 256: 64 lanes, six levels); e = that sum - (double) r.
  walk               acc from 0.0 over the row's entries in ascending position: acc = acc + a T[j][c], then (with a second
                     coefficient) acc = acc + b D[j][c]; out = 2 acc + (2 reg) X[r][c].  A row that is inactive or has no entry is
                     +0.0 in every byte.
  dot                z = x * y elementwise; chunks of 4096 values are folded by lightgcn.fold_256, the chunk sums by fold_256 again.
  CG                 x = 0, r = p = b, rr = dot(r, r), thresh = (tol tol) rr.  Per iteration: pAp = dot(p, A p); not pAp > 0 ->
                     flag 2; else alpha = rr / pAp, x = x + alpha p, r = r - alpha Ap, rr' = dot(r, r), beta = rr' / rr, rr = rr',
                     rr <= thresh -> flag 1, else p = r + beta p.  Once the flag is set x, r and p keep their bytes.
"""
import numpy as np

from .lightgcn import WIDTHS, Graph, _walk, check_width, fold_256  # noqa: F401

DOT_CHUNK = 4096
CURVATURES = ('full', 'gn')
RUNNING, CONVERGED, NON_POSITIVE = 0, 1, 2
LOG_BLOCK = 16                      # the device loop reads its log once per LOG_BLOCK iterations


# ---------------------------------------------------------------------------------------------------------------- argument checks
def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_args(curvature='full', damping=None, steps=1, iters=512, tol=1e-8, l2=1.0):
    """-> (l2, damping) as floats, damping None resolved to 0.1 * l2 for 'full' and 0 for 'gn'; ValueError otherwise."""
    if curvature not in CURVATURES:
        raise ValueError(f"curvature must be 'full' or 'gn', not {curvature!r}")
    if not (isinstance(l2, (int, float, np.floating, np.integer)) and np.isfinite(l2) and l2 > 0):
        raise ValueError(f'l2 must be positive and finite, not {l2!r}')
    l2 = float(l2)
    if damping is None:
        damping = 0.1 * l2 if curvature == 'full' else 0.0
    if not (isinstance(damping, (int, float, np.floating, np.integer)) and np.isfinite(damping) and damping >= 0):
        raise ValueError(f'damping must be finite and >= 0, not {damping!r}')
    damping = float(damping)
    if curvature == 'full' and damping == 0.0:
        raise ValueError("curvature='full' needs damping > 0: the objective is invariant under a common rotation of both tables, so the "
                         "full Hessian has a rotation null space and is singular without damping (curvature='gn' may run undamped)")
    if not (_is_int(steps) and steps >= 1):
        raise ValueError(f'steps must be an integer >= 1, not {steps!r}')
    if not (_is_int(iters) and iters >= 1):
        raise ValueError(f'iters must be an integer >= 1, not {iters!r}')
    if not (isinstance(tol, (float, np.floating)) and 0.0 < tol < 1.0):
        raise ValueError(f'tol must lie in (0, 1), not {tol!r}')
    return l2, damping


def check_model(model_type='mf', loss='mse'):
    """The update is defined for MF with the MSE loss only."""
    if model_type != 'mf':
        raise ValueError(f"Newton-step unlearning is defined for model='mf' only, not {model_type!r} (LightGCN's tables are no free parameters)")
    if loss != 'mse':
        raise ValueError(f"Newton-step unlearning is defined for loss='mse' only, not {loss!r} (BPR has another objective)")


def check_scope(scope, n_user, n_item):
    """scope 'all', or (users, items): the rows that may move (None in a slot: all rows of that side); every other row is frozen.
    -> (free_u, free_i) bool masks."""
    if isinstance(scope, str):
        if scope != 'all':
            raise ValueError(f"scope must be 'all' or (users, items), not {scope!r}")
        return np.ones(n_user, dtype=bool), np.ones(n_item, dtype=bool)
    if not (isinstance(scope, (tuple, list)) and len(scope) == 2):
        raise ValueError(f"scope must be 'all' or (users, items), not {scope!r}")
    out = []
    for ids, n, what in ((scope[0], n_user, 'user'), (scope[1], n_item, 'item')):
        m = np.ones(n, dtype=bool)
        if ids is not None:
            ids = np.asarray(ids).reshape(-1)
            if len(ids) and (not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= n):
                raise ValueError(f'scope: {what} rows must be integers in [0, {n})')
            m[:] = False
            m[ids.astype(np.int64)] = True
        out.append(m)
    return out[0], out[1]


def active_rows(graph, scope='all'):
    """-> (active_u, active_i, emptied_u, emptied_i) bool masks of a graph of the remaining triples."""
    free_u, free_i = check_scope(scope, graph.n_user, graph.n_item)
    has_u, has_i = np.diff(graph.off_u) > 0, np.diff(graph.off_i) > 0
    return has_u & free_u, has_i & free_i, ~has_u, ~has_i


# ---------------------------------------------------------------------------------------------------------------- the contract
def _lanes(a):
    return a.reshape(len(a), -1, 4)


def _tree(p):
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def coef_ref(graph, U, V, r, P=None, Q=None):
    """Per CSR entry k: e_k = U[u_k] . V[i_k] - r_k, or with a direction t_k = P[u_k] . V[i_k] + U[u_k] . Q[i_k] (float64 [N])."""
    d = check_width(np.shape(U)[1])
    assert np.shape(V)[1] == d
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    u, i = graph.row_u.astype(np.int64), graph.col.astype(np.int64)
    if (P is None) != (Q is None):
        raise ValueError('a direction is both P and Q')
    if P is None:
        a, b = _lanes(U[u]), _lanes(V[i])
        p = a[..., 0] * b[..., 0]
        for k in (1, 2, 3):
            p = p + a[..., k] * b[..., k]
        return _tree(p) - np.asarray(r, dtype=np.float32).astype(np.float64)
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    a, b, c, e = _lanes(P[u]), _lanes(V[i]), _lanes(U[u]), _lanes(Q[i])
    p = a[..., 0] * b[..., 0]
    for k in (1, 2, 3):
        p = p + a[..., k] * b[..., k]
    for k in (0, 1, 2, 3):
        p = p + c[..., k] * e[..., k]
    return _tree(p)


def walk_ref(off, idx, map, a, T, b, D, reg, X, active=None):
    """out[r][c] = 2 acc + (2 reg) X[r][c], acc the chain over the row's entries (ascending, from 0.0) of a[q] T[idx][c] and then
    b[q] D[idx][c] (b, D optional), q = map[k] on the CSC side (map None: q = k).  Inactive and empty rows: +0.0."""
    T, X = np.asarray(T, dtype=np.float64), np.asarray(X, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    n = len(off) - 1
    live = np.diff(off) > 0
    if active is not None:
        live &= np.asarray(active).astype(bool)
    acc = np.zeros((n, T.shape[1]), dtype=np.float64)
    for rows, at in _walk(off, n):
        m = live[rows]
        rows, at = rows[m], at[m]
        q = at if map is None else map[at].astype(np.int64)
        j = idx[at].astype(np.int64)
        acc[rows] = acc[rows] + a[q][:, None] * T[j]
        if b is not None:
            acc[rows] = acc[rows] + np.asarray(b, dtype=np.float64)[q][:, None] * np.asarray(D, dtype=np.float64)[j]
    out = 2.0 * acc + (2.0 * float(reg)) * X
    out[~live] = 0.0
    return out


def matvec_ref(graph, U, V, r, P, Q, l2, damping=0.0, curvature='full', active=None, e=None):
    """(H + 2 damping I) (P, Q) -> (HU, HV); active = (active_u, active_i) or None."""
    if curvature not in CURVATURES:
        raise ValueError(f"curvature must be 'full' or 'gn', not {curvature!r}")
    g = graph
    au, ai = active if active is not None else (None, None)
    t = coef_ref(g, U, V, r, P, Q)
    b = None
    if curvature == 'full':
        b = coef_ref(g, U, V, r) if e is None else e
    reg = float(l2) + float(damping)
    HU = walk_ref(g.off_u, g.col, None, t, V, b, Q, reg, P, au)
    HV = walk_ref(g.off_i, g.row, g.to_csr, t, U, b, P, reg, Q, ai)
    return HU, HV


def grad_ref(graph, U, V, r, l2, active=None, e=None):
    """grad F -> (gU, gV), +0.0 on inactive and emptied rows."""
    g = graph
    au, ai = active if active is not None else (None, None)
    if e is None:
        e = coef_ref(g, U, V, r)
    U64, V64 = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    return (walk_ref(g.off_u, g.col, None, e, V, None, None, l2, U64, au),
            walk_ref(g.off_i, g.row, g.to_csr, e, U, None, None, l2, V64, ai))


def dot_ref(x, y):
    """sum x y of two float64 vectors of one length in the kernel's two-level order."""
    z = np.asarray(x, dtype=np.float64).reshape(-1) * np.asarray(y, dtype=np.float64).reshape(-1)
    return fold_256([fold_256(z[a:a + DOT_CHUNK]) for a in range(0, max(len(z), 1), DOT_CHUNK)])


def objective_ref(graph, U, V, r, l2, e=None):
    """F(theta) = dot(e, e) + l2 * dot(theta, theta), theta the two tables end to end."""
    if e is None:
        e = coef_ref(graph, U, V, r)
    th = np.concatenate([np.asarray(U, dtype=np.float64).reshape(-1), np.asarray(V, dtype=np.float64).reshape(-1)])
    return dot_ref(e, e) + float(l2) * dot_ref(th, th)


def cg_ref(A, b, iters=512, tol=1e-8):
    """Conjugate gradients on A x = b from x = 0 (A: flat float64 vector -> flat float64 vector), in the kernel's order.
    -> (x, log): log['rr'] float64 [iters_run], log['flag'] int32 [iters_run], 'iters_run' (the iterations up to and including
    the first whose flag is set) and 'status' (the last flag)."""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x, r, p = np.zeros_like(b), b.copy(), b.copy()
    rr = dot_ref(r, r)
    thresh = (float(tol) * float(tol)) * rr
    flag = CONVERGED if rr <= thresh else RUNNING
    hist, flags = [], []
    for _ in range(int(iters)):
        if flag == RUNNING:
            Ap = np.asarray(A(p), dtype=np.float64).reshape(-1)
            pAp = dot_ref(p, Ap)
            if not pAp > 0.0:
                flag = NON_POSITIVE
            else:
                alpha = rr / pAp
                x = x + alpha * p
                r = r - alpha * Ap
                rr_new = dot_ref(r, r)
                beta = rr_new / rr
                rr = rr_new
                if rr <= thresh:
                    flag = CONVERGED
                else:
                    p = r + beta * p
        hist.append(rr)
        flags.append(flag)
        if flag != RUNNING:
            break
    return x, {'rr': np.asarray(hist, dtype=np.float64), 'flag': np.asarray(flags, dtype=np.int32), 'iters_run': len(hist), 'status': int(flag)}


def solve_ref(graph, U, V, r, bU, bV, l2, damping, curvature='full', active=None, e=None, iters=512, tol=1e-8):
    """cg_ref on the shard's system: -> (xU, xV, log)."""
    nu = graph.n_user * np.shape(U)[1]
    if e is None and curvature == 'full':
        e = coef_ref(graph, U, V, r)

    def A(p):
        HU, HV = matvec_ref(graph, U, V, r, p[:nu].reshape(np.shape(U)), p[nu:].reshape(np.shape(V)), l2, damping, curvature, active, e)
        return np.concatenate([HU.reshape(-1), HV.reshape(-1)])
    x, log = cg_ref(A, np.concatenate([np.asarray(bU).reshape(-1), np.asarray(bV).reshape(-1)]), iters, tol)
    return x[:nu].reshape(np.shape(U)), x[nu:].reshape(np.shape(V)), log


def newton_unlearn_ref(uid, iid, rating, U, V, l2, damping=None, curvature='full', steps=1, iters=512, tol=1e-8, scope='all'):
    """The whole update on float32 tables [n_user, d], [n_item, d] and the remaining triples: -> (U, V float32, logs).
    Emptied rows become +0.0 first.  Per step: e, the gradient and the solve at the current theta; a solve that ended with
    status 2, or a step that does not reduce F, is not applied -- the tables keep the last good bytes, the step's log says why
    ('applied': False, 'reason') and no further step is tried."""
    l2, damping = check_args(curvature, damping, steps, iters, tol, l2)
    U, V = np.array(U, dtype=np.float32), np.array(V, dtype=np.float32)
    g = Graph(uid, iid, len(U), len(V))
    r = np.asarray(rating, dtype=np.float32)[g.pos]
    au, ai, eu, ei = active_rows(g, scope)
    U[eu], V[ei] = 0.0, 0.0
    e = coef_ref(g, U, V, r)
    F = objective_ref(g, U, V, r, l2, e)
    logs = []
    for _ in range(steps):
        gU, gV = grad_ref(g, U, V, r, l2, (au, ai), e)
        xU, xV, log = solve_ref(g, U, V, r, -gU, -gV, l2, damping, curvature, (au, ai), e, iters, tol)
        log['F_before'] = F
        if log['status'] == NON_POSITIVE:
            log.update(applied=False, reason='non-positive curvature met by the solve', F_after=F)
            logs.append(log)
            break
        U1, V1 = U.copy(), V.copy()                                          # (only active rows are written: a frozen -0.0 stays)
        U1[au], V1[ai] = (U.astype(np.float64) + xU).astype(np.float32)[au], (V.astype(np.float64) + xV).astype(np.float32)[ai]
        e1 = coef_ref(g, U1, V1, r)
        F1 = objective_ref(g, U1, V1, r, l2, e1)
        if not F1 < F:
            log.update(applied=False, reason='the step did not reduce the objective', F_after=F1)
            logs.append(log)
            break
        U, V, e, F = U1, V1, e1, F1
        log.update(applied=True, reason='', F_after=F1)
        logs.append(log)
    return U, V, logs
