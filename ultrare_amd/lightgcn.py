"""The LightGCN backbone, stated in numpy: the contract of csrc/gcn.hip (include/ultrare_gcn.h) and of engine.GcnJob.

A shard's graph is bipartite: users on one side, items on the other, an edge per training triple (a repeated pair stays two edges;
the rating plays no part in propagation).  With s[node] = float32(1 / sqrt(deg)) the normalised adjacency is A[u][i] = s_u s_i per
edge.  L layers: X^0 = (P, Q) the parameters, X^(l+1) = A X^l, and the model read by everything downstream is the layer mean
(U*, V*) = (1 / (L + 1)) sum_l X^l -- two tables, scored like an MF model.  The loss is MSELoss(sum) of U*[u] . V*[i] against the
rating over a batch; its gradient with respect to (U*, V*) is G; A is symmetric, so the gradient with respect to (P, Q) is
c (G + A G + ... + A^L G), evaluated by Horner's rule with L more propagates; the update is torch's SGD(momentum, weight_decay).

propagate_ref, forward_ref, loss_grad_ref, backward_ref and sgd_update_ref are BIT contracts at dtype float32: every operation is
one float32 operation rounded on its own, a chain is walked in ascending position and never split.  At dtype float64 the same
lines are the float64 restatement (the prediction is then a plain dot).  train_ref is whole training at either dtype.
"""
import numpy as np

MAX_LAYERS = 8
WIDTHS = (4, 8, 16, 32, 64, 128, 256)


class Graph:
    """CSR (users' rows, sorted by (uid, iid, p)) and CSC (items' rows, sorted by (iid, uid, p)) of the triples at file positions
    p = 0 .. N - 1.  off_u [n_user + 1] int64, col [N] int32 (item of a CSR entry), row_u [N] int32 (its user), pos [N] int32 (its file
    position); off_i, row [N] (user of a CSC entry), to_csr [N] int32 (the CSR position of a CSC entry); s_u, s_i float32."""

    def __init__(self, uid, iid, n_user, n_item):
        uid, iid, n_user, n_item = check_triples(uid, iid, n_user, n_item)
        N = len(uid)
        p = np.arange(N)
        csr = np.lexsort((p, iid, uid))
        csc = np.lexsort((p, uid, iid))
        inv = np.empty(N, dtype=np.int64)
        inv[csr] = p
        self.n_user, self.n_item, self.N = n_user, n_item, N
        deg_u, deg_i = np.bincount(uid, minlength=n_user), np.bincount(iid, minlength=n_item)
        self.off_u = np.concatenate([[0], np.cumsum(deg_u)]).astype(np.int64)
        self.off_i = np.concatenate([[0], np.cumsum(deg_i)]).astype(np.int64)
        self.col, self.row_u, self.pos = iid[csr].astype(np.int32), uid[csr].astype(np.int32), csr.astype(np.int32)
        self.row, self.to_csr = uid[csc].astype(np.int32), inv[csc].astype(np.int32)
        self.s_u, self.s_i = inv_sqrt_degree(deg_u), inv_sqrt_degree(deg_i)
        self.inv_deg = False

    def side(self, side):
        """(off, idx, s_src, s_dst, n_dst, n_src) of 'csr' (items -> users) or 'csc' (users -> items)."""
        if side not in ('csr', 'csc'):
            raise ValueError(f"side {side!r}: 'csr' or 'csc'")
        off, idx, s_src, s_dst, n_dst, n_src = ((self.off_u, self.col, self.s_i, self.s_u, self.n_user, self.n_item) if side == 'csr' else
                                                (self.off_i, self.row, self.s_u, self.s_i, self.n_item, self.n_user))
        if self.inv_deg:                                # (tests only: the plant 1 / deg_dst in place of s_dst s_src)
            s_src, s_dst = np.ones_like(s_src), (s_dst.astype(np.float64) ** 2).astype(np.float32)
        return off, idx, s_src, s_dst, n_dst, n_src


def check_triples(uid, iid, n_user, n_item):
    """The argument checks of a graph: -> (uid int64, iid int64, n_user, n_item), or ValueError."""
    uid, iid = np.asarray(uid), np.asarray(iid)
    n_user, n_item = int(n_user), int(n_item)
    if uid.ndim != 1 or uid.shape != iid.shape:
        raise ValueError(f'uid and iid must be one-dimensional and equally long, not {uid.shape} and {iid.shape}')
    if not (1 <= n_user < 2 ** 31 and 1 <= n_item < 2 ** 31 and len(uid) < 2 ** 31):
        raise ValueError('n_user and n_item must lie in 1 .. 2^31 - 1, and there must be fewer than 2^31 triples')
    uid, iid = uid.astype(np.int64), iid.astype(np.int64)
    if len(uid) and (uid.min() < 0 or uid.max() >= n_user):
        raise ValueError(f'a user id lies outside [0, {n_user})')
    if len(iid) and (iid.min() < 0 or iid.max() >= n_item):
        raise ValueError(f'an item id lies outside [0, {n_item})')
    return uid, iid, n_user, n_item


def check_layers(layers):
    if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or not 0 <= layers <= MAX_LAYERS:
        raise ValueError(f'layers must be an integer in 0 .. {MAX_LAYERS}, not {layers!r}')
    return int(layers)


def check_width(d):
    if d not in WIDTHS:
        raise ValueError(f'd must be a power of two in 4 .. 256, not {d!r}')
    return int(d)


def inv_sqrt_degree(deg):
    """s = float32(1 / sqrt(float64(deg))), 0 for deg = 0."""
    deg = np.asarray(deg, dtype=np.float64)
    with np.errstate(divide='ignore'):
        return np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0).astype(np.float32)


def layer_scale(layers):
    return np.float32(1.0 / (layers + 1))


def _walk(off, n_rows):
    """The entries of every row one rank at a time: yields (rows, positions) for rank 0, 1, ... -- every chain advances in ascending
    position, all rows side by side."""
    length = np.diff(off)
    for j in range(int(length.max()) if n_rows else 0):
        rows = np.flatnonzero(length > j)
        yield rows, off[rows] + j


def propagate_ref(off, idx, s_src, s_dst, X, add=None, sum=None, dtype=np.float32):
    """out[r][c] = [add[r][c] +] s_dst[r] * (sum over the row's entries j, ascending, from +0: s_src[j] * X[j][c]), every operation
    rounded on its own; sum (if given) is advanced IN PLACE by the value stored.  An empty row gives +0 (or add)."""
    T = dtype
    X, s_src, s_dst = np.asarray(X, dtype=T), np.asarray(s_src).astype(T), np.asarray(s_dst).astype(T)
    n = len(off) - 1
    t = np.zeros((n, X.shape[1]), dtype=T)
    for rows, at in _walk(off, n):
        j = idx[at]
        t[rows] = t[rows] + s_src[j][:, None] * X[j]
    y = s_dst[:, None] * t
    if add is not None:
        y = np.asarray(add, dtype=T) + y
    if sum is not None:
        assert sum.dtype == T
        sum[...] = sum + y
    return y


def forward_ref(g, P, Q, layers, dtype=np.float32):
    """-> (U*, V*): the layer mean of the parameters and their `layers` propagations."""
    T = dtype
    Xu, Xi = np.array(P, dtype=T), np.array(Q, dtype=T)
    Su, Si = Xu.copy(), Xi.copy()
    for _ in range(layers):
        Xu, Xi = (propagate_ref(*g.side('csr')[:4], Xi, sum=Su, dtype=T), propagate_ref(*g.side('csc')[:4], Xu, sum=Si, dtype=T))
    c = T(layer_scale(layers))
    return Su * c, Si * c


def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in float64, the sum is rounded to odd there (Boldo-Melquiond), so the
    final rounding to float32 is the single rounding of the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                                      # TwoSum: p + c = s + err exactly
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def score_ref(U, V, uid, iid):
    """ure_score of ONE model at the pairs (uid, iid), bit for bit (csrc/score_dot.h): a lane holds four consecutive columns and
    runs p = a0 b0, p = fmaf(a_k, b_k, p); the d / 4 lane values are added as a balanced tree of adjacent pairs."""
    a, b = np.asarray(U, dtype=np.float32)[uid], np.asarray(V, dtype=np.float32)[iid]
    d = 4
    while d < a.shape[1]:
        d *= 2                                                              # the device's width: zero columns up to a power of two
    a, b = (np.pad(t, ((0, 0), (0, d - t.shape[1]))).reshape(len(t), -1, 4) for t in (a, b))
    p = a[..., 0] * b[..., 0]
    for k in (1, 2, 3):
        p = _fma32(a[..., k], b[..., k], p)
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def loss_grad_ref(g, Ustar, Vstar, rating, batch_idx, dtype=np.float32):
    """The batch = the triples at the file positions batch_idx.  -> (G_u, G_i, loss, pred [N] with NaN outside the batch):
    e_p = pred_p - r_p; G_u[u] = the chain from +0 over the row's CSR entries in the batch, ascending CSR position, of
    (2 e_p) * V*[iid_p]; G_i likewise over the CSC with U*; loss = sum e_p^2 in float64 -- per user a chain over the same entries
    from 0.0, the users then added as ure_epoch_sse_batch adds them (lane t of 256 takes the users t, t + 256, ... in ascending
    order, the 256 lane sums are folded pairwise: w = 128, 64, ... 1, lane t += lane t + w)."""
    T = dtype
    Ustar, Vstar = np.asarray(Ustar, dtype=T), np.asarray(Vstar, dtype=T)
    in_batch = np.zeros(g.N, dtype=bool)
    in_batch[np.asarray(batch_idx, dtype=np.int64)] = True                  # by file position
    in_csr = in_batch[g.pos]
    u, i = g.row_u.astype(np.int64), g.col.astype(np.int64)
    r = np.asarray(rating).astype(T)[g.pos]
    if T == np.float32:
        pred = score_ref(Ustar, Vstar, u, i)
    else:
        pred = (Ustar[u] * Vstar[i]).sum(axis=1, dtype=T)
    e = pred - r
    ge = T(2) * e
    Gu, Gi = np.zeros_like(Ustar), np.zeros_like(Vstar)
    row_loss = np.zeros(g.n_user, dtype=np.float64)
    for rows, at in _walk(g.off_u, g.n_user):
        m = in_csr[at]
        rows, at = rows[m], at[m]
        Gu[rows] = Gu[rows] + ge[at][:, None] * Vstar[i[at]]
        row_loss[rows] = row_loss[rows] + e[at].astype(np.float64) * e[at].astype(np.float64)
    for rows, at in _walk(g.off_i, g.n_item):
        k = g.to_csr[at]
        m = in_csr[k]
        rows, k = rows[m], k[m]
        Gi[rows] = Gi[rows] + ge[k][:, None] * Ustar[u[k]]
    pred_file = np.full(g.N, np.nan, dtype=T)
    pred_file[g.pos[in_csr]] = pred[in_csr]
    return Gu, Gi, fold_256(row_loss), pred_file


def fold_256(x):
    """ure_epoch_sse_batch's order over float64 values: lane t of 256 adds x[t], x[t + 256], ... from 0.0; pairwise fold."""
    x = np.asarray(x, dtype=np.float64)
    pad = np.zeros(-(-max(len(x), 1) // 256) * 256)
    pad[:len(x)] = x
    part = np.zeros(256)
    for chunk in pad.reshape(-1, 256):
        part = part + chunk
    w = 128
    while w > 0:
        part[:w] = part[:w] + part[w:2 * w]
        w >>= 1
    return float(part[0])


def backward_ref(g, Gu, Gi, layers, dtype=np.float32, plant=None):
    """-> (gP, gQ) = c H^L with H^0 = G, H_u^l = G_u + prop_CSR(H_i^(l-1)), H_i^l = G_i + prop_CSC(H_u^(l-1))."""
    T = dtype
    Gu, Gi = np.asarray(Gu, dtype=T), np.asarray(Gi, dtype=T)
    Hu, Hi = Gu, Gi
    for _ in range(layers):
        add = (None, None) if plant == 'no_readd' else (Gu, Gi)
        Hu, Hi = (propagate_ref(*g.side('csr')[:4], Hi, add=add[0], dtype=T), propagate_ref(*g.side('csc')[:4], Hu, add=add[1], dtype=T))
    c = T(layer_scale(layers))
    return Hu * c, Hi * c


def sgd_update_ref(w, m, g, lr, lam, mu, first, dtype=np.float32):
    """torch.optim.SGD(momentum=mu, weight_decay=lam): g' = g + lam w; m = g' on the first step of the job, else mu m + g';
    w = w - lr m.  -> (w, m).  lam, mu and lr are taken at their float32 values."""
    T = dtype
    lr, lam, mu = T(np.float32(lr)), T(np.float32(lam)), T(np.float32(mu))
    w, m, g = np.asarray(w, dtype=T), np.asarray(m, dtype=T), np.asarray(g, dtype=T)
    g1 = g + lam * w
    m = g1 if first else mu * m + g1
    return w - lr * m, m


PLANTS = ('no_layer0', 'no_readd', 'inv_deg', 'stale_lr')


def train_ref(uid, iid, rating, P0, Q0, orders, batch, lr_host, lam, mu, layers, dtype=np.float64, plant=None):
    """Whole training of one shard: per epoch e and step t the batch orders[e][t B : (t + 1) B], forward, loss gradient, backward,
    update.  -> dict: U, V [epochs, ...] the final tables (U*, V*) after every epoch, P, Q [epochs, ...] the parameters, loss [epochs]
    = sqrt(the epoch's summed batch losses / N) as sgd_cases.sgd_train_ref reports it, sse [epochs] the sums themselves.
    dtype=np.float32 is the bit contract of engine.GcnJob.
    plant (tests only), one of PLANTS: the layer-0 term missing from the mean; a backward that does not re-add G; 1 / deg in place of
    1 / sqrt(deg_u deg_i); the previous epoch's lr in an epoch's first step."""
    assert plant is None or plant in PLANTS
    T = dtype
    layers = check_layers(layers)
    g = Graph(uid, iid, len(P0), len(Q0))
    g.inv_deg = plant == 'inv_deg'
    lr_host = np.asarray(lr_host, dtype=np.float32)
    P, Q = np.array(P0, dtype=T), np.array(Q0, dtype=T)
    mP, mQ = np.zeros_like(P), np.zeros_like(Q)
    N, E = g.N, len(orders)
    steps = (N + batch - 1) // batch
    out = dict(U=[], V=[], P=[], Q=[])
    sse, first = np.zeros(E), True

    def forward():
        U, V = forward_ref(g, P, Q, layers, dtype=T)
        if plant == 'no_layer0' and layers:
            c = T(layer_scale(layers))
            U, V = U - P * c, V - Q * c
        return U, V

    for e in range(E):
        for t in range(steps):
            lr = lr_host[e - 1 if plant == 'stale_lr' and t == 0 and e > 0 else e]
            U, V = forward()
            Gu, Gi, loss, _ = loss_grad_ref(g, U, V, rating, orders[e][t * batch:(t + 1) * batch], dtype=T)
            sse[e] += loss
            gP, gQ = backward_ref(g, Gu, Gi, layers, dtype=T, plant=plant)
            if plant == 'no_layer0' and layers:
                c = T(layer_scale(layers))
                gP, gQ = gP - Gu * c, gQ - Gi * c
            P, mP = sgd_update_ref(P, mP, gP, lr, lam, mu, first, dtype=T)
            Q, mQ = sgd_update_ref(Q, mQ, gQ, lr, lam, mu, first, dtype=T)
            first = False
        U, V = forward()
        for name, a in (('U', U), ('V', V), ('P', P), ('Q', Q)):
            out[name].append(a.copy())
    out = {k: np.stack(v) for k, v in out.items()}
    out['sse'], out['loss'] = sse, np.sqrt(sse / max(N, 1))
    return out
