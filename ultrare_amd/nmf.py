"""The NeuMF backbone, stated in numpy: the contract of csrc/nmf.hip (include/ultrare_nmf.h) and of engine.NmfJob.

NeuMF (He et al. 2017) as rating regression.  A model is two tables and one vector:
    U [n_user, k + e] = [user_mat_mf | user_mat_mlp],  V [n_item, k + e] = [item_mat_mf | item_mat_mlp],  e = layers[0] / 2
    dense = W_0 [L1, L0] row-major, b_0 [L1], W_1, b_1, ..., h [k + Lm], c, zeros up to a multiple of 4
For a pair (u, i): g = pg * qg, a_0 = [pm ; qm], a_(j+1) = relu(W_j a_j + b_j), pred = c + h[:k] . g + h[k:] . a_m; the loss is
MSELoss(sum) against the rating, the derivative of relu at a pre-activation <= 0 is 0, the update is torch's SGD(momentum,
weight_decay) over every parameter.

forward_ref, backward_ref, weight_grad_ref, row_sum_ref, score_ref, sse_ref and lightgcn.sgd_update_ref are BIT contracts at dtype
float32: every operation is one float32 operation rounded on its own, a chain is walked in ascending index from +0.0 and never split
(but the weight-gradient sums, which are chains over chunks of CHUNK slots whose sums are then added in chunk order).  At dtype
float64 the same lines are the float64 restatement.  train_ref is whole training at either dtype.

A step's batch is named by rank: rank[q] is the place of CSR entry q in the epoch's order; entry q is in step s iff
s B <= rank[q] < (s + 1) B and its slot is rank[q] - s B.  Per-entry intermediates are indexed by slot, so the weight-gradient
sums run in the batch's own sample order.
"""
import numpy as np

from . import lightgcn
from .lightgcn import sgd_update_ref                      # noqa: F401  (the update is LightGCN's, over tables and dense alike)

MAX_FC = 4
MAX_WIDTH = 128
CHUNK = 256                     # URE_NMF_CHUNK
LDS_BYTES = 61440               # URE_NMF_LDS_BYTES: what a workgroup stages of a stack


class Shape:
    """Where everything of a (k, layers) lies: in the dense vector, in an act row [g | a_0 | .. | a_m] and in a dlt row
    [delta_1 | .. | delta_m] (csrc/nmf.hip: NmfShape)."""

    def __init__(self, k, layers):
        self.k, self.layers = k, layers = check_layers(k, layers)
        self.m, self.e = len(layers) - 1, layers[0] // 2
        self.wd = k + self.e
        at, self.w_at, self.b_at = 0, [], []
        for j in range(self.m):
            self.w_at.append(at)
            at += layers[j + 1] * layers[j]
            self.b_at.append(at)
            at += layers[j + 1]
        self.h_at, self.c_at = at, at + k + layers[-1]
        self.n_real = self.c_at + 1
        self.n_dense = (self.n_real + 3) // 4 * 4
        self.a_at = [k + sum(layers[:j]) for j in range(self.m + 1)]
        self.A = k + sum(layers)
        self.d_at = [0] + [sum(layers[1:j]) for j in range(1, self.m + 1)]          # d_at[j], j = 1 .. m ([0] unused)
        self.Dw = sum(layers[1:])

    def unpack(self, dense):
        """-> (W [m] of [L_(j+1), L_j], b [m], h [k + Lm], c) as views of the dense vector."""
        L = self.layers
        W = [dense[self.w_at[j]:self.b_at[j]].reshape(L[j + 1], L[j]) for j in range(self.m)]
        b = [dense[self.b_at[j]:self.b_at[j] + L[j + 1]] for j in range(self.m)]
        return W, b, dense[self.h_at:self.c_at], dense[self.c_at]

    def pack(self, W, b, h, c, dtype=np.float32):
        dense = np.zeros(self.n_dense, dtype=dtype)
        for j in range(self.m):
            dense[self.w_at[j]:self.b_at[j]] = np.asarray(W[j]).reshape(-1)
            dense[self.b_at[j]:self.b_at[j] + self.layers[j + 1]] = b[j]
        dense[self.h_at:self.c_at] = h
        dense[self.c_at] = c
        return dense


def lds_bytes(k, layers):
    """The LDS a workgroup of the kernels needs for the stack (include/ultrare_nmf.h)."""
    w = sum(layers[j] * (layers[j + 1] + 1) + layers[j + 1] for j in range(len(layers) - 1)) + k + layers[-1] + 1
    return 4 * (w + 4 * (k + sum(layers) + 2 * MAX_WIDTH))


def check_layers(k, layers):
    """The argument checks of a model: -> (k, [L0 .. Lm]) as ints, or ValueError.  k and L1 .. Lm are powers of two in 4 .. 128,
    L0 in 8 .. 128, 1 <= m <= 4, and the stack fits the kernels' LDS budget."""
    def width(v, lo, what):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= MAX_WIDTH or v & (v - 1):
            raise ValueError(f'nmf: {what} must be a power of two in {lo} .. {MAX_WIDTH}, not {v!r}')
        return int(v)
    if isinstance(layers, (str, bytes)) or not hasattr(layers, '__len__'):
        raise ValueError(f'nmf: layers must be a list [L0, L1, ..., Lm], not {layers!r}')
    if not 2 <= len(layers) <= MAX_FC + 1:
        raise ValueError(f'nmf: layers must hold 2 .. {MAX_FC + 1} widths (1 .. {MAX_FC} fully connected layers), not {len(layers)}')
    k = width(k, 4, 'k')
    layers = [width(v, 8 if j == 0 else 4, f'layers[{j}]') for j, v in enumerate(layers)]
    if lds_bytes(k, layers) > LDS_BYTES:
        raise ValueError(f'nmf: k = {k}, layers = {layers} needs {lds_bytes(k, layers)} bytes of LDS per workgroup; the kernels stage at most {LDS_BYTES}')
    return k, layers


def check_model(U, V, dense, k, layers, n_user=None, n_item=None):
    """-> Shape, or ValueError for tables or a dense vector of the wrong shape."""
    S = Shape(k, layers)
    for name, t, rows in (('U', U, n_user), ('V', V, n_item)):
        if len(np.shape(t)) != 2 or np.shape(t)[1] != S.wd or (rows is not None and np.shape(t)[0] != rows) or np.shape(t)[0] < 1:
            raise ValueError(f'nmf: {name} has shape {tuple(np.shape(t))}: [{"rows" if rows is None else rows}, {S.wd}] (k + layers[0] / 2 columns) is needed')
    if tuple(np.shape(dense)) != (S.n_dense,):
        raise ValueError(f'nmf: dense has shape {tuple(np.shape(dense))}: ({S.n_dense},) is needed for k = {S.k}, layers = {S.layers}')
    return S


PLANTS = ('relu_leak', 'no_bias_grad', 'head_swapped', 'stale_lr')


def _head(S, h, plant):
    """(the head's weights of g, of a_m): h = [hg | ha]; the plant reads it as [ha | hg]."""
    Lm = S.layers[-1]
    return (h[Lm:], h[:Lm]) if plant == 'head_swapped' else (h[:S.k], h[S.k:])


def forward_ref(U, V, dense, k, layers, uid, iid, dtype=np.float32, plant=None):
    """-> (pred [n], act [n, A]) at the pairs (uid, iid): act = [g | a_0 | .. | a_m] per pair."""
    T = dtype
    S = Shape(k, layers)
    W, b, h, c = S.unpack(np.asarray(dense, dtype=T))
    u, v = np.asarray(U, dtype=T)[uid], np.asarray(V, dtype=T)[iid]
    n = len(u)
    act = np.zeros((n, S.A), dtype=T)
    act[:, :k] = u[:, :k] * v[:, :k]
    act[:, k:k + S.e], act[:, k + S.e:k + 2 * S.e] = u[:, k:], v[:, k:]
    for j in range(S.m):
        a = act[:, S.a_at[j]:S.a_at[j] + S.layers[j]]
        t = np.zeros((n, S.layers[j + 1]), dtype=T)
        for i in range(S.layers[j]):
            t = t + W[j][:, i][None, :] * a[:, i][:, None]
        z = t + b[j][None, :]
        act[:, S.a_at[j + 1]:S.a_at[j + 1] + S.layers[j + 1]] = np.where(z <= 0, T(0), z)
    hg, ha = _head(S, h, plant)
    am = act[:, S.a_at[S.m]:]
    t = np.zeros(n, dtype=T)
    for col in range(k):
        t = t + hg[col] * act[:, col]
    for col in range(S.layers[-1]):
        t = t + ha[col] * am[:, col]
    return t + c, act


def backward_ref(U, V, dense, k, layers, uid, iid, act, err, dtype=np.float32, plant=None):
    """-> (dlt [n, Dw] = [delta_1 | .. | delta_m], emb [n, 2 (k + e)] = [dpg | dpm | dqg | dqm]) of sum err^2 per pair."""
    T = dtype
    S = Shape(k, layers)
    W, b, h, c = S.unpack(np.asarray(dense, dtype=T))
    u, v = np.asarray(U, dtype=T)[uid], np.asarray(V, dtype=T)[iid]
    act, n = np.asarray(act, dtype=T), len(u)
    ge = T(2) * np.asarray(err, dtype=T)
    hg, ha = _head(S, h, plant)
    dlt, emb = np.zeros((n, S.Dw), dtype=T), np.zeros((n, 2 * S.wd), dtype=T)
    dg = ge[:, None] * hg[None, :]
    emb[:, :k], emb[:, S.wd:S.wd + k] = dg * v[:, :k], dg * u[:, :k]
    a_of = lambda j: act[:, S.a_at[j]:S.a_at[j] + S.layers[j]]
    mask = lambda a, d: d if plant == 'relu_leak' else np.where(a > 0, d, T(0))
    d = mask(a_of(S.m), ge[:, None] * ha[None, :])
    dlt[:, S.d_at[S.m]:S.d_at[S.m] + S.layers[S.m]] = d
    for j in range(S.m - 1, -1, -1):
        t = np.zeros((n, S.layers[j]), dtype=T)
        for o in range(S.layers[j + 1]):
            t = t + W[j][o][None, :] * d[:, o][:, None]
        if j > 0:
            d = mask(a_of(j), t)
            dlt[:, S.d_at[j]:S.d_at[j] + S.layers[j]] = d
        else:
            emb[:, k:S.wd], emb[:, S.wd + k:] = t[:, :S.e], t[:, S.e:]
    return dlt, emb


def _chunk_chain(terms):
    """The two-level chain over axis 0: chunks of CHUNK rows in ascending order from +0.0, the chunk sums added in chunk order
    starting from the first."""
    total = None
    for s0 in range(0, len(terms), CHUNK):
        t = np.zeros(terms.shape[1:], dtype=terms.dtype)
        for row in terms[s0:s0 + CHUNK]:
            t = t + row
        total = t if total is None else total + t
    return total


def weight_grad_ref(err, act, dlt, k, layers, dtype=np.float32, plant=None):
    """-> g_dense, laid out as dense (the padding +0.0), from the slots' rows in slot order."""
    T = dtype
    S = Shape(k, layers)
    err, act, dlt = np.asarray(err, dtype=T), np.asarray(act, dtype=T), np.asarray(dlt, dtype=T)
    ge = T(2) * err
    W, b = [], []
    for j in range(S.m):
        d = dlt[:, S.d_at[j + 1]:S.d_at[j + 1] + S.layers[j + 1]]
        a = act[:, S.a_at[j]:S.a_at[j] + S.layers[j]]
        W.append(_chunk_chain(d[:, :, None] * a[:, None, :]))
        b.append(np.zeros(S.layers[j + 1], dtype=T) if plant == 'no_bias_grad' else _chunk_chain(d))
    feat = np.concatenate([act[:, :k], act[:, S.a_at[S.m]:]], axis=1)
    gh = _chunk_chain(ge[:, None] * feat)
    if plant == 'head_swapped':
        gh = np.concatenate([gh[k:], gh[:k]])
    return S.pack(W, b, gh, _chunk_chain(ge), dtype=T)


def row_sum_ref(off, map, rank, lo, n_slots, E, col0, width, err=None, dtype=np.float32):
    """-> (G [n_rows, width], row_loss float64 [n_rows] or None): per row the chain from +0.0, over its entries in the batch in
    ascending position, of E[slot][col0 : col0 + width]; row_loss the float64 chain of err[slot]^2 over the same entries."""
    T = dtype
    E, n_rows = np.asarray(E, dtype=T), len(off) - 1
    rank = np.asarray(rank, dtype=np.int64)
    G = np.zeros((n_rows, width), dtype=T)
    row_loss = None if err is None else np.zeros(n_rows, dtype=np.float64)
    for rows, at in lightgcn._walk(np.asarray(off), n_rows):
        q = at if map is None else np.asarray(map)[at]
        s = rank[q] - lo
        m = (s >= 0) & (s < n_slots)
        rows, s = rows[m], s[m]
        G[rows] = G[rows] + E[s, col0:col0 + width]
        if err is not None:
            ee = np.asarray(err)[s].astype(np.float64)
            row_loss[rows] = row_loss[rows] + ee * ee
    return G, row_loss


def score_ref(models, k, layers, uid, iid, dtype=np.float32):
    """The ensemble mean of `models` = [(U, V, dense), ...] at the pairs under ure_score's protocol: acc = 0; acc = fl(acc + p_s)
    in list order; pred = fl(acc / S)."""
    T = dtype
    acc = np.zeros(len(uid), dtype=T)
    for U, V, dense in models:
        acc = acc + forward_ref(U, V, dense, k, layers, uid, iid, dtype=T)[0]
    return acc / T(len(models))


SCORE_PARTIALS = 2048           # URE_SCORE_PARTIALS


def sse_ref(pred, rating):
    """The SCORE_PARTIALS doubles ure_nmf_score writes to sse on its last call, bit for bit: W = min(ceil(n / 4), SCORE_PARTIALS)
    workgroups of four waves; wave w takes the pairs w, w + 4 W, ... in ascending order and runs sq = fmaf(er, er, sq) from +0.0
    with er = fl(pred - rating); a workgroup's partial is the float64 chain from 0.0 over its four waves; zeros behind."""
    pred, rating = np.asarray(pred, dtype=np.float32), np.asarray(rating, dtype=np.float32)
    n = len(pred)
    blocks = min(-(-n // 4), SCORE_PARTIALS)
    n_waves = 4 * blocks
    er = pred - rating
    sq = np.zeros(n_waves, dtype=np.float32)
    for j0 in range(0, n, n_waves):
        e = er[j0:j0 + n_waves]
        sq[:len(e)] = lightgcn._fma32(e, e, sq[:len(e)])
    out = np.zeros(SCORE_PARTIALS, dtype=np.float64)
    part = sq.reshape(blocks, 4).astype(np.float64)
    t = np.zeros(blocks)
    for w in range(4):
        t = t + part[:, w]
    out[:blocks] = t
    return out


def batch_entries(rank, lo, n_slots):
    """The CSR entry of every slot 0 .. n_slots - 1 of the batch lo <= rank < lo + n_slots (rank a permutation)."""
    s = np.asarray(rank, dtype=np.int64) - lo
    q = np.flatnonzero((s >= 0) & (s < n_slots))
    return q[np.argsort(s[q])]


def step_ref(g, rating_csr, rank, lo, n_slots, U, V, dense, k, layers, dtype=np.float32, plant=None):
    """One step's gradients: -> (gU, gV, g_dense, loss): forward and backward of the batch's entries in slot order, the
    weight-gradient sums, the two masked row sums and the loss (lightgcn.fold_256 over the users' float64 chains)."""
    T = dtype
    S = Shape(k, layers)
    q = batch_entries(rank, lo, n_slots)
    uid, iid = g.row_u[q].astype(np.int64), g.col[q].astype(np.int64)
    pred, act = forward_ref(U, V, dense, k, layers, uid, iid, dtype=T, plant=plant)
    err = pred - np.asarray(rating_csr).astype(T)[q]
    dlt, emb = backward_ref(U, V, dense, k, layers, uid, iid, act, err, dtype=T, plant=plant)
    g_dense = weight_grad_ref(err, act, dlt, k, layers, dtype=T, plant=plant)
    gU, row_loss = row_sum_ref(g.off_u, None, rank, lo, n_slots, emb, 0, S.wd, err=err, dtype=T)
    gV, _ = row_sum_ref(g.off_i, g.to_csr, rank, lo, n_slots, emb, S.wd, S.wd, dtype=T)
    return gU, gV, g_dense, lightgcn.fold_256(row_loss)


def epoch_rank(g, order):
    """rank [nnz] int32 in CSR order from an epoch's order (file positions in training order)."""
    file_rank = np.empty(g.N, dtype=np.int32)
    file_rank[np.asarray(order, dtype=np.int64)] = np.arange(g.N, dtype=np.int32)
    return file_rank[g.pos]


def train_ref(uid, iid, rating, U0, V0, dense0, orders, batch, lr_host, lam, mu, k, layers, dtype=np.float64, plant=None):
    """Whole training of one shard: per epoch e and step t the batch orders[e][t B : (t + 1) B].  -> dict: U, V, dense
    [epochs, ...] the parameters after every epoch, sse [epochs] the epoch's summed batch losses, loss = sqrt(sse / N).
    dtype=np.float32 is the bit contract of engine.NmfJob.
    plant (tests only), one of PLANTS: a relu that passes the gradient at a pre-activation <= 0; no bias gradient; a head that
    reads its input as [a_m ; g]; the previous epoch's lr in an epoch's first step."""
    assert plant is None or plant in PLANTS
    T = dtype
    S = check_model(U0, V0, dense0, k, layers)
    g = lightgcn.Graph(uid, iid, len(U0), len(V0))
    r_csr = np.asarray(rating)[g.pos]
    lr_host = np.asarray(lr_host, dtype=np.float32)
    U, V, dense = np.array(U0, dtype=T), np.array(V0, dtype=T), np.array(dense0, dtype=T)
    mU, mV, md = np.zeros_like(U), np.zeros_like(V), np.zeros_like(dense)
    N, E = g.N, len(orders)
    steps = (N + batch - 1) // batch
    out = dict(U=[], V=[], dense=[])
    sse, first = np.zeros(E), True
    for e in range(E):
        rank = epoch_rank(g, orders[e])
        for t in range(steps):
            lr = lr_host[e - 1 if plant == 'stale_lr' and t == 0 and e > 0 else e]
            lo = t * batch
            gU, gV, gd, loss = step_ref(g, r_csr, rank, lo, min(batch, N - lo), U, V, dense, S.k, S.layers, dtype=T, plant=plant)
            sse[e] += loss
            U, mU = sgd_update_ref(U, mU, gU, lr, lam, mu, first, dtype=T)
            V, mV = sgd_update_ref(V, mV, gV, lr, lam, mu, first, dtype=T)
            dense, md = sgd_update_ref(dense, md, gd, lr, lam, mu, first, dtype=T)
            first = False
        for name, a in (('U', U), ('V', V), ('dense', dense)):
            out[name].append(a.copy())
    out = {name: np.stack(v) for name, v in out.items()}
    out['sse'], out['loss'] = sse, np.sqrt(sse / max(N, 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Catalogue sweeps (csrc/nmf_rank.hip, include/ultrare_nmf_rank.h): top-k and exact ranks under an ensemble.
# ---------------------------------------------------------------------------------------------------------------------
RANK_LDS_BYTES = 163840         # URE_NMF_RANK_LDS_BYTES: what a workgroup of the tile kernels may hold
RANK_PLANTS = ('fma', 'item_first')


def prefix_ref(U, dense, k, layers, uid, dtype=np.float32):
    """-> [n, L1]: the layer-0 chains of forward_ref stopped after the user half -- output o's chain over a_0 = [pm ; qm] in
    ascending i from +0.0, its first e terms.  They depend on (model, user, o) alone; the tile kernel sums them once per user."""
    T = dtype
    S = Shape(k, layers)
    W = S.unpack(np.asarray(dense, dtype=T))[0]
    pm = np.asarray(U, dtype=T)[uid][:, S.k:]
    t = np.zeros((len(pm), S.layers[1]), dtype=T)
    for i in range(S.e):
        t = t + W[0][:, i][None, :] * pm[:, i][:, None]
    return t


def forward_from_prefix_ref(prefix, V, dense, k, layers, U, uid, iid, dtype=np.float32, plant=None, want_a1=False):
    """-> pred [n] (want_a1: (pred, a_1 [n, L1])): forward_ref's prediction with the layer-0 chains of pair j continued from prefix[j] (prefix_ref at uid) over
    qm, then the rest of the stack, the GMF products and the head.  The same float32 operations in the same order as forward_ref,
    hence the same bytes.
    plant (tests only), one of RANK_PLANTS: every chain's terms as fused multiply-adds; the item half summed from +0.0 on its
    own and added to the prefix."""
    assert plant is None or plant in RANK_PLANTS
    T = dtype
    S = Shape(k, layers)
    W, b, h, c = S.unpack(np.asarray(dense, dtype=T))
    u, v = np.asarray(U, dtype=T)[uid], np.asarray(V, dtype=T)[iid]
    n, e = len(v), S.e
    def mad(t, w, x):                                       # one term of a chain: fl(t + fl(w * x)); the plant: fmaf(w, x, t)
        if plant != 'fma':
            return t + w * x
        w, x = np.broadcast_arrays(np.asarray(w, dtype=T), np.asarray(x, dtype=T))
        return lightgcn._fma32(*np.broadcast_arrays(w, x, t)).astype(T)
    t = np.array(prefix, dtype=T)
    if plant == 'item_first':
        t = np.zeros_like(t)
    for i in range(e):
        t = mad(t, W[0][:, e + i][None, :], v[:, k + i][:, None])
    if plant == 'item_first':
        t = np.asarray(prefix, dtype=T) + t
    z = t + b[0][None, :]
    a = a1 = np.where(z <= 0, T(0), z)
    for j in range(1, S.m):
        t = np.zeros((n, S.layers[j + 1]), dtype=T)
        for i in range(S.layers[j]):
            t = mad(t, W[j][:, i][None, :], a[:, i][:, None])
        z = t + b[j][None, :]
        a = np.where(z <= 0, T(0), z)
    g = u[:, :k] * v[:, :k]
    t = np.zeros(n, dtype=T)
    for col in range(k):
        t = mad(t, h[col], g[:, col])
    for col in range(S.layers[-1]):
        t = mad(t, h[k + col], a[:, col])
    return (t + c, a1) if want_a1 else t + c


def order_bits(s):
    """rec_score.h's order_bits of float32 scores as uint32: larger for the better score; NaN below -inf, -0.0 == +0.0."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    b = s.view(np.uint32).copy()
    b[(b << np.uint32(1)) == 0] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    out = np.where(neg, ~b, b | np.uint32(0x80000000))
    out[np.isnan(s)] = 0
    return out.astype(np.uint32)


def rank_keys(s, items):
    """rec_key: (order_bits(score) << 32) | ~item as uint64 -- larger for the better item, unique per item."""
    return (order_bits(s).astype(np.uint64) << np.uint64(32)) | (~np.asarray(items).astype(np.uint32)).astype(np.uint64)


def _excl_row(excl, q):
    return np.zeros(0, dtype=np.int64) if excl is None else np.asarray(excl[1])[excl[0][q]:excl[0][q + 1]].astype(np.int64)


def catalogue_scores_ref(models, k, layers, users, n_item):
    """-> [n, n_item] float32: score_ref of every (user, item) pair."""
    users = np.asarray(users, dtype=np.int64)
    items = np.arange(n_item, dtype=np.int64)
    return np.stack([score_ref(models, k, layers, np.full(n_item, u, dtype=np.int64), items) for u in users]).astype(np.float32)


def recommend_ref(models, k, layers, users, n_item, top_k, excl=None, scores=None):
    """ure_nmf_recommend_topk: -> (scores [n, top_k] float32, items [n, top_k] int64): per query row the top_k non-excluded items
    under score_ref's ensemble mean, in key order (score descending, NaN below -inf, -0.0 == +0.0, then item id ascending);
    padding is (NaN, -1).  excl = (off [n + 1], items) or None.  scores: catalogue_scores_ref's matrix when the caller has it."""
    sc = catalogue_scores_ref(models, k, layers, users, n_item) if scores is None else np.asarray(scores, dtype=np.float32)
    n = len(sc)
    out_s, out_i = np.full((n, top_k), np.nan, dtype=np.float32), np.full((n, top_k), -1, dtype=np.int64)
    for q in range(n):
        keep = np.ones(n_item, dtype=bool)
        keep[_excl_row(excl, q)] = False
        ids = np.flatnonzero(keep)
        best = ids[np.argsort(rank_keys(sc[q, ids], ids))[::-1][:top_k]]
        out_s[q, :len(best)], out_i[q, :len(best)] = sc[q, best], best
    return out_s, out_i


def rank_ref(models, k, layers, users, targets, excl=None, scores=None, n_item=None):
    """ure_nmf_rank_pairs: -> ranks int32 [n_targets] in input order: for target t of query row q the number of non-excluded items
    whose key beats t's, -1 when t is excluded.  targets = (off [n + 1], items): any order, duplicates, empty rows."""
    n_item = len(models[0][1]) if n_item is None else n_item
    sc = catalogue_scores_ref(models, k, layers, users, n_item) if scores is None else np.asarray(scores, dtype=np.float32)
    t_off, t_items = np.asarray(targets[0], dtype=np.int64), np.asarray(targets[1], dtype=np.int64)
    ranks = np.zeros(len(t_items), dtype=np.int32)
    for q in range(len(sc)):
        keep = np.ones(n_item, dtype=bool)
        keep[_excl_row(excl, q)] = False
        keys = rank_keys(sc[q], np.arange(n_item))
        live = np.sort(keys[keep])
        for j in range(t_off[q], t_off[q + 1]):
            t = t_items[j]
            ranks[j] = len(live) - np.searchsorted(live, keys[t], side='right') if keep[t] else -1
    return ranks


def rank_lds_bytes(k, layers, QW, pshift, top_k=None):
    """The LDS of a workgroup of the tile kernels at (QW, pshift) (include/ultrare_nmf_rank.h): the scorer's bytes plus the
    selection state (top_k given) or the counting state."""
    S = Shape(k, layers)
    L = S.layers
    w = sum(L[j] * (L[j + 1] + 1) + L[j + 1] for j in range(S.m)) + k + L[-1] + 1
    wa = max(L[1], L[3] if S.m >= 4 else 0) if S.m >= 2 else 0
    wb = L[2] if S.m >= 3 else 0
    tile = -(-4 * (w + 65 * S.e + 4 * QW * (k + L[1] + (wa + wb) * (64 >> pshift))) // 16) * 16
    return tile + (4 * QW * (12 * (top_k + 64) + 272) if top_k is not None else 49152 + 48 * QW)


def rank_plan(k, layers, top_k=None):
    """-> (QW, pshift) the entries run the stack at: the first of the header's list that fits RANK_LDS_BYTES, or None."""
    m = len(layers) - 1
    for QW, p in ((4, 0), (2, 0), (1, 0), (1, 1), (1, 2), (1, 3)):
        if rank_lds_bytes(k, layers, QW, p, top_k) <= RANK_LDS_BYTES:
            return QW, p
        if m == 1:
            break
    return None
