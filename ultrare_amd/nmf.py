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
