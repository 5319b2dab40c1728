"""BPR training with device-side negative sampling, stated in numpy: the contract of csrc/bpr.hip (include/ultrare_bpr.h) and of
engine.GcnJob(loss='bpr').

A batch is the set of training triples the MSE job trains on (the file positions orders[e][t B : (t + 1) B]); every triple is a
positive, whatever its rating (no rating threshold).  Each CSR entry q = (u, i) gets ONE negative j per epoch, uniform over the
items user u has no triple for in this shard's graph; the loss of a batch is sum_q -log sigmoid(x_q), x_q = s(u, i) - s(u, j), over
the final tables (U*, V*) of lightgcn.forward_ref.  Propagation, the backward and the SGD update are lightgcn's, unchanged; with
layers = 0 this is plain BPR-MF.

sample_ref, neg_index_ref and -- on GIVEN x and w arrays -- walks_ref are BIT contracts; of coef_ref the scores and x are (at
float32), w is not (two exp implementations need not agree): it is held to 1 float32 ulp of the float64 value.  At dtype float64
the same lines are the float64 restatement.  train_ref is whole training at either dtype.
"""
import numpy as np

from .lightgcn import Graph, _walk, backward_ref, check_layers, fold_256, forward_ref, score_ref, sgd_update_ref

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
PLANTS = ('no_neg_item_grad', 'epoch_blind', 'any_item', 'sign')


def mix(z):
    """The splitmix64 finaliser on uint64 arrays (arithmetic wraps)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def stream_key(seed, shard):
    """The key of a shard's negative draws: mix(seed + GOLDEN * (shard + 1)) in wrapping uint64 arithmetic -> Python int in
    0 .. 2^64 - 1.  It does not touch torch's generator; a retrained shard keeps its key and draws from its post-deletion graph."""
    s = (int(seed) + 0x9E3779B97F4A7C15 * (int(shard) + 1)) & 0xFFFFFFFFFFFFFFFF
    return int(mix(np.uint64(s)))


def distinct_csr(g):
    """(off_d int64 [n_user + 1], col_d int32) -- every user's DISTINCT items, ascending: the graph's CSR when no pair repeats."""
    keep = np.ones(g.N, dtype=bool)
    if g.N > 1:
        keep[1:] = (g.row_u[1:] != g.row_u[:-1]) | (g.col[1:] != g.col[:-1])
    deg = np.bincount(g.row_u[keep], minlength=g.n_user)
    off_d = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return off_d, np.ascontiguousarray(g.col[keep], dtype=np.int32)


def check_negatives(g, off_d):
    """ValueError, by name, for a user with triples and no item left to draw (m_u == 0)."""
    m = g.n_item - np.diff(off_d)
    full = np.flatnonzero((np.diff(g.off_u) > 0) & (m <= 0))
    if len(full):
        raise ValueError(f'user {int(full[0])} has a triple for every one of the {g.n_item} items: BPR has no negative to draw for it')


def select_ref(c, n_item, r):
    """The r-th item (r = 0 .. n_item - len(c) - 1) that is not in c (distinct items, ascending): r + #{t : c[t] - t <= r}; the
    keys c[t] - t do not decrease, so the count is one binary search."""
    c = np.asarray(c, dtype=np.int64)
    return int(r) + int(np.searchsorted(c - np.arange(len(c)), int(r), side='right'))


def sample_ref(g, off_d, col_d, key, epoch, plant=None):
    """neg int32 [nnz], in CSR order: the negative of every entry in `epoch`.
    z = mix(key + GOLDEN * (1 + (epoch << 32) + p)), p the entry's FILE position; r = ((z >> 32) * m_u) >> 32;
    neg = r + #{t : c_u[t] - t <= r}.  plant (tests only): 'epoch_blind' leaves the epoch out, 'any_item' draws from all items."""
    u = g.row_u.astype(np.int64)
    e = 0 if plant == 'epoch_blind' else int(epoch)
    ctr = np.uint64(1) + (np.uint64(e) << np.uint64(32)) + g.pos.astype(np.uint64)
    with np.errstate(over='ignore'):
        z = mix(np.uint64(int(key) & 0xFFFFFFFFFFFFFFFF) + GOLDEN * ctr)
    if plant == 'any_item':
        return ((z >> np.uint64(32)) * np.uint64(g.n_item) >> np.uint64(32)).astype(np.int32)
    m = np.maximum(g.n_item - np.diff(off_d), 0)[u].astype(np.uint64)
    r = ((z >> np.uint64(32)) * m >> np.uint64(32)).astype(np.int64)
    b = off_d[u]
    lo, hi = b.copy(), off_d[u + 1].copy()
    while (lo < hi).any():                                  # the count by binary search, all entries side by side
        live = lo < hi
        mid = np.minimum((lo + hi) // 2, len(col_d) - 1)
        le = live & (col_d[mid].astype(np.int64) - (mid - b) <= r)
        lo = np.where(le, mid + 1, lo)
        hi = np.where(live & ~le, mid, hi)
    return np.minimum(r + (lo - b), g.n_item - 1).astype(np.int32)


def neg_index_ref(neg, row_u, n_item):
    """The CSR entries grouped by negative item: off_n int64 [n_item + 1], map_n int32 [nnz] (CSR position, ascending inside an item),
    usr_n = row_u[map_n]."""
    neg = np.asarray(neg, dtype=np.int64)
    map_n = np.argsort(neg, kind='stable').astype(np.int32)
    off_n = np.concatenate([[0], np.cumsum(np.bincount(neg, minlength=n_item))]).astype(np.int64)
    return off_n, map_n, np.asarray(row_u, dtype=np.int32)[map_n]


def in_batch_csr(g, batch_idx):
    """bool [nnz]: the CSR entries whose file position is in batch_idx."""
    in_file = np.zeros(g.N, dtype=bool)
    in_file[np.asarray(batch_idx, dtype=np.int64)] = True
    return in_file[g.pos]


def coef_w(x):
    """w = float32(-1 / (1 + exp((double)x))) of float32 x; in float64, the same expression unrounded."""
    with np.errstate(over='ignore'):
        w = -1.0 / (1.0 + np.exp(np.asarray(x, dtype=np.float64)))
    return w.astype(np.asarray(x).dtype)


def loss_terms(x):
    """-log sigmoid(x) = max(-x, 0) + log1p(exp(-|x|)), float64."""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def coef_ref(g, Ustar, Vstar, neg, in_csr, dtype=np.float32, plant=None):
    """-> (w, x, s_pos, s_neg) [nnz] in CSR order, +0.0 outside the batch: s_pos = s(u, i), s_neg = s(u, neg) (score_ref's bytes at
    float32, a plain dot at float64), x = fl(s_pos - s_neg), w = coef_w(x)."""
    T = dtype
    Ustar, Vstar = np.asarray(Ustar, dtype=T), np.asarray(Vstar, dtype=T)
    u, i, j = g.row_u.astype(np.int64), g.col.astype(np.int64), np.asarray(neg, dtype=np.int64)
    if T == np.float32:
        sp, sn = score_ref(Ustar, Vstar, u, i), score_ref(Ustar, Vstar, u, j)
    else:
        sp, sn = (Ustar[u] * Vstar[i]).sum(axis=1, dtype=T), (Ustar[u] * Vstar[j]).sum(axis=1, dtype=T)
    x = sp - sn
    w = coef_w(x)
    if plant == 'sign':
        w = -w
    zero = T(0)
    return tuple(np.where(in_csr, a, zero).astype(T) for a in (w, x, sp, sn))


def walks_ref(g, index, Ustar, Vstar, neg, w, x, in_csr, dtype=np.float32, plant=None):
    """The two gradient walks on GIVEN w and x (CSR order) -> (G_u, G_i, row_loss float64 [n_user]).
    G_u[u]: the chain from +0 over the user's CSR entries in the batch, ascending, of fl(w_q * fl(V*[i] - V*[neg_q])).
    G_i[r]: ONE chain from +0: the item's CSC entries in the batch, ascending CSC position, terms fl(w_q * U*[u]); then, in the same
    accumulator, the item's entries of the negative index in the batch, ascending q, terms fl(fl(-w_q) * U*[u]).
    row_loss[u]: the float64 chain of loss_terms(x_q) over G_u's entries.  index = (off_n, map_n, usr_n)."""
    T = dtype
    Ustar, Vstar = np.asarray(Ustar, dtype=T), np.asarray(Vstar, dtype=T)
    w, x = np.asarray(w, dtype=T), np.asarray(x, dtype=T)
    off_n, map_n, usr_n = index
    u, i, j = g.row_u.astype(np.int64), g.col.astype(np.int64), np.asarray(neg, dtype=np.int64)
    term = loss_terms(x)
    Gu, Gi = np.zeros_like(Ustar), np.zeros_like(Vstar)
    row_loss = np.zeros(g.n_user, dtype=np.float64)
    for rows, at in _walk(g.off_u, g.n_user):
        m = in_csr[at]
        rows, at = rows[m], at[m]
        Gu[rows] = Gu[rows] + w[at][:, None] * (Vstar[i[at]] - Vstar[j[at]])
        row_loss[rows] = row_loss[rows] + term[at]
    for rows, at in _walk(g.off_i, g.n_item):
        k = g.to_csr[at]
        m = in_csr[k]
        rows, k = rows[m], k[m]
        Gi[rows] = Gi[rows] + w[k][:, None] * Ustar[u[k]]
    if plant != 'no_neg_item_grad':
        for rows, at in _walk(off_n, g.n_item):
            q = map_n[at]
            m = in_csr[q]
            rows, q, at = rows[m], q[m], at[m]
            Gi[rows] = Gi[rows] + (-w[q])[:, None] * Ustar[usr_n[at].astype(np.int64)]
    return Gu, Gi, row_loss


def loss_grad_ref(g, index, Ustar, Vstar, neg, batch_idx, dtype=np.float32, plant=None):
    """The batch = the triples at the file positions batch_idx, neg and index those of the epoch.
    -> (G_u, G_i, loss = fold_256(row_loss), w, x): the contract's own w on its own x."""
    in_csr = in_batch_csr(g, batch_idx)
    w, x, _, _ = coef_ref(g, Ustar, Vstar, neg, in_csr, dtype=dtype, plant=plant)
    Gu, Gi, row_loss = walks_ref(g, index, Ustar, Vstar, neg, w, x, in_csr, dtype=dtype, plant=plant)
    return Gu, Gi, fold_256(row_loss), w, x


def train_ref(uid, iid, P0, Q0, orders, batch, lr_host, lam, mu, layers, key, dtype=np.float64, plant=None):
    """Whole BPR training of one shard: per epoch the negatives and their index, per step forward, loss gradient, backward, update.
    -> what lightgcn.train_ref returns, with loss_sum [epochs] (the summed batch losses) in place of sse and loss = loss_sum / N.
    dtype=np.float32 is the contract of engine.GcnJob(loss='bpr') (bit for bit but for w).  plant (tests only): one of PLANTS."""
    assert plant is None or plant in PLANTS
    T = dtype
    layers = check_layers(layers)
    g = Graph(uid, iid, len(P0), len(Q0))
    off_d, col_d = distinct_csr(g)
    check_negatives(g, off_d)
    lr_host = np.asarray(lr_host, dtype=np.float32)
    P, Q = np.array(P0, dtype=T), np.array(Q0, dtype=T)
    mP, mQ = np.zeros_like(P), np.zeros_like(Q)
    N, E = g.N, len(orders)
    steps = (N + batch - 1) // batch
    out = dict(U=[], V=[], P=[], Q=[], neg=[])
    loss_sum, first = np.zeros(E), True
    for e in range(E):
        neg = sample_ref(g, off_d, col_d, key, e, plant=plant)
        index = neg_index_ref(neg, g.row_u, g.n_item)
        for t in range(steps):
            U, V = forward_ref(g, P, Q, layers, dtype=T)
            Gu, Gi, loss, _, _ = loss_grad_ref(g, index, U, V, neg, orders[e][t * batch:(t + 1) * batch], dtype=T, plant=plant)
            loss_sum[e] += loss
            gP, gQ = backward_ref(g, Gu, Gi, layers, dtype=T)
            P, mP = sgd_update_ref(P, mP, gP, lr_host[e], lam, mu, first, dtype=T)
            Q, mQ = sgd_update_ref(Q, mQ, gQ, lr_host[e], lam, mu, first, dtype=T)
            first = False
        U, V = forward_ref(g, P, Q, layers, dtype=T)
        for name, a in (('U', U), ('V', V), ('P', P), ('Q', Q), ('neg', neg)):
            out[name].append(a.copy())
    out = {k: np.stack(v) for k, v in out.items()}
    out['loss_sum'], out['loss'] = loss_sum, loss_sum / max(N, 1)
    return out
