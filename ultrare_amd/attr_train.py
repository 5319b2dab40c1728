"""In-training attribute unlearning, stated in numpy (csrc/attr_train.hip, include/ultrare_attr_train.h, engine.GcnJob(attr=...);
DESIGN 4.29).  Nothing here touches the device.

The reference's training loop (baseTrain, utils.py:46-111) has three branches: var='nor' is the plain loss; var='d2d' adds, at every
optimizer step, eta * mmd_loss(U[user1], U[user2]); var='u2u' adds eta * trace(U^T Lap U) of the complete bipartite graph
user1 - user2.  user1 / user2 are the batch's distinct users (user.unique(), then torch.isin) of attribute group 1 / group 2.  Its own
branch cannot run as written (it reads model.user_mat_mf, rbk materialises m x m x d, buildLap densifies n_user x n_user per batch), so
this is opt-in and no parity claim, as attribute unlearning itself (attr_unlearn.py).

  selection   batch_groups_ref: the users with at least one triple in the batch that are in id1, ascending, then those in id2.
  validity    step_valid: the term of a step is applied when both groups are present and -- for 'd2d' -- the bandwidth (fix_sigma
              counts as it) is positive and finite.  Otherwise the step's term is SKIPPED: value 0, no gradient, where the reference
              would produce NaN (a mean over an empty block, 0 / 0).
  training    train_ref: lightgcn.train_ref (or bpr.train_ref) with one addition per step.  After the loss gradient (G_u, G_i) of the
              final embeddings (U*, V*) and before the backward propagations: G_u[rows[i]] += eta g[i], g the gradient of
              attr_unlearn.mmd_ref / u2u_ref on U*[rows]; the bandwidth is recomputed from the step's rows, no gradient through it.
              With layers = 0, U* is the parameter table (the reference's reading); with layers > 0 the final embedding (the
              reference: "to be modified when using LightGCN").
"""
import numpy as np

from . import lightgcn
from .attr_unlearn import MAX_D, _real, bandwidth_ref, check_groups, check_mmd_args, check_var, mmd_ref, u2u_ref

DIS_TYPES = ('nor', 'd2d', 'u2u')


def check_eta(eta):
    return _real('eta', eta)


def check_k(k):
    """ValueError unless the embedding width fits the attribute kernels."""
    if not 1 <= int(k) <= MAX_D:
        raise ValueError(f'in-training attribute unlearning needs an embedding width k in 1 .. {MAX_D}, not k = {k}')
    return int(k)


def _file_users(graph_or_pair):
    if isinstance(graph_or_pair, lightgcn.Graph):
        g = graph_or_pair
        uid = np.empty(g.N, dtype=np.int64)
        uid[g.pos] = g.row_u
        return uid
    return np.asarray(graph_or_pair[0]).astype(np.int64)


def batch_groups_ref(graph_or_pair, in_batch, id1, id2):
    """graph_or_pair: a lightgcn.Graph or (uid, iid) by file position; in_batch: bool [N] by file position.  -> (rows int32, n1, n2):
    the users with at least one triple in the batch that are in id1, in ascending id, then those in id2, in ascending id -- the order
    unique() + isin give."""
    uid = _file_users(graph_or_pair)
    in_batch = np.asarray(in_batch, dtype=bool)
    if in_batch.shape != uid.shape:
        raise ValueError(f'in_batch has shape {in_batch.shape}, the triples {uid.shape}')
    users = np.unique(uid[in_batch])
    u1 = users[np.isin(users, np.asarray(id1, dtype=np.int64))]
    u2 = users[np.isin(users, np.asarray(id2, dtype=np.int64))]
    return np.concatenate([u1, u2]).astype(np.int32), len(u1), len(u2)


def step_valid(n1, n2, var, bandwidth=None):
    """Whether a step's term is applied: both groups present and, for 'd2d', a positive finite bandwidth."""
    check_var(var)
    if n1 < 1 or n2 < 1:
        return False
    if var == 'd2d':
        return bool(bandwidth is not None and np.isfinite(bandwidth) and bandwidth > 0)
    return True


def step_term_ref(Ustar, rows, n1, n2, var, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """(valid, value, grad float64 [n1 + n2, d] or None) of one step's term on the rows `rows` of U* (float64 arithmetic on the given
    values)."""
    if n1 < 1 or n2 < 1:
        return False, 0.0, None
    if var == 'u2u':
        value, grad = u2u_ref(Ustar, rows, n1)[:2]
        return True, value, grad
    bw = fix_sigma if fix_sigma is not None else bandwidth_ref(np.asarray(Ustar)[np.asarray(rows, dtype=np.int64)].astype(np.float64))
    if not step_valid(n1, n2, var, bw):
        return False, 0.0, None
    value, grad = mmd_ref(Ustar, rows, n1, kernel_mul, kernel_num, fix_sigma)[:2]
    return True, value, grad


def check_train_args(n_user, k, id1, id2, var, eta=1.0, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """The argument checks of a training job with the term -> (id1 int64, id2 int64, eta, kernel_mul, kernel_num, fix_sigma)."""
    check_var(var)
    check_k(k)
    rows, n1, _ = check_groups(id1, id2, n_user)
    kernel_mul, kernel_num, fix_sigma = check_mmd_args(kernel_mul, kernel_num, fix_sigma)
    return rows[:n1].astype(np.int64), rows[n1:].astype(np.int64), check_eta(eta), kernel_mul, kernel_num, fix_sigma


def train_ref(uid, iid, rating, P0, Q0, orders, batch, lr_host, lam, mu, layers, id1, id2, var, eta=1.0, kernel_mul=2.0, kernel_num=5,
              fix_sigma=None, dtype=np.float64, loss='mse', key=0, eta_of_step=None):
    """lightgcn.train_ref (loss='mse') or bpr.train_ref (loss='bpr', negatives under `key`; rating is not read) with the term added at
    every step.  -> what they return, plus dis [epochs] (the sum of the applied steps' values), skipped [epochs] (steps whose term was
    skipped), counts [epochs, steps, 2] and loss = sqrt((sse + eta dis) / N) as utils.py:108 reports it (BPR: (loss_sum + eta dis) / N).
    dtype=np.float32 is a float32 CPU execution used as a yardstick, no bit contract: the MMD kernels are held to bounds, not bits.
    eta_of_step (tests only): callable (epoch, step) -> the eta of that step."""
    from . import bpr
    if loss not in ('mse', 'bpr'):
        raise ValueError(f"loss {loss!r}: 'mse' or 'bpr'")
    T = dtype
    layers = lightgcn.check_layers(layers)
    P, Q = np.array(P0, dtype=T), np.array(Q0, dtype=T)
    id1, id2, eta, kernel_mul, kernel_num, fix_sigma = check_train_args(len(P), P.shape[1], id1, id2, var, eta, kernel_mul, kernel_num, fix_sigma)
    g = lightgcn.Graph(uid, iid, len(P), len(Q))
    if loss == 'bpr':
        off_d, col_d = bpr.distinct_csr(g)
        bpr.check_negatives(g, off_d)
    lr_host = np.asarray(lr_host, dtype=np.float32)
    mP, mQ = np.zeros_like(P), np.zeros_like(Q)
    N, E = g.N, len(orders)
    steps = (N + batch - 1) // batch
    out = dict(U=[], V=[], P=[], Q=[])
    base, dis, skipped, first = np.zeros(E), np.zeros(E), np.zeros(E, dtype=np.int64), True
    counts = np.zeros((E, steps, 2), dtype=np.int64)
    for e in range(E):
        if loss == 'bpr':
            neg = bpr.sample_ref(g, off_d, col_d, key, e)
            index = bpr.neg_index_ref(neg, g.row_u, g.n_item)
        for t in range(steps):
            idx = np.asarray(orders[e][t * batch:(t + 1) * batch], dtype=np.int64)
            U, V = lightgcn.forward_ref(g, P, Q, layers, dtype=T)
            if loss == 'bpr':
                Gu, Gi, value = bpr.loss_grad_ref(g, index, U, V, neg, idx, dtype=T)[:3]
            else:
                Gu, Gi, value = lightgcn.loss_grad_ref(g, U, V, rating, idx, dtype=T)[:3]
            base[e] += value
            in_batch = np.zeros(N, dtype=bool)
            in_batch[idx] = True
            rows, n1, n2 = batch_groups_ref(g, in_batch, id1, id2)
            counts[e, t] = n1, n2
            valid, term, grad = step_term_ref(U, rows, n1, n2, var, kernel_mul, kernel_num, fix_sigma)
            if valid:
                step_eta = eta if eta_of_step is None else float(eta_of_step(e, t))
                dis[e] += term
                Gu = np.array(Gu, dtype=T)
                Gu[rows.astype(np.int64)] = Gu[rows.astype(np.int64)] + T(step_eta) * grad.astype(T)
            else:
                skipped[e] += 1
            gP, gQ = lightgcn.backward_ref(g, Gu, Gi, layers, dtype=T)
            P, mP = lightgcn.sgd_update_ref(P, mP, gP, lr_host[e], lam, mu, first, dtype=T)
            Q, mQ = lightgcn.sgd_update_ref(Q, mQ, gQ, lr_host[e], lam, mu, first, dtype=T)
            first = False
        U, V = lightgcn.forward_ref(g, P, Q, layers, dtype=T)
        for name, a in (('U', U), ('V', V), ('P', P), ('Q', Q)):
            out[name].append(a.copy())
    out = {k: np.stack(v) for k, v in out.items()}
    out['dis'], out['skipped'], out['counts'] = dis, skipped, counts
    if loss == 'mse':
        out['sse'] = base
        out['loss'] = np.sqrt(np.maximum(base + eta * dis, 0.0) / max(N, 1))
    else:
        out['loss_sum'] = base
        out['loss'] = (base + eta * dis) / max(N, 1)
    return out
