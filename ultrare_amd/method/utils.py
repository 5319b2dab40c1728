"""Model, evaluation and OT grouping with the reference's names (method/utils.py of
the reference), backed by the HIP engine.

  seed_all     utils.py:21-25
  MF           utils.py:30-43    two embedding tables; forward = row-wise dot
  NMF          (new)             NeuMF: the reference's user_mat_mf / user_mat_mlp (sisa.py:39-50) beside an MLP and a head; forward =
                                 the HIP scoring kernel of csrc/nmf.hip; refuse_nmf: what needs two dot-product tables says so
  baseTest     utils.py:115-187  ensemble mean score, RMSE, HR@10, NDCG@10 (a list of MF models or a list of NMF models)
  fit_combiner (new)             fitted weights of the shard scores in place of their mean (baseTest(..., combiner=))
  recommend    (new)             top-k items over the whole catalogue from the same ensemble mean
  rank_eval    (new)             full-ranking HR@K / Recall@K / NDCG@K / MRR of the test pairs (rank_metrics: the reduction)
  fold_in      (new)             rows for new users against frozen item tables (one batched ridge solve on the device)
  als_sweeps   (new)             alternating least squares from a model's tables by the same solve
  trainer_l2   (new)             the ridge strength at which fold_in gives the trainer's own fixed point
  wmf_sweeps   (new)             implicit-feedback ALS (weighted MF): als_sweeps with a confidence per entry and the Gram trick
  wmf_fold_in  (new)             fold_in under that objective: the user half alone, against frozen items
  computeNDCG / computeDCG  utils.py:190-210
  ot_cluster   utils.py:628-656  OT balanced clustering (exact EMD; solver='sinkhorn': entropic OT on the device)
  kmeans       utils.py:354-418  (balanced) k-means, a comparison clusterer
  findNeighbor utils.py:422-455  the k-nearest-neighbour user graph
  lpa          utils.py:458-519  (balanced) label propagation, a comparison clusterer
  kmedoids     utils.py:546-611  (balanced) k-medoids, a comparison clusterer
  rbk / mmd_loss  utils.py:223-267  the multi-bandwidth Gaussian kernel matrix and the MMD loss of two groups (streamed)
  attribute_unlearn (new)        post-training attribute unlearning: a short fine-tune of the groups' user rows on the
                                 MMD ('d2d') or Laplacian ('u2u', utils.py:75-78 with buildLap) loss
  saveObject / loadObject / timefn  utils.py:319-326, 616-626

Training does not go through a `baseTrain(dataloader, model, loss_fn, opt, ...)` loop:
the per-batch forward / backward / SGD step of utils.py:58-91 is one fused kernel
launch per step, driven by engine.TrainJob from Scratch.train.
"""
import ctypes
import os
import pickle
import time
from functools import wraps

import numpy as np
import torch
from torch import nn

from .. import _native as nv
from .. import engine
from ..combine import Combiner, check_fit_args, first_group_map, mean_weights, newton_fit
from ..read import as_loader
from ..rng import seed_all  # noqa: F401  (re-exported under the reference's name)
from ..sparse_group import Compressed, check_cluster_args, dense_rows

STD = 1
OT_WARM_ITERS = 400      # dual-ascent steps that warm-start the exact OT solver (ure_ot_potentials) at large n


def ot_warm_iters(n):
    """Fewer steps for small problems: the solver finishes a rough start of a few thousand points in a millisecond, while
    every ascent step is two launches (n = 6,040, ten rounds, the ascent starting from the round before's potentials: at least 60 / 40 / 30 / 20 / 10 steps
    11.6 / 10.0 / 9.8 / 8.9 / 8.6 ms at k = 5, 19.3-20.4 / 18.6 / 18.3 / 18.3 / 18.7 at k = 16; the same labels)."""
    return int(min(OT_WARM_ITERS, max(20, n // 400)))


class MF(nn.Module):
    """utils.py:30-43.  Constructed on the CPU with exactly the reference's four normal
    fills (so the global torch stream advances identically); `.to('cuda')` moves the
    tables to HBM.  forward() scores (uid, iid) pairs with the HIP scoring kernel."""

    def __init__(self, n_user, n_item, k=16):
        super().__init__()
        self.k = k
        self.user_mat = nn.Embedding(n_user, k)
        self.item_mat = nn.Embedding(n_item, k)
        self.init_weight()

    def init_weight(self):
        nn.init.normal_(self.user_mat.weight, std=STD)
        nn.init.normal_(self.item_mat.weight, std=STD)

    @classmethod
    def from_tables(cls, U, V):
        """Wrap trained device tables without drawing from any generator."""
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        m.k = U.shape[1]
        m.user_mat = nn.Embedding(U.shape[0], U.shape[1], _weight=U)
        m.item_mat = nn.Embedding(V.shape[0], V.shape[1], _weight=V)
        m.requires_grad_(False)
        return m

    def forward(self, uid, iid):
        U, V, d = padded_tables(self)
        uid = uid.to(device=U.device, dtype=torch.int32).contiguous()
        iid = iid.to(device=U.device, dtype=torch.int32).contiguous()
        pred = torch.empty(uid.numel(), dtype=torch.float32, device=U.device)
        import ctypes
        Up = (ctypes.c_void_p * 1)(U.data_ptr())
        Vp = (ctypes.c_void_p * 1)(V.data_ptr())
        nv.check(nv.lib().ure_score(Up, Vp, 1, 1, 1, 1, nv.ptr(uid), nv.ptr(iid), None, uid.numel(), d,
                                    nv.ptr(pred), None, nv.stream_handle()), 'ure_score')
        return pred


class NMF(nn.Module):
    """NeuMF as rating regression (ultrare_amd/nmf.py): the reference's attribute names user_mat_mf, item_mat_mf, user_mat_mlp,
    item_mat_mlp (method/sisa.py:39-50), the MLP fc[j] = nn.Linear(L_j, L_(j+1)) and the head nn.Linear(k + Lm, 1).
    Constructed on the CPU after seed_all, like MF.  The draws from torch's generator, in order: the four embeddings' normal_(std=0.01)
    fills in the order above (they are made without nn.Embedding's own N(0, 1) fill: nothing is drawn and thrown away), then torch's
    default fill of every nn.Linear in layer order, the head last.
    forward() scores (uid, iid) pairs with the HIP scoring kernel (no sigmoid: the loss is MSELoss(sum) on rating / 5)."""

    EMB_STD = 0.01

    def __init__(self, n_user, n_item, k, layers):
        from ..nmf import check_layers
        super().__init__()
        self.k, self.layers = check_layers(k, layers)
        e = self.layers[0] // 2
        def emb(rows, width):                               # (skip_init: no N(0, 1) fill first)
            table = nn.utils.skip_init(nn.Embedding, rows, width)
            nn.init.normal_(table.weight, std=self.EMB_STD)
            return table
        self.user_mat_mf = emb(n_user, self.k)
        self.item_mat_mf = emb(n_item, self.k)
        self.user_mat_mlp = emb(n_user, e)
        self.item_mat_mlp = emb(n_item, e)
        self.fc = nn.ModuleList([nn.Linear(a, b) for a, b in zip(self.layers[:-1], self.layers[1:])])
        self.head = nn.Linear(self.k + self.layers[-1], 1)

    @classmethod
    def from_tables(cls, U, V, dense, k, layers):
        """Wrap trained device tensors (nmf.py's U [n_user, k + e], V [n_item, k + e] and dense vector) without drawing from any
        generator: every parameter is a copy-free view or a contiguous copy of them."""
        from ..nmf import Shape
        S = Shape(k, layers)
        m = cls.__new__(cls)
        nn.Module.__init__(m)
        m.k, m.layers = S.k, S.layers
        emb = lambda t: nn.Embedding(t.shape[0], t.shape[1], _weight=t.contiguous())
        m.user_mat_mf, m.item_mat_mf = emb(U[:, :S.k]), emb(V[:, :S.k])
        m.user_mat_mlp, m.item_mat_mlp = emb(U[:, S.k:]), emb(V[:, S.k:])
        W, b, h, c = S.unpack(dense)

        def linear(weight, bias):                             # (skip_init: no default fill, so no draw)
            lin = nn.utils.skip_init(nn.Linear, weight.shape[1], weight.shape[0])
            lin.weight, lin.bias = nn.Parameter(weight.clone()), nn.Parameter(bias.clone())
            return lin
        m.fc = nn.ModuleList([linear(Wj, bj) for Wj, bj in zip(W, b)])
        m.head = linear(h.reshape(1, -1), c.reshape(1))
        m.requires_grad_(False)
        return m

    def tables(self):
        """(U [n_user, k + e], V [n_item, k + e], dense) float32 on the parameters' device, as nmf.py and the kernels hold a model.
        Packed once and kept until a parameter is replaced, moved or written in place (its address or version changes): forward and
        baseTest do not concatenate the tables again per call.  Read-only for the caller."""
        from ..nmf import Shape
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        kept = getattr(self, '_packed', None)
        if kept is not None and kept[0] == key:
            return kept[1]
        S = Shape(self.k, self.layers)
        w = lambda p: p.detach().float()
        U = torch.cat([w(self.user_mat_mf.weight), w(self.user_mat_mlp.weight)], dim=1).contiguous()
        V = torch.cat([w(self.item_mat_mf.weight), w(self.item_mat_mlp.weight)], dim=1).contiguous()
        parts = [p.reshape(-1) for lin in self.fc for p in (w(lin.weight), w(lin.bias))] + [w(self.head.weight).reshape(-1), w(self.head.bias).reshape(-1)]
        dense = torch.cat(parts + [U.new_zeros(S.n_dense - S.n_real)])
        self._packed = (key, (U, V, dense))
        return U, V, dense

    def forward(self, uid, iid):
        U, V, dense = self.tables()
        if not U.is_cuda:
            raise nv.NativeError('model tables are not on the HIP device (call model.to("cuda")): no CPU fallback')
        return engine.nmf_score(U, V, dense, self.k, self.layers, uid.to(device=U.device, dtype=torch.int32).contiguous(),
                                iid.to(device=U.device, dtype=torch.int32).contiguous())


def refuse_nmf(models, who):
    """ValueError when `who` -- something defined for a model scored as the dot product of two tables -- is handed the 'nmf' backbone."""
    for m in (models if isinstance(models, (list, tuple)) else [models]):
        if isinstance(m, NMF):
            raise ValueError(f"{who} needs a model scored as the dot product of two tables ('mf' or 'lightgcn'): the 'nmf' backbone scores "
                             'a pair through an MLP and has no such tables')


def padded_tables(model):
    """(U, V, d) as contiguous device tensors whose width is the kernels' padded d."""
    refuse_nmf(model, 'padded_tables')
    U, V = model.user_mat.weight.detach(), model.item_mat.weight.detach()
    if not U.is_cuda:
        raise nv.NativeError('model tables are not on the HIP device (call model.to("cuda")): no CPU fallback')
    d = engine.pad_dim(U.shape[1])

    def fix(t):
        if t.shape[1] == d and t.is_contiguous() and t.dtype == torch.float32:
            return t
        out = torch.zeros(t.shape[0], d, dtype=torch.float32, device=t.device)
        out[:, :t.shape[1]] = t
        return out
    return fix(U), fix(V), d


def baseTest(dataloader, models, loss_fn=None, device=None, verbose=0, top_k=10, combiner=None):
    """utils.py:115-187: (rmse, ndcg, hr) of the mean-ensemble of `models` on a test
    loader.  loss_fn / device are accepted for signature compatibility.  combiner (fit_combiner's result, optional): the
    pairs are scored with its fitted weights instead of the mean; without one nothing changes."""
    n_nmf = sum(isinstance(m, NMF) for m in models)
    if n_nmf and n_nmf != len(models):
        raise ValueError(f"baseTest takes models of one backbone: {n_nmf} of {len(models)} are 'nmf'")
    if n_nmf and combiner is not None:
        refuse_nmf(models, 'baseTest(combiner=)')
    ev = as_loader(dataloader).eval_set()
    if n_nmf:                                                # one scoring call per model (engine.EvalSet.evaluate_nmf); the rest is shared
        rmse, ndcg, hr = ev.evaluate_nmf([m.tables() + (m.k, m.layers) for m in models], top_k=top_k)
        if verbose == 2:
            print(f'Test - RMSE: {rmse:>.4f}, NDCG: {ndcg:>.3f}, HR: {hr:>.3f}')
        return rmse, ndcg, hr
    tabs = [padded_tables(m) for m in models]
    d = tabs[0][2]
    if combiner is None:
        rmse, ndcg, hr = ev.evaluate([(U, V) for U, V, _ in tabs], d, top_k=top_k)
    else:
        rmse, ndcg, hr = ev.evaluate([(U, V) for U, V, _ in tabs], d, top_k=top_k, combiner=combiner)
    if verbose == 2:
        print(f'Test - RMSE: {rmse:>.4f}, NDCG: {ndcg:>.3f}, HR: {hr:>.3f}')
    return rmse, ndcg, hr


def fit_combiner(models, train_data, link='linear', l2=0.0, groups=None, max_iter=25, tol=1e-10):
    """Fit the weights that combine the scores of `models` (the learned third stage of SISA) on training pairs.
    For a pair, z = b + sum_s w[s] * score_s; link='linear' predicts z and minimises the squared error, link='logistic'
    predicts sigmoid(z) and minimises the cross-entropy against the rating / 5; plus (l2 / 2) |w - 1/S|^2, which pulls towards
    the mean ensemble.  train_data: one loader or a list of loaders (as Sisa's train_dlist).  groups (index lists, as
    Group.grouping returns): one independent fit per group -- with a list of loaders, loader g holds group g's pairs (their
    numbers must agree); with one loader, its pairs are split by the first group that lists the user and the pairs of users in
    no group are left out.  Without groups: one fit over all pairs.  A group without pairs keeps the mean's weights.
    Each Newton pass is one launch over pairs that went to the device once (engine.combine_stats); the solve of at most 33
    unknowns runs on the host.  Returns a Combiner for baseTest(..., combiner=); ValueError for bad settings (before any device
    work) and for a singular system (naming l2)."""
    check_fit_args(link, l2, max_iter, tol)
    S = len(models)
    refuse_nmf(models, 'fit_combiner')
    if not 1 <= S <= nv.MAX_MODELS_PER_CALL:
        raise ValueError(f'fit_combiner takes 1 .. {nv.MAX_MODELS_PER_CALL} models, not {S}')
    many = isinstance(train_data, (list, tuple))
    loaders = [as_loader(l) for l in (train_data if many else [train_data])]
    if not loaders:
        raise ValueError('fit_combiner needs training data')
    if groups is not None and many and len(groups) != len(loaders):
        raise ValueError(f'{len(groups)} groups for {len(loaders)} loaders: with a list of loaders, loader g holds the pairs of group g')
    triples = [l.dataset.triples() for l in loaders]
    if groups is not None and not many:
        uid, iid, r = triples[0]
        n_ids = max(int(uid.max()) + 1 if len(uid) else 0, 1 + max((int(max(g)) for g in groups if len(g)), default=0))
        of = first_group_map(groups, n_ids)[uid]
        triples = [(uid[of == g], iid[of == g], r[of == g]) for g in range(len(groups))]
    tabs = [padded_tables(m) for m in models]
    tables, d = [(U, V) for U, V, _ in tabs], tabs[0][2]
    dev = tables[0][0].device
    sets = [engine.PairSet(*t, device=dev) for t in triples]           # on the device once per fit, not once per pass
    per_set = lambda theta: [engine.combine_stats(tables, d, ps, link, theta) for ps in sets if ps.n]
    if groups is None:
        if not any(ps.n for ps in sets):
            raise ValueError('fit_combiner needs at least one training pair')
        # the loaders' stats vectors added in index order: one solve, no second pass over the data
        fits = [newton_fit(lambda theta: np.sum(per_set(theta), axis=0) if len(sets) > 1 else per_set(theta)[0], S, link, l2, max_iter, tol)]
    else:
        empty = {'theta': mean_weights(S), 'n': 0, 'iters': 0, 'loss_before': 0.0, 'loss_after': 0.0, 'grad_norm': 0.0}
        fits = [newton_fit(lambda theta, ps=ps: engine.combine_stats(tables, d, ps, link, theta), S, link, l2, max_iter, tol) if ps.n else empty
                for ps in sets]
    return Combiner(np.stack([f['theta'] for f in fits]), link, None if groups is None else [list(g) for g in groups],
                    **{key: [f[key] for f in fits] for key in ('n', 'iters', 'loss_before', 'loss_after', 'grad_norm')})


def trainer_l2(n_rows, batch, lam):
    """The ridge strength l2 at which a ridge row (fold_in, als_sweeps) is the fixed point of the trainer for that row
    under a frozen opposite table: lam * ceil(n_rows / batch) / 2, with n_rows the shard's ratings and batch its batch size.
    Derivation.  The loss of a step is the SUM of the squared errors of its batch, so a rating j of row x with opposite row
    v_j contributes the gradient 2 e_j v_j, e_j = x . v_j - r_j, once per epoch.  Weight decay adds lam * x to the gradient
    of EVERY row at every optimizer step, ceil(n_rows / batch) times per epoch.  Summed over an epoch the drift of x is
    2 sum_j e_j v_j + lam * ceil(n_rows / batch) * x, and it vanishes where
        (sum_j v_j v_j^T + (lam * ceil(n_rows / batch) / 2) I) x = sum_j r_j v_j,
    the ridge system of strength l2 = lam * ceil(n_rows / batch) / 2.  Momentum scales every gradient by the same
    1 / (1 - mu) in the long run and does not move the fixed point; the learning rate and its decay do not enter either.
    (With several steps per epoch the trainer cycles around this point with an amplitude of the order of the learning rate;
    with one step per epoch it converges to it.)"""
    n_rows, batch = int(n_rows), int(batch)
    if n_rows < 0 or batch < 1:
        raise ValueError(f'need n_rows >= 0 and batch >= 1, not {n_rows}, {batch}')
    return float(lam) * (-(-n_rows // batch)) / 2.0


def _rating_triple(data):
    """(uid int64, iid int64, rating / 5 float32) of a loader (as baseTest accepts one) or of such a triple."""
    if isinstance(data, (tuple, list)) and len(data) == 3:
        uid, iid, r = (np.asarray(a).reshape(-1) for a in data)
    else:
        uid, iid, r = as_loader(data).dataset.triples()
    if not len(uid) == len(iid) == len(r):
        raise ValueError('uid, iid and rating differ in length')
    return uid.astype(np.int64), iid.astype(np.int64), r.astype(np.float32)


def _check_item_table(item_table, S):
    if isinstance(item_table, str):
        if item_table != 'mean':
            raise ValueError(f"item_table must be a model index or 'mean', not {item_table!r}")
    elif isinstance(item_table, bool) or not isinstance(item_table, (int, np.integer)) or not 0 <= int(item_table) < S:
        raise ValueError(f"item_table must be a model index in 0 .. {S - 1} or 'mean', not {item_table!r}")


def fold_in(models, data, l2, l2_n=0.0, item_table='mean'):
    """Rows for the users of `data` with the item tables held fixed: user u's row is the ridge solution
    (sum_j v_j v_j^T + (l2 + l2_n n_u) I)^-1 sum_j r_j v_j over u's n_u ratings, solved in float64 on the device
    (engine.ridge_rows), one workgroup per user.  data: a loader as baseTest accepts one, or a (uid, iid, rating / 5) triple.
    item_table: an int s -- against model s's item table -- or 'mean': the float64 mean of the S item tables rounded to float32
    once (the table whose scores the mean ensemble serves, up to that rounding).  trainer_l2 gives the l2 of the trainer's own
    fixed point.  Returns (users ascending int64, rows [n, k] float32 on the device).  ValueError for bad settings (before any
    device work) and for a system that is not positive definite (naming l2)."""
    from ..ridge import check_ridge_args
    l2, l2_n = check_ridge_args(l2, l2_n)
    S = len(models)
    refuse_nmf(models, 'fold_in')
    if S < 1:
        raise ValueError('fold_in needs at least one model')
    _check_item_table(item_table, S)
    uid, iid, r = _rating_triple(data)
    if len(uid) and (uid.min() < 0 or iid.min() < 0):
        raise ValueError('negative user or item id')
    users, seg = np.unique(uid, return_inverse=True)
    if isinstance(item_table, str):
        tabs = [padded_tables(m) for m in models]
        d = tabs[0][2]
        acc = tabs[0][1].double()
        for _, V, _ in tabs[1:]:
            acc = acc + V.double()
        V = (acc / S).float().contiguous()
    else:
        _, V, d = padded_tables(models[int(item_table)])
    k = int(models[0].k)
    segs = engine.SegmentSet(seg, iid, r, len(users), device=V.device)
    X = engine.ridge_rows(V, d, k, segs, l2, l2_n)
    return users.astype(np.int64), X[:, :k].contiguous()


def _ridge_objective_dev(U, V, k, pairs, reg_u, reg_v, chunk=1 << 20):
    """sum e^2 + sum_rows reg_row |x|^2 in float64 on the device (a diagnostic of als_sweeps, not a hot path)."""
    uid, iid, val = pairs
    tot = torch.zeros((), dtype=torch.float64, device=U.device)
    for a in range(0, uid.numel(), chunk):
        u, i = uid[a:a + chunk].long(), iid[a:a + chunk].long()
        e = (U[u, :k].double() * V[i, :k].double()).sum(dim=1) - val[a:a + chunk].double()
        tot = tot + (e * e).sum()
    tot = tot + (reg_u * (U[:, :k].double() ** 2).sum(dim=1)).sum() + (reg_v * (V[:, :k].double() ** 2).sum(dim=1)).sum()
    return float(tot)


def als_sweeps(model, train_data, l2, l2_n=0.0, sweeps=1):
    """Alternating least squares from `model`'s tables on the device: each sweep solves every user row against V
    (engine.ridge_rows over the users' segments), then every item row against the new U; a row without ratings becomes zero.
    Returns (MF.from_tables(U, V), objectives): the float64 value of sum e^2 + sum_rows (l2 + l2_n n_row) |x|^2 (ratings as
    the float32 rating / 5 the kernel reads) before the first and after every half sweep, 1 + 2 * sweeps numbers computed on
    the device.  Each half sweep minimises the objective exactly over its block.  No RNG is drawn; opt-in, not wired into Sisa
    or the CLI."""
    from ..ridge import check_ridge_args
    l2, l2_n = check_ridge_args(l2, l2_n)
    if isinstance(sweeps, bool) or not isinstance(sweeps, (int, np.integer)) or sweeps < 0:
        raise ValueError(f'sweeps must be an integer >= 0, not {sweeps!r}')
    refuse_nmf(model, 'als_sweeps')
    uid, iid, r = _rating_triple(train_data)
    U, V, d = padded_tables(model)
    k, dev = int(model.k), U.device
    n_user, n_item = int(U.shape[0]), int(V.shape[0])
    by_user = engine.SegmentSet(uid, iid, r, n_user, device=dev)
    by_item = engine.SegmentSet(iid, uid, r, n_item, device=dev)
    pairs = engine.upload_many([uid.astype(np.int32), iid.astype(np.int32), r], dev)
    reg_u = torch.from_numpy(l2 + l2_n * by_user.counts.astype(np.float64)).to(dev)
    reg_v = torch.from_numpy(l2 + l2_n * by_item.counts.astype(np.float64)).to(dev)
    objectives = [_ridge_objective_dev(U, V, k, pairs, reg_u, reg_v)]
    for _ in range(int(sweeps)):
        U = engine.ridge_rows(V, d, k, by_user, l2, l2_n)
        objectives.append(_ridge_objective_dev(U, V, k, pairs, reg_u, reg_v))
        V = engine.ridge_rows(U, d, k, by_item, l2, l2_n)
        objectives.append(_ridge_objective_dev(U, V, k, pairs, reg_u, reg_v))
    return MF.from_tables(U[:, :k].clone().contiguous(), V[:, :k].clone().contiguous()), np.asarray(objectives, dtype=np.float64)


class WmfSweeps:
    """The device state of implicit ALS on one rating set (ultrare_amd/wmf.py): the two CSRs with their confidence
    weights, the current tables and their Gram matrices.  sweep() runs the user half (every user row against V and the Gram
    matrix of ALL of V: engine.gram, engine.wridge_rows) and then the item half against the new U; objective() is the contract's J
    in float64 on the device from the Gram matrices at hand (a diagnostic, not a hot path).  wmf_sweeps and Scratch's 'wmf'
    backbone drive it.  No RNG is drawn."""

    def __init__(self, U, V, d, k, triple, alpha, l2, l2_n):
        uid, iid, r = triple
        self.d, self.k, self.l2, self.l2_n = d, k, l2, l2_n
        dev = U.device
        self.by_user = engine.SegmentSet(uid, iid, r, int(U.shape[0]), device=dev)
        self.by_item = engine.SegmentSet(iid, uid, r, int(V.shape[0]), device=dev)
        self.w_user = engine.confidence(self.by_user.val[:self.by_user.nnz], alpha)
        self.w_item = engine.confidence(self.by_item.val[:self.by_item.nnz], alpha)
        self.uid, self.iid, val = engine.upload_many([uid.astype(np.int32), iid.astype(np.int32), r], dev)
        self.w_pair = engine.confidence(val, alpha)
        self.reg_u = torch.from_numpy(l2 + l2_n * self.by_user.counts.astype(np.float64)).to(dev)
        self.reg_v = torch.from_numpy(l2 + l2_n * self.by_item.counts.astype(np.float64)).to(dev)
        a, b = np.triu_indices(k)
        self.twice = torch.from_numpy(np.where(a == b, 1.0, 2.0)).to(dev)          # the packed triangle holds (a, b), a < b, once
        self.U, self.V = U, V
        self.GU, self.GV = engine.gram(U, d, k), engine.gram(V, d, k)

    def half_user(self):
        self.U = engine.wridge_rows(self.V, self.d, self.k, self.by_user, *self.w_user, self.GV, self.l2, self.l2_n)
        self.GU = engine.gram(self.U, self.d, self.k)

    def half_item(self):
        self.V = engine.wridge_rows(self.U, self.d, self.k, self.by_item, *self.w_item, self.GU, self.l2, self.l2_n)
        self.GV = engine.gram(self.V, self.d, self.k)

    def sweep(self):
        self.half_user()
        self.half_item()

    def objective(self, chunk=1 << 20):
        k, (wg, wb) = self.k, self.w_pair
        tot = (self.twice * self.GU * self.GV).sum()
        for a in range(0, self.uid.numel(), chunk):
            u, i = self.uid[a:a + chunk].long(), self.iid[a:a + chunk].long()
            s = (self.U[u, :k].double() * self.V[i, :k].double()).sum(dim=1)
            g, b = wg[a:a + chunk].double(), wb[a:a + chunk].double()
            tot = tot + (g * s * s - 2.0 * b * s + b).sum()
        tot = tot + (self.reg_u * (self.U[:, :k].double() ** 2).sum(dim=1)).sum() + (self.reg_v * (self.V[:, :k].double() ** 2).sum(dim=1)).sum()
        return float(tot)

    def tables(self):
        """Copies of the current (U [n_user, k], V [n_item, k])."""
        return self.U[:, :self.k].clone().contiguous(), self.V[:, :self.k].clone().contiguous()


def wmf_sweeps(model, train_data, alpha, l2, l2_n=0.0, sweeps=1):
    """Weighted matrix factorisation for implicit feedback by alternating least squares from `model`'s tables on the device
    (ultrare_amd/wmf.py), the implicit twin of als_sweeps.  Every training triple is an observation of preference 1
    and confidence 1 + alpha * rating / 5; every other (user, item) pair counts with preference 0 and confidence 1.  Each sweep
    solves every user row against V and then every item row against the new U (WmfSweeps); a row without observations becomes
    zero.  Returns (MF.from_tables(U, V), objectives): the float64 objective over ALL pairs (wmf.objective_ref) before the first
    and after every half sweep, 1 + 2 * sweeps numbers computed on the device.  ValueError for bad settings before any device
    work (wmf.check_wmf_args: l2 must be > 0) and for the 'nmf' backbone.  No RNG is drawn."""
    from ..wmf import check_wmf_args
    alpha, l2, l2_n, sweeps = check_wmf_args(alpha, l2, l2_n, sweeps)
    refuse_nmf(model, 'wmf_sweeps')
    U, V, d = padded_tables(model)
    job = WmfSweeps(U, V, d, int(model.k), _rating_triple(train_data), alpha, l2, l2_n)
    objectives = [job.objective()]
    for _ in range(sweeps):
        job.half_user()
        objectives.append(job.objective())
        job.half_item()
        objectives.append(job.objective())
    return MF.from_tables(*job.tables()), np.asarray(objectives, dtype=np.float64)


def wmf_fold_in(models, data, alpha, l2, l2_n=0.0, item_table='mean'):
    """fold_in under the implicit-feedback objective of wmf_sweeps: the user half alone, against frozen items.  User u's row
    solves (V^T V + sum_j (c_j - 1) v_j v_j^T + (l2 + l2_n n_u) I) x = sum_j c_j v_j over u's observations, c_j = 1 + alpha *
    rating / 5, with V^T V the Gram matrix of the WHOLE item table (engine.gram, engine.wridge_rows).  data, item_table and the
    return value -- (users ascending int64, rows [n, k] float32 on the device) -- are fold_in's; the rows equal a user half sweep of
    wmf_sweeps on those users against that table.  ValueError for bad settings before any device work."""
    from ..wmf import check_wmf_args
    alpha, l2, l2_n, _ = check_wmf_args(alpha, l2, l2_n, 1)
    S = len(models)
    refuse_nmf(models, 'wmf_fold_in')
    if S < 1:
        raise ValueError('wmf_fold_in needs at least one model')
    _check_item_table(item_table, S)
    uid, iid, r = _rating_triple(data)
    if len(uid) and (uid.min() < 0 or iid.min() < 0):
        raise ValueError('negative user or item id')
    users, seg = np.unique(uid, return_inverse=True)
    if isinstance(item_table, str):
        tabs = [padded_tables(m) for m in models]
        d = tabs[0][2]
        acc = tabs[0][1].double()
        for _, V, _ in tabs[1:]:
            acc = acc + V.double()
        V = (acc / S).float().contiguous()
    else:
        _, V, d = padded_tables(models[int(item_table)])
    k = int(models[0].k)
    segs = engine.SegmentSet(seg, iid, r, len(users), device=V.device)
    wg, wb = engine.confidence(segs.val[:segs.nnz], alpha)
    X = engine.wridge_rows(V, d, k, segs, wg, wb, engine.gram(V, d, k), l2, l2_n)
    return users.astype(np.int64), X[:, :k].contiguous()


def _ranking_weights(combiner, models, users, who):
    """What recommend / rank_eval check of a combiner before any device work (ValueError): NeuMF models by name, the number of
    models it was fitted on, and under the logistic link a query user in no group.  -> a function of the padded tables that
    gives engine's weights = (link, W, group_of_user) on their device."""
    refuse_nmf(models, f'{who}(combiner=)')
    n_user = int(models[0].user_mat.weight.shape[0]) if len(models) else 0
    combiner.check_query(len(models), users, n_user)
    return lambda tabs: (combiner.link_code, *combiner.on_device_for_query(tabs[0][0].device, int(tabs[0][0].shape[0])))


def recommend(models, users, top_k=10, exclude=None, combiner=None):
    """The top_k items of each user in `users` over the whole catalogue, by the score baseTest gives the pair (the mean of
    `models`, bit for bit), ties by ascending item id.  exclude: a scipy CSR with user ids as rows (read.readSparseMat of the
    training set) whose items are never returned.  Returns (scores [n, top_k], items [n, top_k] int64) on the device; a user
    with fewer eligible items than top_k gets (NaN, -1) at the end.  The full model is recommend([model], ...).
    NeuMF models are answered by recommend_nmf.
    combiner (fit_combiner's result, optional): the score is baseTest(..., combiner=)'s for the pair instead, bit for bit, and
    the order is by that float (under the logistic link many items can share 1.0f: ties by item id).  ValueError before any
    device work for a combiner fitted on another number of models and, under the logistic link, for a query user in no group
    (under the linear link such a user takes the mean weights)."""
    refuse_nmf(models, 'recommend')
    users = np.asarray(users.cpu() if torch.is_tensor(users) else users, dtype=np.int64).reshape(-1)
    weights = _ranking_weights(combiner, models, users, 'recommend') if combiner is not None else None
    tabs = [padded_tables(m) for m in models]
    excl = engine.exclusion_rows(exclude, users) if exclude is not None else None
    return engine.recommend([(U, V) for U, V, _ in tabs], tabs[0][2], users, top_k, excl, weights=weights and weights(tabs))


def relevant_pairs(test_data, n_item):
    """The distinct (user, item) pairs of a test loader (accepted as baseTest accepts one), grouped by user:
    (users [n] int64 ascending, off [n + 1] int64, items int32 ascending within each user)."""
    ds = as_loader(test_data).dataset
    u, i = np.asarray(ds.users, dtype=np.int64), np.asarray(ds.items, dtype=np.int64)
    if i.size and (i.min() < 0 or i.max() >= n_item):
        raise ValueError(f'test items outside [0, {n_item})')
    pair = np.unique(u * n_item + i)
    pu, pi = pair // n_item, pair % n_item
    users, counts = np.unique(pu, return_counts=True)
    off = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    return users, off, pi.astype(np.int32)


def rank_metrics(off, ranks, ks=(10, 20)):
    """Full-ranking metrics from the ranks of each user's relevant items (user q's at ranks[off[q]:off[q + 1]], -1 for an
    excluded one, which does not count).  Per user over its R_u counted ranks, users with none skipped:
      HR@K = [min rank < K]    Recall@K = #{rank < K} / |R_u|    MRR = 1 / (1 + min rank)
      NDCG@K = sum over rank < K of 1 / log2(rank + 2), over the ideal sum of 1 / log2(i + 2) for i < min(|R_u|, K)
    Returns {'hr@K', 'recall@K', 'ndcg@K' for each K, 'mrr', 'n_users', 'n_pairs'}: float64 means over the counted users,
    n_pairs the counted ranks."""
    off = np.asarray(off, dtype=np.int64)
    ranks = np.asarray(ranks.cpu() if torch.is_tensor(ranks) else ranks, dtype=np.int64).reshape(-1)
    n = len(off) - 1
    row = np.repeat(np.arange(n), np.diff(off))
    ok = ranks >= 0
    row, r = row[ok], ranks[ok]
    R = np.bincount(row, minlength=n)
    keep = R > 0
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, row, r)
    best = best[keep].astype(np.float64)
    out = {}
    for K in ks:
        K = int(K)
        hit = r < K
        n_hit = np.bincount(row[hit], minlength=n)[keep]
        dcg = np.bincount(row[hit], weights=1.0 / np.log2(r[hit] + 2.0), minlength=n)[keep]
        ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(K) + 2.0))])[np.minimum(R[keep], K)]
        out[f'hr@{K}'] = float(np.mean(best < K)) if keep.any() else 0.0
        out[f'recall@{K}'] = float(np.mean(n_hit / R[keep])) if keep.any() else 0.0
        out[f'ndcg@{K}'] = float(np.mean(dcg / ideal)) if keep.any() else 0.0
    out['mrr'] = float(np.mean(1.0 / (1.0 + best))) if keep.any() else 0.0
    out['n_users'] = int(keep.sum())
    out['n_pairs'] = int(len(r))
    return out


def rank_eval(models, test_data, exclude=None, ks=(10, 20), combiner=None):
    """Full-ranking evaluation of the ensemble mean of `models` (the score baseTest gives a pair, bit for bit): every distinct
    (user, item) pair of `test_data` (a test loader, as baseTest takes) is ranked among ALL items the user has not trained on
    -- exclude: a scipy CSR with user ids as rows, read.readSparseMat of the training set -- by (score, id) as recommend orders
    them, and HR@K, Recall@K, NDCG@K and MRR are taken from those ranks (rank_metrics; every test pair is relevant, no rating
    threshold).  These are NOT baseTest's HR@10 / NDCG@10, which rank a user's test items only against each other.  A test pair
    that is also in `exclude` does not count.  Returns the dict of rank_metrics.  NeuMF models are evaluated by rank_eval_nmf.
    combiner (optional): the ranks under the fitted weights, as recommend(..., combiner=) orders the items, with its refusals."""
    refuse_nmf(models, 'rank_eval')
    if combiner is not None:
        n_item = int(models[0].item_mat.weight.shape[0]) if len(models) else 0
        weights = _ranking_weights(combiner, models, relevant_pairs(test_data, n_item)[0], 'rank_eval')
    tabs = [padded_tables(m) for m in models]
    users, off, items = relevant_pairs(test_data, int(tabs[0][1].shape[0]))
    excl = engine.exclusion_rows(exclude, users) if exclude is not None else None
    ranks = engine.rank_pairs([(U, V) for U, V, _ in tabs], tabs[0][2], users, (off, items), excl,
                              weights=weights(tabs) if combiner is not None else None)
    return rank_metrics(off, ranks, ks)


def _nmf_ensemble(models, who):
    """[(U, V, dense)], k, layers of a list of NMF models of ONE stack, or ValueError."""
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    if not models:
        raise ValueError(f'{who} needs at least one model')
    for m in models:
        if not isinstance(m, NMF):
            raise ValueError(f"{who} takes models of the 'nmf' backbone only, not {type(m).__name__} (recommend / rank_eval serve 'mf' and 'lightgcn')")
    k, layers = models[0].k, list(models[0].layers)
    for m in models:
        if (m.k, list(m.layers)) != (k, layers):
            raise ValueError(f'{who}: the models of an ensemble share one stack, not k = {k}, layers = {layers} and k = {m.k}, layers = {list(m.layers)}')
    tabs = [m.tables() for m in models]
    if not all(t.is_cuda for tab in tabs for t in tab):
        raise nv.NativeError('model tables are not on the HIP device (call model.to("cuda")): no CPU fallback')
    return tabs, k, layers


def recommend_nmf(models, users, top_k=10, exclude=None):
    """recommend for NeuMF models (a list of NMF of one stack): the top_k items of each user over the whole catalogue by the score
    baseTest gives the pair (the ensemble mean of the models' forwards, bit for bit), ties by ascending item id; exclude and the
    return values as recommend's."""
    tabs, k, layers = _nmf_ensemble(models, 'recommend_nmf')
    users = np.asarray(users.cpu() if torch.is_tensor(users) else users, dtype=np.int64).reshape(-1)
    excl = engine.exclusion_rows(exclude, users) if exclude is not None else None
    return engine.nmf_recommend(tabs, k, layers, users, top_k, excl)


def rank_eval_nmf(models, test_data, exclude=None, ks=(10, 20)):
    """rank_eval for NeuMF models (a list of NMF of one stack): every distinct (user, item) pair of `test_data` ranked among all
    items the user has not trained on, by (score, id) as recommend_nmf orders them.  Returns the dict of rank_metrics."""
    tabs, k, layers = _nmf_ensemble(models, 'rank_eval_nmf')
    users, off, items = relevant_pairs(test_data, int(tabs[0][1].shape[0]))
    excl = engine.exclusion_rows(exclude, users) if exclude is not None else None
    ranks = engine.nmf_rank_pairs(tabs, k, layers, users, (off, items), excl)
    return rank_metrics(off, ranks, ks)


def computeNDCG(r, top_k):
    """utils.py:190-207 (host helper; the device kernel computes the same value)."""
    r = np.asarray(r, dtype=np.float64)
    if len(r) == 0:
        return 0
    r = np.concatenate([r, np.zeros(top_k - len(r))])
    return computeDCG(r) / computeDCG(np.ones(top_k))


def computeDCG(r):
    """utils.py:209-210."""
    return r[0] + np.sum(r[1:] / np.log2(np.arange(2, len(r) + 1)))


def dist_rank():
    """(rank, torch.distributed module or None): who writes artifacts when several ranks run the same call."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist
    return 0, None


def atomic_save(path, writer):
    """Write a file under a temporary name and rename it into place: a reader on another rank never sees half of it."""
    tmp = f'{path}.tmp{os.getpid()}'
    writer(tmp)
    os.replace(tmp, path)


def saveObject(filename, obj):
    def write(tmp):
        with open(tmp, 'wb') as output:
            pickle.dump(obj, output, pickle.HIGHEST_PROTOCOL)
    atomic_save(filename + '.pkl', write)


def loadObject(filename):
    with open(filename + '.pkl', 'rb') as input:
        return pickle.load(input)


def timefn(fn):
    """utils.py:616-626."""
    @wraps(fn)
    def measure_time(*args, **kwargs):
        t1 = time.time()
        result = fn(*args, **kwargs)
        print(f"@time: {time.time() - t1: .5f} s")
        return result
    return measure_time


def _is_sparse(X):
    """A SciPy sparse matrix, or the (csr, csc) pair sparse_group.canonical_csr made of one."""
    import sys
    if isinstance(X, tuple):
        return len(X) == 2 and all(isinstance(h, Compressed) for h in X)
    sp = sys.modules.get('scipy.sparse')           # (a sparse matrix cannot exist before scipy.sparse was imported)
    return sp is not None and sp.issparse(X)


def _round_clock(timing):
    """A round's start on the host's clock -> part(name), which ends a part of the round (bench.py's OT leg): it synchronises
    and takes a mark, and last=True appends the round's dict of milliseconds to `timing`.  Nothing unless timing is a list."""
    marks = []

    def part(name, last=False):
        if timing is not None:
            torch.cuda.synchronize()
            marks.append((name, time.perf_counter()))
            if last:
                timing.append({b[0] + '_ms': round((b[1] - a[1]) * 1e3, 4) for a, b in zip(marks[:-1], marks[1:])})
    part('start')
    return part


def _dense_rows(X, k, idx):
    """The row side of _ot_rounds for a float32 array [n, d] -> (start centroids, cost, centroids, mfma_cost): ure_ot_cost
    against centroids that go to the device every round (a timed part of its own), the update by ure_ot_centroids_members;
    mfma_cost() is the MFMA form of the last cost matrix in a buffer of its own (_exact_lp's cross-check)."""
    n, d = X.shape
    L, st, dev = nv.lib(), nv.stream_handle(), engine._device()
    Xd, cd = torch.from_numpy(X).to(dev), None
    dist_d, cent_d = (torch.empty(k, m, dtype=torch.float32, device=dev) for m in (n, d))
    counts_d = torch.empty(k, dtype=torch.int32, device=dev)

    def launch(entry, out):
        nv.check(getattr(L, entry)(nv.ptr(Xd), nv.ptr(cd), n, k, d, nv.ptr(out), st), entry)
        return out

    def cost(centroid, part):
        nonlocal cd
        cd = torch.from_numpy(np.ascontiguousarray(centroid, dtype=np.float32)).to(dev)
        part('centroid_upload')
        return launch('ure_ot_cost', dist_d)

    def centroids(label, sizes):
        # utils.py:648 from member lists: a stable sort of the labels (ascending id inside a cluster = numpy's order of addition)
        # (labels as the narrowest unsigned type: numpy's stable sort of 8- and 16-bit keys is a radix sort -- 0.3 ms instead of 3 at n = 162,000)
        keys = label.astype(np.uint8 if k <= 256 else np.uint16 if k <= 65536 else np.int64)
        order = torch.from_numpy(np.argsort(keys, kind='stable').astype(np.int32)).to(dev)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).to(dev)
        nv.check(L.ure_ot_centroids_members(nv.ptr(Xd), nv.ptr(order), nv.ptr(off), n, k, d, nv.ptr(cent_d), nv.ptr(counts_d), st),
                 'ure_ot_centroids_members')
        return cent_d.cpu().numpy()
    return X[idx], cost, centroids, lambda: launch('ure_ot_cost_mfma', torch.empty_like(dist_d))


def _csr_rows(halves, k, idx):
    """The row side for the checked (csr, csc) pair of a SciPy sparse matrix (the ratings, n_user x n_item), never densified:
    engine.csr_cost and engine.csr_centroids (arithmetic: sparse_group.py; the reference's own branch raises).  The centroids
    stay on the device between rounds, transposed; the host's copy serves the allclose stop.  There is no MFMA form."""
    start = dense_rows(halves[0], idx)
    S = engine.CsrSet(halves)
    Ct = torch.from_numpy(np.ascontiguousarray(start.T)).to(S.device)

    def cost(centroid, part):
        return engine.csr_cost(S, Ct, k)                              # (Ct holds `centroid`)

    def centroids(label, sizes):
        nonlocal Ct
        Ct, _ = engine.csr_centroids(S, label, k)
        return np.ascontiguousarray(Ct.cpu().numpy().T)
    return start, cost, centroids, None


def _exact_lp(n, k, mfma_cost=None, mismatches=None):
    """The solver side of _ot_rounds for the exact LP on the host (the reference's arithmetic) -> (name, solve, why_empty);
    solve(dist_d, part) -> (label, the host matrix).  The cluster potentials, by dual ascent on the device and carried from round
    to round, are a warm start only: the LP is solved exactly for any potentials.  mismatches (a list): every round is also solved
    on mfma_cost() from the same potentials and the labels that differ are counted -- what that form needs before anyone relies on it."""
    pi = np.zeros(k, dtype=np.float64)

    def assign(dist_d, pi, part):                                     # pi in: the previous round's, out: this round's
        nv.check(nv.lib().ure_ot_potentials(nv.ptr(dist_d), n, k, ot_warm_iters(n), pi.ctypes.data, None, nv.stream_handle()), 'ure_ot_potentials')
        part('device_potentials')
        dist = dist_d.cpu().numpy()                                   # [k, n] fp32 (synchronises)
        part('cost_to_host')
        label = nv.ot_assign_warm(dist, pi, want_plan=False)[0]       # exact EMD + argmax (host)
        part('host_solver')
        return label, dist

    def solve(dist_d, part):
        fast_label = None if mismatches is None else assign(mfma_cost(), pi.copy(), _round_clock(None))[0]
        label, dist = assign(dist_d, pi, part)
        if mismatches is not None:
            mismatches.append(int((fast_label != label).sum()))
        return label, dist
    return 'exact', solve, lambda dist_d: f'the exact plan gives every cluster n / k = {n / k:g} points, so k = {k} is too large for n = {n}'


def _sinkhorn(reg, num_iter_max, stop_thr, stats):
    """The solver side for entropic OT on the device (engine.ot_sinkhorn; labels = argmax of each point's plan row), every round
    from zero potentials; solve -> (label, every point's cheapest cost as one row): only these 2 n values come to the host,
    never the [k, n] matrix.  stats receives (iterations, marginal error) of every round."""
    def solve(dist_d, part):
        r = engine.ot_sinkhorn(dist_d, reg, num_iter_max, stop_thr, want_u=False, want_cost_min=True)
        stats.append((r['iters'], r['err']))
        label, cost_min = r['label'].cpu().numpy(), r['cost_min'].cpu().numpy()
        part('device_sinkhorn')
        return label, cost_min[None]
    return 'sinkhorn', solve, lambda dist_d: f'reg = {reg:g} against costs up to {float(dist_d.max()):.4g}: a larger reg balances the groups'


def _ot_rounds(k, rows, solver, max_iters, refuse_empty, timing):
    """utils.py:637-648 for any row side and solver side, until utils.py's allclose stop or max_iters rounds -> (inertia, label)
    of the last round.  The inertia is np.min(. , axis=0).sum() of what solve returned beside the labels: the same float32 values
    in the same order for both solvers.  refuse_empty: a cluster without a point raises; otherwise it is the row side's business."""
    (centroid, cost, centroids, _), (name, solve, why_empty) = rows, solver
    for rnd in range(max_iters):
        part = _round_clock(timing)
        dist_d = cost(centroid, part)
        part('cost_kernel')
        label, costs = solve(dist_d, part)
        sizes = np.bincount(label, minlength=k)
        if refuse_empty and (sizes == 0).any():
            raise ValueError(f'ot_cluster(solver=\'{name}\'): round {rnd}: cluster(s) {np.flatnonzero(sizes == 0).tolist()} received no '
                             f'point, so their centroid (utils.py:648) is undefined; {why_empty(dist_d)}')
        new_centroid = centroids(label, sizes)
        part('centroids', last=True)
        if np.allclose(centroid, new_centroid):
            break
        centroid = new_centroid
    return np.min(costs, axis=0).sum(), label


@timefn
def ot_cluster(X, k, max_iters=10, timing=None, solver='exact', reg=1e-3, num_iter_max=1000, stop_thr=1e-9):
    """utils.py:628-656.  Initial centroids come from the global numpy generator, as in the reference.  Returns (inertia,
    label[int64]).  solver='exact' (the default, the reference's arithmetic: exact EMD) or 'sinkhorn': every round's
    transport is entropic OT solved on the device, an opt-in that is not bit-parity with the reference; reg, num_iter_max and
    stop_thr are its settings and are ignored by the exact solver; ot_cluster.sinkhorn_stats: (iterations, error) per round.
    X may be a SciPy sparse matrix (the ratings): the same rounds (_ot_rounds) then run through the CSR cost and centroid kernels
    and the n x d array is never formed.  A cluster without a point is refused, except by the exact solver on dense rows: the
    reference-parity route carries numpy's NaN row of an empty mean forward (and URE_OT_MFMA=1 sets ot_cluster.mfma_mismatches).
    timing (a list, optional) receives every round's parts in milliseconds, for every combination: centroid_upload_ms (dense
    rows only), cost_kernel_ms, device_potentials_ms + cost_to_host_ms + host_solver_ms or device_sinkhorn_ms, centroids_ms."""
    if solver not in ('exact', 'sinkhorn'):
        raise ValueError(f"solver must be 'exact' or 'sinkhorn', not {solver!r}")
    if solver == 'sinkhorn':
        engine.check_sinkhorn_args(reg, num_iter_max, stop_thr)
    sparse = _is_sparse(X)
    if sparse:
        X = check_cluster_args(X, k)                                  # (the checked (csr, csc) pair)
        n = X[0].shape[0]
    else:
        X = np.ascontiguousarray(X, dtype=np.float32)
        n, _ = X.shape
        if k < 1 or k > n:
            raise ValueError('need 1 <= k <= n clusters')
    if solver == 'sinkhorn' and k > engine.SINKHORN_MAX_K:
        raise ValueError(f'the sinkhorn solver takes at most {engine.SINKHORN_MAX_K} clusters, not {k}')
    idx = np.random.choice(n, size=k, replace=False)
    rows = _csr_rows(X, k, idx) if sparse else _dense_rows(X, k, idx)
    if solver == 'sinkhorn':
        ot_cluster.sinkhorn_stats = []
        side = _sinkhorn(reg, num_iter_max, stop_thr, ot_cluster.sinkhorn_stats)
    elif sparse:
        side = _exact_lp(n, k)
    else:
        ot_cluster.mfma_mismatches = [] if os.environ.get('URE_OT_MFMA', '0') == '1' else None
        side = _exact_lp(n, k, rows[3], ot_cluster.mfma_mismatches)
    inertia, label = _ot_rounds(k, rows, side, max_iters, sparse or solver == 'sinkhorn', timing)
    print(f'{inertia:.3f}', end=' ')
    return inertia, label.astype(np.int64)


# ---------------------------------------------------------------------------
# Comparison clusterers (utils.py:354-418): k-means / balanced k-means on the embedding the
# reference's notebook compared OT grouping against.  Distances and centroid updates run on the
# GPU in scipy's csr arithmetic (labels identical to the reference's), the assignment -- a global
# sort of n*k distances and a greedy fill -- on the host.
# ---------------------------------------------------------------------------
def _best_of(n_init, run):
    """The labels of the first of n_init calls of run() -> (label, inertia, ...) with the smallest inertia below 1e10, else None."""
    best, fin_label = 1e10, None
    for _ in range(n_init):
        label, inertia = run()[:2]
        if inertia < best:
            best, fin_label = inertia, label
    return fin_label


def _host_assign(dist, n, k, capacity):
    """ure_host_kmeans_assign on a host dist [n, k] float32 -> (label int32 [n], inertia): the nearest column, or groups of `capacity` filled in ascending distance."""
    label, inertia = np.empty(n, dtype=np.int32), ctypes.c_double(0.0)
    nv.check(nv.lib().ure_host_kmeans_assign(dist.ctypes.data, n, k, capacity, label.ctypes.data, ctypes.byref(inertia)), 'ure_host_kmeans_assign')
    return label, float(inertia.value)


def _dense_f32(sp_mat):
    return np.ascontiguousarray(sp_mat.toarray() if hasattr(sp_mat, 'toarray') else sp_mat, dtype=np.float32)


def _kmeans_takes_csr(sp_mat):
    """The CSR route (csrc/csr_kmeans.hip): always for a (csr, csc) pair of Compressed, and for a SciPy sparse matrix wider
    than group.DENSE_MAX_ITEMS; everything else keeps the dense route."""
    if not _is_sparse(sp_mat):
        return False
    if isinstance(sp_mat, tuple):
        return True
    from ..group import DENSE_MAX_ITEMS
    return len(sp_mat.shape) != 2 or sp_mat.shape[1] > DENSE_MAX_ITEMS      # (not 2-D: check_kmeans_args refuses it)


def _kmeans_csr_set(sp_mat, k, n_user):
    """The checked matrix on the device; every refusal comes before any device work."""
    from ..sparse_kmeans import check_kmeans_args
    halves = check_kmeans_args(sp_mat, k)
    if halves[0].shape[0] != n_user:
        raise ValueError(f'n_user = {n_user} but the matrix has {halves[0].shape[0]} rows')
    return engine.CsrSet(halves)


def _single_kmeans_csr(k, n_user, S, balanced, max_iter, rounds=None):
    """singleKmeans on the sparse rating matrix S (an engine.CsrSet, checked by check_kmeans_args), never densified: per
    round ure_csr_kmeans_cost -> ure_balanced_fill (the fill, or the argmin) -> the labels and the n chosen distances to
    the host -> ure_csr_kmeans_centroids.  The same draw, the same float32 arithmetic and the same stop as the dense route:
    equal labels and inertia.  rounds (a list) receives the fill's round count of every k-means round."""
    n = S.n
    assert n == n_user
    group_len = int(np.ceil(n_user / k))
    cen_idx = np.random.choice(n_user, k, replace=False)
    Ct = torch.from_numpy(np.ascontiguousarray(dense_rows(S.csr, cen_idx).T)).to(S.device)
    label, inertia = np.zeros(n, dtype=np.int32), 0.0
    for _ in range(max_iter):
        dist_d = engine.csr_kmeans_cost(S, Ct, k)
        label_d, fill_rounds = engine.balanced_fill(dist_d, group_len if balanced else 0)
        if rounds is not None:
            rounds.append(fill_rounds)
        chosen = dist_d.gather(1, label_d.to(torch.int64).unsqueeze(1)).squeeze(1)
        new_label = label_d.cpu().numpy()
        inertia = float(np.sum(chosen.cpu().numpy()))       # numpy's float32 pairwise sum, as ure_host_kmeans_assign restates it
        if (new_label == label).all():
            break
        label = new_label
        Ct, counts = engine.csr_kmeans_centroids(S, label_d, k)
        if int(counts.min().item()) == 0:
            raise ZeroDivisionError('a cluster lost all its members (utils.py:403 divides by its size)')
    return label.astype(np.int64), inertia


def singleKmeans(k, n_user, sp_mat, balanced, max_iter):
    """utils.py:354-404.  sp_mat: csr_matrix or array [n_user, n_embedding]; initial centroids from
    numpy's global generator.  Returns (label int64 [n_user], inertia).  A (csr, csc) pair of sparse_group.Compressed, and a
    SciPy sparse matrix wider than group.DENSE_MAX_ITEMS, run on the sparse matrix (_single_kmeans_csr); bad input is
    refused before any device work."""
    if _kmeans_takes_csr(sp_mat):
        return _single_kmeans_csr(k, n_user, _kmeans_csr_set(sp_mat, k, n_user), balanced, max_iter)
    X = _dense_f32(sp_mat)
    n, d = X.shape
    assert n == n_user
    if k < 1 or k > n:
        raise ValueError('need 1 <= k <= n clusters')
    L, st, dev = nv.lib(), nv.stream_handle(), engine._device()
    group_len = int(np.ceil(n_user / k))
    cen_idx = np.random.choice(n_user, k, replace=False)
    Xd = torch.from_numpy(X).to(dev)
    cent_d = Xd[torch.from_numpy(cen_idx).to(dev)].contiguous()
    dist_d = torch.empty(n, k, dtype=torch.float32, device=dev)
    label_d = torch.empty(n, dtype=torch.int32, device=dev)
    counts_d = torch.empty(k, dtype=torch.int32, device=dev)
    label, inertia = np.zeros(n, dtype=np.int32), 0.0
    for _ in range(max_iter):
        nv.check(L.ure_kmeans_cost(nv.ptr(Xd), nv.ptr(cent_d), n, k, d, nv.ptr(dist_d), st), 'ure_kmeans_cost')
        new_label, inertia = _host_assign(dist_d.cpu().numpy(), n, k, group_len if balanced else 0)
        if (new_label == label).all():
            break
        label = new_label
        label_d.copy_(torch.from_numpy(label))
        nv.check(L.ure_kmeans_centroids(nv.ptr(Xd), nv.ptr(label_d), n, k, d, nv.ptr(cent_d), nv.ptr(counts_d), st),
                 'ure_kmeans_centroids')
        if int(counts_d.min().item()) == 0:
            raise ZeroDivisionError('a cluster lost all its members (utils.py:403 divides by its size)')
    return label.astype(np.int64), inertia


def kmeans(n_group, n_user, sp_mat, balanced=False, n_init=5, max_iter=10):
    """utils.py:406-418: the labels of the best of n_init runs (smallest inertia).  On the CSR route the matrix is checked
    and uploaded once for all runs."""
    if _kmeans_takes_csr(sp_mat):
        S = _kmeans_csr_set(sp_mat, n_group, n_user)
        return _best_of(n_init, lambda: _single_kmeans_csr(n_group, n_user, S, balanced, max_iter))
    return _best_of(n_init, lambda: singleKmeans(n_group, n_user, sp_mat, balanced, max_iter))


# ---------------------------------------------------------------------------
# The user-by-user distance clusterers (utils.py:422-611): the kNN user graph, label propagation and k-medoids.  The
# reference builds a dense n x n array for them (146 MB at ml-1m, 105 GB at n = 162,000); here each needs only a
# reduction of that matrix -- a row's nearest columns, the row sums and the medoid columns, or per-row sums of exp(-D)
# grouped by label -- which csrc/pair_dist.hip computes from tiles that never leave the chip.  `metric=None` takes the
# reference's own contract, a float32 n x n array; 'euclidean' / 'cosine' / 'manhattan' take X [n x d] and stream D, or
# the sparse rating matrix itself (_pair_input), the input the reference documents for these functions.
# The assignments (argmin / argmax, or the balanced greedy fill over a global sort) run on the host.
# ---------------------------------------------------------------------------
def _pair_csr_set(sp_mat, metric, n_user, k=None, k_max=None):
    """The checked sparse matrix on the device (sparse_pair.check_pair_args); every refusal comes before any device work."""
    from ..sparse_pair import check_pair_args
    return engine.CsrSet(check_pair_args(sp_mat, metric, n_user, k, k_max))


def _pair_input(k, n_user, arr, metric, k_max=None):
    """The device distance source of a clusterer call, after the checks that need no device.  A (csr, csc) pair of
    sparse_group.Compressed, and a SciPy sparse matrix wider than group.DENSE_MAX_ITEMS (the rule of _kmeans_takes_csr), go
    through as an engine.CsrSet: D is then streamed from the sparse rows (the CSR tile producer of csrc/pair_dist.hip), bit
    for bit the dense route's D, and n_user x n_item is never formed.  Narrower matrices and arrays keep the dense route."""
    if _kmeans_takes_csr(arr):
        return _pair_csr_set(arr, metric, n_user, k, k_max)
    if not torch.is_tensor(arr):
        arr = _dense_f32(arr) if metric is not None else np.asarray(arr)
    n = int(arr.shape[0]) if len(arr.shape) else 0
    if n != n_user:
        raise ValueError(f'n_user = {n_user} but the input has {n} rows')
    if not 1 <= k <= n:
        raise ValueError(f'need 1 <= k <= n clusters, not k = {k}, n = {n}')
    if k_max is not None and k > k_max:
        raise ValueError(f'at most {k_max} groups, not {k}')
    return engine.pair_source(arr, metric)[0]


def findNeighbor(cache_dir, sp_mat, n_user, var='euclidean', n_neighbor=10):
    """utils.py:422-455: nei_idx int [n_user, n_neighbor], the nearest users of each user by `var` ('euclidean', 'cosine' or
    'manhattan'; ascending distance, exact ties by ascending id, the user itself included), and nei_val float16 = -distance.
    sp_mat: csr_matrix or array [n_user, n_embedding].  Saves np.save(cache_dir + var, [nei_idx, nei_val]) as the reference does.
    As shipped, the reference never reads that cache (`if cache_dir == True` is false for any path), so this always computes
    and then saves.  The distances are the difference form in float32 (csrc/pair_dist.hip), not sklearn's; n_neighbor <= 128.
    A (csr, csc) pair, and a SciPy sparse matrix wider than group.DENSE_MAX_ITEMS, are read as sparse rows and never densified:
    the same lists, and the same cache file, bit for bit."""
    if var not in ('euclidean', 'cosine', 'manhattan'):
        raise ValueError(f"var must be 'euclidean', 'cosine' or 'manhattan', not {var!r}")
    if _kmeans_takes_csr(sp_mat):                  # (the sparse rows themselves: _pair_input's rule)
        X = _pair_csr_set(sp_mat, var, n_user)
    else:
        X = _dense_f32(sp_mat)
        if X.shape[0] != n_user:
            raise ValueError(f'n_user = {n_user} but sp_mat has {X.shape[0]} rows')
    dist, idx = engine.pair_knn(X, n_neighbor, var)
    nei_idx = idx.cpu().numpy().astype(int)
    nei_val = (-dist).cpu().numpy().astype(np.float16)
    np.save(cache_dir + var, [nei_idx, nei_val])
    return nei_idx, nei_val


def _kmedoids_run(k, n, src, R, balanced, max_iter, metric):
    group_len = int(np.ceil(n / k))
    cen_idx = np.random.choice(n, k, replace=False)
    label, inertia = np.zeros(n, dtype=np.int32), 0.0
    for _ in range(max_iter):
        dist = np.ascontiguousarray(engine.pair_cols(src, cen_idx, metric).cpu().numpy())
        new_label, inertia = _host_assign(dist, n, k, group_len if balanced else 0)
        if (new_label == label).all():
            break
        label = new_label
        # as shipped (utils.py:589-594): the new medoid is the member with the smallest sum over ALL n columns (first
        # minimum), not over its own cluster as in textbook PAM
        for c in range(k):
            members = np.flatnonzero(label == c)
            if members.size == 0:
                raise ValueError(f'cluster {c} lost all its members (the reference fails on argmin of an empty array)')
            cen_idx[c] = members[np.argmin(R[members])]
    return label.astype(np.int64), inertia, cen_idx


def singleKmedoids(k, n_user, dist_arr, balanced, max_iter, metric=None, return_medoids=False):
    """utils.py:546-594: one k-medoids run from k medoids drawn by np.random.choice(n_user, k, replace=False) (numpy's global
    generator).  dist_arr: the float32 n x n array (metric None), or X [n x d] with D streamed by `metric`.  Each round assigns
    every user to its nearest medoid (argmin, first minimum) or, balanced, fills groups of ceil(n / k) in ascending distance
    (ure_host_kmeans_assign); the new medoid of a cluster is its member with the smallest row sum over ALL users, as shipped
    (not textbook PAM, which sums over the cluster).  An empty cluster raises ValueError.  Returns (label int64 [n_user],
    inertia = np.sum of the assigned distances in float32), and the final medoids when return_medoids."""
    src = _pair_input(k, n_user, dist_arr, metric)
    R = engine.pair_rowsum(src, metric).cpu().numpy()
    label, inertia, cen_idx = _kmedoids_run(k, n_user, src, R, balanced, max_iter, metric)
    return (label, inertia, cen_idx) if return_medoids else (label, inertia)


def kmedoids(n_group, n_user, arr, balanced=False, n_init=5, max_iter=10, metric=None):
    """utils.py:597-611: the labels of the best of n_init singleKmedoids runs (smallest inertia below 1e10; None when no run
    gets there, as kmeans).  The row sums are computed once and shared by every run."""
    src = _pair_input(n_group, n_user, arr, metric)
    R = engine.pair_rowsum(src, metric).cpu().numpy()
    return _best_of(n_init, lambda: _kmedoids_run(n_group, n_user, src, R, balanced, max_iter, metric))


def _lpa_run(n_group, n, src, balanced, max_iter, metric):
    L = nv.lib()
    group_len = int(np.ceil(n / n_group))
    label = np.random.randint(0, n_group, size=(n))
    inertia = 0.0
    for _ in range(max_iter):
        W = np.ascontiguousarray(engine.pair_label_expsum(src, label, n_group, metric).cpu().numpy())
        if not balanced:
            new_label = W.argmax(axis=1)
            inertia = float(np.sum(W[np.arange(n), new_label]))
        else:
            lab32, inert = np.empty(n, dtype=np.int32), ctypes.c_double(0.0)
            nv.check(L.ure_host_assign_desc_f64(W.ctypes.data, n, n_group, group_len, lab32.ctypes.data, ctypes.byref(inert)),
                     'ure_host_assign_desc_f64')
            new_label, inertia = lab32.astype(np.int64), float(inert.value)
        if (new_label == label).all():
            break
        label = new_label
    return np.asarray(label, dtype=np.int64), inertia


def singleLPA(n_group, n_user, dist_arr, balanced, n_neighbor, max_iter=10, metric=None):
    """utils.py:458-499: label propagation from labels drawn by np.random.randint(0, n_group, size=n_user).  Each round the
    weight of user u for group g is W[u, g] = sum over users i labelled g of exp(-D[i, u]) (float32 exp, float64 sums); the
    new label is the heaviest group (argmax, first maximum) or, balanced, groups of ceil(n / n_group) filled in descending
    weight (ure_host_assign_desc_f64).  n_neighbor is unused, as in the reference.  dist_arr: the float32 n x n array
    (metric None) or X [n x d] with D streamed by `metric`; n_group <= 128.  Returns (label int64, inertia = np.sum of the
    chosen weights).  The reference's progress prints are not reproduced."""
    src = _pair_input(n_group, n_user, dist_arr, metric, k_max=128)
    return _lpa_run(n_group, n_user, src, balanced, max_iter, metric)


def lpa(n_group, n_user, dist_arr, balanced=False, n_init=5, max_iter=10, metric=None):
    """utils.py:502-519: the labels of the n_init singleLPA run with the SMALLEST inertia below 1e10, as shipped (a larger
    weight is the better grouping); None when no run gets there, as kmeans.  Reference defect fixed: utils.py:515 passes
    n_user into singleLPA's `balanced` slot, so the reference always runs balanced LPA; here `balanced` is honoured."""
    src = _pair_input(n_group, n_user, dist_arr, metric, k_max=128)
    return _best_of(n_init, lambda: _lpa_run(n_group, n_user, src, balanced, max_iter, metric))


# ---------------------------------------------------------------------------
# Attribute unlearning (utils.py:223-279; csrc/mmd.hip, the contract is attr_unlearn.py)
# ---------------------------------------------------------------------------
def _two_groups(source, target):
    """(X [n1 + n2, d] float32 on the device, GroupRows) of two device tensors [n1, d], [n2, d]."""
    for t in (source, target):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise nv.NativeError('the MMD kernels run on the HIP device only (no CPU fallback)')
    if source.dim() != 2 or target.dim() != 2 or source.shape[1] != target.shape[1]:
        raise ValueError(f'source and target must be [n1, d] and [n2, d], not {tuple(source.shape)} and {tuple(target.shape)}')
    groups = engine.GroupRows.leading(source.shape[0], target.shape[0], source.device)
    return torch.cat([source.detach().float(), target.detach().float()], dim=0), groups


def rbk(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """utils.py:223-256: the kernel matrix sum_q exp(-|x_i - x_j|^2 / bw_q) [m, m] float32 of the rows of source and target
    (device tensors), built on the device tile by tile.  m = n1 + n2 above 8,192 is refused: mmd_loss needs no matrix."""
    from ..attr_unlearn import RBK_MAX_M, check_mmd_args
    kernel_mul, kernel_num, fix_sigma = check_mmd_args(kernel_mul, kernel_num, fix_sigma)
    m = int(source.shape[0]) + int(target.shape[0])
    if m > RBK_MAX_M:
        raise ValueError(f'rbk would write a {m} x {m} matrix (limit {RBK_MAX_M} rows): use mmd_loss, which streams it')
    X, groups = _two_groups(source, target)
    bw = engine.mmd_bandwidth(X, groups, fix_sigma, check=True)
    return engine.mmd_matrix(X, groups, bw, kernel_mul, kernel_num)


def mmd_loss(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None, want_grad=False):
    """utils.py:258-267: the MMD loss of two groups of rows (device tensors [n1, d], [n2, d]) as a 0-d float64 device tensor;
    the m x m kernel matrix is streamed, never formed.  want_grad: (loss, grad_source [n1, d], grad_target [n2, d]) float32,
    no gradient through the bandwidth (the reference's .data).  ValueError when the bandwidth is not positive and finite."""
    from ..attr_unlearn import check_mmd_args
    kernel_mul, kernel_num, fix_sigma = check_mmd_args(kernel_mul, kernel_num, fix_sigma)
    X, groups = _two_groups(source, target)
    bw = engine.mmd_bandwidth(X, groups, fix_sigma, check=True)
    sums, grad = engine.mmd_loss_grad(X, groups, bw, kernel_mul, kernel_num, want_grad=want_grad)
    loss = engine.mmd_loss_of(sums, groups)
    return (loss, grad[:groups.n1], grad[groups.n1:]) if want_grad else loss


def attribute_unlearn_check(var='d2d', eta=1.0, alpha=0.0, lr=0.1, steps=10, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """The settings of attribute_unlearn, checked on the host (ValueError) -> the eight values."""
    from ..attr_unlearn import check_loop_args, check_mmd_args, check_var
    return (check_var(var),) + check_loop_args(eta, alpha, lr, steps) + check_mmd_args(kernel_mul, kernel_num, fix_sigma)


def attribute_unlearn(model, id1, id2, var='d2d', eta=1.0, alpha=0.0, lr=0.1, steps=10, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """Post-training attribute unlearning: `steps` plain gradient steps U_i -= lr grad_i J on the rows id1 + id2 of
    model.user_mat.weight, in place, J(U) = eta dis(U[id1], U[id2]) + alpha sum_i |U_i - U*_i|^2 with U* the table at entry and
    dis the MMD loss ('d2d', mmd_loss) or the Laplacian value of the complete bipartite graph id1 - id2 ('u2u').  Every other
    row and the item table keep their bytes.  The bandwidth is recomputed from the current rows every step unless fix_sigma is
    given.  The pairwise work is csrc/mmd.hip; the update itself is elementwise float64 on the device, rounded once.  The loop
    reads nothing back: the log -- dict of dis, reg, bandwidth (u2u: NaN), each steps + 1 values, before every step and after
    the last -- comes to the host in one copy at the end.  ValueError before any device work for groups that are empty,
    overlap, repeat a row or leave the table, and for var outside {'d2d', 'u2u'}; ValueError as well for a bandwidth that is
    not positive and finite (at entry: before any change)."""
    from ..attr_unlearn import check_bandwidth
    refuse_nmf(model, 'attribute_unlearn')
    var, eta, alpha, lr, steps, kernel_mul, kernel_num, fix_sigma = attribute_unlearn_check(var, eta, alpha, lr, steps, kernel_mul, kernel_num, fix_sigma)
    W = model.user_mat.weight
    groups = engine.GroupRows(id1, id2, W.shape[0], W.device if W.is_cuda else None)
    U = W.detach()
    if not U.is_cuda:
        raise nv.NativeError('model tables are not on the HIP device (call model.to("cuda")): no CPU fallback')
    if U.dtype != torch.float32 or U.stride(1) != 1:
        raise ValueError('the user table must be float32 with unit column stride')
    at = groups.rows.long()
    start = U.index_select(0, at).double()
    dis_log, reg_log, bw_log = [], [], []
    nan = torch.full((), float('nan'), dtype=torch.float64, device=U.device)
    for t in range(steps + 1):
        if var == 'd2d':
            bw = engine.mmd_bandwidth(U, groups, fix_sigma, check=(t == 0 and fix_sigma is None))
            sums, grad = engine.mmd_loss_grad(U, groups, bw, kernel_mul, kernel_num, want_grad=t < steps)
            dis = engine.mmd_loss_of(sums, groups)
        else:
            bw = nan
            dis, grad = engine.u2u_loss_grad(U, groups, want_grad=t < steps)
        cur = U.index_select(0, at).double()
        delta = cur - start
        dis_log.append(dis)
        reg_log.append((delta * delta).sum())
        bw_log.append(bw)
        if t < steps:
            engine.unlearn_row_step(U, at, start, grad, lr, eta, alpha)
    host = torch.stack(dis_log + reg_log + bw_log).cpu().numpy().reshape(3, steps + 1)
    if var == 'd2d':
        for b in host[2]:
            check_bandwidth(b)
    return {'dis': host[0].tolist(), 'reg': host[1].tolist(), 'bandwidth': host[2].tolist()}


def attribute_attack(model_or_table, id1, id2, hidden=100, folds=5, epochs=None, lr=None, l2=1e-4, seed=0):
    """How much of a binary attribute the user embeddings still carry (the contract is attack.train_ref): a probe with one
    hidden layer of `hidden` relu units (0: logistic regression) is trained on the standardised rows id1 (class 1) and id2 (class 0)
    of the user table by full-batch Adam, `folds`-fold cross-validated, and every row is scored by the fold that held it out.
    model_or_table: a model with user_mat (MF, LightGCN's parameters), or any float32 [n, d <= 128] device tensor with unit column
    stride (final embeddings, one of NeuMF's two user tables, or a torch.cat of both).  The table is read in place and not changed.
    epochs / lr None: attack.DEFAULT_EPOCHS / attack.DEFAULT_LR, chosen on the numpy contract's two synthetic cases and UNTUNED on
    real attribute data.  Everything runs in csrc/attack.hip on one stream; one device-to-host copy, at the end.
    -> dict: auc, bacc, f1 (pooled, out of fold), fold_auc [folds], counts (gt, eq, tp, fn, tn, fp, and per fold gt / eq / n1 / n2),
    loss (first and last epoch, per fold) and settings.  ValueError before any device work for bad groups or settings."""
    from .. import attack as A
    X = model_or_table.user_mat.weight.detach() if hasattr(model_or_table, 'user_mat') else model_or_table
    if not torch.is_tensor(X) or X.dim() != 2:
        raise ValueError('attribute_attack takes a model with user_mat or a 2-d float32 device tensor')
    rows, n1, n2, H, folds, epochs, lr, l2 = A.check_attack_args(X.shape[0], X.shape[1], id1, id2, hidden, folds, epochs, lr, l2)
    if not X.is_cuda:
        raise nv.NativeError('the table is not on the HIP device (call model.to("cuda")): no CPU fallback')
    groups = engine.GroupRows.checked(rows, n1, n2, X.shape[0], X.device)
    fit = engine.attack_fit(X, groups, H, folds, epochs, lr, l2, seed)
    pos, neg = np.arange(n1), np.arange(n1, n1 + n2)
    out = [engine.auc_counts(fit.scores, pos, neg), engine.confusion_counts(fit.scores, pos, neg)]
    sizes = []
    for f in range(folds):
        held = np.flatnonzero(fit.fold_host == f)
        p, n = held[held < n1], held[held >= n1]
        sizes.append((len(p), len(n)))
        out.append(engine.auc_counts(fit.scores, p, n))
    flat = torch.cat([out[0][0], out[0][1].long(), out[1]] + [torch.cat([c, b.long()]) for c, b in out[2:]] +
                     [fit.loss[:, 0].contiguous().view(torch.int64), fit.loss[:, -1].contiguous().view(torch.int64)]).cpu().numpy()
    if flat[2] or any(flat[7 + 3 * f + 2] for f in range(folds)):
        raise ValueError('the probe produced a NaN score: the selected rows of the table are not finite')
    gt, eq, tp, fn, tn, fp = (int(v) for v in (flat[0], flat[1], flat[3], flat[4], flat[5], flat[6]))
    res = A.metrics(gt, eq, tp, fn, tn, fp)
    per = [(int(flat[7 + 3 * f]), int(flat[7 + 3 * f + 1])) + sizes[f] for f in range(folds)]
    res['fold_auc'] = [(g + e / 2.0) / (float(a) * float(b)) for g, e, a, b in per]
    res['counts'] = dict(gt=gt, eq=eq, tp=tp, fn=fn, tn=tn, fp=fp, folds=[dict(gt=g, eq=e, n1=a, n2=b) for g, e, a, b in per])
    loss = flat[7 + 3 * folds:].view(np.float64).reshape(2, folds)
    res['loss'] = dict(first=loss[0].tolist(), last=loss[1].tolist())
    res['settings'] = dict(hidden=H, folds=folds, epochs=epochs, lr=lr, l2=l2, seed=seed, n1=n1, n2=n2, d=int(X.shape[1]))
    return res


def adversarial_unlearn(model, id1, id2, hidden=32, folds=5, rounds=100, disc_epochs=5, disc_lr=1e-2, l2=1e-4, lr=0.1, eta=1.0, alpha=0.0,
                        target='confuse', seed=0):
    """Adversarial attribute unlearning (the contract is adv_unlearn.adversarial_unlearn_ref): `rounds` rounds of a game
    between a discriminator -- attribute_attack's probe, `hidden` relu units, `folds`-fold cross-validated, warm-started and trained
    `disc_epochs` full-batch Adam epochs (disc_lr, l2) per round -- and the rows id1 + id2 of model.user_mat.weight, which take one
    step U_i -= lr (eta g_i + 2 alpha (U_i - U*_i)) per round, IN PLACE: g_i the gradient of the discriminator's cross-entropy on row
    i against the target p = 1 / 2 ('confuse'), under the fold that never trained on row i; U* the table at entry.  Every other row
    and the item table keep their bytes.  target='reverse' (ascending the discriminator's loss) is refused: it diverges.
    The defaults are chosen on two synthetic tables (a planted direction and a null table, DESIGN 4.31's sweep) and are UNTUNED on
    real attribute data.  Judge the result with a FRESH attribute_attack on the moved table, not with the in-loop AUC.
    Everything runs in csrc/attack.hip and csrc/adv.hip on one stream and nothing is read back per round: the log -- dict of
    disc_loss (first and last epoch: [rounds][folds]), auc [rounds] (the in-loop, out-of-fold AUC before the round's step), counts (gt,
    eq per round), reg [rounds] (sum |U - U*|^2 after the round's step) and settings -- comes to the host in one copy at the end.
    ValueError before any device work for bad groups or settings, and at the end when a p was NaN (the rows are not finite)."""
    from ..adv_unlearn import check_adv_args
    refuse_nmf(model, 'adversarial_unlearn')
    W = model.user_mat.weight
    rows, n1, n2, H, folds, rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, tgt = check_adv_args(
        W.shape[0], W.shape[1], id1, id2, hidden, folds, rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, target)
    U = W.detach()
    if not U.is_cuda:
        raise nv.NativeError('model tables are not on the HIP device (call model.to("cuda")): no CPU fallback')
    if U.dtype != torch.float32 or U.stride(1) != 1:
        raise ValueError('the user table must be float32 with unit column stride')
    groups = engine.GroupRows.checked(rows, n1, n2, U.shape[0], U.device)
    fit = engine.adversarial_unlearn(U, groups, H, folds, rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, tgt, seed)
    flat = torch.cat([fit.counts.reshape(-1), fit.nan_flags.long(), fit.reg.view(torch.int64), fit.loss[:, :, 0].contiguous().view(torch.int64).reshape(-1),
                      fit.loss[:, :, -1].contiguous().view(torch.int64).reshape(-1)]).cpu().numpy()
    counts, flags = flat[:2 * rounds].reshape(rounds, 2), flat[2 * rounds:3 * rounds]
    if flags.any():
        raise ValueError('the discriminator produced a NaN p: the selected rows of the table are not finite')
    reg = flat[3 * rounds:4 * rounds].view(np.float64)
    loss = flat[4 * rounds:].view(np.float64).reshape(2, rounds, folds)
    return {'disc_loss': dict(first=loss[0].tolist(), last=loss[1].tolist()),
            'auc': [(int(g) + int(e) / 2.0) / (float(n1) * float(n2)) for g, e in counts],
            'counts': dict(gt=[int(g) for g in counts[:, 0]], eq=[int(e) for e in counts[:, 1]]),
            'reg': reg.tolist(),
            'settings': dict(hidden=H, folds=folds, rounds=rounds, disc_epochs=disc_epochs, disc_lr=disc_lr, l2=l2, lr=lr, eta=eta, alpha=alpha,
                             target=target, seed=seed, n1=n1, n2=n2, d=int(U.shape[1]))}


def newton_unlearn_check(model_type='mf', loss='mse', l2=None, batch=None, lam=None, damping=None, curvature='full', steps=1, iters=512, tol=1e-8,
                         n_rows=0):
    """The settings of newton_unlearn, checked on the host (ValueError) -> (l2, damping).  l2 None: trainer_l2(n_rows, batch, lam)."""
    from ..influence import check_args, check_model
    check_model(model_type, loss)
    if l2 is None:
        if batch is None or lam is None:
            raise ValueError('newton_unlearn needs l2, or batch and lam for l2 = trainer_l2(len(train_data), batch, lam)')
        l2 = trainer_l2(n_rows, batch, lam)
    return check_args(curvature, damping, steps, iters, tol, l2)


def newton_unlearn(model, train_data, l2=None, batch=None, lam=None, damping=None, curvature='full', steps=1, iters=512, tol=1e-8, scope='all'):
    """Approximate unlearning of TRAINED users without retraining (the contract is influence.newton_unlearn_ref):
    `steps` damped Newton steps on F = sum_D e^2 + l2 (|U|^2 + |V|^2) over the REMAINING data D = train_data (a post-deletion
    loader, or a (uid, iid, rating / 5) triple), in place on the two tables of an MF model trained with the MSE loss.  A row
    without an entry in D -- a deleted user's -- becomes +0.0; rows outside scope = (users, items) (None in a slot: all rows of that
    side; 'all': every row) keep their bytes.  Each step solves (H + 2 damping I) x = -grad F by conjugate gradients on the device
    (engine.inf_solve: CSR / CSC Hessian-vector walks in float64, at most `iters` iterations to a relative residual `tol`) and
    rounds theta + x to float32 once.  curvature='full' is the exact Hessian and needs damping > 0 (it is singular along the common
    rotations of both tables); 'gn' is the Gauss-Newton matrix, positive definite and slower to close the gap.
    l2 None: trainer_l2(len(D), batch, lam), the ridge strength of the trainer's own fixed point.  damping None: 0.1 * l2 for 'full'
    and 0 for 'gn' -- the setting of the float64 prototype, a starting point that NOBODY HAS TUNED.
    A step whose solve met non-positive curvature (status 2), or that did not reduce F (the float64 value on the device, one read per
    step), is not applied: the tables keep the last good bytes, the step's log says why and no further step is tried; nothing is
    raised.  Returns the per-step logs: inf_solve's log plus F_before, F_after, applied, reason.  ValueError for bad settings before
    any device work."""
    from .. import influence
    uid, iid, r = _rating_triple(train_data)
    refuse_nmf(model, 'newton_unlearn')
    l2, damping = newton_unlearn_check('mf', 'mse', l2, batch, lam, damping, curvature, steps, iters, tol, len(uid))
    W_u, W_v = model.user_mat.weight, model.item_mat.weight
    n_user, n_item = int(W_u.shape[0]), int(W_v.shape[0])
    free_u, free_i = influence.check_scope(scope, n_user, n_item)
    if len(uid) == 0:
        raise ValueError('newton_unlearn needs at least one remaining rating')
    U, V, d = padded_tables(model)
    k, dev = int(W_u.shape[1]), U.device
    if U.data_ptr() == W_u.data_ptr():
        U = U.clone()
    if V.data_ptr() == W_v.data_ptr():
        V = V.clone()
    graph = engine.GcnGraph(uid, iid, r, n_user, n_item, device=dev)
    g = graph.host
    has_u, has_i = np.diff(g.off_u) > 0, np.diff(g.off_i) > 0
    active = (has_u & free_u, has_i & free_i)
    act = engine._inf_active(graph, active)
    au, ai = act[0].bool(), act[1].bool()
    U[torch.from_numpy(~has_u).to(dev)] = 0.0
    V[torch.from_numpy(~has_i).to(dev)] = 0.0

    def objective(U, V, e):
        parts = engine.inf_objective(graph, U, V, l2, e).cpu().numpy()          # the one read of a step
        return float(parts[0] + l2 * parts[1])

    e = engine.inf_coef(graph, U, V)
    F = objective(U, V, e)
    logs = []
    for _ in range(steps):
        gU, gV = engine.inf_grad(graph, U, V, l2, act, e)
        xU, xV, log = engine.inf_solve(graph, U, V, -gU, -gV, l2, damping, curvature, act, e, iters, tol)
        log['F_before'] = F
        if log['status'] == influence.NON_POSITIVE:
            log.update(applied=False, reason='non-positive curvature met by the solve', F_after=F)
            logs.append(log)
            break
        U1, V1 = U.clone(), V.clone()
        U1[au], V1[ai] = (U.double() + xU).float()[au], (V.double() + xV).float()[ai]
        e1 = engine.inf_coef(graph, U1, V1)
        F1 = objective(U1, V1, e1)
        if not F1 < F:
            log.update(applied=False, reason='the step did not reduce the objective', F_after=F1)
            logs.append(log)
            break
        U, V, e, F = U1, V1, e1, F1
        log.update(applied=True, reason='', F_after=F1)
        logs.append(log)
    with torch.no_grad():
        W_u[:, :k] = U[:, :k]
        W_v[:, :k] = V[:, :k]
    return logs
