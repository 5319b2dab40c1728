"""The stateless C-ABI entry points as PyTorch custom ops (`torch.ops.ultrare.*`).

BASELINE.json's north_star words the boundary as "HIP kernels exposed to Python as PyTorch-ROCm custom ops"; the
boundary of record is the C ABI (include/ultrare_hip.h, bound with ctypes in _native.py) and these ops are thin
calls into the same library: they take and return torch tensors, run on the current HIP stream, and have no CPU
implementation (a CPU tensor is an error, not a fallback).  The training job (ure_job_*) is stateful -- a handle
to resident shards -- and stays behind engine.TrainJob.

    torch.ops.ultrare.mf_score(U, V, uid, iid)          utils.py:42-43    row-wise dot of gathered rows
    torch.ops.ultrare.ot_cost(X, C)                     utils.py:637      [k, n] squared distances, numpy's fp32 order
    torch.ops.ultrare.ot_cost_mfma(X, C)                (same, |x|^2 - 2 x.c + |c|^2 on the matrix cores; cross-check only)
    torch.ops.ultrare.ot_centroids(X, label, k)         utils.py:648      cluster means, numpy's fp32 order
    torch.ops.ultrare.merge_rows(dst, src, rows)        sisa.py:55-56     dst[rows] = src[rows]  (in place)
    torch.ops.ultrare.recommend_topk(Us, Vs, users, excl_off, excl_items, k)
                                                        (new)             full-catalogue top-k of the ensemble mean
    torch.ops.ultrare.rank_pairs(Us, Vs, users, tgt_off, tgt_items, excl_off, excl_items)
                                                        (new)             exact full-catalogue rank of each target pair
    torch.ops.ultrare.pair_knn(X, query, n_nb, metric)  utils.py:422-455  the n_nb nearest users of each query row, D streamed
    torch.ops.ultrare.csr_pair_knn(row_off, col, val, n_item, query, n_nb, metric)
                                                        utils.py:422-455  the same from the rows of a device CSR, bit for bit
    torch.ops.ultrare.ot_sinkhorn(dist, reg, num_iter_max, stop_thr)
                                                        (new)             log-domain Sinkhorn on a [k, n] cost matrix ->
                                                                          (label, u, v, err, iters)
    torch.ops.ultrare.combine_stats(Us, Vs, uid, iid, rating, link, w)
                                                        (new)             the combiner fit's float64 stats vector of a pair set
    torch.ops.ultrare.score_weighted(Us, Vs, uid, iid, rating, link, W, group_of_user)
                                                        (new)             (pred, sse partials) with fitted weight rows
    torch.ops.ultrare.ridge_rows(F, off, idx, val, k, l2, l2_n)
                                                        (new)             the ridge solution of every CSR segment against F
    torch.ops.ultrare.gram(F, k)                        (new)             the packed upper triangle (float64) of F[:, :k]^T F[:, :k]
    torch.ops.ultrare.wridge_rows(F, off, idx, wg, wb, G0, k, l2, l2_n)
                                                        (new)             ridge_rows with a confidence per entry and a Gram matrix
                                                                          added to every system (ultrare_amd/wmf.py)
    torch.ops.ultrare.csr_cost(row_off, col, val, Ct, k)
                                                        (new)             [k, n] squared distances of CSR rows to the
                                                                          centroids held transposed in Ct [n_item, ldc]
    torch.ops.ultrare.csr_centroids(col_off, row, val, label, k)
                                                        (new)             (Ct [n_item, k], counts [k]) from the CSC
    torch.ops.ultrare.csr_kmeans_cost(row_off, col, val, Ct, k)
                                                        utils.py:373-375  [n, k] k-means distances of CSR rows, scipy's fp32 order
    torch.ops.ultrare.csr_kmeans_centroids(col_off, row, val, label, k)
                                                        utils.py:402-403  (Ct [n_item, k], counts [k]): scipy's sparse mean from the CSC
    torch.ops.ultrare.balanced_fill(dist, capacity)     utils.py:377-396  (label [n], rounds [1] on the host) of a device [n, k] matrix:
                                                                          argmin (capacity <= 0) or the balanced greedy fill
    torch.ops.ultrare.mmd_grad(X, rows, n1, kernel_mul, kernel_num, fix_sigma)
                                                        utils.py:223-267  (block sums [4], grad [m, d], bandwidth) of the MMD
                                                                          loss on the rows `rows` of X, the first n1 the source
    torch.ops.ultrare.u2u_grad(X, rows, n1)             utils.py:75-78    (value, grad [m, d]) of trace(U^T Lap U), S - T bipartite
    torch.ops.ultrare.gcn_propagate(off, idx, s_src, s_dst, X, add)
                                                        (new)             one LightGCN propagation over a device CSR / CSC:
                                                                          out[r] = [add[r] +] s_dst[r] sum_j s_src[j] X[j]
    torch.ops.ultrare.attr_select(masks, group, steps, step, cap1, cap2)
                                                        (new)             (rows, counts): a step's users of two attribute groups, an
                                                                          ordered compaction on the device (ultrare_amd/attr_train.py)
    torch.ops.ultrare.bpr_negatives(off_d, col_d, row_u, pos, n_item, key, epoch)
                                                        (new)             neg [nnz]: one epoch's BPR negatives, uniform over the
                                                                          items a CSR entry's user has none of (ultrare_amd/bpr.py)
    torch.ops.ultrare.inf_matvec(off_u, col, row_u, off_i, row, to_csr, rating, U, V, P, Q, l2, damping, full)
                                                        (new)             (HU, HV) float64: the product of the MSE objective's
                                                                          Hessian (full) or Gauss-Newton matrix, plus 2 damping I,
                                                                          with a float64 direction (ultrare_amd/influence.py)
    torch.ops.ultrare.nmf_score(U, V, dense, k, layers, uid, iid)
                                                        (new)             the NeuMF forward of one model (ultrare_amd/nmf.py: U, V
                                                                          [rows, k + layers[0] / 2], dense the layers and the head)
    torch.ops.ultrare.nmf_recommend_topk(Us, Vs, denses, k, layers, users, excl_off, excl_items, top_k)
                                                        (new)             recommend_topk under a NeuMF ensemble of one stack
    torch.ops.ultrare.nmf_rank_pairs(Us, Vs, denses, k, layers, users, tgt_off, tgt_items, excl_off, excl_items)
                                                        (new)             rank_pairs under a NeuMF ensemble of one stack
    torch.ops.ultrare.recommend_topk_weighted(Us, Vs, users, excl_off, excl_items, k, link, W, group_of_user)
                                                        (new)             recommend_topk under the learned shard combiner's scores
    torch.ops.ultrare.rank_pairs_weighted(Us, Vs, users, tgt_off, tgt_items, excl_off, excl_items, link, W, group_of_user)
                                                        (new)             rank_pairs under the learned shard combiner's scores
"""
import ctypes
from typing import List, Optional, Tuple

import torch

from . import _native as nv
from . import engine


def _dev(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise nv.NativeError('ultrare ops run on the HIP device only (no CPU fallback)')


@torch.library.custom_op('ultrare::mf_score', mutates_args=())
def mf_score(U: torch.Tensor, V: torch.Tensor, uid: torch.Tensor, iid: torch.Tensor) -> torch.Tensor:
    _dev(U, V, uid, iid)
    d = engine.pad_dim(U.shape[1])
    assert U.shape[1] == d and V.shape[1] == d and U.is_contiguous() and V.is_contiguous(), 'tables must have the padded width'
    uid, iid = uid.to(torch.int32).contiguous(), iid.to(torch.int32).contiguous()
    pred = torch.empty(uid.numel(), dtype=torch.float32, device=U.device)
    Up, Vp = (ctypes.c_void_p * 1)(U.data_ptr()), (ctypes.c_void_p * 1)(V.data_ptr())
    nv.check(nv.lib().ure_score(Up, Vp, 1, 1, 1, 1, nv.ptr(uid), nv.ptr(iid), None, uid.numel(), d, nv.ptr(pred), None, nv.stream_handle()),
             'ure_score')
    return pred


@mf_score.register_fake
def _(U, V, uid, iid):
    return U.new_empty(uid.numel())


def _cost(fn, X, C):
    _dev(X, C)
    X, C = X.float().contiguous(), C.float().contiguous()
    dist = torch.empty(C.shape[0], X.shape[0], dtype=torch.float32, device=X.device)
    nv.check(fn(nv.ptr(X), nv.ptr(C), X.shape[0], C.shape[0], X.shape[1], nv.ptr(dist), nv.stream_handle()), 'ure_ot_cost')
    return dist


@torch.library.custom_op('ultrare::ot_cost', mutates_args=())
def ot_cost(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    return _cost(nv.lib().ure_ot_cost, X, C)


@torch.library.custom_op('ultrare::ot_cost_mfma', mutates_args=())
def ot_cost_mfma(X: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    return _cost(nv.lib().ure_ot_cost_mfma, X, C)


@ot_cost.register_fake
def _(X, C):
    return X.new_empty(C.shape[0], X.shape[0])


@ot_cost_mfma.register_fake
def _(X, C):
    return X.new_empty(C.shape[0], X.shape[0])


@torch.library.custom_op('ultrare::ot_centroids', mutates_args=())
def ot_centroids(X: torch.Tensor, label: torch.Tensor, k: int) -> torch.Tensor:
    _dev(X, label)
    X, label = X.float().contiguous(), label.to(torch.int32).contiguous()
    C = torch.empty(k, X.shape[1], dtype=torch.float32, device=X.device)
    counts = torch.empty(k, dtype=torch.int32, device=X.device)
    nv.check(nv.lib().ure_ot_centroids(nv.ptr(X), nv.ptr(label), X.shape[0], k, X.shape[1], nv.ptr(C), nv.ptr(counts), nv.stream_handle()),
             'ure_ot_centroids')
    return C


@ot_centroids.register_fake
def _(X, label, k):
    return X.new_empty(k, X.shape[1])


@torch.library.custom_op('ultrare::merge_rows', mutates_args=('dst',))
def merge_rows(dst: torch.Tensor, src: torch.Tensor, rows: torch.Tensor) -> None:
    _dev(dst, src, rows)
    assert dst.is_contiguous() and src.is_contiguous() and dst.shape == src.shape
    rows = rows.to(torch.int64).contiguous()
    nv.check(nv.lib().ure_merge_rows(nv.ptr(dst), nv.ptr(src), nv.ptr(rows), rows.numel(), dst.shape[1], nv.stream_handle()), 'ure_merge_rows')


@torch.library.custom_op('ultrare::recommend_topk', mutates_args=())
def recommend_topk(Us: List[torch.Tensor], Vs: List[torch.Tensor], users: torch.Tensor, excl_off: Optional[torch.Tensor],
                   excl_items: Optional[torch.Tensor], k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _dev(*Us, *Vs, users, *[t for t in (excl_off, excl_items) if t is not None])
    assert len(Us) == len(Vs) and (excl_off is None) == (excl_items is None)
    excl = None if excl_off is None else (excl_off.cpu().numpy(), excl_items.cpu().numpy())
    return engine.recommend(list(zip(Us, Vs)), Us[0].shape[1], users, k, excl)


@recommend_topk.register_fake
def _(Us, Vs, users, excl_off, excl_items, k):
    return Us[0].new_empty(users.numel(), k), Us[0].new_empty(users.numel(), k, dtype=torch.int64)


@torch.library.custom_op('ultrare::rank_pairs', mutates_args=())
def rank_pairs(Us: List[torch.Tensor], Vs: List[torch.Tensor], users: torch.Tensor, tgt_off: torch.Tensor, tgt_items: torch.Tensor,
               excl_off: Optional[torch.Tensor], excl_items: Optional[torch.Tensor]) -> torch.Tensor:
    _dev(*Us, *Vs, users, tgt_off, tgt_items, *[t for t in (excl_off, excl_items) if t is not None])
    assert len(Us) == len(Vs) and (excl_off is None) == (excl_items is None)
    excl = None if excl_off is None else (excl_off.cpu().numpy(), excl_items.cpu().numpy())
    return engine.rank_pairs(list(zip(Us, Vs)), Us[0].shape[1], users, (tgt_off.cpu().numpy(), tgt_items.cpu().numpy()), excl)


@rank_pairs.register_fake
def _(Us, Vs, users, tgt_off, tgt_items, excl_off, excl_items):
    return Us[0].new_empty(tgt_items.numel(), dtype=torch.int32)


def _weights(link, W, group_of_user):
    return link, W.to(torch.float64).contiguous(), None if group_of_user is None else group_of_user.to(torch.int32).contiguous()


@torch.library.custom_op('ultrare::recommend_topk_weighted', mutates_args=())
def recommend_topk_weighted(Us: List[torch.Tensor], Vs: List[torch.Tensor], users: torch.Tensor, excl_off: Optional[torch.Tensor],
                            excl_items: Optional[torch.Tensor], k: int, link: int, W: torch.Tensor,
                            group_of_user: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """engine.recommend(..., weights=(link, W, group_of_user)): (scores [n, k], items [n, k] int64) under score_weighted's scores."""
    _dev(*Us, *Vs, users, W, *[t for t in (excl_off, excl_items, group_of_user) if t is not None])
    assert len(Us) == len(Vs) and (excl_off is None) == (excl_items is None)
    excl = None if excl_off is None else (excl_off.cpu().numpy(), excl_items.cpu().numpy())
    return engine.recommend(list(zip(Us, Vs)), Us[0].shape[1], users, k, excl, weights=_weights(link, W, group_of_user))


@recommend_topk_weighted.register_fake
def _(Us, Vs, users, excl_off, excl_items, k, link, W, group_of_user):
    return Us[0].new_empty(users.numel(), k), Us[0].new_empty(users.numel(), k, dtype=torch.int64)


@torch.library.custom_op('ultrare::rank_pairs_weighted', mutates_args=())
def rank_pairs_weighted(Us: List[torch.Tensor], Vs: List[torch.Tensor], users: torch.Tensor, tgt_off: torch.Tensor, tgt_items: torch.Tensor,
                        excl_off: Optional[torch.Tensor], excl_items: Optional[torch.Tensor], link: int, W: torch.Tensor,
                        group_of_user: Optional[torch.Tensor]) -> torch.Tensor:
    """engine.rank_pairs(..., weights=(link, W, group_of_user)): ranks int32 [len(tgt_items)] under score_weighted's scores."""
    _dev(*Us, *Vs, users, tgt_off, tgt_items, W, *[t for t in (excl_off, excl_items, group_of_user) if t is not None])
    assert len(Us) == len(Vs) and (excl_off is None) == (excl_items is None)
    excl = None if excl_off is None else (excl_off.cpu().numpy(), excl_items.cpu().numpy())
    return engine.rank_pairs(list(zip(Us, Vs)), Us[0].shape[1], users, (tgt_off.cpu().numpy(), tgt_items.cpu().numpy()), excl,
                             weights=_weights(link, W, group_of_user))


@rank_pairs_weighted.register_fake
def _(Us, Vs, users, tgt_off, tgt_items, excl_off, excl_items, link, W, group_of_user):
    return Us[0].new_empty(tgt_items.numel(), dtype=torch.int32)


@torch.library.custom_op('ultrare::pair_knn', mutates_args=())
def pair_knn(X: torch.Tensor, query: Optional[torch.Tensor], n_nb: int, metric: str) -> Tuple[torch.Tensor, torch.Tensor]:
    _dev(X, *([query] if query is not None else []))
    return engine.pair_knn(X, n_nb, None if metric == 'given' else metric, query)


@pair_knn.register_fake
def _(X, query, n_nb, metric):
    n_q = X.shape[0] if query is None else query.numel()
    return X.new_empty(n_q, n_nb), X.new_empty(n_q, n_nb, dtype=torch.int64)


@torch.library.custom_op('ultrare::csr_pair_knn', mutates_args=())
def csr_pair_knn(row_off: torch.Tensor, col: torch.Tensor, val: torch.Tensor, n_item: int, query: Optional[torch.Tensor], n_nb: int,
                 metric: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """pair_knn on the rows of a device CSR of n_item columns (ascending columns inside a row, no repeats; the ids are checked
    against n_item, the order is the caller's word)."""
    _dev(row_off, col, val, *([query] if query is not None else []))
    row_off, col, val = _csr_half(row_off, col, val)
    if n_item < 1 or int(col.max()) >= n_item or int(col.min()) < 0:
        raise ValueError(f'column indices outside [0, {n_item})')
    return engine.pair_knn(engine.CsrSet.from_device(row_off.numel() - 1, n_item, row_off, col, val), n_nb, metric, query)


@csr_pair_knn.register_fake
def _(row_off, col, val, n_item, query, n_nb, metric):
    n_q = row_off.numel() - 1 if query is None else query.numel()
    return val.new_empty(n_q, n_nb), val.new_empty(n_q, n_nb, dtype=torch.int64)


@torch.library.custom_op('ultrare::ot_sinkhorn', mutates_args=())
def ot_sinkhorn(dist: torch.Tensor, reg: float, num_iter_max: int, stop_thr: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, float, int]:
    _dev(dist)
    r = engine.ot_sinkhorn(dist, reg, num_iter_max, stop_thr)
    return r['label'], r['u'], r['v'], r['err'], r['iters']


@ot_sinkhorn.register_fake
def _(dist, reg, num_iter_max, stop_thr):
    k, n = dist.shape
    return (dist.new_empty(n, dtype=torch.int32), dist.new_empty(n, dtype=torch.float64), dist.new_empty(k, dtype=torch.float64), 0.0, 0)


def _pairs(uid, iid, rating):
    return uid.to(torch.int32).contiguous(), iid.to(torch.int32).contiguous(), rating.to(torch.float32).contiguous()


@torch.library.custom_op('ultrare::combine_stats', mutates_args=())
def combine_stats(Us: List[torch.Tensor], Vs: List[torch.Tensor], uid: torch.Tensor, iid: torch.Tensor, rating: torch.Tensor, link: int,
                  w: torch.Tensor) -> torch.Tensor:
    _dev(*Us, *Vs, uid, iid, rating, w)
    assert len(Us) == len(Vs)
    pairs = engine.PairSet.from_device(*_pairs(uid, iid, rating))
    return engine.combine_stats(list(zip(Us, Vs)), Us[0].shape[1], pairs, link, w.to(torch.float64).contiguous(), as_tensor=True)


@combine_stats.register_fake
def _(Us, Vs, uid, iid, rating, link, w):
    S = len(Us)
    return w.new_empty(2 + (S + 1) + (S + 1) * (S + 2) // 2, dtype=torch.float64)


@torch.library.custom_op('ultrare::score_weighted', mutates_args=())
def score_weighted(Us: List[torch.Tensor], Vs: List[torch.Tensor], uid: torch.Tensor, iid: torch.Tensor, rating: torch.Tensor, link: int,
                   W: torch.Tensor, group_of_user: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    _dev(*Us, *Vs, uid, iid, rating, W, *([group_of_user] if group_of_user is not None else []))
    assert len(Us) == len(Vs)
    uid, iid, rating = _pairs(uid, iid, rating)
    gou = None if group_of_user is None else group_of_user.to(torch.int32).contiguous()
    return engine.score_weighted(list(zip(Us, Vs)), Us[0].shape[1], uid, iid, rating, link, W.to(torch.float64).contiguous(), gou)


@score_weighted.register_fake
def _(Us, Vs, uid, iid, rating, link, W, group_of_user):
    return Us[0].new_empty(uid.numel()), Us[0].new_empty(engine.SCORE_PARTIALS, dtype=torch.float64)


@torch.library.custom_op('ultrare::ridge_rows', mutates_args=())
def ridge_rows(F: torch.Tensor, off: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, k: int, l2: float, l2_n: float) -> torch.Tensor:
    _dev(F, off, idx, val)
    segs = engine.SegmentSet.from_device(off.to(torch.int64), idx.to(torch.int32), val.to(torch.float32))
    return engine.ridge_rows(F, F.shape[1], k, segs, l2, l2_n)


@ridge_rows.register_fake
def _(F, off, idx, val, k, l2, l2_n):
    return F.new_empty(off.numel() - 1, F.shape[1])


@torch.library.custom_op('ultrare::gram', mutates_args=())
def gram(F: torch.Tensor, k: int) -> torch.Tensor:
    _dev(F)
    return engine.gram(F, F.shape[1], k)


@gram.register_fake
def _(F, k):
    return F.new_empty(k * (k + 1) // 2, dtype=torch.float64)


@torch.library.custom_op('ultrare::wridge_rows', mutates_args=())
def wridge_rows(F: torch.Tensor, off: torch.Tensor, idx: torch.Tensor, wg: torch.Tensor, wb: torch.Tensor, G0: Optional[torch.Tensor], k: int,
                l2: float, l2_n: float) -> torch.Tensor:
    _dev(F, off, idx, wg, wb, *([G0] if G0 is not None else []))
    wg, wb = wg.to(torch.float32).contiguous(), wb.to(torch.float32).contiguous()
    segs = engine.SegmentSet.from_device(off.to(torch.int64), idx.to(torch.int32), wb)          # (the set's ratings are not read)
    return engine.wridge_rows(F, F.shape[1], k, segs, wg, wb, None if G0 is None else G0.to(torch.float64).contiguous(), l2, l2_n)


@wridge_rows.register_fake
def _(F, off, idx, wg, wb, G0, k, l2, l2_n):
    return F.new_empty(off.numel() - 1, F.shape[1])


def _csr_half(off, idx, val):
    if not (off.dtype == torch.int64 and idx.dtype == torch.int32 and val.dtype == torch.float32):
        raise ValueError('a CSR half is (int64 offsets, int32 indices, float32 values)')
    if off.dim() != 1 or off.numel() < 2 or idx.numel() != val.numel() or idx.numel() < 1:
        raise ValueError('offsets must hold n + 1 values and indices as many entries as values (at least one)')
    return off.contiguous(), idx.contiguous(), val.contiguous()


def _csr_rows(row_off, col, val, Ct, width='>= k'):
    """The CSR half of a cost op as a CsrSet of Ct's item count, its column indices checked against it."""
    _dev(row_off, col, val, Ct)
    row_off, col, val = _csr_half(row_off, col, val)
    if not (Ct.dtype == torch.float32 and Ct.dim() == 2 and Ct.is_contiguous()):
        raise ValueError(f'Ct must be a contiguous float32 [n_item, {width}] tensor, not {tuple(Ct.shape)} {Ct.dtype}')
    if int(col.max()) >= Ct.shape[0] or int(col.min()) < 0:
        raise ValueError(f'column indices outside the {Ct.shape[0]} rows of Ct')
    return engine.CsrSet.from_device(row_off.numel() - 1, Ct.shape[0], row_off, col, val)


def _csr_cols(col_off, row, val, label, k):
    """The CSC half of a centroid op as a CsrSet of as many users as labels, and the labels as int32 [n] in [0, k) (the engine
    call reads the label range back a second time)."""
    _dev(col_off, row, val, label)
    col_off, row, val = _csr_half(col_off, row, val)
    label = label.to(torch.int32).reshape(-1)
    n = label.numel()
    if int(row.max()) >= n or int(row.min()) < 0:
        raise ValueError(f'row indices outside the {n} labels')
    if int(label.min()) < 0 or int(label.max()) >= k:
        raise ValueError(f'label must hold values in [0, {k})')
    return engine.CsrSet.from_device(n, col_off.numel() - 1, col_off=col_off, row=row, cval=val), label


@torch.library.custom_op('ultrare::csr_cost', mutates_args=())
def csr_cost(row_off: torch.Tensor, col: torch.Tensor, val: torch.Tensor, Ct: torch.Tensor, k: int) -> torch.Tensor:
    return engine.csr_cost(_csr_rows(row_off, col, val, Ct), Ct, k)


@csr_cost.register_fake
def _(row_off, col, val, Ct, k):
    return Ct.new_empty(k, row_off.numel() - 1)


@torch.library.custom_op('ultrare::csr_centroids', mutates_args=())
def csr_centroids(col_off: torch.Tensor, row: torch.Tensor, val: torch.Tensor, label: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return engine.csr_centroids(*_csr_cols(col_off, row, val, label, k), k)


@csr_centroids.register_fake
def _(col_off, row, val, label, k):
    return val.new_empty(col_off.numel() - 1, k), val.new_empty(k, dtype=torch.int32)


@torch.library.custom_op('ultrare::csr_kmeans_cost', mutates_args=())
def csr_kmeans_cost(row_off: torch.Tensor, col: torch.Tensor, val: torch.Tensor, Ct: torch.Tensor, k: int) -> torch.Tensor:
    return engine.csr_kmeans_cost(_csr_rows(row_off, col, val, Ct, 'k'), Ct, k)


@csr_kmeans_cost.register_fake
def _(row_off, col, val, Ct, k):
    return Ct.new_empty(row_off.numel() - 1, k)


@torch.library.custom_op('ultrare::csr_kmeans_centroids', mutates_args=())
def csr_kmeans_centroids(col_off: torch.Tensor, row: torch.Tensor, val: torch.Tensor, label: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return engine.csr_kmeans_centroids(*_csr_cols(col_off, row, val, label, k), k)


@csr_kmeans_centroids.register_fake
def _(col_off, row, val, label, k):
    return val.new_empty(col_off.numel() - 1, k), val.new_empty(k, dtype=torch.int32)


@torch.library.custom_op('ultrare::balanced_fill', mutates_args=())
def balanced_fill(dist: torch.Tensor, capacity: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _dev(dist)
    label, rounds = engine.balanced_fill(dist, capacity)
    return label, torch.tensor([rounds], dtype=torch.int64)


@balanced_fill.register_fake
def _(dist, capacity):
    return dist.new_empty(dist.shape[0], dtype=torch.int32), torch.empty(1, dtype=torch.int64)


def _group_rows(X, rows, n1):
    ids = rows.cpu().numpy()
    return engine.GroupRows(ids[:n1], ids[n1:], X.shape[0], X.device)


@torch.library.custom_op('ultrare::mmd_grad', mutates_args=())
def mmd_grad(X: torch.Tensor, rows: torch.Tensor, n1: int, kernel_mul: float, kernel_num: int,
             fix_sigma: Optional[float]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    _dev(X, rows)
    groups = _group_rows(X, rows, n1)
    bw = engine.mmd_bandwidth(X, groups, fix_sigma)
    sums, grad = engine.mmd_loss_grad(X, groups, bw, kernel_mul, kernel_num)
    return sums, grad, bw


@mmd_grad.register_fake
def _(X, rows, n1, kernel_mul, kernel_num, fix_sigma):
    return X.new_empty(4, dtype=torch.float64), X.new_empty(rows.numel(), X.shape[1]), X.new_empty((), dtype=torch.float64)


@torch.library.custom_op('ultrare::u2u_grad', mutates_args=())
def u2u_grad(X: torch.Tensor, rows: torch.Tensor, n1: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _dev(X, rows)
    return engine.u2u_loss_grad(X, _group_rows(X, rows, n1))


@u2u_grad.register_fake
def _(X, rows, n1):
    return X.new_empty((), dtype=torch.float64), X.new_empty(rows.numel(), X.shape[1])


@torch.library.custom_op('ultrare::auc_counts', mutates_args=())
def auc_counts(scores: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """engine.auc_counts: (int64 [2] = pairs with s_p > s_n, pairs with s_p == s_n; int32 [1] = a selected score is NaN)."""
    _dev(scores, pos, neg)
    return engine.auc_counts(scores, pos, neg)


@auc_counts.register_fake
def _(scores, pos, neg):
    return scores.new_empty(2, dtype=torch.int64), scores.new_empty(1, dtype=torch.int32)


@torch.library.custom_op('ultrare::attack_scores', mutates_args=())
def attack_scores(X: torch.Tensor, rows: torch.Tensor, params: torch.Tensor, stats: torch.Tensor, hidden: int) -> torch.Tensor:
    """engine.attack_scores with one packed parameter set (float32 [P]) and its statistics (float32 [2, d]) given as tensors."""
    from . import attack
    _dev(X, rows, params, stats)
    d = int(X.shape[1]) if X.dim() == 2 else -1
    if params.dtype != torch.float32 or stats.dtype != torch.float32 or not 1 <= d <= attack.MAX_D or not 0 <= hidden <= attack.MAX_H or \
            tuple(params.shape) != (attack.n_params(d, hidden),) or tuple(stats.shape) != (2, d):
        raise ValueError(f'attack_scores: params float32 [P(d, hidden)] and stats float32 [2, d] are needed for X {tuple(X.shape)}, hidden = {hidden}')
    fit = engine.AttackFit(params=params.contiguous()[None], stats=stats.contiguous()[None], d=d, hidden=int(hidden), folds=1)
    return engine.attack_scores(fit, X, rows)


@attack_scores.register_fake
def _(X, rows, params, stats, hidden):
    return X.new_empty(rows.numel())


@torch.library.custom_op('ultrare::attack_input_grad', mutates_args=())
def attack_input_grad(X: torch.Tensor, rows: torch.Tensor, n1: int, fold_of: Optional[torch.Tensor], params: torch.Tensor, stats: torch.Tensor,
                      fw: torch.Tensor, hidden: int, target0: float, target1: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """engine.attack_input_grad with the probe given as tensors: params float32 [folds, P], stats float32 [folds, 2, d], fw float32
    [folds, 4], fold_of int32 [m] (None: set 0 serves every row) -> (grad float32 [m, d], p float32 [m])."""
    from . import attack
    _dev(X, rows, params, stats, fw, *([] if fold_of is None else [fold_of]))
    d = int(X.shape[1]) if X.dim() == 2 else -1
    folds = int(params.shape[0]) if params.dim() == 2 else -1
    if [params.dtype, stats.dtype, fw.dtype] != [torch.float32] * 3 or not 1 <= d <= attack.MAX_D or not 0 <= hidden <= attack.MAX_H or \
            not 1 <= folds <= attack.MAX_FOLDS or tuple(params.shape) != (folds, attack.n_params(d, hidden)) or tuple(stats.shape) != (folds, 2, d) or \
            tuple(fw.shape) != (folds, 4) or (fold_of is not None and (fold_of.dtype != torch.int32 or tuple(fold_of.shape) != (rows.numel(),))):
        raise ValueError(f'attack_input_grad: params float32 [folds, P(d, hidden)], stats float32 [folds, 2, d], fw float32 [folds, 4] and fold_of '
                         f'int32 [m] or None are needed for X {tuple(X.shape)}, hidden = {hidden}')
    fit = engine.AttackFit(params=params.contiguous(), stats=stats.contiguous(), fw=fw.contiguous(), d=d, hidden=int(hidden), folds=folds,
                           fold_of=None if fold_of is None else fold_of.contiguous())
    return engine.attack_input_grad(fit, X, _group_rows(X, rows, n1), (target0, target1))


@attack_input_grad.register_fake
def _(X, rows, n1, fold_of, params, stats, fw, hidden, target0, target1):
    return X.new_empty(rows.numel(), X.shape[1]), X.new_empty(rows.numel())


@torch.library.custom_op('ultrare::gcn_propagate', mutates_args=())
def gcn_propagate(off: torch.Tensor, idx: torch.Tensor, s_src: torch.Tensor, s_dst: torch.Tensor, X: torch.Tensor,
                  add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """engine.gcn_propagate on the halves of a graph that are on the device already: off int64 [n_dst + 1], idx int32 [nnz],
    s_src float32 [n_src], s_dst float32 [n_dst], X float32 [n_src, d] (the caller vouches for the index ranges)."""
    from . import lightgcn
    _dev(off, idx, s_src, s_dst, X, *([] if add is None else [add]))
    if [off.dtype, idx.dtype, s_src.dtype, s_dst.dtype, X.dtype] != [torch.int64, torch.int32, torch.float32, torch.float32, torch.float32]:
        raise ValueError('gcn_propagate takes (int64 offsets, int32 indices, float32 s_src, float32 s_dst, float32 X)')
    n_dst, n_src = off.numel() - 1, s_src.numel()
    if X.dim() != 2 or X.shape[0] != n_src or s_dst.numel() != n_dst or n_dst < 1 or idx.numel() < 1:
        raise ValueError(f'gcn_propagate: {n_dst} rows over {n_src} sources do not fit X {tuple(X.shape)} and s_dst [{s_dst.numel()}]')
    d = lightgcn.check_width(int(X.shape[1]))
    X = X.contiguous()
    if add is not None:
        engine._gcn_table(add, n_dst, d, 'add', X.device)
    out = torch.empty(n_dst, d, dtype=torch.float32, device=X.device)
    nv.check(nv.lib().ure_gcn_propagate(nv.ptr(off.contiguous()), nv.ptr(idx.contiguous()), n_dst, n_src, nv.ptr(s_src.contiguous()),
                                        nv.ptr(s_dst.contiguous()), nv.ptr(X), d, nv.ptr(add), None, nv.ptr(out), nv.stream_handle()),
             'ure_gcn_propagate')
    return out


@gcn_propagate.register_fake
def _(off, idx, s_src, s_dst, X, add=None):
    return X.new_empty(off.numel() - 1, X.shape[1])


@torch.library.custom_op('ultrare::attr_select', mutates_args=())
def attr_select(masks: torch.Tensor, group: torch.Tensor, steps: int, step: int, cap1: int, cap2: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """engine.attr_select: the rows of one step of in-training attribute unlearning from the per-user step masks
    (engine.attr_step_masks: int32 [n_user, ceil(steps / 32)]) and group int8 [n_user] -> (rows int32 [cap1 + cap2], counts int32 [2])."""
    _dev(masks, group)
    return engine.attr_select(masks.contiguous(), group.contiguous(), steps, step, cap1, cap2)


@attr_select.register_fake
def _(masks, group, steps, step, cap1, cap2):
    return masks.new_empty(cap1 + cap2, dtype=torch.int32), masks.new_empty(2, dtype=torch.int32)


@torch.library.custom_op('ultrare::bpr_negatives', mutates_args=())
def bpr_negatives(off_d: torch.Tensor, col_d: torch.Tensor, row_u: torch.Tensor, pos: torch.Tensor, n_item: int, key: int, epoch: int) -> torch.Tensor:
    """engine.bpr_negatives on arrays that are on the device already: off_d int64 [n_user + 1] and col_d int32 (the users' distinct
    items, bpr.distinct_csr), row_u and pos int32 [nnz] (a CSR entry's user and file position).  key is taken modulo 2^64 (an
    operator's int is signed: a key of 2^63 or more is passed as key - 2^64).  -> neg int32 [nnz]."""
    _dev(off_d, col_d, row_u, pos)
    if [off_d.dtype, col_d.dtype, row_u.dtype, pos.dtype] != [torch.int64, torch.int32, torch.int32, torch.int32]:
        raise ValueError('bpr_negatives takes (int64 offsets, int32 distinct items, int32 users, int32 file positions)')
    n_user, nnz = off_d.numel() - 1, row_u.numel()
    if n_user < 1 or nnz < 1 or pos.numel() != nnz or not 1 <= col_d.numel() <= nnz or n_item < 1 or not 0 <= epoch < 2 ** 31:
        raise ValueError(f'bpr_negatives: {nnz} entries of {n_user} users over {n_item} items do not fit pos [{pos.numel()}], col_d [{col_d.numel()}]')
    neg = torch.empty(nnz, dtype=torch.int32, device=row_u.device)
    nv.check(nv.lib().ure_bpr_sample(nv.ptr(off_d.contiguous()), nv.ptr(col_d.contiguous()), col_d.numel(), nv.ptr(row_u.contiguous()),
                                     nv.ptr(pos.contiguous()), nnz, n_user, int(n_item), int(key) & 0xFFFFFFFFFFFFFFFF, int(epoch), nv.ptr(neg),
                                     nv.stream_handle()), 'ure_bpr_sample')
    return neg


@bpr_negatives.register_fake
def _(off_d, col_d, row_u, pos, n_item, key, epoch):
    return row_u.new_empty(row_u.numel())


@torch.library.custom_op('ultrare::inf_matvec', mutates_args=())
def inf_matvec(off_u: torch.Tensor, col: torch.Tensor, row_u: torch.Tensor, off_i: torch.Tensor, row: torch.Tensor, to_csr: torch.Tensor,
               rating: torch.Tensor, U: torch.Tensor, V: torch.Tensor, P: torch.Tensor, Q: torch.Tensor, l2: float, damping: float = 0.0,
               full: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """engine.inf_matvec on the halves of a graph that are on the device already (the arrays of lightgcn.Graph: off_u, off_i int64;
    col, row_u, row, to_csr int32 [nnz]; rating float32 [nnz] in CSR order; the caller vouches for the index ranges), float32 tables
    U, V and a float64 direction P, Q.  full: the Hessian, else the Gauss-Newton matrix."""
    import types
    _dev(off_u, col, row_u, off_i, row, to_csr, rating, U, V, P, Q)
    if [off_u.dtype, col.dtype, row_u.dtype, off_i.dtype, row.dtype, to_csr.dtype, rating.dtype] != [torch.int64, torch.int32, torch.int32, torch.int64,
                                                                                                      torch.int32, torch.int32, torch.float32]:
        raise ValueError('inf_matvec takes (int64 off_u, int32 col, int32 row_u, int64 off_i, int32 row, int32 to_csr, float32 rating)')
    nnz, n_user, n_item = col.numel(), off_u.numel() - 1, off_i.numel() - 1
    if nnz < 1 or n_user < 1 or n_item < 1 or [row_u.numel(), row.numel(), to_csr.numel(), rating.numel()] != [nnz] * 4:
        raise ValueError(f'inf_matvec: {nnz} entries of {n_user} users and {n_item} items do not fit the index arrays')
    c = lambda t: t.contiguous()
    g = types.SimpleNamespace(off_u=c(off_u), col=c(col), row_u=c(row_u), off_i=c(off_i), row=c(row), to_csr=c(to_csr), rating=c(rating), nnz=nnz, N=nnz,
                              n_user=n_user, n_item=n_item, device=U.device)
    return engine.inf_matvec(g, U, V, P, Q, l2, damping, 'full' if full else 'gn')


@inf_matvec.register_fake
def _(off_u, col, row_u, off_i, row, to_csr, rating, U, V, P, Q, l2, damping=0.0, full=True):
    return torch.empty_like(P), torch.empty_like(Q)


@torch.library.custom_op('ultrare::nmf_score', mutates_args=())
def nmf_score(U: torch.Tensor, V: torch.Tensor, dense: torch.Tensor, k: int, layers: List[int], uid: torch.Tensor, iid: torch.Tensor) -> torch.Tensor:
    """engine.nmf_score of one model at the pairs (uid, iid): the bytes the training forward gives (nmf.forward_ref in float32)."""
    from . import nmf
    nmf.check_layers(k, list(layers))                        # (a bad stack is a ValueError before anything else)
    _dev(U, V, dense, uid, iid)
    return engine.nmf_score(U.contiguous(), V.contiguous(), dense.contiguous(), k, list(layers), uid.to(torch.int32).contiguous(),
                            iid.to(torch.int32).contiguous())


@nmf_score.register_fake
def _(U, V, dense, k, layers, uid, iid):
    return U.new_empty(uid.numel())


@torch.library.custom_op('ultrare::nmf_recommend_topk', mutates_args=())
def nmf_recommend_topk(Us: List[torch.Tensor], Vs: List[torch.Tensor], denses: List[torch.Tensor], k: int, layers: List[int], users: torch.Tensor,
                       excl_off: Optional[torch.Tensor], excl_items: Optional[torch.Tensor], top_k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """engine.nmf_recommend of the ensemble [(Us[m], Vs[m], denses[m])] of one (k, layers): (scores [n, top_k], items [n, top_k] int64)."""
    from . import nmf
    nmf.check_layers(k, list(layers))                        # (a bad stack is a ValueError before anything else)
    _dev(*Us, *Vs, *denses, users, *[t for t in (excl_off, excl_items) if t is not None])
    assert len(Us) == len(Vs) == len(denses) and (excl_off is None) == (excl_items is None)
    excl = None if excl_off is None else (excl_off.cpu().numpy(), excl_items.cpu().numpy())
    return engine.nmf_recommend([(U.contiguous(), V.contiguous(), d.contiguous()) for U, V, d in zip(Us, Vs, denses)], k, list(layers), users, top_k, excl)


@nmf_recommend_topk.register_fake
def _(Us, Vs, denses, k, layers, users, excl_off, excl_items, top_k):
    return Us[0].new_empty(users.numel(), top_k), Us[0].new_empty(users.numel(), top_k, dtype=torch.int64)


@torch.library.custom_op('ultrare::nmf_rank_pairs', mutates_args=())
def nmf_rank_pairs(Us: List[torch.Tensor], Vs: List[torch.Tensor], denses: List[torch.Tensor], k: int, layers: List[int], users: torch.Tensor,
                   tgt_off: torch.Tensor, tgt_items: torch.Tensor, excl_off: Optional[torch.Tensor], excl_items: Optional[torch.Tensor]) -> torch.Tensor:
    """engine.nmf_rank_pairs of the ensemble [(Us[m], Vs[m], denses[m])] of one (k, layers): ranks int32 [len(tgt_items)]."""
    from . import nmf
    nmf.check_layers(k, list(layers))
    _dev(*Us, *Vs, *denses, users, tgt_off, tgt_items, *[t for t in (excl_off, excl_items) if t is not None])
    assert len(Us) == len(Vs) == len(denses) and (excl_off is None) == (excl_items is None)
    excl = None if excl_off is None else (excl_off.cpu().numpy(), excl_items.cpu().numpy())
    return engine.nmf_rank_pairs([(U.contiguous(), V.contiguous(), d.contiguous()) for U, V, d in zip(Us, Vs, denses)], k, list(layers), users,
                                 (tgt_off.cpu().numpy(), tgt_items.cpu().numpy()), excl)


@nmf_rank_pairs.register_fake
def _(Us, Vs, denses, k, layers, users, tgt_off, tgt_items, excl_off, excl_items):
    return Us[0].new_empty(tgt_items.numel(), dtype=torch.int32)
