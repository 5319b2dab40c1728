"""The batched ridge solves (csrc/mf_ridge.hip) measured on the GPU.  One JSON line.

    python tools/exp_ridge.py [--shapes ml1m,cfg3] [--reps 7] [--epochs 50] [--no-sisa]

Per shape (ml1m: 6,040 user and 3,416 item segments over the 896,914 synthetic training pairs, k = 32; cfg3: 162,000 and
60,000 segments over 22.5 M pairs, k = 128; N(0, 1) tables) and side, device time by events on the stream, medians of --reps
launches after two warm-up launches, the spread (min, max) beside every median, and the peak extra device memory of one call:
  ridge_ms          one ure_ridge_rows pass (longest-first order), and index_order_ms the same without the order
  composition_ms    the torch composition it replaces: the segments longest first in chunks padded to the chunk's longest,
                    Gram by float64 bmm, torch.linalg.cholesky_ex and cholesky_solve, each chunk at most --chunk-mb of
                    gathered rows, and the largest difference between the two results relative to the row's largest entry
and, unless --no-sisa, on the ml-1m-shaped synthetic SISA of tools/exp_combine.py (5 shards, k = 32, --epochs epochs, parallel):
  2 % of the users are deleted with Sisa.unlearn and folded back in with utils.trainer_l2 under both `against` modes; their
  test (rmse, ndcg, hr@10) as trained members and as folded-in users, the relative distance between the folded and the trained
  rows, and the host time of the fold_in and forget_folded calls (with a synchronise).
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ultrare_amd import _native as nv  # noqa: E402
from ultrare_amd import engine, synth  # noqa: E402

SHAPES = {'ml1m': (synth.ML1M, 32), 'cfg3': (synth.ML25M, 128)}


def event_ms(fn, reps, warmup=2):
    """-> {'median', 'min', 'max'} of the device time of fn() in ms, and the peak extra device memory of one call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {'median': round(float(np.median(ts)), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4), 'peak_extra_mb': round(peak / 2**20, 2)}


def composition(F, k, segs, l2, l2_n, chunk_bytes):
    """The torch form of ridge_rows: X [m, k] float32.  Segments longest first, a chunk holds as many as keep the padded
    [c, L, k] float64 gather and the [c, k, k] Gram batch under chunk_bytes each."""
    m, dev = segs.m, F.device
    order = np.argsort(-segs.counts, kind='stable')
    off = segs.off
    X = torch.zeros(m, k, dtype=torch.float32, device=dev)
    eye = torch.eye(k, dtype=torch.float64, device=dev)
    at = 0
    while at < m:
        L = int(segs.counts[order[at]])
        if L == 0:
            break
        c = max(1, min(m - at, chunk_bytes // (L * k * 8), chunk_bytes // (k * k * 8)))
        rows = torch.from_numpy(order[at:at + c]).to(dev)
        start, cnt = off[rows], torch.from_numpy(segs.counts[order[at:at + c]]).to(dev)
        pos = torch.arange(L, device=dev)[None, :]
        live = pos < cnt[:, None]
        j = torch.where(live, start[:, None] + pos, torch.zeros_like(pos))
        A = F[segs.idx[j].long(), :k].double() * live[:, :, None]
        r = segs.val[j].double() * live
        G = torch.bmm(A.transpose(1, 2), A) + (l2 + l2_n * cnt.double())[:, None, None] * eye
        b = torch.bmm(A.transpose(1, 2), r[:, :, None])
        R, info = torch.linalg.cholesky_ex(G)
        X[rows] = torch.cholesky_solve(b, R)[:, :, 0].float()
        at += c
    return X


def shape_times(name, data, reps, chunk_bytes):
    spec, k = SHAPES[name]
    d = engine.pad_dim(k)
    uid, iid, r = data['train']
    r = (r / 5).astype(np.float32)
    L, st = nv.lib(), nv.stream_handle()
    out = {'shape': name, 'k': k, 'pairs': len(uid)}
    gen = torch.Generator(device='cuda').manual_seed(1)
    l2, l2_n = 0.5, 0.0
    for side, seg, other, m, n_fixed in (('user', uid, iid, spec['n_user'], spec['n_item']), ('item', iid, uid, spec['n_item'], spec['n_user'])):
        F = torch.randn(n_fixed, d, device='cuda', generator=gen)
        segs = engine.SegmentSet(seg, other, r, m)
        X = torch.empty(m, d, dtype=torch.float32, device='cuda')
        status = torch.empty(2, dtype=torch.int32, device='cuda')

        def ridge(order):
            nv.check(L.ure_ridge_rows(nv.ptr(F), n_fixed, d, k, nv.ptr(segs.off), nv.ptr(segs.idx), nv.ptr(segs.val), m, nv.ptr(order), l2, l2_n,
                                      nv.ptr(X), nv.ptr(status), None, 0, st), 'ure_ridge_rows')
        res = {'segments': m, 'longest': int(segs.counts.max()), 'x_mb': round(m * d * 4 / 2**20, 2)}
        res['ridge_ms'] = event_ms(lambda: ridge(segs.order), reps)
        res['index_order_ms'] = event_ms(lambda: ridge(None), reps)
        assert status.cpu().tolist() == [0, -1]
        mine = X[:, :k].clone()
        res['composition_ms'] = event_ms(lambda: composition(F, k, segs, l2, l2_n, chunk_bytes), reps)
        theirs = composition(F, k, segs, l2, l2_n, chunk_bytes)
        scale = theirs.abs().amax(dim=1).clamp_min(1e-30)
        res['ridge_vs_composition_rel'] = float(((mine - theirs).abs().amax(dim=1) / scale).max())
        out[side] = res
        del F, segs, X, mine, theirs
        torch.cuda.empty_cache()
    return out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, round((time.perf_counter() - t0) * 1e3, 3)


def sisa_leg(data, epochs):
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import baseTest, trainer_l2
    from ultrare_amd.read import RatingData, loadData
    S, k = 5, 32
    n_user, n_item = data['n_user'], data['n_item']
    shard_of, groups = synth.uniform_shards(n_user, S)

    class P:
        lam, seed, batch, lr, lr_decay, momentum, parallel = 0.1, 42, 30000, 0.001, 0.95, 0.9, True
    P.k, P.epochs, P.n_user, P.n_item = k, epochs, n_user, n_item

    def loaders(triple, shuffle):
        return [loadData(RatingData(np.vstack(p)), P.batch, 24, shuffle) for p in synth.split_shards(triple, shard_of, S)]

    def total(triple):
        return loadData(RatingData(np.vstack([np.concatenate([p[c] for p in synth.split_shards(triple, shard_of, S)]) for c in range(3)])), P.batch, 24, False)
    ted, tot, trd = loaders(data['test'], False), total(data['test']), loaders(data['train'], True)
    sisa = Sisa(P, 'mf', S, groups)
    torch.manual_seed(42)
    ml = sisa.learn(trd, ted, tot, 0, '')
    dels = np.sort(np.random.RandomState(1).choice(n_user, int(0.02 * n_user), replace=False))
    theirs = total(tuple(x[np.isin(data['test'][0], dels)] for x in data['test']))
    trained_rows = ml[0].user_mat.weight.detach()[torch.from_numpy(dels).cuda()].clone()
    out = {'shards': S, 'k': k, 'epochs': epochs, 'deleted_users': len(dels), 'all_users_test': list(baseTest(tot, ml)),
           'as_trained_members_test': list(baseTest(theirs, ml))}
    keep = ~np.isin(data['train'][0], dels)
    trd_del = loaders(tuple(x[keep] for x in data['train']), True)
    s2 = Sisa(P, 'mf', S, [list(g) for g in groups])
    torch.manual_seed(42)
    s2.unlearn([copy.deepcopy(m) for m in ml], trd_del, ted, tot, dels.tolist(), 0, '')
    out['retrained_shards'] = len(s2.retrained)
    out['after_unlearn_test'] = list(baseTest(theirs, s2.model_list))
    gone = set(dels.tolist())
    s2.group_index = [[u for u in g if u not in gone] for g in s2.group_index]
    mine = tuple(x[~keep] for x in data['train'])
    triple = (mine[0].astype(np.int64), mine[1].astype(np.int64), (mine[2] / 5).astype(np.float32))
    l2 = trainer_l2(max(len(l.dataset) for l in trd_del), P.batch, P.lam)
    out['l2'] = l2
    home = shard_of[dels].astype(np.int64)
    for mode in ('home', 'ensemble'):
        s2.fold_in(triple, l2, groups=home, against=mode)                # warm-up of the call path
        s2.forget_folded(dels)
        _, ms_in = host_ms(lambda: s2.fold_in(triple, l2, groups=home, against=mode))
        rows = s2.model_list[0].user_mat.weight.detach()[torch.from_numpy(dels).cuda()]
        out[mode] = {'fold_in_ms': ms_in, 'test': list(baseTest(theirs, s2.model_list)),
                     'rows_rel_distance_to_trained': float((rows - trained_rows).norm() / trained_rows.norm()),
                     'rows_norm_over_trained_norm': float(rows.norm() / trained_rows.norm())}
        _, out[mode]['forget_folded_ms'] = host_ms(lambda: s2.forget_folded(dels))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--epochs', type=int, default=50)
    ap.add_argument('--chunk-mb', type=int, default=1024)
    ap.add_argument('--no-sisa', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('exp_ridge needs the GPU: nothing is measured on the host')
    out = {'gpu': torch.cuda.get_device_name(0), 'reps': a.reps, 'chunk_mb': a.chunk_mb, 'shapes': []}
    ml1m = None
    for name in [s for s in a.shapes.split(',') if s]:
        data = synth.make_dataset(**SHAPES[name][0])
        if name == 'ml1m':
            ml1m = data
        out['shapes'].append(shape_times(name, data, a.reps, a.chunk_mb << 20))
        del data
        torch.cuda.empty_cache()
    if not a.no_sisa:
        out['sisa'] = sisa_leg(ml1m or synth.make_dataset(**synth.ML1M), a.epochs)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
