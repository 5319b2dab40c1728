"""Weighted matrix factorisation for implicit feedback (csrc/wmf.hip) measured on the GPU.  One JSON line per leg,
each printed as soon as it is done.  Run by no test.

    python tools/exp_wmf.py [--shapes ml1m,cfg3] [--reps 7] [--comp-reps 3] [--no-toy]

Per shape (ml1m: 6,040 x 3,416, the 896,914 synthetic training pairs, k = 32; cfg3: 162,000 x 60,000, 22.5 M pairs, k = 128; N(0, 1)
tables, alpha = 40, l2 = 0.1: the untuned defaults), device time by events on the stream, medians of --reps launches after two
warm-up launches with (min, max) beside every median, and the peak extra device memory of one call:
  gram_ms           ure_gram of the item table and of the user table
  user / item       one half sweep's ure_wridge_rows (longest-first order, G0 given) and, the first yardstick, ure_ridge_rows -- the
                    plain kernel -- on the same segments, with the ratio of the two medians
  sweep_ms          a whole sweep: gram, user half, gram, item half, back to back
  composition_ms    the second yardstick, a torch composition of one half sweep: float64 F.T @ F, the segments longest first in chunks
                    padded to the chunk's longest, the weighted normal equations by float64 bmm, torch.linalg.cholesky_ex and
                    cholesky_solve (--comp-reps launches), and the largest difference between the two results relative to the row's
                    largest entry
and, unless --no-toy, on tests/golden/toy with 3 uniform shards, k = 16, ONE seed (42) and untuned defaults throughout: HR@10 / NDCG@10
from utils.rank_eval (training items excluded) of the ensembles trained by MSE ('mf', 50 epochs), by BPR ('lightgcn' with 0 layers, 50
epochs) and by WMF (10 sweeps, alpha = 40, l2 = 0.1).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from ultrare_amd import _native as nv  # noqa: E402
from ultrare_amd import engine, synth  # noqa: E402

SHAPES = {'ml1m': (synth.ML1M, 32), 'cfg3': (synth.ML25M, 128)}
ALPHA, L2 = 40.0, 0.1


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


def composition(F, k, segs, wg, wb, l2, chunk_bytes):
    """The torch form of one half sweep: X [m, k] float32."""
    m, dev = segs.m, F.device
    Fk = F[:, :k].double()
    G0 = Fk.T @ Fk
    order = np.argsort(-segs.counts, kind='stable')
    X = torch.zeros(m, k, dtype=torch.float32, device=dev)
    eye = torch.eye(k, dtype=torch.float64, device=dev)
    at = 0
    while at < m:
        L = int(segs.counts[order[at]])
        if L == 0:
            break
        c = max(1, min(m - at, chunk_bytes // (L * k * 8), chunk_bytes // (k * k * 8)))
        rows = torch.from_numpy(order[at:at + c]).to(dev)
        start, cnt = segs.off[rows], torch.from_numpy(segs.counts[order[at:at + c]]).to(dev)
        pos = torch.arange(L, device=dev)[None, :]
        live = pos < cnt[:, None]
        j = torch.where(live, start[:, None] + pos, torch.zeros_like(pos))
        A = Fk[segs.idx[j].long()] * live[:, :, None]
        G = torch.bmm(A.transpose(1, 2), A * wg[j].double()[:, :, None]) + G0 + l2 * eye
        b = torch.bmm(A.transpose(1, 2), (wb[j].double() * live)[:, :, None])
        R, _ = torch.linalg.cholesky_ex(G)
        X[rows] = torch.cholesky_solve(b, R)[:, :, 0].float()
        at += c
    return X


def shape_times(name, data, reps, comp_reps, chunk_bytes):
    spec, k = SHAPES[name]
    d = engine.pad_dim(k)
    uid, iid, r = data['train']
    r = (r / 5).astype(np.float32)
    L, st = nv.lib(), nv.stream_handle()
    out = {'leg': 'shape', 'shape': name, 'k': k, 'pairs': len(uid), 'alpha': ALPHA, 'l2': L2}
    gen = torch.Generator(device='cuda').manual_seed(1)
    tables = {'item': torch.randn(spec['n_item'], d, device='cuda', generator=gen), 'user': torch.randn(spec['n_user'], d, device='cuda', generator=gen)}
    out['gram_ms'] = {side: event_ms(lambda T=T: engine.gram(T, d, k), reps) for side, T in tables.items()}
    calls = {}
    for side, seg, other, fixed in (('user', uid, iid, 'item'), ('item', iid, uid, 'user')):
        F = tables[fixed]
        n_fixed, m = int(F.shape[0]), int(tables[side].shape[0])
        segs = engine.SegmentSet(seg, other, r, m)
        wg, wb = engine.confidence(segs.val, ALPHA)
        G0 = engine.gram(F, d, k)
        X = torch.empty(m, d, dtype=torch.float32, device='cuda')
        status = torch.empty(2, dtype=torch.int32, device='cuda')

        def weighted(F=F, n_fixed=n_fixed, segs=segs, wg=wg, wb=wb, G0=G0, X=X, status=status, m=m):
            nv.check(L.ure_wridge_rows(nv.ptr(F), n_fixed, d, k, nv.ptr(segs.off), nv.ptr(segs.idx), nv.ptr(wg), nv.ptr(wb), m, nv.ptr(segs.order),
                                       nv.ptr(G0), L2, 0.0, nv.ptr(X), nv.ptr(status), None, 0, st), 'ure_wridge_rows')

        def plain(F=F, n_fixed=n_fixed, segs=segs, X=X, status=status, m=m):
            nv.check(L.ure_ridge_rows(nv.ptr(F), n_fixed, d, k, nv.ptr(segs.off), nv.ptr(segs.idx), nv.ptr(segs.val), m, nv.ptr(segs.order), L2, 0.0,
                                      nv.ptr(X), nv.ptr(status), None, 0, st), 'ure_ridge_rows')
        res = {'segments': m, 'longest': int(segs.counts.max()), 'x_mb': round(m * d * 4 / 2**20, 2)}
        res['ridge_rows_ms'] = event_ms(plain, reps)
        res['wridge_rows_ms'] = event_ms(weighted, reps)
        assert status.cpu().tolist() == [0, -1]
        res['weighted_over_plain'] = round(res['wridge_rows_ms']['median'] / res['ridge_rows_ms']['median'], 4)
        mine = X[:, :k].clone()
        if comp_reps > 0:
            res['composition_ms'] = event_ms(lambda: composition(F, k, segs, wg, wb, L2, chunk_bytes), comp_reps, warmup=1)
            theirs = composition(F, k, segs, wg, wb, L2, chunk_bytes)
            scale = theirs.abs().amax(dim=1).clamp_min(1e-30)
            res['wridge_vs_composition_rel'] = float(((mine - theirs).abs().amax(dim=1) / scale).max())
            del theirs
        out[side] = res
        calls[side] = (weighted, F)
        torch.cuda.empty_cache()

    def sweep():
        engine.gram(tables['item'], d, k)
        calls['user'][0]()
        engine.gram(tables['user'], d, k)
        calls['item'][0]()
    out['sweep_ms'] = event_ms(sweep, reps)
    return out


def toy_leg():
    from ultrare_amd.method import utils
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.read import RatingData, loadData, readRating, readSparseMat
    G = os.path.join(ROOT, 'tests', 'golden', 'toy')
    train, test, n_user, n_item, S = os.path.join(G, '0_train.csv'), os.path.join(G, '0_test.csv'), 1508, 2071, 3
    tr, idx = readRating(train, n_user, 5, [], [], S, [])
    te, _ = readRating(test, n_user, 5, [], [], S, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    tot = loadData(RatingData(np.hstack(te)), 3000, 24, False)
    seen = readSparseMat(train, n_user, n_item)

    class P:
        k, lam, seed, batch, lr, lr_decay, momentum, parallel = 16, 0.1, 42, 3000, 0.001, 0.95, 0.9, False
    P.n_user, P.n_item = n_user, n_item
    out = {'leg': 'toy', 'shards': S, 'k': 16, 'seed': 42, 'note': 'one seed, untuned defaults'}
    for label, model_type, extra in (('mf_mse_50_epochs', 'mf', dict(epochs=50)), ('mf_bpr_50_epochs', 'lightgcn', dict(epochs=50, loss='bpr', gcn_layers=0)),
                                     ('wmf_10_sweeps', 'wmf', dict(epochs=10))):
        p = P()
        for key, v in extra.items():
            setattr(p, key, v)
        sisa = Sisa(p, model_type, S, [list(g) for g in idx])
        torch.manual_seed(42)
        ml = sisa.learn(trd, ted, tot, 0, '')
        m = utils.rank_eval(ml, tot, exclude=seen, ks=(10,))
        out[label] = {key: round(float(m[key]), 4) for key in ('hr@10', 'ndcg@10', 'recall@10', 'mrr')}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--comp-reps', type=int, default=3)
    ap.add_argument('--chunk-mb', type=int, default=1024)
    ap.add_argument('--no-toy', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('exp_wmf needs the GPU: nothing is measured on the host')
    print(json.dumps({'leg': 'setup', 'gpu': torch.cuda.get_device_name(0), 'reps': a.reps, 'comp_reps': a.comp_reps, 'chunk_mb': a.chunk_mb}), flush=True)
    if not a.no_toy:
        print(json.dumps(toy_leg()), flush=True)
    for name in [s for s in a.shapes.split(',') if s]:
        data = synth.make_dataset(**SHAPES[name][0])
        print(json.dumps(shape_times(name, data, a.reps, a.comp_reps, a.chunk_mb << 20)), flush=True)
        del data
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
