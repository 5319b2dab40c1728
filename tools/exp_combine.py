"""The learned shard combiner (csrc/mf_combine.hip) measured on the GPU.  One JSON line.

    python tools/exp_combine.py [--shapes ml1m,cfg3] [--reps 7] [--epochs 50] [--no-sisa]

Per shape (ml1m: 5 models, d = 32, the 896,914 synthetic training pairs; cfg3: 32 models, d = 128, 22.5 M pairs; random
tables, the user table shared as after Sisa's merge), device time by events on the stream, medians of --reps launches after
two warm-up launches, the spread (min, max) beside every median, and the peak extra device memory of one call:
  stats_ms          one fused ure_combine_stats pass (link 0 and link 1)
  floor_ms          the S single-model ure_score passes into an [S, n] float32 matrix: the gathers the fused pass shares
  composition_ms    the torch composition the fused pass replaces: those S passes, then P.double() products for g and H
  weighted_ms       one ure_score_weighted pass, beside mean_ms, ure_score's mean over the same models
and, unless --no-sisa, on the ml-1m-shaped synthetic SISA of tools/e2e_sisa.py (5 shards, k = 32, --epochs epochs, parallel):
  accuracy          train loss and test (rmse, ndcg, hr) of the mean, the global and the per-group combiner, both links, W
  refit_ms          a whole Sisa.fit_combiner call (pairs to the device, every Newton pass, the host solves) on the
                    post-deletion loaders, per-group, both links, host clock with a synchronise, beside unlearn_ms, the
                    Sisa.unlearn call it follows, measured the same way in the same process
"""
import argparse
import copy
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ultrare_amd import _native as nv  # noqa: E402
from ultrare_amd import combine, engine, synth  # noqa: E402

SHAPES = {'ml1m': (synth.ML1M, 5, 32), 'cfg3': (synth.ML25M, 32, 128)}


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


def shape_times(name, data, reps):
    spec, S, d = SHAPES[name]
    uid, iid, r = data['train']
    pairs = engine.PairSet(uid, iid, (r / 5).astype(np.float32))
    n = pairs.n
    gen = torch.Generator(device='cuda').manual_seed(1)
    U = torch.randn(spec['n_user'], d, device='cuda', generator=gen) * d ** -0.25
    tables = [(U, torch.randn(spec['n_item'], d, device='cuda', generator=gen) * d ** -0.25) for _ in range(S)]
    L, st = nv.lib(), nv.stream_handle()
    theta = torch.from_numpy(combine.mean_weights(S)).cuda()
    out = {'shape': name, 'S': S, 'd': d, 'pairs': n, 'scratch_mb': round(L.ure_combine_stats_scratch(n, S) / 2**20, 2)}
    for link in (0, 1):
        out[f'stats_ms_link{link}'] = event_ms(lambda: engine.combine_stats(tables, d, pairs, link, theta, as_tensor=True), reps)

    ptrs = [((ctypes.c_void_p * 1)(Ut.data_ptr()), (ctypes.c_void_p * 1)(Vt.data_ptr())) for Ut, Vt in tables]

    def score_all():
        P = torch.empty(S, n, dtype=torch.float32, device='cuda')
        for s, (Up, Vp) in enumerate(ptrs):
            nv.check(L.ure_score(Up, Vp, 1, 1, 1, 0, nv.ptr(pairs.uid), nv.ptr(pairs.iid), None, n, d, nv.ptr(P[s]), None, st), 'ure_score')
        return P

    def composition():
        P = score_all()
        X = torch.cat([P.double(), torch.ones(1, n, dtype=torch.float64, device='cuda')])        # [S + 1, n]
        z = theta @ X
        res = z - pairs.rating.double()
        return 0.5 * (res * res).sum(), X @ res, X @ X.T

    out['floor_ms'] = event_ms(score_all, reps)
    out['composition_ms'] = event_ms(composition, reps)
    # the two agree (link 0, the mean start)
    got = engine.combine_stats(tables, d, pairs, 0, theta)
    loss, g, H = composition()
    _, wl, wg, wH = combine.unpack_stats(got, S)
    out['fused_vs_composition'] = {'loss_rel': abs(wl - float(loss)) / float(loss), 'g_rel': float(np.abs(wg - g.cpu().numpy()).max() / np.abs(wg).max()),
                                   'H_rel': float(np.abs(wH - H.cpu().numpy()).max() / np.abs(wH).max())}
    W = torch.from_numpy(np.tile(combine.mean_weights(S), (S, 1))).cuda()
    gou = torch.from_numpy((np.arange(spec['n_user']) % S).astype(np.int32)).cuda()
    pred = torch.empty(n, dtype=torch.float32, device='cuda')
    sse = torch.empty(engine.SCORE_PARTIALS, dtype=torch.float64, device='cuda')
    for link in (0, 1):
        out[f'weighted_ms_link{link}'] = event_ms(lambda: engine.score_weighted(tables, d, pairs.uid, pairs.iid, pairs.rating, link, W, gou, pred=pred, sse=sse), reps)
    Up = (ctypes.c_void_p * S)(*[Ut.data_ptr() for Ut, _ in tables])
    Vp = (ctypes.c_void_p * S)(*[Vt.data_ptr() for _, Vt in tables])
    out['mean_ms'] = event_ms(lambda: nv.check(L.ure_score(Up, Vp, S, S, 1, 1, nv.ptr(pairs.uid), nv.ptr(pairs.iid), nv.ptr(pairs.rating), n, d, nv.ptr(pred),
                                                           nv.ptr(sse), st), 'ure_score'), reps)
    return out


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {'median': round(float(np.median(ts)), 3), 'min': round(min(ts), 3), 'max': round(max(ts), 3)}


def sisa_leg(data, epochs, reps):
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import baseTest, fit_combiner
    from ultrare_amd.read import RatingData, loadData
    S, k = 5, 32
    n_user, n_item = data['n_user'], data['n_item']
    shard_of, groups = synth.uniform_shards(n_user, S)

    class P:
        lam, seed, batch, lr, lr_decay, momentum, parallel = 0.1, 42, 30000, 0.001, 0.95, 0.9, True
    P.k, P.epochs, P.n_user, P.n_item = k, epochs, n_user, n_item

    def loaders(triple, shuffle):
        return [loadData(RatingData(np.vstack(p)), P.batch, 24, shuffle) for p in synth.split_shards(triple, shard_of, S)]
    ted = loaders(data['test'], False)
    tot = loadData(RatingData(np.vstack([np.concatenate([p[c] for p in synth.split_shards(data['test'], shard_of, S)]) for c in range(3)])), P.batch, 24, False)
    trd = loaders(data['train'], True)
    sisa = Sisa(P, 'mf', S, groups)
    torch.manual_seed(42)
    ml = sisa.learn(trd, ted, tot, 0, '')
    out = {'shards': S, 'k': k, 'epochs': epochs, 'accuracy': {'mean': {'test': list(baseTest(tot, ml))}}}
    for link in ('linear', 'logistic'):
        for name, grp in (('global', None), ('per_group', groups)):
            c = fit_combiner(ml, trd, link, groups=grp)
            out['accuracy'][f'{link}_{name}'] = {'train_loss_mean_start': float(c.loss_before.sum()), 'train_loss': float(c.loss_after.sum()),
                                                 'iters': c.iters.tolist(), 'grad_norm': float(c.grad_norm.max()), 'test': list(baseTest(tot, ml, combiner=c)),
                                                 'W': np.round(c.W, 5).tolist(),
                                                 'home_weight_is_largest': [bool(np.argmax(c.W[g, :S]) == g) for g in range(len(c.W))] if grp else None}
    # a deletion, the retraining it asks for, and the refit that follows
    del_user = np.random.RandomState(1).choice(n_user, int(0.02 * n_user), replace=False)
    keep = ~np.isin(data['train'][0], del_user)
    un = []
    for rep in range(reps + 1):
        trd_del = loaders(tuple(x[keep] for x in data['train']), True)
        s2 = Sisa(P, 'mf', S, groups)
        snap = [copy.deepcopy(m) for m in ml]
        torch.manual_seed(42)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s2.unlearn(snap, trd_del, ted, tot, del_user.tolist(), 0, '')
        torch.cuda.synchronize()
        s2._check_closed()
        un.append((time.perf_counter() - t0) * 1e3)
    un = un[1:]
    out['unlearn_ms'] = {'median': round(float(np.median(un)), 3), 'min': round(min(un), 3), 'max': round(max(un), 3)}
    out['retrained_shards'] = len(s2.retrained)
    for link in ('linear', 'logistic'):
        s2.fit_combiner(trd_del, link)                       # warm-up
        out[f'refit_ms_{link}'] = host_ms(lambda: s2.fit_combiner(trd_del, link), reps)
        out[f'refit_iters_{link}'] = s2.combiner.iters.tolist()
        out[f'refit_test_{link}'] = list(s2.test_combined(tot, 0, ''))
    out['unlearn_test_mean'] = [s2.log0['total_rmse'], s2.log0['total_ndcg'], s2.log0['total_hr']]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--epochs', type=int, default=50)
    ap.add_argument('--no-sisa', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('exp_combine needs the GPU: nothing is measured on the host')
    out = {'gpu': torch.cuda.get_device_name(0), 'reps': a.reps, 'shapes': []}
    ml1m = None
    for name in [s for s in a.shapes.split(',') if s]:
        data = synth.make_dataset(**SHAPES[name][0])
        if name == 'ml1m':
            ml1m = data
        out['shapes'].append(shape_times(name, data, a.reps))
        del data
        torch.cuda.empty_cache()
    if not a.no_sisa:
        out['sisa'] = sisa_leg(ml1m or synth.make_dataset(**synth.ML1M), a.epochs, a.reps)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
