"""Newton-step (influence) unlearning (csrc/influence.hip) measured on one GPU.  One JSON line.

    python tools/exp_influence.py [--shapes ml1m,cfg3] [--reps 5] [--epochs 50] [--no-sisa]

Per shape -- shard 0 of the uniform grouping of the synthetic set, its users renumbered: ml1m 1,208 x 3,416 at d = 32 (5 shards),
cfg3 5,062 x 60,000 at d = 128 (32 shards):
  matvec      engine.inf_matvec (full curvature, residuals held) against the torch float64 double-backward composition it replaces
              (two gathers, autograd.grad with create_graph, a second autograd.grad): device time by events, medians of --reps
              after two warm-ups with (min, max), the peak extra device memory of one call, and the largest relative difference
  steps       tables brought near the ALS fixed point of the shard (utils.als_sweeps, --sweeps sweeps, l2 = trainer_l2), 2 % of its
              users deleted: utils.newton_unlearn with the defaults for one step and for three -- CG iterations, wall time (host
              clock with a synchronise), peak memory, and the objective's gap to the yardstick (--sweeps further ALS sweeps on what
              remains) beside the gap of "zero the emptied rows and stop"
and, unless --no-sisa, on the ml-1m-shaped synthetic SISA of tools/exp_combine.py (5 shards, k = 32, --epochs epochs of SGD, parallel),
2 % of the users deleted:
  sisa        Sisa.unlearn_influence (defaults; and curvature='gn') against Sisa.unlearn and against "zero the rows and stop" on the
              same request: wall time, and closeness to the RETRAINED ensemble -- objective gap per shard on its remaining data, max
              and RMS difference of the mean ensemble's predictions on the test set, rank_eval HR@10 / NDCG@10 of each
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
from ultrare_amd import engine, synth  # noqa: E402
from ultrare_amd.method import utils  # noqa: E402
from ultrare_amd.method.utils import MF  # noqa: E402

SHAPES = {'ml1m': (synth.ML1M, 5, 32), 'cfg3': (synth.ML25M, 32, 128)}
BATCH, LAM = 30000, 0.1


def event_ms(fn, reps, warmup=2):
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


def host_once(fn):
    """-> (result, wall ms with a synchronise on both sides, peak extra device memory in MiB)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round((time.perf_counter() - t0) * 1e3, 3), round((torch.cuda.max_memory_allocated() - base) / 2**20, 2)


def shard_zero(name):
    spec, S, d = SHAPES[name]
    data = synth.make_dataset(**spec)
    shard_of, _ = synth.uniform_shards(spec['n_user'], S)
    u, i, r = data['train']
    pick = shard_of[u] == 0
    users, uu = np.unique(u[pick], return_inverse=True)
    return uu.astype(np.int64), i[pick].astype(np.int64), (r[pick] / 5).astype(np.float32), len(users), spec['n_item'], d


def matvec_leg(case, reps):
    u, i, r, n_user, n_item, d = case
    g = engine.GcnGraph(u, i, r, n_user, n_item)
    gen = torch.Generator(device='cuda').manual_seed(1)
    U = torch.randn(n_user, d, device='cuda', generator=gen) * d ** -0.25
    V = torch.randn(n_item, d, device='cuda', generator=gen) * d ** -0.25
    P = torch.randn(n_user, d, device='cuda', generator=gen, dtype=torch.float64)
    Q = torch.randn(n_item, d, device='cuda', generator=gen, dtype=torch.float64)
    l2 = utils.trainer_l2(len(u), BATCH, LAM)
    e = engine.inf_coef(g, U, V)
    ud, idd, rd = (torch.from_numpy(a).cuda() for a in (u, i, r.astype(np.float64)))

    def composition():
        Ut, Vt = U.double().requires_grad_(True), V.double().requires_grad_(True)
        res = (Ut[ud] * Vt[idd]).sum(dim=1) - rd
        F = (res * res).sum() + l2 * ((Ut * Ut).sum() + (Vt * Vt).sum())
        gU, gV = torch.autograd.grad(F, (Ut, Vt), create_graph=True)
        return torch.autograd.grad((gU * P).sum() + (gV * Q).sum(), (Ut, Vt))

    out = {'kernel_ms': event_ms(lambda: engine.inf_matvec(g, U, V, P, Q, l2, 0.0, 'full', None, e), reps),
           'kernel_gn_ms': event_ms(lambda: engine.inf_matvec(g, U, V, P, Q, l2, 0.0, 'gn'), reps),
           'composition_ms': event_ms(composition, reps)}
    HU, HV = engine.inf_matvec(g, U, V, P, Q, l2, 0.0, 'full', None, e)
    wU, wV = composition()
    # (a row without entries is left out of the system: +0.0 from the kernel, 2 l2 P[row] from the composition -- not compared)
    has_u, has_i = (torch.from_numpy(np.diff(o) > 0).cuda() for o in (g.host.off_u, g.host.off_i))
    out['rows_without_entries'] = [int((~has_u).sum()), int((~has_i).sum())]
    out['rel_diff'] = float(max(((HU - wU)[has_u].abs().max() / wU.abs().max()).item(), ((HV - wV)[has_i].abs().max() / wV.abs().max()).item()))
    return out


def steps_leg(case, sweeps):
    u, i, r, n_user, n_item, d = case
    l2 = utils.trainer_l2(len(u), BATCH, LAM)
    gen = torch.Generator(device='cuda').manual_seed(2)
    start = MF.from_tables(torch.randn(n_user, d, device='cuda', generator=gen) * 0.1, torch.randn(n_item, d, device='cuda', generator=gen) * 0.1)
    start, obj = utils.als_sweeps(start, (u, i, r), l2, sweeps=sweeps)
    gone = np.random.RandomState(1).choice(n_user, max(1, int(0.02 * n_user)), replace=False)
    keep = ~np.isin(u, gone)
    rest = (u[keep], i[keep], r[keep])
    l2r = utils.trainer_l2(int(keep.sum()), BATCH, LAM)
    _, yard = utils.als_sweeps(copy.deepcopy(start), rest, l2r, sweeps=sweeps)
    g = engine.GcnGraph(*rest, n_user, n_item)

    def F_of(model):
        U, V, _ = utils.padded_tables(model)
        parts = engine.inf_objective(g, U.contiguous(), V.contiguous(), l2r).cpu().numpy()
        return float(parts[0] + l2r * parts[1])

    zeroed = copy.deepcopy(start)
    zeroed.user_mat.weight[torch.from_numpy(gone).cuda()] = 0.0
    out = {'l2': l2r, 'als_sweeps': sweeps, 'ratings_left': int(keep.sum()), 'users_deleted': len(gone), 'als_objective_last_two': [float(obj[-2]), float(obj[-1])],
           'F_yardstick': float(yard[-1]), 'gap_zero_rows_only': F_of(zeroed) - float(yard[-1])}
    utils.newton_unlearn(copy.deepcopy(start), rest, l2=l2r, iters=16)                       # warm-up (allocator, code objects)
    for steps in (1, 3):
        m = copy.deepcopy(start)
        logs, ms, peak = host_once(lambda: utils.newton_unlearn(m, rest, l2=l2r, steps=steps))
        out[f'steps{steps}'] = {'wall_ms': ms, 'peak_extra_mb': peak, 'cg_iters': [l['iters_run'] for l in logs], 'status': [l['status'] for l in logs],
                                'applied': [l['applied'] for l in logs], 'gap': F_of(m) - float(yard[-1])}
    m = copy.deepcopy(start)
    logs, ms, peak = host_once(lambda: utils.newton_unlearn(m, rest, l2=l2r, curvature='gn', steps=1))
    out['gn_steps1'] = {'wall_ms': ms, 'cg_iters': [l['iters_run'] for l in logs], 'status': [l['status'] for l in logs], 'applied': [l['applied'] for l in logs],
                        'gap': F_of(m) - float(yard[-1])}
    return out


def sisa_leg(data, epochs):
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.read import RatingData, loadData
    S, k = 5, 32
    n_user, n_item = data['n_user'], data['n_item']
    shard_of, groups = synth.uniform_shards(n_user, S)

    class P:
        lam, seed, batch, lr, lr_decay, momentum, parallel = LAM, 42, BATCH, 0.001, 0.95, 0.9, True
    P.k, P.epochs, P.n_user, P.n_item = k, epochs, n_user, n_item

    def loaders(triple, shuffle):
        return [loadData(RatingData(np.vstack(p)), P.batch, 24, shuffle) for p in synth.split_shards(triple, shard_of, S)]
    parts = synth.split_shards(data['test'], shard_of, S)
    ted = loaders(data['test'], False)
    tot = loadData(RatingData(np.vstack([np.concatenate([p[c] for p in parts]) for c in range(3)])), P.batch, 24, False)
    trd = loaders(data['train'], True)
    sisa = Sisa(P, 'mf', S, groups)
    torch.manual_seed(42)
    ml = sisa.learn(trd, ted, tot, 0, '')
    del_user = np.random.RandomState(1).choice(n_user, int(0.02 * n_user), replace=False)
    keep = ~np.isin(data['train'][0], del_user)
    rest_parts = synth.split_shards(tuple(x[keep] for x in data['train']), shard_of, S)
    trd_del = loaders(tuple(x[keep] for x in data['train']), True)
    tu, ti = (torch.from_numpy(np.concatenate([p[c] for p in parts]).astype(np.int64)).cuda() for c in (0, 1))

    def predictions(models):
        U = models[0].user_mat.weight.detach().double()
        return sum((U[tu] * m.item_mat.weight.detach().double()[ti]).sum(dim=1) for m in models) / len(models)

    def shard_F(models):
        out = []
        for s in range(S):
            u, i, r = rest_parts[s]
            g = engine.GcnGraph(u, i, r, n_user, n_item)
            l2 = utils.trainer_l2(len(u), BATCH, LAM)
            U = models[s].user_mat.weight.detach().clone()
            own = np.zeros(n_user, dtype=bool)
            own[np.asarray(groups[s], dtype=np.int64)] = True
            U[torch.from_numpy(~own).cuda()] = 0.0                 # a shard's objective is over its own rows
            parts_ = engine.inf_objective(g, U.contiguous(), models[s].item_mat.weight.detach().contiguous(), l2).cpu().numpy()
            out.append(float(parts_[0] + l2 * parts_[1]))
        return out

    def run(how, **kw):
        s2 = Sisa(P, 'mf', S, groups)
        snap = [copy.deepcopy(m) for m in ml]
        torch.manual_seed(42)
        if how == 'retrain':
            _, ms, peak = host_once(lambda: (s2.unlearn(snap, trd_del, ted, tot, del_user.tolist(), 0, ''), s2._check_closed()))
        elif how == 'zero':
            def zero():
                s2.model_list = snap
                s2._set_rows(del_user)
                s2.test(tot, 0, '')
            _, ms, peak = host_once(zero)
        else:
            _, ms, peak = host_once(lambda: s2.unlearn_influence(snap, trd_del, tot, del_user.tolist(), 0, '', **kw))
        return s2, ms, peak

    run('retrain')                                                 # warm-up
    run('influence', iters=16)
    ref, ms, peak = run('retrain')
    want, F_ref = predictions(ref.model_list), shard_F(ref.model_list)
    out = {'shards': S, 'k': k, 'epochs': epochs, 'users_deleted': len(del_user), 'retrain': {'wall_ms': ms, 'peak_extra_mb': peak, 'shards': ref.retrained,
                                                                                              'rank': utils.rank_eval(ref.model_list, tot, ks=(10,)), 'log0': ref.log0}}
    for name, how, kw in (('zero_rows_only', 'zero', {}), ('influence_full_1', 'influence', {}), ('influence_full_3', 'influence', dict(steps=3)),
                          ('influence_gn_1', 'influence', dict(curvature='gn'))):
        s2, ms, peak = run(how, **kw)
        diff = predictions(s2.model_list) - want
        F = shard_F(s2.model_list)
        rec = {'wall_ms': ms, 'peak_extra_mb': peak, 'pred_max_diff': float(diff.abs().max()), 'pred_rms_diff': float((diff * diff).mean().sqrt()),
               'objective_gap_per_shard': [a - b for a, b in zip(F, F_ref)], 'rank': utils.rank_eval(s2.model_list, tot, ks=(10,)), 'log0': s2.log0}
        if how == 'influence':
            rec['shards'] = s2.influenced
            rec['steps'] = {str(s): [(l['iters_run'], l['status'], bool(l['applied'])) for l in logs] for s, logs in s2.influence_logs.items()}
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--epochs', type=int, default=50)
    ap.add_argument('--sweeps', type=int, default=100)
    ap.add_argument('--no-sisa', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('exp_influence needs the GPU: nothing is measured on the host')
    out = {'gpu': torch.cuda.get_device_name(0), 'reps': a.reps, 'shapes': {}}
    for name in [s for s in a.shapes.split(',') if s]:
        case = shard_zero(name)
        out['shapes'][name] = {'users': case[3], 'items': case[4], 'd': case[5], 'ratings': len(case[0]), 'matvec': matvec_leg(case, a.reps),
                               'steps': steps_leg(case, a.sweeps)}
        print(json.dumps({name: out['shapes'][name]}), flush=True)
        del case
        torch.cuda.empty_cache()
    if not a.no_sisa:
        out['sisa'] = sisa_leg(synth.make_dataset(**synth.ML1M), a.epochs)
    print(json.dumps(out, default=float), flush=True)


if __name__ == '__main__':
    main()
