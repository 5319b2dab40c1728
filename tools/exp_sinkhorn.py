"""The entropic OT solver of csrc/ot_sinkhorn.hip (engine.ot_sinkhorn) at the ml-1m user shape and BASELINE.json configs[3]'s
(162,000 users, d = 128), and at 1,000,000 x 64 when it fits, beside the exact path.  One JSON line for all shapes.

    python tools/exp_sinkhorn.py [--shapes 6040x5,6040x16,162000x32,1000000x64] [--d 128] [--reps 3]

Per shape and for reg = 1e-3 (the reference's `lam`, capped at 1000 iterations) and reg = 0.05 median(M) (converging):
  iter_us      device time of one iteration, from two solves with stop_thr = 0 (never stops) of 40 and 140 iterations
  solve_ms     the whole ure_ot_sinkhorn call (host clock, synchronised), and its iterations
  round_ms     one ot_cluster(solver='sinkhorn') round (cost, solve, labels down, sort, centroids; max_iters=1), host clock
and exact_round_ms, one ot_cluster round of the exact path (cost matrix to the host, exact LP), for comparison.  The
embedding is the clustered normal one of the OT pins (12 centres, d = 128); the cost is ure_ot_cost's [k, n] matrix.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ultrare_amd import _native as nv  # noqa: E402
from ultrare_amd import engine  # noqa: E402
from ultrare_amd.method.utils import ot_cluster  # noqa: E402


def embedding(n, d, seed=0):
    rs = np.random.RandomState(seed)
    centers = rs.standard_normal((12, d)) * 0.8
    return (centers[rs.randint(0, 12, n)] + rs.standard_normal((n, d)) * 0.6).astype(np.float32)


def host_ms(fn, reps):
    best = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(best))


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='6040x5,6040x16,162000x32,1000000x64')
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('exp_sinkhorn needs the GPU: nothing is measured on the host')
    out = {'gpu': torch.cuda.get_device_name(0), 'd': a.d, 'shapes': []}
    for shape in a.shapes.split(','):
        n, k = map(int, shape.split('x'))
        need = n * a.d * 4 + n * k * 4 + nv.lib().ure_ot_sinkhorn_scratch(n, k) + n * 24
        free, _ = torch.cuda.mem_get_info()
        if need > 0.8 * free:
            out['shapes'].append({'n': n, 'k': k, 'skipped': f'needs {need / 2**30:.1f} GiB'})
            continue
        X = embedding(n, a.d)
        Xd = torch.from_numpy(X).cuda()
        C = torch.from_numpy(X[np.random.RandomState(1).choice(n, k, replace=False)]).cuda()
        dist = torch.empty(k, n, dtype=torch.float32, device='cuda')
        nv.check(nv.lib().ure_ot_cost(nv.ptr(Xd), nv.ptr(C), n, k, a.d, nv.ptr(dist), nv.stream_handle()), 'ure_ot_cost')
        med = float(dist.median())
        row = {'n': n, 'k': k, 'cost_max': float(dist.max()), 'cost_median': med}
        for tag, reg in (('lam', 1e-3), ('rel', 0.05 * med)):
            solve = lambda it, thr=1e-9: engine.ot_sinkhorn(dist, reg, it, thr, want_u=False, want_cost_min=True)
            solve(10)
            t40, t140 = host_ms(lambda: solve(40, 0.0), a.reps), host_ms(lambda: solve(140, 0.0), a.reps)
            r = solve(1000)
            sizes = np.bincount(r['label'].cpu().numpy(), minlength=k)
            row[tag] = {'reg': reg, 'iter_us': round((t140 - t40) / 100 * 1e3, 2), 'iters': r['iters'], 'err': r['err'],
                        'solve_ms': round(host_ms(lambda: solve(1000), a.reps), 3), 'group_min_max': [int(sizes.min()), int(sizes.max())]}

            def one_round():
                np.random.seed(0)
                quiet(lambda: ot_cluster(X, k, max_iters=1, solver='sinkhorn', reg=reg))
            try:
                one_round()
                row[tag]['round_ms'] = round(host_ms(one_round, a.reps), 3)
            except ValueError as e:                        # an empty group at this reg
                row[tag]['round_ms'] = None
                row[tag]['round_error'] = str(e)[:120]

        def exact_round():
            np.random.seed(0)
            quiet(lambda: ot_cluster(X, k, max_iters=1))
        if n <= 200000:
            exact_round()
            row['exact_round_ms'] = round(host_ms(exact_round, a.reps), 3)
        out['shapes'].append(row)
        del Xd, C, dist
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
