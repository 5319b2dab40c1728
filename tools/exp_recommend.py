"""Full-catalogue top-k recommendation (engine.recommend -> ure_recommend_topk) against the plain torch composition
(per-shard matmul, mean, mask, torch.topk) on the same inputs.  One JSON line per shape.

    python tools/exp_recommend.py [--shapes ml1m,cfg3,s128] [--window 1.0]

Tables are random normal (the kernel's cost does not depend on the values); the exclusion set is random at the given
density.  Times are device events around back-to-back calls after a warm-up, over a window of about --window seconds;
kernel times alone come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ultrare_amd import engine  # noqa: E402

PEAK_FP32 = 157.3e12          # MI355X FP32 vector peak (spec)

SHAPES = {
    # name: (n_user, n_query, n_item, S, d, k, exclusion density)
    'ml1m': (6040, 6040, 3416, 5, 32, 10, 0.048),        # ml-1m: 1,000,209 ratings over 6,040 x 3,706 (4.5-4.8 % dense)
    'cfg3': (162541, 4096, 60000, 32, 128, 100, 0.0),    # BASELINE.json configs[3]: 32 shards, 60 k items, d = 128
    's128': (162541, 256, 60000, 128, 128, 100, 0.0),    # 128-shard ensemble
}


def timed(fn, window):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(3, int(window / one))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3, reps      # us per call


def torch_topk(tables, users_t, k, mask):
    acc = None
    for U, V in tables:
        s = U[users_t] @ V.T
        acc = s if acc is None else acc + s
    acc = acc / len(tables)
    if mask is not None:
        acc = acc.masked_fill(mask, float('-inf'))
    return torch.topk(acc, k, dim=1)


def run(name, window, no_torch):
    n_user, n_query, n_item, S, d, k, dens = SHAPES[name]
    g = torch.Generator(device='cuda').manual_seed(0)
    # (every shard of a SISA ensemble shares the merged user table; one U per shard here keeps the kernel's loads general)
    tables = [(torch.randn(n_user, d, device='cuda', generator=g), torch.randn(n_item, d, device='cuda', generator=g)) for _ in range(S)]
    rng = np.random.default_rng(1)
    users = rng.choice(n_user, n_query, replace=False)
    excl, mask = None, None
    if dens > 0:
        rows = [np.flatnonzero(rng.random(n_item) < dens).astype(np.int32) for _ in range(n_query)]
        off = np.zeros(n_query + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rows], out=off[1:])
        excl = (off, np.concatenate(rows))
        mask = torch.zeros(n_query, n_item, dtype=torch.bool)
        mask[torch.from_numpy(np.repeat(np.arange(n_query), np.diff(off))), torch.from_numpy(excl[1].astype(np.int64))] = True
        mask = mask.cuda()
    us, reps = timed(lambda: engine.recommend(tables, d, users, k, excl), window)
    flop = 2.0 * n_query * n_item * S * d
    out = {'shape': name, 'n_query': n_query, 'n_item': n_item, 'S': S, 'd': d, 'k': k, 'excluded': int(len(excl[1])) if excl else 0,
           'recommend_us': round(us, 1), 'calls': reps, 'gflop': round(flop / 1e9, 2), 'tflops': round(flop / us / 1e6, 2),
           'peak_share': round(flop / us / 1e6 / (PEAK_FP32 / 1e12), 4),
           'scratch_bytes': int(engine.nv.lib().ure_recommend_scratch(n_query, n_item, k))}
    if not no_torch:
        users_t = torch.from_numpy(users).cuda()
        tus, treps = timed(lambda: torch_topk(tables, users_t, k, mask), window)
        _, items = engine.recommend(tables, d, users, k, excl)
        _, titems = torch_topk(tables, users_t, k, mask)
        a, b = items.cpu().numpy(), titems.cpu().numpy()
        differ = sum(set(a[q].tolist()) != set(b[q].tolist()) for q in range(n_query))
        out.update({'torch_us': round(tus, 1), 'torch_calls': treps, 'speedup_vs_torch': round(tus / us, 3), 'topk_sets_differing': int(differ)})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3,s128')
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--no-torch', action='store_true', help='time the kernel only (for a rocprofv3 run)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for name in a.shapes.split(','):
        run(name, a.window, a.no_torch)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
