"""Exact full-catalogue ranks (engine.rank_pairs -> ure_rank_pairs) against top-k recommendation at k = 10 on the same inputs
(the scoring is shared) and against the plain torch composition (per-shard matmul, mean, masked sort, searchsorted: it does
NOT reproduce the ensemble's scores or break ties by id).  One JSON line per shape.

    python tools/exp_rank.py [--shapes ml1m,cfg3] [--window 1.0] [--no-torch]

Tables are random normal (the kernels' cost does not depend on the values); targets and the exclusion set are random at the
given sizes.  Times are device events around back-to-back calls after a warm-up, over a window of about --window seconds;
kernel times alone come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--no-torch).
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

SHAPES = {
    # name: (n_user, n_query, n_item, S, d, targets per user (mean), exclusion density)
    'ml1m': (6040, 6040, 3416, 5, 32, 33, 0.048),        # ml-1m: ~200 k test pairs, the 991 k training pairs excluded
    'cfg3': (162541, 4096, 60000, 32, 128, 50, 0.0),     # BASELINE.json configs[3]: 32 shards, 60 k items, d = 128
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


def torch_ranks(tables, users_t, mask, tq, tpos, titems):
    """The composition a torch user would write: the [n_query, n_item] mean score matrix, excluded items at -inf, rows sorted,
    each target's count of greater scores by searchsorted (ties are not broken by id; the sums are the GEMM's)."""
    acc = None
    for U, V in tables:
        s = U[users_t] @ V.T
        acc = s if acc is None else acc + s
    acc = acc / len(tables)
    ts = acc[tq, titems]
    if mask is not None:
        acc = acc.masked_fill(mask, float('-inf'))
    srt, _ = torch.sort(acc, dim=1)
    tmax = int(tpos.max()) + 1 if tpos.numel() else 1
    pad = torch.full((acc.shape[0], tmax), float('inf'), device=acc.device)
    pad[tq, tpos] = ts
    r = acc.shape[1] - torch.searchsorted(srt, pad, right=True)
    return r[tq, tpos]


def run(name, window, no_torch):
    n_user, n_query, n_item, S, d, per_user, dens = SHAPES[name]
    g = torch.Generator(device='cuda').manual_seed(0)
    tables = [(torch.randn(n_user, d, device='cuda', generator=g), torch.randn(n_item, d, device='cuda', generator=g)) for _ in range(S)]
    rng = np.random.default_rng(1)
    users = rng.choice(n_user, n_query, replace=False)
    counts = rng.poisson(per_user, n_query)
    tgt = [rng.choice(n_item, min(c, n_item), replace=False).astype(np.int32) for c in counts]
    t_off = np.zeros(n_query + 1, dtype=np.int64)
    np.cumsum(counts, out=t_off[1:])
    targets = (t_off, np.concatenate(tgt))
    excl, mask = None, None
    if dens > 0:
        rows = []
        for t in tgt:
            r = np.flatnonzero(rng.random(n_item) < dens)
            rows.append(np.setdiff1d(r, t).astype(np.int32))          # training and test pairs are disjoint
        e_off = np.zeros(n_query + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rows], out=e_off[1:])
        excl = (e_off, np.concatenate(rows))
        mask = torch.zeros(n_query, n_item, dtype=torch.bool)
        mask[torch.from_numpy(np.repeat(np.arange(n_query), np.diff(e_off))), torch.from_numpy(excl[1].astype(np.int64))] = True
        mask = mask.cuda()
    us, reps = timed(lambda: engine.rank_pairs(tables, d, users, targets, excl), window)
    rec_us, rec_reps = timed(lambda: engine.recommend(tables, d, users, 10, excl), window)
    n_t = len(targets[1])
    out = {'shape': name, 'n_query': n_query, 'n_item': n_item, 'S': S, 'd': d, 'targets': int(n_t),
           'max_targets_per_user': int(counts.max()), 'excluded': int(len(excl[1])) if excl else 0,
           'rank_us': round(us, 1), 'calls': reps, 'recommend_k10_us': round(rec_us, 1), 'recommend_calls': rec_reps,
           'rank_over_recommend': round(us / rec_us, 3),
           'scratch_bytes': int(engine.nv.lib().ure_rank_pairs_scratch(n_query, n_t, n_item, d))}
    if not no_torch:
        users_t = torch.from_numpy(users).cuda()
        tq = torch.from_numpy(np.repeat(np.arange(n_query), counts)).cuda()
        tpos = torch.from_numpy(np.concatenate([np.arange(c) for c in counts])).cuda()
        titems = torch.from_numpy(targets[1].astype(np.int64)).cuda()
        tus, treps = timed(lambda: torch_ranks(tables, users_t, mask, tq, tpos, titems), window)
        a = engine.rank_pairs(tables, d, users, targets, excl).cpu().numpy()
        b = torch_ranks(tables, users_t, mask, tq, tpos, titems).cpu().numpy()
        out.update({'torch_us': round(tus, 1), 'torch_calls': treps, 'speedup_vs_torch': round(tus / us, 3),
                    'torch_ranks_differing': int((a != b).sum()), 'torch_note': 'torch scores are not the ensemble\'s; ties not by id'})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--no-torch', action='store_true', help='time the kernels only (for a rocprofv3 run)')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for name in a.shapes.split(','):
        run(name, a.window, a.no_torch)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
