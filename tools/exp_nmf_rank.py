"""Full-catalogue top-10 and test-set ranking under a NeuMF ensemble (csrc/nmf_rank.hip) measured on the GPU against
the two routes that existed before it.  One JSON line per shape.

    python tools/exp_nmf_rank.py [--shapes ml1m,cfg3] [--reps 7] [--yard-users 128]

Shapes: the ml-1m ensemble (6,040 users x 3,416 items, 5 shards, k = 32, layers [64, 32], 4.8 % of every row excluded, 33 test
items a user) and a BASELINE.json configs[3]-like one (4,096 users x 60,000 items, 32 shards, k = 128, layers [128, 64], nothing
excluded, 50 test items a user).  Parameters are random (the kernels' cost does not depend on the values); every shard has its own
tables.  Per shape, medians of --reps calls after two warm-up calls with (min, max) beside them, device events round the calls, one
GPU process, the three routes one after the other:
  recommend_ms, rank_ms          engine.nmf_recommend (top 10) and engine.nmf_rank_pairs of the test pairs
  yard_*                         the composition that existed: engine.nmf_score over all (user, item) pairs in user chunks, one call a
                                 shard, then the mask and torch.topk, or one stable sort a row and a gather for the ranks.  Bit-equal
                                 scores by construction (checked: yard_topk_rows_differing, yard_ranks_differing)
  torch_*                        a torch composition on the matrix cores: per shard the two halves of layer 0 as two matmuls added by
                                 broadcast, nn.Linear layers, the GMF term as a matmul; it does not reproduce the scores
  *_peak_mb                      peak device memory of one call above what was resident before it
At a shape where the composition would take minutes a call it is timed on the first --yard-users users (yard_users in the line), and
so is the new route beside it (recommend_sub_ms, rank_sub_ms): the ratio is of two measurements at the same size.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ultrare_amd import engine, nmf  # noqa: E402

SHAPES = {
    # name: (n_user = n_query, n_item, S, k, layers, exclusion density, test items a user, whether the yardstick runs on a subset)
    'ml1m': (6040, 3416, 5, 32, [64, 32], 0.048, 33, False),
    'cfg3': (4096, 60000, 32, 128, [128, 64], 0.0, 50, True),
    'tiny': (64, 300, 2, 8, [16, 8], 0.05, 5, True),                  # a rehearsal of the script, not a measurement
}
TOP_K = 10


def spread(ts):
    return {'median': round(float(np.median(ts)), 3), 'min': round(min(ts), 3), 'max': round(max(ts), 3)}


def event_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return spread(ts)


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)


def rows_csr(rng, n, n_item, per_row=None, density=None):
    rows = [np.unique(rng.integers(0, n_item, per_row)).astype(np.int32) if per_row else np.flatnonzero(rng.random(n_item) < density).astype(np.int32)
            for _ in range(n)]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, np.concatenate(rows).astype(np.int32)


def sub_csr(c, n):
    return None if c is None else (c[0][:n + 1], c[1][:c[0][n]])


class Chunked:
    """What both compositions share: user chunks, the exclusion mask of a chunk, top-k and ranks from a chunk's score matrix."""

    def __init__(self, n_item, users, excl, targets, chunk):
        self.n_item, self.users, self.chunk = n_item, torch.from_numpy(users).cuda(), chunk
        self.excl = None if excl is None else (torch.from_numpy(excl[0]).cuda(), torch.from_numpy(excl[1].astype(np.int64)).cuda())
        self.t_off, self.t_items = torch.from_numpy(targets[0]).cuda(), torch.from_numpy(targets[1].astype(np.int64)).cuda()

    def masked(self, sc, q0, q1):
        if self.excl is not None:
            off, items = self.excl
            a, b = int(off[q0]), int(off[q1])
            row = torch.repeat_interleave(torch.arange(q1 - q0, device='cuda'), off[q0 + 1:q1 + 1] - off[q0:q1])
            sc[row, items[a:b]] = float('-inf')
        return sc

    def run(self, scores_of, want):
        out = []
        for q0 in range(0, len(self.users), self.chunk):
            q1 = min(q0 + self.chunk, len(self.users))
            sc = self.masked(scores_of(self.users[q0:q1]), q0, q1)
            if want == 'topk':
                out.append(torch.topk(sc, TOP_K, dim=1)[1])
            else:
                pos = torch.empty_like(sc, dtype=torch.int64)
                order = torch.sort(sc, dim=1, descending=True, stable=True)[1]
                pos.scatter_(1, order, torch.arange(self.n_item, device='cuda').expand_as(order))
                a, b = int(self.t_off[q0]), int(self.t_off[q1])
                row = torch.repeat_interleave(torch.arange(q1 - q0, device='cuda'), self.t_off[q0 + 1:q1 + 1] - self.t_off[q0:q1])
                out.append(pos[row, self.t_items[a:b]])
        return torch.cat(out)


def yard_scores(dev, k, layers, n_item):
    """engine.nmf_score over every pair of a user chunk, one call a shard."""
    iid_of = {}

    def scores_of(users):
        n = len(users)
        if n not in iid_of:
            iid_of[n] = torch.arange(n_item, dtype=torch.int32, device='cuda').repeat(n)
        uid = users.to(torch.int32).repeat_interleave(n_item)
        pred = None
        for m, (U, V, dense) in enumerate(dev):
            pred = engine.nmf_score(U, V, dense, k, layers, uid, iid_of[n], pred=pred, n_models_total=len(dev), first=m == 0, last=m == len(dev) - 1)
        return pred.view(n, n_item)
    return scores_of


def torch_scores(dev, k, layers, n_item):
    """The model as matmuls: layer 0 split into its user and item halves, the rest nn.functional.linear, the GMF term a matmul."""
    S = nmf.Shape(k, layers)
    parts = []
    for U, V, dense in dev:
        W, b, h, c = S.unpack(dense)
        parts.append((U, V, W, b, h, c, V[:, k:] @ W[0][:, S.e:].T, (V[:, :k] * h[:k]).contiguous()))

    def scores_of(users):
        acc = None
        for U, V, W, b, h, c, item_half, vg in parts:
            a = torch.relu((U[users, k:] @ W[0][:, :S.e].T + b[0])[:, None, :] + item_half[None, :, :])
            for Wj, bj in zip(W[1:], b[1:]):
                a = torch.relu(torch.nn.functional.linear(a, Wj, bj))
            s = U[users, :k] @ vg.T + a @ h[k:] + c
            acc = s if acc is None else acc + s
        return acc / len(parts)
    return scores_of


def run(name, reps, yard_users):
    n_user, n_item, n_models, k, layers, dens, per_user, subset = SHAPES[name]
    S = nmf.Shape(k, layers)
    g = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *shape, scale: scale * torch.randn(*shape, device='cuda', generator=g)
    dev = [(rnd(n_user, S.wd, scale=0.3), rnd(n_item, S.wd, scale=0.3), rnd(S.n_dense, scale=0.1)) for _ in range(n_models)]
    rng = np.random.default_rng(1)
    users = rng.permutation(n_user).astype(np.int64)
    excl = rows_csr(rng, n_user, n_item, density=dens) if dens > 0 else None
    targets = rows_csr(rng, n_user, n_item, per_row=per_user)
    out = {'shape': name, 'n_query': n_user, 'n_item': n_item, 'S': n_models, 'k': k, 'layers': layers, 'top_k': TOP_K, 'targets': int(len(targets[1])),
           'excluded': int(len(excl[1])) if excl else 0, 'reps': reps, 'forwards': n_user * n_item * n_models,
           'plan_topk': nmf.rank_plan(k, layers, TOP_K), 'plan_rank': nmf.rank_plan(k, layers, None)}
    rec = lambda n=n_user: engine.nmf_recommend(dev, k, layers, users[:n], TOP_K, sub_csr(excl, n))
    rank = lambda n=n_user: engine.nmf_rank_pairs(dev, k, layers, users[:n], sub_csr(targets, n), sub_csr(excl, n))
    out['recommend_ms'], out['rank_ms'] = event_ms(rec, reps), event_ms(rank, reps)
    out['recommend_peak_mb'], out['rank_peak_mb'] = peak_mb(rec), peak_mb(rank)
    ny = min(yard_users, n_user) if subset else n_user
    out['yard_users'] = ny
    if ny != n_user:
        out['recommend_sub_ms'], out['rank_sub_ms'] = event_ms(lambda: rec(ny), reps), event_ms(lambda: rank(ny), reps)
    chunk = max(1, min(ny, (1 << 24) // n_item))                      # 16 M pairs a chunk: 192 MB of ids and scores
    C = Chunked(n_item, users[:ny], sub_csr(excl, ny), sub_csr(targets, ny), chunk)
    for tag, scores_of, ch in (('yard', yard_scores(dev, k, layers, n_item), chunk),
                               ('torch', torch_scores(dev, k, layers, n_item), max(1, min(ny, (1 << 26) // (n_item * max(layers[1:])))))):
        C.chunk = ch
        out[f'{tag}_chunk_users'] = ch
        out[f'{tag}_recommend_ms'] = event_ms(lambda: C.run(scores_of, 'topk'), reps)
        out[f'{tag}_rank_ms'] = event_ms(lambda: C.run(scores_of, 'rank'), reps)
        out[f'{tag}_recommend_peak_mb'], out[f'{tag}_rank_peak_mb'] = peak_mb(lambda: C.run(scores_of, 'topk')), peak_mb(lambda: C.run(scores_of, 'rank'))
        items, ranks = rec(ny)[1], rank(ny)
        titems, tranks = C.run(scores_of, 'topk'), C.run(scores_of, 'rank')
        out[f'{tag}_topk_rows_differing'] = int((items.sort(dim=1)[0] != titems.sort(dim=1)[0]).any(dim=1).sum())
        keep = ranks >= 0                                             # (an excluded target: -1 here, a -inf tie there)
        out[f'{tag}_ranks_differing'] = int((ranks[keep].long() != tranks[keep]).sum())
    new_r, new_k = (out['recommend_sub_ms'] if ny != n_user else out['recommend_ms']), (out['rank_sub_ms'] if ny != n_user else out['rank_ms'])
    for tag in ('yard', 'torch'):
        out[f'{tag}_over_new_recommend'] = round(out[f'{tag}_recommend_ms']['median'] / new_r['median'], 2)
        out[f'{tag}_over_new_rank'] = round(out[f'{tag}_rank_ms']['median'] / new_k['median'], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--yard-users', type=int, default=128)
    a = ap.parse_args()
    if a.reps < 7:
        raise SystemExit('medians of at least seven calls')
    if not torch.cuda.is_available():
        raise SystemExit('exp_nmf_rank needs the GPU: nothing is measured on the host')
    torch.cuda.set_device(0)
    for name in a.shapes.split(','):
        run(name, a.reps, a.yard_users)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
