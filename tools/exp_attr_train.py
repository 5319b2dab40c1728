"""In-training attribute unlearning (csrc/attr_train.hip) measured on the GPU.  One JSON line.

    python tools/exp_attr_train.py [--shapes shard-L0,shard-L2,fullmf] [--reps 5] [--step-timeout 600]

Per shape a synthetic shard (seeded; user activity skewed as 1 / rank^0.7, two attribute groups of every other user):
  shard-L0, shard-L2  an ml-1m SISA shard: 1,208 users x 3,416 items, 200,000 ratings, d = 32, B = 30,000, layers 0 and 2 -- nearly
                      every user is in every batch
  fullmf              a full-MF-like shape: 6,040 users x 3,416 items, 1,000,000 ratings, d = 16, B = 3,000, layers 0 -- a batch
                      selects a strict subset of the users
and per dis_type ('d2d', 'u2u'), device time by events on the stream, medians over --reps epochs after one warm-up epoch with
(min, max) beside every median:
  step_ms / plain_step_ms   an optimizer step of the job with the term / of the same job without it (an epoch's time over its steps)
  term_ms                   the selection, the loss at device counts and the hand-off of one step (GcnJob._attr_term) alone, and
                            term_share = term_ms / step_ms
  masks_ms                  the per-epoch mask pass (ure_attr_step_masks)
  torch_term_ms             the torch composition of one step's term: autograd through a cdist-based MMD (or the bipartite sum of
                            squared distances) on the batch's rows of the same table, the rows read from the device selection
  rows                      (n1, n2) of that step; peak_mb / plain_peak_mb: peak device memory of the job and one epoch over what was
                            allocated before it
Every shape runs in a child process of its own under --step-timeout seconds; after a child that fails or runs out of time nothing
more is started."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

# n_user, n_item, N, d, B, layers
SHAPES = {'shard-L0': (1208, 3416, 200_000, 32, 30_000, 0), 'shard-L2': (1208, 3416, 200_000, 32, 30_000, 2), 'fullmf': (6040, 3416, 1_000_000, 16, 3_000, 0)}


def stats(ts):
    return {'median': round(float(np.median(ts)), 4), 'min': round(float(min(ts)), 4), 'max': round(float(max(ts)), 4)}


def event_ms(fn, reps, warmup=1):
    import torch
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
    return ts


def triples(n_user, n_item, N, seed=11):
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, n_user + 1) ** 0.7
    uid = rs.choice(n_user, N, p=p / p.sum())
    uid[:n_user] = np.arange(n_user)                        # every user has a rating
    return uid, rs.randint(0, n_item, N), (rs.randint(1, 6, N) / 5).astype(np.float32)


def shape_times(name, reps):
    import torch
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    n_user, n_item, N, d, B, layers = SHAPES[name]
    uid, iid, rating = triples(n_user, n_item, N)
    rs = np.random.RandomState(5)
    init = (0.1 * rs.standard_normal((n_user, d)).astype(np.float32), 0.1 * rs.standard_normal((n_item, d)).astype(np.float32))
    epochs = reps + 1
    orders = np.stack([rs.permutation(N) for _ in range(epochs)]).astype(np.int32)
    id1, id2 = np.arange(0, n_user, 2), np.arange(1, n_user, 2)
    graph = engine.GcnGraph(uid, iid, rating, n_user, n_item)
    out = {'shape': name, 'n_user': n_user, 'n_item': n_item, 'N': N, 'd': d, 'B': B, 'layers': layers, 'steps': (N + B - 1) // B}

    def epochs_ms(job):
        return [t / job.steps for t in event_ms(lambda: job.run_epochs(1), reps)]

    def job_of(**kw):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        job = engine.GcnJob(graph, init, orders, d, layers, B, epochs, 1e-3, 0.1, 0.9, **kw)
        ts = epochs_ms(job)
        return job, ts, round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)

    plain, ts, out['plain_peak_mb'] = job_of()
    out['plain_step_ms'] = stats(ts)
    plain.close()
    for var in ('d2d', 'u2u'):
        job, ts, peak = job_of(attr=(id1, id2), dis_type=var, eta=1e-3)
        r = {'step_ms': stats(ts), 'peak_mb': peak, 'skipped': job.epoch_skipped().tolist()}
        st, a = nv.stream_handle(), job._attr
        U, Gu = job._sides(job._t['Star'])[0], job._sides(job._t['G'])[0]
        s = job.steps // 2
        r['term_ms'] = stats(event_ms(lambda: job._attr_term(0, s, U, Gu, st), max(reps, 5)))
        r['term_share'] = round(r['term_ms']['median'] / r['step_ms']['median'], 4)
        r['masks_ms'] = stats(event_ms(lambda: engine._attr_masks(graph, job._tag, a['groups'].group, job.steps, a['masks'], st), max(reps, 5)))
        n1, n2 = (int(x) for x in a['counts'].cpu())
        r['rows'] = [n1, n2]
        rows = a['rows'][:n1 + n2].long()
        X = U[:, :d].detach().clone()

        def torch_term():
            Xg = X.clone().requires_grad_(True)
            x = Xg[rows]
            D = torch.cdist(x, x) ** 2
            if var == 'u2u':
                loss = D[:n1, n1:].sum()
            else:
                m = n1 + n2
                bw = D.detach().sum() / (m * m - m) / 4.0
                K = sum(torch.exp(-D / (bw * 2.0 ** q)) for q in range(5))
                loss = K[:n1, :n1].mean() + K[n1:, n1:].mean() - K[:n1, n1:].mean() - K[n1:, :n1].mean()
            loss.backward()
            return Xg.grad
        r['torch_term_ms'] = stats(event_ms(torch_term, max(reps, 5)))
        got = a['grad'][:n1 + n2].clone()
        want = torch_term()[rows]
        r['grad_vs_torch_rel'] = float((got - want).abs().max() / want.abs().max())
        job.close()
        out[var] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='shard-L0,shard-L2,fullmf')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step-timeout', type=int, default=600)
    ap.add_argument('--child', default=None, help='(internal) measure this one shape in this process')
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('exp_attr_train needs the GPU: nothing is measured on the host')
        res = shape_times(a.child, a.reps)
        res['gpu'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'reps': a.reps, 'shapes': []}
    for name in [s for s in a.shapes.split(',') if s]:
        if name not in SHAPES:
            raise SystemExit(f'unknown shape {name!r}: {sorted(SHAPES)}')
        # a fresh child per shape under its own time limit; after a failure nothing more is started on the GPU
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', name, '--reps', str(a.reps)], capture_output=True, text=True,
                               timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            out['stopped'] = f'{name}: no result within {a.step_timeout} s'
            break
        lines = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
        if p.returncode != 0 or not lines:
            out['stopped'] = f'{name}: exit {p.returncode}: {p.stderr.strip().splitlines()[-3:]}'
            break
        res = json.loads(lines[-1][7:])
        out['gpu'] = res.pop('gpu')
        out['shapes'].append(res)
    print(json.dumps(out), flush=True)
    if 'stopped' in out:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
