"""The LightGCN backbone (csrc/gcn.hip) measured on the GPU against torch compositions of the same arithmetic.  One JSON line.

    python tools/exp_lightgcn.py [--shapes ml1m,cfg3] [--reps 7] [--step-timeout 600]

Per shape -- one shard of a 5-shard ml-1m call (1,208 users x 3,416 items, 180 k ratings, d = 32) and one of BASELINE.json configs[3]
(5,062 users x 60,000 items, 703 k ratings, d = 128), both synthetic (synth.make_dataset: log-normal user activity, 1 / rank item
popularity), L = 2, B = 30,000 -- medians of --reps calls after two warm-up calls, (min, max) beside every median, device events
around the launches:
  propagate_csr_ms, propagate_csc_ms   one engine.gcn_propagate per side (users from items; items from users: the side with the
                                       long rows), with the algorithmic bytes nnz (4 + 4 d) + rows 4 d of each and the fraction of
                                       8 TB/s they come to at the median
  sparse_mm_csr_ms, sparse_mm_csc_ms   the float32 torch composition of the same products: torch.sparse.mm of the normalised
                                       adjacency (a CSR tensor with the values s_dst s_src, built once outside the clock) with X
  step_ms                              one training step of engine.GcnJob (forward, residual, two gradient walks, backward, update);
                                       launches_per_step beside it, and the step's parts timed apart: forward_ms, loss_grad_ms,
                                       backward_ms, update_ms
  torch_step_ms                        one step of the torch composition: sparse.mm forward under autograd, MSELoss(sum) on the
                                       batch, backward, torch.optim.SGD(momentum, weight_decay); the adjacency as a coalesced COO tensor
  peak_mb, torch_peak_mb               peak device memory of either route above what the graph and the tables held before the step
  walk_multiple                        what a masked walk reads per step over what the batch needs: nnz / B
Every shape runs in a child process of its own under --step-timeout seconds; after a child that fails or runs out of time nothing
more is started.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

# (a tenth of the ratings held out, as the real sets do: synth.make_dataset keeps at least one test rating per user)
SHAPES = {'ml1m': (dict(n_user=1208, n_item=3416, n_train=180000, n_test=20000), 32), 'cfg3': (dict(n_user=5062, n_item=60000, n_train=703000, n_test=78000), 128)}
LAYERS, BATCH, HBM_TBS = 2, 30000, 8.0


def spread(ts):
    return {'median': round(float(np.median(ts)), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}


def event_ms(fn, reps, warmup=2):
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
    return spread(ts)


def peak_mb(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)


def shape_times(name, reps):
    import torch
    from ultrare_amd import engine, lightgcn, synth
    spec, d = SHAPES[name]
    uid, iid, r = synth.make_dataset(**spec)['train']
    n_user, n_item, N = spec['n_user'], spec['n_item'], len(uid)
    graph = engine.GcnGraph(uid, iid, (r / 5).astype(np.float32), n_user, n_item)
    g = graph.host
    rs = np.random.RandomState(0)
    P0, Q0 = (rs.standard_normal((n_user, d)) * 0.1).astype(np.float32), (rs.standard_normal((n_item, d)) * 0.1).astype(np.float32)
    out = {'shape': name, 'n_user': n_user, 'n_item': n_item, 'nnz': N, 'd': d, 'layers': LAYERS, 'batch': BATCH, 'walk_multiple': round(N / BATCH, 1),
           'longest_user_row': int(np.diff(g.off_u).max()), 'longest_item_row': int(np.diff(g.off_i).max()),
           'median_user_row': int(np.median(np.diff(g.off_u))), 'median_item_row': int(np.median(np.diff(g.off_i)))}
    Pd, Qd = torch.from_numpy(P0).cuda(), torch.from_numpy(Q0).cuda()

    # ---- one propagate per side against torch.sparse.mm of the normalised adjacency
    def adjacency(side):
        off, idx, s_src, s_dst, n_dst, n_src = g.side(side)
        val = np.repeat(s_dst, np.diff(off)) * s_src[idx]
        return torch.sparse_csr_tensor(torch.from_numpy(off), torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(val.astype(np.float32)),
                                       size=(n_dst, n_src)).cuda()
    for side, X, rows in (('csr', Qd, n_user), ('csc', Pd, n_item)):
        A = adjacency(side)
        buf = torch.empty(rows, d, dtype=torch.float32, device='cuda')
        mine = event_ms(lambda: engine.gcn_propagate(graph, side, X, out=buf), reps)
        theirs = event_ms(lambda: torch.sparse.mm(A, X), reps)
        nbytes = N * (4 + 4 * d) + rows * 4 * d
        out[f'propagate_{side}_ms'], out[f'sparse_mm_{side}_ms'] = mine, theirs
        out[f'propagate_{side}_bytes'] = nbytes
        out[f'propagate_{side}_hbm_fraction'] = round(nbytes / (mine['median'] * 1e-3) / (HBM_TBS * 1e12), 4)
        ref = torch.sparse.mm(A, X)
        out[f'propagate_{side}_max_diff_from_sparse_mm'] = float((engine.gcn_propagate(graph, side, X) - ref).abs().max())
        del A, ref

    # ---- one training step of the job, and its parts
    epochs = 2
    orders = np.stack([rs.permutation(N) for _ in range(epochs)]).astype(np.int32)
    lr, lam, mu = 1e-3, 0.1, 0.9

    def make_job():
        return engine.GcnJob(graph, (P0, Q0), orders, d, LAYERS, BATCH, epochs, lr, lam, mu)
    job = make_job()
    out['steps_per_epoch'] = job.steps
    out['launches_per_step'] = 4 * LAYERS + 7
    job._step(0, 0)
    out['peak_mb'] = peak_mb(lambda: job._step(0, 1))
    out['job_tables_mb'] = round(job._pool.numel() * 4 / 2**20, 1)
    state = {'s': 2}

    def one_step():
        job._step(0, state['s'] % job.steps)
        state['s'] += 1
    out['step_ms'] = event_ms(one_step, reps)

    def forward():
        job._star_at = -1
        job._forward()
    out['forward_ms'] = event_ms(forward, reps)
    tag = engine.gcn_step_tags(graph, orders[0], BATCH)
    U, V = job.padded_tables(0)
    out['loss_grad_ms'] = event_ms(lambda: engine.gcn_loss_grad(graph, tag, 1, U, V), reps)

    def backward():
        src = job._t['G']
        for l in range(LAYERS):
            dst = job._t['Xa'] if l % 2 == 0 else job._t['Xb']
            job._layer(src, dst, job._t['G'], None, None)
            src = dst
    out['backward_ms'] = event_ms(backward, reps)
    w, m, gr = torch.zeros_like(job._t['W']), torch.zeros_like(job._t['W']), torch.zeros_like(job._t['W'])
    out['update_ms'] = event_ms(lambda: engine.gcn_sgd_step(w, m, gr, lr, lam, mu, False, gscale=1 / 3), reps)
    job.close()
    del w, m, gr

    # ---- the torch composition: sparse forward under autograd, MSELoss(sum), SGD
    A, At = adjacency('csr').to_sparse_coo().coalesce(), adjacency('csc').to_sparse_coo().coalesce()      # (COO: the layout torch's sparse autograd takes)
    P, Q = Pd.clone().requires_grad_(True), Qd.clone().requires_grad_(True)
    opt = torch.optim.SGD([P, Q], lr=lr, momentum=mu, weight_decay=lam)
    loss_fn = torch.nn.MSELoss(reduction='sum')
    uid_d, iid_d = torch.from_numpy(uid.astype(np.int64)).cuda(), torch.from_numpy(iid.astype(np.int64)).cuda()
    r_d = torch.from_numpy((r / 5).astype(np.float32)).cuda()
    order_d = torch.from_numpy(orders[0].astype(np.int64)).cuda()
    c = float(lightgcn.layer_scale(LAYERS))
    state = {'s': 0}

    def torch_step():
        s = state['s'] % (N // BATCH)
        state['s'] += 1
        idx = order_d[s * BATCH:(s + 1) * BATCH]
        opt.zero_grad()
        Xu, Xi, Su, Si = P, Q, P, Q
        for _ in range(LAYERS):
            Xu, Xi = torch.sparse.mm(A, Xi), torch.sparse.mm(At, Xu)
            Su, Si = Su + Xu, Si + Xi
        loss = loss_fn(((Su * c)[uid_d[idx]] * (Si * c)[iid_d[idx]]).sum(1), r_d[idx])
        loss.backward()
        opt.step()
    torch_step()
    out['torch_peak_mb'] = peak_mb(torch_step)
    out['torch_step_ms'] = event_ms(torch_step, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--step-timeout', type=int, default=600)
    ap.add_argument('--child', default=None, help='(internal) measure this one shape in this process')
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('exp_lightgcn needs the GPU: nothing is measured on the host')
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
