"""Rating-based OT grouping on the sparse matrix (csrc/csr_group.hip) measured on the GPU.  One JSON line.

    python tools/exp_csr_group.py [--shapes ml1m,cfg3] [--reps 7] [--step-timeout 600]

Per shape (ml1m: 6,040 x 3,416 with the 896,914 synthetic training ratings, k = 5; cfg3: 162,000 x 60,000 with 22.5 M ratings,
k = 32; values = rating / 5 rounded to float16 as readSparseMat holds them; centroids = k sampled rows, labels uniform), device
time by events on the stream, medians of --reps calls after two warm-up calls with (min, max) beside every median:
  cost_ms            one engine.csr_cost call (the cc launch and the main kernel)
  cc_ms              the cc launch of a cost call on its own: engine.csr_cost of a one-row, one-entry matrix against the same Ct (the
                     centroid norms in the contract's order, k workgroups, plus a main kernel with one row to do)
  centroids_ms       one engine.csr_centroids call (counts and the owner-computes kernel)
  torch_cost_ms      the torch composition of the cost: torch.sparse.mm of the float64 CSR with the float64 centroids, the row
                     norms by a second sparse product and the centroid norms, combined as (xx - 2 dot) + cc; and the largest
                     difference between the two cost matrices relative to the largest entry
  torch_centroids_ms the torch composition of the centroids: index_add_ of the float64 values into [k, n_item] by (label of the
                     entry's user, item), divided by the counts
  round_host_ms      one full exact round as ot_cluster runs it (cost, device potentials, the matrix to the host, the exact
                     LP, labels to the device, centroids, centroids to the host), host clock with a synchronise
  peak_mb            peak device memory of the kernel path (the CsrSet, one cost and one centroid call) beside dense_mb, what
                     the n_user x n_item float32 array of the dense route would take
Every shape runs in a child process of its own under --step-timeout seconds; after a child that fails or runs out of time
nothing more is started.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SHAPES = {'ml1m': ('ML1M', 5), 'cfg3': ('ML25M', 32)}


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
    return {'median': round(float(np.median(ts)), 4), 'min': round(min(ts), 4), 'max': round(max(ts), 4)}


def shape_times(name, reps):
    import torch
    from scipy import sparse
    from ultrare_amd import _native as nv
    from ultrare_amd import engine, synth
    from ultrare_amd import sparse_group as sg
    from ultrare_amd.method.utils import ot_warm_iters
    spec, k = getattr(synth, SHAPES[name][0]), SHAPES[name][1]
    uid, iid, r = synth.make_dataset(**spec)['train']
    n, n_item = spec['n_user'], spec['n_item']
    val = (r / 5).astype(np.float16).astype(np.float32)
    halves = sg.canonical_csr(sparse.coo_matrix((val, (uid, iid)), shape=(n, n_item)))
    csr, csc = halves
    rs = np.random.RandomState(0)
    C = sg.dense_rows(csr, rs.choice(n, k, replace=False))
    label = rs.randint(0, k, n)
    out = {'shape': name, 'n': n, 'n_item': n_item, 'nnz': csr.nnz, 'k': k, 'longest_row': int(np.diff(csr.off).max()),
           'longest_column': int(np.diff(csc.off).max()), 'dense_mb': round(n * n_item * 4 / 2**20, 1),
           'ct_mb': round(n_item * k * 4 / 2**20, 2)}

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    S = engine.CsrSet(halves)
    Ct = torch.from_numpy(np.ascontiguousarray(C.T)).cuda()
    label_d = torch.from_numpy(label.astype(np.int32)).cuda()
    dist = engine.csr_cost(S, Ct, k)
    engine.csr_centroids(S, label_d, k)
    torch.cuda.synchronize()
    out['peak_mb'] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
    mine = dist.clone()

    out['cost_ms'] = event_ms(lambda: engine.csr_cost(S, Ct, k), reps)
    one_row = engine.CsrSet(sparse.csr_matrix((np.ones(1, dtype=np.float32), np.zeros(1, dtype=np.int32), np.array([0, 1])), shape=(1, n_item)))
    out['cc_ms'] = event_ms(lambda: engine.csr_cost(one_row, Ct, k), reps)
    out['centroids_ms'] = event_ms(lambda: engine.csr_centroids(S, label_d, k), reps)

    # the torch composition: float64 CSR products and index_add_
    crow, ccol = S.row_off, S.col.long()
    X64 = torch.sparse_csr_tensor(crow, ccol, S.val.double(), size=(n, n_item))
    X64sq = torch.sparse_csr_tensor(crow, ccol, S.val.double() ** 2, size=(n, n_item))
    C64 = torch.from_numpy(C.astype(np.float64)).cuda()
    ones = torch.ones(n_item, 1, dtype=torch.float64, device='cuda')

    def torch_cost():
        dot = torch.sparse.mm(X64, C64.T)                               # [n, k]
        xx = torch.sparse.mm(X64sq, ones)                               # [n, 1]
        cc = (C64 * C64).sum(dim=1)
        return ((xx - 2.0 * dot) + cc[None, :]).clamp_min(0.0).T.float().contiguous()
    item_of_entry = torch.repeat_interleave(torch.arange(n_item, device='cuda'), S.col_off[1:] - S.col_off[:-1])
    v64 = S.cval.double()

    def torch_centroids():
        lab = label_d.long()
        flat = torch.zeros(k * n_item, dtype=torch.float64, device='cuda')
        flat.index_add_(0, lab[S.row.long()] * n_item + item_of_entry, v64)
        counts = torch.bincount(lab, minlength=k)
        return (flat.view(k, n_item) / counts[:, None].double()).float()
    out['torch_cost_ms'] = event_ms(torch_cost, reps)
    theirs = torch_cost()
    out['cost_vs_torch_rel'] = float((mine - theirs).abs().max() / theirs.abs().max())
    out['torch_centroids_ms'] = event_ms(torch_centroids, reps)
    del theirs, X64, X64sq

    # one full exact round as ot_cluster runs it
    L, st = nv.lib(), nv.stream_handle()

    def one_round():
        pi = np.zeros(k, dtype=np.float64)
        d = engine.csr_cost(S, Ct, k)
        nv.check(L.ure_ot_potentials(nv.ptr(d), n, k, ot_warm_iters(n), pi.ctypes.data, None, st), 'ure_ot_potentials')
        host = d.cpu().numpy()
        lab, _, _, _ = nv.ot_assign_warm(host, pi, want_plan=False)
        new_Ct, _ = engine.csr_centroids(S, lab, k)
        return np.ascontiguousarray(new_Ct.cpu().numpy().T)
    one_round()
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_round()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    out['round_host_ms'] = {'median': round(float(np.median(ts)), 3), 'min': round(min(ts), 3), 'max': round(max(ts), 3)}
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
            raise SystemExit('exp_csr_group needs the GPU: nothing is measured on the host')
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
            out['stopped'] = f'{name}: exit {p.returncode}: {p.stderr.strip().splitlines()[-1:] }'
            break
        res = json.loads(lines[-1][7:])
        out['gpu'] = res.pop('gpu')
        out['shapes'].append(res)
    print(json.dumps(out), flush=True)
    if 'stopped' in out:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
