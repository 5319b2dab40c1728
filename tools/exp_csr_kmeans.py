"""k-means / balanced k-means on the sparse rating matrix (csrc/csr_kmeans.hip) measured on the GPU.  One JSON line.

    python tools/exp_csr_kmeans.py [--shapes ml1m,cfg3] [--reps 7] [--step-timeout 600]

Per shape (ml1m: 6,040 x 3,416 with the 896,914 synthetic training ratings, k = 5; cfg3: 162,000 x 60,000 with 22.5 M ratings,
k = 32; values = rating / 5 rounded to float16 as readSparseMat holds them; centroids = k sampled rows, labels = the balanced
fill of their distances), medians of --reps calls after two warm-up calls with (min, max) beside every median:
  cost_ms            one engine.csr_kmeans_cost call (the csq launch and the main kernel), device events
  csq_ms             the csq launch of a cost call on its own: the same call on a one-row, one-entry matrix against the same Ct
  centroids_ms       one engine.csr_kmeans_centroids call (counts and the owner-computes kernel), device events
  dense_cost_ms, dense_centroids_ms
                     ure_kmeans_cost / ure_kmeans_centroids on the dense [n, n_item] array, where it fits (dense_mb below
                     --dense-limit-mb), and whether the two routes agree bit for bit
  fill_ms            one engine.balanced_fill call at capacity ceil(n / k) on the cost call's matrix; it synchronises once per
                     round, so the host's clock around the call and a final synchronise; fill_rounds beside it
  host_fill_ms       what it replaces, as the dense route runs it: the [n, k] matrix to the host, then ure_host_kmeans_assign
                     (the keys, the sort, the walk and the inertia); the host's clock; and whether the labels are equal
  argmin_ms          engine.balanced_fill at capacity 0, device events
  kmeans_ms          one whole kmeans(k, n, (csr, csc), balanced=True) call -- the upload, n_init = 5 runs of up to 10 rounds --
                     on the host's clock; run_rounds: the fill's round count in every k-means round of one run
  dense_kmeans_ms    the same call on the dense array (the route a wide SciPy matrix took before), where it fits
  peak_mb            peak device memory of the whole CSR kmeans call beside dense_mb, what the n_user x n_item float32 array
                     of the dense route would take
Every shape runs in a child process of its own under --step-timeout seconds; after a child that fails or runs out of time
nothing more is started.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SHAPES = {'ml1m': ('ML1M', 5), 'cfg3': ('ML25M', 32)}


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


def host_ms(fn, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def shape_times(name, reps, dense_limit_mb):
    import torch
    from scipy import sparse
    from ultrare_amd import _native as nv
    from ultrare_amd import engine, synth
    from ultrare_amd import sparse_group as sg
    from ultrare_amd.method import utils
    spec, k = getattr(synth, SHAPES[name][0]), SHAPES[name][1]
    uid, iid, r = synth.make_dataset(**spec)['train']
    n, n_item = spec['n_user'], spec['n_item']
    val = (r / 5).astype(np.float16).astype(np.float32)
    halves = sg.canonical_csr(sparse.coo_matrix((val, (uid, iid)), shape=(n, n_item)))
    csr, csc = halves
    rs = np.random.RandomState(0)
    cen_idx = rs.choice(n, k, replace=False)
    C = sg.dense_rows(csr, cen_idx)
    capacity = int(np.ceil(n / k))
    dense_mb = n * n_item * 4 / 2**20
    out = {'shape': name, 'n': n, 'n_item': n_item, 'nnz': csr.nnz, 'k': k, 'capacity': capacity, 'longest_row': int(np.diff(csr.off).max()),
           'longest_column': int(np.diff(csc.off).max()), 'dense_mb': round(dense_mb, 1), 'ct_mb': round(n_item * k * 4 / 2**20, 2)}
    L, st = nv.lib(), nv.stream_handle()

    # the whole call first, in a clean allocator: its peak is the route's
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    np.random.seed(0)
    utils.kmeans(k, n, halves, balanced=True)
    torch.cuda.synchronize()
    out['peak_mb'] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)

    def whole():
        np.random.seed(0)
        utils.kmeans(k, n, halves, balanced=True)
    out['kmeans_ms'] = host_ms(whole, 3, warmup=0)

    S = engine.CsrSet(halves)
    np.random.seed(0)
    run_rounds = []
    utils._single_kmeans_csr(k, n, S, True, 10, rounds=run_rounds)
    out['run_rounds'] = run_rounds

    Ct = torch.from_numpy(np.ascontiguousarray(C.T)).cuda()
    dist = engine.csr_kmeans_cost(S, Ct, k)
    label_d, fill_rounds = engine.balanced_fill(dist, capacity)
    out['fill_rounds'] = fill_rounds
    out['cost_ms'] = event_ms(lambda: engine.csr_kmeans_cost(S, Ct, k), reps)
    one_row = engine.CsrSet(sparse.csr_matrix((np.ones(1, dtype=np.float32), np.zeros(1, dtype=np.int32), np.array([0, 1])), shape=(1, n_item)))
    out['csq_ms'] = event_ms(lambda: engine.csr_kmeans_cost(one_row, Ct, k), reps)
    out['centroids_ms'] = event_ms(lambda: engine.csr_kmeans_centroids(S, label_d, k), reps)
    out['fill_ms'] = host_ms(lambda: engine.balanced_fill(dist, capacity), reps)
    out['argmin_ms'] = event_ms(lambda: engine.balanced_fill(dist, 0), reps)

    # what the fill replaces, as the dense route runs it: the matrix to the host, the keys, the sort, the walk, the inertia
    host_label = np.empty(n, dtype=np.int32)
    inertia = ctypes.c_double(0.0)

    def host_fill():
        host = dist.cpu().numpy()
        nv.check(L.ure_host_kmeans_assign(host.ctypes.data, n, k, capacity, host_label.ctypes.data, ctypes.byref(inertia)), 'ure_host_kmeans_assign')
    out['host_fill_ms'] = host_ms(host_fill, min(reps, 3))
    out['fill_equals_host'] = bool(np.array_equal(label_d.cpu().numpy(), host_label))

    if dense_mb <= dense_limit_mb:
        Xd = torch.from_numpy(sg.dense_rows(csr, np.arange(n))).cuda()
        cent_d = torch.from_numpy(C).cuda()
        dense_dist = torch.empty(n, k, dtype=torch.float32, device='cuda')
        dense_cent = torch.empty(k, n_item, dtype=torch.float32, device='cuda')
        counts = torch.empty(k, dtype=torch.int32, device='cuda')
        out['dense_cost_ms'] = event_ms(lambda: nv.check(L.ure_kmeans_cost(nv.ptr(Xd), nv.ptr(cent_d), n, k, n_item, nv.ptr(dense_dist), st), 'ure_kmeans_cost'), reps)
        out['dense_centroids_ms'] = event_ms(lambda: nv.check(L.ure_kmeans_centroids(nv.ptr(Xd), nv.ptr(label_d), n, k, n_item, nv.ptr(dense_cent),
                                                                                    nv.ptr(counts), st), 'ure_kmeans_centroids'), min(reps, 3), warmup=1)
        new_Ct, _ = engine.csr_kmeans_centroids(S, label_d, k)
        out['routes_agree_bitwise'] = bool(torch.equal(dense_dist.view(torch.int32), dist.view(torch.int32)) and
                                           torch.equal(dense_cent.view(torch.int32), new_Ct.T.contiguous().view(torch.int32)))
        del Xd
        dense = sg.dense_rows(csr, np.arange(n))

        def dense_whole():
            np.random.seed(0)
            utils.kmeans(k, n, dense, balanced=True)
        out['dense_kmeans_ms'] = host_ms(dense_whole, 1, warmup=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--step-timeout', type=int, default=600)
    ap.add_argument('--dense-limit-mb', type=float, default=4096.0)
    ap.add_argument('--child', default=None, help='(internal) measure this one shape in this process')
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('exp_csr_kmeans needs the GPU: nothing is measured on the host')
        res = shape_times(a.child, a.reps, a.dense_limit_mb)
        res['gpu'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'reps': a.reps, 'shapes': []}
    for name in [s for s in a.shapes.split(',') if s]:
        if name not in SHAPES:
            raise SystemExit(f'unknown shape {name!r}: {sorted(SHAPES)}')
        # a fresh child per shape under its own time limit; after a failure nothing more is started on the GPU
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', name, '--reps', str(a.reps), '--dense-limit-mb',
                                str(a.dense_limit_mb)], capture_output=True, text=True, timeout=a.step_timeout)
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
