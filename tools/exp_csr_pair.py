"""The pair-distance reductions on the sparse rating matrix (the CSR tile producer of csrc/pair_dist.hip) measured on
the GPU.  One JSON line.

    python tools/exp_csr_pair.py [--shapes ml1m,cfg3] [--reps 3] [--step-timeout 500] [--full-limit-s 60]

Per shape (ml1m: 6,040 x 3,416 with the 896,914 synthetic training ratings; cfg3: 162,000 x 60,000 with 22.5 M ratings; values =
the ratings 1 .. 5 as float32) and per metric (euclidean, cosine, manhattan), medians of --reps calls after one warm-up call
with (min, max) beside every median, device events:
  knn_ms        engine.pair_knn(CsrSet, 10): ten neighbours of every user
  rowsum_ms     engine.pair_rowsum(CsrSet)
  lpa_ms        one label propagation round's device part, engine.pair_label_expsum(CsrSet, label, k = 8)
  dense_*_ms    the same three calls on the densified [n, n_item] array, where it fits below --dense-limit-mb, and whether the
                two routes agree bit for bit
  csr_peak_mb, dense_peak_mb
                peak device memory over upload and one kNN call, per route
A full pass costs n^2 / 2 pair merges however few rows are asked, so at a shape where nobody knows the time the tool first runs
kNN for --probe-rows query rows against all users (knn_probe_ms) and extrapolates to all rows (knn_estimate_s, by the count
of row tiles).  Only when the estimate is below --full-limit-s seconds are the full calls of that metric run, one call each;
otherwise they are 'not measured'.  Every shape runs in a child process of its own under --step-timeout seconds; after a child
that fails or runs out of time nothing more is started.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SHAPES = {'ml1m': 'ML1M', 'cfg3': 'ML25M'}
METRICS = ('euclidean', 'cosine', 'manhattan')
LPA_K = 8


def spread(ts):
    return {'median': round(float(np.median(ts)), 3), 'min': round(min(ts), 3), 'max': round(max(ts), 3)}


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
    return spread(ts)


def peak_mb(make_source):
    import torch
    from ultrare_amd import engine
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    src = make_source()
    engine.pair_knn(src, 10, 'euclidean', np.arange(64))
    torch.cuda.synchronize()
    return src, round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)


def shape_times(name, reps, dense_limit_mb, probe_rows, full_limit_s):
    import torch
    from scipy import sparse
    from ultrare_amd import engine, synth
    from ultrare_amd import sparse_group as sg
    spec = getattr(synth, SHAPES[name])
    uid, iid, r = synth.make_dataset(**spec)['train']
    n, n_item = spec['n_user'], spec['n_item']
    halves = sg.canonical_csr(sparse.coo_matrix((r.astype(np.float32), (uid, iid)), shape=(n, n_item)))
    csr = halves[0]
    lens = np.diff(csr.off)
    dense_mb = n * n_item * 4 / 2**20
    out = {'shape': name, 'n': n, 'n_item': n_item, 'nnz': csr.nnz, 'longest_row': int(lens.max()), 'median_row': int(np.median(lens)),
           'dense_mb': round(dense_mb, 1), 'lpa_k': LPA_K, 'probe_rows': probe_rows, 'metrics': {}}
    S, out['csr_peak_mb'] = peak_mb(lambda: engine.CsrSet.from_device(
        n, n_item, torch.from_numpy(csr.off).cuda(), torch.from_numpy(csr.idx).cuda(), torch.from_numpy(csr.val).cuda()))
    label = np.random.RandomState(0).randint(0, LPA_K, n)
    probe = np.random.RandomState(1).choice(n, min(probe_rows, n), replace=False)
    row_tiles = -(-n // 64)
    Xd = None
    if dense_mb <= dense_limit_mb:
        Xd, out['dense_peak_mb'] = peak_mb(lambda: torch.from_numpy(sg.dense_rows(csr, np.arange(n))).cuda())
    for metric in METRICS:
        m = out['metrics'][metric] = {}
        m['knn_probe_ms'] = event_ms(lambda: engine.pair_knn(S, 10, metric, probe), reps)
        m['knn_estimate_s'] = round(m['knn_probe_ms']['median'] * row_tiles / -(-len(probe) // 64) / 1e3, 2)
        if m['knn_estimate_s'] > full_limit_s:
            m['knn_ms'] = m['rowsum_ms'] = m['lpa_ms'] = 'not measured'
            continue
        full_reps = reps if m['knn_estimate_s'] < 2 else 1
        warm = 1 if m['knn_estimate_s'] < 2 else 0
        m['knn_ms'] = event_ms(lambda: engine.pair_knn(S, 10, metric), full_reps, warm)
        m['rowsum_ms'] = event_ms(lambda: engine.pair_rowsum(S, metric), full_reps, warm)
        m['lpa_ms'] = event_ms(lambda: engine.pair_label_expsum(S, label, LPA_K, metric), full_reps, warm)
        if Xd is not None:
            m['dense_knn_ms'] = event_ms(lambda: engine.pair_knn(Xd, 10, metric), full_reps, warm)
            m['dense_rowsum_ms'] = event_ms(lambda: engine.pair_rowsum(Xd, metric), full_reps, warm)
            m['dense_lpa_ms'] = event_ms(lambda: engine.pair_label_expsum(Xd, label, LPA_K, metric), full_reps, warm)
            a, b = engine.pair_knn(S, 10, metric), engine.pair_knn(Xd, 10, metric)
            same = torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
            same = same and torch.equal(engine.pair_rowsum(S, metric).view(torch.int32), engine.pair_rowsum(Xd, metric).view(torch.int32))
            same = same and torch.equal(engine.pair_label_expsum(S, label, LPA_K, metric).view(torch.int64),
                                        engine.pair_label_expsum(Xd, label, LPA_K, metric).view(torch.int64))
            m['routes_agree_bitwise'] = bool(same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--step-timeout', type=int, default=500)
    ap.add_argument('--dense-limit-mb', type=float, default=4096.0)
    ap.add_argument('--probe-rows', type=int, default=1024)
    ap.add_argument('--full-limit-s', type=float, default=60.0)
    ap.add_argument('--child', default=None, help='(internal) measure this one shape in this process')
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('exp_csr_pair needs the GPU: nothing is measured on the host')
        res = shape_times(a.child, a.reps, a.dense_limit_mb, a.probe_rows, a.full_limit_s)
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
                                str(a.dense_limit_mb), '--probe-rows', str(a.probe_rows), '--full-limit-s', str(a.full_limit_s)],
                               capture_output=True, text=True, timeout=a.step_timeout)
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
        print(f'{name}: measured', file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    if 'stopped' in out:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
