"""The distance-matrix reductions of csrc/pair_dist.hip (engine.pair_knn / pair_rowsum / pair_label_expsum) at the ml-1m user
shape and at BASELINE.json configs[3] (162,000 users, d = 128), beside a chunked torch composition of the kNN (torch.cdist +
topk over row blocks: the dot-product expansion on the matrix cores, no exact tie rule).  One JSON line per shape.

    python tools/exp_cluster.py [--shapes ml1m,cfg3] [--window 1.0] [--no-torch]

Embeddings are random normal (the kernels' cost does not depend on the values).  Times are device events around back-to-back
calls after a warm-up, over a window of about --window seconds.  `elem_ops` counts the n * n * d difference terms of one pass.
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

SHAPES = {'ml1m': (6040, 32), 'cfg3': (162000, 128)}


def timed(fn, window):
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
    return a.elapsed_time(b) / reps, reps            # ms per call


def torch_knn(X, k, block=4096):
    out = []
    for i in range(0, X.shape[0], block):
        out.append(torch.cdist(X[i:i + block], X).topk(k, dim=1, largest=False))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('exp_cluster needs the GPU: nothing is measured on the host')
    for name in a.shapes.split(','):
        n, d = SHAPES[name]
        X = torch.from_numpy(np.random.default_rng(1).standard_normal((n, d)).astype(np.float32)).cuda()
        label = np.random.default_rng(2).integers(0, 8, size=n)
        res = {'shape': name, 'n': n, 'd': d, 'elem_ops': n * n * d, 'gpu': torch.cuda.get_device_name(0)}
        for metric in ('euclidean', 'cosine', 'manhattan'):
            res[f'knn10_{metric}_ms'], res[f'knn10_{metric}_reps'] = timed(lambda: engine.pair_knn(X, 10, metric), a.window)
        res['rowsum_euclidean_ms'], _ = timed(lambda: engine.pair_rowsum(X, 'euclidean'), a.window)
        res['lpa_expsum_k8_euclidean_ms'], _ = timed(lambda: engine.pair_label_expsum(X, label, 8, 'euclidean'), a.window)
        if not a.no_torch:
            res['torch_cdist_topk10_ms'], _ = timed(lambda: torch_knn(X, 10), a.window)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
