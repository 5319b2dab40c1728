#!/usr/bin/env python3
"""Golden vectors of the user-by-user distance clusterers (utils.py:422-611: findNeighbor, singleLPA / lpa,
singleKmedoids / kmedoids).  Runs ONLY in the build container, through make_golden's harness (the reference on
sys.path, the `ot` stub, stable argsort): it drives the real reference on the toy user embedding kmeans_toy.npz['X']
(n = 1,508, d = 16) and writes inputs and outputs only, to cluster_toy.npz next to this script.

  D_sha256                          sha256 of the given array D (float32 n x n), which is not stored: toy_distances(X),
                                    euclidean distances in float64 rounded once to float32, is bit-reproducible from X
                                    (tests/test_gpu_cluster.py rebuilds it the same way and checks this digest)
  km_k{4,5}_{plain,bal}_*           singleKmedoids on D, 3 seeded runs: labels, inertia, final medoids, initial
                                    medoids; and the labels of kmedoids(n_init=3) from the same seed
  lpa_{plain,bal}_*                 singleLPA (arguments in the right order) on D, k = 4, 3 seeded runs: labels,
                                    inertia, and each user's relative margin between its best and second-best weight
                                    in the last round
  nn_{euclidean,cosine,manhattan}_* findNeighbor(n_neighbor=10) on csr rows: nei_idx, nei_val

usage: python tests/golden/make_golden_cluster.py
"""
import hashlib
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (registers the `ot` stub and puts the reference on sys.path)

RU = MG.RU
N_RUNS = 3


def toy_distances(X):
    """D[u, v] = float32(sqrt(sum_j (x_uj - x_vj)^2)) computed in float64: elementwise IEEE operations, numpy's fixed
    pairwise order over the d = 16 features, one rounding to float32.  Row blocks only bound the temporary's size."""
    X64 = X.astype(np.float64)
    D = np.empty((len(X), len(X)), dtype=np.float32)
    for i in range(0, len(X), 128):
        D[i:i + 128] = np.sqrt(((X64[i:i + 128, None, :] - X64[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    return D


def _spy_choice():
    """Record the arrays np.random.choice returns: singleKmedoids updates its medoid array in place, so the recorded
    object holds the final medoids after the call."""
    seen = []
    orig = np.random.choice

    def spy(*a, **kw):
        r = orig(*a, **kw)
        seen.append((r, r.copy()))
        return r
    return seen, orig, spy


def gen_kmedoids(D, out):
    n = D.shape[0]
    for k in (4, 5):
        for balanced in (False, True):
            tag = f'km_k{k}_{"bal" if balanced else "plain"}'
            np.random.seed(11)
            probe = np.random.get_state()
            seen, orig, spy = _spy_choice()
            labels, inertias, finals, inits = [], [], [], []
            np.random.choice = spy
            try:
                with MG.quiet(), MG.stable_sort():
                    for _ in range(N_RUNS):
                        lab, inertia = RU.singleKmedoids(k, n, D, balanced, 10)
                        labels.append(np.asarray(lab, dtype=np.int64))
                        inertias.append(np.float32(inertia))
                        finals.append(seen[-1][0].copy())
                        inits.append(seen[-1][1])
            finally:
                np.random.choice = orig
            np.random.set_state(probe)
            with MG.quiet(), MG.stable_sort():
                fin = RU.kmedoids(k, n, D, balanced=balanced, n_init=N_RUNS, max_iter=10)
            out[tag + '_labels'] = np.array(labels, dtype=np.int8)
            out[tag + '_inertia'] = np.array(inertias, dtype=np.float32)
            out[tag + '_medoids'] = np.array(finals, dtype=np.int64)
            out[tag + '_inits'] = np.array(inits, dtype=np.int64)
            out[tag + '_label'] = np.asarray(fin, dtype=np.int8)
            print(f'{tag}: inertia={[float(x) for x in inertias]} counts={np.bincount(fin, minlength=k)}', flush=True)


def gen_lpa(D, out):
    n, k = D.shape[0], 4
    for balanced in (False, True):
        tag = f'lpa_{"bal" if balanced else "plain"}'
        np.random.seed(13)
        labels, inertias, margins = [], [], []
        with MG.quiet(), MG.stable_sort():
            for _ in range(N_RUNS):
                lab, inertia = RU.singleLPA(k, n, D, balanced, 10, max_iter=10)
                # the weights of a round from `lab` (those that produced it once the run has converged)
                W = np.zeros((n, k))
                for i in range(n):
                    W[:, lab[i]] += np.exp(-D[i])
                top = np.sort(W, axis=1)[:, ::-1]
                margins.append((top[:, 0] - top[:, 1]) / top[:, 0])
                labels.append(np.asarray(lab, dtype=np.int64))
                inertias.append(float(inertia))
        out[tag + '_labels'] = np.array(labels, dtype=np.int8)
        out[tag + '_inertia'] = np.array(inertias, dtype=np.float64)
        out[tag + '_margin'] = np.array(margins, dtype=np.float64)
        print(f'{tag}: inertia={inertias}', flush=True)


def gen_neighbors(X, out):
    from scipy.sparse import csr_matrix
    sp = csr_matrix(X)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                             # findNeighbor saves var + '.npy' under cache_dir
        try:
            for var in ('euclidean', 'cosine', 'manhattan'):
                t0 = time.time()
                idx, val = RU.findNeighbor('', sp, X.shape[0], var=var, n_neighbor=10)
                out[f'nn_{var}_idx'] = np.asarray(idx, dtype=np.int16)
                out[f'nn_{var}_val'] = np.asarray(val, dtype=np.float16)
                print(f'findNeighbor {var}: {time.time() - t0:.1f}s', flush=True)
        finally:
            os.chdir(cwd)


if __name__ == '__main__':
    X = np.load(os.path.join(HERE, 'kmeans_toy.npz'))['X']
    D = toy_distances(X)
    out = {'X': X, 'D_sha256': np.array(hashlib.sha256(D.tobytes()).hexdigest())}
    gen_kmedoids(D, out)
    gen_lpa(D, out)
    gen_neighbors(X, out)
    np.savez_compressed(os.path.join(HERE, 'cluster_toy.npz'), **out)
