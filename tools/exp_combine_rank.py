"""Top-10 and test-pair ranks under the learned shard combiner (engine.recommend / rank_pairs with weights= ->
ure_recommend_topk_weighted / ure_rank_pairs_weighted) measured on the GPU against the mean route and against the
composition they replace (engine.score_weighted over all n_query x n_item pairs, a mask, torch.topk), and the ranking metrics
of a small multi-shard ensemble under the mean, a global-weight and a per-group combiner.  One JSON line per shape.

    python tools/exp_combine_rank.py [--shapes ml1m,cfg3] [--rounds 7] [--window 0.3] [--no-compose] [--quality]

Timing: every route is warmed up, then the routes are ALTERNATED for --rounds rounds in one process; a round times each route by
device events around back-to-back calls filling about --window seconds.  Reported: the median over the rounds with the smallest
and largest round, in microseconds per call.  The engine calls include their host part (id upload, scratch allocation), as a
caller pays it.  Tables are random normal (the kernels' cost does not depend on the values), weights the mean disturbed, three
user groups dealt out as user % 3; the exclusion set is random at the shape's density and each user has `tpu` random targets.
Not run by the tests or by bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ultrare_amd import combine, engine  # noqa: E402

SHAPES = {
    # name: (n_user, n_query, n_item, S, d, exclusion density, targets per user)
    'ml1m': (6040, 6040, 3416, 5, 32, 0.048, 33),         # ml-1m: the shape and the ~200 k targets tools/exp_recommend.py / exp_rank.py quote
    'cfg3': (162541, 4096, 60000, 32, 128, 0.0, 50),      # BASELINE.json configs[3]: 32 shards, 60 k items, d = 128
}


def one_round(fn, window):
    """us per call of fn over about `window` seconds of back-to-back calls, by device events."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(2, int(window / max(time.perf_counter() - t0, 1e-6)))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def alternate(routes, rounds, window):
    """{name: {'median_us', 'min_us', 'max_us'}} of the routes, alternated round by round after a warm-up of each."""
    for fn in routes.values():
        fn()
        fn()
    times = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            times[name].append(one_round(fn, window))
    return {name: {'median_us': round(float(np.median(t)), 1), 'min_us': round(min(t), 1), 'max_us': round(max(t), 1)} for name, t in times.items()}


def csr_rows(rng, n, n_item, count=None, density=None):
    rows = [np.sort(rng.choice(n_item, count, replace=False)).astype(np.int32) if count is not None else
            np.flatnonzero(rng.random(n_item) < density).astype(np.int32) for _ in range(n)]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, np.concatenate(rows)


def run(name, rounds, window, compose):
    n_user, n_query, n_item, S, d, dens, tpu = SHAPES[name]
    g = torch.Generator(device='cuda').manual_seed(0)
    scale = d ** -0.25
    tables = [(torch.randn(n_user, d, device='cuda', generator=g) * scale, torch.randn(n_item, d, device='cuda', generator=g) * scale) for _ in range(S)]
    rng = np.random.default_rng(1)
    users = rng.choice(n_user, n_query, replace=False)
    excl = csr_rows(rng, n_query, n_item, density=dens) if dens > 0 else None
    targets = csr_rows(rng, n_query, n_item, count=tpu)
    gou = torch.from_numpy((np.arange(n_user) % 3).astype(np.int32)).cuda()
    W = {link: torch.from_numpy((combine.mean_weights(S)[None, :] + 0.5 * rng.standard_normal((3, S + 1)) / S) * (1.0 if link == 0 else 3.0)).cuda()
         for link in (0, 1)}
    wts = {link: (link, W[link], gou) for link in (0, 1)}
    routes = {'recommend_mean': lambda: engine.recommend(tables, d, users, 10, excl),
              'recommend_linear': lambda: engine.recommend(tables, d, users, 10, excl, weights=wts[0]),
              'recommend_logistic': lambda: engine.recommend(tables, d, users, 10, excl, weights=wts[1]),
              'rank_mean': lambda: engine.rank_pairs(tables, d, users, targets, excl),
              'rank_linear': lambda: engine.rank_pairs(tables, d, users, targets, excl, weights=wts[0]),
              'rank_logistic': lambda: engine.rank_pairs(tables, d, users, targets, excl, weights=wts[1])}
    out = {'shape': name, 'n_query': n_query, 'n_item': n_item, 'S': S, 'd': d, 'top_k': 10, 'targets': int(len(targets[1])),
           'excluded': int(len(excl[1])) if excl else 0, 'rounds': rounds, 'window_s': window}
    if compose:
        # the composition the new calls replace: the pair lists are built once, outside the timing (in its favour)
        uid = torch.from_numpy(np.repeat(users.astype(np.int32), n_item)).cuda()
        iid = torch.arange(n_item, dtype=torch.int32, device='cuda').repeat(n_query)
        mask = None
        if excl is not None:
            mask = torch.zeros(n_query, n_item, dtype=torch.bool, device='cuda')
            mask[torch.from_numpy(np.repeat(np.arange(n_query), np.diff(excl[0]))).cuda(), torch.from_numpy(excl[1].astype(np.int64)).cuda()] = True

        def composed(link):
            pred, _ = engine.score_weighted(tables, d, uid, iid, None, link, W[link], gou)
            sc = pred.view(n_query, n_item)
            if mask is not None:
                sc = sc.masked_fill(mask, float('-inf'))
            return torch.topk(sc, 10, dim=1)
        routes['compose_linear'] = lambda: composed(0)
        routes['compose_logistic'] = lambda: composed(1)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        composed(1)
        torch.cuda.synchronize()
        out['compose_peak_bytes'] = int(torch.cuda.max_memory_allocated() - base)        # above the tables and the pair lists
        out['compose_pair_list_bytes'] = int(uid.numel() * 8)
        torch.cuda.reset_peak_memory_stats()
        engine.recommend(tables, d, users, 10, excl, weights=wts[1])
        torch.cuda.synchronize()
        out['recommend_peak_bytes'] = int(torch.cuda.max_memory_allocated() - base)
        # where no two scores of a user tie, the composition and the call name the same items
        a = engine.recommend(tables, d, users, 10, excl, weights=wts[0])[1].cpu().numpy()
        b = composed(0)[1].cpu().numpy()
        out['rows_differing_from_composition'] = int((a != b).any(axis=1).sum())
    out['times'] = alternate(routes, rounds, window)
    t = out['times']
    for kind in ('recommend', 'rank'):
        for link in ('linear', 'logistic'):
            out[f'{kind}_{link}_over_mean'] = round(t[f'{kind}_{link}']['median_us'] / t[f'{kind}_mean']['median_us'], 3)
    if compose:
        for link in ('linear', 'logistic'):
            out[f'compose_{link}_over_recommend'] = round(t[f'compose_{link}']['median_us'] / t[f'recommend_{link}']['median_us'], 3)
    print(json.dumps(out), flush=True)


def quality():
    """rank_eval (HR / Recall / NDCG @ 10, 20 and MRR) under the mean, a global-weight and a per-group combiner, both links, on the
    synthetic set of tools/exp_bpr.py's accuracy(): 3,000 users x 3,416 items, 300 k training and 30 k test ratings, 3 uniform user
    shards each trained with GcnJob (d = 32, L = 2, 30 epochs, MSE).  ONE seed: a reading, not a distribution."""
    from scipy.sparse import coo_matrix
    from ultrare_amd import synth
    from ultrare_amd.method.utils import MF, fit_combiner, rank_eval
    from ultrare_amd.read import RatingData, loadData
    n_user, n_item, d, S, epochs, layers, batch = 3000, 3416, 32, 3, 30, 2, 3000
    data = synth.make_dataset(n_user=n_user, n_item=n_item, n_train=300000, n_test=30000)
    (uid, iid, r), (tu, ti, tr) = data['train'], data['test']
    test = loadData(RatingData(np.vstack([tu, ti, tr / 5]).astype(np.float64)), 30000, 1, False)
    train_csr = coo_matrix((np.ones(len(uid), np.float32), (uid, iid)), shape=(n_user, n_item)).tocsr()
    rs = np.random.RandomState(1)
    shard_of = rs.permutation(n_user) % S
    P0, Q0 = (rs.standard_normal((n_user, d)) * 0.1).astype(np.float32), (rs.standard_normal((n_item, d)) * 0.1).astype(np.float32)
    U = torch.zeros(n_user, d, device='cuda')
    Vs, loaders, groups = [], [], []
    for s in range(S):
        m = shard_of[uid] == s
        graph = engine.GcnGraph(uid[m], iid[m], (r[m] / 5).astype(np.float32), n_user, n_item)
        orders = np.stack([rs.permutation(int(m.sum())) for _ in range(epochs)]).astype(np.int32)
        job = engine.GcnJob(graph, (P0, Q0), orders, d, layers, batch, epochs, 1e-3, 0.1, 0.9, 0.95, 1)
        job.run()
        Us, V = job.tables(0)
        rows = torch.from_numpy(np.flatnonzero(shard_of == s)).cuda()
        U[rows] = Us[rows]                                  # (SISA's merge: a user's row comes from the shard that trained it)
        Vs.append(V.clone().contiguous())
        job.close()
        loaders.append(loadData(RatingData(np.vstack([uid[m], iid[m], r[m] / 5]).astype(np.float64)), 30000, 1, False))
        groups.append(np.flatnonzero(shard_of == s).tolist())
    models = [MF.from_tables(U.clone(), V) for V in Vs]
    rnd = lambda mtr: {k: round(float(v), 5) for k, v in mtr.items()}
    out = {'n_user': n_user, 'n_item': n_item, 'n_train': len(uid), 'n_test': len(tu), 'shards': S, 'd': d, 'layers': layers, 'epochs': epochs,
           'seeds': 1, 'mean': rnd(rank_eval(models, test, exclude=train_csr))}
    for link in ('linear', 'logistic'):
        for label, grp in (('global', None), ('per_group', groups)):
            c = fit_combiner(models, loaders, link, l2=1e-3, groups=grp)
            out[f'{link}_{label}'] = rnd(rank_eval(models, test, exclude=train_csr, combiner=c))
            out[f'{link}_{label}_W'] = np.round(c.W, 4).tolist()
    print(json.dumps({'quality': out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window', type=float, default=0.3)
    ap.add_argument('--no-compose', action='store_true', help='skip the score_weighted + torch.topk composition (0.25 G pairs at cfg3)')
    ap.add_argument('--quality', action='store_true', help='also the ranking metrics of a synthetic multi-shard ensemble, one seed')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for name in [s for s in a.shapes.split(',') if s]:
        run(name, a.rounds, a.window, not a.no_compose)
        torch.cuda.empty_cache()
    if a.quality:
        quality()


if __name__ == '__main__':
    main()
