"""BPR training (csrc/bpr.hip) measured on the GPU against the MSE step of the same job, a torch composition, and -- for
what it is for -- the ranking metrics of a BPR-trained against an MSE-trained ensemble.  One JSON line.

    python tools/exp_bpr.py [--shapes ml1m,cfg3] [--reps 7] [--step-timeout 600] [--no-accuracy]

Per shape -- exp_lightgcn.py's two synthetic shards: one of a 5-shard ml-1m call (1,208 x 3,416, 180 k ratings, d = 32) and one of
BASELINE.json configs[3] (5,062 x 60,000, 703 k ratings, d = 128) -- and per layer count L = 2 and L = 0 (BPR-MF), B = 30,000;
medians of --reps calls after two warm-up calls, (min, max) beside every median, device events around the launches:
  bpr_step_ms, mse_step_ms     one training step of engine.GcnJob(loss='bpr') and of the MSE job (the path the parent commit has,
                               byte for byte) at the same shape; bpr_loss_grad_ms / mse_loss_grad_ms: the launches that differ
                               (coefficient pass + two walks + fold against residual pass + two walks + fold)
  epoch_start_ms               the per-epoch negative draw (sample_ms) and negative index (index_ms), and epoch_start_share: its
                               share of an epoch of steps_per_epoch BPR steps
  torch_step_ms                the torch composition: sparse.mm forward under autograd, -logsigmoid of the score difference on the
                               batch (negatives given), backward, torch.optim.SGD(momentum, weight_decay)
  peak_mb, torch_peak_mb       peak device memory of a step of either route above what was held before it; bpr_state_mb: the
                               per-epoch arrays and the sort's scratch the BPR job holds beside the MSE job's
'accuracy' (one child of its own): a synthetic set of 3,000 users x 3,416 items (300 k train, 30 k test ratings) split into 3 uniform
user shards, every shard trained with GcnJob (d = 32, L = 2, 30 epochs, the default schedule) once per loss; rank_eval (all items the
user has not trained on) of both ensembles: HR@10, NDCG@10, MRR.
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

from exp_lightgcn import SHAPES, event_ms, peak_mb  # noqa: E402

BATCH, KEY = 30000, 20240608


def shape_times(name, reps):
    import torch
    from ultrare_amd import engine, lightgcn, synth
    spec, d = SHAPES[name]
    uid, iid, r = synth.make_dataset(**spec)['train']
    n_user, n_item, N = spec['n_user'], spec['n_item'], len(uid)
    graph = engine.GcnGraph(uid, iid, (r / 5).astype(np.float32), n_user, n_item)
    engine.bpr_prepare(graph)
    rs = np.random.RandomState(0)
    P0, Q0 = (rs.standard_normal((n_user, d)) * 0.1).astype(np.float32), (rs.standard_normal((n_item, d)) * 0.1).astype(np.float32)
    epochs = 2
    orders = np.stack([rs.permutation(N) for _ in range(epochs)]).astype(np.int32)
    lr, lam, mu = 1e-3, 0.1, 0.9
    out = {'shape': name, 'n_user': n_user, 'n_item': n_item, 'nnz': N, 'd': d, 'batch': BATCH, 'distinct_pairs': int(graph.col_d.numel()), 'layers': {}}

    # ---- the per-epoch work: the draw and the index
    neg = engine.bpr_negatives(graph, KEY, 0)
    state = {'e': 0}

    def sample():
        state['e'] += 1
        engine._bpr_sample(graph, KEY, state['e'], neg, engine.nv.stream_handle())
    out['sample_ms'] = event_ms(sample, reps)
    off_n = torch.empty(n_item + 1, dtype=torch.int64, device='cuda')
    map_n, usr_n = torch.empty_like(neg), torch.empty_like(neg)
    scratch = torch.empty(int(engine.nv.lib().ure_bpr_index_scratch(N, n_item)), dtype=torch.uint8, device='cuda')
    out['index_ms'] = event_ms(lambda: engine._bpr_index(graph, neg, off_n, map_n, usr_n, scratch, engine.nv.stream_handle()), reps)

    def epoch_start():
        sample()
        engine._bpr_index(graph, neg, off_n, map_n, usr_n, scratch, engine.nv.stream_handle())
    out['epoch_start_ms'] = event_ms(epoch_start, reps)
    out['index_scratch_mb'] = round(scratch.numel() / 2**20, 2)

    tag = engine.gcn_step_tags(graph, orders[0], BATCH)
    for layers in (2, 0):
        res = {}
        for loss in ('bpr', 'mse'):
            job = engine.GcnJob(graph, (P0, Q0), orders, d, layers, BATCH, epochs, lr, lam, mu, loss=loss, key=KEY)
            job._step(0, 0)
            res[f'{loss}_peak_mb'] = peak_mb(lambda: job._step(0, 1))
            state = {'s': 2}

            def one_step():
                job._step(0, 1 + state['s'] % (job.steps - 1))             # (never step 0: the epoch start is timed apart)
                state['s'] += 1
            res[f'{loss}_step_ms'] = event_ms(one_step, reps)
            U, V = job.padded_tables(0)
            if loss == 'bpr':
                index = (job._bpr['off_n'], job._bpr['map_n'], job._bpr['usr_n'])
                res['bpr_loss_grad_ms'] = event_ms(lambda: engine.bpr_loss_grad(graph, tag, 1, U, V, job._bpr['neg'], index), reps)
                res['bpr_state_mb'] = round(sum(t.numel() * t.element_size() for t in job._bpr.values()) / 2**20, 2)
                res['steps_per_epoch'] = job.steps
            else:
                res['mse_loss_grad_ms'] = event_ms(lambda: engine.gcn_loss_grad(graph, tag, 1, U, V), reps)
            job.close()
        res['bpr_over_mse_step'] = round(res['bpr_step_ms']['median'] / res['mse_step_ms']['median'], 3)
        epoch = out['epoch_start_ms']['median'] + res['steps_per_epoch'] * res['bpr_step_ms']['median']
        res['epoch_start_share'] = round(out['epoch_start_ms']['median'] / epoch, 4)

        # ---- the torch composition: sparse forward under autograd, -logsigmoid, SGD; the negatives are given
        g = graph.host

        def adjacency(side):
            off, idx, s_src, s_dst, n_dst, n_src = g.side(side)
            val = np.repeat(s_dst, np.diff(off)) * s_src[idx]
            return torch.sparse_csr_tensor(torch.from_numpy(off), torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(val.astype(np.float32)),
                                           size=(n_dst, n_src)).cuda().to_sparse_coo().coalesce()
        A, At = (adjacency('csr'), adjacency('csc')) if layers else (None, None)
        P, Q = torch.from_numpy(P0).cuda().requires_grad_(True), torch.from_numpy(Q0).cuda().requires_grad_(True)
        opt = torch.optim.SGD([P, Q], lr=lr, momentum=mu, weight_decay=lam)
        uid_d, iid_d = torch.from_numpy(uid.astype(np.int64)).cuda(), torch.from_numpy(iid.astype(np.int64)).cuda()
        neg_file = torch.empty(N, dtype=torch.int64, device='cuda')
        neg_file[graph.pos.long()] = neg.long()
        order_d = torch.from_numpy(orders[0].astype(np.int64)).cuda()
        c = float(lightgcn.layer_scale(layers))
        state = {'s': 0}

        def torch_step():
            s = state['s'] % (N // BATCH)
            state['s'] += 1
            idx = order_d[s * BATCH:(s + 1) * BATCH]
            opt.zero_grad()
            Xu, Xi, Su, Si = P, Q, P, Q
            for _ in range(layers):
                Xu, Xi = torch.sparse.mm(A, Xi), torch.sparse.mm(At, Xu)
                Su, Si = Su + Xu, Si + Xi
            Us = (Su * c)[uid_d[idx]]
            x = (Us * (Si * c)[iid_d[idx]]).sum(1) - (Us * (Si * c)[neg_file[idx]]).sum(1)
            (-torch.nn.functional.logsigmoid(x).sum()).backward()
            opt.step()
        torch_step()
        res['torch_peak_mb'] = peak_mb(torch_step)
        res['torch_step_ms'] = event_ms(torch_step, reps)
        del A, At, P, Q, opt
        out['layers'][f'L{layers}'] = res
    return out


def accuracy():
    """rank_eval of a BPR-trained and an MSE-trained ensemble of 3 uniform user shards on one synthetic set."""
    import torch
    from scipy.sparse import coo_matrix
    from ultrare_amd import bpr, engine, synth
    from ultrare_amd.method.utils import MF, rank_eval
    from ultrare_amd.read import RatingData, loadData
    n_user, n_item, d, S, epochs, layers = 3000, 3416, 32, 3, 30, 2
    data = synth.make_dataset(n_user=n_user, n_item=n_item, n_train=300000, n_test=30000)
    (uid, iid, r), (tu, ti, tr) = data['train'], data['test']
    test = loadData(RatingData(np.vstack([tu, ti, tr / 5]).astype(np.float64)), 30000, 1, False)
    train_csr = coo_matrix((np.ones(len(uid), np.float32), (uid, iid)), shape=(n_user, n_item)).tocsr()
    rs = np.random.RandomState(1)
    shard_of = rs.permutation(n_user) % S
    P0, Q0 = (rs.standard_normal((n_user, d)) * 0.1).astype(np.float32), (rs.standard_normal((n_item, d)) * 0.1).astype(np.float32)
    out = {'n_user': n_user, 'n_item': n_item, 'n_train': len(uid), 'n_test': len(tu), 'shards': S, 'd': d, 'layers': layers, 'epochs': epochs}
    for loss in ('mse', 'bpr'):
        U = torch.zeros(n_user, d, device='cuda')
        Vs, last = [], []
        for s in range(S):
            m = shard_of[uid] == s
            graph = engine.GcnGraph(uid[m], iid[m], (r[m] / 5).astype(np.float32), n_user, n_item)
            orders = np.stack([rs.permutation(int(m.sum())) for _ in range(epochs)]).astype(np.int32)
            job = engine.GcnJob(graph, (P0, Q0), orders, d, layers, BATCH, epochs, 1e-3, 0.1, 0.9, 0.95, 1, loss=loss, key=bpr.stream_key(42, s + 1))
            job.run()
            Us, V = job.tables(0)
            rows = torch.from_numpy(np.flatnonzero(shard_of == s)).cuda()
            U[rows] = Us[rows]                              # (SISA's merge: a user's row comes from the shard that trained it)
            Vs.append(V.clone().contiguous())
            last.append(float(job.epoch_loss(0)[-1] / graph.N))
            job.close()
        metrics = rank_eval([MF.from_tables(U.clone(), V) for V in Vs], test, exclude=train_csr, ks=(10,))
        out[loss] = {k: round(float(v), 5) for k, v in metrics.items()}
        out[loss]['last_epoch_mean_batch_loss'] = [round(x, 5) for x in last]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--step-timeout', type=int, default=600)
    ap.add_argument('--no-accuracy', action='store_true')
    ap.add_argument('--child', default=None, help='(internal) measure this one shape (or "accuracy") in this process')
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('exp_bpr needs the GPU: nothing is measured on the host')
        res = accuracy() if a.child == 'accuracy' else shape_times(a.child, a.reps)
        res['gpu'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'reps': a.reps, 'shapes': []}
    names = [s for s in a.shapes.split(',') if s]
    for name in names:
        if name not in SHAPES:
            raise SystemExit(f'unknown shape {name!r}: {sorted(SHAPES)}')
    for name in names + ([] if a.no_accuracy else ['accuracy']):
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
        if name == 'accuracy':
            out['accuracy'] = res
        else:
            out['shapes'].append(res)
    print(json.dumps(out), flush=True)
    if 'stopped' in out:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
