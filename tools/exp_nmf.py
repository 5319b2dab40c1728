"""The NeuMF backbone (csrc/nmf.hip) measured on the GPU against a torch composition of the same model.  One JSON line.

    python tools/exp_nmf.py [--shapes ml1m,cfg3] [--reps 7] [--step-timeout 600] [--request]

Per shape -- one shard of a 5-shard ml-1m call (1,208 users x 3,416 items, 180 k ratings, k = 32, layers [64, 32]) and one of
BASELINE.json configs[3] (5,062 users x 60,000 items, 703 k ratings, k = 128, layers [128, 64]), both synthetic (synth.make_dataset),
B = 30,000 -- medians of --reps calls after two warm-up calls, (min, max) beside every median, device events round the launches:
  step_ms                one training step of engine.NmfJob (seven launches); its entries timed apart: forward_backward_ms,
                         weight_grad_ms, row_sum_user_ms, row_sum_item_ms, update_ms
  torch_step_ms          one step of the torch composition: four dense nn.Embedding, nn.Linear layers and head, relu, MSELoss(sum) on
                         the batch, backward, torch.optim.SGD(momentum, weight_decay) over every parameter (it has the matrix cores)
  score_ms, torch_score_ms   one scoring pass of the shard's test pairs: engine.nmf_score against the same module's forward
  peak_mb, torch_peak_mb     peak device memory of a step of either route above what was resident before it
  epoch_loss, torch_epoch_loss   sqrt(sum of the batch losses / N) of ONE epoch from the same init and orders at lr = 1e-5, and
                         score_max_diff_from_torch: the two are the same model
--request: the ml-1m-shaped 5-shard request (6,040 x 3,416, 900 k ratings, k = 16, layers [64, 32], 50 epochs) through Sisa('nmf') at
the default lr = 0.001, at 1e-5 and at 1e-6, beside Sisa('mf') at the default: whether the tables stay finite, and the final total RMSE.
This is ONE run of every number.  Every shape runs in a child process of its own under --step-timeout seconds; after a child that
fails or runs out of time nothing more is started.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SHAPES = {'ml1m': (dict(n_user=1208, n_item=3416, n_train=180000, n_test=20000), 32, [64, 32]),
          'cfg3': (dict(n_user=5062, n_item=60000, n_train=703000, n_test=78000), 128, [128, 64])}
BATCH = 30000


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


class TorchNMF:
    """The composition: four dense embeddings, linear layers, SGD -- from the same init as the job."""

    def __init__(self, model, lr, lam, mu):
        import copy
        import torch
        self.m = copy.deepcopy(model).to('cuda').requires_grad_(True)
        self.opt = torch.optim.SGD(self.m.parameters(), lr=lr, momentum=mu, weight_decay=lam)
        self.loss_fn = torch.nn.MSELoss(reduction='sum')

    def forward(self, u, i):
        import torch
        m = self.m
        a = torch.cat([m.user_mat_mlp(u), m.item_mat_mlp(i)], dim=1)
        for lin in m.fc:
            a = torch.relu(lin(a))
        return m.head(torch.cat([m.user_mat_mf(u) * m.item_mat_mf(i), a], dim=1)).squeeze(1)

    def step(self, u, i, r):
        self.opt.zero_grad()
        loss = self.loss_fn(self.forward(u, i), r)
        loss.backward()
        self.opt.step()
        return loss


def shape_times(name, reps):
    import torch
    from ultrare_amd import _native as nv, engine, synth
    from ultrare_amd.method.utils import NMF
    spec, k, layers = SHAPES[name]
    data = synth.make_dataset(**spec)
    uid, iid, r = data['train']
    tu, ti, tr = data['test']
    n_user, n_item, N = spec['n_user'], spec['n_item'], len(uid)
    r5 = (r / 5).astype(np.float32)
    graph = engine.GcnGraph(uid, iid, r5, n_user, n_item)
    torch.manual_seed(0)
    model = NMF(n_user, n_item, k, layers)
    init = tuple(t.numpy() for t in model.tables())
    rs = np.random.RandomState(0)
    epochs, lr, lam, mu = 2, 1e-5, 0.1, 0.9
    orders = np.stack([rs.permutation(N) for _ in range(epochs)]).astype(np.int32)
    out = {'shape': name, 'n_user': n_user, 'n_item': n_item, 'nnz': N, 'k': k, 'layers': layers, 'batch': BATCH, 'lr': lr, 'walk_multiple': round(N / BATCH, 1)}

    # ---- the job: one epoch's loss, then a step and its entries
    job = engine.NmfJob(graph, init, orders, k, layers, BATCH, epochs, lr, lam, mu)
    out['steps_per_epoch'], out['launches_per_step'] = job.steps, 7
    out['job_params_mb'] = round(job._pool.numel() * 4 / 2**20, 1)
    out['job_slot_buffers_mb'] = round(sum(t.numel() * t.element_size() for t in (job._err, job._act, job._dlt, job._emb, job._scratch)) / 2**20, 1)
    job.run_epochs(1)
    out['epoch_loss'] = float(np.sqrt(job.epoch_sse()[0] / N))
    U, V, dense = (t.clone() for t in job.params())
    out['peak_mb'] = peak_mb(lambda: job._step(1, 0))
    state = {'s': 1}

    def one_step():
        job._step(1, 1 + state['s'] % (job.steps - 1))        # (not step 0: that one also gathers the epoch's ranks)
        state['s'] += 1
    out['step_ms'] = event_ms(one_step, reps)
    g, S, L, st = graph, job.shape, nv.lib(), nv.stream_handle()
    lay, m = nv.ptr(job._lay), len(job._lay)
    (pU, pV, pd), (gU, gV, gd) = job._part(0), job._part(2)
    lo, n_slots = BATCH, min(BATCH, N - BATCH)
    out['forward_backward_ms'] = event_ms(lambda: nv.check(L.ure_nmf_forward_backward(
        nv.ptr(g.row_u), nv.ptr(g.col), nv.ptr(g.rating), nv.ptr(job._rank), g.nnz, lo, n_slots, pU.data_ptr(), pV.data_ptr(), g.n_user, g.n_item,
        pd.data_ptr(), S.k, lay, m, nv.ptr(job._err), None, nv.ptr(job._act), nv.ptr(job._dlt), nv.ptr(job._emb), st), 'ure_nmf_forward_backward'), reps)
    out['weight_grad_ms'] = event_ms(lambda: nv.check(L.ure_nmf_weight_grad(
        nv.ptr(job._err), nv.ptr(job._act), nv.ptr(job._dlt), n_slots, S.k, lay, m, gd.data_ptr(), nv.ptr(job._scratch), job._scratch_bytes, 0, st),
        'ure_nmf_weight_grad'), reps)
    out['row_sum_user_ms'] = event_ms(lambda: nv.check(L.ure_nmf_row_sum(
        nv.ptr(g.off_u), None, nv.ptr(job._rank), g.n_user, g.nnz, lo, n_slots, nv.ptr(job._emb), 2 * S.wd, 0, S.wd, nv.ptr(job._err), gU.data_ptr(),
        nv.ptr(job._row_loss), st), 'ure_nmf_row_sum'), reps)
    out['row_sum_item_ms'] = event_ms(lambda: nv.check(L.ure_nmf_row_sum(
        nv.ptr(g.off_i), nv.ptr(g.to_csr), nv.ptr(job._rank), g.n_item, g.nnz, lo, n_slots, nv.ptr(job._emb), 2 * S.wd, S.wd, S.wd, None, gV.data_ptr(),
        None, st), 'ure_nmf_row_sum'), reps)
    w, mo, gr = (torch.zeros(job.n_params, dtype=torch.float32, device='cuda') for _ in range(3))
    out['update_ms'] = event_ms(lambda: engine.gcn_sgd_step(w, mo, gr, lr, lam, mu, False), reps)
    job.close()
    del w, mo, gr

    # ---- scoring: the kernel against the module's forward on the same trained parameters
    tud, tid = torch.from_numpy(tu.astype(np.int32)).cuda(), torch.from_numpy(ti.astype(np.int32)).cuda()
    pred = torch.empty(len(tu), dtype=torch.float32, device='cuda')
    out['n_test'] = len(tu)
    out['score_ms'] = event_ms(lambda: engine.nmf_score(U, V, dense, k, layers, tud, tid, pred=pred), reps)
    trained = TorchNMF(NMF.from_tables(U, V, dense, k, layers), lr, lam, mu)
    tul, til = tud.long(), tid.long()
    with torch.no_grad():
        out['torch_score_ms'] = event_ms(lambda: trained.forward(tul, til), reps)
        out['score_max_diff_from_torch'] = float((trained.forward(tul, til) - pred).abs().max())
    del trained

    # ---- the torch composition from the same init and orders: one epoch's loss, then a step
    comp = TorchNMF(model, lr, lam, mu)
    uid_d, iid_d = torch.from_numpy(uid.astype(np.int64)).cuda(), torch.from_numpy(iid.astype(np.int64)).cuda()
    r_d, order_d = torch.from_numpy(r5).cuda(), torch.from_numpy(orders.astype(np.int64)).cuda()

    def torch_step(e, s):
        idx = order_d[e][s * BATCH:(s + 1) * BATCH]
        return comp.step(uid_d[idx], iid_d[idx], r_d[idx])
    total = sum(float(torch_step(0, s)) for s in range(-(-N // BATCH)))
    out['torch_epoch_loss'] = float(np.sqrt(total / N))
    out['torch_peak_mb'] = peak_mb(lambda: torch_step(1, 0))
    state = {'s': 1}

    def one_torch_step():
        torch_step(1, 1 + state['s'] % (N // BATCH - 1))
        state['s'] += 1
    out['torch_step_ms'] = event_ms(one_torch_step, reps)
    return out


def request():
    """The 5-shard ml-1m-shaped request, 50 epochs: NeuMF at the default lr, at 1e-5 and at 1e-6, MF at the default."""
    import warnings

    import torch
    from ultrare_amd import synth
    from ultrare_amd.config import InsParam
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.read import RatingData, loadData
    n_user, n_item, S = 6040, 3416, 5
    data = synth.make_dataset(n_user=n_user, n_item=n_item, n_train=900000, n_test=100000)
    shard_of, groups = synth.uniform_shards(n_user, S)
    tr, te = synth.split_shards(data['train'], shard_of, S), synth.split_shards(data['test'], shard_of, S)
    trd = [loadData(RatingData(np.stack(t)), BATCH, 24) for t in tr]
    ted = [loadData(RatingData(np.stack(t)), BATCH, 24, False) for t in te]
    tot = loadData(RatingData(np.hstack([np.stack(t) for t in te])), BATCH, 24, False)
    out = []
    for model, lr in (('nmf', None), ('nmf', 1e-5), ('nmf', 1e-6), ('mf', None)):
        p = InsParam('toy', 50, layers=[64, 32], k=16, model=model, lr=lr, data_dir='.')
        p.n_user, p.n_item, p.batch = n_user, n_item, BATCH
        torch.manual_seed(42)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            s = Sisa(p, model, S, groups)
        ml = s.learn(trd, ted, tot, 0, '')
        finite = all(bool(torch.isfinite(q).all()) for m in ml for q in m.parameters())
        out.append({'model': model, 'lr': p.lr, 'epochs': 50, 'tables_finite': finite, 'total_rmse': s.log0['total_rmse'], 'total_ndcg': s.log0['total_ndcg'],
                    'total_hr': s.log0['total_hr'], 'train_loss_first_last': [s.log['train_loss'][0], s.log['train_loss'][-1]]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ml1m,cfg3')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--step-timeout', type=int, default=600)
    ap.add_argument('--request', action='store_true', help='also run the 5-shard, 50-epoch request at the default lr')
    ap.add_argument('--child', default=None, help='(internal) measure this one shape in this process')
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('exp_nmf needs the GPU: nothing is measured on the host')
        res = {'request': request()} if a.child == 'request' else shape_times(a.child, a.reps)
        res['gpu'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'reps': a.reps, 'runs': 1, 'shapes': []}
    for name in [s for s in a.shapes.split(',') if s] + (['request'] if a.request else []):
        if name not in SHAPES and name != 'request':
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
        if name == 'request':
            out['request'] = res['request']
        else:
            out['shapes'].append(res)
    print(json.dumps(out), flush=True)
    if 'stopped' in out:
        raise SystemExit(1)


if __name__ == '__main__':
    main()
