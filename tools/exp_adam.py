"""The fused Adam step (csrc/mf_train.hip: mf_adam_step_kernel) measured on the GPU.  One JSON line, and --out FILE.

    python tools/exp_adam.py [--shapes bench,cfg3] [--epochs 3] [--torch-steps 5] [--out profiles/r05/exp_adam.json]

Per shape (bench: 5 uniform shards of the ml-1m-shaped synthetic set, d = 32; cfg3: 32 shards of the 25 M-shaped set, d = 128 --
BASELINE.json configs[3] at its literal width; B = 30,000, lr 1e-3, N(0, 1) tables, --epochs epochs of every shard side by side):
  adam                  us per launch of mf_adam_step_kernel (ure_job_train_profiled: events around every launch, the epochs after
                        the first), the peak device memory of the job and its run, finite_tables after the last epoch
  sgd_dense             the same for the default kernel with lazy_rows = False: the like-for-like comparison -- both stream every
                        row in every step, Adam moves 24 P dense bytes per step where SGD moves 16 P
  sgd_default           the default kernel as the product runs it (lazy rows in closed form, no touch mode), for scale
  torch_adam            dense nn.Embedding x 2 + torch.optim.Adam(weight_decay) + MSELoss(sum) on the device, ONE shard (the first):
                        ms per optimizer step by events, median of --torch-steps after two warm-up steps, and its peak memory;
                        a job advances all its shards per launch, so the composition's time for the job is n_shards times that
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from ultrare_amd import engine, rng, synth  # noqa: E402

SHAPES = {'bench': (synth.ML1M, 5, 32), 'cfg3': (synth.ML25M, 32, 128)}
BATCH, LR, LAM = 30000, 1e-3, 0.1


def job_leg(shards, inits, tags, d, epochs, **kw):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    job = engine.TrainJob(shards, inits, tags, d, BATCH, epochs, LR, LAM, 0.9, 0.95, touch=False, **kw)
    tps = max(job.steps_per_epoch(s) for s in range(len(shards)))
    job.run(tps)                                            # the first epoch: warm-up (and the standalone tag passes of epoch 0)
    step_ms, n_step, _, _ = job.run_profiled(job.ticks - job.done)
    finite = all(bool(torch.isfinite(t).all()) for s in range(len(shards)) for t in job.padded_tables(s))
    loss = [float(x) for x in np.sqrt(job.epoch_sse(0) / shards[0].N)]
    peak = torch.cuda.max_memory_allocated() - base
    job.close()
    return dict(us_per_launch=round(1e3 * step_ms / max(n_step, 1), 3), launches=int(n_step), peak_job_mb=round(peak / 2**20, 1),
                finite_tables=finite, train_rmse_shard0=[round(x, 4) if np.isfinite(x) else None for x in loss])


def torch_leg(part, n_user, n_item, d, init, steps):
    dev = engine._device()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    U, V = torch.nn.Embedding(n_user, d, device=dev), torch.nn.Embedding(n_item, d, device=dev)
    with torch.no_grad():
        U.weight.copy_(torch.as_tensor(init[0]))
        V.weight.copy_(torch.as_tensor(init[1]))
    opt = torch.optim.Adam(list(U.parameters()) + list(V.parameters()), lr=LR, weight_decay=LAM)
    loss_fn = torch.nn.MSELoss(reduction='sum')
    uid, iid, r = (torch.as_tensor(np.asarray(x)).to(dev) for x in part)
    uid, iid, r = uid.long(), iid.long(), r.float()
    perm = torch.randperm(len(uid), device=dev)
    ts = []
    for s in range(steps + 2):
        idx = perm[(s * BATCH) % max(len(uid) - BATCH, 1):][:BATCH]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        opt.zero_grad()
        loss_fn((U(uid[idx]) * V(iid[idx])).sum(1), r[idx]).backward()
        opt.step()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    peak = torch.cuda.max_memory_allocated() - base
    return dict(ms_per_step_one_shard=round(float(np.median(ts[2:])), 4), min=round(min(ts[2:]), 4), max=round(max(ts[2:]), 4),
                peak_mb_one_shard=round(peak / 2**20, 1))


def shape_leg(name, epochs, torch_steps):
    spec, n_shards, d = SHAPES[name]
    data = synth.make_dataset(**spec, seed=synth.SEED)
    shard_of, _ = synth.uniform_shards(spec['n_user'], n_shards)
    parts = synth.split_shards(data['train'], shard_of, n_shards)
    torch.manual_seed(42)
    inits, tags = [], []
    for p in parts:
        inits.append(rng.mf_init(spec['n_user'], spec['n_item'], d))
        tags.append(rng.epoch_tags(rng.epoch_seeds(epochs, True), len(p[0]), BATCH, threads=8))
    shards = [engine.ShardData(*p, spec['n_user'], spec['n_item']) for p in parts]
    P = n_shards * (spec['n_user'] + spec['n_item']) * d
    out = dict(n_shards=n_shards, d=d, batch=BATCH, epochs=epochs, rows=[len(p[0]) for p in parts], table_elements=P)
    out['adam'] = job_leg(shards, inits, tags, d, epochs, optimizer='adam')
    out['sgd_dense'] = job_leg(shards, inits, tags, d, epochs, lazy_rows=False)
    out['sgd_default'] = job_leg(shards, inits, tags, d, epochs, lazy_rows=True)
    out['adam_over_sgd_dense'] = round(out['adam']['us_per_launch'] / out['sgd_dense']['us_per_launch'], 3)
    out['torch_adam'] = torch_leg(parts[0], spec['n_user'], spec['n_item'], d, inits[0], torch_steps)
    out['torch_over_adam_per_step'] = round(n_shards * 1e3 * out['torch_adam']['ms_per_step_one_shard'] / out['adam']['us_per_launch'], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='bench,cfg3')
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--torch-steps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from ultrare_amd import build as lib_build
    out = dict(tool='exp_adam', device=torch.cuda.get_device_name(0), source_hash=lib_build.source_hash())
    for name in a.shapes.split(','):
        out[name] = shape_leg(name, a.epochs, a.torch_steps)
        print(json.dumps({name: out[name]}), flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
