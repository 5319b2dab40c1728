"""Shared case builders of tests/test_cpu_nmf.py and tests/test_gpu_nmf.py (no pytest plugin: a plain module beside them).

A case is one shard with made-up ratings in the pattern of adam_cases.Case (a quarter of the ratings on one item, users and
items without a rating, a repeated pair, a partial last step, lr changing every epoch), a GMF width, an MLP stack and a schedule.
reference(case) holds what both files compare against, computed once per process: nmf.train_ref in float64 -- the contract -- and
two float32 CPU executions of the same training: train_ref in float32 and torch float32 autograd."""
import functools
import os

import numpy as np
import torch

import adam_cases
from adam_cases import ulp32                       # noqa: F401
from ultrare_amd import nmf

LR = 1e-3
STAGE_SHAPES = [(4, [8, 4]), (8, [16, 8]), (32, [64, 32]), (16, [64, 32, 16, 8]), (64, [128, 64]), (16, [32, 128, 4])]


def model_init(rs, n_user, n_item, k, layers, std=0.3):
    """(U0, V0, dense0) float32: normal tables, and torch's default bounds (uniform in +-1 / sqrt(fan_in)) for the layers and the
    head -- drawn from `rs`, not from torch, so that the kernel tests do not depend on NMF's order of draws."""
    S = nmf.Shape(k, layers)
    U0 = (std * rs.standard_normal((n_user, S.wd))).astype(np.float32)
    V0 = (std * rs.standard_normal((n_item, S.wd))).astype(np.float32)
    W, b = [], []
    for j in range(S.m):
        bound = 1.0 / np.sqrt(S.layers[j])
        W.append(rs.uniform(-bound, bound, (S.layers[j + 1], S.layers[j])))
        b.append(rs.uniform(-bound, bound, S.layers[j + 1]))
    bound = 1.0 / np.sqrt(k + S.layers[-1])
    return U0, V0, S.pack(W, b, rs.uniform(-bound, bound, k + S.layers[-1]), rs.uniform(-bound, bound))


class Case(adam_cases.Case):
    """adam_cases.Case (N ratings, a share `hot` on the last item, the first no_u users and no_i items without one, duplicates
    allowed) with a NeuMF model, a momentum and a weight decay; one pair is repeated on purpose."""

    def __init__(self, n_user, n_item, k, layers, N, B, epochs, seed, lam=0.1, mu=0.9, lr_decay=0.7, lr_step=1, no_u=3, no_i=4):
        super().__init__(n_user, n_item, k, N, B, epochs, seed=seed, lr=LR, lr_decay=lr_decay, lr_step=lr_step, no_u=no_u, no_i=no_i)
        self.uid[-1], self.iid[-1] = self.uid[0], self.iid[0]           # a repeated pair, apart in the file
        self.k, self.layers, self.lam, self.mu = k, list(layers), lam, mu
        self.U0, self.V0, self.dense0 = model_init(np.random.RandomState(2000 + seed), n_user, n_item, k, layers)

    def __repr__(self):
        return f'{self.n_user}x{self.n_item}-k{self.k}-{"_".join(map(str, self.layers))}-N{self.N}-B{self.B}-E{self.epochs}'

    def graph(self):
        from ultrare_amd import engine
        return engine.GcnGraph(self.uid, self.iid, self.rating, self.n_user, self.n_item)

    def job(self, graph=None):
        """The case as an NmfJob on the current device."""
        from ultrare_amd import engine
        return engine.NmfJob(graph or self.graph(), (self.U0, self.V0, self.dense0), self.orders, self.k, self.layers, self.B, self.epochs, LR,
                             self.lam, self.mu, self.lr_decay, self.lr_step)

    def train_ref(self, dtype=np.float64, plant=None):
        return nmf.train_ref(self.uid, self.iid, self.rating, self.U0, self.V0, self.dense0, self.orders, self.B, self.lr_host, self.lam, self.mu,
                             self.k, self.layers, dtype=dtype, plant=plant)


# (n_user, n_item, k, layers, N, B, epochs): one to three hidden layers, widths 4 .. 128, the last step of an epoch partial
WHOLE_CASES = [
    Case(40, 30, 8, [16, 8], 500, 200, 3, seed=1),
    Case(50, 45, 32, [64, 32], 700, 300, 3, seed=2),
    Case(33, 21, 16, [64, 32, 16, 8], 400, 150, 3, seed=3),
    Case(45, 35, 64, [128, 64], 450, 200, 2, seed=4),
    Case(30, 40, 4, [8, 4], 420, 200, 2, seed=5, lam=0.03, mu=0.5),
]


def torch_nmf(case, dtype):
    """NeuMF with torch autograd (embedding lookups, F.linear, relu), MSELoss(sum) and torch.optim.SGD(momentum, weight_decay) over
    every parameter, on the CPU in `dtype` -> dict as nmf.train_ref returns it."""
    S = nmf.Shape(case.k, case.layers)
    k = S.k
    leaf = lambda a: torch.from_numpy(np.array(a)).to(dtype).clone().requires_grad_(True)
    P, Q = leaf(case.U0), leaf(case.V0)
    W0, b0, h0, c0 = S.unpack(case.dense0)
    W, b, h, c = [leaf(w) for w in W0], [leaf(x) for x in b0], leaf(h0), leaf(np.array([c0]))
    params = [P, Q] + W + b + [h, c]
    opt = torch.optim.SGD(params, lr=float(case.lr_host[0]), momentum=float(np.float32(case.mu)), weight_decay=float(np.float32(case.lam)))
    loss_fn = torch.nn.MSELoss(reduction='sum')
    uid, iid = torch.from_numpy(case.uid.astype(np.int64)), torch.from_numpy(case.iid.astype(np.int64))
    r = torch.from_numpy(case.rating).to(dtype)

    def forward(u, i):
        pu, qi = P[u], Q[i]
        a = torch.cat([pu[:, k:], qi[:, k:]], dim=1)
        for Wj, bj in zip(W, b):
            a = torch.relu(torch.nn.functional.linear(a, Wj, bj))
        return c + (pu[:, :k] * qi[:, :k]) @ h[:k] + a @ h[k:]

    out = dict(U=[], V=[], dense=[])
    sse = np.zeros(case.epochs)
    for e in range(case.epochs):
        for grp in opt.param_groups:
            grp['lr'] = float(case.lr_host[e])
        order = torch.from_numpy(case.orders[e].astype(np.int64))
        for s in range(case.steps):
            idx = order[s * case.B:(s + 1) * case.B]
            opt.zero_grad()
            loss = loss_fn(forward(uid[idx], iid[idx]), r[idx])
            loss.backward()
            opt.step()
            sse[e] += float(loss.detach().double())
        np_ = lambda t: t.detach().numpy()
        out['U'].append(np_(P).copy())
        out['V'].append(np_(Q).copy())
        out['dense'].append(S.pack([np_(w) for w in W], [np_(x) for x in b], np_(h), np_(c)[0], dtype=np_(P).dtype))
    out = {name: np.stack(v) for name, v in out.items()}
    out['sse'], out['loss'] = sse, np.sqrt(sse / case.N)
    return out


def distance(ref64, run):
    """The maximum absolute difference over both tables and the dense vector (every layer, bias, the head and its bias) after the
    last epoch, plus the maximum relative difference over the epoch losses.  Nothing is left out."""
    tab = max(float(np.abs(np.asarray(run[name][-1], dtype=np.float64) - ref64[name][-1]).max()) for name in ('U', 'V', 'dense'))
    return tab + float(np.abs(np.asarray(run['loss'], dtype=np.float64) / ref64['loss'] - 1.0).max())


def wmax(ref64):
    return float(max(np.abs(ref64[name]).max() for name in ('U', 'V', 'dense')))


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> dict: 'f64' the contract, 'f32' train_ref in float32 (the bit contract of the job), 't32' torch's float32 run, 'E_y' the
    larger of their two distances from 'f64', 'bound' = 4 * max(E_y, ulp32(largest |w|)): the factor lightgcn_cases.reference uses."""
    ref = dict(f64=case.train_ref(), f32=case.train_ref(dtype=np.float32), t32=torch_nmf(case, torch.float32))
    ref['E_y'] = max(distance(ref['f64'], ref['f32']), distance(ref['f64'], ref['t32']))
    ref['bound'] = 4 * max(ref['E_y'], ulp32(wmax(ref['f64'])))
    return ref


def stage_model(k, layers, n_user, n_item, seed):
    """A model for the stage tests: model_init, with two units of the first layer planted so that their pre-activation is exactly
    zero for every pair -- a zero weight row under a bias of 0.0 and one under a bias of -0.0.  (A chain that starts at +0.0
    cannot end at -0.0, so both give z = +0.0: what is planted is the bias' sign.)"""
    U, V, dense = model_init(np.random.RandomState(3000 + seed), n_user, n_item, k, layers, std=0.5)
    S = nmf.Shape(k, layers)
    W, b, _, _ = S.unpack(dense)
    W[0][0, :], W[0][1, :] = 0.0, 0.0
    b[0][0], b[0][1] = 0.0, -0.0
    return U, V, dense


# ---- the artifacts of the other backbones (tests/golden/backbone_artifacts.json: recorded from the commit before the 'nmf' backbone)
ARTIFACT_RUNS = (('mf', 2), ('mf', 0), ('lightgcn', 2))          # (--model, --group) on the toy set, --epoch 2, --group-type uniform


def artifact_args(model, group, data_dir, save_dir):
    return ['--dataset', 'toy', '--epoch', '2', '--group', str(group), '--group-type', 'uniform', '--model', model, '--verbose', '0', '--data-dir', data_dir,
            '--save-dir', save_dir]


def artifact_digests(root):
    """{relative path: sha256} of every file a run wrote under `root`.  *.npy tables and deletion.npy by their bytes; a log by its
    series without the wall-clock 'time' strings; model*.pth by the names, shapes and bytes of its state dict (not by the
    container torch.save wraps them in); param.pkl by its fields with the data paths cut to their file names."""
    import hashlib
    import pickle
    out = {}
    for d, _, files in os.walk(root):
        for f in sorted(files):
            path = os.path.join(d, f)
            h = hashlib.sha256()
            if f.startswith('log') and f.endswith('.npy'):
                log = np.load(path, allow_pickle=True).item()
                h.update(repr(sorted((name, v) for name, v in log.items() if name != 'time')).encode())
            elif f.endswith('.pth'):
                for name, t in sorted(torch.load(path, map_location='cpu').items()):
                    h.update(f'{name} {tuple(t.shape)} {t.dtype}'.encode() + t.contiguous().numpy().tobytes())
            elif f == 'param.pkl':
                with open(path, 'rb') as fh:
                    fields = dict(vars(pickle.load(fh)))
                for name in ('train_dir', 'test_dir'):
                    fields[name] = os.path.basename(fields[name])
                h.update(repr(sorted((name, np.asarray(v).tolist() if isinstance(v, np.ndarray) else v) for name, v in fields.items())).encode())
            else:
                with open(path, 'rb') as fh:
                    h.update(fh.read())
            out[os.path.relpath(path, root)] = h.hexdigest()
    return out
