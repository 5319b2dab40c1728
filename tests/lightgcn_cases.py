"""Shared case builders of tests/test_cpu_lightgcn.py and tests/test_gpu_lightgcn.py (no pytest plugin: a plain module beside them).

A case is one shard with made-up ratings in the pattern of adam_cases.Case (a hot item, users and items without a rating, repeated
pairs), a width, a layer count and a schedule.  reference(case) holds what both files compare against, computed once per process:
lightgcn.train_ref in float64 -- the contract -- and two float32 CPU executions of the same training: train_ref in float32 and torch
float32 autograd on the dense normalised adjacency."""
import functools

import numpy as np
import torch

import adam_cases
from adam_cases import ulp32                       # noqa: F401
from ultrare_amd import lightgcn

LR = 1e-3
ROW_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 300)
LONG_ROW = 1500
ROW_COUNTS = (1, 67, 257)
N_SRC = 211


class Case(adam_cases.Case):
    """adam_cases.Case (N ratings, a share `hot` on the last item, the first no_u users and no_i items without one, duplicates
    allowed) with a layer count, a momentum and a weight decay; one pair is repeated on purpose."""

    def __init__(self, n_user, n_item, d, N, B, epochs, layers, seed, lam=0.1, mu=0.9, lr_decay=0.7, lr_step=1, no_u=3, no_i=4):
        super().__init__(n_user, n_item, d, N, B, epochs, seed=seed, lr=LR, lr_decay=lr_decay, lr_step=lr_step, no_u=no_u, no_i=no_i)
        self.uid[-1], self.iid[-1] = self.uid[0], self.iid[0]           # a repeated pair, apart in the file
        self.layers, self.lam, self.mu = layers, lam, mu

    def __repr__(self):
        return f'{super().__repr__()}-L{self.layers}'

    def graph(self):
        from ultrare_amd import engine
        return engine.GcnGraph(self.uid, self.iid, self.rating, self.n_user, self.n_item)

    def job(self, graph=None, **kw):
        """The case as a GcnJob on the current device."""
        from ultrare_amd import engine
        args = dict(layers=self.layers)
        args.update(kw)
        return engine.GcnJob(graph or self.graph(), (self.U0, self.V0), self.orders, self.d, args.pop('layers'), self.B, self.epochs, LR, self.lam,
                             self.mu, self.lr_decay, self.lr_step, **args)

    def train_ref(self, dtype=np.float64, plant=None, layers=None):
        return lightgcn.train_ref(self.uid, self.iid, self.rating, self.U0, self.V0, self.orders, self.B, self.lr_host, self.lam, self.mu,
                                  self.layers if layers is None else layers, dtype=dtype, plant=plant)


# (n_user, n_item, d, N, B, epochs, layers): widths 8, 32, 64, 128, 256 and L = 1, 2, 3; the last step of an epoch is partial, a
# quarter of the ratings sit on one item (a row of 100+ entries beside rows of one), lr differs from epoch to epoch
WHOLE_STEP_CASES = [
    Case(40, 30, 8, 500, 200, 3, 1, seed=1),
    Case(50, 45, 32, 700, 300, 3, 2, seed=2),
    Case(33, 21, 64, 400, 150, 3, 3, seed=3),
    Case(45, 35, 128, 450, 200, 2, 2, seed=4),
    Case(30, 40, 256, 420, 200, 2, 1, seed=5, lam=0.03, mu=0.5),
]
# the same five graphs at small widths, for the float64 checks on the CPU (the width plays no part there)
SMALL_CASES = [Case(c.n_user, c.n_item, 4 + 4 * i, c.N, c.B, c.epochs, c.layers, seed=10 + i, lam=c.lam, mu=c.mu) for i, c in enumerate(WHOLE_STEP_CASES)]


def torch_lightgcn(case, dtype, layers=None):
    """LightGCN with torch autograd on the DENSE normalised adjacency A [n_user, n_item] (an entry per triple, repeated pairs added),
    MSELoss(sum) and torch.optim.SGD(momentum, weight_decay), on the CPU in `dtype` -> dict as lightgcn.train_ref returns it."""
    L = case.layers if layers is None else layers
    g = lightgcn.Graph(case.uid, case.iid, case.n_user, case.n_item)
    A = np.zeros((case.n_user, case.n_item))
    np.add.at(A, (case.uid, case.iid), g.s_u[case.uid].astype(np.float64) * g.s_i[case.iid].astype(np.float64))
    A = torch.from_numpy(A).to(dtype)
    P = torch.from_numpy(case.U0).to(dtype).clone().requires_grad_(True)
    Q = torch.from_numpy(case.V0).to(dtype).clone().requires_grad_(True)
    opt = torch.optim.SGD([P, Q], lr=float(case.lr_host[0]), momentum=float(np.float32(case.mu)), weight_decay=float(np.float32(case.lam)))
    loss_fn = torch.nn.MSELoss(reduction='sum')
    uid, iid = torch.from_numpy(case.uid.astype(np.int64)), torch.from_numpy(case.iid.astype(np.int64))
    r = torch.from_numpy(case.rating).to(dtype)
    c = float(lightgcn.layer_scale(L))                 # the contract's constant: float32(1 / (L + 1))

    def forward():
        Xu, Xi, Su, Si = P, Q, P, Q
        for _ in range(L):
            Xu, Xi = A @ Xi, A.t() @ Xu
            Su, Si = Su + Xu, Si + Xi
        return Su * c, Si * c

    out = dict(U=[], V=[], P=[], Q=[])
    sse = np.zeros(case.epochs)
    for e in range(case.epochs):
        for grp in opt.param_groups:
            grp['lr'] = float(case.lr_host[e])
        order = torch.from_numpy(case.orders[e].astype(np.int64))
        for s in range(case.steps):
            idx = order[s * case.B:(s + 1) * case.B]
            opt.zero_grad()
            U, V = forward()
            loss = loss_fn((U[uid[idx]] * V[iid[idx]]).sum(1), r[idx])
            loss.backward()
            opt.step()
            sse[e] += float(loss.detach().double())
        with torch.no_grad():
            U, V = forward()
        for name, t in (('U', U), ('V', V), ('P', P), ('Q', Q)):
            out[name].append(t.detach().numpy().copy())
    out = {k: np.stack(v) for k, v in out.items()}
    out['sse'], out['loss'] = sse, np.sqrt(sse / case.N)
    return out


def distance(ref64, run):
    """The maximum absolute difference over both final tables and both parameter tables after the last epoch, plus the maximum
    relative difference over the epoch losses.  Nothing is left out."""
    tab = max(float(np.abs(np.asarray(run[k][-1], dtype=np.float64) - ref64[k][-1]).max()) for k in ('U', 'V', 'P', 'Q'))
    return tab + float(np.abs(np.asarray(run['loss'], dtype=np.float64) / ref64['loss'] - 1.0).max())


def wmax(ref64):
    return float(max(np.abs(ref64[k]).max() for k in ('U', 'V', 'P', 'Q')))


@functools.lru_cache(maxsize=None)
def reference(case, layers=None):
    """-> dict: 'f64' the contract, 'f32' train_ref in float32 (the bit contract of the job), 't32' torch's float32 run, 'E_y' the
    larger of their two distances from 'f64', 'bound' = 4 * max(E_y, ulp32(largest |w|)): the factor the Adam and SGD tests use."""
    ref = dict(f64=case.train_ref(layers=layers), f32=case.train_ref(dtype=np.float32, layers=layers), t32=torch_lightgcn(case, torch.float32, layers=layers))
    ref['E_y'] = max(distance(ref['f64'], ref['f32']), distance(ref['f64'], ref['t32']))
    ref['bound'] = 4 * max(ref['E_y'], ulp32(wmax(ref['f64'])))
    return ref


def prop_rows(n_rows, seed=0):
    """A matrix for the propagate tests as triples (row, index): n_rows rows over N_SRC sources whose lengths run through
    ROW_LENGTHS (row 0 and the last row are empty when there are at least three), one row of LONG_ROW entries when there are 67 or
    more; a single row has 300.  Indices are drawn with repeats; 0 and N_SRC - 1 both occur."""
    rs = np.random.RandomState(100 + n_rows + seed)
    if n_rows == 1:
        lengths = [300]
    else:
        lengths = [ROW_LENGTHS[(r * 7) % len(ROW_LENGTHS)] for r in range(n_rows)]
        lengths[1:1 + len(ROW_LENGTHS)] = ROW_LENGTHS[::-1]                   # every length, whatever n_rows >= 22
        lengths[0] = lengths[-1] = 0
        if n_rows >= 67:
            lengths[n_rows // 2] = LONG_ROW
    row = np.repeat(np.arange(n_rows), lengths).astype(np.int32)
    idx = rs.randint(0, N_SRC, len(row)).astype(np.int32)
    idx[0], idx[-1] = 0, N_SRC - 1
    return row, idx, lengths
