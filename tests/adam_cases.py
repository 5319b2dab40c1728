"""Shared case builders of tests/test_cpu_adam.py and tests/test_gpu_adam.py (no pytest plugin: a plain module beside them).

A case is one shard with made-up ratings: its triples, N(0, 1) start tables, the epoch orders and the learning rates of a StepLR
schedule.  reference(case) holds what both files compare against, computed once per process: the float64 contract
(ultrare_amd.adam.adam_train_ref) and torch.optim.Adam on dense embeddings, in float64 and in float32 on the CPU."""
import functools

import numpy as np
import torch

LAM, BETAS, EPS = 0.1, (0.9, 0.999), 1e-8
G_MIN = 1e-3          # elements whose float64 |g| falls below this at any step are left out of the comparison ...
LEAVE_OUT_CAP = 0.01  # ... at most this share per case


class Case:
    def __init__(self, n_user, n_item, d, N, B, epochs, seed=0, lr=1e-2, lr_decay=0.95, lr_step=1, hot=0.25, no_u=0, no_i=0):
        """N ratings over the users [no_u, n_user) and the items [no_i, n_item) (the first no_u users and no_i items have none), a
        share `hot` of them on the last item; duplicates of a pair are allowed."""
        rs = np.random.RandomState(1000 + seed)
        self.n_user, self.n_item, self.d, self.N, self.B, self.epochs = n_user, n_item, d, N, B, epochs
        self.lr, self.lr_decay, self.lr_step = lr, lr_decay, lr_step
        self.uid = rs.randint(no_u, n_user, N).astype(np.int32)
        self.iid = rs.randint(no_i, n_item - 1 if hot else n_item, N).astype(np.int32)
        self.iid[rs.permutation(N)[:int(N * hot)]] = n_item - 1
        self.rating = (rs.randint(1, 6, N) / 5).astype(np.float32)
        self.U0 = rs.standard_normal((n_user, d)).astype(np.float32)
        self.V0 = rs.standard_normal((n_item, d)).astype(np.float32)
        self.orders = np.stack([rs.permutation(N) for _ in range(epochs)]).astype(np.int32)
        # StepLR as engine.TrainJob makes it: float32 values
        self.lr_host = np.array([lr * (lr_decay ** (t // lr_step)) for t in range(epochs)], dtype=np.float32)
        self.steps = (N + B - 1) // B
        self.no_u, self.no_i = no_u, no_i

    def __repr__(self):
        return f'{self.n_user}x{self.n_item}-d{self.d}-N{self.N}-B{self.B}-E{self.epochs}'

    def job(self, **kw):
        """The case as a one-shard Adam job on the current device."""
        return make_job([self], **kw)


def make_job(cases, **kw):
    from ultrare_amd import engine
    c0 = cases[0]
    shards = [engine.ShardData(c.uid, c.iid, c.rating, c.n_user, c.n_item) for c in cases]
    args = dict(optimizer='adam', betas=BETAS, eps=EPS)
    args.update(kw)
    return engine.TrainJob(shards, [(c.U0, c.V0) for c in cases], [c.orders for c in cases], c0.d, c0.B, c0.epochs, c0.lr, LAM, 0.9,
                           c0.lr_decay, c0.lr_step, **args)


# (n_user, n_item, d, N, B, epochs): one case per kind of row width (narrow, 32, and the two-pieces-per-lane widths 64, 128, 256).  One item draws a quarter
# of the ratings: more than one work unit (8 * lanes slots) at every width, beside rows of a single unit.
WHOLE_STEP_CASES = [
    Case(40, 30, 8, 600, 256, 4, seed=1),
    Case(70, 50, 32, 2000, 512, 3, seed=2),
    Case(33, 21, 64, 900, 300, 3, seed=3),
    Case(45, 35, 128, 800, 300, 3, seed=4),
    Case(50, 40, 256, 1200, 500, 3, seed=5),
]


def decay_case(d):
    """37 x 29, 9 users and 7 items without a rating, 3 steps per epoch (the last partial), every epoch its own learning rate."""
    return Case(37, 29, d, 300, 128, 3, seed=10 + d, hot=0, no_u=9, no_i=7)


def torch_adam(case, dtype):
    """torch.optim.Adam(weight_decay=lam) on two dense embeddings with MSELoss(sum), on the CPU in `dtype`, the betas, eps and lam at
    their float32 values: -> (U, V, loss [epochs]) as numpy arrays."""
    from ultrare_amd.adam import betas32
    b1, b2, eps = betas32(BETAS, EPS)
    U = torch.nn.Embedding(case.n_user, case.d, dtype=dtype)
    V = torch.nn.Embedding(case.n_item, case.d, dtype=dtype)
    with torch.no_grad():
        U.weight.copy_(torch.from_numpy(case.U0))
        V.weight.copy_(torch.from_numpy(case.V0))
    opt = torch.optim.Adam(list(U.parameters()) + list(V.parameters()), lr=float(case.lr_host[0]), betas=(b1, b2), eps=eps,
                           weight_decay=float(np.float32(LAM)))
    loss_fn = torch.nn.MSELoss(reduction='sum')
    uid, iid = torch.from_numpy(case.uid.astype(np.int64)), torch.from_numpy(case.iid.astype(np.int64))
    r = torch.from_numpy(case.rating).to(dtype)
    losses = np.zeros(case.epochs)
    for e in range(case.epochs):
        for g in opt.param_groups:
            g['lr'] = float(case.lr_host[e])
        order = torch.from_numpy(case.orders[e].astype(np.int64))
        for s in range(case.steps):
            idx = order[s * case.B:(s + 1) * case.B]
            opt.zero_grad()
            loss = loss_fn((U(uid[idx]) * V(iid[idx])).sum(1), r[idx])
            loss.backward()
            opt.step()
            losses[e] += float(loss.detach().double())
    return U.weight.detach().numpy().copy(), V.weight.detach().numpy().copy(), losses


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> dict: 'f64' (U, V, loss) of the float64 contract, 'keep' (mask_U, mask_V) of the elements that are compared, 'left_out' their
    complement's share, 't32' torch's float32 run, 'E_t' its distance from the contract."""
    from ultrare_amd.adam import adam_train_ref
    U, V, loss, gu, gv = adam_train_ref(case.uid, case.iid, case.rating, case.U0, case.V0, case.orders, case.B, case.lr_host, LAM, BETAS, EPS)
    keep = (gu >= G_MIN, gv >= G_MIN)
    left_out = 1.0 - (keep[0].sum() + keep[1].sum()) / (keep[0].size + keep[1].size)
    t32 = torch_adam(case, torch.float32)
    ref = dict(f64=(U, V, loss), keep=keep, left_out=float(left_out), t32=t32)
    ref['E_t'] = distance(ref, *t32)
    return ref


def distance(ref, U, V, loss):
    """max over the compared elements of |table - contract| and over the epochs of the relative loss difference."""
    U64, V64, loss64 = ref['f64']
    ku, kv = ref['keep']
    return float(max(np.abs(U.astype(np.float64) - U64)[ku].max(), np.abs(V.astype(np.float64) - V64)[kv].max(),
                     np.abs(np.asarray(loss, dtype=np.float64) / loss64 - 1.0).max()))


def ulp32(x):
    return float(np.spacing(np.float32(x)))
