"""Shared case builders of tests/test_cpu_bpr.py and tests/test_gpu_bpr.py (no pytest plugin: a plain module beside them).

A case is a lightgcn_cases.Case (its ratings play no part: every triple is a positive) with a key for the negative draws.
reference(case) holds what both files compare against, computed once per process: bpr.train_ref in float64 -- the contract -- and two
float32 CPU executions of the same training: train_ref in float32 and torch float32 autograd (-logsigmoid on the dense normalised
adjacency, the contract's negatives)."""
import functools

import numpy as np
import torch

import lightgcn_cases as C
from adam_cases import ulp32                       # noqa: F401
from ultrare_amd import bpr, lightgcn

KEYS = (0, 20240608, 2 ** 63 + 5)
EPOCHS = (0, 1, 49)


class Case(C.Case):
    """lightgcn_cases.Case with the key of its negative draws."""

    def __init__(self, *a, key=20240608, **kw):
        super().__init__(*a, **kw)
        self.key = key

    def __repr__(self):
        return f'{super().__repr__()}-bpr'

    def job(self, graph=None, **kw):
        return super().job(graph, **{**dict(loss='bpr', key=self.key), **kw})

    def train_ref(self, dtype=np.float64, plant=None, layers=None):
        return bpr.train_ref(self.uid, self.iid, self.U0, self.V0, self.orders, self.B, self.lr_host, self.lam, self.mu,
                             self.layers if layers is None else layers, self.key, dtype=dtype, plant=plant)

    def host(self):
        """(graph, off_d, col_d) on the host."""
        g = lightgcn.Graph(self.uid, self.iid, self.n_user, self.n_item)
        return (g,) + bpr.distinct_csr(g)


def _like(c, layers=None, **kw):
    return Case(c.n_user, c.n_item, c.d, c.N, c.B, c.epochs, c.layers if layers is None else layers, lam=c.lam, mu=c.mu, **kw)


# the five shapes of lightgcn_cases.WHOLE_STEP_CASES (widths 8 .. 256, L = 1, 2, 3, a partial last step, a hot item) and one with L = 0
WHOLE_STEP_CASES = [_like(c, seed=41 + i) for i, c in enumerate(C.WHOLE_STEP_CASES)] + [_like(C.WHOLE_STEP_CASES[1], layers=0, seed=47)]
# the same graphs at small widths, for the float64 checks on the CPU (the width plays no part there)
SMALL_CASES = [Case(c.n_user, c.n_item, 4 + 4 * i, c.N, c.B, c.epochs, c.layers, seed=50 + i, lam=c.lam, mu=c.mu) for i, c in enumerate(WHOLE_STEP_CASES)]
# one the contract itself learns on: tables of small entries (so no pair starts saturated), a step size that moves them, eight epochs
# (for train_ref only, which reads lr_host: Case.job() would train at lightgcn_cases.LR)
LEARNABLE = Case(40, 30, 8, 500, 200, 8, 1, seed=61, lam=0.01, lr_decay=1.0)
LEARNABLE.U0, LEARNABLE.V0 = (LEARNABLE.U0 * np.float32(0.1)).astype(np.float32), (LEARNABLE.V0 * np.float32(0.1)).astype(np.float32)
LEARNABLE.lr_host = np.full(LEARNABLE.epochs, 0.05, dtype=np.float32)


def torch_bpr(case, dtype, layers=None):
    """BPR with torch autograd on the DENSE normalised adjacency: loss = sum -logsigmoid(s(u, i) - s(u, j)) over the batch, j the
    contract's negative of the epoch, torch.optim.SGD(momentum, weight_decay), on the CPU in `dtype` -> dict as bpr.train_ref's."""
    L = case.layers if layers is None else layers
    g, off_d, col_d = case.host()
    A = np.zeros((case.n_user, case.n_item))
    np.add.at(A, (case.uid, case.iid), g.s_u[case.uid].astype(np.float64) * g.s_i[case.iid].astype(np.float64))
    A = torch.from_numpy(A).to(dtype)
    P = torch.from_numpy(case.U0).to(dtype).clone().requires_grad_(True)
    Q = torch.from_numpy(case.V0).to(dtype).clone().requires_grad_(True)
    opt = torch.optim.SGD([P, Q], lr=float(case.lr_host[0]), momentum=float(np.float32(case.mu)), weight_decay=float(np.float32(case.lam)))
    uid, iid = torch.from_numpy(case.uid.astype(np.int64)), torch.from_numpy(case.iid.astype(np.int64))
    c = float(lightgcn.layer_scale(L))

    def forward():
        Xu, Xi, Su, Si = P, Q, P, Q
        for _ in range(L):
            Xu, Xi = A @ Xi, A.t() @ Xu
            Su, Si = Su + Xu, Si + Xi
        return Su * c, Si * c

    out = dict(U=[], V=[], P=[], Q=[])
    loss_sum = np.zeros(case.epochs)
    for e in range(case.epochs):
        for grp in opt.param_groups:
            grp['lr'] = float(case.lr_host[e])
        neg_file = np.empty(case.N, dtype=np.int64)
        neg_file[g.pos] = bpr.sample_ref(g, off_d, col_d, case.key, e)
        neg_file = torch.from_numpy(neg_file)
        order = torch.from_numpy(case.orders[e].astype(np.int64))
        for s in range(case.steps):
            idx = order[s * case.B:(s + 1) * case.B]
            opt.zero_grad()
            U, V = forward()
            x = (U[uid[idx]] * V[iid[idx]]).sum(1) - (U[uid[idx]] * V[neg_file[idx]]).sum(1)
            loss = -torch.nn.functional.logsigmoid(x).sum()
            loss.backward()
            opt.step()
            loss_sum[e] += float(loss.detach().double())
        with torch.no_grad():
            U, V = forward()
        for name, t in (('U', U), ('V', V), ('P', P), ('Q', Q)):
            out[name].append(t.detach().numpy().copy())
    out = {k: np.stack(v) for k, v in out.items()}
    out['loss_sum'], out['loss'] = loss_sum, loss_sum / case.N
    return out


distance, wmax = C.distance, C.wmax


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> dict: 'f64' the contract, 'f32' train_ref in float32, 't32' torch's float32 run, 'E_y' the larger of their two distances
    from 'f64', 'bound' = 4 * max(E_y, ulp32(largest |w|)): the rule and the factor of lightgcn_cases.reference."""
    ref = dict(f64=case.train_ref(), f32=case.train_ref(dtype=np.float32), t32=torch_bpr(case, torch.float32))
    ref['E_y'] = max(distance(ref['f64'], ref['f32']), distance(ref['f64'], ref['t32']))
    ref['bound'] = 4 * max(ref['E_y'], ulp32(wmax(ref['f64'])))
    return ref


@functools.lru_cache(maxsize=None)
def plant_distance(case, plant):
    """The distance of a planted float64 training from the contract's."""
    return distance(reference(case)['f64'], case.train_ref(plant=plant))


# ------------------------------------------------------------------ graphs for the sampler and the index
def sampler_triples(n_item, nnz, seed=0):
    """(uid, iid, n_user): nnz triples over n_item items whose users' row lengths run through lightgcn_cases.ROW_LENGTHS (cut so
    that every user keeps an item to draw), file order shuffled; every fifth entry repeats its user's previous pair.  With two
    items every user holds item 0 alone: item 1 is every entry's negative and item 0 nobody's."""
    rs = np.random.RandomState(7000 + n_item % 1000 + nnz + seed)
    uid, iid, u = [], [], 0
    while len(uid) < nnz:
        want = min(C.ROW_LENGTHS[(u * 7 + 3) % len(C.ROW_LENGTHS)], nnz - len(uid))
        distinct = min(want, n_item - 1)
        items = np.sort(rs.choice(n_item, distinct, replace=False)) if n_item > 2 else np.zeros(distinct, np.int64)
        row = list(items)
        while len(row) < want and row:
            row.append(row[-1])                             # (rows longer than the catalogue allows: repeated pairs)
        for k in range(4, len(row), 5):
            row[k] = row[k - 1]
        uid += [u] * len(row)
        iid += row
        u += 1
    perm = rs.permutation(nnz)
    return np.asarray(uid, np.int32)[perm], np.asarray(iid, np.int32)[perm], u + 1          # (the last user has no triple)


def long_row_triples():
    """67 users over 2,000 items, lightgcn_cases.prop_rows' lengths: one row of 1,500 entries (drawn with repeats, so pairs repeat)."""
    row, _, lengths = C.prop_rows(67)
    rs = np.random.RandomState(7100)
    iid = rs.randint(0, 2000, len(row)).astype(np.int32)
    perm = rs.permutation(len(row))
    return row[perm], iid[perm], 67, 2000
