"""Shared case builders of tests/test_cpu_attr_train.py and tests/test_gpu_attr_train.py (no pytest plugin: a plain module beside them).

A case is a bpr_cases.Case (one shard of made-up ratings, a width, a layer count, a schedule, the key of the BPR negatives) with two
attribute groups of users, a dis_type and a loss.  reference(case) holds what both files compare against, computed once per process:
attr_train.train_ref in float64 -- the contract -- and two float32 CPU executions of the same training: train_ref in float32 and
torch float32 autograd of the reference's LITERAL loss (rbk as written with its m x m x d temporary, or trace(U^T Lap U) with a dense
Laplacian)."""
import functools

import numpy as np
import torch

import bpr_cases
import lightgcn_cases as C
from adam_cases import ulp32
from ultrare_amd import attr_train, bpr, lightgcn


class Case(bpr_cases.Case):
    def __init__(self, n_user, n_item, d, N, B, epochs, layers, seed, var, loss='mse', eta=1.0, fix_sigma=None, **kw):
        super().__init__(n_user, n_item, d, N, B, epochs, layers, seed=seed, **kw)
        self.var, self.loss, self.eta, self.fix_sigma = var, loss, eta, fix_sigma
        # group 1: the even users, group 2: the odd ones, the users 5, 6 and 7 in neither; the first no_u users have no rating
        ids = np.arange(n_user)
        free = (ids >= 5) & (ids <= 7)
        self.id1, self.id2 = ids[(ids % 2 == 0) & ~free], ids[(ids % 2 == 1) & ~free]

    def __repr__(self):
        return f'{C.Case.__repr__(self)}-{self.loss}-{self.var}'

    def job(self, graph=None, **kw):
        args = dict(loss=self.loss, key=self.key, attr=(self.id1, self.id2), dis_type=self.var, eta=self.eta, fix_sigma=self.fix_sigma)
        args.update(kw)
        return C.Case.job(self, graph, **args)

    def train_ref(self, dtype=np.float64, layers=None, **kw):
        args = dict(eta=self.eta, fix_sigma=self.fix_sigma, dtype=dtype, loss=self.loss, key=self.key)
        args.update(kw)
        return attr_train.train_ref(self.uid, self.iid, self.rating, self.U0, self.V0, self.orders, self.B, self.lr_host, self.lam, self.mu,
                                    self.layers if layers is None else layers, self.id1, self.id2, self.var, **args)


# ---- the reference's literal losses, in torch ---------------------------------------------------------------------------------------
def rbk(source, target, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
    """utils.py:223-256 restated: the m x m x d temporary and all."""
    n = int(source.size(0)) + int(target.size(0))
    total = torch.cat([source, target], dim=0)
    total0 = total.unsqueeze(0).expand(n, n, int(total.size(1)))
    total1 = total.unsqueeze(1).expand(n, n, int(total.size(1)))
    L2 = ((total0 - total1) ** 2).sum(2)
    bandwidth = fix_sigma if fix_sigma else torch.sum(L2.detach()) / (n ** 2 - n)
    bandwidth = bandwidth / kernel_mul ** (kernel_num // 2)
    return sum(torch.exp(-L2 / (bandwidth * kernel_mul ** i)) for i in range(kernel_num))


def mmd_loss(source, target, **kw):
    n1 = int(source.size(0))
    K = rbk(source, target, **kw)
    return torch.mean(K[:n1, :n1]) + torch.mean(K[n1:, n1:]) - torch.mean(K[:n1, n1:]) - torch.mean(K[n1:, :n1])


def dense_laplacian(n_user, user1, user2, dtype):
    """D - A of the complete bipartite graph user1 - user2, dense n_user x n_user (utils.py:270-279)."""
    A = np.zeros((n_user, n_user))
    for i in user1:
        for j in user2:
            A[i, j] = A[j, i] = 1.0
    return torch.from_numpy(np.diag(A.sum(axis=1)) - A).to(dtype)


def torch_groups(user, id1, id2):
    """The reference's lines 68-70."""
    uni = user.unique()
    return uni[torch.isin(uni, id1)], uni[torch.isin(uni, id2)]


def torch_train(case, dtype, layers=None, eta_of_step=None):
    """Training with torch autograd of the literal loss MSELoss(sum) (or the BPR sum) + eta * mmd_loss(U*[user1], U*[user2]) or
    + eta * trace(U*^T Lap U*), LightGCN on the dense normalised adjacency, torch.optim.SGD, on the CPU in `dtype`.  A step with an
    empty group has no term (the literal loss is NaN there).  -> dict as attr_train.train_ref returns it."""
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
    id1, id2 = torch.from_numpy(case.id1.astype(np.int64)), torch.from_numpy(case.id2.astype(np.int64))
    c = float(lightgcn.layer_scale(L))
    if case.loss == 'bpr':
        off_d, col_d = bpr.distinct_csr(g)

    def forward():
        Xu, Xi, Su, Si = P, Q, P, Q
        for _ in range(L):
            Xu, Xi = A @ Xi, A.t() @ Xu
            Su, Si = Su + Xu, Si + Xi
        return Su * c, Si * c

    out = dict(U=[], V=[], P=[], Q=[])
    base, dis, skipped = np.zeros(case.epochs), np.zeros(case.epochs), np.zeros(case.epochs, dtype=np.int64)
    for e in range(case.epochs):
        for grp in opt.param_groups:
            grp['lr'] = float(case.lr_host[e])
        if case.loss == 'bpr':
            neg_file = np.empty(case.N, dtype=np.int64)
            neg_file[g.pos] = bpr.sample_ref(g, off_d, col_d, case.key, e)
            neg_file = torch.from_numpy(neg_file)
        order = torch.from_numpy(case.orders[e].astype(np.int64))
        for s in range(case.steps):
            idx = order[s * case.B:(s + 1) * case.B]
            opt.zero_grad()
            U, V = forward()
            if case.loss == 'bpr':
                x = (U[uid[idx]] * V[iid[idx]]).sum(1) - (U[uid[idx]] * V[neg_file[idx]]).sum(1)
                loss = -torch.nn.functional.logsigmoid(x).sum()
            else:
                loss = loss_fn((U[uid[idx]] * V[iid[idx]]).sum(1), r[idx])
            base[e] += float(loss.detach().double())
            user1, user2 = torch_groups(uid[idx], id1, id2)
            term = None
            if len(user1) and len(user2):
                if case.var == 'u2u':
                    term = torch.trace(U.T @ (dense_laplacian(case.n_user, user1.tolist(), user2.tolist(), dtype) @ U))
                else:
                    term = mmd_loss(U[user1], U[user2], fix_sigma=case.fix_sigma)
                    if not bool(torch.isfinite(term)):
                        term = None
            if term is None:
                skipped[e] += 1
            else:
                eta = case.eta if eta_of_step is None else float(eta_of_step(e, s))
                dis[e] += float(term.detach().double())
                loss = loss + eta * term
            loss.backward()
            opt.step()
        with torch.no_grad():
            U, V = forward()
        for name, t in (('U', U), ('V', V), ('P', P), ('Q', Q)):
            out[name].append(t.detach().numpy().copy())
    out = {k: np.stack(v) for k, v in out.items()}
    out['dis'], out['skipped'] = dis, skipped
    out['loss'] = np.sqrt((base + case.eta * dis) / case.N) if case.loss == 'mse' else (base + case.eta * dis) / case.N
    return out


distance, wmax = C.distance, C.wmax


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> dict: 'f64' the contract, 'f32' train_ref in float32, 't32' torch's float32 run of the literal loss, 'E_y' the larger of their
    two distances from 'f64', 'bound' = 4 * max(E_y, ulp32(largest |w|)): the rule and the factor of lightgcn_cases.reference."""
    ref = dict(f64=case.train_ref(), f32=case.train_ref(dtype=np.float32), t32=torch_train(case, torch.float32))
    ref['E_y'] = max(distance(ref['f64'], ref['f32']), distance(ref['f64'], ref['t32']))
    ref['bound'] = 4 * max(ref['E_y'], ulp32(wmax(ref['f64'])))
    return ref


# the CPU toy: 24 users, 16 items, 200 triples, d = 8, B = 64, 2 epochs
CPU_CASES = [Case(24, 16, 8, 200, 64, 2, layers, seed=70 + i, var=var, no_u=2, no_i=1)
             for i, (layers, var) in enumerate(((0, 'd2d'), (1, 'd2d'), (0, 'u2u'), (1, 'u2u')))]
# whole training on the device: 40 users x 24 items, 600 triples, d = 8, B = 128, 3 epochs
GPU_CASES = [Case(40, 24, 8, 600, 128, 3, layers, seed=80 + i, var=var, loss=loss, no_i=2)
             for i, (layers, var, loss) in enumerate((L, v, l) for L in (0, 2) for v in ('d2d', 'u2u') for l in ('mse', 'bpr'))]
