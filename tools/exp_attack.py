"""The attribute-inference attacker (csrc/attack.hip) measured on the GPU.  One JSON line.  Run by no test.

    python tools/exp_attack.py [--parts time,leak,train] [--reps 7] [--epochs 200] [--step-timeout 900]

time   per shape -- ml1m-users (6,040 x 16) and cfg3-users (162,000 x 128), two groups of every other user, hidden 100, 5 folds --
       device time by events of utils.attribute_attack's device work (fit + score + pair counts), medians over --reps with (min, max),
       and peak device memory over what was allocated before; the same for the torch composition: nn.Sequential(Linear, ReLU, Linear)
       + torch.optim.Adam, full batch, the folds one after another on standardised rows, and a torch.sort-based AUC.  Both AUCs are
       reported beside the times.
leak   the toy set (tests/golden/toy, 2 uniform shards, 'lightgcn' with 0 layers = MF) trained by Sisa.learn, then an attribute
       direction planted into the merged user table (every other user shifted by three standard deviations along one random
       direction): the attacker's AUC / BAcc / F1 and the ensemble's test RMSE / HR@10 on it, and the same after
       Sisa.attribute_unlearn with var in (d2d, u2u) and eta in (0.1, 1, 10) (steps 10).
train  the same set trained with dis_type nor, d2d (eta 0.1, 1) and u2u (eta 1e-6, 1e-4, 1; a run whose table is no longer finite is
       reported as diverged); the attribute is the users' activity (above the median number of
       training ratings against the rest): the attacker's AUC / BAcc / F1 on the final user table and the test RMSE / HR@10 of each.
Every part runs in a child process of its own under --step-timeout seconds; after a child that fails or runs out of time nothing
more is started."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

SHAPES = {'ml1m-users': (6040, 16), 'cfg3-users': (162000, 128)}


def stats(ts):
    return {'median': round(float(np.median(ts)), 4), 'min': round(float(min(ts)), 4), 'max': round(float(max(ts)), 4)}


def event_ms(fn, reps, warmup=1):
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
    return ts


def peak_mb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def planted_table(n, d, shift, seed=3):
    rs = np.random.RandomState(seed)
    X = (0.1 * rs.randn(n, d)).astype(np.float32)
    id1, id2 = np.arange(0, n, 2), np.arange(1, n, 2)
    direction = rs.randn(d)
    X[id1] += (shift * 0.1 * direction / np.linalg.norm(direction)).astype(np.float32)
    return X, id1, id2


def torch_attack(X, id1, id2, hidden, folds, epochs, lr, l2, seed):
    """The torch composition: the same model, loss, optimizer, fold plan and initial parameters as the contract."""
    import torch
    from ultrare_amd import adam, attack as A
    n1, n2 = len(id1), len(id2)
    at = torch.from_numpy(np.concatenate([id1, id2])).to(X.device)
    x = X.index_select(0, at)
    m, d = x.shape
    fold_of = torch.from_numpy(A.fold_plan(n1, n2, folds, seed)).to(X.device)
    p0 = A.init_params(d, hidden, folds, seed)
    y = (torch.arange(m, device=X.device) < n1).float()
    b1, b2, eps = adam.betas32(A.BETAS, A.EPS)
    scores = torch.empty(m, device=X.device)
    for f in range(folds):
        tr = fold_of != f
        mean, std = x[tr].mean(0), x[tr].std(0, unbiased=False)
        z = (x - mean) / std
        net = torch.nn.Sequential(torch.nn.Linear(d, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, 1)).to(X.device)
        W1, bb1, w2, bb2 = A.unpack(p0[f], d, hidden)
        with torch.no_grad():
            net[0].weight.copy_(torch.from_numpy(W1)), net[0].bias.zero_(), net[2].weight.copy_(torch.from_numpy(w2)[None]), net[2].bias.zero_()
        opt = torch.optim.Adam(net.parameters(), lr=lr, betas=(b1, b2), eps=eps)
        n_tr, n_pos = int(tr.sum()), int((tr & (y > 0)).sum())
        w = torch.where(y > 0, n_tr / (2.0 * n_pos), n_tr / (2.0 * (n_tr - n_pos)))[tr]
        for _ in range(epochs):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(net(z[tr])[:, 0], y[tr], weight=w, reduction='sum') / n_tr
            loss = loss + 0.5 * l2 * (net[0].weight.square().sum() + net[2].weight.square().sum())
            loss.backward()
            opt.step()
        with torch.no_grad():
            held = ~tr
            scores[held] = torch.sigmoid(net(z[held])[:, 0])
    # AUC by one sort: the mean rank of the positives (ties by their mean rank)
    order = torch.sort(scores).values
    lo, hi = torch.searchsorted(order, scores[:n1], right=False), torch.searchsorted(order, scores[:n1], right=True)
    ranks = (lo + hi + 1).double() / 2.0
    return float((ranks.sum() - n1 * (n1 + 1) / 2.0) / (float(n1) * n2))


def part_time(reps, epochs):
    import torch
    from ultrare_amd.method import utils
    out = {}
    for name, (n, d) in SHAPES.items():
        X, id1, id2 = planted_table(n, d, 3.0)
        Xt = torch.from_numpy(X).cuda()
        kw = dict(hidden=100, folds=5, epochs=epochs, lr=1e-2, l2=1e-4, seed=0)
        ours = lambda: utils.attribute_attack(Xt, id1, id2, **kw)
        theirs = lambda: torch_attack(Xt, id1, id2, **kw)
        (res, mb), (auc_t, mb_t) = peak_mb(ours), peak_mb(theirs)
        out[name] = dict(rows=n, d=d, epochs=epochs, ms=stats(event_ms(ours, reps)), torch_ms=stats(event_ms(theirs, max(reps // 2, 1))),
                         peak_mb=mb, torch_peak_mb=mb_t, auc=res['auc'], torch_auc=auc_t)
    return out


TOY = os.path.join(ROOT, 'tests', 'golden', 'toy')
TOY_USERS, TOY_ITEMS, TOY_SHARDS = 1508, 2071, 2


class ToyParam:
    """The InsParam fields Scratch / Sisa read, for the 'lightgcn' backbone with gcn_layers = 0 (plain MF with the term)."""

    def __init__(self, epochs, dis_type='nor', attr=(), dis_eta=1.0):
        self.k, self.lam, self.seed, self.batch = 16, 0.1, 42, 3000
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = TOY_USERS, TOY_ITEMS, False
        self.optimizer, self.gcn_layers = 'sgd', 0
        self.dis_type, self.attr, self.dis_eta = dis_type, list(attr), dis_eta


def toy_loaders():
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(os.path.join(TOY, '0_train.csv'), TOY_USERS, 5, [], [], TOY_SHARDS, [])
    te, _ = readRating(os.path.join(TOY, '0_test.csv'), TOY_USERS, 5, [], [], TOY_SHARDS, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    return idx, trd, ted, loadData(RatingData(np.hstack(te)), 3000, 24, False)


def toy_learn(loaders, train_epochs, dis_type='nor', attr=(), dis_eta=1.0):
    """One Sisa.learn of the toy set (tests/golden/toy: 1,508 users, 2 uniform shards) -> the trained Sisa object."""
    import torch
    from ultrare_amd.method.sisa import Sisa
    idx, trd, ted, tot = loaders
    s = Sisa(ToyParam(train_epochs, dis_type, attr, dis_eta), 'lightgcn', TOY_SHARDS, idx)
    torch.manual_seed(42)
    s.learn(trd, ted, tot, 0, '')
    return s


def accuracy(sisa, tot):
    """Test RMSE and HR@10 of the ensemble on the whole test set (utils.baseTest)."""
    from ultrare_amd.method.utils import baseTest
    rmse, _, hr = baseTest(tot, sisa.model_list)
    return {'rmse': round(float(rmse), 5), 'hr10': round(float(hr), 5)}


def pick(res):
    return {k: round(res[k], 5) for k in ('auc', 'bacc', 'f1')}


def part_leak(epochs, train_epochs=20):
    """A planted attribute direction: every other user's row of the trained, merged user table is shifted along one random direction
    by three times the table's standard deviation.  The attacker and the accuracy before, and after Sisa.attribute_unlearn."""
    import torch
    loaders = toy_loaders()
    id1, id2 = np.arange(0, TOY_USERS, 2), np.arange(1, TOY_USERS, 2)
    kw = dict(hidden=100, folds=5, epochs=epochs, seed=0)

    def planted():
        s = toy_learn(loaders, train_epochs)
        U = s.model_list[0].user_mat.weight.detach()
        rs = np.random.RandomState(3)
        direction = rs.randn(U.shape[1])
        shift = 3.0 * float(U.std()) * direction / np.linalg.norm(direction)
        U[torch.from_numpy(id1).to(U.device)] += torch.from_numpy(shift.astype(np.float32)).to(U.device)
        return s
    s = planted()
    out = {'before': {**pick(s.attribute_attack(id1, id2, **kw)), **accuracy(s, loaders[3])}}
    for var, lr in (('d2d', 0.1), ('u2u', 1e-5)):
        for eta in (0.1, 1.0, 10.0):
            s = planted()
            try:
                s.attribute_unlearn(id1, id2, var=var, eta=eta, steps=10, lr=lr)
                row = {**pick(s.attribute_attack(id1, id2, **kw)), **accuracy(s, loaders[3])}
            except ValueError as e:
                row = {'error': str(e)[:200]}
            out[f'{var}_eta{eta:g}'] = row
    return out


def part_train(epochs, train_epochs=20):
    """In-training: the toy set trained with dis_type nor / d2d / u2u; the attribute is the users' activity (more ratings in the
    training file than the median user against the rest), which the embeddings of a trained model do carry."""
    import torch
    from ultrare_amd import _native as nv
    loaders = toy_loaders()
    uid = np.asarray(nv.read_csv(os.path.join(TOY, '0_train.csv'))[0], dtype=np.int64)
    count = np.bincount(uid, minlength=TOY_USERS)
    users = np.flatnonzero(count > 0)
    heavy = count[users] > np.median(count[users])
    id1, id2 = users[heavy], users[~heavy]
    out = {'groups': [int(len(id1)), int(len(id2))]}
    for dis_type, eta in (('nor', 1.0), ('d2d', 0.1), ('d2d', 1.0), ('u2u', 1e-6), ('u2u', 1e-4), ('u2u', 1.0)):
        s = toy_learn(loaders, train_epochs, dis_type, (id1, id2) if dis_type != 'nor' else (), eta)
        name = dis_type if dis_type == 'nor' else f'{dis_type}_eta{eta:g}'
        if not bool(torch.isfinite(s.model_list[0].user_mat.weight).all()):
            out[name] = {'diverged': True}          # (the summed term outgrew the step size: a finding, not a failure of the tool)
            continue
        out[name] = {**pick(s.attribute_attack(id1, id2, hidden=100, folds=5, epochs=epochs, seed=0)), **accuracy(s, loaders[3])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='time,leak,train')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--epochs', type=int, default=200)
    ap.add_argument('--step-timeout', type=int, default=900)
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child:
        fn = {'time': lambda: part_time(args.reps, args.epochs), 'leak': lambda: part_leak(args.epochs), 'train': lambda: part_train(args.epochs)}[args.child]
        print(json.dumps(fn()))
        return
    out = {}
    for part in args.parts.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', part, '--reps', str(args.reps), '--epochs', str(args.epochs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            out[part] = {'error': f'no result within {args.step_timeout} s'}
            break
        if r.returncode != 0:
            out[part] = {'error': r.stderr[-400:], 'rc': r.returncode}
            break
        out[part] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
