"""Adversarial attribute unlearning (csrc/adv.hip) measured on the GPU.  One JSON line.  Run by no test.

    python tools/exp_adv.py [--parts time,leak,activity] [--reps 7] [--rounds 100] [--epochs 200] [--step-timeout 900]

time      per shape -- 6,040 x 16, 6,040 x 32 and 162,000 x 128 users, two groups of every other user, the defaults of
          utils.adversarial_unlearn (hidden 32, 5 folds, 5 discriminator epochs per round) -- device time by events, medians over
          --reps with (min, max), of ONE ure_adv_input_grad call (engine.attack_input_grad on a fitted probe) and of a whole fine-tune
          of --rounds rounds, and the fine-tune's peak device memory over what was allocated before; the same for the torch
          composition: nn.Sequential(Linear, ReLU, Linear) discriminators + torch.optim.Adam restarted every round, the folds one
          after another, autograd.grad with respect to the rows, the same round structure and update.
leak      the toy set (tests/golden/toy, 2 uniform shards, 'lightgcn' with 0 layers = MF) trained by Sisa.learn, then an attribute
          direction planted into the merged user table (tools/exp_attack.py's: every other user shifted by three standard deviations
          along one random direction): a fresh attacker's AUC / BAcc / F1 (hidden 100, 5 folds, --epochs) and the ensemble's test
          RMSE / HR@10 before and after Sisa.adversarial_unlearn under its defaults.
activity  the same set, trained plainly; the attribute is the users' activity (above the median number of training ratings against
          the rest), which the embeddings of a trained model do carry: the same figures before and after.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exp_attack import TOY, TOY_USERS, accuracy, event_ms, peak_mb, pick, planted_table, stats, toy_learn, toy_loaders  # noqa: E402

SHAPES = {'ml1m-users-16': (6040, 16), 'ml1m-users-32': (6040, 32), 'cfg3-users': (162000, 128)}


def torch_game(X, id1, id2, hidden, folds, rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, seed):
    """The torch composition of the round loop, in place on X: the same model, loss, optimizer, fold plan, initial parameters, round
    structure and update as the contract."""
    import torch
    from ultrare_amd import adam, attack as A
    n1, n2 = len(id1), len(id2)
    at = torch.from_numpy(np.concatenate([id1, id2])).to(X.device)
    m, d = n1 + n2, X.shape[1]
    fold_of = torch.from_numpy(A.fold_plan(n1, n2, folds, seed)).to(X.device)
    p0 = A.init_params(d, hidden, folds, seed)
    y = (torch.arange(m, device=X.device) < n1).float()
    b1, b2, eps = adam.betas32(A.BETAS, A.EPS)
    nets, weights = [], []
    for f in range(folds):
        net = torch.nn.Sequential(torch.nn.Linear(d, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, 1)).to(X.device)
        W1, bb1, w2, bb2 = A.unpack(p0[f], d, hidden)
        with torch.no_grad():
            net[0].weight.copy_(torch.from_numpy(W1)), net[0].bias.zero_(), net[2].weight.copy_(torch.from_numpy(w2)[None]), net[2].bias.zero_()
        tr = fold_of != f
        n_tr, n_pos = int(tr.sum()), int((tr & (y > 0)).sum())
        nets.append(net)
        weights.append(torch.where(y > 0, n_tr / (2.0 * n_pos), n_tr / (2.0 * (n_tr - n_pos))))
    start = X.index_select(0, at).double()
    for _ in range(rounds):
        x = X.index_select(0, at).requires_grad_(True)
        total = 0.0
        for f in range(folds):
            tr = fold_of != f
            xd = x.detach()
            mean, std = xd[tr].mean(0), xd[tr].std(0, unbiased=False)
            z = (xd[tr] - mean) / std
            opt = torch.optim.Adam(nets[f].parameters(), lr=disc_lr, betas=(b1, b2), eps=eps)
            for _ in range(disc_epochs):
                opt.zero_grad(set_to_none=True)
                loss = torch.nn.functional.binary_cross_entropy_with_logits(nets[f](z)[:, 0], y[tr], weight=weights[f][tr], reduction='sum') / int(tr.sum())
                loss = loss + 0.5 * l2 * (nets[f][0].weight.square().sum() + nets[f][2].weight.square().sum())
                loss.backward()
                opt.step()
            held = ~tr
            logit = nets[f]((x[held] - mean) / std)[:, 0]
            total = total + (weights[f][held] * torch.nn.functional.binary_cross_entropy_with_logits(logit, torch.full_like(logit, 0.5), reduction='none')).sum()
        g = torch.autograd.grad(total, x)[0]
        cur = x.detach().double()
        X.index_copy_(0, at, (cur - lr * (eta * g.double() + (2.0 * alpha) * (cur - start))).float())
    return X


def part_time(reps, rounds):
    import torch
    from ultrare_amd import engine
    from ultrare_amd.adv_unlearn import DEFAULTS
    from ultrare_amd.method import utils
    out = {}
    for name, (n, d) in SHAPES.items():
        X, id1, id2 = planted_table(n, d, 3.0)
        Xt = torch.from_numpy(X).cuda()
        s = dict(DEFAULTS, rounds=rounds)
        groups = engine.GroupRows(id1, id2, n, Xt.device)
        fit = engine.attack_fit(Xt, groups, s['hidden'], s['folds'], 5, s['disc_lr'], s['l2'], 0)
        one = lambda: engine.attack_input_grad(fit, Xt, groups)
        model = utils.MF.from_tables(Xt.clone(), torch.zeros(4, d, device='cuda'))

        def ours():
            model.user_mat.weight.data.copy_(Xt)
            return utils.adversarial_unlearn(model, id1, id2, **s)
        Y = Xt.clone()

        def theirs():
            Y.copy_(Xt)
            return torch_game(Y, id1, id2, s['hidden'], s['folds'], rounds, s['disc_epochs'], s['disc_lr'], s['l2'], s['lr'], s['eta'], s['alpha'], 0)
        (log, mb), (_, mb_t) = peak_mb(ours), peak_mb(theirs)
        rms = lambda T: round(float((T - Xt).square().sum(1).mean().sqrt()), 4)
        out[name] = dict(rows=n, d=d, rounds=rounds, input_grad_ms=stats(event_ms(one, reps)), ms=stats(event_ms(ours, reps)),
                         torch_ms=stats(event_ms(theirs, max(reps // 2, 1))), peak_mb=mb, torch_peak_mb=mb_t,
                         in_loop_auc=[round(log['auc'][0], 4), round(log['auc'][-1], 4)], rms_move=rms(model.user_mat.weight.detach()), torch_rms_move=rms(Y))
    return out


def _before_after(s, id1, id2, tot, epochs, rounds):
    kw = dict(hidden=100, folds=5, epochs=epochs, seed=0)
    out = {'groups': [int(len(id1)), int(len(id2))], 'before': {**pick(s.attribute_attack(id1, id2, **kw)), **accuracy(s, tot)}}
    logs = s.adversarial_unlearn(id1, id2, rounds=rounds)
    moved = [g for g in logs if 'skipped' not in g]
    out['after'] = {**pick(s.attribute_attack(id1, id2, **kw)), **accuracy(s, tot)}
    out['parts_moved'] = [len(moved), len(logs)]
    out['rms_move'] = round(float(np.sqrt(sum(g['reg'][-1] for g in moved) / max(sum(sum(g['rows']) for g in moved), 1))), 5)
    out['in_loop_auc'] = [[round(g['auc'][0], 4), round(g['auc'][-1], 4)] for g in moved]
    return out


def part_leak(epochs, rounds, train_epochs=20):
    import torch
    loaders = toy_loaders()
    id1, id2 = np.arange(0, TOY_USERS, 2), np.arange(1, TOY_USERS, 2)
    s = toy_learn(loaders, train_epochs)
    U = s.model_list[0].user_mat.weight.detach()
    rs = np.random.RandomState(3)
    direction = rs.randn(U.shape[1])
    shift = 3.0 * float(U.std()) * direction / np.linalg.norm(direction)
    U[torch.from_numpy(id1).to(U.device)] += torch.from_numpy(shift.astype(np.float32)).to(U.device)
    return _before_after(s, id1, id2, loaders[3], epochs, rounds)


def part_activity(epochs, rounds, train_epochs=20):
    from ultrare_amd import _native as nv
    loaders = toy_loaders()
    uid = np.asarray(nv.read_csv(os.path.join(TOY, '0_train.csv'))[0], dtype=np.int64)
    count = np.bincount(uid, minlength=TOY_USERS)
    users = np.flatnonzero(count > 0)
    heavy = count[users] > np.median(count[users])
    return _before_after(toy_learn(loaders, train_epochs), users[heavy], users[~heavy], loaders[3], epochs, rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='time,leak,activity')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--rounds', type=int, default=100)
    ap.add_argument('--epochs', type=int, default=200)
    ap.add_argument('--step-timeout', type=int, default=900)
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child:
        fn = {'time': lambda: part_time(args.reps, args.rounds), 'leak': lambda: part_leak(args.epochs, args.rounds),
              'activity': lambda: part_activity(args.epochs, args.rounds)}[args.child]
        print(json.dumps(fn()))
        return
    out = {}
    for part in args.parts.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', part, '--reps', str(args.reps), '--rounds', str(args.rounds), '--epochs', str(args.epochs)]
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
