"""Adversarial attribute unlearning, stated in numpy: the contract of csrc/adv.hip (include/ultrare_adv.h) and of
engine.attack_input_grad / engine.adversarial_unlearn / utils.adversarial_unlearn.  Nothing here touches the device.

A discriminator is trained to tell the two attribute groups apart and the embeddings are moved so that it cannot.  The discriminator
is the probe of attack.py, cross-validated: a position is always judged by the fold that HELD IT OUT, a discriminator that has never
trained on that row.  The reference ships nothing like it, so this is opt-in and no parity claim.  The rules are attack.py's: every
float32 operation is rounded on its own, chains start from +0.0 in ascending index, dtype=float64 is the reference execution.

  input gradient  of the ROW'S OWN term w_class[f][y] * CE(p, target[y]) with respect to the row, f = fold_of[i]:
                  forward = attack.forward_ref; p = attack._sigmoid of the float32 logit (float64, rounded once);
                  coef = fl(w_class[f][y] * fl(p - target[y])) -- no division by m_train;
                  delta_h = fl(coef * w2[h]) where a_h > 0, else +0.0 (H = 0: the one linear unit, delta = coef);
                  s_c = the chain over h = 0 .. He - 1 from +0.0 of fl(delta_h * W1[h][c]); grad[i][c] = fl(s_c * inv_std[f][c]).
                  No gradient through the mean or 1 / std: they are constants of the round.
  target          (0, 1) is the attacker's own class-balanced cross-entropy; (0.5, 0.5) is the CONFUSION target, whose minimum is
                  p = 1 / 2 for both classes.  Ascending the attacker's cross-entropy instead ('reverse') diverges on this contract
                  (rows moved by 46, AUC 0.96) and is not offered.
  round t         attack.standardize_ref on the current rows; disc_epochs epochs of attack.train_ref's training from the previous
                  round's parameters (Adam's moments and bias correction restart every round); the input gradient at the new
                  parameters; x <- float32(x - lr (eta g + 2 alpha (x - x*))), evaluated in float64 and rounded once, x* the rows at
                  entry (utils.attribute_unlearn's update line).
"""
import numpy as np

from . import attack as A
from .attr_unlearn import _real, check_groups

TARGETS = {'confuse': (0.5, 0.5)}
# chosen on the two synthetic tables of tests/attack_cases.py (the sweep) and UNTUNED on real attribute data
DEFAULTS = dict(hidden=32, folds=5, rounds=100, disc_epochs=5, disc_lr=1e-2, l2=1e-4, lr=0.1, eta=1.0, alpha=0.0, target='confuse', seed=0)
PLANTS = ('own_fold', 'no_inv_std', 'relu_mask_dropped', 'target_is_label', 'stale_stats')


def check_target(target):
    if target == 'reverse':
        raise ValueError("target 'reverse' (gradient reversal: ascending the discriminator's cross-entropy) is not offered: it diverges on "
                         "the contract (rows moved by 46, the fresh attacker's AUC 0.96); use 'confuse'")
    if not isinstance(target, str) or target not in TARGETS:
        raise ValueError(f"target must be 'confuse', not {target!r}")
    return TARGETS[target]


def check_loop(rounds=100, disc_epochs=5, disc_lr=1e-2, l2=1e-4, lr=0.1, eta=1.0, alpha=0.0, target='confuse'):
    """The settings of the round loop, or ValueError -> (rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, (target0, target1))."""
    rounds, disc_epochs = A._int('rounds', rounds, 1, 1 << 20), A._int('disc_epochs', disc_epochs, 1, 1 << 20)
    disc_lr, lr = _real('disc_lr', disc_lr, positive=True), _real('lr', lr, positive=True)
    eta, alpha, l2 = _real('eta', eta), _real('alpha', alpha), _real('l2', l2)
    for name, v in (('eta', eta), ('alpha', alpha), ('l2', l2)):
        if v < 0:
            raise ValueError(f'{name} must be >= 0, not {v!r}')
    return rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, check_target(target)


def check_adv_args(n_rows, d, id1, id2, hidden=32, folds=5, rounds=100, disc_epochs=5, disc_lr=1e-2, l2=1e-4, lr=0.1, eta=1.0, alpha=0.0,
                   target='confuse'):
    """Every refusal, before any device work -> (rows int32 [n1 + n2], n1, n2, H, folds, rounds, disc_epochs, disc_lr, l2, lr, eta,
    alpha, (target0, target1)).  hidden and folds are attack.check_settings', the groups attr_unlearn.check_groups'."""
    loop = check_loop(rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, target)
    A._int('hidden', hidden, 0, A.MAX_H), A._int('the table width d', d, 1, A.MAX_D), A._int('folds', folds, 2, A.MAX_FOLDS)
    rows, n1, n2 = check_groups(id1, id2, n_rows)
    H, folds = A.check_settings(d, n1, n2, hidden, folds, loop[1], loop[2], loop[3])[:2]
    return (rows, n1, n2, H, folds) + loop


def fold_weights(n1, fold_of, folds, dtype=np.float32):
    """fw [folds, 4] = (w_class of class 0, of class 1, m_train, 0) of every fold: ure_attack_train's and ure_adv_input_grad's."""
    fold_of = np.asarray(fold_of)
    y = np.arange(len(fold_of)) < n1
    fw = np.zeros((folds, 4), dtype=dtype)
    for f in range(folds):
        cw, m_train = A.class_weights(y, fold_of != f, dtype=dtype)
        fw[f, :2], fw[f, 2] = cw, m_train
    return fw


def fold_groups(fold_of, folds):
    """The plan of ure_adv_input_grad -> (perm int32 [m], fold_off int32 [folds + 2]): the positions grouped by fold in ascending
    order, group `folds` holding those whose fold lies outside [0, folds)."""
    fo = np.asarray(fold_of, dtype=np.int64)
    key = np.where((fo >= 0) & (fo < folds), fo, folds)
    perm = np.argsort(key, kind='stable').astype(np.int32)
    off = np.zeros(folds + 2, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(key, minlength=folds + 1))
    return perm, off


def input_grad_ref(params, stats, x, y, fold_of, fw, target, H, dtype=np.float32, p=None, plant=None):
    """-> (grad [m, d], p [m]) of the rows x [m, d] with labels y under the sets fold_of (None: set 0); the module docstring's
    lines.  A fold_of entry outside [0, folds) gives a NaN row and a NaN p.  p given (float32 [m], the device's own): the sigmoid
    is skipped and everything after it is pure float32 -- the bit-for-bit half.  plant: tests only."""
    assert plant is None or plant in PLANTS
    T = dtype
    x = np.asarray(x)
    m, d = x.shape
    folds, He = len(params), max(H, 1)
    fo = np.zeros(m, dtype=np.int64) if fold_of is None else np.asarray(fold_of, dtype=np.int64)
    y = np.asarray(y).astype(np.int64)
    tgt = np.asarray(target, dtype=np.float32).astype(T)
    if plant == 'target_is_label':
        tgt = np.array([0, 1], dtype=T)
    grad, p_out = np.full((m, d), np.nan, dtype=T), np.full(m, np.nan, dtype=T)
    for f in range(folds):
        at = np.flatnonzero(fo == f)
        if not len(at):
            continue
        g = (f + 1) % folds if plant == 'own_fold' else f           # (a set that trained on these positions)
        W1, b1, w2, b2 = A.unpack(np.asarray(params[g], dtype=T), d, H)
        logit, z, r = A.forward_ref(params[g], stats[g], x[at], d, H, dtype=T)
        pf = A._sigmoid(logit.astype(T)) if p is None else np.asarray(p)[at].astype(T)
        wrow = np.asarray(fw, dtype=T)[g, :2][y[at]]
        coef = (wrow * (pf - tgt[y[at]])).astype(T)
        if H == 0:
            delta = coef[:, None]
        elif plant == 'relu_mask_dropped':
            delta = (coef[:, None] * w2[None, :]).astype(T)
        else:
            delta = np.where(r > 0, coef[:, None] * w2[None, :], T(0)).astype(T)
        s = np.zeros((len(at), d), dtype=T)
        for h in range(He):
            s = s + delta[:, h][:, None] * W1[h][None, :]
        inv = np.ones(d, dtype=T) if plant == 'no_inv_std' else np.asarray(stats[g][1], dtype=T)
        grad[at], p_out[at] = s * inv[None, :], pf
    return grad, p_out


def update_ref(x, start, g, lr, eta, alpha):
    """x <- float32(x - lr (eta g + 2 alpha (x - x*))): float64, rounded once."""
    x64 = np.asarray(x).astype(np.float64)
    return (x64 - lr * (eta * np.asarray(g).astype(np.float64) + (2.0 * alpha) * (x64 - np.asarray(start).astype(np.float64)))).astype(np.float32)


def adversarial_unlearn_ref(X, rows, n1, fold_of, params0, H, rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, target=(0.5, 0.5),
                            dtype=np.float64, plant=None):
    """The round loop on the rows `rows` of the float32 table X -> (the moved table float32, log).  log: loss_first / loss_last float64
    [rounds, folds] (the discriminator's loss of the round's first and last epoch), gt / eq int64 [rounds] (the pair counts of the
    round's out-of-fold p as float32: the in-loop AUC is (gt + eq / 2) / (n1 n2)), reg float64 [rounds] (sum |x - x*|^2 after the
    round's update), p_rounds [rounds, m], and of the LAST round p [m], grad [m, d], params [folds, P], stats.  plant: tests only ('stale_stats': the
    gradient is taken under the statistics of round 0)."""
    T = dtype
    X = np.array(X, dtype=np.float32)
    rows = np.asarray(rows, dtype=np.int64)
    fold_of = np.asarray(fold_of)
    m, folds = len(rows), len(params0)
    y = (np.arange(m) < n1).astype(np.int64)
    fw = fold_weights(n1, fold_of, folds, dtype=T)
    start = X[rows].copy()
    params = np.asarray(params0).astype(T)
    pos, neg = np.arange(n1), np.arange(n1, m)
    log = dict(loss_first=np.zeros((rounds, folds)), loss_last=np.zeros((rounds, folds)), gt=np.zeros(rounds, dtype=np.int64),
               eq=np.zeros(rounds, dtype=np.int64), reg=np.zeros(rounds), p_rounds=np.zeros((rounds, m), dtype=T))
    stats0 = None
    for t in range(rounds):
        fit = A.train_ref(X, rows, n1, fold_of, params, H, disc_epochs, disc_lr, l2, dtype=T)
        params, stats = fit['params'], fit['stats']
        stats0 = stats if stats0 is None else stats0
        x = X[rows]
        g, p = input_grad_ref(params, stats0 if plant == 'stale_stats' else stats, x, y, fold_of, fw, target, H, dtype=T, plant=plant)
        log['loss_first'][t], log['loss_last'][t] = fit['loss'][:, 0], fit['loss'][:, -1]
        log['p_rounds'][t] = p
        log['gt'][t], log['eq'][t] = A.auc_counts_ref(p.astype(np.float32), pos, neg)
        X[rows] = update_ref(x, start, g, lr, eta, alpha)
        delta = X[rows].astype(np.float64) - start.astype(np.float64)
        log['reg'][t] = float((delta * delta).sum())
    log.update(p=p, grad=g, params=params, stats=stats)
    return X, log
