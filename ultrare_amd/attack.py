"""The attribute-inference attacker, stated in numpy: the contract of csrc/attack.hip (include/ultrare_attack.h) and of
engine.attack_fit / utils.attribute_attack.  Nothing here touches the device.

The metric of the attribute-unlearning literature: a small MLP is trained on the user embeddings to predict a binary attribute,
cross-validated, and the out-of-fold AUC / balanced accuracy / F1 say how much of the attribute the embeddings still carry.  The
reference ships no attacker, so this is opt-in and no parity claim.

  rows        m = n1 + n2 selected rows of a float32 table; position i < n1 is class 1 (y = 1, attr_unlearn's source group), the
              rest class 0.  fold_of[i] (fold_plan) is the fold that HOLDS position i OUT: fold f trains on fold_of != f.
  parameters  one packed float32 image per fold: [W1 H x d | b1 H | w2 H | b2], or [w d | b] for H = 0 (logistic regression),
              which the kernels read as one linear hidden unit with w2 = 1, b2 = 0 (the same bits).
  stats       standardize_ref: per fold and column the mean and 1 / std of the fold's training rows.  Float64 sums in
              lightgcn.fold_256's order over ALL m positions, a held-out position adding +0.0; the mean first, then the squared
              deviations from it (two passes); the two results rounded to float32 once.  A zero-variance column gets 1 / std = 0.
  forward     z = fl(fl(x - mean) * inv_std); a_h = the chain over c = 0 .. d - 1 from +0.0 of fl(W1[h][c] * z_c), then + b1[h];
              relu (a <= 0 -> +0.0); the logit t = the chain over h of fl(w2[h] * r_h), then + b2; p = 1 / (1 + exp(-t)) evaluated in
              float64 on the float32 logit and rounded to float32 once (the correctly rounded sigmoid but for the float64 exp's last bit).
  gradient    of the class-balanced binary cross-entropy, weights w_class = m_train / (2 n_class) (float32 of the float64 quotient):
              coef = fl(w_class * fl(p - y)) on a training position, +0.0 on a held-out one (masked, not skipped: one row walk
              serves every fold).  delta_h = fl(coef * w2[h]) where a_h > 0, else +0.0.  The sums over positions of
              delta_h z_c, delta_h, coef r_h and coef are two-level chains exactly as nmf._chunk_chain: CHUNK positions per chain in
              ascending order from +0.0, the chunk sums added in chunk order.
  update      g = fl(sum / float32(m_train)); g = fl(g + fl(l2 * w)) on weights (biases: l2 read as 0); then adam.adam_update_ref's
              lines with weight decay 0: full-batch Adam, one step per epoch, the scalars adam.adam_scalars' (betas 0.9 / 0.999,
              eps 1e-8: MLPClassifier's).
  loss        per fold and epoch, at the parameters the epoch starts from: the float64 mean over the training positions of
              w_class * softplus(-t or t) (chunk chains in position order, the chunk sums folded by fold_256) + l2 / 2 |W|^2
              (fold_256 over the packed index, biases adding 0.0).  It holds log and exp: no bit contract.

Everything except exp (and the reported loss) is one float32 operation rounded on its own at dtype=float32; dtype=float64 is the
reference execution.
"""
import numpy as np

from . import adam
from .attr_unlearn import _real, check_groups
from .lightgcn import fold_256

MAX_D = 128             # URE_ATTACK_MAX_D
MAX_H = 128             # URE_ATTACK_MAX_H
MAX_FOLDS = 16          # URE_ATTACK_MAX_FOLDS
MAX_ROWS = 1 << 24      # URE_ATTACK_MAX_ROWS: float32(m_train) is exact up to here
CHUNK = 256             # URE_ATTACK_CHUNK (= nmf.CHUNK)
BETAS = (0.9, 0.999)
EPS = 1e-8
# untuned on real attribute data; chosen on the contract (the sweep's table)
DEFAULT_EPOCHS = 500
DEFAULT_LR = 1e-2


def n_params(d, H):
    return H * d + 2 * H + 1 if H > 0 else d + 1


def _int(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError(f'{name} must be an integer in {lo} .. {hi if hi is not None else ""}, not {v!r}')
    return int(v)


def check_settings(d, n1, n2, hidden=100, folds=5, epochs=None, lr=None, l2=1e-4):
    """The settings of a probe on groups of n1 and n2 rows of width d, or ValueError -> (H, folds, epochs, lr, l2); epochs / lr None are
    the defaults.  The one place these rules are written: check_attack_args and engine.attack_fit both call it."""
    H = _int('hidden', hidden, 0, MAX_H)
    _int('the table width d', d, 1, MAX_D)
    folds = _int('folds', folds, 2, MAX_FOLDS)
    epochs = _int('epochs', DEFAULT_EPOCHS if epochs is None else epochs, 1, 1 << 20)
    lr, l2 = _real('lr', DEFAULT_LR if lr is None else lr, positive=True), _real('l2', l2)
    if l2 < 0:
        raise ValueError(f'l2 must be >= 0, not {l2!r}')
    if min(n1, n2) < folds:
        raise ValueError(f'the groups hold {n1} and {n2} rows: each needs at least folds = {folds}, so that every held-out part has both classes')
    if n1 + n2 > MAX_ROWS:
        raise ValueError(f'{n1 + n2} selected rows: the probe takes at most {MAX_ROWS}')
    return H, folds, epochs, lr, l2


def check_attack_args(n_rows, d, id1, id2, hidden=100, folds=5, epochs=None, lr=None, l2=1e-4):
    """Every refusal, before any device work -> (rows int32 [n1 + n2], n1, n2, H, folds, epochs, lr, l2)."""
    _int('hidden', hidden, 0, MAX_H), _int('the table width d', d, 1, MAX_D), _int('folds', folds, 2, MAX_FOLDS)     # (settings before groups)
    rows, n1, n2 = check_groups(id1, id2, n_rows)
    return (rows, n1, n2) + check_settings(d, n1, n2, hidden, folds, epochs, lr, l2)


def fold_plan(n1, n2, folds, seed):
    """fold_of int32 [n1 + n2]: stratified, from np.random.RandomState(seed), class by class.  Class 1's permutation is dealt to the
    folds 0, 1, 2, ... in turn and class 0's goes on where it stopped: per class and in total the fold sizes differ by at most one."""
    rs = np.random.RandomState(seed)
    fold_of = np.empty(n1 + n2, dtype=np.int32)
    at = 0
    for lo, n in ((0, n1), (n1, n2)):
        perm = rs.permutation(n)
        fold_of[lo + perm] = (at + np.arange(n)) % folds
        at += n
    return fold_of


def init_params(d, H, folds, seed):
    """float32 [folds, P]: Glorot-uniform weights (bound sqrt(6 / (fan_in + fan_out)), MLPClassifier's for relu), zero biases, fold
    after fold from one np.random.RandomState(seed)."""
    rs = np.random.RandomState(seed)
    out = np.zeros((folds, n_params(d, H)), dtype=np.float32)
    for f in range(folds):
        if H > 0:
            b1, b2 = np.sqrt(6.0 / (d + H)), np.sqrt(6.0 / (H + 1))
            out[f, :H * d] = rs.uniform(-b1, b1, H * d)
            out[f, H * d + H:H * d + 2 * H] = rs.uniform(-b2, b2, H)
        else:
            b = np.sqrt(6.0 / (d + 1))
            out[f, :d] = rs.uniform(-b, b, d)
    return out


def unpack(p, d, H):
    """(W1 [He, d], b1 [He], w2 [He] or None, b2 or None) of one packed image; He = max(H, 1)."""
    p = np.asarray(p)
    if H == 0:
        return p[:d].reshape(1, d), p[d:d + 1], None, None
    return p[:H * d].reshape(H, d), p[H * d:H * d + H], p[H * d + H:H * d + 2 * H], p[H * d + 2 * H]


def weight_mask(d, H):
    """bool [P]: which packed entries are weights (the l2 term and its gradient leave the biases out)."""
    m = np.zeros(n_params(d, H), dtype=bool)
    He = max(H, 1)
    m[:He * d] = True
    if H > 0:
        m[H * d + H:H * d + 2 * H] = True
    return m


PLANTS = ('no_class_weight', 'heldout_leaks', 'stats_from_all_rows', 'stale_bias_correction', 'ties_as_wins')


def _fold_256_cols(v):
    """lightgcn.fold_256 of every column of v (float64 [m, d]) at once."""
    m, d = v.shape
    pad = np.zeros((-(-max(m, 1) // 256) * 256, d))
    pad[:m] = v
    part = np.zeros((256, d))
    for chunk in pad.reshape(-1, 256, d):
        part = part + chunk
    w = 128
    while w > 0:
        part[:w] = part[:w] + part[w:2 * w]
        w >>= 1
    return part[0]


def standardize_ref(X, rows, fold_of, folds, dtype=np.float32, plant=None):
    """stats [folds, 2, d] = (mean, 1 / std) of every fold's training rows (the module docstring's order); float32 is the bit
    contract of ure_attack_standardize, float64 leaves the two results unrounded."""
    x = np.asarray(X)[np.asarray(rows, dtype=np.int64)].astype(np.float64)
    fold_of = np.asarray(fold_of)
    out = np.zeros((folds, 2, x.shape[1]), dtype=dtype)
    for f in range(folds):
        mask = np.ones(len(x), dtype=bool) if plant == 'stats_from_all_rows' else fold_of != f
        n = float(mask.sum())
        mean = _fold_256_cols(np.where(mask[:, None], x, 0.0)) / n
        dev = np.where(mask[:, None], x - mean, 0.0)
        var = _fold_256_cols(dev * dev) / n
        with np.errstate(divide='ignore'):
            inv = np.where(var > 0, 1.0 / np.sqrt(var), 0.0)
        out[f, 0], out[f, 1] = mean.astype(dtype), inv.astype(dtype)
    return out


def _sigmoid(t):
    """1 / (1 + exp(-t)) evaluated in float64 and rounded to t's type once."""
    with np.errstate(over='ignore'):
        return (1.0 / (1.0 + np.exp(-t.astype(np.float64)))).astype(t.dtype)


def forward_ref(p, stats_f, x, d, H, dtype=np.float32):
    """One parameter set on the rows x [m, d] -> (logit [m], z [m, d], r [m, He]): r the hidden activations (H = 0: the logit)."""
    T = dtype
    W1, b1, w2, b2 = unpack(np.asarray(p, dtype=T), d, H)
    z = (np.asarray(x).astype(T) - np.asarray(stats_f[0], dtype=T)[None, :]) * np.asarray(stats_f[1], dtype=T)[None, :]
    t = np.zeros((len(z), len(W1)), dtype=T)
    for c in range(d):
        t = t + W1[:, c][None, :] * z[:, c][:, None]
    a = t + b1[None, :]
    if H == 0:
        return a[:, 0], z, a
    r = np.where(a <= 0, T(0), a)
    t = np.zeros(len(z), dtype=T)
    for h in range(H):
        t = t + w2[h] * r[:, h]
    return t + b2, z, r


def _chunks(v):
    """v [m, ...] as [n_chunks, CHUNK, ...], zero rows behind (a +0.0 term leaves a chain's bits alone: it never holds -0.0)."""
    m = len(v)
    nc = -(-m // CHUNK)
    pad = np.zeros((nc * CHUNK,) + v.shape[1:], dtype=v.dtype)
    pad[:m] = v
    return pad.reshape((nc, CHUNK) + v.shape[1:])


def _chunk_chain(term, like):
    """nmf._chunk_chain with every chunk walked at once: term(k) = the term of position k of every chunk [n_chunks, ...]."""
    t = np.zeros_like(like)
    for k in range(CHUNK):
        t = t + term(k)
    total = t[0]
    for j in range(1, len(t)):
        total = total + t[j]
    return total


def class_weights(y, mask, dtype=np.float32, plant=None):
    """(w [2] = (of class 0, of class 1), m_train): m_train / (2 n_class), the float64 quotient rounded to dtype."""
    n = int(mask.sum())
    n1 = int((mask & (y > 0)).sum())
    if plant == 'no_class_weight':
        return np.ones(2, dtype=dtype), n
    with np.errstate(divide='ignore'):
        return np.array([n / (2.0 * (n - n1)), n / (2.0 * n1)]).astype(dtype), n


def grad_ref(p, logit, z, r, y, mask, cw, d, H, dtype=np.float32):
    """-> (g [P] the chunk-chained sums, laid out as the parameters; coef [m]; loss_sum float64 = the fold_256 of the chunks'
    float64 chains of w_class softplus)."""
    T = dtype
    m = len(logit)
    W1, b1, w2, b2 = unpack(np.asarray(p, dtype=T), d, H)
    yT = y.astype(T)
    wrow = np.asarray(cw, dtype=T)[y.astype(np.int64)]
    coef = np.where(mask, wrow * (_sigmoid(logit.astype(T)) - yT), T(0)).astype(T)
    chained = T == np.float32            # float64: numpy's own sums (their order is 2^-53 business, and the yardstick stays quick)
    cz, cc = _chunks(z), _chunks(coef)
    nc = len(cc)
    if H == 0:
        gW = _chunk_chain(lambda k: cc[:, k, None] * cz[:, k], np.zeros((nc, d), dtype=T)) if chained else coef @ z
        gb = _chunk_chain(lambda k: cc[:, k], np.zeros(nc, dtype=T)) if chained else coef.sum()
        g = np.concatenate([gW, [gb]])
    else:
        delta = np.where(r > 0, coef[:, None] * w2[None, :], T(0)).astype(T)
        if chained:
            cd, cr = _chunks(delta), _chunks(np.asarray(r, dtype=T))
            gW = _chunk_chain(lambda k: cd[:, k, :, None] * cz[:, k, None, :], np.zeros((nc, H, d), dtype=T))
            gb1 = _chunk_chain(lambda k: cd[:, k], np.zeros((nc, H), dtype=T))
            gw2 = _chunk_chain(lambda k: cc[:, k, None] * cr[:, k], np.zeros((nc, H), dtype=T))
            gb2 = _chunk_chain(lambda k: cc[:, k], np.zeros(nc, dtype=T))
        else:
            gW, gb1, gw2, gb2 = delta.T @ z, delta.sum(axis=0), coef @ r, coef.sum()
        g = np.concatenate([gW.reshape(-1), gb1, gw2, [gb2]])
    s = np.where(y > 0, -logit, logit).astype(np.float64)
    row = _chunks(np.where(mask, wrow.astype(np.float64) * (np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s)))), 0.0))
    chunks = np.zeros(nc)
    for k in range(CHUNK):
        chunks = chunks + row[:, k]
    return g.astype(T), coef, fold_256(chunks)


def l2_sum_ref(p, d, H):
    """fold_256 over the packed index of float64 w^2, the biases adding 0.0."""
    w = np.asarray(p).astype(np.float64)
    return fold_256(np.where(weight_mask(d, H), w * w, 0.0))


def scalars(epochs, lr, dtype=np.float32):
    """[epochs, 2] = (lr / (1 - beta1^t), sqrt(1 - beta2^t)), t = 1 .. epochs: adam.adam_scalars (float32) or unrounded."""
    b1, b2, _ = adam.betas32(BETAS, EPS)
    lr_host = np.full(epochs, lr, dtype=np.float64)
    return adam.adam_scalars(lr_host, 1, b1, b2) if dtype == np.float32 else adam._scalars64(lr_host, 1, b1, b2)


def adam_ref(w, mom, var, g_sum, m_train, l2, wmask, s1, s2, dtype=np.float32):
    """One update of a fold's packed parameters from the gradient sums -> (w', m', v'), adam.adam_update_ref's order."""
    T = dtype
    b1, b2, eps = (T(v) for v in adam.betas32(BETAS, EPS))
    w, mom, var = (np.asarray(v, dtype=T) for v in (w, mom, var))
    g = np.asarray(g_sum, dtype=T) / T(m_train)
    g = g + np.where(wmask, T(np.float32(l2)), T(0)) * w
    c1, c2 = T(1) - b1, T(1) - b2
    mom = mom + c1 * (g - mom)
    var = b2 * var + (c2 * g) * g
    den = np.sqrt(var) / T(s2) + eps
    return w - T(s1) * (mom / den), mom, var


def train_ref(X, rows, n1, fold_of, params0, H, epochs, lr, l2, dtype=np.float64, plant=None, keep_first_grad=False):
    """Whole training of all folds, then the out-of-fold score of every position from the one fold that held it out.
    -> dict: params [folds, P], stats [folds, 2, d], scores [m], loss float64 [folds, epochs] (+ grad0 [folds, P]: the first
    epoch's gradient sums, when asked).  dtype=float32 is the float32 contract, float64 the yardstick.  plant: tests only."""
    assert plant is None or plant in PLANTS
    T = dtype
    rows = np.asarray(rows, dtype=np.int64)
    x = np.asarray(X)[rows]
    m, d = x.shape
    fold_of = np.asarray(fold_of)
    params0 = np.asarray(params0)
    folds = len(params0)
    y = (np.arange(m) < n1).astype(np.int32)
    stats = standardize_ref(X, rows, fold_of, folds, dtype=T, plant=plant)
    sc = scalars(epochs, lr, dtype=T)
    wmask = weight_mask(d, H)
    out = dict(params=np.zeros(params0.shape, dtype=T), stats=stats, scores=np.zeros(m, dtype=T), loss=np.zeros((folds, epochs)),
               grad0=np.zeros(params0.shape, dtype=T))
    for f in range(folds):
        own = fold_of != f
        cw, m_train = class_weights(y, own, dtype=T, plant=plant)
        mask = np.ones(m, dtype=bool) if plant == 'heldout_leaks' else own
        p = params0[f].astype(T)
        mom, var = np.zeros_like(p), np.zeros_like(p)
        for e in range(epochs):
            logit, z, r = forward_ref(p, stats[f], x, d, H, dtype=T)
            g, _, loss_sum = grad_ref(p, logit, z, r, y, mask, cw, d, H, dtype=T)
            out['loss'][f, e] = loss_sum / m_train + 0.5 * float(np.float32(l2)) * l2_sum_ref(p, d, H)
            if e == 0 and keep_first_grad:
                out['grad0'][f] = g
            s = sc[e - 1 if plant == 'stale_bias_correction' and e > 0 else e]
            p, mom, var = adam_ref(p, mom, var, g, m_train, l2, wmask, s[0], s[1], dtype=T)
        out['params'][f] = p
        held = np.flatnonzero(fold_of == f)
        out['scores'][held] = _sigmoid(forward_ref(p, stats[f], x[held], d, H, dtype=T)[0])
    return out


def score_ref(X, rows, fold_of, params, stats, H, dtype=np.float32):
    """ure_attack_score: p of every selected row under the set fold_of[i] (fold_of None: under set 0)."""
    x = np.asarray(X)[np.asarray(rows, dtype=np.int64)]
    fo = np.zeros(len(x), dtype=np.int64) if fold_of is None else np.asarray(fold_of, dtype=np.int64)
    out = np.zeros(len(x), dtype=dtype)
    for f in np.unique(fo):
        at = np.flatnonzero(fo == f)
        out[at] = _sigmoid(forward_ref(params[f], stats[f], x[at], x.shape[1], H, dtype=dtype)[0])
    return out


def _picked(scores, pos, neg):
    s = np.asarray(scores, dtype=np.float32)
    sp, sn = s[np.asarray(pos, dtype=np.int64)], s[np.asarray(neg, dtype=np.int64)]
    if len(sp) < 1 or len(sn) < 1:
        raise ValueError('both index lists need at least one entry')
    if np.isnan(sp).any() or np.isnan(sn).any():
        raise ValueError('a selected score is NaN: the pair counts are not defined')
    return sp, sn


def auc_counts_ref(scores, pos, neg, plant=None):
    """(gt, eq): the number of (positive, negative) pairs with s_p > s_n and with s_p == s_n, on float32 values (-0.0 == +0.0), by
    sort + searchsorted.  A NaN among the selected scores is refused."""
    sp, sn = _picked(scores, pos, neg)
    v = np.sort(sn + np.float32(0))              # -0.0 + 0.0 = +0.0: one zero in the order
    sp = sp + np.float32(0)
    lo, hi = np.searchsorted(v, sp, side='left'), np.searchsorted(v, sp, side='right')
    gt, eq = int(lo.astype(np.int64).sum()), int((hi - lo).astype(np.int64).sum())
    return (gt + eq, 0) if plant == 'ties_as_wins' else (gt, eq)


def confusion_ref(scores, pos, neg, thr=0.5):
    """(tp, fn, tn, fp): a score > thr (as a float32) predicts class 1."""
    sp, sn = _picked(scores, pos, neg)
    thr = np.float32(thr)
    tp, fp = int((sp > thr).sum()), int((sn > thr).sum())
    return tp, len(sp) - tp, len(sn) - fp, fp


def metrics(gt, eq, tp, fn, tn, fp):
    """dict(auc, bacc, f1) in Python floats; F1 is of class 1, 0.0 when it has no true positive."""
    n1, n2 = tp + fn, tn + fp
    auc = (gt + eq / 2.0) / (float(n1) * float(n2))
    bacc = 0.5 * (tp / float(n1) + tn / float(n2))
    f1 = 2.0 * tp / float(2 * tp + fp + fn) if tp > 0 else 0.0
    return dict(auc=auc, bacc=bacc, f1=f1)
