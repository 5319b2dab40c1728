"""Cases of the attribute-inference attacker shared by tests/test_cpu_attack.py and tests/test_gpu_attack.py (cases only: no
fixtures, nothing from the reference).  Two fixed synthetic tables in synth's style -- seeded numpy generators, float32 -- plus the
score lists of the pair-count tests.

  planted   the rows of class 1 are shifted by SHIFT along one random unit direction of a standard normal table;
  null      the same generator without the shift: the labels are independent of the rows.

What the float64 contract (attack.train_ref, SETTINGS below) gives on them, written down from a run and checked by
tests/test_cpu_attack.py::test_planted_is_clearly_above_null:

  planted   pooled AUC 0.9957, per fold 0.9974 / 0.9935 (spread, max - min: 0.0039)
  null      pooled AUC 0.5385, per fold 0.5520 / 0.5272 (spread 0.0248)

The gap, 0.4572, is 18 times the larger of the two spreads (the test asks for ten).  The sizes are what makes that possible: the
null table's per-fold AUC scatters around 0.5 with a standard deviation of sqrt((a + b + 1) / (12 a b)) = 0.026 at a = 225, b = 300
held-out rows, whatever the probe does; three folds of the same table would scatter too widely for a factor of ten.
"""
import numpy as np

N_ROWS, D = 1200, 8
N1, N2 = 450, 600
SHIFT = 4.0
SETTINGS = dict(hidden=8, folds=2, epochs=40, lr=1e-2, l2=1e-4, seed=5)
LOGISTIC = dict(hidden=0, folds=2, epochs=25, lr=3e-2, l2=1e-3, seed=9)


def table(planted, seed=2024):
    """(X float32 [N_ROWS, D], id1 int64 [N1], id2 int64 [N2]): the groups are unsorted picks of the rows."""
    rs = np.random.RandomState(seed)
    X = rs.randn(N_ROWS, D).astype(np.float32)
    ids = rs.permutation(N_ROWS)[:N1 + N2]
    id1, id2 = ids[:N1].astype(np.int64), ids[N1:].astype(np.int64)
    direction = rs.randn(D)
    direction /= np.linalg.norm(direction)
    if planted:
        X[id1] += (SHIFT * direction).astype(np.float32)
    return X, id1, id2


def fit_contract(X, id1, id2, settings, dtype, plant=None, **kw):
    """attack.train_ref under a case's settings -> (its dict, rows, n1, n2, fold_of, params0)."""
    from ultrare_amd import attack as A
    s = settings
    rows, n1, n2, H, folds, epochs, lr, l2 = A.check_attack_args(len(X), X.shape[1], id1, id2, s['hidden'], s['folds'], s['epochs'], s['lr'], s['l2'])
    fold_of = A.fold_plan(n1, n2, folds, s['seed'])
    p0 = A.init_params(X.shape[1], H, folds, s['seed'])
    return A.train_ref(X, rows, n1, fold_of, p0, H, epochs, lr, l2, dtype=dtype, plant=plant, **kw), rows, n1, n2, fold_of, p0


def aucs(scores, n1, n2, fold_of):
    """(pooled AUC, [per-fold AUC]) of out-of-fold scores by position, from attack.auc_counts_ref."""
    from ultrare_amd import attack as A
    pos, neg = np.arange(n1), np.arange(n1, n1 + n2)
    auc = lambda p, n: (lambda gt, eq: (gt + eq / 2.0) / (len(p) * len(n)))(*A.auc_counts_ref(scores, p, n))
    return auc(pos, neg), [auc(pos[fold_of[pos] == f], neg[fold_of[neg] == f]) for f in range(int(fold_of.max()) + 1)]


def score_cases():
    """{name: (scores float32, pos, neg)} of the pair-count tests: random, heavy ties, all equal, signed zeros, single entries."""
    rs = np.random.RandomState(7)
    out = {}
    s = rs.rand(300).astype(np.float32)
    idx = rs.permutation(300)
    out['random'] = (s, idx[:130], idx[130:])
    out['ties'] = ((np.floor(s * 4) / 4).astype(np.float32), idx[:130], idx[130:])
    out['all_equal'] = (np.full(300, 0.5, dtype=np.float32), idx[:7], idx[7:90])
    z = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, -0.0], dtype=np.float32)
    out['signed_zeros'] = (z, np.array([1, 2, 4]), np.array([0, 3, 5, 6]))
    out['one_positive'] = (s, idx[:1], idx[1:])
    out['one_negative'] = (s, idx[1:], idx[:1])
    return out


def double_loop(scores, pos, neg):
    """(gt, eq) by the literal double loop."""
    gt = eq = 0
    for i in pos:
        for j in neg:
            gt += bool(scores[i] > scores[j])
            eq += bool(scores[i] == scores[j])
    return gt, eq
