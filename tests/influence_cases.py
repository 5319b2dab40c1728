"""The cases of the Newton-step (influence) unlearning tests (test_cpu_influence.py, test_gpu_influence.py): the smallest shapes at
which each piece can still go wrong, built once and left unchanged."""
import functools
import types

import numpy as np

from ultrare_amd import influence
from ultrare_amd.lightgcn import WIDTHS, Graph  # noqa: F401


def _case(uid, iid, rating, U, V, l2, **kw):
    g = Graph(uid, iid, len(U), len(V))
    c = types.SimpleNamespace(uid=np.asarray(uid, dtype=np.int64), iid=np.asarray(iid, dtype=np.int64), rating=np.asarray(rating, dtype=np.float32),
                              U=np.asarray(U, dtype=np.float32), V=np.asarray(V, dtype=np.float32), l2=float(l2), g=g, n_user=len(U), n_item=len(V),
                              d=U.shape[1], **kw)
    c.r = c.rating[g.pos]                                # the ratings in CSR order
    return c


@functools.lru_cache(maxsize=None)
def case_a():
    """7 users x 5 items, d = 4, 40 triples: user 3 and item 2 have none, (0, 0) is listed three times on purpose, user 5 and item 4
    are frozen by the scope."""
    rng = np.random.default_rng(20250101)
    users, items = np.array([0, 1, 2, 4, 5, 6]), np.array([0, 1, 3, 4])
    uid = np.concatenate([[0, 0, 0], users, rng.choice(users, 40 - 3 - len(users))])
    iid = np.concatenate([[0, 0, 0], items, items[:2], rng.choice(items, 40 - 3 - len(users))])
    rating = rng.uniform(0.2, 1.0, 40).astype(np.float32)
    U, V = rng.normal(0, 0.5, (7, 4)).astype(np.float32), rng.normal(0, 0.5, (5, 4)).astype(np.float32)
    scope = (np.array([0, 1, 2, 3, 4, 6]), np.array([0, 1, 2, 3]))
    c = _case(uid, iid, rating, U, V, 0.3, scope=scope)
    assert len(uid) == 40 and np.diff(c.g.off_u)[3] == 0 and np.diff(c.g.off_i)[2] == 0
    c.active = influence.active_rows(c.g, scope)[:2]
    assert not c.active[0][5] and not c.active[1][4] and not c.active[0][3] and not c.active[1][2]
    return c


LONG_ROW = 130


@functools.lru_cache(maxsize=None)
def case_b(d):
    """3 users x 130 items at width d: user 1 holds all 130 items (longer than one tile of the widest lane group, 64, with a tail of
    2), user 0 three of them, user 2 seven."""
    rng = np.random.default_rng(7 + d)
    uid = np.concatenate([np.full(LONG_ROW, 1), np.full(3, 0), np.full(7, 2)])
    iid = np.concatenate([rng.permutation(LONG_ROW), rng.choice(LONG_ROW, 3, replace=False), rng.choice(LONG_ROW, 7, replace=False)])
    order = rng.permutation(len(uid))
    uid, iid = uid[order], iid[order]
    rating = rng.uniform(0.2, 1.0, len(uid)).astype(np.float32)
    U, V = rng.normal(0, 0.3, (3, d)).astype(np.float32), rng.normal(0, 0.3, (LONG_ROW, d)).astype(np.float32)
    c = _case(uid, iid, rating, U, V, 0.2, scope='all')
    c.active = influence.active_rows(c.g)[:2]
    return c


def direction(c, seed=1):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, c.U.shape), rng.normal(0, 1, c.V.shape)


# ---------------------------------------------------------------------------------------------------------------- case C
def als_sweep(uid, iid, r, U, V, l2):
    """One exact float64 ALS sweep on F = sum e^2 + l2 (|U|^2 + |V|^2): every user row against V, then every item row against the new
    U; a row without ratings becomes zero."""
    d = U.shape[1]

    def half(rows, cols, X, n):
        A = np.zeros((n, d, d))
        b = np.zeros((n, d))
        np.add.at(A, rows, X[cols][:, :, None] * X[cols][:, None, :])
        np.add.at(b, rows, r[:, None] * X[cols])
        out = np.linalg.solve(A + l2 * np.eye(d), b[:, :, None])[:, :, 0]
        out[np.bincount(rows, minlength=n) == 0] = 0.0
        return out
    U = half(uid, iid, V, len(U))
    V = half(iid, uid, U, len(V))
    return U, V


def objective64(uid, iid, r, U, V, l2):
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    e = (U[uid] * V[iid]).sum(axis=1) - r
    return float((e * e).sum() + l2 * ((U * U).sum() + (V * V).sum()))


@functools.lru_cache(maxsize=None)
def case_c():
    """The prototype's recipe at 60 x 40 x 8 with 900 triples and l2 = 0.3: ratings a rank-8 product plus N(0, 0.1) noise scaled to
    [0.2, 1] and rounded to float32; the start is 300 ALS sweeps on all triples (rounded to float32, as a model's tables are); users
    0, 1 and 2 are deleted; the yardstick is 600 further float64 ALS sweeps on the remaining triples from that start."""
    n_user, n_item, d, N, l2 = 60, 40, 8, 900, 0.3
    rng = np.random.default_rng(20250102)
    A, B = rng.normal(0, 1, (n_user, d)), rng.normal(0, 1, (n_item, d))
    uid, iid = rng.integers(0, n_user, N), rng.integers(0, n_item, N)
    raw = (A[uid] * B[iid]).sum(axis=1) + rng.normal(0, 0.1, N)
    rating = (0.2 + 0.8 * (raw - raw.min()) / (raw.max() - raw.min())).astype(np.float32)
    r64 = rating.astype(np.float64)
    U, V = rng.normal(0, 0.1, (n_user, d)), rng.normal(0, 0.1, (n_item, d))
    for _ in range(300):
        U, V = als_sweep(uid, iid, r64, U, V, l2)
    U0, V0 = U.astype(np.float32), V.astype(np.float32)
    deleted = np.array([0, 1, 2])
    keep = ~np.isin(uid, deleted)
    Y, Z = U0.astype(np.float64), V0.astype(np.float64)
    for _ in range(600):
        Y, Z = als_sweep(uid[keep], iid[keep], r64[keep], Y, Z, l2)
    c = _case(uid[keep], iid[keep], rating[keep], U0, V0, l2, scope='all', deleted=deleted)
    c.F_yard = objective64(c.uid, c.iid, r64[keep], Y, Z, l2)
    Uz, Vz = U0.copy(), V0.copy()
    _, _, eu, ei = influence.active_rows(c.g)
    Uz[eu], Vz[ei] = 0.0, 0.0
    c.F_zeroed = objective64(c.uid, c.iid, r64[keep], Uz, Vz, l2)
    c.objective = lambda U, V: objective64(c.uid, c.iid, r64[keep], U, V, l2)
    return c


@functools.lru_cache(maxsize=None)
def case_c_steps(steps):
    """newton_unlearn_ref with the defaults on case C, computed once per number of steps."""
    c = case_c()
    return influence.newton_unlearn_ref(c.uid, c.iid, c.rating, c.U, c.V, c.l2, steps=steps)
