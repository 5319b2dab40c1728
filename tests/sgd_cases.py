"""Shared case builders of tests/test_cpu_sgd.py and tests/test_gpu_sgd.py (no pytest plugin: a plain module beside them).

The SGD step of a training job (momentum, weight decay, StepLR) off the default schedule.  A case is one shard with made-up ratings
(in the pattern of adam_cases.Case: a hot item, users and items without a rating), a schedule is (lam, mu, lr_decay, lr_step).  reference(case, schedule)
holds what both files compare against, computed once per process: sgd_train_ref in float64 -- the contract -- and E_y, the distance
from it of two float32 executions of the same recurrence (the C oracle and sgd_train_ref in float32)."""
import functools

import numpy as np

import adam_cases
from adam_cases import ulp32                       # noqa: F401  (the one definition both optimizers' tests use)

LR = 1e-3
DEFAULT = (0.1, 0.9, 0.95, 50)                     # what every other training test of the suite runs: lr is a constant below 51 epochs
NO_DECAY = (0.0, 0.9, 0.5, 1)
NO_MOMENTUM = (0.1, 0.0, 0.5, 1)
PLAIN = (0.0, 0.0, 1.0, 1)
MIXED = (0.03, 0.5, 0.7, 2)
LARGE = (1.0, 0.99, 0.5, 1)                        # (drives the long d = 64 case to NaN in float64: short cases only)
PLANTS = ('mu_fixed', 'stale_lr', 'skip_first')


class Case:
    """One shard in the pattern of adam_cases.Case, without a schedule of its own: n_user x n_item (default 60 x 300), seeded, N ratings over
    the users [5, n_user) and the items [40, n_item) (the first 5 users and 40 items have none), a quarter of them on the last item,
    duplicates of a pair allowed, N(0, 1) start tables, lr 1e-3.  With 300 items and 6 or 70 steps per epoch most items miss most steps:
    in a touch route nearly every update is followed by a closed-form advance, many of them across an epoch boundary.
    The schedule comes with every call: lr_of(schedule), job(schedule)."""

    def __init__(self, kind, d, N, B, epochs, seed, schedules, n_user=60, n_item=300, no_u=5, no_i=40, hot=0.25):
        rs = np.random.RandomState(1000 + seed)
        self.kind, self.schedules = kind, tuple(schedules)
        self.n_user, self.n_item, self.d, self.N, self.B, self.epochs = n_user, n_item, d, N, B, epochs
        self.uid = rs.randint(no_u, n_user, N).astype(np.int32)
        self.iid = rs.randint(no_i, n_item - 1, N).astype(np.int32)
        self.iid[rs.permutation(N)[:int(N * hot)]] = n_item - 1
        self.rating = (rs.randint(1, 6, N) / 5).astype(np.float32)
        self.U0 = rs.standard_normal((n_user, d)).astype(np.float32)
        self.V0 = rs.standard_normal((n_item, d)).astype(np.float32)
        self.orders = np.stack([rs.permutation(N) for _ in range(epochs)]).astype(np.int32)
        self.steps = (N + B - 1) // B
        self.no_u, self.no_i = no_u, no_i

    def __repr__(self):
        return f'{self.kind}-k{self.d}'

    def lr_of(self, schedule):
        """StepLR as engine.TrainJob makes it: float32 values."""
        _, _, lr_decay, lr_step = schedule
        return np.array([LR * (lr_decay ** (t // lr_step)) for t in range(self.epochs)], dtype=np.float32)

    def job(self, schedule, **kw):
        return make_job([self], schedule, **kw)


def make_job(cases, schedule, **kw):
    """The cases as the shards of one SGD job on the current device (one batch size and one epoch count per job: the first case's)."""
    from ultrare_amd import engine
    c0 = cases[0]
    assert all((c.d, c.B, c.epochs) == (c0.d, c0.B, c0.epochs) for c in cases)
    lam, mu, lr_decay, lr_step = schedule
    shards = [engine.ShardData(c.uid, c.iid, c.rating, c.n_user, c.n_item) for c in cases]
    return engine.TrainJob(shards, [(c.U0, c.V0) for c in cases], [c.orders for c in cases], c0.d, c0.B, c0.epochs, LR, lam, mu, lr_decay, lr_step, **kw)


_ALL = (DEFAULT, NO_DECAY, NO_MOMENTUM, PLAIN, MIXED)
# 6 steps per epoch, the last one partial (1500 = 5 * 256 + 220); k = 20 is padded to 32 columns on the device
SHORT = [Case('short', d, 1500, 256, 4, seed=d, schedules=_ALL + (LARGE,)) for d in (8, 20, 32, 128)]
# 70 steps per epoch: more than one 64-step window
LONG = [Case('long', d, 1400, 20, 3, seed=100 + d, schedules=_ALL) for d in (16, 64)]
# two shards of one job (one batch size, one epoch count) whose epochs differ in length: 38 steps (the last one partial) and 35,
# so their epochs end on different ticks
PAIR = [Case('pair38', 32, 1500, 40, 3, seed=201, schedules=(MIXED,)), Case('pair35', 32, 1400, 40, 3, seed=202, schedules=(MIXED,))]
# a short and a long-shaped shard side by side: 6 and 70 steps per epoch at the long case's batch size -- the short one has finished all
# its epochs before the long one ends its first, and the long one's epochs cross a 64-step window
UNEQUAL = [Case('pair6', 32, 120, 20, 3, seed=203, schedules=(MIXED,)), Case('pair70', 32, 1400, 20, 3, seed=204, schedules=(MIXED,))]
SHORT32 = SHORT[2]
LONG16 = LONG[0]
PAIRS = [(c, s) for c in SHORT + LONG + PAIR + UNEQUAL for s in c.schedules]          # every (case, schedule) a GPU test uses


def sid(schedule):
    return '/'.join(f'{x:g}' for x in schedule)


def ids(params):
    """pytest ids of a list of (case, schedule[, route]) parameters."""
    return ['-'.join([repr(p[0]), sid(p[1])] + list(p[2:])) for p in params]


def sgd_train_ref(uid, iid, rating, U0, V0, orders, batch, lr_host, lam, mu, dtype=np.float64, plant=None):
    """torch.optim.SGD(momentum=mu, weight_decay=lam) under MSELoss(sum) on dense tables, in plain numpy: per step
    err = sum(U[u] * V[i]) - r, the summed-loss gradients 2 err V[i] and 2 err U[u] scattered with np.add.at, g += lam w for every row of
    both tables, m = g on the very first step, else m = mu m + g, and w -= lr m.  lam and mu are taken at their float32 values, lr_host
    as float32 values.  -> (U [epochs, n_user, d], V [epochs, n_item, d]: the tables after every epoch, loss [epochs]:
    sqrt(sum of the epoch's batch losses / N)).  dtype=np.float32 runs the same lines in float32.
    plant (tests only): one of PLANTS -- mu fixed at 0.9 whatever is asked for; the previous epoch's lr in an epoch's first step; rows
    that are not in an epoch's first batch skipping that step."""
    assert plant is None or plant in PLANTS
    T = dtype
    lam, mu = T(np.float32(lam)), T(np.float32(0.9 if plant == 'mu_fixed' else mu))
    lr_host = np.asarray(lr_host, dtype=np.float32)
    W = [np.array(U0, dtype=T), np.array(V0, dtype=T)]
    M = [np.zeros_like(W[0]), np.zeros_like(W[1])]
    ids, r = (uid.astype(np.int64), iid.astype(np.int64)), rating.astype(T)
    N, E = len(uid), len(orders)
    steps = (N + batch - 1) // batch
    out, loss, first = ([], []), np.zeros(E), True
    for e in range(E):
        for s in range(steps):
            lr = T(lr_host[e - 1 if plant == 'stale_lr' and s == 0 and e > 0 else e])
            idx = orders[e][s * batch:(s + 1) * batch]
            b = (ids[0][idx], ids[1][idx])
            rows = (W[0][b[0]], W[1][b[1]])
            err = (rows[0] * rows[1]).sum(axis=1, dtype=T) - r[idx]
            loss[e] += float((err * err).sum(dtype=T))
            ge = (T(2) * err)[:, None]
            for t in (0, 1):
                g = np.zeros_like(W[t])
                np.add.at(g, b[t], ge * rows[1 - t])
                g += lam * W[t]
                m = g if first else mu * M[t] + g
                w = W[t] - lr * m
                if plant == 'skip_first' and s == 0:
                    skip = np.ones(len(w), dtype=bool)
                    skip[b[t]] = False
                    m[skip], w[skip] = M[t][skip], W[t][skip]
                M[t], W[t] = m, w
            first = False
        for t in (0, 1):
            out[t].append(W[t].copy())
    return np.stack(out[0]), np.stack(out[1]), np.sqrt(loss / N)


def ref_run(case, schedule, dtype=np.float64, plant=None):
    lam, mu = schedule[:2]
    return sgd_train_ref(case.uid, case.iid, case.rating, case.U0, case.V0, case.orders, case.B, case.lr_of(schedule), lam, mu, dtype=dtype, plant=plant)


def oracle_run(case, schedule):
    """oracle.cpu_ref.train_epoch (the C oracle's float32 dense optimizer) under the schedule: -> (U [epochs, ...], V [epochs, ...]: the
    tables after every epoch, loss [epochs])."""
    from oracle import cpu_ref as O
    lam, mu = schedule[:2]
    st = O.MFState(case.U0.copy(), case.V0.copy())
    U, V, loss = [], [], []
    for e, lr in enumerate(case.lr_of(schedule)):
        loss.append(O.train_epoch(st, (case.uid, case.iid, case.rating), np.ascontiguousarray(case.orders[e]), case.B, float(lr), lam, mu)[0])
        U.append(st.U.copy())
        V.append(st.V.copy())
    return np.stack(U), np.stack(V), np.array(loss)


@functools.lru_cache(maxsize=None)
def reference(case, schedule):
    """-> dict: 'f64' (U [epochs, ...], V [epochs, ...], loss [epochs]) of the float64 run, 'wmax' its largest |w| over all epochs,
    'oracle' and 'f32' the two float32 executions in the same layout, 'E_y_oracle' and 'E_y_f32' [epochs] their distances from the float64
    run after every epoch (tables of that epoch, losses up to it), 'E_y_epoch' the larger of the two (two independent executions, so
    that one lucky run cannot set the scale), 'bound_epoch' = 4 * max(E_y_epoch, ulp32(wmax)): the factor Adam's tests use; 'E_y' and
    'bound' are those of the last epoch, what whole training is held to."""
    ref = dict(f64=ref_run(case, schedule))
    with np.errstate(all='ignore'):
        ref['wmax'] = float(max(np.abs(ref['f64'][0]).max(), np.abs(ref['f64'][1]).max()))
        ref['oracle'] = oracle_run(case, schedule)
        ref['f32'] = ref_run(case, schedule, dtype=np.float32)
        for name in ('oracle', 'f32'):
            U, V, loss = ref[name]
            ref['E_y_' + name] = [distance(ref, U[e], V[e], loss[:e + 1], epoch=e) for e in range(case.epochs)]
        ref['E_y_epoch'] = [max(a, b) for a, b in zip(ref['E_y_oracle'], ref['E_y_f32'])]
        ref['bound_epoch'] = [4 * max(E_y, ulp32(ref['wmax'])) for E_y in ref['E_y_epoch']]
        ref['E_y'], ref['bound'] = ref['E_y_epoch'][-1], ref['bound_epoch'][-1]
    return ref


def distance(ref, U, V, loss, epoch=-1):
    """adam_cases.distance with nothing left out (SGD is linear in g): the maximum absolute difference over both tables from the float64
    tables after `epoch`, and the maximum relative difference over the epoch losses given (the first len(loss) epochs)."""
    U64, V64, loss64 = ref['f64']
    loss = np.atleast_1d(np.asarray(loss, dtype=np.float64))
    return adam_cases.distance(dict(f64=(U64[epoch], V64[epoch], loss64[:len(loss)]), keep=(Ellipsis, Ellipsis)), np.asarray(U), np.asarray(V), loss)
