"""SGD training on the device off its default schedule, every execution route of the step kernel against the float64 restatement of
tests/sgd_cases.py (why: tests/test_cpu_sgd.py).  The yardstick is E_y, the distance from float64 of two float32 executions of the same
recurrence on the CPU; a route passes with E_k <= 4 * max(E_y, ulp32(max |w|)), the factor Adam's tests use.  Whole training, epoch by
epoch with reads in between, the end-of-epoch snapshots, two shards of different length in one job, and the Scratch surface."""
import os

import numpy as np
import pytest
import torch

import sgd_cases as C

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071

# route -> (TrainJob arguments, URE_TOUCH_INDEX, the (touch_mode, lazy_rows) the job must report: a plan change cannot quietly move a
# test to another kernel)
ROUTES = {
    'dense': (dict(touch=False, lazy_rows=False), None, (0, False)),         # the default kernel, decay rows streamed
    'lazy': (dict(touch=False, lazy_rows=True), None, (0, True)),            # the default kernel, decay rows in closed form
    'touch': (dict(touch=True), None, (1, True)),                            # touch mode 1, one window
    'ahead': (dict(touch=True, final_only=True), None, (2, True)),           # touch mode 2: no reads before the end
    'index': (dict(touch='index'), None, (3, True)),                         # touch mode 3
    'windows': (dict(touch=True), '0', (1, True)),                           # touch mode 1 in 64-step windows (epochs of 70 steps)
}
SHORT_ROUTES, LONG_ROUTES = ('dense', 'lazy', 'touch', 'ahead', 'index'), ('lazy', 'index', 'windows')
TWO = (C.MIXED, C.NO_MOMENTUM)


def _job(cases, schedule, route, monkeypatch, **kw):
    args, use_index, plan = ROUTES[route]
    for name in ('URE_TOUCH', 'URE_TOUCH_AHEAD', 'URE_TOUCH_INDEX'):
        monkeypatch.delenv(name, raising=False)
    if use_index is not None:
        monkeypatch.setenv('URE_TOUCH_INDEX', use_index)
    job = C.make_job(cases, schedule, **args, **kw)
    assert (job.touch_mode, job.lazy_rows) == plan, (route, job.touch_mode, job.lazy_rows)
    return job


def _np(t):
    return t.detach().cpu().numpy()


def _loss(job, s, case, n=None):
    return np.sqrt(job.epoch_sse(s)[:n] / case.N)


def _check(tag, ref, E_k, epoch=-1):
    """Print the figures, then hold E_k to the bound of the epoch the tables were read after."""
    E_y, bound = ref['E_y_epoch'][epoch], ref['bound_epoch'][epoch]
    print(f'{tag}: E_k {E_k:.3g} E_y {E_y:.3g} ulp32(max|w| = {ref["wmax"]:.3g}) {C.ulp32(ref["wmax"]):.3g} ratio {4 * E_k / bound:.3g}')
    assert E_k <= bound, (tag, E_k, E_y, bound)


# ------------------------------------------------------------------ 1. whole training against float64
WHOLE = [(c, s, r) for cases, routes in ((C.SHORT, SHORT_ROUTES), (C.LONG, LONG_ROUTES)) for c in cases for s in c.schedules for r in routes]


@pytest.mark.parametrize('case,schedule,route', WHOLE, ids=C.ids(WHOLE))
def test_whole_training_is_as_close_to_float64_as_a_float32_run(case, schedule, route, monkeypatch):
    """E_k = the distance of the job's final tables and per-epoch train losses from the float64 run (maximum absolute difference over
    both tables, maximum relative difference over the losses; nothing left out), E_y the same distance of the C oracle and of the
    float32 numpy run, whichever is larger: E_k <= 4 * max(E_y, ulp32(max |w|)).  A momentum, weight decay or per-epoch learning rate
    that is wrong in any closed-form table, kernel argument or scalar stands 100 times and more above that bound under one of the
    schedules (tests/test_cpu_sgd.py)."""
    ref = C.reference(case, schedule)
    job = _job([case], schedule, route, monkeypatch)
    job.run()
    U, V = job.tables(0)
    E_k = C.distance(ref, _np(U), _np(V), _loss(job, 0, case))
    job.close()
    _check(f'{route} {case!r} {C.sid(schedule)}', ref, E_k)


# ------------------------------------------------------------------ 2. epoch by epoch: materialize, read, resume under a changing lr
BY_EPOCH = [(c, s, r) for c, routes in ((C.SHORT32, ('dense', 'lazy', 'touch', 'index')), (C.LONG16, LONG_ROUTES)) for s in TWO for r in routes]


@pytest.mark.parametrize('case,schedule,route', BY_EPOCH, ids=C.ids(BY_EPOCH))
def test_tables_read_after_every_epoch_follow_float64(case, schedule, route, monkeypatch):
    """The tables are read at every epoch end and held to the float64 tables of that epoch under the same bound, with E_y the float32
    runs' distance after that epoch (smaller in the early epochs); training goes on from the read (rows that only decay are brought up
    to date, then carried on at the next epoch's learning rate)."""
    ref = C.reference(case, schedule)
    job = _job([case], schedule, route, monkeypatch)
    for e in range(case.epochs):
        job.run_epochs(1)
        U, V = job.tables(0)
        E_k = C.distance(ref, _np(U), _np(V), _loss(job, 0, case, e + 1), epoch=e)
        _check(f'{route} {case!r} {C.sid(schedule)} epoch {e}', ref, E_k, e)
    job.close()


# ------------------------------------------------------------------ 3. snapshots
def _tables_by_epoch(case, schedule, route, monkeypatch, **kw):
    job = _job([case], schedule, route, monkeypatch, **kw)
    out = []
    for e in range(case.epochs):
        job.run_epochs(1)
        out.append(tuple(t.clone() for t in job.padded_tables(0)))
    job.close()
    return out


SNAP = [(c, s, r) for c, routes in ((C.SHORT32, ('lazy', 'touch', 'index')), (C.LONG16, LONG_ROUTES)) for s in TWO for r in routes]


@pytest.mark.parametrize('mode', [True, 'compact'], ids=['full', 'compact'])
@pytest.mark.parametrize('case,schedule,route', SNAP, ids=C.ids(SNAP))
def test_snapshots_are_the_tables_read_at_the_epoch_ends(case, schedule, route, mode, monkeypatch):
    """A job that runs through and keeps end-of-epoch snapshots against the same job read epoch by epoch: the same bytes, under
    schedules whose learning rate changes at (nearly) every epoch.  In full snapshots the rows without a rating are
    float32(snap_a[e]) * w0 bit for bit."""
    want = _tables_by_epoch(case, schedule, route, monkeypatch, snapshots=mode)
    job = _job([case], schedule, route, monkeypatch, snapshots=mode)
    job.run()
    st, sh = job.state[0], job.shards[0]
    if mode == 'compact':
        assert job.snapshots == 'compact'
        rows = torch.as_tensor(sh._sched_host[:sh.n_active, 0].astype(np.int64)).to(st['snap'].device)
        for e in range(case.epochs):
            assert torch.equal(st['snap'][e], torch.cat(want[e])[rows]), e
    else:
        assert job.snapshots == 'full'
        snapU, snapV = job.snapshots_of(0)
        a = _np(st['snap_a'])
        assert a.dtype == np.float32 and a.shape == (case.epochs,)
        for e in range(case.epochs):
            assert torch.equal(snapU[e], want[e][0]) and torch.equal(snapV[e], want[e][1]), e
            for snap, w0, n in ((snapU, case.U0, case.no_u), (snapV, case.V0, case.no_i)):
                assert _np(snap[e][:n, :case.d]).tobytes() == (a[e] * w0[:n]).tobytes(), e
    job.close()


# ------------------------------------------------------------------ 4. two shards of different length in one job
TWO_SHARDS = [(C.PAIR, r) for r in ('lazy', 'touch', 'index')] + [(C.UNEQUAL, r) for r in ('lazy', 'index', 'windows')]


@pytest.mark.parametrize('pair,route', TWO_SHARDS, ids=[f'{"+".join(map(repr, p))}-{r}' for p, r in TWO_SHARDS])
def test_two_shards_of_different_length_train_as_they_do_alone(pair, route, monkeypatch):
    """A job has one batch size and one epoch count, so its shards differ in steps per epoch.  38 beside 35 steps (B = 40): the epochs
    end on different ticks, one window each.  6 beside 70 steps (B = 20: a short and a long-shaped shard): the short one has finished
    all its epochs before the long one ends its first, and the long one's epochs cross a 64-step window (touch=True takes mode 3 there,
    so mode 1 is asked for as on the long cases: the windows route).  The learning rate changes at an epoch end of each.  Each shard
    against its own float64 run, and its bytes those of the same shard trained alone."""
    both = _job(pair, C.MIXED, route, monkeypatch)
    assert [both.steps_per_epoch(s) for s in range(2)] == [c.steps for c in pair] and pair[0].steps != pair[1].steps
    both.run()
    for s, case in enumerate(pair):
        ref = C.reference(case, C.MIXED)
        U, V = (t.clone() for t in both.tables(s))
        sse = both.epoch_sse(s)
        _check(f'{route} {case!r} beside the other', ref, C.distance(ref, _np(U), _np(V), _loss(both, s, case)))
        alone = _job([case], C.MIXED, route, monkeypatch)
        alone.run()
        U1, V1 = alone.tables(0)
        assert torch.equal(U, U1) and torch.equal(V, V1) and np.array_equal(sse, alone.epoch_sse(0)), s
        alone.close()
    both.close()


# ------------------------------------------------------------------ 5. the surface forwards what it is given
class Param:
    """The InsParam fields Scratch reads."""

    def __init__(self, epochs, lam, momentum, lr_decay):
        self.k, self.lam, self.seed, self.batch = 16, lam, 42, 3000
        self.lr, self.lr_decay, self.momentum, self.epochs = 1e-3, lr_decay, momentum, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, False


def test_scratch_train_forwards_lam_momentum_and_lr_decay(monkeypatch):
    """Scratch.train with lam = 0.03, momentum = 0.5, lr_decay = 0.7 gives the bytes of a direct job built with those values.  Scratch
    decays the learning rate every 50 epochs, so the run has 52: the last two epochs train at 0.7 * lr, and a direct job that differs in
    lr_decay alone (0.95) gives other bytes, as does one built with the defaults."""
    from ultrare_amd import engine
    from ultrare_amd.method.scratch import Scratch, prepare_shard
    from ultrare_amd.method.utils import seed_all
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, [], [], 1, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], 1, idx)
    trd, ted = loadData(RatingData(tr[0]), 3000, 24), loadData(RatingData(te[0]), 3000, 24, False)
    p = Param(52, 0.03, 0.5, 0.7)
    sc = Scratch(p, 'mf')
    torch.manual_seed(42)
    model = sc.train(trd, ted, [], 0, '')
    got = (model.user_mat.weight.detach().cpu().numpy().tobytes(), model.item_mat.weight.detach().cpu().numpy().tobytes())
    direct = []
    for lam, mu, lr_decay in ((p.lam, p.momentum, p.lr_decay), (p.lam, p.momentum, 0.95), (0.1, 0.9, 0.95)):
        torch.manual_seed(42)                               # (the CPU generator feeds the inits and the epochs' seeds; seed_all leaves it alone)
        seed_all(p.seed)
        shard, init, perms = prepare_shard(trd, N_USER, N_ITEM, p.k, p.epochs, False)
        job = engine.TrainJob([shard], [init], [perms], p.k, 3000, p.epochs, p.lr, lam, mu, lr_decay)
        job.run()
        U, V = job.tables(0)
        direct.append((_np(U.contiguous()).tobytes(), _np(V.contiguous()).tobytes()))
        loss = np.sqrt(job.epoch_sse(0) / shard.N)
        job.close()
        if len(direct) == 1:
            assert sc.log['train_loss'] == [float(x) for x in loss]
    assert got == direct[0]
    for other in direct[1:]:
        assert got[0] != other[0] and got[1] != other[1]
