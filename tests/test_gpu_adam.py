"""engine.TrainJob(..., optimizer='adam') on the device: mf_adam_step_kernel against the numpy contract (ultrare_amd/adam.py) bit for
bit where the gradient is known exactly, against the float64 contract with torch's float32 run as the yardstick for whole steps,
its determinism, the Scratch / Sisa surface, and the wide configuration SGD with momentum diverges on."""
import copy
import os

import numpy as np
import pytest
import torch

import adam_cases as C
from ultrare_amd import adam

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


# ------------------------------------------------------------------ 1. the update's arithmetic, bit for bit
@pytest.mark.parametrize('d', [4, 8, 16, 32, 64, 128, 256])
def test_rows_without_interactions_are_the_contract_bit_for_bit(d):
    """9 users and 7 items have no rating: their gradient is exactly lam * w in every step, so after every epoch their w, m and v
    are the bytes of decay_rows_ref -- a difference is a wrong scalar, step index, buffer or rounding."""
    case = C.decay_case(d)
    job = case.job()
    want_u = adam.decay_rows_ref(case.U0[:case.no_u], case.lr_host, case.steps, C.LAM, C.BETAS, C.EPS)
    want_v = adam.decay_rows_ref(case.V0[:case.no_i], case.lr_host, case.steps, C.LAM, C.BETAS, C.EPS)
    for e in range(case.epochs):
        job.run_epochs(1)
        U, V = job.padded_tables(0)
        st = job.state[0]
        got_u = [x[:case.no_u].cpu().numpy() for x in (U, st['mU'], st['vU'])]
        got_v = [x[:case.no_i].cpu().numpy() for x in (V, st['mV'], st['vV'])]
        for name, got, want in zip('wmv' * 2, got_u + got_v, list(want_u[e]) + list(want_v[e])):
            assert got.tobytes() == want.tobytes(), (d, e, name, float(np.abs(got - want).max()))
    assert np.isfinite(job.tables(0)[0].cpu().numpy()).all()
    job.close()


# ------------------------------------------------------------------ 2. whole steps against float64, torch's float32 run the yardstick
@pytest.mark.parametrize('case', C.WHOLE_STEP_CASES, ids=repr)
def test_whole_training_is_as_close_to_float64_as_torch_float32(case):
    """E_k = max |kernel - float64 contract| and E_t = max |torch float32 CPU Adam - float64 contract| over the tables after the last
    step and the per-epoch train losses (relative); elements whose float64 |g| falls below 1e-3 at any step are left out of both
    (at most 1 % of a case: tests/test_cpu_adam.py).  Both are float32 executions of one recurrence that differ in the order of
    a row's gradient sum and in fused multiply-adds: E_k <= 4 * max(E_t, ulp32(max |w|)); a wrong bias correction or step count is 100
    to 1000 times the yardstick."""
    ref = C.reference(case)
    job = case.job()
    job.run()
    U, V = job.tables(0)
    E_k = C.distance(ref, U.cpu().numpy(), V.cpu().numpy(), job.epoch_sse(0))
    wmax = max(np.abs(ref['f64'][0]).max(), np.abs(ref['f64'][1]).max())
    bound = 4 * max(ref['E_t'], C.ulp32(wmax))
    print(f'{case!r}: E_k {E_k:.3g} E_t {ref["E_t"]:.3g} ulp32(max|w| = {wmax:.3g}) {C.ulp32(wmax):.3g} left out {ref["left_out"]:.4%}')
    job.close()
    assert ref['left_out'] <= C.LEAVE_OUT_CAP
    assert E_k <= bound, (E_k, ref['E_t'], bound)


# ------------------------------------------------------------------ 3. determinism
def _job_bytes(job, s):
    U, V = job.padded_tables(s)
    st = job.state[s]
    return [_bytes(x) for x in (U, V, st['mU'], st['mV'], st['vU'], st['vV'], st['sse'])]


def test_same_inputs_same_bytes_alone_or_beside_other_shards():
    cases = [C.Case(70, 50, 32, 2000, 512, 3, seed=2), C.Case(64, 40, 32, 1500, 512, 3, seed=21), C.Case(30, 90, 32, 2300, 512, 3, seed=22)]
    runs = []
    for group in ([cases[0]], [cases[0]], cases, [cases[2], cases[1], cases[0]]):
        job = C.make_job(group)
        job.run()
        runs.append({id(c): _job_bytes(job, s) for s, c in enumerate(group)})
        job.close()
    first = runs[0][id(cases[0])]
    assert runs[1][id(cases[0])] == first                      # two jobs on the same inputs
    assert runs[2][id(cases[0])] == first                      # beside two others: another grid mapping
    assert runs[3][id(cases[0])] == first
    assert runs[2][id(cases[1])] == runs[3][id(cases[1])] and runs[2][id(cases[2])] == runs[3][id(cases[2])]


# ------------------------------------------------------------------ 4. the surface
class Param:
    """The InsParam fields Scratch / Sisa read, with the Adam option."""

    def __init__(self, epochs, k=16, batch=3000, parallel=False, lr=0.01):
        self.k, self.lam, self.seed, self.batch = k, 0.1, 42, batch
        self.lr, self.lr_decay, self.momentum, self.epochs = lr, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, parallel
        self.optimizer, self.betas, self.eps = 'adam', (0.9, 0.999), 1e-8


def _loaders(S, del_user=()):
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, list(del_user), [], S, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], S, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    return idx, trd, ted, loadData(RatingData(np.hstack(te)), 3000, 24, False)


def test_scratch_train_with_adam_gives_the_tables_of_a_direct_job():
    from ultrare_amd import engine
    from ultrare_amd.method.scratch import Scratch, prepare_shard
    from ultrare_amd.method.utils import seed_all
    _, trd, ted, _ = _loaders(1)
    p = Param(2)
    sc = Scratch(p, 'mf')
    torch.manual_seed(42)
    model = sc.train(trd[0], ted[0], [], 0, '')
    torch.manual_seed(42)                                   # (the CPU generator feeds the inits and the epochs' seeds; seed_all leaves it alone)
    seed_all(p.seed)
    shard, init, perms = prepare_shard(trd[0], N_USER, N_ITEM, p.k, p.epochs, False)
    job = engine.TrainJob([shard], [init], [perms], p.k, 3000, p.epochs, p.lr, p.lam, p.momentum, p.lr_decay, optimizer='adam')
    assert (job.lazy_rows, job.touch_mode) == (False, 0)
    job.run()
    U, V = job.tables(0)
    assert _bytes(model.user_mat.weight) == _bytes(U.contiguous()) and _bytes(model.item_mat.weight) == _bytes(V.contiguous())
    loss = np.sqrt(job.epoch_sse(0) / shard.N)
    job.close()
    assert sc.log['train_loss'] == [float(x) for x in loss]
    for key in ('train_loss', 'test_rmse', 'test_ndcg', 'test_hr'):
        assert len(sc.log[key]) == p.epochs and np.isfinite(sc.log[key]).all(), key
    assert sc.log['train_loss'][1] < sc.log['train_loss'][0]


def test_sisa_with_adam_parallel_equals_sequential_and_unlearns_one_shard():
    from ultrare_amd.method.sisa import Sisa
    idx, trd, ted, tot = _loaders(3)
    res = []
    for par in (False, True):
        s = Sisa(Param(2, parallel=par), 'mf', 3, idx)
        torch.manual_seed(42)
        ml = s.learn(trd, ted, tot, 0, '')
        res.append(([_bytes(m.item_mat.weight) for m in ml], _bytes(ml[0].user_mat.weight), s.log0, ml, s.log))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert all(np.isfinite(v).all() for k, v in res[1][4].items() if k != 'time')
    # deleting users of shard 1 retrains that shard only
    del_user = [int(u) for u in idx[1][:5]]
    idx2, trd2, ted2, tot2 = _loaders(3, del_user)
    before = [_bytes(m.item_mat.weight) for m in res[1][3]]
    s2 = Sisa(Param(2, parallel=True), 'mf', 3, idx2)
    torch.manual_seed(42)
    ml2 = s2.unlearn([copy.deepcopy(m) for m in res[1][3]], trd2, ted2, tot2, del_user, 0, '')
    assert s2.retrained == [1]
    after = [_bytes(m.item_mat.weight) for m in ml2]
    assert after[0] == before[0] and after[2] == before[2] and after[1] != before[1]
    assert np.isfinite([s2.log0['total_rmse'], s2.log0['total_ndcg'], s2.log0['total_hr']]).all()
    assert all(np.isfinite(v).all() for k, v in s2.log.items() if k != 'time')


# ------------------------------------------------------------------ 5. the case that motivates it, in miniature
def test_wide_tables_train_where_sgd_diverges():
    """3,000 x 1,500, 300 k ratings with skewed items, B = 30,000, d = 128, N(0, 1) tables, lr 1e-2: the summed loss drives
    SGD with momentum to NaN in its first epoch; Adam's bounded step stays finite and its train loss falls in every epoch."""
    from ultrare_amd import engine
    rs = np.random.RandomState(7)
    n_user, n_item, N, d, B, E = 3000, 1500, 300000, 128, 30000, 6
    uid = rs.randint(0, n_user, N).astype(np.int32)
    iid = np.floor(rs.random_sample(N) ** 3 * n_item).astype(np.int32)
    r = (rs.randint(1, 6, N) / 5).astype(np.float32)
    U0, V0 = rs.standard_normal((n_user, d)).astype(np.float32), rs.standard_normal((n_item, d)).astype(np.float32)
    orders = np.stack([rs.permutation(N) for _ in range(E)]).astype(np.int32)
    job = engine.TrainJob([engine.ShardData(uid, iid, r, n_user, n_item)], [(U0, V0)], [orders], d, B, E, 1e-2, 0.1, 0.9, 0.95, optimizer='adam')
    job.run()
    U, V = job.tables(0)
    assert bool(torch.isfinite(U).all()) and bool(torch.isfinite(V).all())
    loss = np.sqrt(job.epoch_sse(0) / N)
    job.close()
    print('train RMSE per epoch:', [round(float(x), 4) for x in loss])
    assert np.isfinite(loss).all() and (np.diff(loss) < 0).all(), loss
