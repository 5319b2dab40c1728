"""Batched ridge solves, host side (-m "not gpu"): ure_ridge_rows rejects every bad argument before any HIP call and its
scratch query follows its formula; the numpy restatement of the contract (ridge.ridge_rows_ref), which the GPU tests hold the
kernel to, is checked against independent math; trainer_l2 against its formula and a simulation of the trainer's update;
the CSR builder of engine.SegmentSet; fold_in / Sisa.fold_in / Sisa.forget_folded refuse bad settings before device work;
Sisa.learn / unlearn keep self.folded right (the training body monkeypatched).  Nothing here initialises HIP."""
import ctypes
import types

import numpy as np
import pytest


@pytest.fixture(scope='session')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ---- 1. the C calls -------------------------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(0x1000)                         # never dereferenced: every check fails before the device is touched


def _ridge(nv, n_fixed=10, d=16, k=16, m=5, l2=0.5, l2_n=0.0, scratch_bytes=0, F=True, off=True, idx=True, val=True, order=False, X=True,
           status=True):
    f = lambda on: FAKE if on else None
    return nv.lib().ure_ridge_rows(f(F), n_fixed, d, k, f(off), f(idx), f(val), m, f(order), l2, l2_n, f(X), f(status), None, scratch_bytes, None)


@pytest.mark.parametrize('kw,word', [({'F': False}, 'F && off'), ({'off': False}, 'F && off'), ({'idx': False}, 'F && off'), ({'val': False}, 'F && off'),
                                     ({'X': False}, 'F && off'), ({'status': False}, 'F && off'), ({'n_fixed': 0}, 'n_fixed >= 1'),
                                     ({'k': 0}, 'k >= 1'), ({'k': -3}, 'k >= 1'), ({'k': 17}, 'k <= d'), ({'d': 24, 'k': 8}, 'pow2(d)'),
                                     ({'d': 2, 'k': 2}, 'd >= 4'), ({'d': 256, 'k': 200}, 'd <= kRrMaxD'), ({'d': 256, 'k': 16}, 'd <= kRrMaxD'),
                                     ({'d': 0, 'k': 1}, 'k <= d'), ({'m': -1}, 'm >= 0'), ({'m': 1 << 31}, 'm <= INT32_MAX'),
                                     ({'l2': -1e-9}, 'l2 >= 0.0'), ({'l2': float('nan')}, 'l2 >= 0.0'), ({'l2': float('inf')}, 'l2 <= DBL_MAX'),
                                     ({'l2_n': -1.0}, 'l2_n >= 0.0'), ({'l2_n': float('nan')}, 'l2_n >= 0.0'), ({'l2_n': float('inf')}, 'l2_n <= DBL_MAX'),
                                     ({'scratch_bytes': -1}, 'scratch_bytes >= need')])
def test_ridge_rows_rejects_bad_arguments(nv, kw, word):
    assert _ridge(nv, **kw) == -1
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


def test_scratch_follows_its_formula_and_the_abi_is_15(nv):
    L = nv.lib()
    assert L.ure_abi_version() == 15 == nv.ABI_VERSION
    for m in (0, 1, 6040, 162000, (1 << 31) - 1):
        for k in (1, 5, 16, 32, 100, 128):
            assert L.ure_ridge_rows_scratch(m, k) == 0, (m, k)           # G never leaves the chip
    for m, k in [(-1, 16), (10, 0), (10, -2), (10, 129), (10, 256)]:
        assert L.ure_ridge_rows_scratch(m, k) == -1, (m, k)


# ---- 2. the contract against independent math ---------------------------------------------------------------------------
def _case(m, k, n_fixed, seed, lens=None):
    rs = np.random.RandomState(seed)
    F = rs.standard_normal((n_fixed, k + 3)).astype(np.float32)        # wider than k: only the first k columns enter
    lens = rs.randint(0, 3 * k, m) if lens is None else np.asarray(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rs.randint(0, n_fixed, off[-1]).astype(np.int32)
    val = (rs.randint(1, 6, off[-1]) / 5.0).astype(np.float32)
    return F, off, idx, val


@pytest.mark.parametrize('k,l2,l2_n', [(1, 0.5, 0.0), (5, 0.5, 0.05), (16, 1e-2, 0.0), (32, 1e-2, 0.05)])
def test_ref_equals_numpy_solve_on_the_same_systems(k, l2, l2_n):
    from ultrare_amd import ridge
    F, off, idx, val = _case(40, k, 50, seed=k)
    X, failed = ridge.ridge_rows_ref(F, k, off, idx, val, l2, l2_n)
    assert failed == [] and X.shape == (40, k) and X.dtype == np.float64
    for s in range(40):
        a, b = off[s], off[s + 1]
        if a == b:
            assert not X[s].any()
            continue
        f = F[idx[a:b], :k].astype(np.float64)
        G = f.T @ f + (l2 + l2_n * (b - a)) * np.eye(k)
        want = np.linalg.solve(G, f.T @ val[a:b].astype(np.float64))
        # both are backward-stable float64 solves: the difference is bounded by a few cond(G) eps
        assert np.abs(X[s] - want).max() <= 64 * np.linalg.cond(G) * np.finfo(np.float64).eps * np.abs(want).max(), s


def test_gradient_of_the_objective_vanishes_at_the_ref_answer():
    from ultrare_amd import ridge
    k, l2, l2_n = 6, 0.3, 0.02
    F, off, idx, val = _case(1, k, 30, seed=3, lens=[25])
    x = ridge.ridge_rows_ref(F, k, off, idx, val, l2, l2_n)[0][0]
    f, r = F[idx, :k].astype(np.float64), val.astype(np.float64)
    obj = lambda z: ((f @ z - r) ** 2).sum() + (l2 + l2_n * len(r)) * (z @ z)
    h = 1e-5
    grad = np.array([(obj(x + h * e) - obj(x - h * e)) / (2 * h) for e in np.eye(k)])
    scale = 2 * np.abs(f.T @ r).max()                     # the size of the gradient's two cancelling halves
    assert np.abs(grad).max() <= 1e-8 * scale
    assert obj(x) < obj(x + 1e-3) and obj(x) < obj(x * 0.999)


def test_empty_segment_gives_the_zero_row_and_never_fails():
    from ultrare_amd import ridge
    F, off, idx, val = _case(3, 4, 10, seed=0, lens=[0, 6, 0])
    for l2 in (0.0, 0.5):
        X, failed = ridge.ridge_rows_ref(F, 4, off, idx, val, l2)
        assert failed == [] and not X[0].any() and not X[2].any() and X[1].any()


def test_rank_deficient_segment_without_ridge_is_reported_not_returned():
    from ultrare_amd import ridge
    F, off, idx, val = _case(3, 4, 10, seed=1, lens=[9, 1, 12])         # one rating cannot fix four unknowns
    X, failed = ridge.ridge_rows_ref(F, 4, off, idx, val, 0.0, 0.0)
    assert failed == [1] and np.isnan(X[1]).all() and np.isfinite(X[[0, 2]]).all()
    X, failed = ridge.ridge_rows_ref(F, 4, off, idx, val, 1e-3, 0.0)
    assert failed == [] and np.isfinite(X).all()
    X, failed = ridge.ridge_rows_ref(F, 4, off, idx, val, 0.0, 1e-3)    # the count-scaled term alone makes it definite too
    assert failed == [] and np.isfinite(X).all()
    Fn = F.copy()
    Fn[idx[0], 0] = np.nan
    assert 0 in ridge.ridge_rows_ref(Fn, 4, off, idx, val, 0.5)[1]


@pytest.mark.parametrize('bad', [-1e-3, float('nan'), float('inf'), 'big', None, True])
def test_check_ridge_args(bad):
    from ultrare_amd import ridge
    assert ridge.check_ridge_args(0, 0.5) == (0.0, 0.5)
    with pytest.raises(ValueError, match='l2 must'):
        ridge.check_ridge_args(bad)
    with pytest.raises(ValueError, match='l2_n must'):
        ridge.check_ridge_args(0.1, bad)


# ---- 3. trainer_l2 ---------------------------------------------------------------------------------------------------------
def test_trainer_l2_matches_its_formula():
    from ultrare_amd.method.utils import trainer_l2
    assert trainer_l2(896914, 30000, 0.1) == 0.1 * 30 / 2
    assert trainer_l2(30000, 30000, 0.1) == 0.05 and trainer_l2(30001, 30000, 0.1) == 0.1
    assert trainer_l2(1, 3000, 0.2) == 0.1 and trainer_l2(0, 3000, 0.2) == 0.0
    for n, b, lam in [(12345, 100, 0.03), (7, 7, 1.0), (22500000, 30000, 0.1)]:
        assert trainer_l2(n, b, lam) == lam * np.ceil(n / b) / 2
    with pytest.raises(ValueError):
        trainer_l2(10, 0, 0.1)


def test_full_batch_sgd_with_momentum_and_weight_decay_converges_to_the_ridge_row():
    """The trainer's update for ONE row against a frozen table, one step per epoch (batch >= n_rows): gradient of the SUM of
    squared errors plus lam * x, torch.optim.SGD's momentum buffer.  Its limit is the ridge row at trainer_l2."""
    from ultrare_amd import ridge
    from ultrare_amd.method.utils import trainer_l2
    rs = np.random.RandomState(0)
    k, n, lam, mu, lr = 4, 12, 0.1, 0.9, 1e-3
    V = rs.standard_normal((n, k)).astype(np.float32)
    r = (rs.randint(1, 6, n) / 5.0).astype(np.float32)
    f, rr = V.astype(np.float64), r.astype(np.float64)
    x, buf = rs.standard_normal(k), np.zeros(k)
    for _ in range(60000):
        g = 2 * f.T @ (f @ x - rr) + lam * x
        buf = mu * buf + g
        x = x - lr * buf
    l2 = trainer_l2(n, 3000, lam)
    assert l2 == lam / 2
    want = ridge.ridge_rows_ref(V, k, [0, n], np.arange(n), r, l2)[0][0]
    assert np.abs(x - want).max() <= 1e-10 * np.abs(want).max()
    other = ridge.ridge_rows_ref(V, k, [0, n], np.arange(n), r, lam)[0][0]     # (the naive strength is measurably elsewhere)
    assert np.abs(x - other).max() > 1e-4 * np.abs(want).max()


# ---- 4. the CSR builder ------------------------------------------------------------------------------------------------------
def test_segment_csr_is_stable_with_right_offsets_and_longest_first_order():
    from ultrare_amd import ridge
    seg = np.array([2, 0, 2, 3, 0, 2, 5, 5])
    other = np.array([7, 1, 3, 9, 0, 3, 4, 2])
    r = np.arange(8, dtype=np.float64) / 10
    off, idx, val, order = ridge.segment_csr(seg, other, r, 7)
    assert off.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == np.float32 and order.dtype == np.int32
    assert off.tolist() == [0, 2, 2, 5, 6, 6, 8, 8]
    assert idx.tolist() == [1, 0, 7, 3, 3, 9, 4, 2]                      # inside a segment: the order given, repeats kept
    assert np.array_equal(val, np.array([1, 4, 0, 2, 5, 3, 6, 7], dtype=np.float32) / np.float32(10))
    assert order.tolist() == [2, 0, 5, 3, 1, 4, 6]                       # longest first, equal lengths by ascending id
    rs = np.random.RandomState(1)
    seg = rs.randint(0, 70000, 200000)                                   # more than 65,536 segments: the wide-key sort
    other = rs.randint(0, 1000, 200000)
    off, idx, val, order = ridge.segment_csr(seg, other, np.ones(200000), 70000)
    perm = np.argsort(seg, kind='stable')
    assert np.array_equal(idx, other[perm]) and np.array_equal(np.diff(off), np.bincount(seg, minlength=70000))
    lens = np.diff(off)[order]
    assert (np.diff(lens) <= 0).all() and sorted(order.tolist()) == list(range(70000))
    off, idx, val, order = ridge.segment_csr([], [], [], 3)
    assert off.tolist() == [0, 0, 0, 0] and len(idx) == 0 and order.tolist() == [0, 1, 2]


@pytest.mark.parametrize('seg,other,r,n', [([0, 3], [1, 1], [0.2, 0.4], 3), ([-1, 0], [1, 1], [0.2, 0.4], 3), ([0, 1], [-2, 1], [0.2, 0.4], 3),
                                           ([0, 1], [1, 1 << 31], [0.2, 0.4], 3), ([0, 1, 2], [1, 1], [0.2, 0.4], 3), ([0, 1], [1, 1], [0.2], 3),
                                           ([], [], [], -1)])
def test_segment_csr_refuses_ids_out_of_range(seg, other, r, n):
    from ultrare_amd import ridge
    with pytest.raises(ValueError):
        ridge.segment_csr(np.asarray(seg, dtype=np.int64), np.asarray(other, dtype=np.int64), r, n)


def test_segment_set_refuses_before_device_work(nv, monkeypatch):
    from ultrare_amd import engine
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match='segment ids outside'):
        engine.SegmentSet([0, 9], [1, 1], [0.2, 0.4], 3)


# ---- 5. the operator surface refuses bad settings before device work ------------------------------------------------------
def _no_device(monkeypatch):
    from ultrare_amd import engine

    def no_device():
        raise AssertionError('device work started')
    monkeypatch.setattr(engine, '_device', no_device)
    monkeypatch.setattr(engine, 'ridge_rows', lambda *a, **kw: no_device())
    monkeypatch.setattr(engine, 'merge_rows', lambda *a, **kw: no_device())


def _triple(users, seed=0, per_user=4):
    rs = np.random.RandomState(seed)
    uid = np.repeat(np.asarray(users, dtype=np.int64), per_user)
    return uid, rs.randint(0, 9, len(uid)), rs.randint(1, 6, len(uid)) / 5.0


def _loader(users, seed=0):
    from ultrare_amd.read import RatingData, loadData
    return loadData(RatingData(np.vstack(_triple(users, seed))), 30, 0)


BAD_L2 = [{'l2': -1e-3}, {'l2': float('nan')}, {'l2': float('inf')}, {'l2': 'big'}, {'l2': 0.5, 'l2_n': -1.0}, {'l2': 0.5, 'l2_n': float('nan')}]


@pytest.mark.parametrize('kw', BAD_L2 + [{'l2': 0.5, 'item_table': 2}, {'l2': 0.5, 'item_table': -1}, {'l2': 0.5, 'item_table': 'median'},
                                         {'l2': 0.5, 'item_table': 1.0}])
def test_fold_in_refuses_bad_settings_before_device_work(nv, kw, monkeypatch):
    from ultrare_amd.method import utils
    _no_device(monkeypatch)
    models = [object(), object()]               # never looked at: every check comes first
    for data in (_loader([8, 9]), _triple([8, 9])):
        with pytest.raises(ValueError):
            utils.fold_in(models, data, **kw)
    with pytest.raises(ValueError, match='at least one model'):
        utils.fold_in([], _triple([8]), 0.5)
    with pytest.raises(ValueError, match='negative'):
        utils.fold_in(models, (np.array([-1]), np.array([0]), np.array([0.2])), 0.5)


@pytest.mark.parametrize('kw', BAD_L2 + [{'l2': 0.5, 'sweeps': -1}, {'l2': 0.5, 'sweeps': 1.5}])
def test_als_sweeps_refuses_bad_settings_before_device_work(nv, kw, monkeypatch):
    from ultrare_amd.method import utils
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        utils.als_sweeps(object(), _triple([0, 1]), **kw)


def _sisa(n_user=12):
    from ultrare_amd.method.sisa import Sisa
    param = types.SimpleNamespace(n_user=n_user, n_item=9, k=4, lam=0.1, seed=1, lr=1e-3, lr_decay=0.95, momentum=0.9, epochs=1, batch=30,
                                  parallel=True)
    s = Sisa(param, 'mf', 2, [[0, 1, 2, 3], [4, 5, 6]])
    s.model_list = [object(), object()]
    return s


@pytest.mark.parametrize('users,kw', [([8, 9], k) for k in BAD_L2] +
                         [([8, 9], {'l2': 0.5, 'against': 'both'}),
                          ([8, 5], {'l2': 0.5}),                                   # 5 is in group 1 already
                          ([0], {'l2': 0.5}),
                          ([8, 12], {'l2': 0.5}),                                  # id >= n_user
                          ([8, 400], {'l2': 0.5}),
                          ([8, 9], {'l2': 0.5, 'groups': [0]}),                    # another length
                          ([8, 9], {'l2': 0.5, 'groups': [0, 1, 1]}),
                          ([8, 9], {'l2': 0.5, 'groups': [0, 2]}),                 # outside 0 .. n_group - 1
                          ([8, 9], {'l2': 0.5, 'groups': [-1, 0]}),
                          ([8, 9], {'l2': 0.5, 'groups': [0.5, 1.0]})])
def test_sisa_fold_in_refuses_bad_settings_before_device_work(nv, users, kw, monkeypatch):
    _no_device(monkeypatch)
    s = _sisa()
    s.combiner = 'fitted'
    with pytest.raises(ValueError):
        s.fold_in(_loader(users), **kw)
    assert s.group_index == [[0, 1, 2, 3], [4, 5, 6]] and s.folded == {} and s.combiner == 'fitted'      # nothing was changed


def test_sisa_fold_in_needs_models_and_ratings(nv, monkeypatch):
    _no_device(monkeypatch)
    s = _sisa()
    s.model_list = []
    with pytest.raises(ValueError, match='call learn first'):
        s.fold_in(_loader([8]), 0.5)
    s = _sisa()
    with pytest.raises(ValueError, match='at least one rating'):
        s.fold_in((np.zeros(0, int), np.zeros(0, int), np.zeros(0)), 0.5)
    with pytest.raises(ValueError, match='items outside'):
        s.fold_in((np.array([8]), np.array([9]), np.array([0.2])), 0.5)


def test_forget_folded_refuses_a_user_that_was_not_folded(nv, monkeypatch):
    _no_device(monkeypatch)
    s = _sisa()
    s.folded = {8: 0}
    s.group_index[0].append(8)
    s.combiner = 'fitted'
    with pytest.raises(ValueError, match=r'users \[2, 9\] were not folded in.*unlearn'):
        s.forget_folded([8, 2, 9])
    assert s.folded == {8: 0} and s.group_index[0] == [0, 1, 2, 3, 8] and s.combiner == 'fitted'


def test_default_assignment_fills_the_smallest_group_first(nv, monkeypatch):
    """The bookkeeping of fold_in with the device part replaced: groups of 4 and 3 users take 8 -> group 1, then 9 -> group 0
    (a tie: the lowest id), then 10 -> group 1."""
    import torch
    from ultrare_amd.method import sisa as sisa_mod
    from ultrare_amd.method.sisa import Sisa
    seen = []
    monkeypatch.setattr(sisa_mod.utils, 'fold_in', lambda models, data, l2, l2_n, table: (seen.append((table, np.unique(data[0]).tolist())) or
                                                                                            (np.unique(data[0]), torch.zeros(len(np.unique(data[0])), 4))))
    monkeypatch.setattr(Sisa, '_set_rows', lambda self, users, rows=None: None)
    s = _sisa()
    s.combiner = 'fitted'
    users, home = s.fold_in(_loader([10, 8, 9]), 0.5)
    assert users.tolist() == [8, 9, 10] and home.tolist() == [1, 0, 1]
    assert s.group_index == [[0, 1, 2, 3, 9], [4, 5, 6, 8, 10]] and s.folded == {8: 1, 9: 0, 10: 1} and s.combiner is None
    assert seen == [(0, [9]), (1, [8, 10])]                              # 'home': each against its own group's item table
    seen.clear()
    users, home = s.fold_in(_loader([11]), 0.5, groups=[0], against='ensemble')
    assert home.tolist() == [0] and seen == [('mean', [11])] and s.folded[11] == 0
    s.forget_folded([9, 10])
    assert s.group_index == [[0, 1, 2, 3, 11], [4, 5, 6, 8]] and s.folded == {8: 1, 11: 0}


# ---- 6. learn and unlearn keep self.folded right ----------------------------------------------------------------------------
def test_learn_clears_folded_and_unlearn_drops_the_retrained_shards_folded_users(nv, monkeypatch):
    import torch
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import MF

    monkeypatch.setattr(Sisa, '_train_parallel', lambda self, ids, *a, **kw: {i: MF(12, 9, 4) for i in ids})
    monkeypatch.setattr(Sisa, '_merge', lambda self, merged, ids: None)
    monkeypatch.setattr(Sisa, 'test', lambda self, *a: None)
    torch.manual_seed(0)
    s = _sisa()
    s.model_list = []
    loaders = [_loader([0, 1, 2, 3], 1), _loader([4, 5, 6], 2)]
    s.folded = {8: 0, 9: 1}
    models = s.learn(loaders, loaders, loaders[0], 0, '')
    assert s.folded == {}
    s.group_index = [[0, 1, 2, 3, 8, 10], [4, 5, 6, 9]]
    s.folded = {8: 0, 10: 0, 9: 1}
    s.unlearn(models, loaders, loaders, loaders[0], [5], 0, '')          # a trained user of group 1
    assert s.retrained == [1] and s.folded == {8: 0, 10: 0}
    s.unlearn(models, loaders, loaders, loaders[0], [], 0, '')           # nothing retrained: nothing dropped
    assert s.folded == {8: 0, 10: 0}
    s.unlearn(models, loaders, loaders, loaders[0], [10], 0, '')         # a folded user passed to unlearn retrains its home shard
    assert s.retrained == [0] and s.folded == {}
