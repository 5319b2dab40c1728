"""The learned shard combiner, host side (-m "not gpu"): ure_combine_stats / ure_score_weighted reject every bad argument
before any HIP call and their size queries follow their formulas; fit_combiner / Sisa.fit_combiner refuse bad settings
before device work; the numpy restatement of the contract (stats_contract, predict_contract), which the GPU tests hold the
kernels to, drives the host's Newton fit against independent math; Sisa.learn / unlearn drop a fitted combiner (checked
here, with the training body monkeypatched).  Nothing here initialises HIP."""
import ctypes
import types

import numpy as np
import pytest


# ---- the contract in numpy ---------------------------------------------------------------------------------------------
def z_contract(P, theta):
    """z[j] = b + sum_s w[s] * (double)p[j, s], added in the order b, s = 0, 1, ..., every product rounded before it is added."""
    P = np.asarray(P)
    theta = np.asarray(theta, dtype=np.float64)
    S = P.shape[1]
    z = np.full(len(P), theta[S], dtype=np.float64)
    for s in range(S):
        z = z + theta[s] * P[:, s].astype(np.float64)
    return z


def link_contract(link, z):
    """-> (mu, h): link 0 linear, link 1 logistic (exp(-z) may overflow to inf for z << 0: mu is then 0, as on the device)."""
    if link == 0:
        return z, np.ones_like(z)
    with np.errstate(over='ignore'):
        mu = 1.0 / (1.0 + np.exp(-z))
    return mu, mu * (1.0 - mu)


def stats_terms(P, r, link, theta):
    """The per-pair terms of every entry of the stats vector: [n_pairs, len - 1] (entry 0, n, has none)."""
    P = np.asarray(P)
    S = P.shape[1]
    X = np.concatenate([P.astype(np.float64), np.ones((len(P), 1))], axis=1)
    r = np.asarray(r).astype(np.float64)
    z = z_contract(P, theta)
    mu, h = link_contract(link, z)
    loss = (mu - r) ** 2 / 2 if link == 0 else np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))) - r * z
    iu = np.triu_indices(S + 1)
    return np.concatenate([loss[:, None], (mu - r)[:, None] * X, h[:, None] * X[:, iu[0]] * X[:, iu[1]]], axis=1)


def stats_contract(P, r, link, theta):
    """{ n, sum loss, g = sum (mu - r) x, upper triangle of H = sum h x x^T (row-major) } in float64."""
    T = stats_terms(P, r, link, theta)
    return np.concatenate([[float(len(T))], T.sum(axis=0)])


def predict_contract(P, link, rows):
    """pred[j] = (float32)link(z[j]) with the weight row rows[j] ([n, S + 1]) of pair j."""
    P = np.asarray(P)
    S = P.shape[1]
    z = rows[:, S].astype(np.float64).copy()
    for s in range(S):
        z = z + rows[:, s] * P[:, s].astype(np.float64)
    return link_contract(link, z)[0].astype(np.float32)


def synthetic_scores(n, S, seed, noise=0.3):
    """Well-conditioned shard scores: a common signal plus independent noise per shard, ratings in [0.2, 1]."""
    rs = np.random.RandomState(seed)
    r = rs.choice(np.arange(1, 6), n).astype(np.float32) / np.float32(5)
    P = (r[:, None] * rs.uniform(0.5, 1.0, S)[None, :] + noise * rs.standard_normal((n, S))).astype(np.float32)
    return P, r


@pytest.fixture(scope='session')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ---- 1. the C calls refuse bad arguments -------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(0x1000)                         # never dereferenced: every check fails before the device is touched


def _tables(S, hole=None):
    n = max(S, 1)
    return (ctypes.c_void_p * n)(*[None if k == hole else 0x1000 for k in range(n)])


def _stats(nv, S=3, n=100, d=16, link=0, scratch_bytes=None, U=True, V=True, uid=True, iid=True, rating=True, w=True, out=True, scratch=True, hole=None):
    L = nv.lib()
    if scratch_bytes is None:
        scratch_bytes = max(L.ure_combine_stats_scratch(n, S), 0)
    f = lambda on: FAKE if on else None
    return L.ure_combine_stats(_tables(S, hole) if U else None, _tables(S) if V else None, S, f(uid), f(iid), f(rating), n, d, link, f(w), f(out),
                               f(scratch), scratch_bytes, None)


def _weighted(nv, S=3, n=100, d=16, link=0, n_groups=1, n_user=10, U=True, V=True, uid=True, iid=True, rating=True, W=True, gou=False, pred=True,
              sse=True, hole=None):
    f = lambda on: FAKE if on else None
    return nv.lib().ure_score_weighted(_tables(S, hole) if U else None, _tables(S) if V else None, S, f(uid), f(iid), f(rating), n, d, link, f(W),
                                       n_groups, f(gou), n_user, f(pred), f(sse), None)


BAD_COMMON = [({'U': False}, 'U_tables && V_tables'), ({'V': False}, 'U_tables && V_tables'), ({'S': 0}, 'n_models >= 1'),
              ({'S': 33}, 'n_models <= URE_MAX_MODELS_PER_CALL'), ({'uid': False}, 'uid && iid'), ({'iid': False}, 'uid && iid'),
              ({'n': 0}, 'n >= 1'), ({'n': -5}, 'n >= 1'), ({'d': 0}, 'pow2(d)'), ({'d': 2}, 'd >= 4'), ({'d': 24}, 'pow2(d)'),
              ({'d': 512}, 'd <= 256'), ({'link': 2}, 'link == 0 || link == 1'), ({'link': -1}, 'link == 0 || link == 1'),
              ({'hole': 1}, 'U_tables[m] && V_tables[m]')]


@pytest.mark.parametrize('kw,word', BAD_COMMON + [({'rating': False}, 'uid && iid && rating'), ({'w': False}, 'w && out && scratch'),
                                                  ({'out': False}, 'w && out && scratch'), ({'scratch': False}, 'w && out && scratch'),
                                                  ({'scratch_bytes': 0}, 'scratch_bytes >= ure_combine_stats_scratch'),
                                                  ({'n': 1000, 'S': 32, 'scratch_bytes': 16 * 596 * 8 - 1}, 'scratch_bytes >= ure_combine_stats_scratch')])
def test_combine_stats_rejects_bad_arguments(nv, kw, word):
    assert _stats(nv, **kw) == -1
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


@pytest.mark.parametrize('kw,word', BAD_COMMON + [({'pred': False}, 'uid && iid && pred'), ({'rating': False}, '!sse || rating'),
                                                  ({'W': False}, 'W'), ({'n_groups': 0}, 'n_groups >= 1'), ({'n_groups': -2}, 'n_groups >= 1'),
                                                  ({'gou': True, 'n_user': 0}, '!group_of_user || n_user >= 1')])
def test_score_weighted_rejects_bad_arguments(nv, kw, word):
    assert _weighted(nv, **kw) == -1
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


def test_stats_len_and_scratch_follow_their_formulas(nv):
    L = nv.lib()
    from ultrare_amd import combine
    for S in range(1, 33):
        want = 2 + (S + 1) + (S + 1) * (S + 2) // 2
        assert L.ure_combine_stats_len(S) == want == combine.stats_len(S)
    assert L.ure_combine_stats_len(32) == 596
    for S in (0, -1, 33):
        assert L.ure_combine_stats_len(S) == -1
    for n, S in [(1, 1), (63, 2), (64, 5), (65, 5), (100003, 3), (64 * 2048, 32), (64 * 2048 + 1, 32), (22500000, 32), (1 << 40, 7)]:
        blocks = min(-(-n // 64), 2048)
        assert L.ure_combine_stats_scratch(n, S) == blocks * L.ure_combine_stats_len(S) * 8, (n, S)
    assert L.ure_combine_stats_scratch(22500000, 32) < 64 << 20          # the point of not writing n x S (2.9 GB)
    for n, S in [(0, 3), (-1, 3), (10, 0), (10, 33)]:
        assert L.ure_combine_stats_scratch(n, S) == -1, (n, S)


# ---- 2. the operator surface refuses bad settings before device work ------------------------------------------------------
def _loader(n=50, seed=0, n_user=8):
    from ultrare_amd.read import RatingData, loadData
    rs = np.random.RandomState(seed)
    return loadData(RatingData(np.vstack([rs.randint(0, n_user, n), rs.randint(0, 9, n), rs.randint(1, 6, n) / 5.0])), 30, 0)


def _no_device(monkeypatch):
    from ultrare_amd import engine

    def no_device():
        raise AssertionError('device work started')
    monkeypatch.setattr(engine, '_device', no_device)


BAD_SETTINGS = [{'link': 'probit'}, {'link': None}, {'link': 0}, {'l2': -1e-3}, {'l2': float('nan')}, {'l2': float('inf')}, {'l2': 'big'},
                {'max_iter': 0}, {'max_iter': -4}, {'max_iter': 2.5}, {'tol': -1.0}, {'tol': float('nan')}]


@pytest.mark.parametrize('kw', BAD_SETTINGS + [{'groups': [[0, 1], [2, 3], [4]]}])
def test_fit_combiner_refuses_bad_settings_before_device_work(nv, kw, monkeypatch):
    from ultrare_amd.method import utils
    _no_device(monkeypatch)
    models = [object(), object()]               # never looked at: every check comes first
    with pytest.raises(ValueError):
        utils.fit_combiner(models, [_loader(seed=1), _loader(seed=2)], **kw)


def test_fit_combiner_refuses_no_or_too_many_models(nv, monkeypatch):
    from ultrare_amd.method import utils
    _no_device(monkeypatch)
    for models in ([], [object()] * 33):
        with pytest.raises(ValueError, match='models'):
            utils.fit_combiner(models, _loader())


def _sisa(n_group=2, groups=((0, 1, 2, 3), (4, 5, 6, 7))):
    from ultrare_amd.method.sisa import Sisa
    param = types.SimpleNamespace(n_user=8, n_item=9, k=4, lam=0.1, seed=1, lr=1e-3, lr_decay=0.95, momentum=0.9, epochs=1, batch=30, parallel=True)
    return Sisa(param, 'mf', n_group, [list(g) for g in groups])


@pytest.mark.parametrize('kw', [k for k in BAD_SETTINGS if 'max_iter' not in k and 'tol' not in k])
def test_sisa_fit_combiner_refuses_bad_settings_before_device_work(nv, kw, monkeypatch):
    _no_device(monkeypatch)
    s = _sisa()
    s.model_list = [object(), object()]
    with pytest.raises(ValueError):
        s.fit_combiner([_loader(seed=1), _loader(seed=2)], **kw)
    assert s.combiner is None


def test_sisa_fit_combiner_refuses_a_loader_list_of_another_length(nv, monkeypatch):
    _no_device(monkeypatch)
    s = _sisa()
    s.model_list = [object(), object()]
    with pytest.raises(ValueError, match='3 training loaders for 2 groups'):
        s.fit_combiner([_loader(seed=1), _loader(seed=2), _loader(seed=3)])


def test_test_combined_without_a_combiner_raises(nv, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match='no combiner'):
        _sisa().test_combined(_loader(), 0, '')


# ---- 3. the contract against independent math ---------------------------------------------------------------------------
def _fit(P, r, link, l2=0.0, max_iter=25, tol=1e-10):
    from ultrare_amd import combine
    return combine.newton_fit(lambda theta: stats_contract(P, r, combine.LINKS[link], theta), P.shape[1], link, l2, max_iter, tol)


def test_stats_contract_is_the_gradient_and_hessian_of_its_loss():
    """Central differences of the summed loss reproduce g and H for both links (float64, step 1e-5)."""
    from ultrare_amd import combine
    P, r = synthetic_scores(400, 3, seed=2)
    theta = np.array([0.4, -0.2, 0.7, 0.1])
    for link in (0, 1):
        n, loss, g, H = combine.unpack_stats(stats_contract(P, r, link, theta), 3)
        assert n == 400
        f = lambda t: stats_contract(P, r, link, t)[1]
        e = np.eye(4) * 1e-5
        g_fd = np.array([(f(theta + e[a]) - f(theta - e[a])) / 2e-5 for a in range(4)])
        np.testing.assert_allclose(g, g_fd, rtol=1e-6, atol=1e-6 * np.abs(g).max())
        H_fd = np.array([[(stats_contract(P, r, link, theta + e[a])[2 + b] - stats_contract(P, r, link, theta - e[a])[2 + b]) / 2e-5 for b in range(4)]
                         for a in range(4)])
        np.testing.assert_allclose(H, H_fd, rtol=1e-6, atol=1e-6 * np.abs(H).max())
        assert np.array_equal(H, H.T)


@pytest.mark.parametrize('S,n', [(1, 300), (3, 2000), (5, 5000), (32, 20000)])
def test_linear_fit_without_ridge_is_least_squares(S, n):
    P, r = synthetic_scores(n, S, seed=S)
    A = np.concatenate([P.astype(np.float64), np.ones((n, 1))], axis=1)
    want, *_ = np.linalg.lstsq(A, r.astype(np.float64), rcond=None)
    fit = _fit(P, r, 'linear')
    assert fit['iters'] == 1 and fit['passes'] == 2 and fit['n'] == n
    # cond(A) is below 100 here, so lstsq's own error is ~1e-14: 1e-9 relative to the largest coefficient
    assert np.abs(fit['theta'] - want).max() <= 1e-9 * np.abs(want).max()
    res = A @ want - r
    assert abs(fit['loss_after'] - 0.5 * res @ res) <= 1e-9 * fit['loss_after']
    assert fit['loss_after'] <= fit['loss_before']
    assert fit['grad_norm'] <= 1e-9 * n           # the certificate of the second pass


def test_linear_fit_with_huge_ridge_is_the_mean_ensemble_with_its_mean_residual():
    P, r = synthetic_scores(3000, 4, seed=9)
    fit = _fit(P, r, 'linear', l2=1e12)
    w, b = fit['theta'][:4], fit['theta'][4]
    assert np.abs(w - 0.25).max() <= 1e-6
    mean_pred = z_contract(P, [0.25] * 4 + [0.0])
    assert abs(b - np.mean(r.astype(np.float64) - mean_pred)) <= 1e-6


@pytest.mark.parametrize('l2', [0.0, 1.0, 100.0])
def test_logistic_fit_reaches_a_stationary_point_without_ever_increasing(l2):
    P, r = synthetic_scores(4000, 5, seed=4)
    fit = _fit(P, r, 'logistic', l2=l2)
    assert 1 <= fit['iters'] < 25
    assert fit['grad_norm'] <= 1e-8 * 4000
    obj = fit['objective']
    assert len(obj) == fit['iters'] + 1 and all(b < a for a, b in zip(obj[:-1], obj[1:]))
    assert fit['loss_after'] < fit['loss_before']
    # a Newton step recomputed here from the fitted point moves nothing
    from ultrare_amd import combine
    n, loss, g, H = combine.unpack_stats(stats_contract(P, r, 1, fit['theta']), 5)
    m = np.array([1.0] * 5 + [0.0])
    delta = np.linalg.solve(H + l2 * np.diag(m), g + l2 * m * (fit['theta'] - combine.mean_weights(5)))
    assert np.abs(delta).max() <= 1e-8


def test_objective_never_increases_when_steps_must_be_halved():
    """A start far from the optimum of a saturating problem: scores scaled so that the first full Newton step overshoots."""
    rs = np.random.RandomState(0)
    P = (rs.standard_normal((500, 2)) * 30).astype(np.float32)
    r = (rs.uniform(size=500) < 1 / (1 + np.exp(-(0.2 * P[:, 0] - 0.1 * P[:, 1])))).astype(np.float32)
    fit = _fit(P, r, 'logistic', l2=1e-3, max_iter=60)
    obj = fit['objective']
    assert all(b < a for a, b in zip(obj[:-1], obj[1:]))
    assert fit['passes'] > fit['iters'] + 1          # some step was halved
    assert fit['loss_after'] < fit['loss_before']


def test_singular_system_raises_naming_l2():
    P, r = synthetic_scores(200, 2, seed=1)
    P[:, 1] = P[:, 0]                                 # two identical shards: H is singular
    for link in ('linear', 'logistic'):
        with pytest.raises(ValueError, match='l2 = 0'):
            _fit(P, r, link)
        fit = _fit(P, r, link, l2=1e-3)               # the ridge makes it definite; the twins share the weight
        assert abs(fit['theta'][0] - fit['theta'][1]) <= 1e-9
    with pytest.raises(ValueError, match='l2'):
        _fit(np.full((10, 1), np.nan, np.float32), r[:10], 'linear')


def test_max_iter_caps_the_accepted_steps():
    P, r = synthetic_scores(1000, 3, seed=6)
    assert _fit(P, r, 'logistic', max_iter=2)['iters'] == 2


def test_first_group_rule_and_users_outside_every_group():
    from ultrare_amd import combine
    groups = [[0, 1, 2], [2, 3], [5]]
    assert combine.first_group_map(groups, 7).tolist() == [0, 0, 0, 1, -1, 2, -1]       # user 2: the first group that lists it
    W = np.tile(combine.mean_weights(2), (3, 1))
    assert combine.Combiner(W, 'linear', groups).group_of_user(7).tolist() == [0, 0, 0, 1, -1, 2, -1]
    with pytest.raises(ValueError, match='in no group'):
        combine.Combiner(W, 'logistic', groups).group_of_user(7)
    assert combine.Combiner(W[:1], 'logistic').group_of_user(7) is None
    with pytest.raises(ValueError, match='outside'):
        combine.first_group_map([[0, 9]], 7)
    with pytest.raises(ValueError):
        combine.Combiner(W, 'linear')                 # three rows need their groups
    with pytest.raises(ValueError):
        combine.Combiner(W, 'linear', groups[:2])


# ---- 4. a combiner never survives a deletion ---------------------------------------------------------------------------
def test_learn_and_unlearn_drop_the_combiner(nv, monkeypatch):
    """Checked on the CPU: the training body, the merge and the test are replaced; what is left of learn / unlearn is their
    own bookkeeping, and the fitted weights must be gone before any of it runs."""
    import torch
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import MF
    seen = []

    def fake_train(self, ids, *a, **kw):
        seen.append(self.combiner)
        return {i: MF(8, 9, 4) for i in ids}
    monkeypatch.setattr(Sisa, '_train_parallel', fake_train)
    monkeypatch.setattr(Sisa, '_merge', lambda self, merged, ids: None)
    monkeypatch.setattr(Sisa, 'test', lambda self, *a: None)
    torch.manual_seed(0)
    s = _sisa()
    assert s.combiner is None
    loaders = [_loader(seed=1), _loader(seed=2)]
    s.combiner = 'fitted'
    models = s.learn(loaders, loaders, loaders[0], 0, '')
    assert s.combiner is None and seen == [None]
    s.combiner = 'fitted'
    s.unlearn(models, loaders, loaders, loaders[0], [5], 0, '')
    assert s.combiner is None and seen == [None, None] and s.retrained == [1]
    s.combiner = 'fitted'
    s.unlearn(models, loaders, loaders, loaders[0], [], 0, '')            # nothing to retrain: the weights still go
    assert s.combiner is None
    with pytest.raises(ValueError, match='no combiner'):
        s.test_combined(loaders[0], 0, '')
