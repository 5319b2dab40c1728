"""The learned shard combiner on the device (csrc/mf_combine.hip), held to the numpy contract of tests/test_cpu_combine.py:
the per-model score pin, the stats reduction, bitwise reproducibility, weighted scoring against the mean and against the
contract, the fit on the reference's toy ensembles, Sisa end to end, the torch ops and the configs[3] shape."""
import ctypes
import os
import time

import numpy as np
import pytest
import torch

if __name__ == '__main__':          # the scale test's child process: what conftest.py does for a pytest run
    import sys
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

from oracle import cpu_ref as O
from test_cpu_combine import predict_contract, stats_contract, stats_terms

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071
EPS32 = float(np.finfo(np.float32).eps)


def random_case(n, S, d, n_user=300, n_item=200, seed=0, shared_u=False):
    """S random models of width d (scores of unit scale) and n random pairs with ratings in {0.2 .. 1}, on the device."""
    rs = np.random.RandomState(seed * 1000 + n % 997 + S * 7 + d)
    scale = d ** -0.25
    U0 = torch.from_numpy((rs.standard_normal((n_user, d)) * scale).astype(np.float32)).cuda()
    tables = []
    for _ in range(S):
        U = U0 if shared_u else torch.from_numpy((rs.standard_normal((n_user, d)) * scale).astype(np.float32)).cuda()
        tables.append((U, torch.from_numpy((rs.standard_normal((n_item, d)) * scale).astype(np.float32)).cuda()))
    uid = rs.randint(0, n_user, n).astype(np.int32)
    iid = rs.randint(0, n_item, n).astype(np.int32)
    r = (rs.randint(1, 6, n) / 5.0).astype(np.float32)
    return tables, (uid, iid, r)


def device_scores(tables, d, uid, iid):
    """P [n, S] float32: every model's score vector as ure_score gives it for that model alone (first = 1, last = 0)."""
    from ultrare_amd import _native as nv
    u, i = torch.from_numpy(uid).cuda(), torch.from_numpy(iid).cuda()
    P = torch.empty(len(tables), len(uid), dtype=torch.float32, device='cuda')
    for s, (U, V) in enumerate(tables):
        Up, Vp = (ctypes.c_void_p * 1)(U.data_ptr()), (ctypes.c_void_p * 1)(V.data_ptr())
        nv.check(nv.lib().ure_score(Up, Vp, 1, 1, 1, 0, nv.ptr(u), nv.ptr(i), None, len(uid), d, nv.ptr(P[s]), None, nv.stream_handle()), 'ure_score')
    return P.cpu().numpy().T.copy()


# ---- 5. the score pin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [4, 8, 16, 32, 64, 128, 256])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 100003])
def test_stats_see_the_scores_of_ure_score(n, d):
    from ultrare_amd import engine
    S = 3
    tables, (uid, iid, r) = random_case(n, S, d)
    P = device_scores(tables, d, uid, iid)
    pairs = engine.PairSet(uid, iid, r)
    for s in range(S):
        w = np.zeros(S + 1)
        w[s] = 1.0
        got = engine.combine_stats(tables, d, pairs, 'linear', w)
        assert got[0] == n
        terms = P[:, s].astype(np.float64) - r.astype(np.float64)
        err = abs(got[2 + S] - terms.sum())
        print(f'n={n} d={d} s={s}: |g[S] - sum| = {err:.3g} of {np.abs(terms).sum():.6g}')
        assert err <= 1e-12 * np.abs(terms).sum()


# ---- 6. the reduction against the contract ---------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 2, 5, 32])
@pytest.mark.parametrize('link', [0, 1])
@pytest.mark.parametrize('kind', ['mean', 'random', 'saturated'])
def test_stats_match_the_contract_on_the_device_scores(S, link, kind):
    from ultrare_amd import combine, engine
    n, d = 20011, 32
    tables, (uid, iid, r) = random_case(n, S, d, seed=1)
    P = device_scores(tables, d, uid, iid)
    rs = np.random.RandomState(S)
    theta = combine.mean_weights(S) if kind == 'mean' else rs.standard_normal(S + 1)
    if kind == 'saturated':            # |z| up to 50: the sigmoid is 0 or 1 to the last bit for many pairs
        z = np.concatenate([P.astype(np.float64), np.ones((n, 1))], axis=1) @ theta
        theta = theta * (50.0 / np.abs(z).max())
    got = engine.combine_stats(tables, d, (uid, iid, r), link, theta)
    assert got.shape == (combine.stats_len(S),) and np.isfinite(got).all()
    want = stats_contract(P, r, link, theta)
    mag = np.abs(stats_terms(P, r, link, theta)).sum(axis=0)
    assert got[0] == want[0] == n
    rel = np.abs(got[1:] - want[1:]) / np.maximum(mag, np.finfo(np.float64).tiny)
    print(f'S={S} link={link} {kind}: worst entry error {rel.max():.3g} of its sum of magnitudes')
    assert (np.abs(got[1:] - want[1:]) <= 1e-12 * mag).all()


def test_stats_of_loaders_add_up_to_the_stats_of_their_union():
    """What the global fit relies on: the per-loader vectors added in index order are the stats of all pairs (to rounding)."""
    from ultrare_amd import engine
    tables, (uid, iid, r) = random_case(5000, 4, 16, seed=2)
    theta = np.array([0.3, 0.1, 0.4, 0.2, 0.05])
    whole = engine.combine_stats(tables, 16, (uid, iid, r), 'logistic', theta)
    parts = [engine.combine_stats(tables, 16, (uid[a:b], iid[a:b], r[a:b]), 'logistic', theta) for a, b in ((0, 1234), (1234, 1235), (1235, 5000))]
    np.testing.assert_allclose(np.sum(parts, axis=0), whole, rtol=1e-12, atol=1e-12 * np.abs(whole).max())


# ---- 7. determinism --------------------------------------------------------------------------------------------------------
def _toy_models(tag='S3'):
    from ultrare_amd.method.utils import MF
    g = np.load(os.path.join(G, 'sisa_toy.npz'))
    S = int(tag[1:])
    U = torch.from_numpy(g[f'{tag}_learn_Umerged']).cuda()
    models = [MF.from_tables(U, torch.from_numpy(g[f'{tag}_learn_V{i}']).cuda()) for i in range(S)]
    return models, [g[f'{tag}_index{i}'].tolist() for i in range(S)]


def _toy_loaders(S, del_user=()):
    from ultrare_amd.read import RatingData, loadData, readRating
    tr, idx = readRating(TRAIN, N_USER, 5, list(del_user), [], S, [])
    te, _ = readRating(TEST, N_USER, 5, [], [], S, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    tot = loadData(RatingData(np.hstack(te)), 3000, 24, False)
    return idx, trd, ted, tot


@pytest.mark.parametrize('link', ['linear', 'logistic'])
def test_two_fits_give_the_same_bytes_on_any_stream(link):
    from ultrare_amd.method.utils import fit_combiner
    models, groups = _toy_models()
    idx, trd, _, _ = _toy_loaders(3)
    assert idx == groups
    a = fit_combiner(models, trd, link, l2=1e-3, groups=groups)
    b = fit_combiner(models, trd, link, l2=1e-3, groups=groups)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        c = fit_combiner(models, trd, link, l2=1e-3, groups=groups)
    torch.cuda.synchronize()
    assert a.W.shape == (3, 4) and a.W.tobytes() == b.W.tobytes() == c.W.tobytes()
    assert a.loss_after.tobytes() == b.loss_after.tobytes() == c.loss_after.tobytes()
    assert a.iters.tolist() == b.iters.tolist() == c.iters.tolist()


# ---- 8. weighted scoring -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,d', [(1, 16), (3, 16), (5, 32), (32, 128)])
def test_mean_weights_score_like_the_mean_within_the_float32_bound(S, d):
    from ultrare_amd import _native as nv
    from ultrare_amd import combine, engine
    n = 30011
    tables, (uid, iid, r) = random_case(n, S, d, seed=3)
    P = device_scores(tables, d, uid, iid)
    u, i, rt = (torch.from_numpy(a).cuda() for a in (uid, iid, r))
    mean = torch.empty(n, dtype=torch.float32, device='cuda')
    sse = torch.empty(engine.SCORE_PARTIALS, dtype=torch.float64, device='cuda')
    Up = (ctypes.c_void_p * S)(*[U.data_ptr() for U, _ in tables])
    Vp = (ctypes.c_void_p * S)(*[V.data_ptr() for _, V in tables])
    nv.check(nv.lib().ure_score(Up, Vp, S, S, 1, 1, nv.ptr(u), nv.ptr(i), nv.ptr(rt), n, d, nv.ptr(mean), nv.ptr(sse), nv.stream_handle()), 'ure_score')
    W = torch.from_numpy(combine.mean_weights(S)[None, :]).cuda()
    pred, wsse = engine.score_weighted(tables, d, u, i, rt, 'linear', W)
    # NOT bit-equal by contract: a float64 weighted sum rounded once against a float32 running sum and a division
    bound = 4 * S * EPS32 * np.abs(P).sum(axis=1) / S
    diff = np.abs(pred.cpu().numpy().astype(np.float64) - mean.cpu().numpy().astype(np.float64))
    print(f'S={S} d={d}: worst |weighted - mean| / bound = {(diff / np.maximum(bound, 1e-300)).max():.3g}')
    assert (diff <= bound).all()
    rmse_mean, rmse_w = np.sqrt(sse.cpu().numpy().sum() / n), np.sqrt(wsse.cpu().numpy().sum() / n)
    assert abs(rmse_mean - rmse_w) <= 1e-6 * rmse_mean
    # a map that puts every user outside every group is the same mean (link 0)
    outside = torch.full((300,), -1, dtype=torch.int32, device='cuda')
    junk = torch.full((2, S + 1), 7.0, dtype=torch.float64, device='cuda')
    pred2, _ = engine.score_weighted(tables, d, u, i, rt, 'linear', junk, outside)
    assert torch.equal(pred, pred2)


def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


@pytest.mark.parametrize('d', [4, 8, 16, 32, 64, 128, 256])
@pytest.mark.parametrize('link', [0, 1])
def test_weighted_scores_follow_the_contract_at_every_width(link, d):
    """score_weighted_kernel<d / 4> round the edges of its 64-pair tile: the predictions against the contract on ure_score's
    scores, the layout of the squared-error partials (one per tile, zeros behind them, whatever the buffer held) and their sum."""
    from ultrare_amd import engine
    for S in (1, 5):
        for n in (1, 63, 64, 65, 257):
            tables, (uid, iid, r) = random_case(n, S, d, seed=7)
            P = device_scores(tables, d, uid, iid)
            W = np.random.RandomState(100 * S + n + d).standard_normal((2, S + 1))
            gou = (np.arange(300) % 2).astype(np.int32)
            u, i, rt = (torch.from_numpy(a).cuda() for a in (uid, iid, r))
            sse = torch.full((engine.SCORE_PARTIALS,), float('nan'), dtype=torch.float64, device='cuda')
            pred, sse = engine.score_weighted(tables, d, u, i, rt, link, torch.from_numpy(W).cuda(), torch.from_numpy(gou).cuda(), sse=sse)
            pred, sse = pred.cpu().numpy(), sse.cpu().numpy()
            ulps = _ulps(pred, predict_contract(P, link, W[gou[uid]]))
            used = min(-(-n // 64), engine.SCORE_PARTIALS)
            want_sse = ((pred.astype(np.float64) - r.astype(np.float64)) ** 2).sum()
            print(f'd={d} link={link} S={S} n={n}: worst {ulps.max():.2g} ulp, {used} partials, sse {sse.sum():.9g} against {want_sse:.9g}')
            assert ulps.max() <= 1.0
            assert sse.shape == (engine.SCORE_PARTIALS,) and (sse[used:] == 0.0).all() and np.isfinite(sse[:used]).all()
            assert abs(sse.sum() - want_sse) <= 1e-6 * want_sse


@pytest.mark.parametrize('link', ['linear', 'logistic'])
@pytest.mark.parametrize('per_group', [False, True])
def test_fitted_weights_score_as_the_contract_and_basetest_follows(link, per_group):
    from ultrare_amd import combine
    from ultrare_amd.method.utils import baseTest, fit_combiner, padded_tables
    models, groups = _toy_models()
    _, trd, _, tot = _toy_loaders(3)
    c = fit_combiner(models, trd, link, l2=1e-3, groups=groups if per_group else None)
    assert c.W.shape == ((3, 4) if per_group else (1, 4))
    got = baseTest(tot, models, combiner=c)
    ev = tot.eval_set()
    dev_pred = ev.predictions()
    uid, iid, r = tot.dataset.triples()
    tables = [padded_tables(m)[:2] for m in models]
    P = device_scores(tables, 16, uid, iid)
    rows = c.W[combine.first_group_map(groups, N_USER)[uid]] if per_group else np.repeat(c.W, len(uid), axis=0)
    want_pred = predict_contract(P, c.link_code, rows)
    ulps = _ulps(dev_pred, want_pred)
    print(f'{link} per_group={per_group}: {int((ulps > 0).sum())} of {len(uid)} predictions differ from the contract, worst {ulps.max():.2g} ulp')
    assert ulps.max() <= 1.0
    # every user of the toy test set is evaluated.  The ranking is checked on the DEVICE's predictions: where they differ
    # from the contract's by an ulp, a tie between two of a user's items could flip a rank; with equal bytes the two
    # references coincide anyway
    want = O.eval_from_pred(uid.astype(np.int64), r, dev_pred, 3000)
    print(f'  (rmse, ndcg, hr) = {got}; on the contract\'s predictions: {O.eval_from_pred(uid.astype(np.int64), r, want_pred, 3000)}')
    assert abs(got[0] - want[0]) <= 1e-6 * want[0]
    assert abs(got[1] - want[1]) <= 1e-12
    n_users = len(np.unique(uid))
    assert round(got[2] * n_users * 10) == round(want[2] * n_users * 10) and abs(got[2] - want[2]) <= 1e-12          # the same hits
    # without a combiner nothing changes
    plain = baseTest(tot, models)
    assert plain == baseTest(tot, models, combiner=None)


def test_logistic_combiner_refuses_a_user_outside_every_group():
    from ultrare_amd import combine
    from ultrare_amd.method.utils import baseTest
    models, groups = _toy_models()
    _, _, _, tot = _toy_loaders(3)
    W = np.tile(combine.mean_weights(3), (3, 1))
    short = [groups[0], groups[1], groups[2][:-1]]
    with pytest.raises(ValueError, match='in no group'):
        baseTest(tot, models, combiner=combine.Combiner(W, 'logistic', short))
    baseTest(tot, models, combiner=combine.Combiner(W, 'linear', short))          # the linear link gives that user the mean
    with pytest.raises(ValueError, match='fitted on 3 models'):
        baseTest(tot, models[:2], combiner=combine.Combiner(W, 'linear', groups))


# ---- 9. the reference's toy ensembles ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['S3', 'S4'])
def test_fit_on_the_reference_ensembles_never_loses_to_the_mean_on_its_training_pairs(tag):
    from ultrare_amd.method.utils import baseTest, fit_combiner
    S = int(tag[1:])
    models, groups = _toy_models(tag)
    idx, trd, _, tot = _toy_loaders(S)
    assert idx == groups
    glob = fit_combiner(models, trd, 'linear', l2=0.0)
    per = fit_combiner(models, trd, 'linear', l2=0.0, groups=groups)
    n_train = sum(len(l.dataset) for l in trd)
    assert glob.n.tolist() == [n_train] and per.n.tolist() == [len(l.dataset) for l in trd]
    assert glob.iters.tolist() == [1] and per.iters.tolist() == [1] * S
    # consequences of the contract, not measurements: the mean lies in the hypothesis class, per-group nests the global fit
    slack = 1e-9
    assert glob.loss_after[0] <= glob.loss_before[0] * (1 + slack)
    for g in range(S):
        assert per.loss_after[g] <= per.loss_before[g] * (1 + slack), g
    assert per.loss_after.sum() <= glob.loss_after[0] * (1 + slack)
    assert abs(per.loss_before.sum() - glob.loss_before[0]) <= 1e-9 * glob.loss_before[0]       # the same mean start, split
    assert glob.grad_norm[0] <= 1e-9 * n_train and (per.grad_norm <= 1e-9 * n_train).all()
    res = {'mean': baseTest(tot, models), 'global': baseTest(tot, models, combiner=glob), 'per-group': baseTest(tot, models, combiner=per)}
    print(f'{tag}: train loss mean {glob.loss_before[0]:.4f} -> global {glob.loss_after[0]:.4f} -> per-group {per.loss_after.sum():.4f}')
    for name, m in res.items():
        print(f'  test (rmse, ndcg, hr) {name}: {m}')          # recorded, not asserted: a property of 2-3-epoch toy models
        assert np.isfinite(m).all()
    print('  W per group:\n', per.W)


# ---- 10. Sisa end to end -------------------------------------------------------------------------------------------------------
class Param:
    def __init__(self, epochs, parallel):
        self.k, self.lam, self.seed, self.batch = 16, 0.1, 42, 3000
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, epochs
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, parallel


@pytest.mark.parametrize('parallel', [False, True])
def test_sisa_learn_fit_test_unlearn_refit(parallel, tmp_path):
    import copy
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import baseTest
    idx, trd, ted, tot = _toy_loaders(3)
    sisa = Sisa(Param(3, parallel), 'mf', 3, idx)
    torch.manual_seed(42)
    ml = sisa.learn(trd, ted, tot, 0, str(tmp_path))
    assert sisa.combiner is None
    with pytest.raises(ValueError, match='no combiner'):
        sisa.test_combined(tot, 0, '')
    log0 = dict(sisa.log0)
    c = sisa.fit_combiner(trd)
    assert c is sisa.combiner and c.W.shape == (3, 4) and c.link == 'linear'
    assert c.n.tolist() == [len(l.dataset) for l in trd]
    got = sisa.test_combined(tot, 0, str(tmp_path))
    assert np.isfinite(got).all()
    assert got == baseTest(tot, sisa.model_list, combiner=sisa.combiner)
    saved = np.load(tmp_path / 'log0c.npy', allow_pickle=True).item()
    assert saved == sisa.log0c == {'total_rmse': got[0], 'total_ndcg': got[1], 'total_hr': got[2]}
    sisa.test(tot, 0, '')                                           # the mean's test is blind to a combiner being there
    assert sisa.log0 == log0
    assert np.load(tmp_path / 'log0.npy', allow_pickle=True).item() == log0
    one = sisa.fit_combiner(trd, link='logistic', l2=1e-2, per_group=False)
    assert one.W.shape == (1, 4) and one.groups is None and one.n.tolist() == [sum(len(l.dataset) for l in trd)]
    assert np.isfinite(sisa.test_combined(tot, 0, '')).all()

    del_user = np.load(os.path.join(G, 'sisa_toy.npz'))['S3_unA_del_user'].tolist()
    idx2, trd2, ted2, tot2 = _toy_loaders(3, del_user)
    s2 = Sisa(Param(3, parallel), 'mf', 3, idx2)
    s2.combiner = c
    torch.manual_seed(42)
    s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, '')
    assert s2.combiner is None
    with pytest.raises(ValueError, match='no combiner'):
        s2.test_combined(tot2, 0, '')
    c2 = s2.fit_combiner(trd2)
    n_after = sum(len(l.dataset) for l in trd2)
    assert int(c2.n.sum()) == n_after < int(c.n.sum())              # no deleted user's pair entered the stats
    dels = set(del_user)
    assert not any(dels & set(l.dataset.users.tolist()) for l in trd2)
    assert np.isfinite(s2.test_combined(tot2, 0, '')).all()
    assert c2.W.tobytes() != c.W.tobytes()


# ---- the torch ops -------------------------------------------------------------------------------------------------------------
def test_torch_ops_equal_the_engine_calls():
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    from ultrare_amd import ops  # noqa: F401  (registers torch.ops.ultrare.*)
    S, d = 4, 16
    tables, (uid, iid, r) = random_case(7001, S, d, seed=5)
    u, i, rt = (torch.from_numpy(a).cuda() for a in (uid, iid, r))
    Us, Vs = [U for U, _ in tables], [V for _, V in tables]
    theta = np.array([0.5, 0.2, -0.1, 0.3, 0.02])
    w = torch.from_numpy(theta).cuda()
    for link in (0, 1):
        got = torch.ops.ultrare.combine_stats(Us, Vs, u, i, rt, link, w)
        assert np.array_equal(got.cpu().numpy(), engine.combine_stats(tables, d, (uid, iid, r), link, theta))
        W = torch.from_numpy(np.stack([theta, theta[::-1].copy()])).cuda()
        gou = torch.from_numpy((np.arange(300) % 2).astype(np.int32)).cuda()
        pred, sse = torch.ops.ultrare.score_weighted(Us, Vs, u, i, rt, link, W, gou)
        want_pred, want_sse = engine.score_weighted(tables, d, u, i, rt, link, W, gou)
        assert torch.equal(pred, want_pred) and torch.equal(sse, want_sse)
        pred0, _ = torch.ops.ultrare.score_weighted(Us, Vs, u, i, rt, link, W, None)
        assert torch.equal(pred0, engine.score_weighted(tables, d, u, i, rt, link, W[:1].contiguous())[0])
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.combine_stats([U.cpu() for U in Us], Vs, u, i, rt, 0, w)
    with pytest.raises(ValueError, match='outside the tables'):
        engine.combine_stats(tables, d, (uid + 300, iid, r), 0, theta)


# ---- 11. scale -------------------------------------------------------------------------------------------------------------------
SCALE_TIME_LIMIT_S = 900        # the child's own limit: building 25 M synthetic ratings on the host is most of it


def test_configs3_shape_one_stats_pass_and_one_scoring_pass_within_memory_bound():
    """32 shards, d = 128, 162,000 users x 60,000 items, 22.5 M pairs: the merged user table and 32 item tables.  Runs in a
    child process under a time limit of its own (_scale_body below), so that a pass that does not come back ends there."""
    import subprocess
    import sys
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), 'scale']
    out = subprocess.run(cmd, timeout=SCALE_TIME_LIMIT_S, capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0 and 'scale ok' in out.stdout


def _scale_body():
    from ultrare_amd import _native as nv
    from ultrare_amd import combine, engine, synth
    S, d = 32, 128
    spec = synth.ML25M
    data = synth.make_dataset(**spec)
    uid, iid, r = data['train']
    assert len(uid) == 22500000
    pairs = engine.PairSet(uid, iid, (r / 5).astype(np.float32))
    gen = torch.Generator(device='cuda').manual_seed(1)
    U = torch.randn(spec['n_user'], d, device='cuda', generator=gen) * d ** -0.25
    tables = [(U, torch.randn(spec['n_item'], d, device='cuda', generator=gen) * d ** -0.25) for _ in range(S)]
    theta = combine.mean_weights(S)
    want_scratch = nv.lib().ure_combine_stats_scratch(pairs.n, S)
    assert 0 < want_scratch < 64 << 20
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    got = engine.combine_stats(tables, d, pairs, 'logistic', theta)
    t1 = time.perf_counter()
    grown = torch.cuda.max_memory_allocated() - base
    assert engine.combine_stats.last_scratch_bytes == want_scratch
    # the scratch, the 596-double result and the weights, plus the caching allocator's block rounding
    assert grown <= want_scratch + (4 << 20), grown
    assert got[0] == pairs.n and np.isfinite(got).all()
    n, loss, g, H = combine.unpack_stats(got, S)
    assert 0 < H[S, S] <= n * 0.25 and (np.linalg.eigvalsh(H) > 0).all()
    W = torch.from_numpy(np.tile(theta, (S, 1))).cuda()
    gou = torch.from_numpy((np.arange(spec['n_user']) % S).astype(np.int32)).cuda()
    pred, sse = engine.score_weighted(tables, d, pairs.uid, pairs.iid, pairs.rating, 'logistic', W, gou)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f'stats pass {1e3 * (t1 - t0):.1f} ms, scoring pass {1e3 * (t2 - t1):.1f} ms (host clock, first calls), scratch {want_scratch / 2**20:.2f} MiB')
    assert torch.isfinite(pred).all() and float(pred.min()) > 0 and float(pred.max()) < 1
    assert np.isfinite(sse.cpu().numpy()).all()
    # a sample of the pairs against the contract
    pick = np.random.RandomState(0).choice(pairs.n, 2000, replace=False)
    P = device_scores(tables, d, uid[pick].astype(np.int32), iid[pick].astype(np.int32))
    want = predict_contract(P, 1, np.tile(theta, (len(pick), 1)))
    assert _ulps(pred.cpu().numpy()[pick], want).max() <= 1.0
    print('scale ok')


if __name__ == '__main__':
    import sys
    assert sys.argv[1:] == ['scale']
    _scale_body()
