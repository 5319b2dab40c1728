"""Entropic OT grouping, host side (-m "not gpu"): ure_ot_sinkhorn rejects every bad argument before any HIP call, its
scratch follows its formula, ot_cluster(solver=...) refuses bad settings before device work, and the numpy restatement of
the solver's contract (POT's sinkhorn_log with uniform marginals), which the GPU tests hold the kernels to, agrees with an
independent plain-scaling Sinkhorn where that form is stable.  Nothing here initialises HIP."""
import ctypes
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def lse(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def sinkhorn_contract(M, reg, num_iter_max=1000, stop_thr=1e-9):
    """The contract: M [n, k] (the transpose of ure_ot_cost's [k, n] matrix), all arithmetic in float64.
    -> (u [n], v [k], label [n], iters, err)."""
    n, k = M.shape
    Mr = -M.astype(np.float64) / reg
    loga, logb = np.log(np.full(n, 1.0 / n)), np.log(np.full(k, 1.0 / k))
    u, v, iters, err = np.zeros(n), np.zeros(k), num_iter_max, np.nan
    for ii in range(num_iter_max):
        v = logb - lse(Mr + u[:, None], 0)
        u = loga - lse(Mr + v[None, :], 1)
        if ii % 10 == 0:
            err = np.linalg.norm(np.exp(Mr + u[:, None] + v[None, :]).sum(0) - np.exp(logb))
            if err < stop_thr:
                iters = ii + 1
                break
    label = np.argmax(Mr + v[None, :], axis=1)
    return u, v, label, iters, err


def ot_cluster_contract(X, k, max_iters=10, reg=1e-3, num_iter_max=1000, stop_thr=1e-9):
    """utils.py:628-656 with the contract in place of ot.emd; the centroids drawn from numpy's global generator.
    -> (inertia, label, rounds, [(iters, err) per round])."""
    n, _ = X.shape
    centroid = X[np.random.choice(n, size=k, replace=False)]
    stats = []
    for rnd in range(max_iters):
        dist = ((X - centroid[:, np.newaxis]) ** 2).sum(axis=2)
        inertia = np.min(dist, axis=0).sum()
        _, _, label, iters, err = sinkhorn_contract(dist.T, reg, num_iter_max, stop_thr)
        stats.append((iters, err))
        new_centroid = np.array([X[label == i].mean(axis=0) for i in range(k)])
        if np.allclose(centroid, new_centroid):
            break
        centroid = new_centroid
    return inertia, label, rnd + 1, stats


@pytest.fixture(scope='session')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


FAKE = ctypes.c_void_p(0x1000)                         # never dereferenced: every check fails before the device is touched


def _call(nv, n=100, k=4, reg=0.5, num_iter_max=10, stop_thr=1e-9, scratch_bytes=None, dist=True, v=True, label=True, scratch=True,
          host_out=True):
    L = nv.lib()
    if scratch_bytes is None:
        scratch_bytes = max(L.ure_ot_sinkhorn_scratch(n, k), 0)
    iters, err = ctypes.c_int32(-7), ctypes.c_double(-7.0)
    rc = L.ure_ot_sinkhorn(FAKE if dist else None, n, k, reg, num_iter_max, stop_thr, None, FAKE if v else None, FAKE if label else None, None,
                           FAKE if scratch else None, scratch_bytes, ctypes.byref(iters) if host_out else None,
                           ctypes.byref(err) if host_out else None, None)
    assert iters.value == -7 and err.value == -7.0            # nothing written on a refused call
    return rc


@pytest.mark.parametrize('kw,word', [({'dist': False}, 'dist && v && label && scratch && iters && err'),
                                     ({'v': False}, 'dist && v && label'), ({'label': False}, 'dist && v && label'),
                                     ({'scratch': False}, 'scratch'), ({'host_out': False}, 'iters && err'),
                                     ({'n': 0, 'scratch_bytes': 1 << 20}, 'n >= 1'), ({'n': 1 << 31, 'scratch_bytes': 1 << 40}, 'n <= INT32_MAX'),
                                     ({'k': 0, 'scratch_bytes': 1 << 20}, 'k >= 1'), ({'k': 1025, 'scratch_bytes': 1 << 30}, 'k <= kSinkhornMaxK'),
                                     ({'reg': 0.0}, 'reg > 0'), ({'reg': -1.0}, 'reg > 0'), ({'reg': float('nan')}, 'reg > 0'),
                                     ({'reg': float('inf')}, 'std::isfinite(reg)'),
                                     ({'num_iter_max': 0}, 'num_iter_max >= 1'), ({'num_iter_max': -3}, 'num_iter_max >= 1'),
                                     ({'stop_thr': -1e-9}, 'stop_thr >= 0'), ({'stop_thr': float('nan')}, 'stop_thr >= 0'),
                                     ({'scratch_bytes': 0}, 'scratch_bytes >= ure_ot_sinkhorn_scratch'),
                                     ({'n': 1000, 'k': 7, 'scratch_bytes': 1000 * 8}, 'scratch_bytes >= ure_ot_sinkhorn_scratch')])
def test_sinkhorn_rejects_bad_arguments(nv, kw, word):
    assert _call(nv, **kw) == -1
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


def test_sinkhorn_scratch_formula(nv):
    L = nv.lib()
    al = lambda x: (x + 255) // 256 * 256
    for n, k in [(1, 1), (7, 3), (255, 33), (256, 5), (257, 5), (6040, 16), (162000, 32), (4096, 1024), (1000000, 64), ((1 << 31) - 1, 1024)]:
        B = -(-n // 256)
        want = 256 + al(2 * k * 8) + al(8 * n) + 2 * al(8 * B * k)
        assert L.ure_ot_sinkhorn_scratch(n, k) == want, (n, k)
    for n, k in [(0, 4), (-1, 4), (1 << 31, 4), (10, 0), (10, 1025)]:
        assert L.ure_ot_sinkhorn_scratch(n, k) == -1, (n, k)


@pytest.mark.parametrize('kw', [{'solver': 'bogus'}, {'solver': None}, {'solver': 'sinkhorn', 'reg': 0}, {'solver': 'sinkhorn', 'reg': -1e-3},
                                {'solver': 'sinkhorn', 'reg': float('nan')}, {'solver': 'sinkhorn', 'reg': float('inf')},
                                {'solver': 'sinkhorn', 'num_iter_max': 0}, {'solver': 'sinkhorn', 'num_iter_max': 2.5},
                                {'solver': 'sinkhorn', 'stop_thr': -1.0}])
def test_ot_cluster_refuses_bad_settings_before_device_work(nv, kw, monkeypatch):
    from ultrare_amd import engine
    from ultrare_amd.method import utils

    def no_device():
        raise AssertionError('device work started')
    monkeypatch.setattr(engine, '_device', no_device)
    state = np.random.get_state()[1].copy()
    X = np.random.RandomState(0).rand(20, 3).astype(np.float32)
    with pytest.raises(ValueError):
        utils.ot_cluster(X, 3, **kw)
    assert np.array_equal(np.random.get_state()[1], state)            # not even the centroid draw happened


def test_ot_cluster_refuses_too_many_clusters_for_sinkhorn(nv, monkeypatch):
    from ultrare_amd import engine
    from ultrare_amd.method import utils
    monkeypatch.setattr(engine, '_device', lambda: (_ for _ in ()).throw(AssertionError('device work started')))
    with pytest.raises(ValueError, match='at most 1024'):
        utils.ot_cluster(np.zeros((1100, 2), np.float32), 1025, solver='sinkhorn')


def test_group_rejects_bad_reg_before_device_work(nv, monkeypatch, tmp_path):
    from ultrare_amd import engine
    from ultrare_amd.group import Group
    monkeypatch.setattr(engine, '_device', lambda: (_ for _ in ()).throw(AssertionError('device work started')))
    X = np.random.RandomState(1).rand(30, 4).astype(np.float32)
    with pytest.raises(ValueError, match='reg'):
        Group(None, 'toy', user_mat=X).grouping('toy', 3, 'emb-sinkhorn', verbose=False, data_dir=str(tmp_path), reg=0.0)
    assert not (tmp_path / 'toy' / 'val' / 'emb-sinkhorn3.npy').exists()


def plain_sinkhorn(M, reg, num_iter_max, stop_thr):
    """Sinkhorn in the scaling form (POT's sinkhorn_knopp with uniform marginals), stable only when exp(-M / reg) is."""
    n, k = M.shape
    K = np.exp(-M.astype(np.float64) / reg)
    a, b = np.full(n, 1.0 / n), np.full(k, 1.0 / k)
    u, v, iters, err = np.ones(n), np.ones(k), num_iter_max, np.nan
    for ii in range(num_iter_max):
        v = b / (K.T @ u)
        u = a / (K @ v)
        if ii % 10 == 0:
            err = np.linalg.norm((u[:, None] * K * v[None, :]).sum(0) - b)
            if err < stop_thr:
                iters = ii + 1
                break
    return np.log(u), np.log(v), np.argmax(K * v[None, :], axis=1), iters, err


@pytest.mark.parametrize('case', ['toy_k5', 'toy_k7', 'random'])
def test_contract_agrees_with_plain_scaling_at_large_reg(case):
    if case == 'random':
        M = (np.random.RandomState(3).rand(300, 6) * 4).astype(np.float32)
    else:
        M = np.load(os.path.join(G, 'ot_toy.npz'))[case[-2:] + '_round0_dist']
    reg = 0.25 * float(np.median(M))
    u, v, label, iters, err = sinkhorn_contract(M, reg)
    pu, pv, plabel, piters, perr = plain_sinkhorn(M, reg, 1000, 1e-9)
    assert iters == piters < 1000
    assert err < 1e-9 and perr < 1e-9
    np.testing.assert_allclose(u, pu, rtol=0, atol=1e-9 * np.abs(pu).max())
    np.testing.assert_allclose(v, pv, rtol=0, atol=1e-9 * np.abs(pv).max())
    assert np.array_equal(label, plabel)
    # the plan's marginals hold
    P = np.exp(-M.astype(np.float64) / reg + u[:, None] + v[None, :])
    np.testing.assert_allclose(P.sum(1), 1.0 / len(M), rtol=1e-6)
    np.testing.assert_allclose(P.sum(0), 1.0 / M.shape[1], rtol=1e-6)


def test_contract_reproduces_the_issue_figures_on_the_toy_costs():
    """The first k = 5 cost matrix of the toy set: capped at reg = 1e-3 (the reference's `lam`), converging at 0.05 median(M)."""
    M = np.load(os.path.join(G, 'ot_toy.npz'))['k5_round0_dist']
    _, _, label, iters, err = sinkhorn_contract(M, 1e-3)
    assert iters == 1000 and abs(err - 0.1753) < 1e-3
    assert np.bincount(label).tolist() == [249, 215, 229, 283, 532]
    _, _, label, iters, err = sinkhorn_contract(M, 0.05 * float(np.median(M)))
    assert iters == 81 and err < 1e-9
    assert np.bincount(label).tolist() == [298, 307, 312, 298, 293]
