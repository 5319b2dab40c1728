"""Entropic OT grouping on the device (csrc/ot_sinkhorn.hip), held to the numpy contract of tests/test_cpu_sinkhorn.py:
the kernel on given cost matrices (converging and capped), bitwise reproducibility, ot_cluster(solver='sinkhorn') end to end
against utils.py:628-656 with the contract as its solver, Group.grouping / Instance.runGroup with 'emb-sinkhorn', the torch
op, and the (162,000, 32) shape with its memory bound."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from test_cpu_sinkhorn import ot_cluster_contract, sinkhorn_contract

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER = 1508


def cost_case(name):
    """[n, k] float32 costs of a named case."""
    if name.startswith('toy'):
        return np.load(os.path.join(G, 'ot_toy.npz'))[name[4:] + '_round0_dist']
    n, k = map(int, name.split('x'))
    return (np.random.RandomState(n * 7 + k).rand(n, k) * 10).astype(np.float32)


def run_device(M, reg, num_iter_max, stop_thr=1e-9):
    from ultrare_amd import engine
    dist = torch.from_numpy(np.ascontiguousarray(M.T)).cuda()
    return engine.ot_sinkhorn(dist, reg, num_iter_max, stop_thr, want_u=True, want_cost_min=True)


def assert_matches_contract(M, reg, num_iter_max, r):
    u, v, label, iters, err = sinkhorn_contract(M, reg, num_iter_max)
    assert r['iters'] == iters
    # both err are sums of n plan entries whose exponents carry ~1e-14 of rounding: below 1e-12 they are rounding noise
    assert abs(r['err'] - err) <= 1e-6 * err + 1e-12, (r['err'], err)
    tol = 1e-6 * float(M.max())
    gu, gv = r['u'].cpu().numpy(), r['v'].cpu().numpy()
    assert np.abs(reg * (gu - u)).max() <= tol
    assert np.abs(reg * (gv - v)).max() <= tol
    logp = -M.astype(np.float64) / reg + v[None, :]
    if M.shape[1] > 1:
        top2 = -np.partition(-logp, 1, axis=1)[:, :2]
        near = top2[:, 0] - top2[:, 1] < 1e-5 * float(M.max()) / reg
    else:
        near = np.zeros(len(M), bool)
    glabel = r['label'].cpu().numpy()
    assert np.array_equal(glabel[~near], label[~near]), int((glabel != label).sum())
    assert np.array_equal(r['cost_min'].cpu().numpy(), M.min(axis=1))
    return iters


CASES = ['1x1', '7x3', '255x33', 'toy_k4', 'toy_k5', 'toy_k7', '6040x16', '20000x128', '4096x1024']


@pytest.mark.parametrize('name', CASES)
def test_kernel_converging_reg_matches_contract(name):
    M = cost_case(name)
    reg = 0.05 * float(np.median(M))
    iters = assert_matches_contract(M, reg, 1000, run_device(M, reg, 1000))
    assert iters < 1000


@pytest.mark.parametrize('name', CASES)
def test_kernel_reference_lam_is_capped_and_matches_contract(name):
    """reg = 1e-3, the reference's `lam`: on these costs the solve runs to its cap (a cap of 30 on the largest shapes keeps the
    numpy side short)."""
    M = cost_case(name)
    cap = 1000 if M.size <= 200000 else 30
    iters = assert_matches_contract(M, 1e-3, cap, run_device(M, 1e-3, cap))
    if M.shape[1] > 1 and len(M) > 1:
        assert iters == cap


def test_two_calls_are_bitwise_identical():
    M = cost_case('20000x128')
    for reg, cap in ((0.05 * float(np.median(M)), 1000), (1e-3, 25)):
        a, b = run_device(M, reg, cap), run_device(M, reg, cap)
        assert a['iters'] == b['iters'] and a['err'] == b['err']
        for key in ('u', 'v', 'label', 'cost_min'):
            assert torch.equal(a[key], b[key]), key


def test_one_cluster_takes_every_point_in_one_iteration():
    M = cost_case('1000x1')
    r = run_device(M, 0.1, 1000)
    assert r['iters'] == 1 and r['err'] < 1e-9
    assert not r['label'].any()


def test_non_finite_marginal_error_is_an_error():
    from ultrare_amd import _native as nv
    with pytest.raises(nv.NativeError, match='not finite'):
        run_device(cost_case('255x33') + 1.0, 1e-300, 50)


def test_torch_op_equals_the_c_call():
    from ultrare_amd import _native as nv
    from ultrare_amd import ops  # noqa: F401  (registers torch.ops.ultrare.*)
    M = cost_case('6040x16')
    reg = 0.05 * float(np.median(M))
    dist = torch.from_numpy(np.ascontiguousarray(M.T)).cuda()
    label, u, v, err, iters = torch.ops.ultrare.ot_sinkhorn(dist, reg, 1000, 1e-9)
    n, k = len(M), M.shape[1]
    L = nv.lib()
    nbytes = L.ure_ot_sinkhorn_scratch(n, k)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    cu, cv = torch.empty(n, dtype=torch.float64, device='cuda'), torch.empty(k, dtype=torch.float64, device='cuda')
    cl = torch.empty(n, dtype=torch.int32, device='cuda')
    ci, ce = ctypes.c_int32(), ctypes.c_double()
    nv.check(L.ure_ot_sinkhorn(nv.ptr(dist), n, k, reg, 1000, 1e-9, nv.ptr(cu), nv.ptr(cv), nv.ptr(cl), None, nv.ptr(scratch), nbytes,
                               ctypes.byref(ci), ctypes.byref(ce), nv.stream_handle()), 'ure_ot_sinkhorn')
    assert torch.equal(label, cl) and torch.equal(u, cu) and torch.equal(v, cv)
    assert iters == ci.value and err == ce.value
    with pytest.raises(nv.NativeError):
        torch.ops.ultrare.ot_sinkhorn(dist.cpu(), reg, 1000, 1e-9)


# ---- ot_cluster end to end -------------------------------------------------------------------------------------------
def _ml1m_X():
    from test_gpu_pins import ot_embedding
    g = np.load(os.path.join(G, 'ot_ml1m.npz'))
    X = ot_embedding(int(g['n']), int(g['d']), int(g['seed']))
    assert float(X.astype(np.float64).sum()) == float(g['X_sum'])
    return X


@pytest.mark.parametrize('data,k', [('toy', 4), ('toy', 5), ('toy', 7), ('ml1m', 5), ('ml1m', 16)])
def test_ot_cluster_sinkhorn_matches_contract_rounds(data, k):
    from ultrare_amd.method.utils import ot_cluster
    X = np.load(os.path.join(G, 'ot_toy.npz'))['X'] if data == 'toy' else _ml1m_X()
    np.random.seed(0)
    inertia, label = ot_cluster(X, k, solver='sinkhorn')
    stats = list(ot_cluster.sinkhorn_stats)
    np.random.seed(0)
    want_inertia, want_label, rounds, want_stats = ot_cluster_contract(X, k)
    assert len(stats) == rounds
    assert [s[0] for s in stats] == [s[0] for s in want_stats]
    assert np.array_equal(label, want_label)
    assert float(inertia) == float(want_inertia)


def test_ot_cluster_empty_cluster_names_the_round():
    """Ten points on two sites and three centroids drawn among them: two centroids coincide, their cost columns are equal,
    and the first maximum leaves the second of them without a point."""
    from ultrare_amd.method.utils import ot_cluster
    X = np.zeros((10, 2), np.float32)
    X[5:] = 1.0
    np.random.seed(1)
    with pytest.raises(ValueError, match='round 0'):
        ot_cluster(X, 3, solver='sinkhorn')


# ---- Group.grouping and runGroup ---------------------------------------------------------------------------------------
def test_group_grouping_sinkhorn_writes_and_rereads_its_cache(tmp_path):
    from ultrare_amd.group import Group
    from ultrare_amd.method.utils import ot_cluster
    X = np.load(os.path.join(G, 'ot_toy.npz'))['X']
    reg = 0.3
    np.random.seed(0)
    res = Group(None, 'toy', user_mat=X).grouping('toy', 5, 'emb-sinkhorn', verbose=False, data_dir=str(tmp_path), reg=reg)
    path = tmp_path / 'toy' / 'val' / 'emb-sinkhorn5.npy'
    assert path.exists()
    np.random.seed(0)
    _, label = ot_cluster(X, 5, solver='sinkhorn', reg=reg)
    assert res == [np.flatnonzero(label == c).tolist() for c in range(5)]
    again = Group(None, 'toy', user_mat=None).grouping('toy', 5, 'emb-sinkhorn', verbose=False, data_dir=str(tmp_path))
    assert again == res
    arr = np.load(path, allow_pickle=True)
    assert arr.dtype == object and [list(x) for x in arr] == res


def test_instance_run_group_emb_sinkhorn(tmp_path):
    from ultrare_amd.config import InsParam, Instance
    data = tmp_path / 'data'
    (data / 'toy').mkdir(parents=True)
    shutil.copy(TRAIN, data / 'toy' / '0_train.csv')
    shutil.copy(TEST, data / 'toy' / '0_test.csv')
    save = tmp_path / 'result'
    torch.manual_seed(42)
    p0 = InsParam('toy', 3, 24, [32], 0, 2, 'rand', data_dir=str(data))
    Instance(p0, save_dir=str(save)).runFull(is_save=True, verbose=0)
    p3 = InsParam('toy', 2, 24, [32], 3, 2, 'rand', data_dir=str(data))
    ins = Instance(p3, save_dir=str(save))
    models = ins.runGroup(is_save=True, learn_type='sisa', group_type='emb-sinkhorn', n_group=3, verbose=0)
    assert len(models) == 3
    g3 = save / '2' / 'rand' / 'toy_g3'
    for f in ('MF_emb-sinkhorn_sisa_learn/log0.npy', 'MF_emb-sinkhorn_sisa_unlearn/log0.npy'):
        assert (g3 / f).exists(), f
    groups = np.load(data / 'toy' / 'val' / 'emb-sinkhorn3.npy', allow_pickle=True)
    assert sorted(u for g in groups for u in g) == list(range(N_USER))


# ---- scale ---------------------------------------------------------------------------------------------------------------
def test_162k_by_32_capped_matches_contract_within_memory_bound():
    from test_gpu_pins import ot_embedding
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    n, k, d = 162000, 32, 128
    X = ot_embedding(n, d, 5)
    rs = np.random.RandomState(0)
    C = X[rs.choice(n, k, replace=False)]
    Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dist = torch.empty(k, n, dtype=torch.float32, device='cuda')
    nv.check(nv.lib().ure_ot_cost(nv.ptr(Xd), nv.ptr(Cd), n, k, d, nv.ptr(dist), nv.stream_handle()), 'ure_ot_cost')
    r = engine.ot_sinkhorn(dist, 1e-3, 50, 1e-9, want_u=True, want_cost_min=True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    # the cost matrix, the scratch and the O(n) outputs, plus up to 1 MiB of the caching allocator's block rounding; a float64
    # [n, k] plan alone would be 41 MB more
    outputs = n * (8 + 4 + 4) + k * 8
    assert grown <= n * k * 4 + nv.lib().ure_ot_sinkhorn_scratch(n, k) + outputs + (1 << 20), grown
    M = dist.cpu().numpy().T
    assert r['iters'] == 50
    assert_matches_contract(M, 1e-3, 50, r)
