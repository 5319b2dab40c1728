"""Attribute unlearning on the device (-m gpu): csrc/mmd.hip held to the numpy contract of ultrare_amd/attr_unlearn.py under
the bounds that module derives (never tuned here), the bitwise guarantees (streams, want_grad, unselected memory), rbk,
the fine-tune loop against the contract and against the reference's float32 loop of tests/golden/attr_toy.npz,
Sisa.attribute_unlearn on a 3-shard toy ensemble, the memory ceiling and the torch ops."""
import os

import numpy as np
import pytest
import torch

from ultrare_amd import attr_unlearn as au

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071
U32 = 2.0 ** -24
PLANTED_LR = 4.0            # chosen with attribute_unlearn_ref: its own dis falls at each of the 10 steps (at 16.0 it does not)


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'attr_toy.npz')), np.load(os.path.join(G, 'kmeans_toy.npz'))['X'].astype(np.float32)


def _planted_table(x, ld, seed, fill=float('nan')):
    """(host table [n_tab, ld] holding the rows of x at an unsorted, non-contiguous selection and `fill` everywhere else --
    the unselected rows and the padding columns d .. ld - 1 --, rows)."""
    m, d = x.shape
    rng = np.random.default_rng(seed)
    n_tab = 2 * m + 7
    rows = rng.permutation(n_tab)[:m]
    W = np.full((n_tab, ld), fill, dtype=np.float32)
    W[rows, :d] = x
    return W, rows


def _device_eval(W, rows, n1, d, kernel_mul, kernel_num, fix_sigma, want_grad=True, stream=None):
    from ultrare_amd import engine
    Wt = W if torch.is_tensor(W) else torch.from_numpy(W).cuda()
    groups = engine.GroupRows(rows[:n1], rows[n1:], Wt.shape[0], Wt.device)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    X = Wt[:, :d]
    bw = engine.mmd_bandwidth(X, groups, fix_sigma, stream=stream)
    sums, grad = engine.mmd_loss_grad(X, groups, bw, kernel_mul, kernel_num, want_grad=want_grad, stream=stream)
    if stream is not None:
        stream.synchronize()
    return engine.mmd_loss_of(sums, groups), sums, grad, bw


def _check_against_contract(x, n1, kernel_mul, kernel_num, fix_sigma, seed, tag):
    from ultrare_amd import _native as nv
    m, d = x.shape
    ld = d + 3
    W, rows = _planted_table(x, ld, seed)
    loss, sums, grad, bw = _device_eval(W, rows, n1, d, kernel_mul, kernel_num, fix_sigma)
    want_loss, want_grad, want_bw, bound_loss, bound_grad = au.mmd_ref(W[:, :d], rows, n1, kernel_mul, kernel_num, fix_sigma)
    err = abs(float(loss) - want_loss)
    ratio = float((np.abs(grad.cpu().numpy().astype(np.float64) - want_grad) / bound_grad).max())
    print(f'{tag}: loss error {err:.3g} (bound {bound_loss:.3g}), gradient error / bound max {ratio:.3g}, splits {nv.lib().ure_mmd_splits(m, d)}')
    assert abs(float(bw) - want_bw) <= 1e-12 * want_bw
    assert err <= bound_loss
    assert ratio <= 1.0
    assert 0 < nv.lib().ure_mmd_scratch(m, d) <= 64 * m * d * 4 + 2 ** 20


# ---- 1. value and gradient against the contract ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(5))
def test_fixture_cases_match_the_contract_and_the_reference(gold, case):
    g, X = gold
    n1, n2, d = (int(v) for v in g['cases'][case])
    _check_against_contract(X[:n1 + n2, :d], n1, 2.0, 5, None, case, f'fixture case {case}')
    # the reference's own float32 numbers, through the public mmd_loss on contiguous tensors
    from ultrare_amd.method import utils
    src, tgt = torch.from_numpy(X[:n1, :d].copy()).cuda(), torch.from_numpy(X[n1:n1 + n2, :d].copy()).cuda()
    loss, gs, gt = utils.mmd_loss(src, tgt, want_grad=True)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.is_cuda
    _, _, _, bound_loss, bound_grad = au.mmd_ref(X[:, :d], np.arange(n1 + n2), n1)
    assert abs(float(loss) - float(g[f'loss_{case}'])) <= 2 * bound_loss            # (each side within one bound of the contract)
    got = torch.cat([gs, gt]).cpu().numpy().astype(np.float64)
    assert (np.abs(got - g[f'grad_{case}']) <= 2 * bound_grad).all()
    assert torch.equal(utils.mmd_loss(src, tgt), loss)


SHAPES = [(63, 1), (64, 64), (65, 64), (1, 200), (700, 900)]


@pytest.mark.parametrize('d', [1, 5, 16, 17, 32, 33, 64, 128])       # (33 and 64: both ends of the DQ = 4 instantiation, 33 <= d <= 64)
@pytest.mark.parametrize('shape', SHAPES)
def test_synthetic_crossings_match_the_contract(d, shape):
    n1, n2 = shape
    rng = np.random.default_rng(1000 * d + n1)
    x = (0.5 * rng.normal(size=(n1 + n2, d))).astype(np.float32)
    x[n1:] += np.float32(0.25)
    for kernel_mul, kernel_num in ((2.0, 5), (1.5, 1), (2.0, 16)):
        for fix_sigma in (None, 0.75 * d):
            _check_against_contract(x, n1, kernel_mul, kernel_num, fix_sigma, d + n1, f'd={d} {shape} mul={kernel_mul} num={kernel_num} sigma={fix_sigma}')


def test_the_tested_shapes_run_with_and_without_a_column_split():
    from ultrare_amd import _native as nv
    splits = {nv.lib().ure_mmd_splits(n1 + n2, 16) for n1, n2 in SHAPES}
    assert 1 in splits and max(splits) > 1, splits
    assert nv.lib().ure_mmd_splits(63 + 1, 16) == 1 and nv.lib().ure_mmd_splits(700 + 900, 16) > 1


# ---- 2. bandwidth and u2u -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,d', [((1, 1), 16), ((5, 7), 16), ((65, 64), 5), ((700, 900), 128), ((300, 3000), 17)])
def test_bandwidth_and_u2u_match_the_contract(shape, d):
    from ultrare_amd import engine
    n1, n2 = shape
    rng = np.random.default_rng(d + n1)
    x = (rng.normal(size=(n1 + n2, d)) + 3.0).astype(np.float32)          # (a mean well away from zero)
    W, rows = _planted_table(x, d + 5, n2)
    Wt = torch.from_numpy(W).cuda()
    groups = engine.GroupRows(rows[:n1], rows[n1:], Wt.shape[0], Wt.device)
    bw = float(engine.mmd_bandwidth(Wt[:, :d], groups))
    want_bw = au.bandwidth_ref(x.astype(np.float64))
    assert abs(bw - want_bw) <= 1e-12 * want_bw
    assert float(engine.mmd_bandwidth(Wt[:, :d], groups, fix_sigma=2.5)) == 2.5
    value, grad = engine.u2u_loss_grad(Wt[:, :d], groups)
    want, want_grad, bound_value, bound_grad = au.u2u_ref(W[:, :d], rows, n1)
    print(f'u2u {shape} d={d}: value error {abs(float(value) - want):.3g} (bound {bound_value:.3g})')
    assert abs(float(value) - want) <= bound_value
    assert (np.abs(grad.cpu().numpy().astype(np.float64) - want_grad) <= bound_grad).all()
    value2, none = engine.u2u_loss_grad(Wt[:, :d], groups, want_grad=False)
    assert none is None and torch.equal(value2, value)


def test_u2u_matches_the_reference_buildlap_value(gold):
    from ultrare_amd import engine
    g, X = gold
    n1, n2, d = (int(v) for v in g['u2u_shape'])
    Xt = torch.from_numpy(X[:, :d].copy()).cuda()
    value, _ = engine.u2u_loss_grad(Xt, engine.GroupRows(np.arange(n1), np.arange(n1, n1 + n2), len(X)))
    assert abs(float(value) - float(g['u2u_value'])) <= 1e-5 * float(g['u2u_value'])


def test_all_rows_equal_is_refused():
    from ultrare_amd.method import utils
    same = torch.ones(4, 8, device='cuda')
    with pytest.raises(ValueError, match='bandwidth'):
        utils.mmd_loss(same[:2], same[2:])
    assert np.isfinite(float(utils.mmd_loss(same[:2], same[2:], fix_sigma=1.0)))


# ---- 3. bitwise guarantees ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,d', [((65, 64), 17), ((700, 900), 32)])
def test_streams_want_grad_and_unselected_memory_change_no_byte(shape, d):
    n1, n2 = shape
    rng = np.random.default_rng(7)
    x = rng.normal(size=(n1 + n2, d)).astype(np.float32)
    W, rows = _planted_table(x, d + 4, 3)
    Wt = torch.from_numpy(W).cuda()
    _, sums, grad, bw = _device_eval(Wt, rows, n1, d, 2.0, 5, None)
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        _, s2, g2, b2 = _device_eval(Wt, rows, n1, d, 2.0, 5, None, stream=stream)
        assert torch.equal(s2, sums) and torch.equal(g2, grad) and torch.equal(b2, bw)
    _, s3, g3, _ = _device_eval(Wt, rows, n1, d, 2.0, 5, None, want_grad=False)
    assert g3 is None and torch.equal(s3, sums)
    # the unselected rows and the padding columns hold NaN above; any other content gives the same bytes
    W7, rows7 = _planted_table(x, d + 4, 3, fill=7.0)
    assert np.array_equal(rows7, rows) and np.isnan(W).any() and not np.isnan(W7).any()
    _, s4, g4, b4 = _device_eval(W7, rows, n1, d, 2.0, 5, None)
    assert torch.equal(s4, sums) and torch.equal(g4, grad) and torch.equal(b4, bw)
    assert torch.isfinite(grad).all() and torch.isfinite(sums).all()


# ---- 4. rbk ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel_num', [5, 16])
def test_rbk_is_symmetric_and_reproduces_mmd_loss(gold, kernel_num):
    from ultrare_amd.method import utils
    X = gold[1]
    n1, n2, d = 130, 170, 16
    src, tgt = torch.from_numpy(X[:n1, :d].copy()).cuda(), torch.from_numpy(X[n1:n1 + n2, :d].copy()).cuda()
    K = utils.rbk(src, tgt, kernel_num=kernel_num)
    assert K.shape == (n1 + n2, n1 + n2) and K.dtype == torch.float32
    assert torch.equal(K, K.T.contiguous())
    assert torch.equal(torch.diagonal(K), torch.full((n1 + n2,), float(kernel_num), device='cuda'))
    K64 = K.double()
    means = K64[:n1, :n1].mean() + K64[n1:, n1:].mean() - K64[:n1, n1:].mean() - K64[n1:, :n1].mean()
    loss = utils.mmd_loss(src, tgt, kernel_num=kernel_num)
    bound_loss = au.mmd_ref(X[:, :d], np.arange(n1 + n2), n1, 2.0, kernel_num)[3]
    assert abs(float(means) - float(loss)) <= bound_loss
    want = au.kernel_matrix_ref(X[:n1 + n2, :d].astype(np.float64), au.bandwidth_ref(X[:n1 + n2, :d].astype(np.float64)), 2.0, kernel_num)
    assert np.abs(K.cpu().numpy() - want).max() <= bound_loss / 4


def test_rbk_refuses_more_than_8192_rows():
    from ultrare_amd.method import utils
    a, b = torch.zeros(5000, 4, device='cuda'), torch.ones(3193, 4, device='cuda')
    with pytest.raises(ValueError, match='mmd_loss'):
        utils.rbk(a, b)
    assert utils.rbk(a[:100], b[:100]).shape == (200, 200)


# ---- 5. attribute_unlearn ---------------------------------------------------------------------------------------------------------
def _toy_model(X, d=16):
    from ultrare_amd.method.utils import MF
    rng = np.random.default_rng(11)
    return MF.from_tables(torch.from_numpy(X[:, :d].copy()).cuda(), torch.from_numpy(rng.normal(size=(50, d)).astype(np.float32)).cuda())


def test_one_step_matches_the_contract(gold):
    from ultrare_amd.method import utils
    g, X = gold
    n1, n2, d = (int(v) for v in g['cases'][0])
    id1, id2 = np.arange(n1), np.arange(n1, n1 + n2)
    lr, eta = 8.0, 1.5
    model = _toy_model(X)
    log = utils.attribute_unlearn(model, id1, id2, 'd2d', eta=eta, alpha=0.0, lr=lr, steps=1)
    want, want_log = au.attribute_unlearn_ref(X[:, :d], id1, id2, 'd2d', eta, 0.0, lr, 1)
    bound_loss, bound_grad = au.mmd_ref(X[:, :d], np.arange(n1 + n2), n1)[3:]
    got = model.user_mat.weight.detach().cpu().numpy().astype(np.float64)
    tol = lr * eta * bound_grad + 2 * U32 * np.abs(want[:n1 + n2])
    err = np.abs(got[:n1 + n2] - want[:n1 + n2])
    print(f'one step: error / tolerance max {(err / tol).max():.3g}, moved {np.abs(want - X[:, :d]).max():.3g}')
    assert (err <= tol).all()
    assert np.array_equal(got[n1 + n2:], X[n1 + n2:, :d].astype(np.float64))
    assert len(log['dis']) == 2 and abs(log['dis'][0] - want_log['dis'][0]) <= bound_loss and log['reg'][0] == 0.0
    assert abs(log['bandwidth'][0] - want_log['bandwidth'][0]) <= 1e-12 * want_log['bandwidth'][0]


def test_three_steps_stay_as_close_to_the_contract_as_the_reference_loop(gold):
    from ultrare_amd.method import utils
    g, X = gold
    n1, n2, d = (int(v) for v in g['cases'][0])
    id1, id2 = np.arange(n1), np.arange(n1, n1 + n2)
    kw = dict(eta=float(g['loop_eta']), alpha=float(g['loop_alpha']), lr=float(g['loop_lr']), steps=int(g['loop_steps']))
    model = _toy_model(X)
    utils.attribute_unlearn(model, id1, id2, 'd2d', **kw)
    want, _ = au.attribute_unlearn_ref(X[:, :d], id1, id2, 'd2d', **kw)
    got = model.user_mat.weight.detach().cpu().numpy().astype(np.float64)[:n1 + n2]
    dist_device = np.abs(got - want[:n1 + n2]).max()
    dist_reference = np.abs(g['loop_rows'].astype(np.float64) - want[:n1 + n2]).max()
    print(f'three steps: device vs contract {dist_device:.3g}, reference float32 vs contract {dist_reference:.3g}')
    assert dist_device <= 4 * dist_reference


@pytest.mark.parametrize('var', ['d2d', 'u2u'])
def test_fine_tune_touches_only_the_groups_and_is_reproducible(gold, var):
    from ultrare_amd.method import utils
    X = gold[1]
    n1, n2, d = 130, 170, 16
    rng = np.random.default_rng(2)
    pick = rng.permutation(len(X))[:n1 + n2]
    id1, id2 = pick[:n1], pick[n1:]
    start = X[:, :d].copy()
    start[id2] += np.float32(0.5)                                 # the planted attribute: one group shifted in every feature
    lr = PLANTED_LR if var == 'd2d' else 3e-4
    want_log = au.attribute_unlearn_ref(start, id1, id2, var, 1.0, 0.05, lr, 10)[1]
    assert (np.diff(want_log['dis']) < 0).all()                   # the contract's own dis falls at every step at this lr
    tables, logs = [], []
    for _ in range(2):
        model = _toy_model(start)
        V0 = model.item_mat.weight.detach().clone()
        logs.append(utils.attribute_unlearn(model, id1, id2, var, eta=1.0, alpha=0.05, lr=lr, steps=10))
        tables.append(model.user_mat.weight.detach().clone())
        assert torch.equal(model.item_mat.weight.detach(), V0)
    assert torch.equal(tables[0], tables[1])
    assert all(np.array_equal(logs[0][k], logs[1][k], equal_nan=True) for k in ('dis', 'reg', 'bandwidth'))
    log = logs[0]
    assert len(log['dis']) == len(log['reg']) == len(log['bandwidth']) == 11
    assert (np.diff(log['dis']) < 0).all(), log['dis']
    assert log['reg'][0] == 0.0 and log['reg'][1] > 0
    assert np.allclose(log['dis'], want_log['dis'], rtol=1e-4)
    got = tables[0].cpu().numpy()
    outside = np.setdiff1d(np.arange(len(X)), pick)
    assert np.array_equal(got[outside], start[outside])
    assert not np.array_equal(got[pick], start[pick])


# ---- 6. Sisa ------------------------------------------------------------------------------------------------------------------------
class Param:
    def __init__(self):
        self.k, self.lam, self.seed, self.batch = 16, 0.1, 42, 3000
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, 3
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, True


def test_sisa_attribute_unlearn_moves_own_shard_rows_only():
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import MF, baseTest
    from ultrare_amd.read import RatingData, loadData, readRating
    g = np.load(os.path.join(G, 'sisa_toy.npz'))
    U = torch.from_numpy(g['S3_learn_Umerged']).cuda()
    groups = [g[f'S3_index{i}'].tolist() for i in range(3)]
    sisa = Sisa(Param(), 'mf', 3, groups)
    sisa.model_list = [MF.from_tables(U, torch.from_numpy(g[f'S3_learn_V{i}']).cuda()) for i in range(3)]
    sisa.combiner = object()
    te, _ = readRating(TEST, N_USER, 5, [], [], 3, groups)
    tot = loadData(RatingData(np.hstack(te)), 3000, 24, False)
    before = U.clone()
    V_before = [m.item_mat.weight.detach().clone() for m in sisa.model_list]
    # id1 from every shard, id2 from shards 0 and 1 only: shard 2 has an empty side
    id1 = groups[0][:40] + groups[1][:30] + groups[2][:20]
    id2 = groups[0][40:90] + groups[1][30:75]
    logs = sisa.attribute_unlearn(id1, id2, var='d2d', lr=4.0, steps=3, alpha=0.01)
    assert len(logs) == 3 and 'skipped' in logs[2] and logs[2]['rows'] == (20, 0)
    assert logs[0]['rows'] == (40, 50) and logs[1]['rows'] == (30, 45) and len(logs[0]['dis']) == 4
    assert sisa.combiner is None
    after = sisa.model_list[0].user_mat.weight.detach()
    assert all(m.user_mat.weight.data_ptr() == after.data_ptr() for m in sisa.model_list)
    changed = set(torch.nonzero((after != before).any(dim=1)).reshape(-1).tolist())
    own = (set(groups[0]) | set(groups[1])) & (set(id1) | set(id2))
    assert changed and changed <= own and not changed & set(groups[2])
    assert len(changed) > len(own) // 2
    for m, V0 in zip(sisa.model_list, V_before):
        assert torch.equal(m.item_mat.weight.detach(), V0)
    sisa.test(tot, 0, '')
    rmse, ndcg, hr = baseTest(tot, sisa.model_list)
    assert sisa.log0 == {'total_rmse': rmse, 'total_ndcg': ndcg, 'total_hr': hr}
    from ultrare_amd.method import utils
    for got, want in zip(sisa.recommend(np.arange(8), 5), utils.recommend(sisa.model_list, np.arange(8), 5)):
        assert torch.equal(got, want)


# ---- 7. memory and the torch ops ------------------------------------------------------------------------------------------------------
def test_a_value_and_gradient_call_stays_far_below_the_matrix():
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    m, d = 8192, 32
    X = torch.randn(m, d, device='cuda')
    groups = engine.GroupRows.leading(4096, 4096, X.device)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    bw = engine.mmd_bandwidth(X, groups)
    sums, grad = engine.mmd_loss_grad(X, groups, bw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f'm = {m}, d = {d}: peak {peak / 2 ** 20:.1f} MiB over the inputs (the matrix alone: 256 MiB), splits {nv.lib().ure_mmd_splits(m, d)}')
    assert peak < 64 * 2 ** 20
    assert 0 < nv.lib().ure_mmd_scratch(m, d) <= 64 * m * d * 4 + 2 ** 20
    assert torch.isfinite(grad).all() and torch.isfinite(sums).all()


def test_torch_ops_equal_the_engine_calls():
    import ultrare_amd.ops  # noqa: F401
    rng = np.random.default_rng(3)
    x = rng.normal(size=(150, 17)).astype(np.float32)
    W, rows = _planted_table(x, 20, 5)
    Wt = torch.from_numpy(W).cuda()
    rows_t = torch.from_numpy(rows.astype(np.int32)).cuda()
    _, sums, grad, bw = _device_eval(Wt, rows, 60, 17, 1.5, 3, None)
    s2, g2, b2 = torch.ops.ultrare.mmd_grad(Wt[:, :17], rows_t, 60, 1.5, 3, None)
    assert torch.equal(s2, sums) and torch.equal(g2, grad) and torch.equal(b2, bw)
    from ultrare_amd import engine
    groups = engine.GroupRows(rows[:60], rows[60:], Wt.shape[0], Wt.device)
    value, ug = engine.u2u_loss_grad(Wt[:, :17], groups)
    v2, ug2 = torch.ops.ultrare.u2u_grad(Wt[:, :17], rows_t, 60)
    assert torch.equal(v2, value) and torch.equal(ug2, ug)
