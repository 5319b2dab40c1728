"""Attribute unlearning, host side (-m "not gpu"): the numpy contract of csrc/mmd.hip (ultrare_amd/attr_unlearn.py) against
the reference's float32 mmd_loss / autograd / buildLap values of tests/golden/attr_toy.npz under the contract's own derived
bounds, the fine-tune loop against the reference's, a finite-difference check of the gradient, every refusal that must come
before any device work, and the new C entry points' argument checks.  Nothing here initialises HIP."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='session')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


@pytest.fixture(scope='module')
def au():
    from ultrare_amd import attr_unlearn
    return attr_unlearn


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(G, 'attr_toy.npz')), np.load(os.path.join(G, 'kmeans_toy.npz'))['X'].astype(np.float32)


# ---- 1. the contract against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(5))
def test_contract_matches_the_reference_under_the_derived_bounds(au, gold, case):
    g, X = gold
    n1, n2, d = (int(v) for v in g['cases'][case])
    loss, grad, bw, bound_loss, bound_grad = au.mmd_ref(X[:, :d], np.arange(n1 + n2), n1)
    err_loss = abs(loss - float(g[f'loss_{case}']))
    ratio = np.abs(grad - g[f'grad_{case}'].astype(np.float64)) / bound_grad
    print(f'case {case}: loss error {err_loss:.3g} (bound {bound_loss:.3g}), gradient error / bound max {ratio.max():.3g}')
    assert err_loss <= bound_loss
    assert ratio.max() <= 1.0
    assert grad.shape == (n1 + n2, d) and bw > 0


def test_contract_catches_a_dropped_column_and_a_wrong_block_weight(au, gold):
    """The bounds are tight enough to tell: the gradient without one column's term, or with S x T weighted as S x S, fails."""
    g, X = gold
    n1, n2, d = (int(v) for v in g['cases'][0])
    x = X[:n1 + n2, :d].astype(np.float64)
    loss, grad, bw, _, bound_grad = au.mmd_ref(x, np.arange(n1 + n2), n1)
    bws = au.bandwidths(bw, 2.0, 5)
    L = ((x[0] - x) ** 2).sum(-1)
    w = sum((-2.0 / b) * np.exp(-L / b) for b in bws)
    j = n1 + 3
    dropped = grad[0] - (-2.0 / (n1 * n2)) * w[j] * (x[0] - x[j])
    assert (np.abs(dropped - grad[0]) > bound_grad[0]).any()
    wrong = grad[0] - ((-2.0 / (n1 * n2)) - 2.0 / (n1 * n1)) * w[j] * (x[0] - x[j])
    assert (np.abs(wrong - grad[0]) > bound_grad[0]).any()


def test_bandwidth_closed_form_is_the_explicit_sum(au, gold):
    X = gold[1][:97, :16].astype(np.float64)
    explicit = ((X[:, None, :] - X[None, :, :]) ** 2).sum() / (97 * 97 - 97)
    assert abs(au.bandwidth_ref(X) - explicit) <= 1e-13 * explicit


def test_u2u_contract_matches_buildlap(au, gold):
    g, X = gold
    n1, n2, d = (int(v) for v in g['u2u_shape'])
    value, grad, bound_value, bound_grad = au.u2u_ref(X[:, :d], np.arange(n1 + n2), n1)
    assert abs(value - float(g['u2u_value'])) <= 1e-5 * abs(value)
    x = X[:n1 + n2, :d].astype(np.float64)
    explicit = sum(((x[i] - x[j]) ** 2).sum() for i in range(n1) for j in range(n1, n1 + n2))
    assert abs(value - explicit) <= 1e-12 * explicit
    want = np.concatenate([2 * (n2 * x[:n1] - x[n1:].sum(0)), 2 * (n1 * x[n1:] - x[:n1].sum(0))])
    assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max()
    assert bound_value > 0 and (bound_grad > 0).all()


def test_contract_gradient_is_the_finite_difference_of_its_loss(au):
    rng = np.random.default_rng(5)
    x = rng.normal(size=(6, 3))
    rows, n1, sigma = np.arange(6), 2, 1.7                     # (the bandwidth held fixed: no gradient flows through it)
    _, grad, _, _, _ = au.mmd_ref(x, rows, n1, 2.0, 5, sigma)
    h = 1e-5
    for i in range(6):
        for f in range(3):
            up, dn = x.copy(), x.copy()
            up[i, f] += h
            dn[i, f] -= h
            fd = (au.mmd_ref(up, rows, n1, 2.0, 5, sigma)[0] - au.mmd_ref(dn, rows, n1, 2.0, 5, sigma)[0]) / (2 * h)
            assert abs(fd - grad[i, f]) <= 1e-6 * np.abs(grad).max()


def test_contract_loop_agrees_with_the_reference_loop(au, gold):
    """The float64 loop against the reference's float32 loop: the distance the GPU test's tolerance is built from.  The
    reference rounds every step to float32 (u |U| each) and carries its float32 gradient; three steps of rows of size ~1 stay
    within a few u."""
    g, X = gold
    n1, n2, d = (int(v) for v in g['cases'][0])
    T, log = au.attribute_unlearn_ref(X[:n1 + n2, :d], np.arange(n1), np.arange(n1, n1 + n2), 'd2d', float(g['loop_eta']), float(g['loop_alpha']),
                                      float(g['loop_lr']), int(g['loop_steps']))
    dist = np.abs(T - g['loop_rows'].astype(np.float64)).max()
    moved = np.abs(T - X[:n1 + n2, :d]).max()
    print(f'contract vs reference loop: {dist:.3g}; the loop moved the rows by up to {moved:.3g}')
    assert dist <= 8 * 2.0 ** -24 * np.abs(T).max()
    assert moved > 100 * dist
    assert len(log['dis']) == len(log['reg']) == len(log['bandwidth']) == 4 and log['reg'][0] == 0.0 and log['reg'][1] > 0


# ---- 2. refusals before any device work ----------------------------------------------------------------------------------
def test_argument_checks_raise_value_error(au):
    for bad in (dict(kernel_mul=0.0), dict(kernel_mul=-1.0), dict(kernel_mul=float('nan')), dict(kernel_num=0), dict(kernel_num=17),
                dict(kernel_num=2.5), dict(kernel_num=True), dict(fix_sigma=0.0), dict(fix_sigma=-2.0), dict(fix_sigma=float('inf'))):
        with pytest.raises(ValueError):
            au.check_mmd_args(**bad)
    assert au.check_mmd_args(1.5, 16, 0.25) == (1.5, 16, 0.25)
    for d in (0, 129):
        with pytest.raises(ValueError):
            au.check_width(d)
    with pytest.raises(ValueError):
        au.check_width(16, 8)
    for id1, id2 in (([], [1]), ([1], []), ([1, 2], [2, 3]), ([1, 1], [2]), ([0], [10]), ([-1], [2]), ([0.5], [2])):
        with pytest.raises(ValueError):
            au.check_groups(id1, id2, 10)
    rows, n1, n2 = au.check_groups([4, 2], [9, 0, 1], 10)
    assert rows.dtype == np.int32 and rows.tolist() == [4, 2, 9, 0, 1] and (n1, n2) == (2, 3)
    with pytest.raises(ValueError):
        au.check_var('nor')
    for bad in (dict(eta=float('nan')), dict(alpha=-1.0), dict(lr=float('inf')), dict(steps=-1), dict(steps=1.5)):
        with pytest.raises(ValueError):
            au.check_loop_args(**{**dict(eta=1.0, alpha=0.0, lr=0.1, steps=1), **bad})
    x = np.ones((4, 3))
    with pytest.raises(ValueError):                            # all rows equal: the reference returns NaN
        au.mmd_ref(x, np.arange(4), 2)
    assert np.isfinite(au.mmd_ref(x, np.arange(4), 2, fix_sigma=1.0)[0])


def test_public_surface_refuses_on_the_host():
    """utils.attribute_unlearn / Sisa.attribute_unlearn / rbk check their arguments before they look at a device."""
    import torch
    from ultrare_amd.method import utils
    from ultrare_amd.method.sisa import Sisa
    model = utils.MF.from_tables(torch.zeros(10, 4), torch.zeros(6, 4))
    for kw in (dict(id1=[1, 2], id2=[2, 3]), dict(id1=[], id2=[3]), dict(id1=[1], id2=[10]), dict(id1=[1, 1], id2=[3]),
               dict(id1=[1], id2=[3], var='nor'), dict(id1=[1], id2=[3], kernel_num=0), dict(id1=[1], id2=[3], steps=-1)):
        with pytest.raises(ValueError):
            utils.attribute_unlearn(model, **kw)
    with pytest.raises(ValueError, match='mmd_loss'):
        utils.rbk(torch.zeros(5000, 4), torch.zeros(3193, 4))
    s = Sisa.__new__(Sisa)
    s.model_list, s.n_user, s.n_group, s.group_index = [model], 10, 1, [list(range(10))]
    for kw in (dict(id1=[1, 2], id2=[2, 3]), dict(id1=[1], id2=[3], var='x'), dict(id1=[1], id2=[11])):
        with pytest.raises(ValueError):
            s.attribute_unlearn(**kw)
    s.model_list = []
    with pytest.raises(ValueError):
        s.attribute_unlearn([1], [3])


# ---- 3. the C entry points -----------------------------------------------------------------------------------------------
def test_new_symbols_exist_and_the_abi_number_is_unchanged(nv):
    L = nv.lib()
    for name in ('ure_mmd_scratch', 'ure_mmd_splits', 'ure_mmd_bandwidth', 'ure_mmd_loss_grad', 'ure_u2u_loss_grad', 'ure_mmd_matrix'):
        assert name in nv.EXPORTS and hasattr(L, name)
    assert L.ure_abi_version() == 15 == nv.ABI_VERSION


def test_scratch_function_refuses_and_stays_linear(nv):
    L = nv.lib()
    for m, d in ((1, 16), (0, 16), (-5, 16), (100, 0), (100, 129), (2 ** 31 - 64, 16), (2 ** 31, 16)):
        assert L.ure_mmd_scratch(m, d) == -1 and L.ure_mmd_splits(m, d) == -1
    seen = set()
    for m in (2, 63, 64, 65, 300, 1508, 6040, 8192, 162000, 2 ** 31 - 65):
        for d in (1, 5, 16, 17, 32, 128):
            nbytes, splits = L.ure_mmd_scratch(m, d), L.ure_mmd_splits(m, d)
            assert 0 < nbytes <= 64 * m * d * 4 + 2 ** 20
            assert 1 <= splits <= (m + 63) // 64
            assert nbytes >= splits * m * d * 8
            seen.add(splits > 1)
    assert seen == {False, True}
    assert L.ure_mmd_splits(6040, 32) > 1 and L.ure_mmd_splits(162000, 128) == 1


def test_calls_refuse_bad_arguments_without_touching_the_device(nv):
    L = nv.lib()
    one = 8                                                     # (any non-null address: the checks come first)
    assert L.ure_mmd_bandwidth(None, 16, 16, one, 1, 1, one, one, 1 << 30, None) == -1
    assert L.ure_mmd_bandwidth(one, 8, 16, one, 1, 1, one, one, 1 << 30, None) == -1          # ld < d
    assert L.ure_mmd_bandwidth(one, 16, 16, one, 0, 2, one, one, 1 << 30, None) == -1         # an empty group
    assert L.ure_mmd_bandwidth(one, 16, 16, one, 1, 1, one, one, 8, None) == -1               # scratch too small
    assert L.ure_mmd_loss_grad(one, 16, 16, one, 1, 1, 2.0, 0, one, one, None, one, 1 << 30, None) == -1
    assert L.ure_mmd_loss_grad(one, 16, 16, one, 1, 1, 2.0, 17, one, one, None, one, 1 << 30, None) == -1
    assert L.ure_mmd_loss_grad(one, 16, 16, one, 1, 1, 0.0, 5, one, one, None, one, 1 << 30, None) == -1
    assert L.ure_mmd_loss_grad(one, 16, 129, one, 1, 1, 2.0, 5, one, one, None, one, 1 << 30, None) == -1
    assert L.ure_u2u_loss_grad(one, 16, 16, one, 1, 1, None, None, one, 1 << 30, None) == -1
    assert L.ure_mmd_matrix(one, 16, 16, one, 8193, 2.0, 5, one, one, None) == -1
    assert b'argument check failed' in L.ure_last_error()
