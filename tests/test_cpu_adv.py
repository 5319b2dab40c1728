"""Adversarial attribute unlearning without a GPU: the numpy contract (ultrare_amd/adv_unlearn.py) against torch autograd, the claim
the method is offered under (a fresh attacker ends near chance on the planted table), the plants, every refusal, the main.py flags,
and the binding table against the header and the built library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import adv_cases as D
import attack_cases as C
from ultrare_amd import adv_unlearn as V
from ultrare_amd import attack as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -24
TARGETS = [(0.0, 1.0), (0.5, 0.5)]


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


def _rel(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- the contract against autograd ----------------------------------------------------------------------------------------------------
def _autograd(c, target, H):
    """The literal loss in torch float64: row i's own term w_class[f][y_i] * CE(sigmoid(logit_i), target[y_i]) under the set f =
    fold_of[i], the statistics constants; its gradient with respect to x."""
    x = torch.tensor(c['x'].astype(np.float64), requires_grad=True)
    m, d = x.shape
    total, p_all = 0.0, np.zeros(m)
    for f in range(len(c['params'])):
        at = torch.from_numpy(np.flatnonzero(c['fold_of'] == f))
        W1, b1, w2, b2 = (None if v is None else torch.tensor(np.array(v, dtype=np.float64)) for v in A.unpack(c['params'][f], d, H))
        mean, inv = (torch.tensor(c['stats'][f][k].astype(np.float64)) for k in (0, 1))
        z = (x[at] - mean) * inv
        a = z @ W1.T + b1
        logit = a[:, 0] if H == 0 else torch.relu(a) @ w2 + b2
        y = torch.from_numpy(c['y'])[at]
        t = torch.tensor(np.asarray(target, dtype=np.float32).astype(np.float64))[y]
        w = torch.tensor(c['fw'][f, :2].astype(np.float64))[y]
        total = total + (w * torch.nn.functional.binary_cross_entropy_with_logits(logit, t, reduction='none')).sum()
        p_all[at.numpy()] = torch.sigmoid(logit).detach().numpy()
    return torch.autograd.grad(total, x)[0].numpy(), p_all


@pytest.mark.parametrize('H', [0, 1, 8])
@pytest.mark.parametrize('target', TARGETS)
def test_contract_is_autograd_of_the_literal_loss(H, target):
    """Agreement reached (float64 against float64; the two differ in summation order only): at most 5e-16 relative to the largest
    entry of the gradient over the six cases, 2e-16 on p; asserted at 1e-12, as tests/test_cpu_attack.py asserts its 2e-15."""
    c = D.probe(150, 6, H, 3, 10 + H)
    got, p = V.input_grad_ref(c['params'], c['stats'], c['x'], c['y'], c['fold_of'], c['fw'], target, H, dtype=np.float64)
    want, p_want = _autograd(c, target, H)
    print('grad', _rel(got, want), 'p', np.abs(p - p_want).max())
    assert np.abs(want).max() > 1e-3
    assert _rel(got, want) < 1e-12 and np.abs(p - p_want).max() < 1e-12


@pytest.mark.parametrize('H', [0, 7, 64])
def test_float32_contract_follows_the_float64_one(H):
    c = D.probe(300, 17, H, 5, H)
    for target in TARGETS:
        (g32, p32), (g64, p64) = (V.input_grad_ref(c['params'], c['stats'], c['x'], c['y'], c['fold_of'], c['fw'], target, H, dtype=T)
                                  for T in (np.float32, np.float64))
        assert g32.dtype == np.float32 and p32.dtype == np.float32
        print(H, target, _rel(g32, g64), np.abs(p32 - p64).max())
        assert _rel(g32, g64) < 1e-5 and np.abs(p32 - p64).max() < 1e-6
        # the bit-for-bit half: p handed over, the rest pure float32
        again = V.input_grad_ref(c['params'], c['stats'], c['x'], c['y'], c['fold_of'], c['fw'], target, H, dtype=np.float32, p=p32)
        assert again[0].tobytes() == g32.tobytes() and again[1].tobytes() == p32.tobytes()


def test_fold_selection_nan_rows_and_set_zero():
    c = D.probe(40, 5, 4, 3, 1)
    fo = c['fold_of'].copy()
    fo[[3, 17]] = [3, -1]
    g, p = V.input_grad_ref(c['params'], c['stats'], c['x'], c['y'], fo, c['fw'], (0.5, 0.5), 4)
    bad = np.zeros(40, dtype=bool)
    bad[[3, 17]] = True
    assert np.isnan(g[bad]).all() and np.isnan(p[bad]).all() and np.isfinite(g[~bad]).all() and np.isfinite(p[~bad]).all()
    # a position is served by the set that held it out: ure_attack_score's selection
    assert np.array_equal(p[~bad], A.score_ref(c['x'], np.arange(40), c['fold_of'], c['params'], c['stats'], 4)[~bad])
    g0, p0 = V.input_grad_ref(c['params'], c['stats'], c['x'], c['y'], None, c['fw'], (0.5, 0.5), 4)
    one = V.input_grad_ref(c['params'][:1], c['stats'][:1], c['x'], c['y'], np.zeros(40, dtype=np.int32), c['fw'][:1], (0.5, 0.5), 4)
    assert g0.tobytes() == one[0].tobytes() and p0.tobytes() == one[1].tobytes()
    perm, off = V.fold_groups(fo, 3)
    assert perm.dtype == np.int32 and off.dtype == np.int32 and sorted(perm.tolist()) == list(range(40)) and off[0] == 0 and off[-1] == 40
    for f in range(3):
        assert (fo[perm[off[f]:off[f + 1]]] == f).all() and (np.diff(perm[off[f]:off[f + 1]]) > 0).all()
    assert sorted(perm[off[3]:].tolist()) == [3, 17]


# ---- the claim this method rests on ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def games():
    """{planted: (table before, moved table, log, id1, id2)} under adv_cases.GAME in float64, played once."""
    out = {}
    for planted in (True, False):
        X, id1, id2 = C.table(planted)
        moved, log = D.play(X, id1, id2, np.float64, **D.GAME)[:2]
        out[planted] = (X, moved, log, id1, id2)
    return out


def test_the_fresh_attacker_ends_near_chance(games):
    """Observed: planted 0.9957 -> 0.5489, null 0.5385 -> 0.5270 (tests/adv_cases.py states them)."""
    X, moved, log, id1, id2 = games[True]
    before, after = D.fresh_auc(X, id1, id2), D.fresh_auc(moved, id1, id2)
    print('planted', before, after, np.sqrt(log['reg'][-1] / (len(id1) + len(id2))))
    assert abs(before - 0.9957) < 5e-4
    assert after <= D.AUC_CAP
    Xn, moved_n, log_n, _, _ = games[False]
    after_n = D.fresh_auc(moved_n, id1, id2)
    print('null', D.fresh_auc(Xn, id1, id2), after_n, np.sqrt(log_n['reg'][-1] / (len(id1) + len(id2))))
    assert abs(after_n - 0.5) < 0.1
    # only the selected rows moved, and the log has one value per round
    other = np.setdiff1d(np.arange(len(X)), np.concatenate([id1, id2]))
    assert np.array_equal(moved[other], X[other]) and not np.array_equal(moved[id1], X[id1])
    assert log['loss_first'].shape == (100, 2) and log['gt'].shape == log['eq'].shape == log['reg'].shape == (100,)
    assert (np.diff(log['reg'][:5]) > 0).all()


# ---- plants ---------------------------------------------------------------------------------------------------------------------------
def test_every_plant_is_beyond_the_bound_of_the_gpu_comparison():
    """tests/test_gpu_adv.py holds a round's gradient to E_k <= 4 max(E_y, ulp32) of the float64 contract, relative to its largest
    entry: every plant must lie more than 100 x beyond that, on the gradient of the second of two rounds (the statistics of round 0
    are stale only from there on)."""
    X, id1, id2 = C.table(True)
    short = dict(D.GAME, rounds=2)
    base = D.play(X, id1, id2, np.float64, **short)[1]['grad']
    bound = 4 * max(_rel(D.play(X, id1, id2, np.float32, **short)[1]['grad'], base), ULP32)
    assert bound < 1e-4
    for plant in V.PLANTS:
        off = _rel(D.play(X, id1, id2, np.float64, plant=plant, **short)[1]['grad'], base)
        print(plant, off, bound)
        assert off > 100 * bound, plant
    assert set(V.PLANTS) >= {'own_fold', 'no_inv_std', 'relu_mask_dropped', 'target_is_label', 'stale_stats'}
    assert A.PLANTS == ('no_class_weight', 'heldout_leaks', 'stats_from_all_rows', 'stale_bias_correction', 'ties_as_wins')


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal():
    ok = dict(n_rows=100, d=8, id1=np.arange(10), id2=np.arange(10, 30), hidden=4, folds=5, rounds=3, disc_epochs=2, disc_lr=1e-2, l2=0.0, lr=0.1,
              eta=0.0, alpha=0.0, target='confuse')
    out = V.check_adv_args(**ok)
    assert out[1:12] == (10, 20, 4, 5, 3, 2, 1e-2, 0.0, 0.1, 0.0, 0.0) and out[12] == (0.5, 0.5)
    for change, msg in ((dict(hidden=-1), 'hidden'), (dict(hidden=129), 'hidden'), (dict(hidden=1.5), 'hidden'), (dict(hidden=True), 'hidden'),
                        (dict(d=0), 'width'), (dict(d=129), 'width'), (dict(folds=1), 'folds'), (dict(folds=17), 'folds'),
                        (dict(folds=11), 'at least folds'), (dict(id1=np.arange(4)), 'at least folds'),
                        (dict(rounds=0), 'rounds'), (dict(rounds=1.5), 'rounds'), (dict(disc_epochs=0), 'disc_epochs'),
                        (dict(lr=0.0), 'lr'), (dict(lr=-1.0), 'lr'), (dict(lr=float('nan')), 'lr'), (dict(lr=float('inf')), 'lr'),
                        (dict(disc_lr=0.0), 'disc_lr'), (dict(disc_lr=float('nan')), 'disc_lr'), (dict(disc_lr=float('inf')), 'disc_lr'),
                        (dict(eta=-1.0), 'eta'), (dict(eta=float('nan')), 'eta'), (dict(eta=float('inf')), 'eta'),
                        (dict(alpha=-1e-3), 'alpha'), (dict(alpha=float('nan')), 'alpha'), (dict(l2=-1e-3), 'l2'), (dict(l2=float('nan')), 'l2'),
                        (dict(target='reverse'), 'diverges'), (dict(target='label'), "'confuse'"), (dict(target=(0.5, 0.5)), "'confuse'"),
                        (dict(id1=[]), 'empty'), (dict(id1=np.arange(5, 15)), 'share'), (dict(id2=np.arange(90, 110)), 'outside'),
                        (dict(id1=[1, 1, 2, 3, 4]), 'more than once'), (dict(id1=np.arange(10.0)), 'integer')):
        with pytest.raises(ValueError, match=msg):
            V.check_adv_args(**{**ok, **change})
    assert V.DEFAULTS == dict(hidden=32, folds=5, rounds=100, disc_epochs=5, disc_lr=1e-2, l2=1e-4, lr=0.1, eta=1.0, alpha=0.0, target='confuse', seed=0)


def test_main_flags_and_their_refusals_before_anything_runs(tmp_path):
    from ultrare_amd import main
    args = main.parser.parse_args([])
    assert (args.adv_unlearn, args.adv_rounds, args.adv_hidden) == (False, 100, 32)
    args = main.parser.parse_args(['--adv-unlearn', '--adv-rounds', '7', '--adv-hidden', '0', '--attr-file', 'a.npz'])
    assert (args.adv_unlearn, args.adv_rounds, args.adv_hidden, args.attr_file) == (True, 7, 0, 'a.npz')
    assert main.adv_setting(False, None) is None
    attr = str(tmp_path / 'groups.npz')
    np.savez(attr, id1=np.arange(0, 1508, 2), id2=np.arange(1, 1508, 2))
    s = main.adv_setting(True, attr, 'mf', 7, 4)
    assert (s['rounds'], s['hidden'], len(s['id1']), len(s['id2'])) == (7, 4, 754, 754)
    save = tmp_path / 'out'
    base = ['--dataset', 'toy', '--save-dir', str(save)]
    bad = str(tmp_path / 'bad.npz')
    np.savez(bad, id1=np.arange(3))
    far = str(tmp_path / 'far.npz')
    np.savez(far, id1=np.arange(0, 10), id2=np.arange(5, 2000))
    for extra, msg in ((['--adv-unlearn'], '--adv-unlearn needs --attr-file'),
                       (['--adv-unlearn', '--attr-file', attr, '--model', 'nmf'], 'nmf'),
                       (['--adv-unlearn', '--attr-file', attr, '--adv-rounds', '0'], '--adv-rounds'),
                       (['--adv-unlearn', '--attr-file', attr, '--adv-hidden', '129'], '--adv-hidden'),
                       (['--adv-unlearn', '--attr-file', bad], 'id1 and id2'),
                       (['--adv-unlearn', '--attr-file', far], 'outside|share'),
                       (['--adv-unlearn', '--attr-file', attr, '--k', '256'], 'width')):
        with pytest.raises(ValueError, match=msg):
            main.main(base + extra)
        assert not save.exists(), extra
    help_text = main.parser.format_help()
    assert 'not rewritten' in help_text and '--adv-rounds' in help_text and '--adv-hidden' in help_text


# ---- header, binding, library ---------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_adv.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.ADV_EXPORTS) == {'ure_adv_input_grad'}
    for other in (nv.EXPORTS, nv.CSR_PAIR_EXPORTS, nv.GCN_EXPORTS, nv.BPR_EXPORTS, nv.INF_EXPORTS, nv.NMF_EXPORTS, nv.NMF_RANK_EXPORTS, nv.COMBINE_RANK_EXPORTS,
                  nv.ATTR_TRAIN_EXPORTS, nv.ATTACK_EXPORTS):
        assert not declared & set(other)
    assert '#include "ultrare_adv.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    L = ctypes.CDLL(nv.LIB_PATH)
    for name, (res, args) in nv._ADV_PROTOTYPES.items():
        assert hasattr(L, name), name
        assert getattr(nv.lib(), name).argtypes == args
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    from ultrare_amd import build
    assert 'adv.hip' in build.SOURCES and 'adv.hip' not in build.STEP_KERNEL_FILES
    assert re.search(r'#define\s+URE_ADV_RUN\s+256\b', header)
    # the header is part of the identity of the built code
    import inspect
    assert "'ultrare_adv.h'" in inspect.getsource(build.source_hash)


def test_abi_is_where_it_was(nv):
    assert len(nv.EXPORTS) == 96 and not set(nv.EXPORTS) & set(nv.ADV_EXPORTS)
    assert len(nv.ATTACK_EXPORTS) == 7
    assert nv.ABI_VERSION == 15 and nv.lib().ure_abi_version() == 15
    assert '#define URE_ABI_VERSION 15' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()


def test_argument_checks_come_before_any_device_work(nv):
    """Every refusal of the entry returns -1 on a machine without a device: no HIP call was reached."""
    L = nv.lib()
    one = ctypes.c_void_p(8)        # (never dereferenced: the checks refuse first)
    ok = dict(X=one, ld=8, d=8, rows=one, fold_of=one, m=100, n1=30, folds=2, H=4, stats=one, params=one, fw=one, t0=0.5, t1=0.5, grad=one, p=None,
              perm=one, off=one)
    order = list(ok)
    for change in (dict(X=None), dict(rows=None), dict(stats=None), dict(params=None), dict(fw=None), dict(grad=None), dict(d=0), dict(d=129), dict(H=-1),
                   dict(H=129), dict(folds=0), dict(folds=17), dict(m=0), dict(m=(1 << 24) + 1), dict(ld=7), dict(n1=-1), dict(n1=101),
                   dict(t0=float('nan')), dict(t1=float('nan')), dict(t0=float('inf')), dict(t1=-float('inf')), dict(perm=None), dict(off=None)):
        a = {**ok, **change}
        assert L.ure_adv_input_grad(*[a[k] for k in order], None) == -1, change
        assert b'argument check failed' in L.ure_last_error()


def test_no_adv_kernel_spills_or_uses_scratch(nv):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = [r for r in isa_report.kernels(nv.LIB_PATH) if r['name'].startswith('adv_')]
    assert {r['name'] for r in rows} == {'adv_input_grad_kernel'}
    for r in rows:
        assert r['vgpr_spill'] == 0 and r['scratch'] == 0, r
