"""The attribute-inference attacker without a GPU: the numpy contract (ultrare_amd/attack.py) against torch autograd, the fold
plan, the pair counts against the double loop, the two synthetic cases, the plants, every refusal, and the binding table against
the header and the built library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import attack_cases as C
from ultrare_amd import attack as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


@pytest.fixture(scope='module')
def fits():
    """{(planted, plant): the float64 contract's result} of the two tables, computed once."""
    out = {}
    for planted in (True, False):
        X, id1, id2 = C.table(planted)
        for plant in (None,) + A.PLANTS[:4]:
            out[planted, plant] = C.fit_contract(X, id1, id2, C.SETTINGS, np.float64, plant=plant)
        out[planted, 'float32'] = C.fit_contract(X, id1, id2, C.SETTINGS, np.float32)
    return out


def _autograd(X, rows, n1, fold_of, p0, H, epochs, lr, l2):
    """The literal model in torch float64: standardise on the fold's training rows, Linear - ReLU - Linear (or one Linear), the
    class-balanced BCE (mean over the training rows) + l2 / 2 |W|^2, torch.optim.Adam full batch."""
    from ultrare_amd import adam
    x = torch.from_numpy(np.asarray(X)[rows].astype(np.float64))
    m, d = x.shape
    y = (torch.arange(m) < n1).double()
    b1, b2, eps = adam.betas32(A.BETAS, A.EPS)
    l2 = float(np.float32(l2))
    scores, losses = np.zeros(m), []
    for f in range(len(p0)):
        tr = torch.from_numpy(fold_of != f)
        mean, std = x[tr].mean(0), x[tr].std(0, unbiased=False)
        z = (x - mean) / std
        W1, bb1, w2, bb2 = A.unpack(p0[f].astype(np.float64), d, H)
        ps = [torch.tensor(np.array(v), requires_grad=True) for v in ((W1, bb1) if H == 0 else (W1, bb1, w2, bb2))]
        opt = torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps)
        n_tr, n_pos = int(tr.sum()), int((tr & (y > 0)).sum())
        w = torch.where(y > 0, torch.tensor(n_tr / (2.0 * n_pos), dtype=torch.float64), torch.tensor(n_tr / (2.0 * (n_tr - n_pos)), dtype=torch.float64))

        def logit():
            a = z @ ps[0].T + ps[1]
            return a[:, 0] if H == 0 else torch.relu(a) @ ps[2] + ps[3]
        per_fold = []
        for _ in range(epochs):
            opt.zero_grad()
            bce = torch.nn.functional.binary_cross_entropy_with_logits(logit()[tr], y[tr], weight=w[tr], reduction='sum') / n_tr
            loss = bce + 0.5 * l2 * sum((p * p).sum() for p in (ps[:1] if H == 0 else (ps[0], ps[2])))
            per_fold.append(float(loss.detach()))
            loss.backward()
            opt.step()
        losses.append(per_fold)
        held = np.flatnonzero(fold_of == f)
        scores[held] = torch.sigmoid(logit()).detach().numpy()[held]
    return scores, np.array(losses)


@pytest.mark.parametrize('H', [0, 4])
def test_contract_is_autograd_adam_of_the_literal_model(H):
    """Agreement reached (float64 against float64; the two differ in summation order only): scores 2e-15 (H = 4) and 1e-15 (H = 0),
    losses 2e-15; asserted at 1e-12."""
    rs = np.random.RandomState(3)
    X = rs.randn(90, 5).astype(np.float32)
    ids = rs.permutation(90)[:70]
    X[ids[:30]] += 0.7
    rows, n1, n2, H, folds, epochs, lr, l2 = A.check_attack_args(90, 5, ids[:30], ids[30:], H, 2, 12, 1e-2, 1e-3)
    fold_of, p0 = A.fold_plan(n1, n2, folds, 1), A.init_params(5, H, folds, 1)
    got = A.train_ref(X, rows, n1, fold_of, p0, H, epochs, lr, l2, dtype=np.float64)
    scores, losses = _autograd(X, rows, n1, fold_of, p0, H, epochs, lr, l2)
    print('scores', np.abs(got['scores'] - scores).max(), 'loss', np.abs(got['loss'] - losses).max())
    assert np.abs(got['scores'] - scores).max() < 1e-12
    assert np.abs(got['loss'] - losses).max() < 1e-12
    assert (np.diff(got['loss'], axis=1) < 0).all()


def test_float32_contract_follows_the_float64_one():
    X, id1, id2 = C.table(True)
    a, b = (C.fit_contract(X, id1, id2, C.LOGISTIC, T)[0] for T in (np.float32, np.float64))
    assert a['params'].dtype == np.float32 and a['stats'].dtype == np.float32
    assert np.abs(a['scores'] - b['scores']).max() < 1e-5 and np.abs(a['loss'] - b['loss']).max() < 1e-5


@pytest.mark.parametrize('n1,n2,folds', [(2, 2, 2), (5, 5, 5), (16, 16, 16), (7, 40, 3), (101, 57, 5), (3, 1000, 3)])
def test_fold_plan(n1, n2, folds):
    fold_of = A.fold_plan(n1, n2, folds, 11)
    assert fold_of.dtype == np.int32 and fold_of.shape == (n1 + n2,)
    assert np.array_equal(fold_of, A.fold_plan(n1, n2, folds, 11)) and (n1 + n2 < 8 or not np.array_equal(fold_of, A.fold_plan(n1, n2, folds, 12)))
    total = np.bincount(fold_of, minlength=folds)
    c1, c0 = np.bincount(fold_of[:n1], minlength=folds), np.bincount(fold_of[n1:], minlength=folds)
    for sizes in (total, c1, c0):
        assert len(sizes) == folds and sizes.max() - sizes.min() <= 1
    # every fold holds out both classes -- at the minimum admissible group size too -- and trains on both
    assert c1.min() >= 1 and c0.min() >= 1 and (n1 - c1).min() >= 1 and (n2 - c0).min() >= 1


def test_init_params_and_layout():
    p = A.init_params(6, 5, 3, 4)
    assert p.shape == (3, A.n_params(6, 5)) == (3, 41) and p.dtype == np.float32
    assert np.array_equal(p, A.init_params(6, 5, 3, 4)) and not np.array_equal(p[0], p[1])
    W1, b1, w2, b2 = A.unpack(p[0], 6, 5)
    assert W1.shape == (5, 6) and not b1.any() and b2 == 0 and np.abs(W1).max() <= np.sqrt(6 / 11) and np.abs(w2).max() <= 1.0
    assert A.weight_mask(6, 5).sum() == 35 and A.weight_mask(6, 0).tolist() == [True] * 6 + [False]
    q = A.init_params(6, 0, 2, 4)
    assert q.shape == (2, 7) and not q[:, 6].any()


def test_standardize_ref():
    rs = np.random.RandomState(0)
    X = rs.randn(50, 4).astype(np.float32) * 3 + 1
    X[:, 2] = 0.1                      # a zero-variance column
    rows = rs.permutation(50)[:40]
    fold_of = A.fold_plan(15, 25, 4, 0)
    st = A.standardize_ref(X, rows, fold_of, 4)
    assert st.shape == (4, 2, 4) and st.dtype == np.float32
    for f in range(4):
        x = X[rows][fold_of != f].astype(np.float64)
        assert np.allclose(st[f, 0], x.mean(0), rtol=1e-6) and np.allclose(st[f, 1, [0, 1, 3]], 1 / x.std(0)[[0, 1, 3]], rtol=1e-6)
        assert st[f, 1, 2] == 0 and st[f, 0, 2] == np.float32(0.1)


@pytest.mark.parametrize('name', sorted(C.score_cases()))
def test_auc_counts_ref_is_the_double_loop(name):
    scores, pos, neg = C.score_cases()[name]
    gt, eq = A.auc_counts_ref(scores, pos, neg)
    assert (gt, eq) == C.double_loop(scores, pos, neg)
    if name == 'all_equal':
        assert (gt, eq) == (0, len(pos) * len(neg))
    if name == 'signed_zeros':
        assert eq == 6          # -0.0 == +0.0: two zeros among the positives, three among the negatives
    tp, fn, tn, fp = A.confusion_ref(scores, pos, neg)
    assert tp + fn == len(pos) and tn + fp == len(neg) and tp == int((scores[pos] > 0.5).sum())
    wide = np.full(len(scores) + 9, np.nan, dtype=np.float32)      # unselected NaNs do not matter
    wide[:len(scores)] = scores
    assert A.auc_counts_ref(wide, pos, neg) == (gt, eq)


def test_nan_scores_are_refused():
    s = np.array([0.1, np.nan, 0.3], dtype=np.float32)
    for pos, neg in (([1], [0, 2]), ([0], [1])):
        with pytest.raises(ValueError, match='NaN'):
            A.auc_counts_ref(s, pos, neg)
        with pytest.raises(ValueError, match='NaN'):
            A.confusion_ref(s, pos, neg)
    assert A.auc_counts_ref(s, [0], [2]) == (0, 0)
    with pytest.raises(ValueError, match='at least one'):
        A.auc_counts_ref(s, [], [2])


def test_metrics():
    m = A.metrics(6, 2, 3, 1, 1, 1)
    assert m == dict(auc=7 / 8, bacc=0.5 * (3 / 4 + 1 / 2), f1=6 / 8)
    assert A.metrics(0, 0, 0, 2, 3, 0)['f1'] == 0.0


def test_planted_is_clearly_above_null(fits):
    """The one place where the contract's own AUC is pinned (tests/attack_cases.py states the values); the GPU tests compare
    against the contract, never against these numbers."""
    res = {}
    for planted in (True, False):
        out, rows, n1, n2, fold_of, _ = fits[planted, None]
        res[planted] = C.aucs(out['scores'].astype(np.float32), n1, n2, fold_of)
        print('planted' if planted else 'null', res[planted])
    (auc_p, folds_p), (auc_n, folds_n) = res[True], res[False]
    assert abs(auc_p - 0.9957) < 5e-4 and abs(auc_n - 0.5385) < 5e-4
    spread = max(max(folds_p) - min(folds_p), max(folds_n) - min(folds_n))
    assert auc_p - auc_n > 10 * spread
    assert abs(auc_n - 0.5) < 0.1 and auc_p > 0.99
    for planted in (True, False):
        loss = fits[planted, None][0]['loss']
        assert (loss[:, -1] < loss[:, 0]).all()


def test_every_plant_is_beyond_the_bound_of_the_gpu_comparison(fits):
    """tests/test_gpu_attack.py holds the device scores to E_k <= 4 max(E_y, ulp32) of the float64 contract and the pair counts to
    equal integers: every plant of attack.PLANTS must lie outside that, on both tables."""
    ulp32 = 2.0 ** -24
    for planted in (True, False):
        base = fits[planted, None][0]['scores']
        bound = 4 * max(np.abs(fits[planted, 'float32'][0]['scores'] - base).max(), ulp32)
        assert bound < 1e-5
        for plant in A.PLANTS[:4]:
            off = np.abs(fits[planted, plant][0]['scores'] - base).max()
            print(planted, plant, off, bound)
            assert off > 100 * bound, (planted, plant)
    scores, pos, neg = C.score_cases()['ties']
    assert A.auc_counts_ref(scores, pos, neg, plant='ties_as_wins') != A.auc_counts_ref(scores, pos, neg)
    assert set(A.PLANTS) == {'no_class_weight', 'heldout_leaks', 'stats_from_all_rows', 'stale_bias_correction', 'ties_as_wins'}


def test_every_refusal():
    ok = dict(n_rows=100, d=8, id1=np.arange(10), id2=np.arange(10, 30), hidden=4, folds=5, epochs=3, lr=1e-2, l2=0.0)
    A.check_attack_args(**ok)
    for change, msg in ((dict(hidden=-1), 'hidden'), (dict(hidden=129), 'hidden'), (dict(hidden=1.5), 'hidden'), (dict(hidden=True), 'hidden'),
                        (dict(d=0), 'width'), (dict(d=129), 'width'), (dict(folds=1), 'folds'), (dict(folds=17), 'folds'),
                        (dict(folds=11), 'at least folds'), (dict(id1=np.arange(4)), 'at least folds'), (dict(epochs=0), 'epochs'),
                        (dict(lr=0.0), 'lr'), (dict(lr=float('nan')), 'lr'), (dict(lr=float('inf')), 'lr'), (dict(l2=-1e-3), 'l2'),
                        (dict(l2=float('nan')), 'l2'), (dict(id1=[]), 'empty'), (dict(id1=np.arange(5, 15)), 'share'),
                        (dict(id2=np.arange(90, 110)), 'outside'), (dict(id1=[1, 1, 2, 3, 4]), 'more than once'),
                        (dict(id1=np.arange(10.0)), 'integer')):
        with pytest.raises(ValueError, match=msg):
            A.check_attack_args(**{**ok, **change})
    from ultrare_amd import main
    with pytest.raises(ValueError, match='--attack needs --attr-file'):
        main.attack_setting(True, None)
    assert main.attack_setting(False, None) is None
    args = main.parser.parse_args([])
    assert (args.attack, args.attack_hidden, args.attack_folds) == (False, 100, 5)
    args = main.parser.parse_args(['--attack', '--attack-hidden', '0', '--attack-folds', '3', '--attr-file', 'a.npz'])
    assert (args.attack, args.attack_hidden, args.attack_folds, args.attr_file) == (True, 0, 3, 'a.npz')


def test_main_attack_without_attr_file_is_refused_before_anything_runs(tmp_path):
    from ultrare_amd import main
    with pytest.raises(ValueError, match='--attack needs --attr-file'):
        main.main(['--dataset', 'toy', '--attack', '--save-dir', str(tmp_path)])
    assert not os.listdir(tmp_path)
    path = str(tmp_path / 'bad.npz')
    np.savez(path, id1=np.arange(3))
    with pytest.raises(ValueError, match='id1 and id2'):
        main.attack_setting(True, path)


def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_attack.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.ATTACK_EXPORTS) and len(declared) == 7
    for other in (nv.EXPORTS, nv.CSR_PAIR_EXPORTS, nv.GCN_EXPORTS, nv.BPR_EXPORTS, nv.INF_EXPORTS, nv.NMF_EXPORTS, nv.NMF_RANK_EXPORTS, nv.COMBINE_RANK_EXPORTS,
                  nv.ATTR_TRAIN_EXPORTS):
        assert not declared & set(other)
    assert '#include "ultrare_attack.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    L = ctypes.CDLL(nv.LIB_PATH)
    for name, (res, args) in nv._ATTACK_PROTOTYPES.items():
        assert hasattr(L, name), name
        assert getattr(nv.lib(), name).argtypes == args
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    from ultrare_amd import build
    assert 'attack.hip' in build.SOURCES and 'attack.hip' not in build.STEP_KERNEL_FILES
    for name, value in (('URE_ATTACK_MAX_D', A.MAX_D), ('URE_ATTACK_MAX_H', A.MAX_H), ('URE_ATTACK_MAX_FOLDS', A.MAX_FOLDS), ('URE_ATTACK_CHUNK', A.CHUNK)):
        assert re.search(r'#define\s+' + name + r'\s+' + str(value) + r'\b', header), name
    assert '(1 << 24)' in header and A.MAX_ROWS == 1 << 24
    from ultrare_amd import nmf
    assert A.CHUNK == nmf.CHUNK


def test_abi_is_where_it_was(nv):
    assert len(nv.EXPORTS) == 96 and not set(nv.EXPORTS) & set(nv.ATTACK_EXPORTS)
    assert nv.ABI_VERSION == 15 and nv.lib().ure_abi_version() == 15
    assert '#define URE_ABI_VERSION 15' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()


def test_scratch_sizers(nv):
    L = nv.lib()
    for m, d, H, folds in ((1, 8, 4, 2), (100, 0, 4, 2), (100, 129, 4, 2), (100, 8, -1, 2), (100, 8, 129, 2), (100, 8, 4, 1), (100, 8, 4, 17),
                           ((1 << 24) + 1, 8, 4, 2), (4, 8, 4, 5)):
        assert L.ure_attack_scratch(m, d, H, folds) == -1, (m, d, H, folds)
    last = 0
    for m in (2, 255, 256, 257, 1000, 162000, 1 << 24):
        b = L.ure_attack_scratch(m, 16, 8, 2)
        assert b >= last and b % 8 == 0 and b > 0
        last = b
    assert L.ure_attack_scratch(1000, 16, 8, 2) < L.ure_attack_scratch(1000, 17, 8, 2) < L.ure_attack_scratch(1000, 17, 9, 2) < L.ure_attack_scratch(1000, 17, 9, 3)
    # the layout the header states: chunks = ceil(m / 256); 8 F chunks + 8 F + 4 F chunks P + 8 F P
    P, F, chunks = A.n_params(128, 100), 5, -(-162000 // 256)
    assert L.ure_attack_scratch(162000, 128, 100, F) == -(-(8 * F * chunks + 8 * F + 4 * F * chunks * P + 8 * F * P) // 8) * 8
    assert L.ure_attack_scratch(50, 7, 0, 2) == 8 * 2 + 8 * 2 + 4 * 2 * 8 + 8 * 2 * 8
    for n1, n2 in ((0, 5), (5, 0), (1 << 31, 5), (5, 1 << 31)):
        assert L.ure_auc_scratch(n1, n2) == -1
    assert L.ure_auc_scratch(1, 1) == 24 and L.ure_auc_scratch(256, 1024) == 24 and L.ure_auc_scratch(257, 1025) == 80
    assert L.ure_auc_scratch(257, 1024 * 129) == 20 * 2 * 128          # at most 128 splits of the negatives


def test_no_new_kernel_spills_vector_registers(nv):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = [r for r in isa_report.kernels(nv.LIB_PATH) if r['name'].startswith(('attack_', 'auc_', 'confusion_kernel'))]
    names = {r['name'] for r in rows}
    assert {'attack_stats_kernel', 'attack_update_kernel', 'attack_score_kernel', 'auc_tile_kernel', 'auc_sum_kernel', 'confusion_kernel'} <= names
    assert sum(n.startswith('attack_train_kernel<') for n in names) == 16
    for r in rows:
        assert r['vgpr_spill'] == 0 and r['scratch'] == 0, r
