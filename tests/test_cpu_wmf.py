"""Weighted matrix factorisation for implicit feedback without a GPU: the numpy contract (ultrare_amd/wmf.py) against dense
evaluations over ALL user x item pairs at a tiny shape -- which is what proves the Gram trick --, the two-level Gram chain against
its literal loops, the sweeps' monotone objective, every refusal, the command line, the saved parameters, and the binding table
against the header and the built library."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest

import wmf_cases as C
from ultrare_amd import ridge
from ultrare_amd import wmf as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ---- the contract against dense evaluations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha,l2,l2_n', [(40.0, 0.1, 0.0), (3.0, 0.5, 0.05), (0.0, 0.1, 0.0)])
def test_gram_trick_equals_the_dense_weighted_least_squares(alpha, l2, l2_n):
    """Per user the normal equations of the weighted least squares over all 11 items -- confidence 1 + wg and target wb / c on an
    observed item, confidence 1 and target 0 on every other -- solved by np.linalg.solve, against wridge_rows_ref with
    G0 = gram_ref(V), which touches the observed items only."""
    uid, iid, r, _, V = C.tiny()
    k = 3
    off, idx, val, _ = ridge.segment_csr(uid, iid, r, 7)
    wg, wb = W.confidence_ref(val, alpha)
    X, failed = W.wridge_rows_ref(V, k, off, idx, wg, wb, W.gram_ref(V, k), l2, l2_n)
    assert not failed and X.shape == (7, k) and not X[5].any()                 # user 5 has no observation: the zero row
    V64 = V.astype(np.float64)
    worst = 0.0
    for u in range(7):
        a, b = off[u], off[u + 1]
        if a == b:
            continue
        c, cp = np.ones(11), np.zeros(11)
        c[idx[a:b]] += wg[a:b].astype(np.float64)
        cp[idx[a:b]] = wb[a:b].astype(np.float64)
        want = np.linalg.solve(V64.T @ (c[:, None] * V64) + (l2 + l2_n * (b - a)) * np.eye(k), V64.T @ cp)
        worst = max(worst, np.abs(X[u] - want).max() / np.abs(want).max())
    print('largest relative difference', worst)
    assert worst <= 1e-12


def test_confidence_ref():
    r = (np.arange(1, 6) / 5.0).astype(np.float32)
    wg, wb = W.confidence_ref(r, 0.1)
    assert wg.dtype == wb.dtype == np.float32
    assert np.array_equal(wg, np.float32(0.1) * r) and np.array_equal(wb, np.float32(1) + wg)
    wg, wb = W.confidence_ref(r, 0.0)
    assert not wg.any() and (wb == 1).all()


@pytest.mark.parametrize('alpha,l2,l2_n', [(40.0, 0.1, 0.0), (3.0, 0.5, 0.05)])
def test_objective_ref_equals_the_dense_objective(alpha, l2, l2_n):
    uid, iid, r, U, V = C.tiny()
    wg, wb = W.confidence_ref(r, alpha)
    got, want = W.objective_ref(U, V, uid, iid, wg, wb, l2, l2_n), W.objective_dense(U, V, uid, iid, wg, wb, l2, l2_n)
    print(got, want, abs(got - want) / want)
    assert abs(got - want) <= 1e-12 * want
    # the textbook form sum c (p - s)^2 with c = wb, p = 1: equal up to the one float32 rounding of wb = fl32(1 + wg)
    S = U.astype(np.float64) @ V.astype(np.float64).T
    Cm, P = np.ones((7, 11)), np.zeros((7, 11))
    Cm[uid, iid], P[uid, iid] = wb.astype(np.float64), 1.0
    nu, ni = np.bincount(uid, minlength=7), np.bincount(iid, minlength=11)
    book = (Cm * (P - S) ** 2).sum() + ((l2 + l2_n * nu) * (U.astype(np.float64) ** 2).sum(1)).sum() + ((l2 + l2_n * ni) * (V.astype(np.float64) ** 2).sum(1)).sum()
    assert abs(got - book) <= 2.0 ** -22 * book


@pytest.mark.parametrize('alpha,l2,l2_n', [(40.0, 0.1, 0.0), (3.0, 0.5, 0.05)])
def test_sweeps_never_increase_the_objective(alpha, l2, l2_n):
    """Each half sweep minimises J over its block exactly; the float32 rounding of the rows is inside the contract, so an increase
    of 1e-6 |J| is allowed.  Largest relative increase seen: 0.0 in every case (the objective falls at every half sweep)."""
    for (uid, iid, r, U, V) in (C.tiny(), C.rating_set(40, 30, 300, 4) + (C.normal_table(40, 5, 5), C.normal_table(30, 5, 6))):
        U1, V1, obj = W.wmf_sweeps_ref(U, V, uid, iid, r, alpha, l2, l2_n, sweeps=4)
        assert obj.shape == (9,) and obj.dtype == np.float64 and U1.dtype == V1.dtype == np.float32
        rise = max((b - a) / abs(a) for a, b in zip(obj[:-1], obj[1:]))
        print('objectives', obj.tolist(), 'largest relative increase', rise)
        assert all(b <= a + 1e-6 * abs(a) for a, b in zip(obj[:-1], obj[1:]))
        assert obj[-1] < 0.5 * obj[0]
        wg, wb = W.confidence_ref(r, alpha)
        assert obj[-1] == W.objective_ref(U1, V1, uid, iid, wg, wb, l2, l2_n)
    U0, V0, obj0 = W.wmf_sweeps_ref(U, V, uid, iid, r, alpha, l2, l2_n, sweeps=0)
    assert obj0.shape == (1,) and np.array_equal(U0, U) and np.array_equal(V0, V)


def test_a_shard_s_universe_is_its_own_users():
    """Users without observations get the zero row in the first user half, so they add nothing to the Gram matrix of the item half;
    an item nobody rated gets the zero row."""
    uid, iid, r, U, V = C.tiny()
    U1, V1, _ = W.wmf_sweeps_ref(U, V, uid, iid, r, 40.0, 0.1, sweeps=1)
    assert not U1[5].any() and not V1[9].any() and U1[[0, 1, 2, 3, 4, 6]].any(axis=1).all()


# ---- the Gram chain -------------------------------------------------------------------------------------------------------------
def _gram_loops(F, k):
    """The two-level chain written out: Python floats are IEEE doubles, one rounding per multiply-add step (the product is exact)."""
    n = len(F)
    G = None
    for c0 in range(0, n, W.CHUNK):
        part = [[0.0] * k for _ in range(k)]
        for i in range(c0, min(n, c0 + W.CHUNK)):
            f = [float(v) for v in F[i, :k]]
            for a in range(k):
                for b in range(a, k):
                    part[a][b] = part[a][b] + f[a] * f[b]
        if G is None:
            G = part
        else:
            G = [[G[a][b] + part[a][b] for b in range(k)] for a in range(k)]
    return np.array([G[a][b] for a in range(k) for b in range(a, k)])


@pytest.mark.parametrize('n,d,k', [(1, 4, 4), (255, 4, 3), (256, 4, 2), (257, 8, 3), (700, 4, 3)])
def test_gram_ref_is_the_two_level_chain(n, d, k):
    F = C.normal_table(n, d, seed=n)
    got = W.gram_ref(F, k)
    assert got.dtype == np.float64 and got.shape == (k * (k + 1) // 2,)
    assert got.tobytes() == _gram_loops(F, k).tobytes()


@pytest.mark.parametrize('n,d,k', [(1, 4, 4), (255, 8, 5), (256, 16, 16), (257, 32, 32), (513, 64, 64), (3000, 128, 100)])
def test_gram_ref_against_the_float64_product(n, d, k):
    F = C.normal_table(n, d, seed=n + 1)
    f = F[:, :k].astype(np.float64)
    got = W.tri_unpack(W.gram_ref(F, k), k)
    bound = 4 * n * 2.0 ** -53 * (np.abs(f).T @ np.abs(f))
    err = np.abs(got - f.T @ f)
    print('largest error / bound', (err / bound).max())
    assert (err <= bound).all() and np.array_equal(got, got.T)
    assert np.array_equal(W.tri_pack(got), W.gram_ref(F, k))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_check_wmf_args():
    assert W.check_wmf_args(40, 0.1, 0, 3) == (40.0, 0.1, 0.0, 3)
    assert W.check_wmf_args(0.0, 1e-9) == (0.0, 1e-9, 0.0, 1)
    for bad, msg in ((dict(alpha=-1.0), 'alpha'), (dict(alpha=float('nan')), 'alpha'), (dict(alpha=float('inf')), 'alpha'), (dict(alpha=True), 'alpha'),
                     (dict(alpha='40'), 'alpha'), (dict(alpha=1e39), 'alpha'), (dict(l2=0.0), 'l2'), (dict(l2=-0.1), 'l2'), (dict(l2=float('nan')), 'l2'),
                     (dict(l2=float('inf')), 'l2'), (dict(l2_n=-1e-3), 'l2_n'), (dict(l2_n=float('nan')), 'l2_n'), (dict(sweeps=-1), 'sweeps'),
                     (dict(sweeps=1.5), 'sweeps'), (dict(sweeps=True), 'sweeps')):
        with pytest.raises(ValueError, match=msg):
            W.check_wmf_args(**{**dict(alpha=40.0, l2=0.1, l2_n=0.0, sweeps=1), **bad})


def _param(tmp_path, **kw):
    from ultrare_amd.config import InsParam
    return InsParam('toy', 2, 24, [32], 2, 2, 'rand', data_dir=str(tmp_path), **kw)


def test_insparam_and_scratch_refusals(tmp_path, monkeypatch):
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method import sisa as sisa_mod
    p = _param(tmp_path, model='wmf')
    assert p.model == 'wmf' and not hasattr(p, 'wmf_alpha') and not hasattr(p, 'wmf_l2')
    q = _param(tmp_path, model='wmf', wmf_alpha=10, wmf_l2=0.5)
    assert (q.wmf_alpha, q.wmf_l2) == (10.0, 0.5)
    for kw, msg in ((dict(optimizer='adam'), "model='wmf'.*optimizer='adam'"), (dict(loss='bpr'), "model='wmf'.*loss='bpr'"),
                    (dict(unlearn='influence'), "model='wmf'.*unlearn='influence'"), (dict(dis_type='d2d', attr=[[1, 2], [3, 4]]), "model='wmf'.*dis_type='d2d'"),
                    (dict(dis_type='u2u', attr=[[1, 2], [3, 4]]), "model='wmf'.*dis_type='u2u'"), (dict(wmf_l2=0.0), 'l2'), (dict(wmf_alpha=-1.0), 'alpha')):
        with pytest.raises(ValueError, match=msg):
            _param(tmp_path, model='wmf', **kw)
    with pytest.raises(ValueError, match="go with model='wmf'"):
        _param(tmp_path, wmf_alpha=10.0)
    with pytest.raises(ValueError, match="go with model='wmf'"):
        _param(tmp_path, model='lightgcn', wmf_l2=1.0)
    # Scratch and Sisa hold the same table: an object handed other parameters than InsParam would build
    sc = Scratch(p, 'wmf')
    assert (sc.wmf_alpha, sc.wmf_l2) == (W.DEFAULT_ALPHA, W.DEFAULT_L2) == (40.0, 0.1)
    assert (Scratch(q, 'wmf').wmf_alpha, Scratch(q, 'wmf').wmf_l2) == (10.0, 0.5)
    for attr, value, msg in (('optimizer', 'adam', "optimizer='adam'"), ('loss', 'bpr', "loss='bpr'"), ('unlearn', 'influence', "unlearn='influence'"),
                             ('dis_type', 'd2d', "dis_type='d2d'"), ('wmf_l2', 0.0, 'l2')):
        bad = _param(tmp_path, model='wmf')
        setattr(bad, attr, value)
        with pytest.raises(ValueError, match=msg):
            Scratch(bad, 'wmf')
    with pytest.raises(ValueError, match='given_model'):
        sc._train_wmf(None, None, [], False, 0, '', 0, given_model=object())
    # parallel warns and is ignored; more than one rank is refused
    p.parallel = True
    with pytest.warns(UserWarning, match='one after the other'):
        s = Sisa(p, 'wmf', 2, [])
    assert s.parallel is False

    class TwoRanks:
        @staticmethod
        def get_world_size():
            return 2
    monkeypatch.setattr(sisa_mod, '_dist', lambda: TwoRanks)
    with pytest.raises(ValueError, match="model_type='wmf' runs on one rank, not 2"):
        Sisa(_param(tmp_path, model='wmf'), 'wmf', 2, [])
    with pytest.raises(ValueError, match="model='mf' only, not 'wmf'"):
        from ultrare_amd.influence import check_model
        check_model('wmf', 'mse')


def test_a_plain_insparam_keeps_its_pickle(tmp_path):
    """The WMF options are attributes only off their defaults: a plain InsParam pickles to the attributes it had before, in their
    order, and model='wmf' with default options differs from it in `model` alone."""
    plain = _param(tmp_path)
    keys = ['k', 'lam', 'layers', 'seed', 'n_worker', 'batch', 'lr', 'lr_decay', 'momentum', 'epochs', 'n_group', 'dis_type', 'attr', 'parallel',
            'optimizer', 'betas', 'eps', 'loss', 'model', 'gcn_layers', 'del_rating', 'dataset', 'max_rating', 'del_per', 'del_type', 'del_user',
            'n_user', 'n_item', 'train_dir', 'test_dir']
    assert sorted(vars(plain)) == sorted(keys)
    assert list(vars(plain))[:20] == keys[:20]
    wmf = _param(tmp_path, model='wmf')
    assert list(vars(wmf)) == list(vars(plain))
    assert {k for k in vars(plain) if k != 'del_user' and vars(plain)[k] != vars(wmf)[k]} == {'model'}
    wmf.model = 'mf'
    assert pickle.dumps(wmf) == pickle.dumps(plain)


def test_cli_parses_and_the_artifact_prefix(tmp_path):
    from ultrare_amd import main
    from ultrare_amd.config import Instance
    args = main.parser.parse_args([])
    assert (args.model, args.wmf_alpha, args.wmf_l2) == ('mf', 40.0, 0.1)
    args = main.parser.parse_args(['--model', 'wmf', '--wmf-alpha', '10', '--wmf-l2', '0.5', '--epoch', '3'])
    assert (args.model, args.wmf_alpha, args.wmf_l2, args.epoch) == ('wmf', 10.0, 0.5, 3)
    assert 'untuned' in main.parser.format_help().lower()
    with pytest.raises(ValueError, match="model='wmf'.*loss='bpr'"):
        main.main(['--dataset', 'toy', '--model', 'wmf', '--loss', 'bpr', '--save-dir', str(tmp_path / 'r'), '--data-dir', str(tmp_path)])
    with pytest.raises(ValueError, match="go with model='wmf'"):
        main.main(['--dataset', 'toy', '--wmf-alpha', '3', '--save-dir', str(tmp_path / 'r'), '--data-dir', str(tmp_path)])
    assert not (tmp_path / 'r').exists()
    ins = Instance(_param(tmp_path, model='wmf'), save_dir=str(tmp_path / 'save'))
    assert ins._model() == ('wmf', 'WMF_')
    assert Instance(_param(tmp_path), save_dir=str(tmp_path / 'save'))._model() == ('mf', 'MF_')


# ---- the binding ------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_wmf.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.WMF_EXPORTS) == {'ure_gram_scratch', 'ure_gram', 'ure_wridge_rows_scratch', 'ure_wridge_rows'}
    for other in (nv.EXPORTS, nv.CSR_PAIR_EXPORTS, nv.GCN_EXPORTS, nv.BPR_EXPORTS, nv.INF_EXPORTS, nv.NMF_EXPORTS, nv.NMF_RANK_EXPORTS, nv.COMBINE_RANK_EXPORTS,
                  nv.ATTR_TRAIN_EXPORTS, nv.ATTACK_EXPORTS, nv.ADV_EXPORTS):
        assert not declared & set(other)
    main_header = open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    assert '#include "ultrare_wmf.h"' in main_header and 'ure_gram' not in main_header and 'ure_wridge_rows' not in main_header
    L = ctypes.CDLL(nv.LIB_PATH)
    for name, (res, args) in nv._WMF_PROTOTYPES.items():
        assert hasattr(L, name), name
        assert getattr(nv.lib(), name).argtypes == args
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    from ultrare_amd import build
    assert 'wmf.hip' in build.SOURCES and not {'wmf.hip', 'ridge_solve.h'} & set(build.STEP_KERNEL_FILES)
    assert re.search(r'#define\s+URE_GRAM_CHUNK\s+' + str(W.CHUNK) + r'\b', header)
    # the factor and solve stages exist once, in the header both kernels include
    for f in ('mf_ridge.hip', 'wmf.hip'):
        text = open(os.path.join(ROOT, 'ultrare_amd', 'csrc', f)).read()
        assert '#include "ridge_solve.h"' in text and 'rr_factor_solve_store<D>' in text and 'sqrt(' not in text


def test_abi_is_where_it_was(nv):
    assert len(nv.EXPORTS) == 96 and not set(nv.EXPORTS) & set(nv.WMF_EXPORTS)
    assert nv.ABI_VERSION == 15 and nv.lib().ure_abi_version() == 15
    assert '#define URE_ABI_VERSION 15' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()


def test_scratch_sizers(nv):
    L = nv.lib()
    for n, k in ((0, 8), (-1, 8), (1 << 31, 8), (100, 0), (100, 129)):
        assert L.ure_gram_scratch(n, k) == -1, (n, k)
    for n, k, chunks in ((1, 1, 1), (256, 5, 1), (257, 5, 2), (76801, 128, 301), ((1 << 31) - 1, 128, 1 << 23)):
        assert L.ure_gram_scratch(n, k) == chunks * (k * (k + 1) // 2) * 8, (n, k)
    for m, k in ((-1, 8), (10, 0), (10, 129)):
        assert L.ure_wridge_rows_scratch(m, k) == -1
    assert L.ure_wridge_rows_scratch(0, 1) == 0 and L.ure_wridge_rows_scratch(162000, 128) == 0


def test_argument_checks_come_before_any_device_work(nv):
    """Every refusal of the two entries returns -1 from the host checks: these calls hand over pointers that are never read."""
    L = nv.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    ok_g = dict(F=p, n=4, d=8, k=5, G0=p, scratch=p, bytes=1 << 20)
    for change in (dict(F=None), dict(G0=None), dict(scratch=None), dict(bytes=8), dict(n=0), dict(n=1 << 31), dict(k=0), dict(k=9), dict(d=6), dict(d=2), dict(d=256)):
        a = {**ok_g, **change}
        assert L.ure_gram(a['F'], a['n'], a['d'], a['k'], a['G0'], a['scratch'], a['bytes'], None) == -1, change
    ok_w = dict(F=p, n=4, d=8, k=5, off=p, idx=p, wg=p, wb=p, m=2, l2=0.1, l2_n=0.0, X=p, status=p)
    for change in (dict(F=None), dict(off=None), dict(idx=None), dict(wg=None), dict(wb=None), dict(X=None), dict(status=None), dict(n=0), dict(k=0), dict(k=9),
                   dict(d=6), dict(d=256), dict(m=-1), dict(m=1 << 31), dict(l2=-1.0), dict(l2=float('nan')), dict(l2_n=float('inf'))):
        a = {**ok_w, **change}
        assert L.ure_wridge_rows(a['F'], a['n'], a['d'], a['k'], a['off'], a['idx'], a['wg'], a['wb'], a['m'], None, None, a['l2'], a['l2_n'], a['X'],
                                 a['status'], None, 0, None) == -1, change
    assert b'argument check failed' in L.ure_last_error()


def test_no_new_kernel_spills(nv):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = [r for r in isa_report.kernels(nv.LIB_PATH) if r['name'].startswith(('wridge_rows_kernel<', 'gram_chunk_kernel<', 'gram_fold_kernel', 'ridge_rows_kernel<'))]
    names = {r['name'] for r in rows}
    for stem in ('wridge_rows_kernel', 'gram_chunk_kernel', 'ridge_rows_kernel'):
        assert {f'{stem}<{d}>' for d in (4, 8, 16, 32, 64, 128)} <= names
    assert 'gram_fold_kernel' in names
    for r in rows:
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, r
