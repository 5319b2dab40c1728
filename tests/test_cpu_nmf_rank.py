"""NeuMF catalogue sweeps without a GPU: the numpy contract (ultrare_amd/nmf.py: prefix_ref, forward_from_prefix_ref, recommend_ref,
rank_ref), the C ABI's bookkeeping (include/ultrare_nmf_rank.h) and the refusals of every layer of the surface."""
import ctypes
import functools
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import nmf_cases as C
from ultrare_amd import nmf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACKS = [(4, [8, 4]), (32, [32, 16]), (32, [64, 32]), (8, [16, 128, 4]), (16, [16, 8, 8, 4, 4])]


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import _native
    return _native


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def planted_model(k, layers, n_user, n_item, seed):
    """nmf_cases.stage_model (two units of layer 0 with a pre-activation of exactly zero: relu's zero branch) with a NaN planted
    in one item's MLP half and in one user's GMF half."""
    U, V, dense = C.stage_model(k, layers, n_user, n_item, seed)
    V[2, k + 1] = np.nan
    U[3, 0] = np.nan
    return U, V, dense


# ------------------------------------------------------------------ 1. the prefix is exact
@pytest.mark.parametrize('k,layers', STACKS, ids=str)
def test_forward_from_prefix_is_forward_bit_for_bit(k, layers):
    n_user, n_item = 9, 13
    U, V, dense = planted_model(k, layers, n_user, n_item, seed=k)
    uid, iid = (a.reshape(-1) for a in np.meshgrid(np.arange(n_user), np.arange(n_item), indexing='ij'))
    want, act = nmf.forward_ref(U, V, dense, k, layers, uid, iid)
    S = nmf.Shape(k, layers)
    a1 = act[:, S.a_at[1]:S.a_at[1] + S.layers[1]]
    assert (a1[iid != 2, :2] == 0).all() and np.isnan(a1[iid == 2, :2]).all() and np.isnan(want).any() and not np.isnan(want).all()          # the zero branch and the NaN are there
    prefix = nmf.prefix_ref(U, dense, k, layers, uid)
    assert prefix.shape == (len(uid), layers[1]) and prefix.dtype == np.float32
    got = nmf.forward_from_prefix_ref(prefix, V, dense, k, layers, U, uid, iid)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    # the prefix of a user does not depend on the item: one row per user serves the whole catalogue
    per_user = nmf.prefix_ref(U, dense, k, layers, np.arange(n_user))
    assert np.array_equal(bits(per_user[uid]), bits(prefix))
    # the test can fail: fused multiply-adds, or the item half summed on its own, give other bytes -- in a_1 at every stack, in
    # the prediction wherever a_1 reaches it through one layer
    _, a1_got = nmf.forward_from_prefix_ref(prefix, V, dense, k, layers, U, uid, iid, want_a1=True)
    assert np.array_equal(bits(a1_got), bits(a1))
    for plant in nmf.RANK_PLANTS:
        other, a1_other = nmf.forward_from_prefix_ref(prefix, V, dense, k, layers, U, uid, iid, plant=plant, want_a1=True)
        ok = ~np.isnan(want)
        assert np.allclose(other[ok], want[ok], rtol=1e-4, atol=1e-5), plant
        assert not np.array_equal(bits(a1_other), bits(a1)), plant
        assert len(layers) > 2 or not np.array_equal(bits(other), bits(want)), plant


# ------------------------------------------------------------------ 2. top-k and ranks against a brute-force lexsort
def brute(sc_row, excl_row):
    """The eligible items of one row, best first, by a lexsort that does not go through rank_keys: NaN last, -0.0 == +0.0 (the
    comparison of floats), then the item id."""
    s = np.asarray(sc_row, dtype=np.float64).copy()
    nan = np.isnan(s)
    s[nan] = -np.inf
    order = np.lexsort((np.arange(len(s)), -s, nan))          # last key first: not NaN, then score descending, then id
    keep = np.ones(len(s), dtype=bool)
    keep[excl_row] = False
    return order[keep[order]]


@functools.lru_cache(maxsize=None)
def oracle_case():
    """Three models of (8, [16, 8]) over 40 items and 6 users with duplicated item rows (ties across the ensemble), NaN and +-inf
    scores, a row with everything excluded and one with two eligible items."""
    k, layers, n_user, n_item = 8, [16, 8], 6, 40
    models = [list(C.model_init(np.random.RandomState(70 + s), n_user, n_item, k, layers)) for s in range(3)]
    for U, V, dense in models:
        V[[5, 17, 29]] = V[3]                                                          # ties: four items of equal score for every user
        V[11, 0], V[12, 0], V[13, k] = np.inf, -np.inf, np.nan
        U[:, 0] = np.abs(U[:, 0]) + 0.1
    hpos = nmf.Shape(k, layers).h_at
    for _, _, dense in models:
        dense[hpos] = abs(dense[hpos]) + 0.1                                           # so that +inf * pg * h stays +inf
    models = [tuple(m) for m in models]
    users = np.array([0, 1, 2, 3, 4, 1])
    rows = [np.array([3, 4, 30]), np.arange(n_item), np.setdiff1d(np.arange(n_item), [5, 29]), np.zeros(0, int), np.array([11, 12, 13]), np.array([0])]
    off = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    excl = (off, np.concatenate(rows).astype(np.int32))
    sc = nmf.catalogue_scores_ref(models, k, layers, users, n_item)
    return k, layers, models, users, n_item, excl, sc


def test_recommend_ref_and_rank_ref_agree_with_a_lexsort_and_each_other():
    k, layers, models, users, n_item, excl, sc = oracle_case()
    assert np.isnan(sc).any() and np.isposinf(sc).any() and np.isneginf(sc).any()
    assert np.array_equal(bits(sc[:, 5]), bits(sc[:, 3])) and np.array_equal(bits(sc[:, 29]), bits(sc[:, 3]))
    uid, iid = np.repeat(users, n_item), np.tile(np.arange(n_item), len(users))
    assert np.array_equal(bits(nmf.score_ref(models, k, layers, uid, iid)), bits(sc.reshape(-1)))
    for ex in (None, excl):
        for top_k in (1, 7, 40, 64):
            s, it = nmf.recommend_ref(models, k, layers, users, n_item, top_k, ex, scores=sc)
            assert s.shape == it.shape == (len(users), top_k) and s.dtype == np.float32 and it.dtype == np.int64
            for q in range(len(users)):
                want = brute(sc[q], nmf._excl_row(ex, q))[:top_k]
                assert np.array_equal(it[q, :len(want)], want)
                assert np.array_equal(bits(s[q, :len(want)]), bits(sc[q, want]))
                assert (it[q, len(want):] == -1).all() and np.isnan(s[q, len(want):]).all()          # padding is (NaN, -1)
        # ranks of every item of every row (shuffled, with duplicates and an empty row)
        rs = np.random.RandomState(5)
        rows = [rs.permutation(np.concatenate([np.arange(n_item), [3, 3, 11]])) if q != 3 else np.zeros(0, int) for q in range(len(users))]
        t_off = np.zeros(len(users) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rows], out=t_off[1:])
        ranks = nmf.rank_ref(models, k, layers, users, (t_off, np.concatenate(rows)), ex, scores=sc, n_item=n_item)
        assert ranks.dtype == np.int32
        s, it = nmf.recommend_ref(models, k, layers, users, n_item, n_item, ex, scores=sc)
        for q in range(len(users)):
            order = brute(sc[q], nmf._excl_row(ex, q))
            place = {int(i): r for r, i in enumerate(order)}
            got = ranks[t_off[q]:t_off[q + 1]]
            assert [place.get(int(t), -1) for t in rows[q]] == got.tolist()              # an excluded target: -1; equal targets: equal ranks
            for t, r in zip(rows[q], got):
                if r >= 0:
                    assert it[q, r] == t                                             # a target of rank r < k is item r of the top-k row
    s, it = nmf.recommend_ref(models, k, layers, users, n_item, 5, excl, scores=sc)
    assert (it[1] == -1).all() and it[2].tolist() == [5, 29, -1, -1, -1]                 # everything excluded; two tied items left


def test_order_bits_is_the_kernels_order():
    s = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf], dtype=np.float32)
    b = nmf.order_bits(s)
    assert b[0] == 0 and b[3] == b[4] and (np.diff(b[[0, 1, 2, 3, 5, 6, 7]].astype(np.int64)) > 0).all()
    assert (nmf.rank_keys(s[[6, 6]], [4, 9])[0] > nmf.rank_keys(s[[6, 6]], [4, 9])[1])          # ties: the smaller id is better


# ------------------------------------------------------------------ 3. header, binding, library, build list
def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_nmf_rank.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.NMF_RANK_EXPORTS) and len(declared) == 4
    for other in (nv.EXPORTS, nv.CSR_PAIR_EXPORTS, nv.GCN_EXPORTS, nv.BPR_EXPORTS, nv.INF_EXPORTS, nv.NMF_EXPORTS):
        assert not declared & set(other)
    assert len(nv.EXPORTS) == 96 and len(nv.NMF_EXPORTS) == 6
    assert '#include "ultrare_nmf_rank.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    L = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
        assert getattr(nv.lib(), name).argtypes == nv._NMF_RANK_PROTOTYPES[name][1]
    from ultrare_amd import build
    assert 'nmf_rank.hip' in build.SOURCES and 'nmf_rank.hip' not in build.STEP_KERNEL_FILES
    assert "'ultrare_nmf_rank.h'" in inspect.getsource(build.source_hash)
    for name, (res, args) in nv._NMF_RANK_PROTOTYPES.items():
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    assert nmf.RANK_LDS_BYTES == int(re.search(r'#define URE_NMF_RANK_LDS_BYTES (\d+)', header).group(1))


def test_every_admitted_stack_fits_a_workgroup(nv):
    """The header's LDS formula over every stack check_layers admits: a plan exists for the widest selection state (top_k = 128) and
    for the counting state, one-layer stacks run at QW = 4, and the library's sizers agree on a sample that includes the widest."""
    widths = [4, 8, 16, 32, 64, 128]
    admitted = []
    for k in widths:
        for m in range(1, nmf.MAX_FC + 1):
            for rest in itertools.product(widths, repeat=m):
                for L0 in widths[1:]:
                    if nmf.lds_bytes(k, [L0, *rest]) <= nmf.LDS_BYTES:
                        admitted.append((k, [L0, *rest]))
    assert (128, [128, 64]) in admitted and (16, [32, 128, 64, 4]) in admitted and len(admitted) > 1000
    narrow = set()
    for k, layers in admitted:
        for top_k in (128, None):
            plan = nmf.rank_plan(k, layers, top_k)
            assert plan is not None, (k, layers, top_k)
            assert len(layers) > 2 or plan == (4, 0), (k, layers, top_k)
            narrow.add(plan)
    assert (1, 1) in narrow or (1, 2) in narrow                                          # some stack does need the narrow passes
    L = nv.lib()
    for k, layers in [(128, [128, 64]), (16, [32, 128, 64, 4]), (16, [8, 64, 128, 4]), (32, [64, 32]), (16, [16, 8, 8, 4, 4]), (4, [8, 4])]:
        assert (k, layers) in admitted
        lay = np.array(layers, np.int32)
        assert L.ure_nmf_recommend_scratch(5, 100, 128, 2, k, nv.ptr(lay), len(lay)) == 0
        assert L.ure_nmf_rank_pairs_scratch(5, 7, 100, 2, k, nv.ptr(lay), len(lay)) == 7 * 24
    lay = np.array([64, 32], np.int32)
    assert L.ure_nmf_recommend_scratch(3, 1100, 10, 2, 32, nv.ptr(lay), 2) == L.ure_recommend_scratch(3, 1100, 10) == 3 * 2 * 10 * 12


# ------------------------------------------------------------------ 4. argument checks before any HIP call
BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.addressof(BUF)
LAY = np.array([8, 4], np.int32)
BAD_LAY = np.array([8, 3], np.int32)
TABS = (ctypes.c_void_p * 2)(P, P + 4096)
NULL_TAB = (ctypes.c_void_p * 2)(P, None)

ORDER = dict(
    ure_nmf_recommend_topk=('Us', 'Vs', 'Ds', 'n_models', 'k', 'layers', 'n_layers', 'n_user', 'users', 'n_query', 'n_item', 'excl_off', 'excl_items', 'top_k',
                            'scores', 'items', 'scratch', 'bytes', 'stream'),
    ure_nmf_rank_pairs=('Us', 'Vs', 'Ds', 'n_models', 'k', 'layers', 'n_layers', 'n_user', 'users', 'n_query', 'n_item', 'tgt_off', 'tgt_items', 'excl_off',
                        'excl_items', 'ranks', 'scratch', 'bytes', 'stream'),
    ure_nmf_recommend_scratch=('n_query', 'n_item', 'top_k', 'n_models', 'k', 'layers', 'n_layers'),
    ure_nmf_rank_pairs_scratch=('n_query', 'n_targets', 'n_item', 'n_models', 'k', 'layers', 'n_layers'))
# 3 users over 2000 items: two item splits, so the top-k entry needs scratch
BASE = dict(Us=TABS, Vs=TABS, Ds=TABS, n_models=2, k=4, layers=LAY.ctypes.data, n_layers=2, n_user=4, users=P, n_query=3, n_item=2000, excl_off=None,
            excl_items=None, top_k=10, scores=P + 32768, items=P + 36864, scratch=P + 40960, bytes=1 << 13, stream=None, tgt_off=P, tgt_items=P,
            ranks=P + 32768, n_targets=5)


def _bad_calls():
    call = lambda entry, **kw: (entry, [{**BASE, **kw}[name] for name in ORDER[entry]])
    rec, rank = (functools.partial(call, entry) for entry in ('ure_nmf_recommend_topk', 'ure_nmf_rank_pairs'))
    both = [dict(k=3), dict(layers=BAD_LAY.ctypes.data), dict(layers=None), dict(n_layers=1), dict(n_layers=6), dict(n_models=0), dict(Us=None),
            dict(Ds=None), dict(Vs=NULL_TAB), dict(Ds=NULL_TAB), dict(users=None), dict(n_query=0), dict(n_item=0), dict(n_user=0), dict(n_user=1 << 31),
            dict(excl_off=P), dict(excl_items=P)]
    return [f(**kw) for f in (rec, rank) for kw in both] + \
        [rec(top_k=0), rec(top_k=129), rec(scores=None), rec(items=None), rec(bytes=16), rec(scratch=None),
         rank(tgt_off=None), rank(tgt_items=None), rank(ranks=None), rank(bytes=-1), rank(scratch=None)]


@pytest.mark.parametrize('entry,args', _bad_calls(), ids=lambda v: v if isinstance(v, str) else '')
def test_entries_check_their_arguments_before_any_hip_call(nv, entry, args):
    """Through ctypes on a machine without a device: -1 and the check's own message, and the 'device' memory is untouched."""
    ctypes.memset(P, 0x5A, len(BUF))
    assert getattr(nv.lib(), entry)(*args) == -1
    assert b'argument check failed' in nv.lib().ure_last_error()
    assert BUF.raw == b'\x5a' * len(BUF)


def test_short_scratch_is_what_the_sizer_says(nv):
    need = nv.lib().ure_nmf_recommend_scratch(3, 2000, 10, 2, 4, LAY.ctypes.data, 2)
    assert need == 3 * 3 * 10 * 12 and need > 16                      # three splits of 3 x 10 (key, score) entries


def test_sizers_refuse_what_the_entries_refuse(nv):
    L = nv.lib()
    call = lambda entry, **kw: getattr(L, entry)(*[{**BASE, **kw}[name] for name in ORDER[entry]])
    for entry in ('ure_nmf_recommend_scratch', 'ure_nmf_rank_pairs_scratch'):
        assert call(entry) >= 0
        for kw in (dict(k=3), dict(layers=BAD_LAY.ctypes.data), dict(layers=None), dict(n_layers=1), dict(n_layers=6), dict(n_models=0), dict(n_query=0),
                   dict(n_item=0)):
            assert call(entry, **kw) == -1, (entry, kw)
    assert call('ure_nmf_recommend_scratch', top_k=0) == -1 and call('ure_nmf_recommend_scratch', top_k=129) == -1
    assert call('ure_nmf_rank_pairs_scratch', n_targets=-1) == -1 and call('ure_nmf_rank_pairs_scratch', n_targets=1 << 31) == -1
    assert call('ure_nmf_rank_pairs_scratch', n_targets=0) == 0


# ------------------------------------------------------------------ 5. the surface without a device
def _cpu_model(k=8, layers=(16, 8), seed=0):
    from ultrare_amd.method.utils import NMF, seed_all
    seed_all(seed)
    return NMF(11, 7, k, list(layers))


def test_surface_refuses_mixed_backbones_mixed_stacks_and_cpu_tensors():
    from ultrare_amd import _native, engine, ops  # noqa: F401
    from ultrare_amd.config import InsParam
    from ultrare_amd.method import sisa, utils
    m, other, mf = _cpu_model(), _cpu_model(8, (16, 4)), utils.MF(11, 7, 8)
    loader = (np.array([0, 1]), np.array([0, 1]), np.array([0.2, 0.4], np.float32))
    for who, call in (('recommend_nmf', lambda ms: utils.recommend_nmf(ms, [0, 1])), ('rank_eval_nmf', lambda ms: utils.rank_eval_nmf(ms, loader))):
        with pytest.raises(ValueError, match=who + ".*'nmf' backbone only, not MF"):
            call([m, mf])
        with pytest.raises(ValueError, match=who + '.*share one stack'):
            call([m, other])
        with pytest.raises(ValueError, match=who + ' needs at least one model'):
            call([])
        with pytest.raises(_native.NativeError, match='HIP device'):
            call([m, m])
    p = InsParam('toy', 2, data_dir=os.path.join(ROOT, 'tests', 'golden'), model='nmf', layers=[16, 8], k=8)
    s = sisa.Sisa(p, 'nmf', 2, [[0], [1]])
    s.model_list = [m, m]
    with pytest.raises(_native.NativeError, match='HIP device'):
        s.recommend_nmf([0])
    with pytest.raises(_native.NativeError, match='HIP device'):
        s.rank_eval_nmf(loader)
    s.model_list = [m, mf]
    with pytest.raises(ValueError, match="recommend_nmf.*'nmf' backbone only"):
        s.recommend_nmf([0])
    # the engine calls and the operators
    S = nmf.Shape(8, [16, 8])
    z = torch.zeros
    cpu = (z(3, S.wd), z(4, S.wd), z(S.n_dense))
    tgt = (np.array([0, 1, 1]), np.array([2]))
    with pytest.raises(_native.NativeError, match='nmf_recommend runs on the HIP device only'):
        engine.nmf_recommend([cpu], 8, [16, 8], [0, 1], 3)
    with pytest.raises(_native.NativeError, match='nmf_rank_pairs runs on the HIP device only'):
        engine.nmf_rank_pairs([cpu], 8, [16, 8], [0, 1], tgt)
    for call in (lambda: engine.nmf_recommend([cpu], 8, [16, 6], [0], 3), lambda: engine.nmf_rank_pairs([cpu], 8, [16, 6], [0], tgt),
                 lambda: engine.nmf_recommend([], 8, [16, 8], [0], 3)):
        with pytest.raises(ValueError, match='nmf'):
            call()
    lists = ([cpu[0]], [cpu[1]], [cpu[2]])
    users, off, items = z(2, dtype=torch.int64), torch.tensor([0, 1, 1]), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        torch.ops.ultrare.nmf_recommend_topk(*lists, 8, [16, 8], users, None, None, 3)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        torch.ops.ultrare.nmf_rank_pairs(*lists, 8, [16, 8], users, off, items, None, None)
    with pytest.raises(ValueError, match='nmf'):
        torch.ops.ultrare.nmf_recommend_topk(*lists, 8, [16, 6], users, None, None, 3)
    with pytest.raises(ValueError, match='nmf'):
        torch.ops.ultrare.nmf_rank_pairs(*lists, 8, [16, 6], users, off, items, None, None)
