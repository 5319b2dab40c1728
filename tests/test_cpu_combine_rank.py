"""Ranking under the learned shard combiner without a device: the numpy contract (combine.weighted_scores_ref, recommend_ref,
rank_ref) on hand-made score matrices, the C ABI's bookkeeping (include/ultrare_combine_rank.h) and the refusals of every layer
of the surface, each raised before a device is needed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ultrare_amd import combine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


def csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)


# ------------------------------------------------------------------ 1. the score
def test_weight_rows_resolve_the_group_map():
    W = np.array([[1.0, 2.0, 0.5], [3.0, 4.0, -0.5]])
    rows, outside = combine.weight_rows(W, [0, 1, 2, 3, 9, -1], [1, 0, -1, 2])
    assert outside.tolist() == [False, False, True, True, True, True]                 # -1, a group that is not there, ids outside the map
    assert rows[:2].tolist() == [W[1].tolist(), W[0].tolist()] and (rows[2:] == [0.5, 0.5, 0.0]).all()
    rows, outside = combine.weight_rows(W, [5, 0], None)                                # no map: row 0 for everybody
    assert not outside.any() and (rows == W[0]).all()


def test_weighted_scores_are_the_rounded_chain():
    P = np.array([[0.1, 0.7], [-0.0, -0.0], [3.0, -2.0]], dtype=np.float32)
    rows = np.array([[0.25, 0.75, 0.1], [-1.0, -1.0, -0.0], [1e10, 1e10, 0.0]])
    z = [np.float64(0.1) + 0.25 * np.float64(P[0, 0]), None, None]
    z[0] = z[0] + 0.75 * np.float64(P[0, 1])
    got = combine.weighted_scores_ref(P, 0, rows)
    assert got.dtype == np.float32 and got[0] == np.float32(z[0])
    # p = 0.f + score: a score of -0.0 enters as +0.0, so -1 * p is -0.0 and b + that is b's own zero ... -0.0 + -0.0 + -0.0
    assert np.signbit(got[1]) and got[1] == 0
    assert np.signbit(combine.weighted_scores_ref(P[1:2], 0, np.array([[1.0, 1.0, 0.0]])))[0] == False   # noqa: E712  (+0.0, not the -0.0 of w * -0.0)
    lg = combine.weighted_scores_ref(P, 'logistic', rows)
    assert lg[2] == np.float32(1.0) and lg[1] == np.float32(0.5) and abs(lg[0] - 1 / (1 + np.exp(-z[0]))) < 1e-7
    assert combine.weighted_scores_ref(P, 1, -rows)[2] == 0.0                           # exp overflows: 1 / inf
    out = combine.weighted_scores_ref(P, 1, rows, outside=np.array([False, True, False]))
    assert np.isnan(out[1]) and not np.isnan(out[[0, 2]]).any()
    assert not np.isnan(combine.weighted_scores_ref(P, 0, rows, outside=np.array([False, True, False]))).any()


# ------------------------------------------------------------------ 2. the order and the ranks, on hand-made matrices
SC = np.array([[0.5, 1.0, 1.0, np.nan, -np.inf, 0.0, -0.0, 1.0],
               [np.nan, np.nan, 2.0, 2.0, -1.0, np.inf, 1e-45, 2.0]], dtype=np.float32)


def test_order_ties_by_item_id_nan_last_and_signed_zeros_equal():
    s, it = combine.recommend_ref(SC, 8)
    assert it[0].tolist() == [1, 2, 7, 0, 5, 6, 4, 3]                                  # 1.0 x 3 by id, 0.0 == -0.0 by id, -inf, NaN
    assert it[1].tolist() == [5, 2, 3, 7, 6, 4, 0, 1]                                  # the two NaN by id at the end
    assert np.array_equal(s.view(np.int32), np.take_along_axis(SC, it, axis=1).view(np.int32))
    assert it.dtype == np.int64 and s.dtype == np.float32


def test_padding_and_exclusion():
    excl = csr([[1, 2, 7, 0, 5, 6], [5]])
    s, it = combine.recommend_ref(SC, 4, excl)
    assert it[0].tolist() == [4, 3, -1, -1] and np.isnan(s[0, 1:]).all() and s[0, 0] == -np.inf
    assert it[1].tolist() == [2, 3, 7, 6]
    s, it = combine.recommend_ref(SC, 3, csr([np.arange(8), []]))
    assert it[0].tolist() == [-1, -1, -1] and np.isnan(s[0]).all()


def test_ranks_count_the_better_keys_and_agree_with_the_order():
    targets = csr([[7, 1, 1, 3, 6, 5], []])
    assert combine.rank_ref(SC, targets).tolist() == [2, 0, 0, 7, 5, 4]                 # duplicates, the NaN last, -0.0 behind 0.0 by id
    excl = csr([[1, 5], [2]])
    assert combine.rank_ref(SC, targets, excl).tolist() == [1, -1, -1, 5, 3, -1]       # excluded targets, and excluded items do not count
    assert combine.rank_ref(SC, csr([[], []])).tolist() == []
    rs = np.random.RandomState(0)
    sc = rs.randint(0, 6, (5, 40)).astype(np.float32)                                   # many ties
    sc[rs.random_sample(sc.shape) < 0.1] = np.nan
    ex = csr([np.flatnonzero(rs.random_sample(40) < 0.2) for _ in range(5)])
    tg = csr([rs.randint(0, 40, 12) for _ in range(5)])
    for e in (None, ex):
        r = combine.rank_ref(sc, tg, e)
        _, it = combine.recommend_ref(sc, 16, e)
        row = np.repeat(np.arange(5), np.diff(tg[0]))
        low = (r >= 0) & (r < 16)
        assert low.sum() > 10 and np.array_equal(it[row[low], r[low]], tg[1][low])       # a target of rank r < k is item r of the row
        if e is not None:
            hit = np.array([t in e[1][e[0][q]:e[0][q + 1]] for q, t in zip(row, tg[1])])
            assert np.array_equal(r < 0, hit)


# ------------------------------------------------------------------ 3. header, binding, library, build list
def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_combine_rank.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.COMBINE_RANK_EXPORTS) == {'ure_recommend_weighted_scratch', 'ure_recommend_topk_weighted',
                                                        'ure_rank_pairs_weighted_scratch', 'ure_rank_pairs_weighted'}
    for other in (nv.EXPORTS, nv.CSR_PAIR_EXPORTS, nv.GCN_EXPORTS, nv.BPR_EXPORTS, nv.INF_EXPORTS, nv.NMF_EXPORTS, nv.NMF_RANK_EXPORTS):
        assert not declared & set(other)
    assert '#include "ultrare_combine_rank.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    L = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
        assert getattr(nv.lib(), name).argtypes == nv._COMBINE_RANK_PROTOTYPES[name][1]
    from ultrare_amd import build
    assert 'mf_combine_rank.hip' in build.SOURCES and 'mf_combine_rank.hip' not in build.STEP_KERNEL_FILES
    assert "'ultrare_combine_rank.h'" in inspect.getsource(build.source_hash)
    for name, (res, args) in nv._COMBINE_RANK_PROTOTYPES.items():
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    # the arguments are the mean entries' followed by the combiner's five
    for mean, weighted in (('ure_recommend_topk', 'ure_recommend_topk_weighted'), ('ure_rank_pairs', 'ure_rank_pairs_weighted')):
        assert nv._COMBINE_RANK_PROTOTYPES[weighted][1][:-5] == nv._PROTOTYPES[mean][1]


def test_the_lds_sum_of_the_header():
    """The header's table: tile + weight rows + selection or counting state at every width, within the workgroup's 160 KiB."""
    header = open(os.path.join(ROOT, 'include', 'ultrare_combine_rank.h')).read()
    limit = int(re.search(r'#define URE_COMBINE_RANK_LDS_BYTES (\d+)', header).group(1))
    assert limit == 160 * 1024
    worst = {}
    for d in (4, 8, 16, 32, 64, 128, 256):
        QT = 16 if d == 256 else 32
        tile, rows = 4 * (QT * d + 64 * (d + 4)), QT * (33 * 8 + 4)
        worst[d] = (tile + rows + QT * (12 * (128 + 64) + 272), tile + rows + 49152 + 12 * QT)
        assert max(worst[d]) <= limit and (tile + rows) % 16 == 0
    assert worst[128][0] == 141184 and worst[256][1] == 136576 and max(max(v) for v in worst.values()) == 141184
    assert '141,184' in header and '136,576' in header


# ------------------------------------------------------------------ 4. argument checks before any HIP call
BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.addressof(BUF)
TABS = (ctypes.c_void_p * 2)(P, P + 4096)
NULL_TAB = (ctypes.c_void_p * 2)(P, None)
MANY = (ctypes.c_void_p * 33)(*[P] * 33)

ORDER = dict(
    ure_recommend_topk_weighted=('Us', 'Vs', 'n_models', 'users', 'n_query', 'n_item', 'd', 'excl_off', 'excl_items', 'k', 'scores', 'items', 'scratch',
                                 'bytes', 'stream', 'link', 'W', 'n_groups', 'gou', 'n_user'),
    ure_rank_pairs_weighted=('Us', 'Vs', 'n_models', 'users', 'n_query', 'n_item', 'd', 'tgt_off', 'tgt_items', 'excl_off', 'excl_items', 'ranks',
                             'scratch', 'bytes', 'stream', 'link', 'W', 'n_groups', 'gou', 'n_user'),
    ure_recommend_weighted_scratch=('n_query', 'n_item', 'k', 'd', 'n_models', 'link', 'n_groups'),
    ure_rank_pairs_weighted_scratch=('n_query', 'n_targets', 'n_item', 'd', 'n_models', 'link', 'n_groups'))
# 3 users over 2000 items: three item splits, so the top-k entry needs scratch
BASE = dict(Us=TABS, Vs=TABS, n_models=2, users=P, n_query=3, n_item=2000, d=8, excl_off=None, excl_items=None, k=10, scores=P + 32768,
            items=P + 36864, scratch=P + 40960, bytes=1 << 13, stream=None, link=1, W=P, n_groups=2, gou=P, n_user=4, tgt_off=P, tgt_items=P,
            ranks=P + 32768, n_targets=5)
REFUSED = [dict(n_models=0), dict(n_models=33, Us=MANY, Vs=MANY), dict(link=2), dict(link=-1), dict(d=6), dict(d=512), dict(d=2), dict(n_groups=0)]


def _bad_calls():
    call = lambda entry, **kw: (entry, [{**BASE, **kw}[name] for name in ORDER[entry]])
    both = REFUSED + [dict(W=None), dict(n_user=0), dict(Us=None), dict(Vs=NULL_TAB), dict(users=None), dict(n_query=0), dict(n_item=0), dict(excl_off=P),
                      dict(excl_items=P)]
    rec, rank = (lambda **kw: call('ure_recommend_topk_weighted', **kw)), (lambda **kw: call('ure_rank_pairs_weighted', **kw))
    return [f(**kw) for f in (rec, rank) for kw in both] + \
        [rec(k=0), rec(k=129), rec(scores=None), rec(items=None), rec(bytes=16), rec(scratch=None),
         rank(tgt_off=None), rank(tgt_items=None), rank(ranks=None), rank(bytes=-1), rank(scratch=None)]


@pytest.mark.parametrize('entry,args', _bad_calls(), ids=lambda v: v if isinstance(v, str) else '')
def test_entries_check_their_arguments_before_any_hip_call(nv, entry, args):
    """Through ctypes on a machine without a device: -1 and the check's own message, and the 'device' memory is untouched."""
    ctypes.memset(P, 0x5A, len(BUF))
    assert getattr(nv.lib(), entry)(*args) == -1
    assert b'argument check failed' in nv.lib().ure_last_error()
    assert BUF.raw == b'\x5a' * len(BUF)


def test_sizers_refuse_what_the_entries_refuse(nv):
    L = nv.lib()
    call = lambda entry, **kw: getattr(L, entry)(*[{**BASE, **kw}[name] for name in ORDER[entry]])
    assert call('ure_recommend_weighted_scratch') == L.ure_recommend_scratch(3, 2000, 10) == 3 * 3 * 10 * 12
    assert call('ure_rank_pairs_weighted_scratch') == L.ure_rank_pairs_scratch(3, 5, 2000, 8) == 5 * 24
    for entry in ('ure_recommend_weighted_scratch', 'ure_rank_pairs_weighted_scratch'):
        for kw in REFUSED + [dict(n_query=0), dict(n_item=0)]:
            kw = {k: v for k, v in kw.items() if k not in ('Us', 'Vs')}
            assert call(entry, **kw) == -1, (entry, kw)
        for d in (4, 8, 16, 32, 64, 128, 256):                                          # every width the mean route serves, at the widest state
            assert call(entry, d=d, k=128, n_models=32) >= 0, (entry, d)
    assert call('ure_recommend_weighted_scratch', k=0) == -1 and call('ure_recommend_weighted_scratch', k=129) == -1
    assert call('ure_rank_pairs_weighted_scratch', n_targets=-1) == -1 and call('ure_rank_pairs_weighted_scratch', n_targets=1 << 31) == -1
    assert call('ure_rank_pairs_weighted_scratch', n_targets=0) == 0


# ------------------------------------------------------------------ 5. the surface without a device
def _mf(n_user=11, n_item=7, k=8, seed=0):
    from ultrare_amd.method.utils import MF, seed_all
    seed_all(seed)
    return MF(n_user, n_item, k)


LOADER = (np.array([0, 1, 10]), np.array([0, 1, 2]), np.array([0.2, 0.4, 1.0], np.float32))


def _loader():
    from ultrare_amd.read import RatingData, loadData
    return loadData(RatingData(np.stack([a.astype(np.float64) for a in LOADER])), 10, 24, False)


def test_utils_refuse_before_any_device_work():
    from ultrare_amd import _native
    from ultrare_amd.method import utils
    models = [_mf(seed=s) for s in range(3)]                                            # CPU tables: anything that reaches the device path raises NativeError
    W3 = np.tile(combine.mean_weights(3), (2, 1))
    groups = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]                                          # user 10 is in no group
    lin, log = combine.Combiner(W3, 'linear', groups), combine.Combiner(W3, 'logistic', groups)
    two = combine.Combiner(np.tile(combine.mean_weights(2), (2, 1)), 'linear', groups)
    loader = _loader()
    for call in (lambda c, users=(0, 1): utils.recommend(models, list(users), 3, combiner=c), lambda c, users=None: utils.rank_eval(models, loader, combiner=c)):
        with pytest.raises(ValueError, match='fitted on 2 models, not 3'):
            call(two)
        with pytest.raises(_native.NativeError, match='HIP device'):                    # the linear link takes user 10: only the device is missing
            call(lin, (0, 10))
    with pytest.raises(ValueError, match=r"1 of 2 query users are in no group \(the first: 10\): link='logistic'"):
        utils.recommend(models, [0, 10], 3, combiner=log)
    with pytest.raises(ValueError, match="query users are in no group.*link='logistic'"):
        utils.rank_eval(models, loader, combiner=log)                                   # the loader's users are 0, 1 and 10
    with pytest.raises(_native.NativeError, match='HIP device'):
        utils.recommend(models, [0, 9], 3, combiner=log)                                # query users inside the groups: user 10 is not asked about
    with pytest.raises(_native.NativeError, match='HIP device'):
        utils.recommend(models, [0, 10], 3)                                             # no combiner: today's route


def test_utils_refuse_neumf_by_name():
    from ultrare_amd.method import utils
    from ultrare_amd.method.utils import NMF, seed_all
    seed_all(0)
    nm = [NMF(11, 7, 8, [16, 8]) for _ in range(2)]
    c = combine.Combiner(np.tile(combine.mean_weights(2), (1, 1)), 'linear')
    with pytest.raises(ValueError, match="recommend.*'nmf' backbone"):
        utils.recommend(nm, [0], 3, combiner=c)
    with pytest.raises(ValueError, match="rank_eval.*'nmf' backbone"):
        utils.rank_eval(nm, _loader(), combiner=c)


def test_sisa_needs_a_fitted_combiner():
    from ultrare_amd import _native
    from ultrare_amd.config import InsParam
    from ultrare_amd.method import sisa
    p = InsParam('toy', 2, data_dir=os.path.join(ROOT, 'tests', 'golden'), k=8)
    s = sisa.Sisa(p, 'mf', 2, [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10]])
    s.model_list = [_mf(seed=1), _mf(seed=2)]
    for call in (lambda: s.recommend([0], 3, combined=True), lambda: s.rank_eval(_loader(), combined=True)):
        with pytest.raises(ValueError, match='no combiner: call fit_combiner'):
            call()
    s.combiner = combine.Combiner(np.tile(combine.mean_weights(3), (2, 1)), 'linear', s.group_index)
    with pytest.raises(ValueError, match='fitted on 3 models, not 2'):
        s.recommend([0], 3, combined=True)
    s.combiner = combine.Combiner(np.tile(combine.mean_weights(2), (2, 1)), 'logistic', s.group_index)
    for call in (lambda: s.recommend([0], 3, combined=True), lambda: s.rank_eval(_loader(), combined=True), lambda: s.recommend([0], 3)):
        with pytest.raises(_native.NativeError, match='HIP device'):                    # every check passed: only the device is missing
            call()


def test_engine_and_ops_refuse_without_a_device():
    from ultrare_amd import _native, engine, ops  # noqa: F401
    z = torch.zeros
    cpu = [(z(3, 8), z(4, 8))]
    W = z(1, 2, dtype=torch.float64)
    tgt = (np.array([0, 1, 1]), np.array([2]))
    with pytest.raises(_native.NativeError, match='recommend runs on the HIP device only'):
        engine.recommend(cpu, 8, [0, 1], 3, weights=(0, W, None))
    with pytest.raises(_native.NativeError, match='rank_pairs runs on the HIP device only'):
        engine.rank_pairs(cpu, 8, [0, 1], tgt, weights=(0, W, None))
    users, off, items = z(2, dtype=torch.int64), torch.tensor([0, 1, 1]), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        torch.ops.ultrare.recommend_topk_weighted([cpu[0][0]], [cpu[0][1]], users, None, None, 3, 0, W, None)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        torch.ops.ultrare.rank_pairs_weighted([cpu[0][0]], [cpu[0][1]], users, off, items, None, None, 0, W, None)
    # the fake kernels give the shapes and dtypes of the real ones
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        U, V, Wf = torch.empty(5, 8), torch.empty(9, 8), torch.empty(1, 2, dtype=torch.float64)
        s, it = torch.ops.ultrare.recommend_topk_weighted([U], [V], torch.empty(4, dtype=torch.int64), None, None, 3, 1, Wf, None)
        assert s.shape == it.shape == (4, 3) and s.dtype == torch.float32 and it.dtype == torch.int64
        r = torch.ops.ultrare.rank_pairs_weighted([U], [V], torch.empty(4, dtype=torch.int64), torch.empty(5, dtype=torch.int64),
                                                  torch.empty(6, dtype=torch.int32), None, None, 1, Wf, None)
        assert r.shape == (6,) and r.dtype == torch.int32
