"""Exact full-catalogue ranks, host side (-m "not gpu"): the C ABI rejects bad arguments before any HIP call, its scratch grows
with the targets and never with the catalogue, the Python layer refuses CPU models and malformed input before any device
work, and the metric reduction equals a plain per-user loop.  Nothing here initialises HIP."""
import ctypes
import math

import numpy as np
import pytest
import torch


@pytest.fixture(scope='session')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


def _call(nv, n_models=2, users_n=4, n_item=100, d=16, tgt_off=True, tgt_items=True, ranks=True, excl_off=True, excl_items=True,
          scratch=True, scratch_bytes=1 << 20, tables=True):
    L = nv.lib()
    fake = ctypes.c_void_p(0x1000)                    # never dereferenced: every check fails before the device is touched
    tabs = (ctypes.c_void_p * max(n_models, 1))(*([0x2000 if tables else 0] * max(n_models, 1)))
    return L.ure_rank_pairs(tabs, tabs, n_models, fake, users_n, n_item, d, fake if tgt_off else None, fake if tgt_items else None,
                            fake if excl_off else None, fake if excl_items else None, fake if ranks else None, fake if scratch else None,
                            scratch_bytes, None)


@pytest.mark.parametrize('kw,word', [({'n_models': 0}, 'n_models >= 1'), ({'users_n': 0}, 'n_query >= 1'), ({'n_item': 0}, 'n_item >= 1'),
                                     ({'d': 12}, 'pow2(d)'), ({'d': 2}, 'd >= 4'), ({'d': 512}, 'd <= 256'),
                                     ({'tgt_off': False}, 'tgt_off'), ({'tgt_items': False}, 'tgt_items'), ({'ranks': False}, 'ranks'),
                                     ({'excl_items': False}, 'excl_off == nullptr'), ({'excl_off': False}, 'excl_off == nullptr'),
                                     ({'scratch_bytes': -1}, 'scratch_bytes >= 0'), ({'scratch': False}, 'scratch_bytes == 0 || scratch'),
                                     ({'tables': False}, 'U_tables[m] && V_tables[m]')])
def test_rank_pairs_rejects_bad_arguments(nv, kw, word):
    rc = _call(nv, **kw)
    assert rc == -1
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


def test_scratch_grows_with_targets_not_items(nv):
    L = nv.lib()
    b = L.ure_rank_pairs_scratch(4096, 200000, 60000, 128)
    assert 0 < b < 4096 * 60000 * 4 // 10
    assert L.ure_rank_pairs_scratch(4096, 200000, 600000, 128) == b          # more items: no more scratch
    assert L.ure_rank_pairs_scratch(4096, 200000, 1, 4) == b
    assert L.ure_rank_pairs_scratch(4096, 400000, 60000, 128) == 2 * b
    assert L.ure_rank_pairs_scratch(1, 0, 1, 4) == 0
    for args in [(0, 10, 100, 16), (10, -1, 100, 16), (10, 10, 0, 16), (10, 10, 100, 12), (10, 10, 100, 512), (10, 1 << 31, 100, 16)]:
        assert L.ure_rank_pairs_scratch(*args) == -1, args


def _tables():
    return [(torch.zeros(20, 8), torch.zeros(30, 8))]


def test_cpu_models_raise_before_device_work():
    from ultrare_amd import _native as nv
    from ultrare_amd import engine
    from ultrare_amd.method.utils import MF, rank_eval
    from ultrare_amd.read import RatingData, loadData
    with pytest.raises(nv.NativeError, match='HIP device'):
        engine.rank_pairs(_tables(), 8, [0, 1], (np.array([0, 1, 2]), np.array([3, 4])))
    torch.manual_seed(0)
    m = MF(20, 30, 8)
    test = loadData(RatingData([np.array([0, 1]), np.array([2, 3]), np.array([5.0, 4.0])]), 10, 0, False)
    with pytest.raises(nv.NativeError, match='HIP device'):
        rank_eval([m], test)
    assert not torch.cuda.is_initialized()


@pytest.mark.parametrize('users,targets,excl,match', [
    ([0, 20], ([0, 1, 2], [3, 4]), None, 'user ids'),
    ([-1], ([0, 1], [3]), None, 'user ids'),
    ([0, 1], ([0, 1, 2], [3, 30]), None, 'target items outside'),
    ([0, 1], ([0, 1, 2], [-1, 3]), None, 'target items outside'),
    ([0, 1], ([0, 2], [3, 4]), None, 'target offsets'),              # one row short
    ([0, 1], ([1, 1, 2], [3, 4]), None, 'target offsets'),           # does not start at 0
    ([0, 1], ([0, 2, 1], [3, 4]), None, 'target offsets'),           # decreasing, ends short
    ([0, 1], ([0, 1, 3], [3, 4]), None, 'target offsets'),           # ends past the items
    ([0, 1], ([0, 1, 2], [3, 4]), ([0, 1], [3]), 'exclusion offsets'),
    ([0, 1], ([0, 1, 2], [3, 4]), ([0, 1, 2], [3, 31]), 'exclusion items outside'),
])
def test_malformed_input_is_refused_before_device_work(users, targets, excl, match):
    from ultrare_amd import engine
    with pytest.raises(ValueError, match=match):
        engine.rank_pairs(_tables(), 8, users, tuple(np.array(x) for x in targets), None if excl is None else tuple(np.array(x) for x in excl))
    assert not torch.cuda.is_initialized()


def _loop_metrics(off, ranks, ks):
    """The definitions, one user at a time."""
    per = {f'{m}@{K}': [] for K in ks for m in ('hr', 'recall', 'ndcg')}
    per['mrr'] = []
    n_pairs = 0
    for q in range(len(off) - 1):
        r = [int(x) for x in ranks[off[q]:off[q + 1]] if x >= 0]
        if not r:
            continue
        n_pairs += len(r)
        for K in ks:
            per[f'hr@{K}'].append(1.0 if min(r) < K else 0.0)
            per[f'recall@{K}'].append(sum(x < K for x in r) / len(r))
            dcg = sum(1.0 / math.log2(x + 2) for x in r if x < K)
            idcg = sum(1.0 / math.log2(i + 2) for i in range(min(len(r), K)))
            per[f'ndcg@{K}'].append(dcg / idcg)
        per['mrr'].append(1.0 / (1 + min(r)))
    out = {k: float(np.mean(v)) for k, v in per.items()}
    out['n_users'] = len(per['mrr'])
    out['n_pairs'] = n_pairs
    return out


def test_metric_reduction_equals_a_plain_loop():
    from ultrare_amd.method.utils import rank_metrics
    rng = np.random.default_rng(0)
    sizes = [3, 0, 1, 25, 2, 4, 0, 7]
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    ranks = rng.integers(0, 40, off[-1]).astype(np.int32)
    ranks[[0, 4, 5]] = -1                  # user 2's only target excluded: the user is skipped; user 0 keeps two
    ranks[off[5]:off[6]] = -1              # user 5: all excluded
    ranks[off[3]] = 0                      # a first-place hit
    ranks[off[3] + 1] = 0                  # and an equal rank (duplicate target)
    for ks in [(10, 20), (1,), (1, 5, 100)]:   # K = 1, and K larger than every |R_u|
        got, want = rank_metrics(off, ranks, ks), _loop_metrics(off, ranks, ks)
        assert got.keys() == want.keys()
        assert got['n_users'] == want['n_users'] == 5 and got['n_pairs'] == want['n_pairs']
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
            assert isinstance(got[k], (float, int))


def test_metric_reduction_edge_values():
    from ultrare_amd.method.utils import rank_metrics
    off = np.array([0, 3, 4])
    m = rank_metrics(off, np.array([0, 1, 2, 5]), ks=(1, 3))
    assert m['hr@1'] == 0.5 and m['hr@3'] == 0.5 and m['mrr'] == (1.0 + 1.0 / 6) / 2
    assert m['recall@3'] == 0.5 and m['ndcg@3'] == 0.5 and m['recall@1'] == (1 / 3 + 0) / 2
    none = rank_metrics(np.array([0, 1]), np.array([-1]), ks=(10,))
    assert none['n_users'] == 0 and none['n_pairs'] == 0 and none['hr@10'] == 0.0


def test_relevant_pairs_are_distinct_and_grouped():
    from ultrare_amd.method.utils import relevant_pairs
    from ultrare_amd.read import RatingData, loadData
    u = np.array([5, 2, 5, 2, 5, 9])
    i = np.array([7, 3, 1, 3, 7, 0])
    users, off, items = relevant_pairs(loadData(RatingData([u, i, np.ones(6)]), 4, 0, False), 10)
    assert users.tolist() == [2, 5, 9] and off.tolist() == [0, 1, 3, 4] and items.tolist() == [3, 1, 7, 0]
