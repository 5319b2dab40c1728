"""Full-catalogue top-k recommendation, host side (-m "not gpu"): the C ABI rejects bad arguments before any HIP call, its
scratch never holds the score matrix, the exclusion rows are built right, and the Python layer refuses CPU models and
out-of-range users before any device work.  Nothing here initialises HIP."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix


@pytest.fixture(scope='session')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


def _call(nv, n_models=2, users_n=4, n_item=100, d=16, k=10, excl_off=True, excl_items=True, scratch_bytes=1 << 20):
    L = nv.lib()
    fake = ctypes.c_void_p(0x1000)                    # never dereferenced: every check fails before the device is touched
    tabs = (ctypes.c_void_p * max(n_models, 1))(*([0x2000] * max(n_models, 1)))
    return L.ure_recommend_topk(tabs, tabs, n_models, fake, users_n, n_item, d, fake if excl_off else None, fake if excl_items else None,
                                k, fake, fake, fake, scratch_bytes, None)


@pytest.mark.parametrize('kw,word', [({'k': 0}, 'k >= 1'), ({'k': 129}, 'k <= kRecMaxK'), ({'d': 12}, 'pow2(d)'),
                                     ({'n_models': 0}, 'n_models >= 1'), ({'n_item': 0}, 'n_item >= 1'),
                                     ({'excl_items': False}, 'excl_off == nullptr'), ({'scratch_bytes': 0}, 'scratch_bytes >= need')])
def test_recommend_rejects_bad_arguments(nv, kw, word):
    if 'scratch_bytes' in kw:
        kw = dict(kw, users_n=8, n_item=60000)        # several item splits: the call needs scratch
    rc = _call(nv, **kw)
    assert rc != 0
    msg = nv.lib().ure_last_error().decode()
    assert 'argument check failed' in msg and word in msg, msg


def test_scratch_never_holds_the_score_matrix(nv):
    L = nv.lib()
    b = L.ure_recommend_scratch(4096, 60000, 100)
    assert 0 <= b < 4096 * 60000 * 4 // 10
    assert L.ure_recommend_scratch(4096, 600000, 100) <= b          # more items: no more scratch
    assert L.ure_recommend_scratch(256, 60000, 128) < 256 * 60000 * 4 // 4
    assert L.ure_recommend_scratch(1, 1, 1) >= 0
    assert L.ure_recommend_scratch(10, 100, 0) < 0 and L.ure_recommend_scratch(10, 100, 129) < 0 and L.ure_recommend_scratch(0, 100, 5) < 0


def test_exclusion_rows_sort_and_follow_the_query_order():
    from ultrare_amd import engine
    # unsorted column indices inside rows (a CSR built by hand, as scipy allows)
    indptr = np.array([0, 3, 3, 6, 8])
    indices = np.array([9, 2, 5, 7, 1, 4, 3, 0])
    csr = csr_matrix((np.ones(8, dtype=np.float32), indices, indptr), shape=(4, 10))
    assert not csr.has_sorted_indices
    off, items = engine.exclusion_rows(csr, [2, 0, 1, 2, 3])
    assert off.dtype == np.int64 and items.dtype == np.int32
    assert off.tolist() == [0, 3, 6, 6, 9, 11]
    assert items.tolist() == [1, 4, 7, 2, 5, 9, 1, 4, 7, 0, 3]
    with pytest.raises(ValueError):
        engine.exclusion_rows(csr, [4])


def test_recommend_on_cpu_models_raises_before_device_work():
    from ultrare_amd import _native as nv
    from ultrare_amd.method.utils import MF, recommend
    torch.manual_seed(0)
    m = MF(20, 30, 8)
    with pytest.raises(nv.NativeError, match='HIP device'):
        recommend([m], [0, 1], 5)
    from ultrare_amd import engine
    with pytest.raises(nv.NativeError, match='HIP device'):
        engine.recommend([(torch.zeros(20, 8), torch.zeros(30, 8))], 8, [0, 1], 5)
    assert not torch.cuda.is_initialized()


@pytest.mark.parametrize('users', [[0, 20], [-1], [5, 1 << 40]])
def test_out_of_range_users_are_rejected(users):
    from ultrare_amd import engine
    with pytest.raises(ValueError, match='user ids'):
        engine.recommend([(torch.zeros(20, 8), torch.zeros(30, 8))], 8, users, 5)
    assert not torch.cuda.is_initialized()
