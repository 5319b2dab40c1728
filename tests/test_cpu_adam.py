"""The Adam optimizer of a training job, as far as it can be checked without a device: the numpy contract (ultrare_amd/adam.py) against
torch.optim.Adam, the per-step scalars, the pool regions, ure_job_create's refusals (all decided before the first HIP call), the
arguments of TrainJob / Scratch / InsParam / the command line, and the register report of the seven mf_adam_step_kernel instantiations."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import adam_cases as C
from ultrare_amd import adam, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from ultrare_amd import _native
    return _native


def test_scalars_are_the_float64_formulas_rounded_once():
    lr_host = np.array([1e-2 * 0.5 ** (e // 2) for e in range(5)], dtype=np.float32)       # lr_step = 2: the schedule crosses two decay boundaries
    steps, b1, b2 = 3, 0.9, 0.999
    got = adam.adam_scalars(lr_host, steps, b1, b2)
    assert got.shape == (15, 2) and got.dtype == np.float32
    for t in range(15):
        lr = float(lr_host[t // steps])
        assert got[t, 0] == np.float32(lr / (1.0 - b1 ** (t + 1)))
        assert got[t, 1] == np.float32(math.sqrt(1.0 - b2 ** (t + 1)))
    assert len(set(lr_host.tolist())) == 3


def test_update_ref_is_float32_and_keeps_padding_zero():
    w = np.array([0.0, 1.5, -2.0], dtype=np.float32)
    z = np.zeros(3, dtype=np.float32)
    w1, m1, v1 = adam.adam_update_ref(w, z, z, z, 0.1, 0.9, 0.999, 1e-8, 1e-2, 0.03)
    assert w1.dtype == m1.dtype == v1.dtype == np.float32
    assert w1[0] == 0 and m1[0] == 0 and v1[0] == 0            # g = 0: 0 / eps = 0
    assert w1[1] < w[1] and w1[2] > w[2]                       # decay towards zero
    ep = adam.decay_rows_ref(w, np.array([1e-2, 5e-3], dtype=np.float32), 3, 0.1)
    assert len(ep) == 2 and all(a.dtype == np.float32 for e in ep for a in e)


@pytest.mark.parametrize('case', C.WHOLE_STEP_CASES, ids=repr)
def test_contract_equals_torch_adam_in_float64(case):
    """float64 against float64: rounding is 1e-16; the margin covers Adam's amplification where |g| is small and sits three orders
    below the float32 effects tests/test_gpu_adam.py measures."""
    U, V, loss = C.reference(case)['f64']
    Ut, Vt, loss_t = C.torch_adam(case, torch.float64)
    assert np.abs(U - Ut).max() <= 1e-9 and np.abs(V - Vt).max() <= 1e-9
    assert np.abs(loss / loss_t - 1.0).max() <= 1e-9


@pytest.mark.parametrize('case', C.WHOLE_STEP_CASES, ids=repr)
def test_cases_leave_out_at_most_one_percent_and_have_both_kinds_of_rows(case):
    assert C.reference(case)['left_out'] <= C.LEAVE_OUT_CAP
    # the hot item's row takes several work units of 8 * lanes slots at the case's width, some other row exactly one
    unit = 8 * (case.d // 4 if case.d <= 32 else case.d // 8)
    nnz = np.bincount(case.iid, minlength=case.n_item)
    per_user = np.bincount(case.uid, minlength=case.n_user)
    assert nnz[-1] > unit and ((per_user > 0) & (per_user <= unit)).any()


def test_contract_in_float32_is_as_close_as_torch_in_float32():
    """The float32 restatement of whole training (adam_update_ref in a loop) against the same float64 run: within the yardstick the GPU
    test holds the kernel to."""
    case = C.WHOLE_STEP_CASES[0]
    ref = C.reference(case)
    U, V, loss, _, _ = adam.adam_train_ref(case.uid, case.iid, case.rating, case.U0, case.V0, case.orders, case.B, case.lr_host, C.LAM, C.BETAS, C.EPS,
                                           dtype=np.float32)
    assert U.dtype == np.float32
    wmax = max(np.abs(ref['f64'][0]).max(), np.abs(ref['f64'][1]).max())
    assert C.distance(ref, U, V, loss) <= 4 * max(ref['E_t'], C.ulp32(wmax))


def test_regions_without_adam_are_todays_and_with_it_only_grow():
    args = (5, 6, 4, 8, 4)
    for lazy in (True, False):
        for snaps in (False, 'full', 'compact'):
            old = engine.shard_regions(*args, lazy, snaps, 64, 128)
            assert engine.shard_regions(*args, lazy, snaps, 64, 128, adam=False) == old
            pool, snap, end, snap_end = engine.shard_regions(*args, lazy, snaps, 64, 128, adam=True)
            assert list(pool) == list(old[0]) + ['vU', 'vV']
            assert all(pool[n] == old[0][n] for n in old[0]) and (snap, snap_end) == (old[1], old[3])
            assert pool['vU'] == (old[2], 40, (5, 8)) and pool['vV'] == (old[2] + 64, 48, (6, 8)) and end == old[2] + 128
    assert list(engine.shard_regions(*args, True, False)[0]) == ['U', 'V', 'mU', 'mV', 'sse', 'U0', 'V0']


# ure_job_create's new refusals: the base descriptor is a valid Adam shard with made-up device pointers
_BASE = dict(N=100, n_user=8, n_item=8, d=16, batch=10, epochs=2, n_active=16, n_slots=256, n_units=0, lazy_rows=0, lam=0.1, mu=0.9,
             optimizer=1, beta1=0.9, beta2=0.999, eps=1e-8)
_PTR = 0x1000
_SNAPSHOT_FIELDS = ('snapU', 'snapV', 'snap_a', 'snap', 'row_slot')
REFUSALS = [
    ('lazy_rows', [dict(lazy_rows=1)], 'lazy_rows'),
    ('touch_mode_1', [dict(touch_mode=1, lazy_rows=1)], 'touch_mode'),
    ('touch_mode_3', [dict(touch_mode=3)], 'touch_mode'),
    ('compact_snap', [dict(snap=_PTR, snap_a=_PTR, row_slot=_PTR)], 'compact snapshots'),
    ('no_vU', [dict(vU=None)], 'vU and vV'),
    ('no_vV', [dict(vV=None)], 'vU and vV'),
    ('no_opt_sc', [dict(opt_sc=None)], 'opt_sc'),
    ('beta1_is_1', [dict(beta1=1.0)], 'in [0, 1)'),
    ('beta2_negative', [dict(beta2=-0.1)], 'in [0, 1)'),
    ('beta2_nan', [dict(beta2=float('nan'))], 'in [0, 1)'),
    ('eps_zero', [dict(eps=0.0)], 'eps > 0'),
    ('optimizer_2', [dict(optimizer=2)], 'optimizer is 0'),
    ('optimizers_differ', [{}, dict(optimizer=0, lazy_rows=1)], 'shard 1: every shard of a job must ask for the same optimizer'),
    ('optimizers_differ_sgd_first', [dict(optimizer=0, lazy_rows=1), {}], 'same optimizer'),
]


def _fake_shards(lib, changes):
    arr = (lib.UreShard * len(changes))()
    lr = (ctypes.c_float * _BASE['epochs'])(*([1e-3] * _BASE['epochs']))
    for S, change in zip(arr, changes):
        for name, typ in lib.UreShard._fields_:
            if typ is ctypes.c_void_p and name not in _SNAPSHOT_FIELDS:
                setattr(S, name, _PTR)
        S.U[0] = S.U[1] = S.V[0] = S.V[1] = _PTR
        S.lr_host = ctypes.cast(lr, ctypes.c_void_p)
        for name, value in {**_BASE, **change}.items():
            setattr(S, name, value)
    return arr, lr


@pytest.mark.parametrize('changes,message', [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_job_create_refuses_by_reason(lib, changes, message):
    L = lib.lib()
    out = ctypes.c_void_p()
    arr, keep = _fake_shards(lib, changes)
    assert L.ure_job_create(arr, len(changes), ctypes.byref(out)) == -1
    err = L.ure_last_error().decode()
    assert err.startswith('ure_job_create: optimizer refused') and message in err, err
    assert not out.value


def test_descriptor_tail_matches_the_header(lib, tmp_path):
    """The appended fields of the ctypes mirror sit where the header puts them, and the ABI number did not move."""
    import subprocess
    fields = ('n_split', 'optimizer', 'beta1', 'beta2', 'eps', 'vU', 'vV', 'opt_sc')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ultrare_hip.h"\nint main(){printf("%d %zu"' + ' " %zu"' * len(fields) + \
          ', URE_ABI_VERSION, sizeof(ure_shard_t)' + ''.join(f', offsetof(ure_shard_t, {f})' for f in fields) + ');return 0;}'
    exe = str(tmp_path / 'probe')
    subprocess.run(['gcc', '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = lib.UreShard
    assert got == [15, ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert lib.ABI_VERSION == 15 and ctypes.sizeof(S) == 384


class _Shard:
    """What TrainJob reads of a shard before it refuses its arguments."""
    N, n_user, n_item, n_active, device, ready = 100, 8, 8, 16, 'cpu', None


@pytest.mark.parametrize('kw, message', [
    (dict(optimizer='adam', lazy_rows=True), 'lazy_rows'),
    (dict(optimizer='adam', touch=True), 'touch'),
    (dict(optimizer='adam', touch='index'), 'touch'),
    (dict(optimizer='adam', betas=(1.0, 0.999)), 'betas'),
    (dict(optimizer='adam', eps=0.0), 'eps'),
    (dict(optimizer='adamw'), "'sgd' or 'adam'"),
])
def test_train_job_argument_errors(kw, message):
    with pytest.raises(ValueError, match=message):
        engine.TrainJob([_Shard()], [None], [None], 16, 10, 2, 1e-3, 0.1, 0.9, **kw)


def test_optimizer_arguments_are_keyword_only():
    import inspect
    p = inspect.signature(engine.TrainJob.__init__).parameters
    assert [p[n].kind for n in ('optimizer', 'betas', 'eps')] == [inspect.Parameter.KEYWORD_ONLY] * 3
    assert (p['optimizer'].default, p['betas'].default, p['eps'].default) == ('sgd', (0.9, 0.999), 1e-8)
    assert inspect.signature(engine.shard_regions).parameters['adam'].kind == inspect.Parameter.KEYWORD_ONLY


def test_surface_names_and_defaults():
    from ultrare_amd.config import InsParam
    from ultrare_amd.main import parser
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.sisa import Sisa
    p = InsParam('toy', 2)
    assert (p.optimizer, p.lr, p.lr_decay, p.momentum, p.lam, p.k, p.batch) == ('sgd', 0.001, 0.95, 0.9, 0.1, 16, 3000)
    q = InsParam('toy', 2, optimizer='adam', lr=0.01)
    assert (q.optimizer, q.lr, q.betas, q.eps) == ('adam', 0.01, (0.9, 0.999), 1e-8)
    with pytest.raises(ValueError, match='optimizer'):
        InsParam('toy', 2, optimizer='rmsprop')
    assert Scratch(p, 'mf')._optimizer_args() == dict(optimizer='sgd', betas=(0.9, 0.999), eps=1e-8)
    assert Sisa(q, 'mf', 3, [])._optimizer_args()['optimizer'] == 'adam'
    q.optimizer = 'lamb'
    with pytest.raises(ValueError, match='optimizer'):
        Scratch(q, 'mf')
    # a param object from before the option (saved with an earlier version) trains with SGD
    del q.optimizer, q.betas, q.eps
    assert Scratch(q, 'mf').optimizer == 'sgd'
    args = parser.parse_args(['--optimizer', 'adam', '--lr', '0.01'])
    assert (args.optimizer, args.lr) == ('adam', 0.01)
    args = parser.parse_args([])
    assert (args.optimizer, args.lr) == ('sgd', None)


def test_no_adam_step_kernel_instantiation_spills(lib):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = [r for r in isa_report.kernels(lib.LIB_PATH) if r['name'].startswith('mf_adam_step_kernel<')]
    assert sorted(r['name'] for r in rows) == sorted(f'mf_adam_step_kernel<{a}, {b}>' for a, b in ((1, 1), (2, 1), (4, 1), (8, 1), (8, 2), (16, 2), (32, 2)))
    for r in rows:
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, r
