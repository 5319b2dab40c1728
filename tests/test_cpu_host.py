"""CPU-side tests (-m "not gpu"): the C ABI loads and exports what the header declares,
the exact OT solver (a host function of the library) against the reference's goldens,
the host logic (data plumbing, RNG stream, HBM layout building, shard placement) and
the N>1 path's host protocol over gloo with world_size 2.  No kernel is launched."""
import ctypes
import os
import re
import subprocess
import time
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
TRAIN, TEST = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
N_USER, N_ITEM = 1508, 2071


@pytest.fixture(scope='session')
def lib():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ---------------------------------------------------------------- C ABI
def test_library_exports_every_declared_symbol(lib):
    header = open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 14
    L = ctypes.CDLL(lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f'{name} declared in ultrare_hip.h but not exported'
    assert declared == set(lib.EXPORTS), declared ^ set(lib.EXPORTS)
    assert lib.lib().ure_abi_version() == lib.ABI_VERSION


def test_descriptor_struct_matches_header_layout(lib):
    """ctypes mirror of struct ure_shard: compile a probe with the real header."""
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ultrare_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu", sizeof(ure_shard_t),' \
          ' offsetof(ure_shard_t, sched), offsetof(ure_shard_t, U), offsetof(ure_shard_t, N), offsetof(ure_shard_t, lam));return 0;}'
    exe = os.path.join(ROOT, 'tests', '.abi_probe')
    subprocess.run(['gcc', '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe], input=src.encode(), check=True)
    try:
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    finally:
        os.remove(exe)
    S = lib.UreShard
    assert got == [ctypes.sizeof(S), S.sched.offset, S.U.offset, S.N.offset, S.lam.offset]


def test_no_step_kernel_instantiation_spills(lib):
    """at d = 16 (the reference's default k, config.py:19) and d = 8 the step kernel was compiled under the
    register budget tuned for d = 32 and spilled 15-16 VGPRs to scratch.  The per-width budgets (mf_train.hip: step_waves /
    step_kgb) leave none: read from the code objects' metadata notes (tools/isa_report.py), for every instantiation of
    both step kernels."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = [r for r in isa_report.kernels(lib.LIB_PATH) if 'step_kernel<' in r['name']]
    assert len([r for r in rows if r['name'].startswith('mf_step_kernel<')]) == 7
    assert len([r for r in rows if r['name'].startswith('mf_touch_step_kernel<')]) == 7
    for r in rows:
        assert r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0 and r['scratch'] == 0, r
    # and no kernel of the library at all keeps VGPRs in scratch
    assert all(r['vgpr_spill'] == 0 for r in isa_report.kernels(lib.LIB_PATH))


def test_no_kernel_is_built_in_tgsplit_mode(lib, monkeypatch):
    """csrc/perm_tags.hip's waves hand inv[] to each other through global memory with workgroup-scope release (s_waitcnt vmcnt(0)) and
    no acquire-side invalidate -- the LLVM AMDGPU memory model's sequence for NON-tgsplit mode only.  The TG_SPLIT bit of every kernel
    descriptor of the built library must be clear, and the build refuses the flag."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = isa_report.kernels(lib.LIB_PATH)
    assert any(r['name'].startswith('perm_tags_kernel') for r in rows)
    assert all(r['tg_split'] == 0 for r in rows), [r['name'] for r in rows if r['tg_split'] != 0]
    from ultrare_amd import build as lib_build
    monkeypatch.setenv('HIPCC_COMPILE_FLAGS_APPEND', '-O3 -mtgsplit')
    with pytest.raises(RuntimeError, match='tgsplit'):
        lib_build.build(timeline='/tmp/never_built.so')


def test_argument_errors_are_reported_not_crashed(lib):
    L = lib.lib()
    out = ctypes.c_void_p()
    bad = (lib.UreShard * 1)()
    assert L.ure_job_create(bad, 1, ctypes.byref(out)) != 0
    assert b'invalid descriptor' in L.ure_last_error()
    with pytest.raises(lib.NativeError):
        lib.check(L.ure_ot_assign(None, 0, 0, None, None, None), 'ure_ot_assign')


# ure_job_create's refusals: every one is decided on the host before the first HIP call, so descriptors with made-up device
# pointers reach them without a GPU.  Each case = the base descriptor plus the changes of its shards, and a part of the message.
_SNAPSHOT_FIELDS = ('snapU', 'snapV', 'snap_a', 'snap', 'row_slot')
_BASE = dict(N=100, n_user=8, n_item=8, d=16, batch=10, epochs=2, n_active=16, n_slots=256, n_units=0, lazy_rows=1, lam=0.1, mu=0.9)
_PTR = 0x1000
REFUSALS = [
    ('d_differs', [{}, dict(d=32)], 'share d'),
    ('steps_65534', [dict(N=70000, n_slots=70000, batch=1)], '70000 steps/epoch'),
    ('n_multi', [dict(touch_mode=1, n_multi=-1)], 'n_multi outside'),
    ('inv_stage', [dict(inv_stage=None)], 'lacks inv_stage'),
    ('snapU_only', [dict(snapU=_PTR)], 'incomplete snapshot set'),
    ('snap_without_snap_a', [dict(snap=_PTR)], 'incomplete snapshot set'),
    ('modes_1_0', [dict(touch_mode=1), {}], 'shard 1: every shard of a job must ask for it'),
    ('mode_4', [dict(touch_mode=4)], 'touch_mode is 0, 1, 2 or 3'),
    ('modes_1_2', [dict(touch_mode=1), dict(touch_mode=2)], 'same touch mode'),
    ('mode2_steps', [dict(touch_mode=2, batch=1)], 'at most 63 steps'),
    ('mode2_full_snapshots', [dict(touch_mode=2, snapU=_PTR, snapV=_PTR, snap_a=_PTR)], 'compact snapshots only'),
    ('mode2_row_slot', [dict(touch_mode=2, snap=_PTR, snap_a=_PTR)], 'needs row_slot'),
    ('mode3_steps', [dict(touch_mode=3, N=2000, n_slots=2000, batch=1)], 'at most 1008 steps'),
    ('mode3_n_split', [dict(touch_mode=3, n_multi=1, n_split=2)], 'n_split <= n_multi'),
    ('mode3_batch', [dict(touch_mode=3, N=300000, n_slots=300000, batch=250000)], 'at most 200,000'),
    ('mode1_lazy_rows', [dict(touch_mode=1, lazy_rows=0)], 'needs lazy_rows'),
    ('mode1_steps', [dict(touch_mode=1, N=40000, n_slots=40000, batch=1)], 'more than 32000 steps'),
    ('mode1_schedules', [dict(touch_mode=1), dict(touch_mode=1, lam=0.2)], 'schedules differ'),
]


def _fake_shards(lib, changes):
    """The base descriptor once per entry of `changes` (+ that entry's fields); -> (array, the host arrays it points to)."""
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


def test_job_create_refuses_a_zeroed_descriptor_by_name(lib):
    L = lib.lib()
    out = ctypes.c_void_p()
    assert L.ure_job_create((lib.UreShard * 1)(), 1, ctypes.byref(out)) != 0
    assert b'shard 0 has an invalid descriptor' in L.ure_last_error()


@pytest.mark.parametrize('changes,message', [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_job_create_refusal_table(lib, changes, message):
    L = lib.lib()
    out = ctypes.c_void_p()
    arr, keep = _fake_shards(lib, changes)
    assert L.ure_job_create(arr, len(changes), ctypes.byref(out)) != 0
    err = L.ure_last_error().decode()
    assert err.startswith('ure_job_create:') and message in err, err
    assert not out.value


def test_job_create_without_a_device_reports_the_hip_error(lib):
    """The valid base descriptor passes every check; on a host without a device the first HIP call fails, and the half-made job
    is taken apart the same way a refused one is."""
    if torch.cuda.is_available():
        pytest.skip('a device is visible: the made-up pointers must not reach it')
    L = lib.lib()
    out = ctypes.c_void_p()
    for changes in ([{}], [dict(touch_mode=1)] * 2):
        arr, keep = _fake_shards(lib, changes)
        assert L.ure_job_create(arr, len(changes), ctypes.byref(out)) != 0
        assert L.ure_last_error().decode().startswith('ure_job_create:')
        assert not out.value


# ---------------------------------------------------------------- exact OT (host function)
@pytest.mark.parametrize('k', [4, 5, 7])
def test_ot_assign_matches_reference_lp(lib, k):
    g = np.load(os.path.join(G, 'ot_toy.npz'))
    for which, r in (('round0', 0), ('last', -1)):
        M = g[f'k{k}_{which}_dist']                                   # [n, k] cost the reference passed to ot.emd
        label, plan, obj = lib.ot_assign(np.ascontiguousarray(M.T))
        assert np.array_equal(label, g[f'k{k}_round_labels'][r])
        assert abs(obj - g[f'k{k}_round_cost'][r]) < 1e-12
        assert (plan.sum(1) == k).all() and (plan.sum(0) == M.shape[0]).all()
    assert np.array_equal(plan, np.rint(g[f'k{k}_last_plan_nk']).astype(np.int32))


@pytest.mark.parametrize('n,k,seed', [(60, 3, 0), (64, 8, 1), (101, 4, 2), (7, 7, 3), (50, 1, 4), (333, 6, 5)])
def test_ot_assign_vs_highs_random(lib, n, k, seed):
    """Optimal objective equals an independent LP solver's; divisible and ragged n/k."""
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((n, 5)).astype(np.float32)
    C = X[rs.choice(n, k, replace=False)]
    dist = O.ot_cost(X, C)
    label, plan, obj = lib.ot_assign(dist)
    G_ = O.emd_exact(dist.T.astype(np.float64))
    assert abs(obj - float((G_ * dist.T).sum())) < 1e-9
    assert plan.min() >= 0 and (plan.sum(1) == k).all() and (plan.sum(0) == n).all()
    assert np.array_equal(plan, np.rint(G_ * n * k).astype(np.int32))           # the same vertex of the polytope
    # labels agree wherever a point's largest share is unique; an exact half/half split
    # (possible when k is even and k does not divide n) is decided by floating-point noise
    # in a float solver's plan and by np.argmax's first-maximum rule on the exact plan
    srt = np.sort(plan, axis=1)
    unique_max = srt[:, -1] > (srt[:, -2] if k > 1 else -1)
    assert np.array_equal(label[unique_max], np.argmax(G_, axis=1)[unique_max])
    assert np.array_equal(label, np.argmax(plan, axis=1))


def test_ot_assign_ties_and_zero_costs(lib):
    """Degenerate LP (all costs equal / exact zeros): still a feasible balanced plan."""
    for dist in (np.ones((4, 12), np.float32), np.zeros((3, 10), np.float32)):
        label, plan, obj = lib.ot_assign(dist)
        k, n = dist.shape
        assert (plan.sum(1) == k).all() and (plan.sum(0) == n).all()
        assert obj == float(dist[0, 0])


# ---------------------------------------------------------------- host logic
def test_read_rating_matches_oracle_partition():
    from ultrare_amd.read import readRating
    tr = O.load_csv(TRAIN)
    dels = np.random.RandomState(7).choice(N_USER, 12, replace=False).tolist()
    lists, idx = readRating(TRAIN, N_USER, 5, dels, [], 4, [])
    want_idx = O.uniform_groups(N_USER, 4)
    assert idx == want_idx
    for got, want in zip(lists, O.partition(*tr, want_idx, dels)):
        assert np.array_equal(got[0].astype(np.int32), want[0]) and np.array_equal(got[1].astype(np.int32), want[1])
        assert np.array_equal(got[2].astype(np.float32), want[2])
    # sort='a': shards reordered ascending by rating count (read.py:45-50)
    lists_a, idx_a = readRating(TRAIN, N_USER, 5, [], [], 4, [], 'a')
    counts = [a.shape[1] for a in lists_a]
    assert counts == sorted(counts) and idx_a == O.order_by_count(tr[0], want_idx)


def test_product_rng_stream_equals_reference_stream():
    from ultrare_amd import rng
    g = np.load(os.path.join(G, 'full_mf_toy.npz'))
    torch.manual_seed(42)
    U0, V0 = rng.mf_init(N_USER, N_ITEM, 16)
    assert np.array_equal(U0[:8].numpy(), g['U0_head']) and np.array_equal(V0[:8].numpy(), g['V0_head'])
    seeds = rng.epoch_seeds(3, False)
    perms = rng.epoch_perms(seeds, int(g['perm0_n']), threads=3)
    assert np.array_equal(perms[0][:16].numpy(), g['perm0_head'])
    # the threaded expansion is the same as the serial one, and the MF module draws the same as mf_init
    assert torch.equal(perms, rng.epoch_perms(seeds, int(g['perm0_n'])))
    from ultrare_amd.method.utils import MF
    torch.manual_seed(42)
    m = MF(N_USER, N_ITEM, 16)
    assert torch.equal(m.user_mat.weight.detach(), U0) and torch.equal(m.item_mat.weight.detach(), V0)


@pytest.mark.parametrize('n', [0, 1, 2, 17, 3000, 28360])
def test_host_randperm_equals_torch(n):
    """ure_host_randperm (threaded C++) == torch.randperm, seed for seed (read.py:133)."""
    from ultrare_amd import rng
    seeds = [0, 1, 42, 2 ** 31, 2 ** 40 + 12345, 2 ** 63 - 1, 6364136223846793005]
    got = rng.epoch_perms(seeds, n, threads=3)
    assert got.dtype == torch.int32 and got.shape == (len(seeds), n)
    for s, row in zip(seeds, got):
        assert torch.equal(row, rng.epoch_perm(s, n))


def test_epoch_seeds_batched_draw_equals_scalar_draws():
    """rng.epoch_seeds takes all of an epoch loop's int64 draws in one call; the reference draws them
    one by one (scratch.py:78-97 creates 3-4 loader iterators per epoch)."""
    from ultrare_amd import rng
    for with_total in (False, True):
        torch.manual_seed(123)
        got = rng.epoch_seeds(57, with_total)
        after = rng.draw_seed()
        torch.manual_seed(123)
        want = []
        for _ in range(57):
            rng.draw_seed()
            want.append(rng.draw_seed())
            rng.draw_seed()
            if with_total:
                rng.draw_seed()
        assert got == want and after == rng.draw_seed()


def test_shard_layout_invariants():
    """The slot array the kernels walk: every interaction appears once in its user's
    segment and once in its item's, segments are 8-aligned, padded slots never match."""
    from ultrare_amd.engine import ShardData
    tr = O.partition(*O.load_csv(TRAIN), [list(range(N_USER))])[0]
    sh = ShardData(*tr, N_USER, N_ITEM, device=torch.device('cpu'), keep_positions=True)
    sched = sh.sched.numpy()
    n = len(tr[0])
    assert sorted(sched[:, 0].tolist()) == list(range(N_USER + N_ITEM))
    assert (np.diff(sched[:, 3]) <= 0).all()                                  # heaviest first
    assert (sched[:, 1] % 8 == 0).all() and ((sched[:, 2] - sched[:, 1]) % 8 == 0).all()
    assert (sched[:, 2] - sched[:, 1] >= sched[:, 3]).all() and (sched[1:, 1] == sched[:-1, 2]).all()
    assert sh.n_active == (sched[:, 3] > 0).sum() and sched[-1, 2] == sh.n_slots
    oid, r = sh.ent_oid.numpy(), sh.ent_r.numpy()
    up, ip = sh.u_pos, sh.i_pos
    src = sh.ent_src.numpy()
    assert np.array_equal(src[up], np.arange(n)) and np.array_equal(src[ip], np.arange(n)) and (src < 0).sum() == sh.n_slots - 2 * n
    assert len(set(up.tolist()) | set(ip.tolist())) == 2 * n                   # all slots distinct
    assert np.array_equal(oid[up], tr[1]) and np.array_equal(oid[ip], tr[0])
    assert np.array_equal(r[up], tr[2]) and np.array_equal(r[ip], tr[2])
    beg = {int(row): (int(b), int(e)) for row, b, e, _ in sched}
    for j in (0, 1, n // 2, n - 1):
        b, e = beg[int(tr[0][j])]
        assert b <= up[j] < e
        b, e = beg[N_USER + int(tr[1][j])]
        assert b <= ip[j] < e
    assert (sh.ent_tag.numpy() == -1).all()                                    # 0xFFFF everywhere before training
    with pytest.raises(ValueError):
        ShardData(tr[0], tr[1] + N_ITEM, tr[2], N_USER, N_ITEM, device=torch.device('cpu'))


def test_native_ingest_matches_numpy(tmp_path):
    """ure_host_read_csv / ure_host_partition / ure_host_build_layout against numpy."""
    from ultrare_amd import _native as nv
    u, i, r = nv.read_csv(TRAIN, threads=3)
    ou, oi, orr = O.load_csv(TRAIN)
    assert np.array_equal(u, ou) and np.array_equal(i, oi) and np.array_equal(r, orr)
    odd = tmp_path / 'odd.csv'                                    # exponents, blanks, extra column, CRLF, no final newline
    odd.write_text('1,2,3.5\r\n\n3,4,1e-1,999\n 5,6,4\n7,8,0.30000000000000004')
    u2, i2, r2 = nv.read_csv(str(odd))
    assert u2.tolist() == [1, 3, 5, 7] and i2.tolist() == [2, 4, 6, 8] and r2.tolist() == [3.5, 0.1, 4.0, 0.30000000000000004]
    bad = tmp_path / 'bad.csv'
    bad.write_text('1,2\n')
    with pytest.raises(nv.NativeError):
        nv.read_csv(str(bad))
    # partition: same shards as the oracle's np.isin partition, deleted users dropped
    import ctypes
    idx = O.uniform_groups(N_USER, 4)
    dels = [3, 77, 500]
    shard_of = np.full(N_USER, -1, dtype=np.int32)
    for s_, g_ in enumerate(idx):
        shard_of[np.asarray(g_)] = s_
    shard_of[dels] = -1
    counts = np.zeros(4, dtype=np.int64)
    L = nv.lib()
    nv.check(L.ure_host_partition(u.ctypes.data, i.ctypes.data, r.ctypes.data, len(u), shard_of.ctypes.data, N_USER, 4, 5.0,
                                  counts.ctypes.data, None, None, None, None), 'count')
    ouid, oiid, orat = (np.empty(counts.sum(), np.int32), np.empty(counts.sum(), np.int32), np.empty(counts.sum(), np.float32))
    nv.check(L.ure_host_partition(u.ctypes.data, i.ctypes.data, r.ctypes.data, len(u), shard_of.ctypes.data, N_USER, 4, 5.0,
                                  counts.ctypes.data, ouid.ctypes.data, oiid.ctypes.data, orat.ctypes.data, None), 'partition')
    want = O.partition(ou, oi, orr, idx, dels)
    o = 0
    for s_ in range(4):
        c = int(counts[s_])
        assert c == len(want[s_][0])
        assert np.array_equal(ouid[o:o + c], want[s_][0]) and np.array_equal(oiid[o:o + c], want[s_][1])
        assert np.array_equal(orat[o:o + c], want[s_][2])
        o += c
    # layout: identical to a stable-argsort construction
    tr = want[0]
    lay = nv.build_layout(tr[0], tr[1], tr[2], N_USER, N_ITEM, want_pos=True)
    nnz = np.concatenate([np.bincount(tr[0], minlength=N_USER), np.bincount(tr[1], minlength=N_ITEM)])
    order = np.argsort(-nnz, kind='stable')
    assert np.array_equal(lay['sched'][:, 0], order) and np.array_equal(lay['sched'][:, 3], nnz[order])
    for keys, pos, base in ((tr[0], lay['u_pos'], 0), (tr[1], lay['i_pos'], N_USER)):
        beg = np.empty(N_USER + N_ITEM, dtype=np.int64)
        beg[lay['sched'][:, 0]] = lay['sched'][:, 1]
        srt = np.argsort(keys, kind='stable')
        first = np.searchsorted(keys[srt], keys[srt], side='left')
        want_pos = np.empty(len(keys), dtype=np.int64)
        want_pos[srt] = beg[base + keys[srt]] + (np.arange(len(keys)) - first)
        assert np.array_equal(pos, want_pos)
    with pytest.raises(nv.NativeError):
        nv.build_layout(tr[0], tr[1] + N_ITEM, tr[2], N_USER, N_ITEM)


@pytest.mark.parametrize('d', [4, 16, 32, 64, 256])
def test_work_units_cover_every_row_once(d):
    """ure_host_build_units: the units of a row tile its segment exactly, stay inside one workgroup,
    name their leader and count; heavy rows (more pieces than lane groups) get longer pieces."""
    from ultrare_amd import _native as nv
    rs = np.random.RandomState(d)
    n_rows = 700
    nnz = np.sort(np.concatenate([[5000, 2049, 2048, 300], rs.randint(1, 90, n_rows - 30), np.zeros(26, dtype=np.int64)]))[::-1]
    pad = (nnz + 7) // 8 * 8
    beg = np.concatenate([[0], np.cumsum(pad)[:-1]])
    sched = np.stack([rs.permutation(n_rows), beg, beg + pad, nnz], axis=1).astype(np.int32)
    n_active = int((nnz > 0).sum())
    units = nv.build_units(sched, n_active, d)
    lanes = d // 4 if d <= 32 else d // 8
    cap, upb = 8 * lanes, 256 // lanes
    assert len(units) % upb == 0
    real = units[units[:, 0] >= 0]
    assert sorted(set(real[:, 0].tolist())) == sorted(sched[:n_active, 0].tolist())
    by_row = {int(r): (int(b), int(e)) for r, b, e, _ in sched[:n_active]}
    local = np.arange(len(units)) % upb
    block = np.arange(len(units)) // upb
    leader, count, multi = units[:, 3] & 0xFFFF, (units[:, 3] >> 16) & 0x3FFF, (units[:, 3] >> 30) & 1
    for r, (b, e) in by_row.items():
        idx = np.nonzero(units[:, 0] == r)[0]
        assert (np.diff(idx) == 1).all() and len(set(block[idx])) == 1          # consecutive, one workgroup
        assert (count[idx] == len(idx)).all() and (leader[idx] == local[idx[0]]).all()
        assert units[idx[0], 1] == b and units[idx[-1], 2] == e and (units[idx[1:], 1] == units[idx[:-1], 2]).all()
        lens = units[idx, 2] - units[idx, 1]
        assert (lens % 8 == 0).all() and (lens > 0).all()
        assert (lens <= cap).all() or len(idx) <= upb                            # longer pieces only for heavy rows
        if e - b <= cap * upb:
            assert (lens <= cap).all()
    empty = units[:, 0] < 0
    assert (count[empty] == 1).all() and (leader[empty] == local[empty]).all() and (units[empty, 1] == units[empty, 2]).all()
    for blk in range(len(units) // upb):
        m = block == blk
        assert multi[m].min() == multi[m].max() == int((count[m] > 1).any())
    assert nv.build_units(sched, 0, d).shape == (0, 4)


def test_kmeans_assign_host_vs_numpy():
    """ure_host_kmeans_assign (utils.py:377-396): argmin / balanced greedy fill and the float32 pairwise
    inertia against the oracle's numpy statement, incl. exact ties and a NaN row."""
    import ctypes
    from ultrare_amd import _native as nv
    rs = np.random.RandomState(3)
    for n, k in ((37, 3), (500, 7), (1508, 5)):
        dist = rs.rand(n, k).astype(np.float32)
        dist[::11] = np.round(dist[::11], 1)                    # exact ties
        for balanced in (False, True):
            want = O.kmeans_assign(dist, balanced)
            got = np.empty(n, dtype=np.int32)
            inertia = ctypes.c_double()
            nv.check(nv.lib().ure_host_kmeans_assign(dist.ctypes.data, n, k, int(np.ceil(n / k)) if balanced else 0,
                                                     got.ctypes.data, ctypes.byref(inertia)), 'assign')
            assert np.array_equal(got, want)
            assert inertia.value == float(np.sum(dist[np.arange(n), want]))
            if balanced:
                assert np.bincount(got, minlength=k).max() <= int(np.ceil(n / k))
    dist = np.array([[1, np.nan, 0], [2, 1, 3]], dtype=np.float32)
    got = np.empty(2, dtype=np.int32)
    nv.check(nv.lib().ure_host_kmeans_assign(dist.ctypes.data, 2, 3, 0, got.ctypes.data, None), 'assign')
    assert got.tolist() == dist.argmin(axis=1).tolist()
    assert nv.lib().ure_host_kmeans_assign(dist.ctypes.data, 2, 3, -0 + 0, None, None) != 0


def test_shard_placement_is_lpt():
    from ultrare_amd.method.sisa import assign_shards
    assert assign_shards([5, 9, 3, 7], 1) == [0, 0, 0, 0]
    own = assign_shards([5, 9, 3, 7], 2)
    load = [sum(s for s, o in zip([5, 9, 3, 7], own) if o == r) for r in range(2)]
    assert sorted(load) == [12, 12]
    assert sorted(assign_shards([4] * 8, 8)) == list(range(8))


def test_torch_port_matches_reference():
    """bench.py's cpu_baseline port reproduces the reference's numbers (golden E=3)."""
    from oracle import torch_port
    g = np.load(os.path.join(G, 'full_mf_toy.npz'))
    train = O.partition(*O.load_csv(TRAIN), [list(range(N_USER))])[0]
    torch.manual_seed(42)
    # the reference interleaves one extra draw per epoch (test loader seed): emulate by running epoch by epoch
    model, seen, spent, losses = torch_port.train_shard(train, N_USER, N_ITEM, 16, 3000, 1)
    np.testing.assert_allclose(losses, g['E1_train_loss'], rtol=1e-6)
    assert np.abs(model.user_mat.weight.detach().numpy() - g['E1_U']).max() < 1e-5
    assert seen == len(train[0]) and spent > 0


def test_synthetic_dataset_shape():
    from ultrare_amd import synth
    d = synth.make_dataset(300, 200, 9000, 1000, seed=3)
    u, i, r = d['train']
    assert len(u) == 9000 and len(d['test'][0]) == 1000
    allu = np.concatenate([u, d['test'][0]])
    alli = np.concatenate([i, d['test'][1]])
    assert len(np.unique(allu * 200 + alli)) == 10000                          # no duplicate (user, item)
    assert (np.diff(u) >= 0).all() and set(np.unique(r)) <= {1., 2., 3., 4., 5.}
    assert np.bincount(allu, minlength=300).min() >= 20
    so, groups = synth.uniform_shards(300, 4)
    assert groups == O.uniform_groups(300, 4)
    assert sum(len(p[0]) for p in synth.split_shards(d['train'], so, 4)) == 9000


# ---------------------------------------------------------------- N > 1 host protocol over gloo
_WORKER = r'''
import os, sys, time, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from ultrare_amd.method.sisa import assign_shards, prepare_owned, exchange_tables, exchange_plan
from ultrare_amd.read import RatingData, loadData
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
n_user, n_item, k, E, sizes = eval(sys.argv[3])
dist.init_process_group('gloo')
def barrier():          # (dist.barrier() asks the HIP runtime for an accelerator, which opens the GPU on a GPU host: these ranks are CPU only)
    dist.all_reduce(torch.zeros(1))
rs = np.random.RandomState(0)
loaders = [loadData(RatingData(np.vstack([rs.randint(0, n_user, n), rs.randint(0, n_item, n), rs.rand(n)])), 16, 1) for n in sizes]
ids = list(range(len(sizes)))
owner = assign_shards(sizes, world)
prepare_owned(ids[:2], [rank, rank], rank, loaders[:2], 64, 64, 4, 1, on_device=False)      # (library, thread pools: loaded before the clock starts)
torch.manual_seed(42)
barrier()
from ultrare_amd import rng
rng.STATS.update(normals=0, skipped_draws=0)
t0 = time.thread_time()            # (CPU time of this thread: eight ranks and their transport threads share this host's cores)
prep = prepare_owned(ids, owner, rank, loaders, n_user, n_item, k, E, on_device=False)
draw_s = time.thread_time() - t0
stats = dict(rng.STATS)
after = torch.empty((), dtype=torch.int64).random_().item()          # stream position after the call
models = {i: (prep[i][1][0].clone() + 0, prep[i][1][1].clone() + 0) for i in prep}
edges = np.linspace(0, n_user, len(sizes) + 1).astype(int)
rows = {i: torch.as_tensor(rs.permutation(np.arange(edges[i], edges[i + 1]))) for i in ids}     # ragged groups, any order
got = exchange_tables(models, ids, owner, rank, rows, n_item, k, torch.device('cpu'), dist)
full = exchange_tables(models, ids, owner, rank, rows, n_item, k, torch.device('cpu'), dist, full_u=n_user)
all_s = 0.0
if len(ids) > 4:        # the same phase with every shard owned by this rank, under the same load (the other ranks do the same now)
    state = torch.get_rng_state()
    torch.manual_seed(42)
    barrier()
    t0 = time.thread_time()
    prepare_owned(ids, [rank] * len(ids), rank, loaders, n_user, n_item, k, E, on_device=False)
    all_s = time.thread_time() - t0
    torch.set_rng_state(state)
np.savez(sys.argv[2] + f'/rank{rank}.npz', owner=owner, after=after, draw_s=draw_s, all_s=all_s, mine=sorted(prep), normals=stats['normals'], skipped=stats['skipped_draws'],
         usum=[float(got[i][0].double().sum()) for i in ids], vsum=[float(got[i][1].double().sum()) for i in ids],
         fsum=[float(full[i][0].double().sum()) for i in ids],
         **({f'R{i}': rows[i].numpy() for i in ids} if len(ids) <= 4 else {}),
         **({f'U{i}': got[i][0].numpy() for i in ids} if len(ids) <= 4 else {}), **({f'V{i}': got[i][1].numpy() for i in ids} if len(ids) <= 4 else {}),
         **({f'F{i}': full[i][0].numpy() for i in ids} if len(ids) <= 4 else {}),
         **({f'perm{i}': prep[i][2].numpy() for i in prep} if len(ids) <= 4 else {}))
dist.destroy_process_group()
'''


def _run_ranks(tmp_path, world, port, shape):
    script = tmp_path / 'worker.py'
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), OMP_NUM_THREADS='1')
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(tmp_path), repr(shape)], env=dict(env, RANK=str(r)))
             for r in range(world)]
    for p in procs:
        assert p.wait(timeout=400) == 0
    return [np.load(tmp_path / f'rank{r}.npz') for r in range(world)]


def test_two_rank_protocol_over_gloo(tmp_path):
    """world_size 2 on CPU: every rank walks the whole RNG stream, draws for its own shards only, and after the one
    all-gather holds every shard's OWN user rows and item table (sisa.py:52-58 reads nothing else) -- or, with full_u, every
    shard's whole user table (the reference's per-epoch logs, scratch.py:83-86) -- identical to what a single process draws
    sequentially."""
    sizes = [50, 80, 30]
    r0, r1 = _run_ranks(tmp_path, 2, 29631, (20, 10, 4, 2, sizes))
    from ultrare_amd import rng
    torch.manual_seed(42)
    want = {}
    for i, n in enumerate(sizes):
        U0, V0 = rng.mf_init(20, 10, 4)
        want[i] = (U0.numpy(), V0.numpy(), rng.epoch_perms(rng.epoch_seeds(2, True), n).numpy())
    after = torch.empty((), dtype=torch.int64).random_().item()
    assert sorted(set(r0['owner'].tolist())) == [0, 1]
    for r in (r0, r1):
        assert int(r['after']) == after
        for i in range(3):
            assert np.array_equal(r[f'U{i}'], want[i][0][r[f'R{i}']]) and np.array_equal(r[f'V{i}'], want[i][1])
            assert np.array_equal(r[f'F{i}'], want[i][0])                       # full_u: the owner's whole table
        assert r['mine'].tolist() == [i for i in range(3) if int(r['owner'][i]) == (0 if r is r0 else 1)]
    for i in range(3):
        src = r0 if int(r0['owner'][i]) == 0 else r1
        assert np.array_equal(src[f'perm{i}'], want[i][2])


def test_eight_rank_protocol_32_shards_over_gloo(tmp_path):
    """BASELINE.json configs[3]'s placement (32 shards over 8 ranks) rehearsed on CPU: longest-processing-time placement is
    balanced, exchange_plan tiles every rank's segment, every rank ends at the same stream position with the same tables, and
    -- VERDICT r3 item 5 -- no rank spends its draw phase on shards it does not own: the slowest rank stays far below
    what ONE process needs to draw all 32 (round 3 drew the full U0 of the 28 foreign shards on every rank)."""
    from ultrare_amd import rng
    from ultrare_amd.method.sisa import assign_shards, exchange_plan
    n_user, n_item, k, E = 24000, 9000, 32, 2
    rs = np.random.RandomState(7)
    sizes = [int(x) for x in rs.randint(300, 900, 32)]
    world = 8
    owner = assign_shards(sizes, world)
    load = np.bincount(owner, weights=sizes, minlength=world)
    assert np.bincount(owner, minlength=world).min() >= 2 and load.max() - load.min() <= max(sizes)        # LPT: within one shard of even
    where, seg = exchange_plan(list(range(32)), owner, [n_user] * 32, n_item, k, world)
    for r in range(world):
        off = 0
        for i in range(32):
            if owner[i] == r:
                assert where[i] == (r, off)
                off += (n_user + n_item) * k
        assert off <= seg
    ranks = _run_ranks(tmp_path, world, 29637, (n_user, n_item, k, E, sizes))
    torch.manual_seed(42)
    want = [rng.mf_init(n_user, n_item, k) + (rng.epoch_seeds(E, True),) for _ in sizes]
    after = torch.empty((), dtype=torch.int64).random_().item()
    edges = np.linspace(0, n_user, 33).astype(int)
    for r, res in enumerate(ranks):
        assert int(res['after']) == after and res['owner'].tolist() == owner
        assert res['mine'].tolist() == [i for i in range(32) if owner[i] == r]
        np.testing.assert_allclose(res['vsum'], [float(w[1].double().sum()) for w in want], rtol=1e-12)
        np.testing.assert_allclose(res['fsum'], [float(w[0].double().sum()) for w in want], rtol=1e-12)
        np.testing.assert_allclose(res['usum'], [float(w[0][edges[i]:edges[i + 1]].double().sum()) for i, w in enumerate(want)], rtol=1e-9)
    # the host work of the draw phase, counted (its CPU time on a shared host varies by 5x between runs: `draw_s` / `all_s` are
    # recorded, not asserted): a rank computes the two kept N(0, 1) fills of the shards it owns and not one normal more; everything
    # else of the stream -- the discarded fills of its own shards, all four fills and the seeds of the 28 foreign ones -- is skipped
    per_model = (n_user + n_item) * k
    fill = rng.fill_draws(n_user * k) + rng.fill_draws(n_item * k)
    for r, res in enumerate(ranks):
        own = sum(1 for i in range(32) if owner[i] == r)
        assert int(res['normals']) == own * per_model, (r, int(res['normals']), own * per_model)
        assert int(res['skipped']) == own * fill + (32 - own) * (2 * fill + 2 * E * 4), (r, int(res['skipped']))


def test_preprocess_properties_on_unsorted_input(tmp_path):
    """ultrare_amd/preprocess.py on a file whose users are NOT grouped: 5-core property, squeezed ids,
    int(0.9 n) rows per user in train, file order kept in both splits.  (The pin against the
    notebook's own cells is tests/test_parity_pins.py::test_preprocess_matches_the_notebook_run.)"""
    from ultrare_amd.preprocess import preprocess
    rs = np.random.RandomState(0)
    n = 6000
    u = rs.zipf(1.3, n) % 300 + 1
    i = rs.zipf(1.2, n) % 400 + 1
    pairs = np.unique(np.stack([u, i], 1), axis=0)
    pairs = pairs[rs.permutation(len(pairs))]
    dat = tmp_path / 'ratings.dat'
    dat.write_text(''.join(f'{a}::{b}::{rs.randint(1, 6)}::0\n' for a, b in pairs.tolist()))
    info = preprocess(str(dat), str(tmp_path / 'out'), seed=5)
    tr = np.loadtxt(tmp_path / 'out' / 'squ0_train.csv', delimiter=',')
    te = np.loadtxt(tmp_path / 'out' / 'squ0_test.csv', delimiter=',')
    assert info['n_train'] == len(tr) and info['n_test'] == len(te)
    allr = np.vstack([tr, te])
    cu, ci = np.bincount(allr[:, 0].astype(int)), np.bincount(allr[:, 1].astype(int))
    assert cu.min() >= 5 and ci.min() >= 5 and len(cu) == info['n_user'] and len(ci) == info['n_item']
    assert np.array_equal(np.bincount(tr[:, 0].astype(int), minlength=len(cu)), (cu * 0.9).astype(int))
    assert len(np.unique(allr[:, :2], axis=0)) == len(allr)
    # first-appearance squeeze: user ids appear in increasing order of first occurrence over train + test merged in file order
    ud = np.load(tmp_path / 'out' / 'user_dict.npy', allow_pickle=True).item()
    assert sorted(ud.values()) == list(range(info['n_user']))


# ---------------------------------------------------------------- bench.py host logic (no GPU here)
def test_bench_spawn_propagates_rank_failure_without_hanging():
    """`python bench.py --gpus 2` with no launcher starts two rank processes itself.  In this container
    there is no GPU, so every rank stops with the 'needs an MI355X' message: the parent must come back
    promptly with a non-zero code (and must not have touched the GPU itself)."""
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible: covered by tests/test_gpu_multirank.py')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode != 0 and time.time() - t0 < 120
    # the first failing rank decides the code; its peers get a grace period to report by themselves before they are
    # terminated, so at least one message (normally both) arrives
    assert 1 <= p.stderr.count(b'needs an MI355X') <= 2


def test_exchange_plan_is_a_padded_all_gather_v():
    from ultrare_amd.method.sisa import exchange_plan
    ids, owner, sizes = [0, 1, 2, 3, 4], [0, 1, 0, 2, 1], [7, 8, 5, 3, 9]
    where, seg = exchange_plan(ids, owner, sizes, n_item=10, k=4, world=4)
    fill = {r: sum((sizes[p] + 10) * 4 for p in range(5) if owner[p] == r) for r in range(4)}
    assert seg == max(fill.values()) and fill[3] == 0
    for r in range(4):                                   # a rank's shards tile its segment back to back, in ids order
        off = 0
        for p, i in enumerate(ids):
            if owner[p] == r:
                assert where[i] == (r, off)
                off += (sizes[p] + 10) * 4


def test_bench_counts_interactions_exactly():
    import importlib.util
    sp = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    b = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(b)
    sizes, B, E = [70, 25, 100], 30, 3
    tot, per_tick, dense = b.interactions_in_ticks(sizes, B, 0, 12, E, dense_bytes=[1, 10, 100])
    # shard 0: 3 steps/epoch (30, 30, 10); shard 1: 1 step (25), done after tick 3; shard 2: 4 steps (30, 30, 30, 10)
    assert tot == 3 * 70 + 3 * 25 + 3 * 100
    assert per_tick[:4].tolist() == [30 + 25 + 30, 30 + 25 + 30, 10 + 25 + 30, 30 + 0 + 10]
    assert dense[:4].tolist() == [111, 111, 111, 101] and dense[9:].tolist() == [100, 100, 100]


def test_bench_dump_outputs_stays_within_its_budget(tmp_path):
    """--dump-outputs: every shard's (U, V) as float32 .npy files; tables beyond 64 MB in all are cut to one seeded row sample,
    the same from run to run."""
    import importlib.util
    sp = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    b = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(b)

    class Job:
        k, device = 4, torch.device('cpu')

        def __init__(self, tables):
            self.t = tables

        def tables(self, s):
            return self.t[s]
    g = torch.Generator().manual_seed(1)
    small = Job([(torch.randn(60, 4, generator=g), torch.randn(34, 4, generator=g)) for _ in range(2)])
    b.dump_outputs(str(tmp_path / 'small'), {'job': small, 'spec': {'n_user': 60, 'n_item': 34}, 'mine': [3, 4]}, 0, 1)
    assert sorted(os.listdir(tmp_path / 'small')) == ['U3.npy', 'U4.npy', 'V3.npy', 'V4.npy']
    got = np.load(tmp_path / 'small' / 'V4.npy')
    assert got.dtype == np.float32 and np.array_equal(got, small.t[1][1].numpy())
    n_user, n_item = 3_000_000, 1_500_000                    # 2 x 72 MB of tables; row i holds i
    big = Job([tuple(torch.arange(n, dtype=torch.float32)[:, None].expand(n, 4) for n in (n_user, n_item))])
    for d in ('a', 'b'):
        b.dump_outputs(str(tmp_path / d), {'job': big, 'spec': {'n_user': n_user, 'n_item': n_item}, 'mine': [0]}, 1, 2)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['rank1_U0.npy', 'rank1_V0.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= b.DUMP_MAX_BYTES // 2
    for f, n in zip(files, (n_user, n_item)):
        got = np.load(tmp_path / 'a' / f)
        assert got.dtype == np.float32 and np.array_equal(got, np.load(tmp_path / 'b' / f))
        rows = got[:, 0]
        assert 0 < len(rows) < n and (np.diff(rows) > 0).all() and rows[-1] < n and (got == rows[:, None]).all()


# ---------------------------------------------------------------- generator skip-ahead (ure_host_mt_advance)
def test_mt_advance_matches_torch_generator_state():
    """Moving torch's CPU generator past the draws of a call without making them: normal_ of n >= 16 float32
    elements consumes n (+16 when 16 does not divide n) 32-bit outputs, an int64 random_ two each -- the
    resulting state must be torch's own, byte for byte (ATen CPUGeneratorImpl, legacy state layout)."""
    from ultrare_amd import rng
    torch.manual_seed(42)
    s0 = torch.get_rng_state()
    body = 24 + 624 * 8
    for n in (16, 17, 100, 623, 624, 625, 6040 * 32, 3416 * 32, 1508 * 16 + 3):
        torch.set_rng_state(s0)
        torch.empty(n).normal_()
        assert torch.equal(torch.get_rng_state()[:body], rng.advance_state(s0, rng.fill_draws(n))[:body]), n
    torch.set_rng_state(s0)
    torch.empty(200, dtype=torch.int64).random_()
    assert torch.equal(torch.get_rng_state(), rng.advance_state(s0, 400))
    # a chain of calls from a state in the middle of a block
    torch.set_rng_state(s0)
    torch.empty(1000).normal_()
    mid = torch.get_rng_state()
    torch.empty(3, 70).normal_()
    torch.empty(9, dtype=torch.int64).random_()
    assert torch.equal(torch.get_rng_state()[:body], rng.advance_state(mid, rng.fill_draws(210) + 18)[:body])
    assert torch.equal(rng.advance_state(mid, 0), mid)
    with pytest.raises(Exception):
        rng.advance_state(torch.zeros(16, dtype=torch.uint8), 5)


def test_mt_charpoly_table_is_the_generators_own():
    """csrc/mt_jump.cpp's table of MT19937's characteristic polynomial, recomputed here from the generator's output: Berlekamp-Massey on
    one bit of 2 x 19,937 + 200 consecutive outputs (Python's `random` is MT19937; the polynomial is irreducible, so every output bit has
    it as its minimal polynomial)."""
    import random
    from ultrare_amd import _native as nv
    rnd = random.Random(12345)
    n_bits = 2 * 19937 + 200
    C, B, L, m, W = 1, 1, 0, 1, 0
    for n in range(n_bits):
        W = (W << 1) | (rnd.getrandbits(32) & 1)
        if bin(C & W).count('1') & 1:
            T = C
            C ^= B << m
            if 2 * L <= n:
                L, B, m = n + 1 - L, T, 1
            else:
                m += 1
        else:
            m += 1
    assert L == 19937
    want = sorted(L - i for i in range(L + 1) if (C >> i) & 1)            # s_n = sum c_i s_(n-i)  ->  phi(x) = sum c_i x^(L-i)
    got = np.zeros(135, dtype=np.uint16)
    assert nv.lib().ure_host_mt_charpoly(got.ctypes.data, 135) == 135
    assert got.tolist() == want and len(want) == 135 and want[-2] == 19314


def test_mt_jump_equals_the_walk_byte_for_byte():
    """ure_host_mt_advance beyond 4,096 blocks jumps (x^J modulo the characteristic polynomial on the raw word sequence); in pieces below
    that threshold it walks.  Same generator state either way, from the start and the middle of a block, at distances on and off block
    boundaries, up to BASELINE.json configs[3]'s per-shard distance and beyond -- and torch's own state after really making the draws."""
    import ctypes
    from ultrare_amd import _native as nv, rng
    L = nv.lib()

    def walk(s, n, step=2_000_000):
        s = s.clone()
        while n > 0:
            c = min(n, step)
            nv.check(L.ure_host_mt_advance(s.data_ptr(), s.numel(), c), 'ure_host_mt_advance')
            n -= c
        return s
    torch.manual_seed(42)
    fresh = torch.get_rng_state()                        # left = 1: the first draw regenerates
    torch.empty(1000).normal_()
    mid = torch.get_rng_state()
    blk = 624
    for s0 in (fresh, mid):
        for n in (4096 * blk - 1, 4096 * blk, 4096 * blk + 1, 4160 * blk + 377, 5_000_000, 2 * (rng.fill_draws(162000 * 128) + rng.fill_draws(60000 * 128)) + 40,
                  123_456_789):
            assert torch.equal(walk(s0, n), rng.advance_state(s0, n, count=False)), n
    # a chain of jumps = one long walk (the shards of a request)
    a = b = mid
    for _ in range(5):
        a, b = walk(a, 7_000_003), rng.advance_state(b, 7_000_003, count=False)
    assert torch.equal(a, b)
    # torch itself
    g = torch.Generator()
    g.manual_seed(7)
    st = g.get_state().clone()
    torch.empty(6_000_000).normal_(generator=g)
    assert torch.equal(rng.advance_state(st, 6_000_000, count=False), g.get_state())
    # the block form and the support list
    words = np.random.RandomState(3).randint(0, 2 ** 32, 624, dtype=np.uint64).astype(np.uint32)
    ref = words.copy()
    N, M = 624, 397
    for _ in range(70):                                  # 70 plain regenerations in numpy
        x = np.concatenate([ref, np.zeros(N, dtype=np.uint32)])
        for k in range(N):
            y = (x[k] & np.uint32(0x80000000)) | (x[k + 1] & np.uint32(0x7fffffff))
            x[k + N] = x[k + M] ^ (y >> np.uint32(1)) ^ (np.uint32(0x9908b0df) if (y & np.uint32(1)) else np.uint32(0))
        ref = x[N:].copy()
    got = words.copy()
    nv.check(L.ure_host_mt_jump_blocks(got.ctypes.data, 70), 'ure_host_mt_jump_blocks')
    assert np.array_equal(got[1:], ref[1:]) and got[0] == ref[0]
    n_sup = ctypes.c_int32()
    sup = np.zeros(19937, dtype=np.uint16)
    nv.check(L.ure_host_mt_jump_support(70, sup.ctypes.data, len(sup), ctypes.byref(n_sup)), 'ure_host_mt_jump_support')
    assert 0 < n_sup.value < 19937 and np.all(np.diff(sup[:n_sup.value].astype(np.int64)) > 0)
    assert L.ure_host_mt_jump_blocks(None, 5) != 0 and L.ure_host_mt_jump_support(0, sup.ctypes.data, len(sup), ctypes.byref(n_sup)) != 0


def test_shard_streams_at_the_25m_shape_are_cheap_and_exact():
    """the start states of configs[3]'s 32 shards (56.8 M outputs apart) in a cold process -- no memo -- within 20 ms
    (round 4's walk: 0.2-0.6 s), and equal to states reached by walking."""
    import time
    from ultrare_amd import _native as nv, rng
    L = nv.lib()
    os.environ['URE_STREAM_MEMO'] = '0'
    try:
        torch.manual_seed(42)
        s0 = torch.get_rng_state()
        rng.shard_streams(2, 162000, 60000, 128, 5, True)            # (the polynomial of this distance is computed once per process)
        torch.manual_seed(42)
        t0 = time.perf_counter()
        starts, end, seeds = rng.shard_streams(32, 162000, 60000, 128, 5, True, want_seeds=True)
        took = time.perf_counter() - t0
    finally:
        os.environ.pop('URE_STREAM_MEMO', None)
    assert took < 0.06, took                                          # (20 ms asked; CI hosts are noisy: 7-9 ms measured)
    per = sum(rng.model_draws(162000, 60000, 128, 5, True))
    s = s0.clone()
    for i in (0, 1, 2):
        assert torch.equal(starts[i], s)
        n = per
        while n > 0:                                                  # walked: pieces below the jump threshold
            c = min(n, 2_000_000)
            nv.check(L.ure_host_mt_advance(s.data_ptr(), s.numel(), c), 'ure_host_mt_advance')
            n -= c
    g = torch.Generator()
    g.set_state(rng.advance_state(starts[1], sum(rng.model_draws(162000, 60000, 128, 5, True)[:2]), count=False))
    assert rng.epoch_seeds(5, True, generator=g) == seeds[1]


def test_native_model_init_is_torchs_own_fill_bit_for_bit():
    """ure_host_mf_init (utils.py:31-40's kept fills: uniforms off the generator in bulk, the 16-blocks through the installed
    PyTorch's own AVX2 kernels) against `tensor.normal_()`: tables AND generator state, for lengths with and without the redrawn
    tail, from states at the start and in the middle of a generator block, on 1 and 3 threads; the Box-Muller half alone; and the
    refusals.  Where this build cannot reproduce torch (no AVX2, another PyTorch) rng.native_fill_ok() is False and rng.mf_init keeps
    torch's fill -- checked too."""
    from ultrare_amd import _native as nv, rng
    L = nv.lib()
    rng._NATIVE_FILL[0] = None
    ok = rng.native_fill_ok()
    g, h = torch.Generator(), torch.Generator()
    for seed, pre in ((1, 0), (7, 333), (42, 624 * 3 + 1)):
        g.manual_seed(seed)
        if pre:
            torch.empty(pre, dtype=torch.int32).random_(generator=g)
        for (n_user, n_item, k) in ((6040, 3416, 32), (1508, 2071, 16), (37, 5, 5), (1, 16, 1), (313, 17, 3)):
            if min(n_user, n_item) * k < 16:
                continue
            h.set_state(g.get_state())
            for threads in (1, 3):
                g.set_state(h.get_state())
                U0, V0 = rng.mf_init(n_user, n_item, k, generator=g, threads=threads)
                rng._NATIVE_FILL[0] = False                      # torch's own four fills
                try:
                    gt = torch.Generator()
                    gt.set_state(h.get_state())
                    for rows in (n_user, n_item):
                        torch.empty(rows, k).normal_(0, 1, generator=gt)
                    Ut, Vt = torch.empty(n_user, k).normal_(0, 1, generator=gt), torch.empty(n_item, k).normal_(0, 1, generator=gt)
                finally:
                    rng._NATIVE_FILL[0] = ok
                assert torch.equal(U0.view(torch.int32), Ut.view(torch.int32)) and torch.equal(V0.view(torch.int32), Vt.view(torch.int32)), (seed, n_user, k, threads)
                assert torch.equal(g.get_state(), gt.get_state())
    if not ok:
        pytest.skip('this build does not reproduce torch\'s AVX2 fill: rng.mf_init keeps torch\'s own (checked above)')
    # the Box-Muller half alone, in place, equals normal_ on the same uniforms
    g.manual_seed(5)
    st = g.get_state()
    want = torch.empty(16 * 200).normal_(0, 1, generator=g)
    g.set_state(st)
    u = torch.empty(16 * 200).uniform_(0, 1, generator=g)
    assert L.ure_host_normal_blocks(u.data_ptr(), 200, 0.0, 1.0) == 0 and torch.equal(u.view(torch.int32), want.view(torch.int32))
    # refusals: fewer than 16 elements (ATen's scalar path is not restated), not a generator state
    st = g.get_state().clone()
    buf = torch.empty(64)
    assert L.ure_host_mf_init(st.data_ptr(), st.numel(), 0, buf.data_ptr(), 15, buf.data_ptr(), 16, 1) != 0
    assert L.ure_host_mf_init(torch.zeros(5056, dtype=torch.uint8).data_ptr(), 5056, 0, buf.data_ptr(), 16, buf.data_ptr(), 16, 1) != 0
    assert torch.equal(st, g.get_state())


def test_scalar_normal_math_is_torchs_and_the_other_readings_are_not():
    """csrc/normal_math.h -- the per-lane restatement of ATen's normal_fill_16_AVX2 that the DEVICE kernels run (csrc/mf_init.hip) -- on the
    host against `tensor.normal_()` over 2^22 uniforms: variant 0 (the first product of an ambiguous mul + add pair is the fused one) is
    torch's on every value; the three other readings of the two ambiguous pairs are not."""
    from ultrare_amd import _native as nv
    L = nv.lib()
    g = torch.Generator()
    g.manual_seed(5)
    n = 1 << 22
    st = g.get_state()
    want = torch.empty(n).normal_(0, 1, generator=g)
    if not torch.backends.cpu.get_cpu_capability().startswith(('AVX2', 'AVX512')):
        pytest.skip('torch does not run its AVX2 fill on this host')
    bad = []
    for variant in range(4):
        g.set_state(st)
        u = torch.empty(n).uniform_(0, 1, generator=g)
        assert L.ure_host_normal_blocks_scalar(u.data_ptr(), n // 16, variant) == 0
        bad.append(int((u.view(torch.int32) != want.view(torch.int32)).sum()))
    assert bad[0] == 0 and min(bad[1:]) > 0, bad
    assert L.ure_host_normal_blocks_scalar(u.data_ptr(), 1, 4) != 0


def test_batch_init_and_seed_draws_equal_torchs():
    """ure_host_mf_init_batch (all shards of a request in one call, each from its own generator state) and ure_host_draw_int64 (the per-epoch
    seeds of scratch.py:78-97 off a copy of a state moved past the fills) against torch: tables, end states, seeds."""
    import ctypes
    from ultrare_amd import _native as nv, rng
    if not rng.native_fill_ok():
        pytest.skip('this build does not reproduce torch\'s AVX2 fill')
    L = nv.lib()
    n_user, n_item, k, S, E = 301, 77, 7, 5, 9
    nu, ni = n_user * k, n_item * k
    g = torch.Generator()
    g.manual_seed(11)
    torch.empty(100).normal_(generator=g)
    states, want = [], []
    for s in range(S):
        states.append(g.get_state().clone())
        for rows in (n_user, n_item):                                    # the constructors' fills (skipped by the native call)
            torch.empty(rows, k).normal_(0, 1, generator=g)
        U, V = torch.empty(n_user, k).normal_(0, 1, generator=g), torch.empty(n_item, k).normal_(0, 1, generator=g)
        seeds = torch.empty(E * 4, dtype=torch.int64).random_(generator=g)
        want.append((U, V, seeds, g.get_state().clone()))
    skip = rng.fill_draws(nu) + rng.fill_draws(ni)
    block = torch.empty(S, nu + ni)
    mine = [st.clone() for st in states]
    st_a = (ctypes.c_void_p * S)(*[x.data_ptr() for x in mine])
    u_a = (ctypes.c_void_p * S)(*[block[s].data_ptr() for s in range(S)])
    v_a = (ctypes.c_void_p * S)(*[block[s].data_ptr() + 4 * nu for s in range(S)])
    nv.check(L.ure_host_mf_init_batch(S, st_a, mine[0].numel(), (ctypes.c_int64 * S)(*([skip] * S)), u_a, nu, v_a, ni, 3), 'ure_host_mf_init_batch')
    for s in range(S):
        U, V, seeds, end = want[s]
        assert torch.equal(block[s, :nu].view(n_user, k), U) and torch.equal(block[s, nu:].view(n_item, k), V)
        got = np.empty(E * 4, dtype=np.int64)
        nv.check(L.ure_host_draw_int64(states[s].data_ptr(), states[s].numel(), 2 * skip, E * 4, got.ctypes.data), 'ure_host_draw_int64')
        assert np.array_equal(got, seeds.numpy()) and (got >= 0).all()
        # the batch call leaves every state behind its two kept fills: the seeds follow
        g2 = torch.Generator()
        g2.set_state(mine[s])
        assert torch.equal(torch.empty(E * 4, dtype=torch.int64).random_(generator=g2), seeds) and torch.equal(g2.get_state(), end)
    assert L.ure_host_draw_int64(torch.zeros(5056, dtype=torch.uint8).data_ptr(), 5056, 0, 1, got.ctypes.data) != 0


def test_shard_streams_reproduce_the_sequential_draws():
    """rng.shard_streams / mf_init(generator=) / epoch_seeds(generator=): every shard's draws taken from its own
    generator, positioned by skip-ahead, equal the draws a single generator makes shard after shard with the
    reference's four fills (utils.py:31-40), and the global generator ends where it would have."""
    from ultrare_amd import rng
    n_user, n_item, k, E, S = 300, 211, 8, 3, 4
    torch.manual_seed(7)
    want = []
    for _ in range(S):
        torch.empty(n_user, k).normal_()                      # nn.Embedding constructors: discarded
        torch.empty(n_item, k).normal_()
        U0, V0 = torch.empty(n_user, k).normal_(), torch.empty(n_item, k).normal_()
        seeds = [int(torch.empty((), dtype=torch.int64).random_().item()) for _ in range(4 * E)][1::4]
        want.append((U0, V0, seeds))
    end = torch.get_rng_state()
    torch.manual_seed(7)
    starts, after = rng.shard_streams(S, n_user, n_item, k, E, True)
    assert torch.equal(after, end)
    for memo in ('0', '1', '1'):                              # the seeds read off the walk itself (and out of the memo, the third time)
        os.environ['URE_STREAM_MEMO'] = memo
        torch.manual_seed(7)
        s2, a2, seeds = rng.shard_streams(S, n_user, n_item, k, E, True, want_seeds=True)
        assert torch.equal(a2, end) and all(torch.equal(x, y) for x, y in zip(s2, starts)) and seeds == [w[2] for w in want]
    os.environ.pop('URE_STREAM_MEMO', None)
    for i in reversed(range(S)):                              # any order: the streams are independent
        g = torch.Generator()
        g.set_state(starts[i])
        U0, V0 = rng.mf_init(n_user, n_item, k, generator=g)
        assert torch.equal(U0, want[i][0]) and torch.equal(V0, want[i][1])
        assert rng.epoch_seeds(E, True, generator=g) == want[i][2]
    torch.manual_seed(7)
    for _ in range(S):
        rng.skip_model(n_user, n_item, k, E, True)
    assert torch.equal(torch.get_rng_state(), end)
    # the worker-thread form (no device): same init, seeds expanded to the same permutations
    torch.manual_seed(7)
    starts, _ = rng.shard_streams(S, n_user, n_item, k, E, True)
    for i in range(S):
        init, perms = rng.shard_draws_async(starts[i], n_user, n_item, k, E, True, 500, True, threads=2).result()
        assert torch.equal(init[0], want[i][0]) and torch.equal(init[1], want[i][1])
        for e in range(E):
            assert torch.equal(perms[e], rng.epoch_perm(want[i][2][e], 500))
        rng.release(perms)
    assert rng.model_draws(1, 3, 4, E, True) is None          # tables under 16 elements: ATen's scalar path, replayed not skipped
    torch.manual_seed(7)
    a = rng.mf_init(1, 3, 4)
    torch.manual_seed(7)
    torch.empty(1, 4).normal_(); torch.empty(3, 4).normal_()
    assert torch.equal(a[0], torch.empty(1, 4).normal_()) and torch.equal(a[1], torch.empty(3, 4).normal_())


def test_batched_layout_builder_equals_the_single_one(lib):
    """ure_host_build_layouts (all shards of a call in one native call, from int64 / float64 triples as RatingData holds
    them, packed regions, row_slot) against ure_host_build_layout shard by shard."""
    tr = O.load_csv(TRAIN)
    parts = O.partition(*tr, O.uniform_groups(N_USER, 3))
    raw = [(p[0].astype(np.int64), p[1].astype(np.int64), p[2].astype(np.float64)) for p in parts]
    regs = [np.full(lib.layout_region_words(len(r[0]), N_USER, N_ITEM), 12345, dtype=np.int32) for r in raw]
    n_slots, n_active = lib.build_layouts(raw, N_USER, N_ITEM, regs, threads=3)
    rows = N_USER + N_ITEM
    for p, reg, k, na in zip(parts, regs, n_slots, n_active):
        one = lib.build_layout(p[0].astype(np.int32), p[1].astype(np.int32), p[2].astype(np.float32), N_USER, N_ITEM)
        assert one['n_slots'] == k and one['n_active'] == na
        assert np.array_equal(reg[:k], one['ent_oid']) and np.array_equal(reg[k:2 * k].view(np.float32), one['ent_r'])
        assert np.array_equal(reg[2 * k:3 * k], one['ent_src']) and np.array_equal(reg[3 * k:3 * k + 4 * rows].reshape(rows, 4), one['sched'])
        slot = reg[3 * k + 4 * rows:3 * k + 5 * rows]
        want = np.full(rows, -1, dtype=np.int32)
        want[one['sched'][:na, 0]] = np.arange(na)
        assert np.array_equal(slot, want)
    with pytest.raises(lib.NativeError, match='shard 1'):
        bad = [raw[0], (raw[1][0], raw[1][1] + N_ITEM, raw[1][2]), raw[2]]
        lib.build_layouts(bad, N_USER, N_ITEM, regs, threads=2)


def test_draws_of_a_call_on_few_workers_equal_the_sequential_stream():
    """rng.draws_batch_async: the shards of a call on FEWER worker threads than shards (a worker takes several shards: all their
    inits, then their permutation chunks round robin) give every shard the init and the permutations of its place in the one
    sequential stream; a failing worker never leaves a consumer waiting."""
    from ultrare_amd import rng
    S, n_user, n_item, k, E = 5, 37, 23, 8, 4
    torch.manual_seed(11)
    want = []
    for i in range(S):
        init = rng.mf_init(n_user, n_item, k)
        want.append((init, rng.epoch_seeds(E, True)))
    torch.manual_seed(11)
    starts, _ = rng.shard_streams(S, n_user, n_item, k, E, True)
    specs = [dict(start_state=starts[i], n_user=n_user, n_item=n_item, k=k, epochs=E, with_total_test=True, n_rows=300 + 10 * i, shuffle=True,
                  threads=2) for i in range(S)]
    specs[3].update(n_rows=0, shuffle=False, want_perms=False)         # a shard another rank owns: init only
    draws = rng.draws_batch_async(specs, 2)
    for i, dr in enumerate(draws):
        init = dr.init()
        assert torch.equal(init[0], want[i][0][0]) and torch.equal(init[1], want[i][0][1])
    for i, dr in enumerate(draws):
        perms = dr.perms()
        if i == 3:
            assert perms is None
            continue
        for e in range(E):
            assert torch.equal(perms[e], rng.epoch_perm(want[i][1][e], 300 + 10 * i))
        rng.release(perms)
    bad = dict(specs[0], start_state=torch.zeros(3, dtype=torch.uint8))   # not a generator state: the worker raises
    dr = rng.draws_batch_async([bad], 1)[0]
    with pytest.raises(Exception):
        dr.init()


def test_host_cpus_respects_affinity_and_ranks(monkeypatch):
    from ultrare_amd import rng
    n = rng.host_cpus()
    assert 1 <= n <= len(os.sched_getaffinity(0))
    monkeypatch.setenv('LOCAL_WORLD_SIZE', '2')
    assert rng.host_cpus() == max(1, n // 2) or rng.host_cpus() == max(1, len(os.sched_getaffinity(0)) // 2)
    monkeypatch.setenv('URE_PERM_THREADS', '3')
    assert rng.perm_threads() == 3


def test_upload_many_on_the_host_device():
    from ultrare_amd import engine
    arrs = [np.arange(7, dtype=np.int32), np.linspace(0, 1, 5, dtype=np.float32).reshape(5, 1), np.zeros((0, 4), dtype=np.int64)]
    out = engine.upload_many(arrs, torch.device('cpu'))
    for a, t in zip(arrs, out):
        assert tuple(t.shape) == a.shape and np.array_equal(t.numpy(), a)


def test_work_units_of_several_passes(lib):
    """ure_host_build_units with unit_passes > 1 (touch mode, epochs of several windows): the pieces of a row are unit_passes scan
    passes long, still tile the row's segment without gaps, and a row's units still share one workgroup."""
    from ultrare_amd.engine import ShardData
    tr = O.partition(*O.load_csv(TRAIN), [list(range(N_USER))])[0]
    sh = ShardData(*tr, N_USER, N_ITEM, device=torch.device('cpu'))
    sched = sh._sched_host
    d, lanes = 16, 4
    for passes in (1, 3, 8):
        units = lib.build_units(sched, sh.n_active, d, passes)
        upb = 256 // lanes
        assert len(units) % upb == 0
        cover = {}
        for q, (row, beg, end, word) in enumerate(units.tolist()):
            if row < 0:
                continue
            leader, count = word & 0xFFFF, (word >> 16) & 0x3FFF
            assert q // upb == (q - (q % upb) + leader) // upb              # the row's first unit is in the same workgroup
            cover.setdefault(row, []).append((beg, end))
            assert end - beg <= max(8 * lanes * passes, (sched[sched[:, 0] == row][0][2] - sched[sched[:, 0] == row][0][1] + upb - 1) // upb + 8)
        for row, beg, end, nnz in sched[:sh.n_active].tolist():
            pieces = sorted(cover[row])
            assert pieces[0][0] == beg and pieces[-1][1] == end and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
        if passes > 1:
            assert len(units) < len(lib.build_units(sched, sh.n_active, d, 1))


def test_host_batch_tags_are_the_inverse_permutation_in_batches(monkeypatch):
    """ure_host_randperm_tags (struct ure_shard: file_tags): tags[t][perm_t[b]] = b // batch for the very permutations
    ure_host_randperm / torch.randperm give -- the numbers the device otherwise derives from perm (csrc/tag_prep.h).  And when an order
    travels as tags (rng.tags_batch_for): at most 65535 steps, below ATen's huge-n randperm, unless URE_HOST_TAGS=0."""
    from ultrare_amd import rng
    seeds = [3, 2 ** 40 + 17, 99, 12345678901]
    for n, batch in ((1, 5), (7, 3), (1000, 64), (30001, 30000), (180000, 30000), (5000, 1)):
        if -(-n // batch) > 65535:
            continue
        perms = rng.epoch_perms(seeds, n).numpy()
        tags = rng.epoch_tags(seeds, n, batch, threads=3).numpy().view(np.uint16)
        want = np.empty_like(tags)
        for t in range(len(seeds)):
            want[t, perms[t]] = (np.arange(n) // batch).astype(np.uint16)
        assert np.array_equal(tags, want), (n, batch)
    with pytest.raises(Exception):
        rng.epoch_tags(seeds, 70000, 1)                 # more than 65535 steps per epoch
    monkeypatch.delenv('URE_HOST_TAGS', raising=False)
    huge = rng.RANDPERM_HUGE_N
    for n, batch, want in ((1, 5, 5), (65535, 1, 1), (65536, 1, 0), (0, 64, 0), (100, 0, 0), (65535 * 3000, 3000, 3000),
                           (65535 * 3000 + 1, 3000, 0), (huge - 1, 1 << 20, 1 << 20), (huge, 1 << 20, 0)):
        assert rng.tags_batch_for(n, batch) == want, (n, batch)
    monkeypatch.setenv('URE_HOST_TAGS', '0')
    assert rng.tags_batch_for(1000, 64) == 0 and rng.tags_batch_for(1000, 64, honour_env=False) == 64


def test_layouts_and_units_from_one_native_call():
    """ure_host_build_layouts_units: the work units of a table width built behind every layout by the same call equal what
    ure_host_build_units makes of the layout's schedule, for several shards and widths; a region too small for them reports -1
    and leaves the layout intact."""
    from ultrare_amd import engine, _native as nv
    rs = np.random.RandomState(5)
    n_user, n_item = 300, 500
    triples = []
    for n in (4000, 1, 2500, 9000):
        u = rs.randint(0, n_user, n).astype(np.int64)
        i = (rs.zipf(1.3, n) % n_item).astype(np.int64)
        triples.append((u, i, rs.rand(n)))
    for k in (4, 16, 32, 100, 256):
        d = engine.pad_dim(k)
        shards = engine.build_shards(triples, n_user, n_item, torch.device('cpu'), units_for=k)
        plain = engine.build_shards(triples, n_user, n_item, torch.device('cpu'))
        for sh, ref in zip(shards, plain):
            assert (d, False) in sh._units and (d, False) not in ref._units
            got, n_units, n_rows = sh._units[(d, False)]
            want = nv.build_units(ref._sched_host, ref.n_active, d)
            assert n_units == len(want) and n_rows == sh.n_active and np.array_equal(got.numpy(), want)
            for name in ('ent_oid', 'ent_r', 'ent_src', 'sched'):
                assert torch.equal(getattr(sh, name), getattr(ref, name))
            assert torch.equal(sh.units(d), torch.from_numpy(want))                 # what TrainJob asks for
    # a region without room for the units: -1, layout as usual
    u, i, r = triples[0]
    words = nv.layout_region_words(len(u), n_user, n_item)
    reg = [np.zeros(words, dtype=np.int32)]
    k0, a0 = nv.build_layouts([triples[0]], n_user, n_item, reg)
    exact = (3 * int(k0[0]) + 5 * (n_user + n_item) + 7) // 8 * 8
    # (the binding asks for layout_region_words() words; the library is told that only `exact` + 8 of them may be used)
    import ctypes
    L = nv.lib()
    cols = [np.ascontiguousarray(t, dtype=dt) for t, dt in zip(triples[0], (np.int64, np.int64, np.float64))]
    vp = ctypes.c_void_p
    n = np.array([len(u)], dtype=np.int64)
    region_words = np.array([exact + 8], dtype=np.int64)
    n_slots, n_active, n_units = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int64)
    nv.check(L.ure_host_build_layouts_units(1, (vp * 1)(cols[0].ctypes.data), (vp * 1)(cols[1].ctypes.data), (vp * 1)(cols[2].ctypes.data), n.ctypes.data,
                                            n_user, n_item, (vp * 1)(reg[0].ctypes.data), region_words.ctypes.data, n_slots.ctypes.data,
                                            n_active.ctypes.data, 32, n_units.ctypes.data, 1), 'ure_host_build_layouts_units')
    assert n_units[0] == -1 and n_slots[0] == k0[0] and n_active[0] == a0[0]


def test_shard_streams_memo_returns_the_walked_states():
    """rng.shard_streams walks the generator past every shard's draws (a pure function of the state, the distance and the count); a
    request that starts from a state seen before takes the start states from the memo -- byte for byte what the walk gives, and
    what torch's own generator reaches by making the draws."""
    from ultrare_amd import rng
    torch.manual_seed(42)
    rng._STREAM_MEMO.clear()
    a = rng.shard_streams(3, 40, 30, 4, 2, True)
    hits = rng.STATS.get('memo_hits', 0)
    torch.manual_seed(42)
    b = rng.shard_streams(3, 40, 30, 4, 2, True)
    assert rng.STATS.get('memo_hits', 0) == hits + 1
    for x, y in zip(a[0] + [a[1]], b[0] + [b[1]]):
        assert torch.equal(x, y)
    torch.manual_seed(42)
    for i in range(3):
        assert torch.equal(torch.get_rng_state(), a[0][i])
        for n in (40 * 4, 30 * 4, 40 * 4, 30 * 4):
            torch.empty(n).normal_()
        torch.empty(2 * 4, dtype=torch.int64).random_()
    assert torch.equal(torch.get_rng_state(), a[1])
    b[0][0][100] ^= 1                                        # a caller's copy is its own
    torch.manual_seed(42)
    assert torch.equal(rng.shard_streams(3, 40, 30, 4, 2, True)[0][0], a[0][0])
    # seeds out of the memo: the same total distance split differently -- other table sizes, epochs, draws per epoch -- is
    # another entry, and a hit returns the seeds the sequential draws give
    def sequential(n_user, n_item, k, epochs, per):
        torch.manual_seed(42)
        out = []
        for _ in range(3):
            for n in (n_user * k, n_item * k, n_user * k, n_item * k):
                torch.empty(n).normal_()
            out.append(torch.empty(epochs * per, dtype=torch.int64).random_()[1::per].tolist())
        return out
    for (n_user, n_item, k, epochs, total) in ((40, 30, 4, 2, True), (40, 30, 4, 2, True), (38, 32, 4, 2, True), (40, 28, 4, 4, True), (40, 30, 4, 2, False)):
        torch.manual_seed(42)
        got = rng.shard_streams(3, n_user, n_item, k, epochs, total, want_seeds=True)[2]
        assert got == sequential(n_user, n_item, k, epochs, 4 if total else 3), (n_user, n_item, epochs, total)


def test_layouts_built_on_a_native_thread_equal_the_blocking_call():
    """ure_host_build_layouts_units_start / _wait (the request path: engine.LayoutPlan starts the builder on a thread of the library's own)
    against ure_host_build_layouts_units: the same regions, counts and units; an id out of range comes back through _wait with the
    blocking call's code; a handle is good for one wait."""
    from ultrare_amd import _native as nv
    rs = np.random.RandomState(3)
    n_user, n_item, d = 300, 200, 32
    triples = []
    for n in (5000, 1, 777):
        triples.append((rs.randint(0, n_user, n).astype(np.int64), rs.randint(0, n_item, n).astype(np.int64), rs.randint(1, 6, n) / 5.0))
    words = [nv.layout_region_words(len(t[0]), n_user, n_item) + nv.units_capacity_words(len(t[0]), n_user, n_item, d) for t in triples]
    a = [np.zeros(w, dtype=np.int32) for w in words]
    b = [np.zeros(w, dtype=np.int32) for w in words]
    want = nv.build_layouts(triples, n_user, n_item, a, threads=2, units_d=d)
    job = nv.build_layouts_start(triples, n_user, n_item, b, threads=2, units_d=d)
    got = job.result()
    assert all(np.array_equal(x, y) for x, y in zip(want, got))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert job.result() is got                      # (joined once; the counts stay)
    bad = [(np.array([0, n_user], dtype=np.int64), np.array([0, 0], dtype=np.int64), np.array([0.2, 0.4]))]
    region = [np.zeros(nv.layout_region_words(2, n_user, n_item) + nv.units_capacity_words(2, n_user, n_item, d), dtype=np.int32)]
    job = nv.build_layouts_start(bad, n_user, n_item, region, threads=1, units_d=d)
    with pytest.raises(nv.NativeError) as e:
        job.result()
    assert e.value.code == -2
    assert nv.lib().ure_host_build_layouts_units_wait(12345678) != 0


def test_tag_chunks_and_shuffle_choice():
    """rng.default_tag_bounds / rng.shuffle_method (the chunks of epochs a call's device shuffles are launched in, the kernel family per
    chunk): bounds start at 0, end at the epoch count and rise; a call of small shards starts with one small chunk; csrc/perm_chain.hip makes
    every chunk unless URE_SHUFFLE=reservations asks for csrc/perm_tags.hip, which shards beyond 2^20 rows cannot take."""
    from ultrare_amd import rng
    for epochs in (1, 2, 3, 50, 126, 1000):
        for S in (1, 2, 5, 16, 32, 200):
            for n in (5, 56_000, 180_000, 781_000, 896_914, 4_000_000, 22_500_000):
                b = rng.default_tag_bounds(epochs, S, n)
                assert b[0] == 0 and b[-1] == epochs and all(x < y for x, y in zip(b[:-1], b[1:])), (epochs, S, n, b)
    assert rng.default_tag_bounds(50, 5, 180_000) == [0, 12, 50]
    assert rng.default_tag_bounds(3, 1, 22_500_000) == [0, 1, 2, 3]
    assert rng.shuffle_method(180_000, 250, 'auto') == 'chain' and rng.shuffle_method(56_000, 800, 'auto') == 'chain'
    assert rng.shuffle_method((1 << 20) + 1, 800, 'reservations') == 'chain'
    assert rng.shuffle_method(56_000, 8, 'reservations') == 'reservations' and rng.shuffle_method(56_000, 800, 'chain') == 'chain'


def test_perm_table_is_in_launch_order_and_tiled_by_its_chunks():
    """rng.perm_table, the descriptor table of a call's device shuffles (struct ure_perm), against a plain triple loop over chunk, then
    shard, then epoch: row (s, e) writes its tags at base + 2 * (off[s] + e * n_rows[s]) for the 64-element-aligned offsets of rng._pack,
    and the chunks' row ranges tile the table."""
    from ultrare_amd import rng
    n_rows, epochs, batch, base, bounds = (5, 300, 4099), 5, 64, 1 << 20, [0, 2, 5]
    seeds = [[(s + 1) * 1000003 + e * 17 + (1 << 61) for e in range(epochs)] for s in range(len(n_rows))]
    seeds[1][3] = 2 ** 64 - 3                                           # (a sampler seed with the top bit set: the same bits as int64)
    offs, total = rng._pack([epochs * n for n in n_rows])
    assert offs == [0, 64, 1600] and total == 1600 + 20544 and all(o % 64 == 0 for o in offs + [total])
    table, ranges = rng.perm_table(seeds, n_rows, batch, base, offs, bounds)
    want = []
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        for s, n in enumerate(n_rows):
            for e in range(c0, c1):
                sd = seeds[s][e] - (1 << 64) if seeds[s][e] >= 1 << 63 else seeds[s][e]
                want.append((sd, base + 2 * (offs[s] + e * n), n, batch))
    assert table.dtype == rng.PERM_DTYPE and table.shape == (len(want),)
    assert table.tolist() == want
    assert ranges == [(0, 6), (6, 15)]
    assert ranges[0][0] == 0 and ranges[-1][1] == len(table) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    # a batch size per shard gives the same table as one for all
    per_shard, _ = rng.perm_table(seeds, n_rows, [batch] * len(n_rows), base, offs, bounds)
    assert np.array_equal(per_shard, table)
