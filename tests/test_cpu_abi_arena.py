"""The guarded arena of tests/abi_arena.py must be able to FAIL: plain Python "kernels" write into a CPU arena and commit
one fault each, every fault is reported and the clean kernel passes.  Then the host side of tests/test_gpu_abi_memory.py:
every bound name of ultrare_amd/_native.py is classified, every case builds without a device, and the sizers return what
their entries accept and refuse."""
import numpy as np
import pytest
import torch

import test_gpu_abi_memory as M
from abi_arena import ALIGN, GUARD, PREFILLS, Arena, run_prefills, verdict

N = 100          # floats per buffer: 400 bytes, so that no buffer ends on the 256-byte boundary the next one starts on


def _arena():
    A = Arena('cpu')
    A.input('x', np.arange(N, dtype=np.float32) + 1)
    A.output('y', N * 4)
    A.scratch('ws', N * 4)
    return A


def _kernel(fault=None):
    """y = 2 x through a scratch copy of x, as a kernel would stage it; `fault` plants one error."""
    def call(A):
        x, y, ws = A.view('x', torch.float32), A.view('y', torch.float32), A.view('ws', torch.float32)
        flat = A.mem.view(torch.uint8)
        n_ws = N - 1 if fault == 'stale_scratch' else N
        ws[:n_ws] = x[:n_ws]                                 # (stale_scratch: the last scratch word is never written ...)
        y[:] = 2 * ws                                        # (... and still read)
        if fault == 'unwritten_byte':
            flat[A.offset('y') + 17] = A.prefill             # one output byte as the prefill left it
        if fault == 'past_output':
            flat[A.offset('y') + 4 * N:A.offset('y') + 4 * N + 4] = torch.tensor([0, 0, 0x80, 0x3f], dtype=torch.uint8)      # y[N] = 1.0f
        if fault == 'past_scratch':
            flat[A.offset('ws') + 4 * N:A.offset('ws') + 4 * N + 4] = torch.tensor([0, 0, 0x80, 0x3f], dtype=torch.uint8)
        if fault == 'before_output':
            flat[A.offset('y') - 1] = 0xEE
        if fault == 'input_overwritten':
            x[5] = -1.0
    return call


def test_layout_guards_every_buffer_on_both_sides():
    A = _arena().load(0x5A)
    offs = [(A.offset(n), A.size(n)) for n in ('x', 'y', 'ws')]
    end = 0
    for off, size in offs:
        assert off % ALIGN == 0 and off - end >= GUARD
        end = off + size
    assert A.total - end == GUARD
    img = A.mem.numpy()
    assert (img[A.is_guard] == (np.flatnonzero(A.is_guard) % 251)).all()                  # the guard pattern: offset modulo 251
    assert (img[A.offset('y'):A.offset('y') + 4 * N] == 0x5A).all() and (img[A.offset('ws'):A.offset('ws') + 4 * N] == 0x5A).all()
    assert np.array_equal(A.view('x', torch.float32).numpy(), np.arange(N, dtype=np.float32) + 1)
    # no constant prefill equals the pattern over two consecutive bytes
    pat = np.arange(A.total) % 251
    assert all(not ((pat[:-1] == p) & (pat[1:] == p)).any() for p in PREFILLS)


def test_clean_kernel_passes():
    A = _arena()
    reports = run_prefills(A, _kernel())
    assert verdict(reports) == []
    assert reports[0].outputs['y'] == (2 * (np.arange(N, dtype=np.float32) + 1)).tobytes()
    assert all(not r.guards and not r.inputs for r in reports)


@pytest.mark.parametrize('fault,words', [
    ('unwritten_byte', ["output 'y'", 'offset 17']),
    ('stale_scratch', ["output 'y'", f'offset {4 * (N - 1)}']),
    ('past_output', ["guard byte(s) changed near 'y'", f'offset {4 * N}']),
    ('past_scratch', ["guard byte(s) changed near 'ws'", f'offset {4 * N}']),
    ('before_output', ["guard byte(s) changed near 'y'", 'offset -1']),
    ('input_overwritten', ["input 'x' changed", 'offset 22']),          # 6.0f -> -1.0f: the low two bytes of x[5] are 0 in both
])
def test_planted_fault_is_reported(fault, words):
    found = verdict(run_prefills(_arena(), _kernel(fault)))
    assert found, fault
    assert any(all(w in line for w in words) for line in found), (fault, found)
    if fault in ('past_output', 'past_scratch', 'before_output', 'input_overwritten'):
        assert len(found) == len(PREFILLS)                   # seen under every prefill, and nothing else is reported
    else:
        assert all("output 'y'" in line for line in found)


def test_kept_bytes_must_hold_the_prefill():
    """An in-place entry: the rows it does not name are left out of the comparison and must still hold the prefill."""
    def build():
        A = Arena('cpu')
        A.input('x', np.arange(8, dtype=np.float32))
        A.output('y', 64)
        return A
    keep = np.ones(64, dtype=bool)
    keep[8:16] = False

    def good(A):
        A.view('y', torch.float32)[2:4] = A.view('x', torch.float32)[2:4]

    def bad(A):
        good(A)
        A.view('y', torch.float32)[7] = 1.0
    assert verdict(run_prefills(build(), good), keep={'y': keep}) == []
    assert any('must not write' in line for line in verdict(run_prefills(build(), bad), keep={'y': keep}))
    assert verdict(run_prefills(build(), good)) != []        # without the mask the untouched rows read as unwritten


def test_late_bound_pointer_tables_and_empty_buffers():
    A = Arena('cpu')
    A.output('a', 12)
    A.scratch('none', 0)
    A.input('table', lambda A: np.array([A.addr('a'), A.addr('none')], dtype=np.uint64), nbytes=16)
    A.load(0xFF)
    tab = A.view('table', torch.int64).numpy().view(np.uint64)
    assert tab[0] == A.mem.data_ptr() + A.offset('a') and tab[1] == A.addr('none') and A.size('none') == 0
    assert A.addr(None) is None
    A.mem[A.offset('none')] = 0                              # a store "into" the empty buffer lands in its guard
    rep = A.collect()
    assert [c.buffer for c in rep.guards] == ['none'] and rep.guards[0].offset == 0 and rep.scratch['none'] == b''


# ---- the host side of the device cases ---------------------------------------------------------------------------------
def test_every_bound_name_is_classified():
    from ultrare_amd import _native as nv
    missing = [n for n in nv.EXPORTS if n not in M.INVENTORY]
    assert not missing, f'no memory class for {missing}: add an arena case (or name the class) in tests/test_gpu_abi_memory.py'
    assert not [n for n in M.INVENTORY if n not in nv.EXPORTS]
    assert len(M.INVENTORY) == len(nv.EXPORTS) == 96
    for name, (klass, note) in M.INVENTORY.items():
        assert klass in M.CLASSES, name
        if klass == 'sizer':
            assert name.endswith(('_scratch', '_len', '_flag', '_splits')), name
        if klass == 'host':
            assert name.startswith(('ure_host_', 'ure_ot_')) or name in ('ure_abi_version', 'ure_source_hash', 'ure_last_error', 'ure_device_info'), name
        if klass == 'stateful':
            assert name.startswith('ure_job_') and '::test_' in note
        if klass in ('prefilled', 'stateful'):
            path, test = note.split('::')
            assert test in open(__file__.rsplit('tests', 1)[0] + path).read(), note
    covered = {c.entry for c in M.CASES}
    arena = {n for n, (klass, _) in M.INVENTORY.items() if klass == 'arena'}
    assert covered == arena, (sorted(arena - covered), sorted(covered - arena))


def test_removing_a_name_from_the_table_fails(monkeypatch):
    table = dict(M.INVENTORY)
    del table['ure_pair_knn']
    monkeypatch.setattr(M, 'INVENTORY', table)
    with pytest.raises(AssertionError, match='ure_pair_knn'):
        test_every_bound_name_is_classified()


def test_cases_build_without_a_device_and_their_sizers_accept_them():
    """Every case declares its buffers on a CPU arena; each sizer it asks returns >= 0 (Plan.sizer asserts it), the scratch
    has exactly that size, and every sizer but the shuffle's two (run by tests/test_gpu_shuffle.py) is asked by some case."""
    asked = set()
    for case in M.CASES:
        P = case.build(Arena('cpu'))
        P.A.load(0xFF)                                       # the layout holds together
        assert P.call is not None and P.want is not None, case.id
        asked |= {name for name, _, _ in P.sizers}
        for name, args, value in P.sizers:
            assert value >= 0, (case.id, name, args)
        assert all(mask.dtype == bool and mask.size == P.A.size(name) for name, mask in P.keep.items()), case.id
    sizers = {n for n, (klass, _) in M.INVENTORY.items() if klass == 'sizer'}
    assert sizers - asked == {'ure_device_shuffle_tags_scratch', 'ure_device_shuffle_tags_flag'}, sorted(sizers - asked)


@pytest.mark.parametrize('name,args', M.SIZER_REFUSALS, ids=[f'{n[4:]}{a}'.replace(' ', '') for n, a in M.SIZER_REFUSALS])
def test_sizers_refuse_what_their_entries_refuse(name, args):
    from ultrare_amd import _native as nv
    assert int(getattr(nv.lib(), name)(*args)) == -1


def test_sizers_at_the_edge_of_what_they_accept():
    from ultrare_amd import _native as nv
    L = nv.lib()
    assert L.ure_csr_cost_scratch(1) == 8 and L.ure_csr_cost_scratch(256) == 8 * 256
    assert L.ure_csr_kmeans_cost_scratch(1) == 4 and L.ure_csr_kmeans_cost_scratch(256) == 4 * 256
    assert L.ure_mmd_scratch(129, 128) > 0 and L.ure_mmd_splits(129, 128) == 3 and L.ure_mmd_scratch(129, 0) == -1 and L.ure_mmd_scratch(1, 8) == -1
    assert L.ure_balanced_fill_scratch(320, 5) == 4096 + 8 * 320
    assert L.ure_balanced_fill_scratch((1 << 32) // 256 - 1, 256) > 0 and L.ure_balanced_fill_scratch((1 << 32) // 256, 256) == -1
