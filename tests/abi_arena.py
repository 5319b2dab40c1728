"""One byte arena for all the buffers of one C-ABI call: inputs, outputs, scratch and tables of pointers are carved out
of ONE torch.uint8 tensor, every buffer on a 256-byte boundary with at least GUARD bytes of guard zone before and after
it.  Every byte of the arena that belongs to no buffer is a guard byte and holds (its offset modulo 251), a pattern that
no constant prefill equals over two consecutive bytes.  Outputs and scratch are prefilled with one byte value before a
call; after it, Arena.collect() reports every guard byte and every input byte that changed and hands the outputs back
as raw bytes, so that NaN and -0.0 compare by pattern.

The arena works on a CPU tensor as well (tests/test_cpu_abi_arena.py plants faults in it), and is no pytest plugin: a
test imports it like any module.

    A = Arena(device)
    A.input('x', x_numpy)            # bytes the call must leave alone
    A.output('y', n * 4)             # bytes the call must write, all of them
    A.scratch('ws', sizer(...))      # exactly the sizer's size; may be 0 bytes (still fenced by guards)
    A.load(0xFF)                     # guards, inputs, prefill -> the device
    lib.ure_xxx(A.addr('x'), ..., A.addr('y'), A.addr('ws'), A.size('ws'), stream)
    rep = A.collect()                # rep.guards, rep.inputs: lists of Changed; rep.outputs: {name: bytes}
"""
import collections

import numpy as np
import torch

ALIGN = 256
GUARD = 4096          # a layout choice (a page), not a measurement
GUARD_MOD = 251       # prime, so the pattern never lines up with a power-of-two stride
PREFILLS = (0x00, 0xFF, 0x5A)

Changed = collections.namedtuple('Changed', 'buffer offset count first')
Changed.__doc__ = """Bytes that differ from what load() put there: `count` of them, the first at byte `offset` relative to
the START of `buffer` (negative: in the guard zone before it; >= its size: behind it), `first` = (was, is)."""

Report = collections.namedtuple('Report', 'guards inputs outputs scratch')


def guard_pattern(lo, hi):
    return (np.arange(lo, hi, dtype=np.int64) % GUARD_MOD).astype(np.uint8)


class Arena:
    def __init__(self, device='cpu', guard=GUARD):
        self.device, self.guard = torch.device(device), int(guard)
        self.buffers = collections.OrderedDict()        # name -> [kind, nbytes, data, offset]
        self.mem = self.image = None

    # ---- declaring buffers ---------------------------------------------------------------------------------------
    def _add(self, name, kind, nbytes, data=None):
        assert self.mem is None, 'declare every buffer before load()'
        assert name not in self.buffers, name
        self.buffers[name] = [kind, int(nbytes), data, None]
        return name

    def input(self, name, data, nbytes=None):
        """data: a numpy array (its bytes), or a callable(arena) -> numpy array evaluated at load() once the addresses
        are known (a device table of pointers into the arena; nbytes then gives its size)."""
        if callable(data):
            return self._add(name, 'in', nbytes, data)
        data = np.ascontiguousarray(data)
        return self._add(name, 'in', data.nbytes, data)

    def output(self, name, nbytes):
        return self._add(name, 'out', nbytes)

    def scratch(self, name, nbytes):
        return self._add(name, 'scratch', nbytes)

    # ---- layout ------------------------------------------------------------------------------------------------------
    def _layout(self):
        at = 0
        for b in self.buffers.values():
            at = -(-(at + self.guard) // ALIGN) * ALIGN
            b[3] = at
            at += b[1]
        self.total = at + self.guard
        self.mem = torch.zeros(self.total, dtype=torch.uint8, device=self.device)
        self.is_guard = np.ones(self.total, dtype=bool)
        for kind, n, _, off in self.buffers.values():
            self.is_guard[off:off + n] = False

    def offset(self, name):
        return self.buffers[name][3]

    def size(self, name):
        return self.buffers[name][1]

    def addr(self, name):
        """The buffer's address; None (NULL) for name None -- an optional argument left out."""
        if name is None:
            return None
        if self.mem is None:
            self._layout()
        return self.mem.data_ptr() + self.offset(name)

    def view(self, name, dtype=torch.uint8, shape=None):
        """The buffer as a tensor that aliases the arena (what a Python 'kernel' writes through)."""
        if self.mem is None:
            self._layout()
        off, n = self.offset(name), self.size(name)
        t = self.mem[off:off + n].view(dtype)
        return t if shape is None else t.view(*shape)

    # ---- one call ----------------------------------------------------------------------------------------------------
    def load(self, prefill):
        """Guards, inputs and the prefill byte in every output and scratch byte, built on the host and copied in one go."""
        if self.mem is None:
            self._layout()
        img = guard_pattern(0, self.total)
        for name, (kind, n, data, off) in self.buffers.items():
            if callable(data):
                data = np.ascontiguousarray(data(self))
            if data is not None:
                raw = data.reshape(-1).view(np.uint8)
                assert raw.size == n, (name, raw.size, n)
                img[off:off + n] = raw
            else:
                img[off:off + n] = prefill
        self.image, self.prefill = img, prefill
        self.mem.copy_(torch.from_numpy(img))
        return self

    def _changes(self, now, mask):
        """Changed records of the bytes under `mask` that differ from the loaded image, grouped by the nearest buffer."""
        bad = np.flatnonzero(mask & (now != self.image))
        out = []
        if bad.size == 0:
            return out
        names = list(self.buffers)
        starts = np.array([self.offset(n) for n in names])
        ends = starts + np.array([self.size(n) for n in names])
        # a guard byte belongs to the buffer whose edge is nearest; an input byte to its own buffer (distance 0)
        dist = np.maximum(np.maximum(starts[None, :] - bad[:, None], bad[:, None] - (ends[None, :] - 1)), 0)
        owner = np.argmin(dist, axis=1)
        for i in np.unique(owner):
            mine = bad[owner == i]
            out.append(Changed(names[i], int(mine[0] - starts[i]), int(mine.size), (int(self.image[mine[0]]), int(now[mine[0]]))))
        return out

    def collect(self):
        """After the call (and a synchronise on a device): what changed where it must not, and the outputs as bytes."""
        now = self.mem.cpu().numpy()
        is_input = np.zeros(self.total, dtype=bool)
        outputs, scratch = {}, {}
        for name, (kind, n, data, off) in self.buffers.items():
            if kind == 'in':
                is_input[off:off + n] = True
            elif kind == 'out':
                outputs[name] = now[off:off + n].tobytes()
            else:
                scratch[name] = now[off:off + n].tobytes()
        return Report(self._changes(now, self.is_guard), self._changes(now, is_input), outputs, scratch)


def run_prefills(arena, call, prefills=PREFILLS, sync=None):
    """call(arena) once per prefill -> [Report]; sync() after each call (torch.cuda.synchronize on a device)."""
    reports = []
    for p in prefills:
        arena.load(p)
        call(arena)
        if sync is not None:
            sync()
        reports.append(arena.collect())
    return reports


def verdict(reports, prefills=PREFILLS, keep=None):
    """The findings of one case as a list of strings (empty: the memory contract holds).  keep: {output name: bool mask
    over its bytes} -- the bytes an in-place entry must NOT write; they must still hold the prefill and are left out of
    the comparison."""
    keep = keep or {}
    found = []
    for p, r in zip(prefills, reports):
        for c in r.guards:
            found.append(f'prefill {p:#04x}: {c.count} guard byte(s) changed near {c.buffer!r}, first at offset {c.offset} '
                         f'({c.first[0]:#04x} -> {c.first[1]:#04x})')
        for c in r.inputs:
            found.append(f'prefill {p:#04x}: {c.count} byte(s) of input {c.buffer!r} changed, first at offset {c.offset} '
                         f'({c.first[0]:#04x} -> {c.first[1]:#04x})')
        for name, mask in keep.items():
            got = np.frombuffer(r.outputs[name], dtype=np.uint8)
            bad = np.flatnonzero(mask & (got != p))
            if bad.size:
                found.append(f'prefill {p:#04x}: {bad.size} byte(s) of {name!r} that the call must not write changed, first at offset {int(bad[0])}')
    first = reports[0]
    for p, r in zip(prefills[1:], reports[1:]):
        for name in first.outputs:
            a = np.frombuffer(first.outputs[name], dtype=np.uint8)
            b = np.frombuffer(r.outputs[name], dtype=np.uint8)
            diff = a != b
            if name in keep:
                diff &= ~keep[name]
            bad = np.flatnonzero(diff)
            if bad.size:
                i = int(bad[0])
                found.append(f'output {name!r}: {bad.size} byte(s) differ between prefill {prefills[0]:#04x} and {p:#04x}, first at offset {i} '
                             f'({a[i]:#04x} vs {b[i]:#04x}): unwritten, or computed from stale memory')
    return found
