"""Poisoned memory for whole jobs and requests: while active, every buffer that torch hands out UNINITIALISED -- torch.empty,
torch.empty_like, Tensor.new_empty -- comes back with every byte set to one fill value, and the library fills every block of
its own job memory with the same byte (URE_BLOCK_FILL, csrc/block_cache.cpp).  A result that differs between two fills was
computed from a byte nobody wrote (the job's rule; tests/test_gpu_job_memory.py).

A plain module like tests/abi_arena.py -- no conftest, no plugin: a test imports it and passes its own monkeypatch, which puts
everything back when the test ends (or when the `with` block does).

    with poison.active(monkeypatch, 0x5A):
        job = engine.TrainJob(...)

The fill runs on the tensor's device on the current stream (Tensor.fill_), where whoever uses the tensor next is ordered behind
it; it works for CPU tensors alike, which is how tests/test_cpu_poison.py checks the helper without a GPU.
"""
import contextlib

import torch

FILLS = (0x00, 0xFF, 0x5A)            # complementary, as abi_arena.PREFILLS
BLOCK_FILL_ENV = 'URE_BLOCK_FILL'


def _filled(t, fill):
    """t with every byte of its storage range set to `fill`; t itself is returned (same dtype, shape and strides)."""
    if t.numel():
        # (a fresh tensor owns its storage: one that is not contiguous -- empty_like of a strided tensor -- is filled storage-wide)
        flat = t.reshape(-1) if t.is_contiguous() else torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size() - t.storage_offset(),), (1,))
        flat.view(torch.uint8).fill_(fill)
    return t


def install(monkeypatch, fill):
    """Poison with byte `fill` until monkeypatch undoes it."""
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError(f'fill {fill!r} is not a byte')
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def poisoned_empty(*args, **kw):
        return _filled(empty(*args, **kw), fill)

    def poisoned_empty_like(*args, **kw):
        return _filled(empty_like(*args, **kw), fill)

    def poisoned_new_empty(self, *args, **kw):
        return _filled(new_empty(self, *args, **kw), fill)

    monkeypatch.setattr(torch, 'empty', poisoned_empty)
    monkeypatch.setattr(torch, 'empty_like', poisoned_empty_like)
    monkeypatch.setattr(torch.Tensor, 'new_empty', poisoned_new_empty)
    monkeypatch.setenv(BLOCK_FILL_ENV, f'{fill:#04x}')


@contextlib.contextmanager
def active(monkeypatch, fill):
    """Poison inside the block only: fill = None leaves everything as it is (the run without the helper) and makes sure the
    library's fill is off as well."""
    with monkeypatch.context() as m:
        if fill is None:
            m.delenv(BLOCK_FILL_ENV, raising=False)
        else:
            install(m, fill)
        yield
