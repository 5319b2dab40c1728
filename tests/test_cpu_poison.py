"""tests/poison.py on the CPU: every spelling by which the engine takes uninitialised memory from torch is caught, for every
dtype it uses, every byte of the tensor holds the fill, and the originals are back afterwards -- so that the fills of
tests/test_gpu_job_memory.py are fills of something."""
import os

import numpy as np
import pytest
import torch

import poison

DTYPES = [torch.int16, torch.int32, torch.float32, torch.float64, torch.uint8]


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).numpy() if t.dim() else t.reshape(1).view(torch.uint8).numpy()


@pytest.mark.parametrize('fill', poison.FILLS)
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_all_three_spellings_return_filled_memory(dtype, fill, monkeypatch):
    like = torch.zeros(5, 3, dtype=dtype)
    with poison.active(monkeypatch, fill):
        got = {'empty': torch.empty(7, 3, dtype=dtype), 'empty kw': torch.empty(size=(4,), dtype=dtype, device='cpu'),
               'empty 0-dim': torch.empty((), dtype=dtype), 'empty none': torch.empty(0, dtype=dtype),
               'empty_like': torch.empty_like(like), 'empty_like dtype': torch.empty_like(torch.zeros(3, 2), dtype=dtype),
               'empty_like strided': torch.empty_like(torch.zeros(4, 6, dtype=dtype).t()),
               'new_empty': like.new_empty(9), 'new_empty tuple': like.new_empty((2, 5)), 'new_empty dtype': torch.zeros(2).new_empty(3, dtype=dtype)}
    shapes = {'empty': (7, 3), 'empty kw': (4,), 'empty 0-dim': (), 'empty none': (0,), 'empty_like': (5, 3), 'empty_like dtype': (3, 2),
              'empty_like strided': (6, 4), 'new_empty': (9,), 'new_empty tuple': (2, 5), 'new_empty dtype': (3,)}
    for name, t in got.items():
        assert t.dtype == dtype and tuple(t.shape) == shapes[name], name
        assert (_bytes(t) == fill).all(), (name, fill)
    assert got['empty_like strided'].stride() == (1, 6)            # (the normal tensor: strides preserved)


def test_the_fill_is_the_byte_pattern_not_the_value(monkeypatch):
    with poison.active(monkeypatch, 0x5A):
        assert int(torch.empty(1, dtype=torch.int32)[0]) == 0x5A5A5A5A
        assert int(torch.empty(1, dtype=torch.int16)[0]) == 0x5A5A
        assert torch.empty(1, dtype=torch.float32).view(torch.int32)[0] == 0x5A5A5A5A
    with poison.active(monkeypatch, 0xFF):
        assert torch.isnan(torch.empty(3, dtype=torch.float32)).all() and torch.isnan(torch.empty(3, dtype=torch.float64)).all()
        assert int(torch.empty(1, dtype=torch.int32)[0]) == -1


def test_originals_and_environment_are_back_afterwards(monkeypatch):
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    monkeypatch.setenv(poison.BLOCK_FILL_ENV, '7')                 # (whatever the caller had stays the caller's)
    with poison.active(monkeypatch, 0xFF):
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
        assert int(os.environ[poison.BLOCK_FILL_ENV], 0) == 0xFF
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    assert os.environ[poison.BLOCK_FILL_ENV] == '7'
    with poison.active(monkeypatch, None):                         # the run without the helper: nothing patched, the library's fill off
        assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
        assert poison.BLOCK_FILL_ENV not in os.environ
    assert os.environ[poison.BLOCK_FILL_ENV] == '7'


def test_the_environment_value_is_one_the_library_parses(monkeypatch):
    for fill in poison.FILLS:
        with poison.active(monkeypatch, fill):
            text = os.environ[poison.BLOCK_FILL_ENV]
            assert text.startswith('0x') and int(text, 16) == fill


def test_a_fill_that_is_no_byte_is_refused(monkeypatch):
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            with poison.active(monkeypatch, bad):
                pass
    assert np.array_equal(_bytes(torch.zeros(2, dtype=torch.int16)), np.zeros(4, np.uint8))
