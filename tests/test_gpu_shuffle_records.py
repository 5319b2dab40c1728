"""csrc/perm_chain.hip's launches of RECORDS (every permutation of the table at most 2^20 rows: a swap is ONE word in its bucket's
stretch, j | (t_j - q0) << 20, and the bucket pass works the targets out again from the raw words) against ure_host_randperm_tags, bit
for bit: the smallest shapes at which the format can go wrong, and the first table beyond it, which must take the pair path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHES = (1, 7, 30000)
# n = 1, 2, 3; the edges of a bucket of 1,024 targets; of a tile of 16,384 swaps (n - 1 = 16384 k); 65537; the largest j and the top
# bits of a record.  14 permutations of 14 lengths: more than the eight XCD slots.
RECORDS = [1, 2, 3, 1023, 1024, 1025, 2049, 16384, 16385, 16386, 32769, 65537, (1 << 20) - 1, 1 << 20]
# one row too many for records beside permutations of a few rows and more: nine lengths, the pair path
PAIRS = [(1 << 20) + 1, 5, 1, 2, 3, 1025, 2049, 16385, 65537]


def _batch_of(i, n):
    """The batch sizes in turn; a tag is 16 bits, so a length with more than 65,535 steps at its turn's size takes the next larger one."""
    return next(b for b in BATCHES[i % len(BATCHES):] if (n + b - 1) // b <= 65535)


class _Table:
    """Permutations of the given lengths (batch sizes in turn from BATCHES), their tags by the host (made once), their device outputs."""

    def __init__(self, sizes, seed):
        from ultrare_amd import _native as nv, rng
        self.nv, self.L = nv, nv.lib()
        dev = torch.device('cuda:0')
        rs = np.random.RandomState(seed)
        self.cases = [(n, _batch_of(i, n)) for i, n in enumerate(sizes)]
        self.want, self.outs, table = [], [], []
        for n, batch in self.cases:
            seeds = rs.randint(0, 2 ** 62, size=1).astype(np.int64)
            host = torch.empty(1, n, dtype=torch.int16)
            nv.check(self.L.ure_host_randperm_tags(seeds.ctypes.data, 1, n, batch, host.data_ptr(), 0), 'ure_host_randperm_tags')
            out = torch.full((n,), -1, dtype=torch.int16, device=dev)
            table.append((int(seeds[0]), out.data_ptr(), n, batch))
            self.want.append(host[0])
            self.outs.append(out)
        self.rows = np.array(table, dtype=rng.PERM_DTYPE)
        self.dev = dev

    def words(self, n_perms=None):
        n_perms = len(self.cases) if n_perms is None else n_perms
        return int(self.L.ure_device_shuffle_tags_scratch(max(n for n, _ in self.cases[:n_perms]), n_perms))

    def run(self, scratch, n_perms=None):
        """One call for the first n_perms permutations on `scratch`; the flag word cleared before and read 0 behind; every output equal."""
        n_perms = len(self.cases) if n_perms is None else n_perms
        n_max = max(n for n, _ in self.cases[:n_perms])
        tab_d = torch.from_numpy(self.rows[:n_perms].copy().view(np.uint8)).to(self.dev)
        flag_at = int(self.L.ure_device_shuffle_tags_flag(n_max, n_perms))
        scratch[flag_at] = 0
        for o in self.outs[:n_perms]:
            o.fill_(-1)
        self.nv.check(self.L.ure_device_shuffle_tags(tab_d.data_ptr(), n_perms, n_max, scratch.data_ptr(), scratch.numel(), 0, self.nv.stream_handle()),
                      'ure_device_shuffle_tags')
        torch.cuda.synchronize()
        for (n, batch), host, out in list(zip(self.cases, self.want, self.outs))[:n_perms]:
            got = out.cpu()
            assert torch.equal(got, host), (n, batch, int((got != host).sum()))
        assert int(scratch[flag_at]) == 0


def _fill_value(word):
    return int(np.array(word, dtype=np.uint32).view(np.int32)) if word > 0x7fffffff else word


@pytest.mark.parametrize('sizes', [RECORDS, PAIRS], ids=['records', 'pairs_beyond_2_to_20'])
def test_shuffle_tags_of_a_table_on_dirty_scratch(sizes):
    """Each table twice on ONE scratch, filled with 0xFFFFFFFF before the first call and with 0x12345678 before the second."""
    t = _Table(sizes, seed=23)
    scratch = torch.empty(t.words(), dtype=torch.int32, device=t.dev)
    for word in (0xFFFFFFFF, 0x12345678):
        scratch.fill_(_fill_value(word))
        t.run(scratch)


def test_two_calls_of_different_n_perms_on_one_scratch():
    """The scratch of the larger call serves a smaller one: the regions move (per-permutation stride, the count matrix, the flag word), so
    the second call runs over whatever the first left where its own regions lie -- and the first again over the second's leavings."""
    sizes = [65537, 16385, 1025, 32769, 3, 2049, 16386, 1, 1024, 1023, 16384, 2]
    t = _Table(sizes, seed=29)
    scratch = torch.zeros(max(t.words(), t.words(3)), dtype=torch.int32, device=t.dev)
    t.run(scratch)
    t.run(scratch, n_perms=3)
    t.run(scratch)
