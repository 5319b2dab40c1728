"""csrc/perm_chain.hip, pass by pass: the sizes at which the words kernel's ring, the link pass's two launches and the resolve pass
take another path -- against ure_host_randperm_tags, bit for bit, as tests/test_gpu_shuffle.py does for the chain as a whole."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_HOST = {}


def _host_tags(n, batch, seeds):
    """ure_host_randperm_tags of (n, batch, seeds), made once per module run."""
    from ultrare_amd import _native as nv
    key = (n, batch, tuple(int(s) for s in seeds))
    if key not in _HOST:
        sd = np.asarray(seeds, dtype=np.int64)
        host = torch.empty(len(sd), n, dtype=torch.int16)
        nv.check(nv.lib().ure_host_randperm_tags(sd.ctypes.data, len(sd), n, batch, host.data_ptr(), 0), 'ure_host_randperm_tags')
        _HOST[key] = host
    return _HOST[key]


class _Table:
    """Permutations of one launch: (n, batch) cases, `reps` seeds each; the device table, where the tags go and what they must be."""

    def __init__(self, cases, reps, seed):
        from ultrare_amd import rng
        dev = torch.device('cuda:0')
        rs = np.random.RandomState(seed)
        self.cases, self.want, self.outs, table = cases, [], [], []
        for n, batch in cases:
            seeds = rs.randint(0, 2 ** 62, size=reps).astype(np.int64)
            out = torch.full((reps, n), -1, dtype=torch.int16, device=dev)
            table += [(int(seeds[r]), out.data_ptr() + 2 * n * r, n, batch) for r in range(reps)]
            self.want.append(_host_tags(n, batch, seeds))
            self.outs.append(out)
        self.n_perms, self.n_max = len(table), max(n for n, _ in cases)
        self.dev = torch.from_numpy(np.array(table, dtype=rng.PERM_DTYPE).view(np.uint8)).to(dev)

    def scratch_words(self):
        from ultrare_amd import _native as nv
        return int(nv.lib().ure_device_shuffle_tags_scratch(self.n_max, self.n_perms))

    def flag_at(self):
        from ultrare_amd import _native as nv
        return int(nv.lib().ure_device_shuffle_tags_flag(self.n_max, self.n_perms))

    def launch(self, scratch, range_log2=0):
        from ultrare_amd import _native as nv
        nv.check(nv.lib().ure_device_shuffle_tags(self.dev.data_ptr(), self.n_perms, self.n_max, scratch.data_ptr(), scratch.numel(), range_log2,
                                                  nv.stream_handle()), 'ure_device_shuffle_tags')

    def check(self):
        for (n, batch), host, out in zip(self.cases, self.want, self.outs):
            got = out.cpu()
            assert torch.equal(got, host), (n, batch, int((got != host).sum()))


def _run(cases, reps=3, seed=7, fill=0, range_log2=0):
    tab = _Table(cases, reps, seed)
    scratch = torch.full((tab.scratch_words(),), fill, dtype=torch.int32, device='cuda:0')
    scratch[tab.flag_at()] = 0
    tab.launch(scratch, range_log2)
    torch.cuda.synchronize()
    tab.check()
    assert int(scratch[tab.flag_at()]) == 0


RING, MIRROR, BACK = 8192, 512, 1078      # kDrawRing, kDrawMirror, kDrawBack of csrc/perm_chain.hip


def test_words_ring_layout():
    """Word counts n - 1 on and around: the peeled first step's edges (1, 2; 227 and 454, where a word gains a term; 623, the step's
    width; 624, the start block), the first step whose window lies wholly behind the start block (1,246, 1,247; 1,305, 1,306), the ring's
    length, the end of its mirrored head (first written with word 8,192, last with 8,703), the first window that reaches into the mirror
    (word 8,815 reads ring place 8,192) and the first that starts at place 0 again (9,270), two and three ring lengths, and 30,000 words:
    several times round.  One table, one launch, three seeds each."""
    words = [1, 2, 226, 227, 228, 453, 454, 455, 622, 623, 624, 625, 1246, 1247, 1305, 1306,
             RING - 1, RING, RING + 1, RING + MIRROR - 1, RING + MIRROR, RING + MIRROR + 1,
             RING + BACK - 456 - 1, RING + BACK - 456, RING + BACK - 455, RING + BACK - 454, RING + BACK - 1, RING + BACK, RING + BACK + 1,
             2 * RING + 5, 3 * RING + 5, 30000]
    _run([(w + 1, 3000) for w in words], reps=3, seed=21, fill=-1)


def test_words_ring_from_a_start_block():
    """Just beyond 2^21 rows the stream is cut into segments and a segment's ring is filled from its start block in `states`, not from the
    seed: 2,097,153 + 5 rows, two segments, the second one a few words long."""
    _run([(2_097_153 + 5, 30000)], reps=1, seed=5, fill=0x12345678)


LINK_SIZES = [1000, 1025, 7168, 7169, 8192, 8193, 9217, 16384, 16387]     # at ranges of 1,024 targets: 1, 2, 7, 8, 8, 9, 10, 16 and 17 buckets


@pytest.mark.parametrize('fill', [-1, 0x12345678])
@pytest.mark.parametrize('range_log2', [0, 11, 12, 14])
def test_link_heavy_and_light_launch_cover_every_bucket(fill, range_log2):
    """Permutations with fewer buckets than the heavy launch takes (all of them heavy), exactly as many, one and two more, and twice as
    many, in ONE launch, at every range size: every bucket belongs to exactly one of the two launches.  The scratch starts out full of
    -1 (= "no member") or of 0x12345678: a bucket that neither launch handled leaves a wrong tag or raises the flag."""
    _run([(n, 300) for n in LINK_SIZES], reps=3, seed=33, fill=fill, range_log2=range_log2)


@pytest.mark.parametrize('big_first', [True, False])
def test_two_calls_on_one_scratch_back_to_back(big_first):
    """Two calls with different numbers of permutations and different sizes on ONE scratch and one (non-default) stream, nothing between
    them: the second call's first passes overwrite what the first call's heavy link launch and resolve pass read, so every launch of the
    first call -- the heavy link launch on its own grid included -- must be ordered in front of them."""
    big = _Table([(n, 300) for n in LINK_SIZES], 3, seed=41)
    small = _Table([(9217, 7), (5000, 300), (8193, 1)], 2, seed=43)
    first, second = (big, small) if big_first else (small, big)
    scratch = torch.full((max(big.scratch_words(), small.scratch_words()),), -1, dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        first.launch(scratch)
        second.launch(scratch)
    torch.cuda.synchronize()
    first.check()
    second.check()


@pytest.mark.parametrize('batch', [1, 7, 30000, 65535])
def test_resolve_sizes_and_batches(batch):
    """Around a lane's four rows, a resolve workgroup's 4,096 rows and a row past four workgroups' worth; the batch sizes from 1 (the
    tag is the inverse permutation itself; 65,535 rows: tags up to 65,534) to 65,535 rows per batch (every tag 0).  No row raises the flag."""
    sizes = [1, 2, 3, 4095, 4096, 4097, 4 * 1024 * 4 + 1] + ([65535] if batch == 1 else [])
    _run([(n, batch) for n in sizes], reps=3, seed=51 + batch % 13, fill=0)
