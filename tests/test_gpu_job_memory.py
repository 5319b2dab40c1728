"""Whole training jobs and whole requests on poisoned memory (the job's rule: every byte a launch of a job reads was
either filled by ure_job_create or written by an earlier launch of the same job).

tests/poison.py makes every buffer torch hands out uninitialised, and every block of library-owned job memory (URE_BLOCK_FILL,
csrc/block_cache.cpp), start as 0x00, 0xFF or 0x5A in every byte.  Each case builds its job once per fill and collects every byte
a caller can obtain -- tables, padded tables, losses, snapshots, the touch accounting and, in touch_mode 3, the slot index of the last
epoch.  The three runs and a fourth without the helper must give equal bytes, array by array (complementary fills: a byte that is
read before the job wrote it shows in at least one of them), and the 0x00 run must agree with the reference the project already
holds these kernels to -- the C oracle within rel < 2e-5 on the tables and rtol = 2e-5 on the RMSE series (tests/test_gpu_touch.py),
the bound of tests/test_gpu_adam.py for Adam, train_ref(float32) bit for bit for LightGCN -- which ties the four equal results to
a reference.  The fill is the parameter that varies fastest, 0x00 first, so a failure names its pattern.

The shapes are the smallest that make each group of arrays exist (the toy set, 1508 x 2071 with 28 k ratings, k = 16, E = 2
unless a case says otherwise):
  W1  touch_mode 1, 65 steps: two windows, the second of one step -- row masks, work-order masks, pass masks
  W2  touch_mode 2: the second set of work-order masks and the 0xFF hand-over bytes
  W3  touch_mode 1, three shards of different length in one launch, k = 32
  I1  touch_mode 3, three unequal shards, <= 63 steps: one mask word, idx_scatter_short_kernel, chunks of 1,024 slots
  I2  touch_mode 3, 65 steps: two mask words and next_first, the staged and the direct scatter, chunks of 4,096 with a ragged last one
  I3  touch_mode 3, 750 steps: twelve mask words
  I4  touch_mode 3, one item with 5,000 of 5,600 interactions: heavy and split rows -- partial, heavy_map, heavy_cum, step_desc, the
      second launch that adds the parts; thresholds of 1 put all 256 prefix rows into the workgroup classes; compact snapshots
  I5  touch_mode 3, k = 128: two float4 per lane, partial rows of d + 4
  D1  the default kernel, three shards, compact snapshots (_snap_pool comes from torch.empty)
  D2  the default kernel with Adam (vU, vV, the per-step scalars), on the 70 x 50 case of tests/adam_cases.py at d = 32
  G1  a GcnJob on the smallest case of tests/lightgcn_cases.py with empty rows and a row longer than a lane group's stride
"""
import os

import numpy as np
import pytest
import torch

import adam_cases
import lightgcn_cases
import poison
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
TRAIN = os.path.join(G, 'toy', '0_train.csv')
N_USER, N_ITEM = 1508, 2071
FILLS = [0x00, 0xFF, 0x5A, None]                      # None: the helper off
FILL_IDS = ['fill0x00', 'fill0xff', 'fill0x5a', 'nofill']
INDEX_ARRAYS = ('step_begin', 'step_item', 'items', 'sslot', 'W', 'heavy_cnt', 'heavy_cum')


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------- the cases: host inputs made once, the job made per fill
class MfCase:
    """A TrainJob on host inputs: parts [(uid, iid, rating)], inits [(U0, V0)] and perms [[E, N]] as CPU arrays, made once per process."""

    def __init__(self, name, S=1, k=16, B=3000, E=2, n_rows=None, scale=1.0, seed=42, env=(), patch=(), heavy=False, **job_kw):
        self.name, self.S, self.k, self.B, self.E, self.env, self.patch, self.job_kw = name, S, k, B, E, dict(env), dict(patch), job_kw
        self._n_rows, self._scale, self._seed, self._heavy, self._inputs = n_rows, scale, seed, heavy, None
        self.n_user, self.n_item = (5200, 40) if heavy else (N_USER, N_ITEM)

    def inputs(self):
        from ultrare_amd import rng
        if self._inputs is None:
            if self._heavy:                                   # the shard of test_touch_index_mode_heavy_and_split_rows
                rs = np.random.RandomState(3)
                u = np.concatenate([rs.permutation(self.n_user)[:5000], rs.randint(0, self.n_user, 600)])
                i = np.concatenate([np.zeros(5000, dtype=np.int64), rs.randint(1, self.n_item, 600)])
                key = np.unique(u.astype(np.int64) * self.n_item + i)
                u, i = (key // self.n_item).astype(np.int32), (key % self.n_item).astype(np.int32)
                parts = [(u, i, (rs.randint(1, 6, len(u)) / 5).astype(np.float32))]
            else:
                parts = O.partition(*O.load_csv(TRAIN), O.uniform_groups(N_USER, self.S))
                if self._n_rows:
                    parts = [tuple(x[:self._n_rows] for x in p) for p in parts]
            torch.manual_seed(self._seed)
            inits = [tuple(t * self._scale for t in rng.mf_init(self.n_user, self.n_item, self.k)) for _ in parts]
            perms = [rng.epoch_perms(rng.epoch_seeds(self.E, True), len(p[0])) for p in parts]
            self._inputs = (parts, inits, perms)
        return self._inputs

    def prepare(self, m):
        from ultrare_amd import engine
        for key, value in self.env.items():
            m.setenv(key, value)
        for key, value in self.patch.items():
            m.setattr(engine, key, value)

    def make(self):
        from ultrare_amd import engine
        parts, inits, perms = self.inputs()
        shards = [engine.ShardData(*p, self.n_user, self.n_item) for p in parts]
        return engine.TrainJob(shards, inits, perms, self.k, self.B, self.E, 1e-3, 0.1, 0.9, 0.95, **self.job_kw)

    def run(self):
        """-> {array name: numpy array}: every byte the caller of the trained job can obtain."""
        job = self.make()
        self.check_mode(job)
        job.run()
        out = {}
        for s in range(self.S):
            U, V = job.tables(s)
            pU, pV = job.padded_tables(s)
            out.update({f'U{s}': U, f'V{s}': V, f'padded U{s}': pU, f'padded V{s}': pV, f'sse{s}': job.epoch_sse(s)})
            if job.snapshots:
                out[f'snap{s}'] = job.state[s]['snap']
            if job.optimizer == 'adam':
                out.update({f'{name}{s}': job.state[s][name] for name in ('mU', 'mV', 'vU', 'vV')})
            if job.index:
                arrays = {name: job.index_array(s, name) for name in INDEX_ARRAYS}
                arrays['sslot'] = arrays['sslot'][:int(arrays['step_begin'][job.steps_per_epoch(s)])]
                out.update({f'index {name}{s}': a for name, a in arrays.items()})
        if job.touch:
            out['touch rows per step'] = np.asarray(job.touch_rows_per_step(), dtype=np.float64)
        out = {name: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).copy() for name, a in out.items()}
        job.close()
        return out

    def check_mode(self, job):
        want = self.job_kw.get('touch', False)
        mode = 0 if not want else 3 if want == 'index' else 2 if self.job_kw.get('final_only') else 1
        assert job.touch_mode == mode, (self.name, job.touch_mode, mode)
        assert all(1 <= job.steps_per_epoch(s) for s in range(self.S))

    def check_reference(self, got):
        """The 0x00 run against the C oracle's dense optimizer, at the bar of tests/test_gpu_touch.py."""
        parts, inits, perms = self.inputs()
        for s, p in enumerate(parts):
            st = O.MFState(inits[s][0].numpy().copy(), inits[s][1].numpy().copy())
            losses = [O.train_epoch(st, p, perms[s][t].numpy(), self.B, 1e-3, 0.1, 0.9)[0] for t in range(self.E)]
            assert np.isfinite(st.U).all() and np.isfinite(st.V).all()
            ru, rv = rel(got[f'U{s}'], st.U), rel(got[f'V{s}'], st.V)
            print(f'{self.name} shard {s}: rel U {ru:.3g} V {rv:.3g}')
            assert ru < 2e-5 and rv < 2e-5, (self.name, s, ru, rv)
            np.testing.assert_allclose(np.sqrt(got[f'sse{s}'] / len(p[0])), losses, rtol=2e-5)


class AdamCase(MfCase):
    """D2: a case of tests/adam_cases.py, whose reference (the float64 contract, torch's float32 run as the yardstick) and bound
    are those of tests/test_gpu_adam.py: 70 x 50 at d = 32, 2,000 ratings, 4 steps per epoch, 3 epochs, a quarter of the ratings on one
    item (several work units beside rows of one).  Not the toy set: that reference leaves out the elements whose gradient falls below
    1e-3 and allows 1 % of them, and of the toy set's it leaves out 4.3 % (measured on the CPU: the many items without a rating)."""

    def __init__(self, name):
        super().__init__(name, k=32, B=512, E=3)
        self.n_user, self.n_item = 70, 50

    def inputs(self):
        return None

    def _case(self):
        return adam_cases.WHOLE_STEP_CASES[1]

    def make(self):
        job = self._case().job(lazy_rows=False)
        assert job.optimizer == 'adam' and not job.lazy_rows
        return job

    def check_reference(self, got):
        ref = adam_cases.reference(self._case())
        E_k = adam_cases.distance(ref, got['U0'], got['V0'], got['sse0'])
        wmax = max(np.abs(ref['f64'][0]).max(), np.abs(ref['f64'][1]).max())
        bound = 4 * max(ref['E_t'], adam_cases.ulp32(wmax))
        print(f'{self.name}: E_k {E_k:.3g} E_t {ref["E_t"]:.3g} bound {bound:.3g} left out {ref["left_out"]:.4%}')
        assert ref['left_out'] <= adam_cases.LEAVE_OUT_CAP
        assert E_k <= bound, (E_k, ref['E_t'], bound)


class GcnCase:
    """G1: 40 x 30 at d = 8, one layer: 3 users and 4 items without a rating, a quarter of the 500 ratings on one item (a row of 125
    entries: longer than any lane group's stride of at most 64)."""
    name, env, patch = 'G1', {}, {}

    def __init__(self):
        self.case = lightgcn_cases.WHOLE_STEP_CASES[0]

    def prepare(self, m):
        pass

    def run(self):
        c = self.case
        assert c.no_u > 0 and c.no_i > 0 and np.bincount(c.iid).max() > 64
        job = c.job()
        job.run()
        names = ('padded U', 'padded V', 'padded P', 'padded Q', 'M')
        out = dict(zip(names, (*job.padded_tables(0), *job.base_tables(padded=True), job._t['M'])))
        out.update(zip(('U', 'V', 'P', 'Q'), (*job.tables(0), *job.base_tables())))
        out = {name: t.contiguous().cpu().numpy().copy() for name, t in out.items()}
        out['sse'] = job.epoch_sse(0).copy()
        job.close()
        return out

    def check_reference(self, got):
        ref = self.case.train_ref(dtype=np.float32)
        for name in ('U', 'V', 'P', 'Q'):
            assert got[name].shape == ref[name][-1].shape and got[name].tobytes() == ref[name][-1].tobytes(), name
        assert got['sse'].tobytes() == ref['sse'].tobytes()


I4_PATCH = lambda heavy, split: {'INDEX_HEAVY_SLOTS': heavy, 'INDEX_SPLIT_SLOTS': split}
CASES = {c.name: c for c in (
    MfCase('W1', B=437, env={'URE_TOUCH_INDEX': '0'}, touch=True),
    MfCase('W2', B=3000, env={'URE_TOUCH_INDEX': '1'}, touch=True, final_only=True),
    MfCase('W3', S=3, k=32, B=700, touch=True),
    MfCase('I1', S=3, B=700, touch='index'),
    MfCase('I2-staged', B=437, env={'URE_INDEX_STAGED': '1'}, touch='index'),
    MfCase('I2-direct', B=437, env={'URE_INDEX_STAGED': '0'}, touch='index'),
    MfCase('I3', n_rows=27714, B=37, seed=11, touch='index'),
    MfCase('I4-600-16-8', B=600, scale=0.3, seed=21, heavy=True, patch=I4_PATCH(16, 8), touch='index', snapshots='compact'),
    MfCase('I4-2900-1-1', B=2900, scale=0.3, seed=21, heavy=True, patch=I4_PATCH(1, 1), touch='index', snapshots='compact'),
    MfCase('I5', k=128, B=219, scale=0.3, seed=11, touch='index'),
    MfCase('D1', S=3, B=3000, touch=False, snapshots='compact'),
    AdamCase('D2'),
    GcnCase(),
)}
STEPS = {'W1': 65, 'W2': 10, 'I2-staged': 65, 'I2-direct': 65, 'I3': 750, 'I5': 130}        # what the shapes are chosen for

_RUNS = {}           # (case name, fill) -> the arrays of that run; the 0x00 run of a case is what the others are compared with


def run_case(case, fill, monkeypatch):
    if (case.name, fill) not in _RUNS:
        if isinstance(case, MfCase):
            case.inputs()                        # (host inputs: made once, outside the poison)
        with poison.active(monkeypatch, fill):
            with monkeypatch.context() as m:
                case.prepare(m)
                _RUNS[(case.name, fill)] = case.run()
    return _RUNS[(case.name, fill)]


def differences(a, b):
    """Array by array: -> [finding] (empty: equal bytes)."""
    found = [f'arrays differ: {sorted(set(a) ^ set(b))}'] if set(a) != set(b) else []
    for name in sorted(set(a) & set(b)):
        x, y = a[name], b[name]
        if x.shape != y.shape or x.dtype != y.dtype:
            found.append(f'{name}: {x.dtype}{x.shape} against {y.dtype}{y.shape}')
        elif x.tobytes() != y.tobytes():
            bad = np.flatnonzero(np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8))
            found.append(f'{name}: {bad.size} byte(s) differ, the first at byte {int(bad[0])} of {x.nbytes}')
    return found


@pytest.mark.parametrize('fill', FILLS, ids=FILL_IDS)
@pytest.mark.parametrize('name', list(CASES))
def test_a_job_gives_the_same_bytes_on_memory_of_every_fill(name, fill, monkeypatch):
    case = CASES[name]
    got = run_case(case, fill, monkeypatch)
    if isinstance(case, MfCase) and name in STEPS:
        assert -(-len(case.inputs()[0][0][0]) // case.B) == STEPS[name]
    if fill == 0x00:
        assert all(a.size for a in got.values()), [n for n, a in got.items() if not a.size]
        case.check_reference(got)
        return
    found = differences(run_case(case, 0x00, monkeypatch), got)
    assert not found, f'{name}: fill 0x00 against {FILL_IDS[FILLS.index(fill)]}:\n  ' + '\n  '.join(found)


# ---------------------------------------------------------------- a request
@pytest.mark.parametrize('fill', FILLS, ids=FILL_IDS)
@pytest.mark.parametrize('forced', ['default', 'touch'])
def test_a_request_gives_the_same_bytes_on_memory_of_every_fill(forced, fill, tmp_path, monkeypatch):
    """Sisa.learn and two Sisa.unlearn calls of three shards side by side (tests/test_gpu_surface.py, within the goldens it checks
    already): the tags block and the shuffle scratch of rng.device_tags, the EvalSet lane buffers across calls with different model
    counts and the merge all come from torch.empty.  The merged user matrix, every item matrix, log0 and the per-epoch series are
    the same bytes under every fill and without one; once with the kernel the request picks by itself, once forced into touch mode
    as tests/test_gpu_surface_touch.py forces it."""
    from test_gpu_surface import check_sisa_against_reference
    from ultrare_amd import engine
    key = ('request ' + forced, fill)
    if forced == 'touch':
        monkeypatch.setenv('URE_TOUCH', '1')
        monkeypatch.setenv('URE_TOUCH_AHEAD', '1')
    seen = []
    init = engine.TrainJob.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        seen.append(self.touch_mode)
    monkeypatch.setattr(engine.TrainJob, '__init__', spy)
    with poison.active(monkeypatch, fill):
        _RUNS[key] = {n: np.frombuffer(b, np.uint8) for n, b in check_sisa_against_reference(3, 2, True, tmp_path).items()}
    assert seen and all((m > 0) == (forced == 'touch') for m in seen), seen
    if fill == 0x00:
        return
    if (key[0], 0x00) not in _RUNS:
        first = tmp_path / 'first'
        first.mkdir()
        with poison.active(monkeypatch, 0x00):
            _RUNS[(key[0], 0x00)] = {n: np.frombuffer(b, np.uint8) for n, b in check_sisa_against_reference(3, 2, True, first).items()}
    found = differences(_RUNS[(key[0], 0x00)], _RUNS[key])
    assert not found, f'request ({forced}): fill 0x00 against {FILL_IDS[FILLS.index(fill)]}:\n  ' + '\n  '.join(found)


# ---------------------------------------------------------------- another job's leavings
def test_a_job_gives_the_same_bytes_on_blocks_another_job_left(monkeypatch):
    """The production path, the helper off: the blocks of a closed job go to the next one with what it left in them, and the
    predecessor is not the job itself (the twin jobs of test_touch_memory_from_the_block_cache_is_filled_again find their own,
    correct, leavings).  I4 (2900, 1, 1) is trained and closed, then I5, whose index block is the next size up from I2's (the cache
    hands out the smallest idle block that is large enough); an untrained I2 job holds whatever idle block has I2's own size
    meanwhile.  Then I2 trains and must give the bytes it gave on filled memory."""
    want = run_case(CASES['I2-staged'], 0x00, monkeypatch)
    with poison.active(monkeypatch, None):
        with monkeypatch.context() as m:
            CASES['I2-staged'].prepare(m)
            decoy = CASES['I2-staged'].make()
        for name in ('I4-2900-1-1', 'I5'):
            with monkeypatch.context() as m:
                CASES[name].prepare(m)
                CASES[name].run()
        with monkeypatch.context() as m:
            CASES['I2-staged'].prepare(m)
            got = CASES['I2-staged'].run()
        decoy.close()
    found = differences(want, got)
    assert not found, 'I2 after I4 and I5:\n  ' + '\n  '.join(found)


# ---------------------------------------------------------------- the hook itself
def test_the_block_fill_fills_and_a_typo_is_an_error(monkeypatch):
    """URE_BLOCK_FILL: a job's index block starts as the byte -- step_begin is written by the first epoch start (idx_scan2_kernel),
    not by ure_job_create --, anything but a byte is refused by name, unset trains; and the arrays whose length is a device word
    (items, sslot) are not readable before the first epoch start has been enqueued."""
    from ultrare_amd import _native as nv
    case = CASES['I2-staged']
    for text, word in (('0x5A', 0x5A5A5A5A), ('90', 0x5A5A5A5A), ('0x00', 0), ('0', 0), ('255', 0xFFFFFFFF)):
        with monkeypatch.context() as m:
            case.prepare(m)
            m.setenv('URE_BLOCK_FILL', text)
            job = case.make()
            sb = job.index_array(0, 'step_begin')
            assert sb.dtype == np.uint32 and sb.size == job.steps_per_epoch(0) + 1 and (sb == word).all(), (text, sb[:4])
            for name in ('items', 'sslot'):
                with pytest.raises(nv.NativeError, match='first epoch start'):
                    job.index_array(0, name)
            assert job.index_array(0, 'W').size and job.index_array(0, 'heavy_cnt').size == job.steps_per_epoch(0)
            job.run(1)
            assert job.index_array(0, 'items').size and job.index_array(0, 'sslot').size
            job.close()
    for text in ('banana', '256', '-1', '0x5A5A', '5A', '1 2'):
        with monkeypatch.context() as m:
            case.prepare(m)
            m.setenv('URE_BLOCK_FILL', text)
            with pytest.raises(nv.NativeError, match='URE_BLOCK_FILL'):
                case.make()
    for text in (None, ''):
        with monkeypatch.context() as m:
            case.prepare(m)
            m.delenv('URE_BLOCK_FILL', raising=False) if text is None else m.setenv('URE_BLOCK_FILL', text)
            got = case.run()
        assert not differences(run_case(case, 0x00, monkeypatch), got)
