"""Host side of the MI355X engine: HBM layout of a shard, training jobs, evaluation.

This file holds no arithmetic of the hot path -- that lives in csrc/*.hip behind
include/ultrare_hip.h -- only layout building (numpy, once per shard), device memory
(torch tensors) and launches.

HBM layout of one shard:
  slot arrays  ent_oid[n_slots] i32 | ent_r[n_slots] f32 | ent_tag[2][n_slots] u16 -- one 8-aligned,
               padded segment per destination row (users and items), in schedule order
  ent_src[n_slots] i32     slot -> file-order index of its interaction (-1 in padding)
  file_tag[N] u16          scratch: batch of interaction j in the epoch being prepared
  sched[n_user+n_item][4] i32   {row id, first slot, end slot, nnz}, heaviest row first
  units[n_units][4] i32    work units of the step kernel for one table width (ShardData.units(d))
  U[2][n_user][d] V[2][n_item][d] f32 ping-pong weights ; mU, mV momentum (Adam: first moment; vU, vV second moment)
  perm[epochs][N] i32 ; lr[epochs] f32 ; sse[epochs][n_user] f32 (per-user squared error)
"""
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from . import _native as nv

SCORE_PARTIALS = 2048     # URE_SCORE_PARTIALS of the C ABI
SERIES_SCRATCH_BYTES = 256 << 20     # prediction scratch of one ure_eval_series call
LAZY_ROWS = os.environ.get('URE_LAZY_ROWS', '1') != '0'
TOUCH_MAX_STEPS = 32000              # kTouchMaxSteps of csrc/mf_touch.h (epochs longer than 64 steps run in windows of 64)
# touch mode, epochs of several windows: rows of up to this many scan passes are one work item.  Full MF at the 25 M shape, us per
# launch: 106.7 at 1 (a unit per pass), 95.5 at 2, 97.0 at 4, 118.8 at 8, 157.3 at 16, 386.7 at 64 -- a lane group walks its row's
# passes one after the other (a scan, a compaction and a gather each), units work theirs side by side
TOUCH_ROW_PASSES = 2
# ... and the work units of the longer rows take this many passes each (a unit skips the passes without a slot of the step by their masks;
# fewer, larger units: the step visits 1,700 workgroups of them instead of 13,600).  The same leg: 105.8 us at 1, 81.7 at 2, 68.0 at 4,
# 62.9 at 8, 61.6 at 16
TOUCH_UNIT_PASSES = 8
TOUCH_AHEAD_MAX_STEPS = 63           # kAheadMaxSteps of csrc/mf_touch.h
INDEX_MAX_STEPS = 1008               # kIdxMaxSteps of csrc/mf_index.h (touch_mode 3: the epoch's slots sorted by step)
INDEX_HEAVY_SLOTS = 16               # touch_mode 3: rows with at least this many slots per step on average get a workgroup per step ...
INDEX_SPLIT_SLOTS = 384              # ... and with this many, one per 256 slots of the step
INDEX_HEAVY_MAX = 256                # kIdxHeavyMax
INDEX_SHORT_EPOCH_MAX_D = 64         # auto rule: epochs of at most 63 steps take touch_mode 3 up to this table width (beyond it touch_mode 2 / 1)
TOUCH_MIN_TABLE_BYTES = 256 << 20    # auto rule: the job's live rows (w, m, second buffer) exceed the Infinity Cache


# Host timeline of a call (URE_HOST_TRACE=1): (label, seconds) marks that tools/profile_e2e.py prints; off by default.
HOST_TRACE = [] if os.environ.get('URE_HOST_TRACE', '0') == '1' else None


def mark(label):
    if HOST_TRACE is not None:
        import time
        HOST_TRACE.append((label, time.perf_counter()))


def to_device_async(arr, dev):
    """A small host array -> device tensor without stalling the host: through a pooled pinned buffer and an asynchronous
    copy (from pageable memory `.to(device)` waits until the stream has reached and finished the copy)."""
    from . import rng
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if torch.device(dev).type != 'cuda' or t.numel() == 0:
        return t.to(dev)
    stage = rng.SMALL.take(tuple(t.shape), t.dtype)
    stage.numpy()[...] = t.numpy()                       # (a plain memcpy: torch's copy_ would go through its intra-op thread pool)
    out = stage.to(dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    rng.SMALL.give(stage, ev)
    return out


def upload_many(arrays, dev):
    """Several small host arrays -> device tensors through ONE pinned staging buffer and ONE asynchronous copy (each array
    starts on a 64-byte boundary of one device allocation).  A request of 16 shards sends ~50 such descriptors (work units,
    row lists, schedules of scalars): one by one they cost 0.1-0.2 ms of host time each."""
    from . import rng
    arrays = [np.ascontiguousarray(a) for a in arrays]
    if torch.device(dev).type != 'cuda':
        return [torch.from_numpy(a.copy()).to(dev) for a in arrays]
    offs, at = [], 0
    for a in arrays:
        offs.append(at)
        at += (a.nbytes + 63) // 64 * 64
    if at == 0:
        return [torch.from_numpy(a.copy()).to(dev) for a in arrays]
    stage = rng.SMALL.take((at,), torch.uint8)
    host = stage.numpy()
    for a, o in zip(arrays, offs):
        host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    blob = stage.to(dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    rng.SMALL.give(stage, ev)
    out = []
    for a, o in zip(arrays, offs):
        out.append(blob[o:o + a.nbytes].view(torch.from_numpy(np.empty(0, dtype=a.dtype)).dtype).view(a.shape))
    return out


def pad_dim(d):
    """Table width used on the device: next power of two >= max(d, 4).  Padding
    columns are zero at init; their gradient and decay keep them exactly zero."""
    p = 4
    while p < d:
        p *= 2
    if p > 256:
        raise ValueError(f'embedding width {d} > 256 is not supported by the gfx950 kernels')
    return p


def _device():
    if not torch.cuda.is_available():
        raise nv.NativeError('no HIP device visible: the SISA hot path has no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def build_shards(triples, n_user, n_item, device=None, keep_positions=False, units_for=None):
    """The HBM layouts of the shards of one call: triples = [(uid, iid, rating)] -> [ShardData].
    ONE native call builds every layout, side by side on host threads, packed into one pinned staging buffer (pooled); all of them go up
    in ONE asynchronous copy into one device allocation, and the engine-side scratch of all shards (batch tags, inverse-permutation
    stages) comes from two fills.  units_for = a table width k: the work units of that width are built by the same native call and
    travel in the same copy (ShardData.units finds them).  From pageable numpy arrays, shard after shard, the same 22 MB of a 5-shard
    ml-1m call took 9-10 ms of a 20 ms Sisa.learn (profiles/r03/NOTES.md)."""
    return LayoutPlan(triples, n_user, n_item, device, units_for).build(keep_positions)


class LayoutPlan:
    """build_shards in pieces that a request overlaps: __init__ checks the triples and takes the host staging buffer; allocate() (on
    the request's own thread and stream) makes every device allocation and fill from UPPER BOUNDS of the slot counts -- nothing in it
    waits for the layouts --; build() (any thread: a worker of the request, started BEFORE allocate()) runs the native builder, waits
    for allocate(), queues the one copy and returns the ShardData, which hold ADDRESSES; the tensor views of a layout's arrays are
    made when somebody asks for them."""

    def __init__(self, triples, n_user, n_item, device=None, units_for=None):
        from . import rng
        self.n_user, self.n_item = int(n_user), int(n_item)
        self.dev = dev = device or _device()
        self.on_gpu = torch.device(dev).type == 'cuda'
        cols = []
        for uid, iid, rating in triples:
            uid, iid, rating = np.asarray(uid), np.asarray(iid), np.asarray(rating)
            n = len(uid)
            if n == 0:
                raise ValueError('a shard needs at least one interaction')
            if not (len(iid) == n and len(rating) == n):
                raise ValueError('uid / iid / rating lengths differ')
            # (ids outside [0, n_user) x [0, n_item) are refused by the native builder, which walks the arrays anyway)
            cols.append((uid, iid, rating))
        self.cols = cols
        al = lambda x: (x + 7) // 8 * 8                              # every array starts on a 32-byte boundary
        self.d_units = pad_dim(int(units_for)) if units_for else 0
        self.words = [al(nv.layout_region_words(len(c[0]), self.n_user, self.n_item) +
                         (nv.units_capacity_words(len(c[0]), self.n_user, self.n_item, self.d_units) if self.d_units else 0)) for c in cols]
        self.off = np.concatenate([[0], np.cumsum(self.words)]).astype(np.int64)
        self.stage = rng.STAGING.take((int(self.off[-1]),), torch.int32)
        # the native builder starts HERE, on a thread of the library's own (a Python worker took 0.3-0.4 ms to get going while the calling
        # thread held the interpreter); build() joins it
        # ... and sends every shard's layout to the device as soon as it is built (the blob is allocated here for that; as ONE copy behind the
        # last shard, the 1.1 GB of a 32-shard request at the 25 M shape stood between the build and the job for 28 ms)
        self._async = None
        self.blob = None
        self._uploaded = False
        self._stream = None
        if self.d_units:
            host = self.stage.numpy()
            try:
                dev_regions, dev_id, stream = None, -1, None
                if self.on_gpu:
                    with torch.cuda.device(dev):
                        self.blob = torch.empty(int(self.off[-1]), dtype=torch.int32, device=dev)
                        stream = torch.cuda.current_stream(dev)
                    dev_regions = [self.blob.data_ptr() + 4 * int(self.off[s]) for s in range(len(cols))]
                    dev_id = self.blob.device.index
                    self._uploaded, self._stream = True, stream
                mark('layouts native start')
                self._async = nv.build_layouts_start(cols, self.n_user, self.n_item, [host[self.off[s]:self.off[s + 1]] for s in range(len(cols))],
                                                     threads=min(len(cols), rng.host_cpus()), units_d=self.d_units, dev_regions=dev_regions, device=dev_id,
                                                     stream=stream)
            except BaseException:
                rng.STAGING.give(self.stage, None)
                raise
        self._owner = __import__('threading').current_thread()
        self._allocated = __import__('threading').Event()
        self._alloc_error = None

    def allocate(self):
        from . import rng
        cols, dev, al = self.cols, self.dev, (lambda x: (x + 7) // 8 * 8)
        try:
            if self.blob is None:
                self.blob = torch.empty(int(self.off[-1]), dtype=torch.int32, device=dev)
            # engine-side scratch: batch tags (0xFFFF matches no batch; three buffers: touch_mode 2 prepares two epochs ahead) and
            # the stages of the inverse permutation.  Sized for the most slots a shard of n interactions can have.
            self.t_words = [(al(3 * nv.layout_capacity(len(c[0]), self.n_user, self.n_item)), al(len(c[0]))) for c in cols]
            self.z_words = [(al(len(c[0])), al(max(((len(c[0]) + 2047) // 2048) * ((len(c[0]) + 2047) // 2048 + 1), 1) if (len(c[0]) + 2047) // 2048 <= 1024 else 1))
                            for c in cols]
            self.tags = torch.full((sum(a + b for a, b in self.t_words),), -1, dtype=torch.int16, device=dev)
            self.zeros = torch.zeros(sum(a + b for a, b in self.z_words), dtype=torch.int32, device=dev)
            self.allocated = None
            if self.on_gpu:
                self.allocated = torch.cuda.Event()
                self.allocated.record(torch.cuda.current_stream(dev))
        except BaseException as e:
            self._alloc_error = e
            raise
        finally:
            self._allocated.set()
        return self

    def build(self, keep_positions=False):
        from . import rng
        if not self._allocated.is_set() and __import__('threading').current_thread() is self._owner:
            self.allocate()                         # (one thread does everything: build_shards)
        S, cols, off, host = len(self.cols), self.cols, self.off, self.stage.numpy()
        n_user, n_item, dev, d_units = self.n_user, self.n_item, self.dev, self.d_units
        rows = n_user + n_item
        handed_back = False
        try:
            try:
                if self._async is not None:
                    built = self._async.result()
                    self._async = None
                else:
                    mark('w: layouts native start')
                    built = nv.build_layouts(cols, n_user, n_item, [host[off[s]:off[s + 1]] for s in range(S)], threads=min(S, rng.host_cpus()), units_d=d_units)
            except nv.NativeError as e:
                if getattr(e, 'code', None) == -2:             # (-3: a shard beyond 2^31 slots -- reported as it is)
                    raise ValueError(f'user or item id outside [0, n_user) x [0, n_item): {e}') from None
                raise
            mark('w: layouts built (native)')
            if not self._allocated.wait(60.0):
                raise RuntimeError('LayoutPlan.build() on a worker: nobody called allocate()')
            if self._alloc_error is not None:
                raise RuntimeError('the device allocations of the layouts failed') from self._alloc_error
            n_slots, n_active = built[0], built[1]
            n_units = built[2] if d_units else [-1] * S
            al = lambda x: (x + 7) // 8 * 8
            units_at = [al(3 * int(k) + 5 * rows) for k in n_slots]                       # where a shard's units start inside its region (when built)
            used = [a + (al(4 * int(u)) if u > 0 else 0) for a, u in zip(units_at, n_units)]
            end = int(off[S - 1]) + used[S - 1]
            pinned = self.stage.is_pinned() and self.on_gpu
            ready = None
            with (torch.cuda.device(dev) if self.on_gpu else contextlib.nullcontext()):
                if self.on_gpu:
                    # (the allocations and fills were queued on the planner's stream, which need not be this thread's)
                    torch.cuda.current_stream(dev).wait_event(self.allocated)
                if not self._uploaded:
                    self.blob[:end].copy_(self.stage[:end], non_blocking=pinned)      # ONE copy (the slack between the regions travels along)
                if self.on_gpu:
                    # whoever trains on a layout from another stream waits for this event first: TrainJob does
                    ready = torch.cuda.Event()
                    ready.record(self._stream if self._uploaded else torch.cuda.current_stream(dev))     # (the stream the copies went to)
            mark('w: layouts copy queued')
            out, t_at, z_at = [], 0, 0
            for s, (uid, iid, rating) in enumerate(cols):
                sh = object.__new__(ShardData)
                n, k = len(uid), int(n_slots[s])
                sh.N, sh.n_user, sh.n_item, sh.device = n, n_user, n_item, dev
                sh.n_slots, sh.n_active = k, int(n_active[s])
                o = int(off[s])
                ta, tb = self.t_words[s]
                za, zb = self.z_words[s]
                f32, i32, i16 = torch.float32, torch.int32, torch.int16
                # name -> (tensor it lives in, first element, elements, dtype, shape)
                sh._where = {'ent_oid': (self.blob, o, k, i32, None), 'ent_r': (self.blob, o + k, k, f32, None), 'ent_src': (self.blob, o + 2 * k, k, i32, None),
                             'sched': (self.blob, o + 3 * k, 4 * rows, i32, (rows, 4)), '_row_slot': (self.blob, o + 3 * k + 4 * rows, rows, i32, None),
                             'ent_tag': (self.tags, t_at, 3 * k, i16, (3, k)), 'file_tag': (self.tags, t_at + ta, n, i16, None),
                             'inv_stage': (self.zeros, z_at, n, i32, None), 'inv_off': (self.zeros, z_at + za, zb, i32, None)}
                t_at += ta + tb
                z_at += za + zb
                sh._blob = self.blob
                # (the schedule's head stays on the host -- what a job reads of it --; the whole of it, 3.5 MB per shard at the 25 M shape and 6 ms of
                # copying for a 32-shard request, comes back from the device when somebody asks: units of another table width)
                sh._sched_head = host[o + 3 * k:o + 3 * k + 4 * min(rows, INDEX_HEAVY_MAX)].reshape(-1, 4).copy()
                sh.max_row = int(sh._sched_head[0, 3])
                sh.u_pos = sh.i_pos = None
                if keep_positions:                                        # host copies of every interaction's two slots (tests, tools)
                    lay = nv.build_layout(np.ascontiguousarray(uid, dtype=np.int32), np.ascontiguousarray(iid, dtype=np.int32),
                                          np.ascontiguousarray(rating, dtype=np.float32), n_user, n_item, want_pos=True)
                    sh.u_pos, sh.i_pos = lay['u_pos'], lay['i_pos']
                sh._units = {}
                if n_units[s] > 0:
                    ua = o + units_at[s]
                    sh._units[(d_units, False)] = (self.blob[ua:ua + 4 * int(n_units[s])].view(int(n_units[s]), 4), int(n_units[s]), sh.n_active)
                sh.ready = ready
                out.append(sh)
            rng.STAGING.give(self.stage, ready if pinned else None)
            handed_back = True
        finally:
            if not handed_back:
                rng.STAGING.give(self.stage, None)                  # whatever went wrong, the pooled staging buffer goes back
        with ShardData._count_lock:
            ShardData.built += S
        return out


class ShardData:
    """One shard's interactions laid out for the step kernel: every destination row
    (users, then items) owns an 8-aligned, padded segment of one slot array; segments
    follow the row schedule (heaviest first).  Built by build_shards()."""

    def __init__(self, uid, iid, rating, n_user, n_item, device=None, keep_positions=False):
        self.__dict__.update(build_shards([(uid, iid, rating)], n_user, n_item, device, keep_positions)[0].__dict__)

    _count_lock = __import__('threading').Lock()
    built = 0            # layouts built (and uploaded) by this process: lets a measurement show that its timed call paid for them

    def ptr(self, name):
        """Device address of one of the layout's arrays (no tensor is made for it)."""
        base, first, _, dtype, _ = self._where[name]
        return base.data_ptr() + first * base.element_size()

    def __getattr__(self, name):
        # the layout's arrays as tensors (ent_oid, ent_r, ent_src, sched, ent_tag, file_tag, inv_stage, inv_off, _row_slot): views made on first use
        where = self.__dict__.get('_where')
        if name == '_sched_host' and where is not None:
            got = self.sched.cpu().numpy()                   # (synchronises; rare)
            self.__dict__[name] = got
            return got
        if where is None or name not in where:
            raise AttributeError(name)
        base, first, count, dtype, shape = where[name]
        t = base[first:first + count]
        if dtype != base.dtype:
            t = t.view(dtype)
        if shape is not None:
            t = t.view(*shape)
        self.__dict__[name] = t
        return t

    def row_slot(self):
        """Device int32 [n_user + n_item]: a row's index in the schedule when it is one of the n_active rows with
        interactions in this shard (the rows a compact snapshot stores), -1 otherwise."""
        return self._row_slot

    def units(self, d, touch=False, min_passes=1, unit_passes=1):
        """The work units of the step kernel for table width d (device int32 [n_units, 4]).  touch: only the rows
        longer than one scan pass get units (-> (units, n_multi)); the others are worked off per step from a
        compaction of the rows that are trained in it (csrc/mf_touch.h)."""
        key = (d, bool(touch)) if min_passes == 1 and unit_passes == 1 else (d, bool(touch), int(min_passes), int(unit_passes))
        if key not in self._units:
            u, n_units, n_rows = self.units_host(d, touch, min_passes, unit_passes)
            self._units[key] = (to_device_async(u, self.device), n_units, n_rows)
        dev_u, n_units, n_rows = self._units[key]
        return (dev_u, n_units, n_rows) if touch else dev_u

    def units_host(self, d, touch=False, min_passes=1, unit_passes=1):
        """The host half of units(): -> (int32 [max(n_units, 1), 4] array to upload, n_units, rows covered).  touch: only the
        rows of more than min_passes scan passes get units (the others are worked off per row); unit_passes = scan passes per unit."""
        n_rows = self.n_active
        if touch:
            lanes = d // 4 if d <= 32 else d // 8
            seg = self._sched_host[:self.n_active, 2] - self._sched_host[:self.n_active, 1]
            n_rows = int(np.count_nonzero(seg > 8 * lanes * min_passes))
            assert n_rows == 0 or (seg[:n_rows] > 8 * lanes * min_passes).all()          # the schedule is heaviest first
        u = nv.build_units(self._sched_host, n_rows, d, unit_passes)
        return (u if len(u) else np.full((1, 4), -1, np.int32)), len(u), n_rows

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in
                   (self.ent_oid, self.ent_r, self.ent_tag, self.ent_src, self.file_tag, self.sched))


_CLOSED_FORM = {}


def closed_form_scalars(lr_host, steps, lam, mu):
    """a_e with w = a_e * w0 after epoch e for a row that only decays: the optimizer's recurrence
    g = lam*w; m = mu*m + g (m = g on the first step); w -= lr*m, in float64 (as ure_job_materialize)."""
    key = (np.asarray(lr_host, dtype=np.float32).tobytes(), int(steps), float(lam), float(mu))
    if key not in _CLOSED_FORM:
        if len(_CLOSED_FORM) > 256:
            _CLOSED_FORM.clear()
        _CLOSED_FORM[key] = _closed_form_scalars(lr_host, steps, lam, mu)
    return _CLOSED_FORM[key].copy()


def _closed_form_scalars(lr_host, steps, lam, mu):
    a, b, out, t = 1.0, 0.0, [], 0
    for e in range(len(lr_host)):
        lr = float(lr_host[e])
        for _ in range(steps):
            b = lam * a if t == 0 else mu * b + lam * a
            a -= lr * b
            t += 1
        out.append(a)
    return np.asarray(out, dtype=np.float32)


def touch_plan(steps_max, d, batch, live_bytes, lazy_rows, snapshots, touch, final_only, epoch_reads, env=None):
    """The step kernel of a job: -> touch_mode 0 (the default kernel), 1, 2 or 3.  steps_max = optimizer steps per epoch of the job's
    longest shard, d = the padded table width, live_bytes = the job's live rows (w, m, second buffer), snapshots / touch /
    final_only / epoch_reads = TrainJob's arguments as given; env = the environment switches (None: os.environ, read now)."""
    env = os.environ if env is None else env
    use_index = env.get('URE_TOUCH_INDEX', '1')
    # touch mode (csrc/mf_touch.h): a step visits only the rows it trains, the others are advanced in closed form when
    # they are next trained.  Pays when the tables do not fit the caches (configs[3]); URE_TOUCH=0/1 overrides the rule.
    by_rule = False
    if touch is None:
        use_touch = env.get('URE_TOUCH', 'auto')
        by_rule = use_touch == 'auto' and live_bytes > TOUCH_MIN_TABLE_BYTES and bool(final_only or epoch_reads)
        touch = (use_touch == '1') or by_rule
    if not (bool(touch) and lazy_rows and steps_max <= TOUCH_MAX_STEPS):
        return 0
    # touch_mode 2 (csrc/mf_touch.h, "masks one epoch ahead"): no dense pass at the epoch starts; for callers that read the tables
    # only after the last epoch (final_only) and epochs of at most 63 steps.  URE_TOUCH_AHEAD=0 keeps mode 1.
    # Short epochs (<= 63 steps) of NARROW rows: sorting the epoch's slots by step (touch_mode 3) costs ~3 ms per epoch whatever the row width, and saves the
    # scan of every trained row's slots in every step -- most of the traffic at 64-byte rows.  BASELINE.json configs[3]'s shape (32 shards, 27 steps per
    # epoch), epoch time in touch_mode 2 -> 3: d = 16 6.32 -> 4.95 ms, d = 32 6.25 -> 5.87, d = 64 8.36 -> 8.02, d = 128 12.18 -> 13.17
    # (profiles/r04/exp_short_epochs_index.txt).  Under the auto rule touch_mode 3 is taken up to d = 64.
    force_index = touch == 'index' or use_index == '2' or (by_rule and d <= INDEX_SHORT_EPOCH_MAX_D and use_index != '0')
    if final_only and steps_max <= TOUCH_AHEAD_MAX_STEPS and snapshots in (False, None, 'compact') and env.get('URE_TOUCH_AHEAD', '1') != '0' and not force_index:
        return 2
    # touch_mode 3 (csrc/mf_index.h): epochs of more than 63 steps -- the epoch's slots are sorted by step at its start and a step
    # launches over exactly the rows it trains (64-step windows look at every work unit in every step).  URE_TOUCH_INDEX=0 keeps windows.
    if steps_max <= INDEX_MAX_STEPS and batch <= 200000 and (force_index or (steps_max > TOUCH_AHEAD_MAX_STEPS and use_index != '0')):
        return 3
    return 1


def shard_regions(n_user, n_item, n_active, d, epochs, lazy_rows, snapshots, at=0, snap_at=0, *, adam=False):
    """Where one shard's tables live in a job's two device pools: -> (pool, snap, end, snap_end), pool and snap dicts name -> (first float,
    floats, view shape); the shard starts at `at` / `snap_at` (multiples of 64), the next one at end / snap_end.  The float pool: U and V
    (both buffers), mU, mV, sse and -- lazy_rows -- the start tables U0, V0, each rounded up to 64 floats.  The snapshot pool: snapU and
    straight after it snapV ('full') or snap ('compact': the n_active rows), the shard's snapshots as a whole rounded up to 64 floats.
    adam: the second moments vU, vV follow V0 (no other region moves)."""
    al = lambda x: (x + 63) // 64 * 64
    pool, snap, E = {}, {}, epochs
    for name, shape in (('U', (2, n_user, d)), ('V', (2, n_item, d)), ('mU', (n_user, d)), ('mV', (n_item, d)), ('sse', (E, n_user)),
                        ('U0', (n_user if lazy_rows else 0, d)), ('V0', (n_item if lazy_rows else 0, d))) + \
                       ((('vU', (n_user, d)), ('vV', (n_item, d))) if adam else ()):
        pool[name] = (at, math.prod(shape), shape)
        at += al(math.prod(shape))
    for name, shape in {'full': (('snapU', (E, n_user, d)), ('snapV', (E, n_item, d))), 'compact': (('snap', (E, n_active, d)),)}.get(snapshots, ()):
        snap[name] = (snap_at, math.prod(shape), shape)
        snap_at += math.prod(shape)
    return pool, snap, at, al(snap_at)


class _States:
    """TrainJob.state: per shard the views of the job's device memory ({'U', 'V', 'mU', 'mV', 'perm', 'sse', 'snap' ...}), made when first asked for."""

    def __init__(self, n, make):
        import weakref
        # (a weak reference to the job's method: job -> state -> job would be a cycle, and a job's 0.7 GB of device memory -- 660 MB per
        # request measured -- would wait for the cyclic collector instead of going back when the last reference to the job does)
        self._n, self._make, self._got = n, weakref.WeakMethod(make), {}

    def __len__(self):
        return self._n

    def __getitem__(self, s):
        s = s + self._n if s < 0 else s
        if not 0 <= s < self._n:
            raise IndexError(s)
        if s not in self._got:
            make = self._make()
            if make is None:
                raise ReferenceError('the job of these views is gone')
            self._got[s] = make(s)
        return self._got[s]

    def __iter__(self):
        return (self[s] for s in range(self._n))


class TrainJob:
    """A set of shards trained side by side, one optimizer step of each per launch.

    shards : list[ShardData]
    inits  : list of (U0 [n_user,k], V0 [n_item,k]) float32 numpy / CPU tensors
    perms  : list of int32 [epochs, N_s] arrays (numpy or torch; CPU or device), or int16 batch tags (rng.epoch_tags); a device
             tensor may still be arriving (its rng.Arrival)
    """

    def __init__(self, shards, inits, perms, k, batch, epochs, lr, lam, momentum, lr_decay=1.0, lr_step=50, lazy_rows=None, snapshots=False,
                 touch=None, final_only=False, epoch_reads=False, *, optimizer='sgd', betas=(0.9, 0.999), eps=1e-8):
        """touch: None = the auto rule (touch mode when the job's live rows exceed the Infinity Cache AND the caller reads the tables
        at epoch ends only (epoch_reads) or after the last epoch only (final_only): a job in touch mode cannot be read inside an
        epoch), True / False, or 'index' (touch_mode 3 whatever the epoch length).
        optimizer: 'sgd' (momentum, the reference's) or 'adam' (ultrare_amd/adam.py; betas, eps: its parameters, taken at their float32
        values; `momentum` is not used).  Rows without interactions have no closed form under Adam: the job streams them every step
        (lazy_rows False, no touch mode -- asking for either raises ValueError) and its snapshots are full ones."""
        if optimizer not in ('sgd', 'adam'):
            raise ValueError(f"optimizer {optimizer!r}: 'sgd' or 'adam'")
        self.optimizer = optimizer
        if optimizer == 'adam':
            from . import adam
            if lazy_rows:
                raise ValueError("optimizer='adam' has no closed form for rows without interactions: lazy_rows must be False or None")
            if touch:
                raise ValueError("optimizer='adam' does not run in touch mode: touch must be False or None")
            self._beta1, self._beta2, self._eps = adam.betas32(betas, eps)
            if not (0.0 <= self._beta1 < 1.0 and 0.0 <= self._beta2 < 1.0):
                raise ValueError(f'betas {tuple(betas)!r} must lie in [0, 1)')
            if not self._eps > 0.0:
                raise ValueError(f'eps {eps!r} must be positive (as a float32)')
            lazy_rows, touch = False, False
        assert len(shards) == len(inits) == len(perms) and len(shards) > 0
        self.shards, self.k, self.d = shards, int(k), pad_dim(int(k))
        self.batch, self.epochs, self.device = int(batch), int(epochs), shards[0].device
        # StepLR(step_size=50, gamma): lr of epoch t (scratch.py:69,79-80)
        self._lr_host = np.array([lr * (lr_decay ** (t // lr_step)) for t in range(self.epochs)], dtype=np.float32)
        self._lam, self._mu = float(lam), float(momentum)
        # rows a shard never touches only decay: advance them in closed form when the tables are read
        # (URE_LAZY_ROWS=0 streams them every step, exactly as the reference's dense optimizer does)
        self.lazy_rows = LAZY_ROWS if lazy_rows is None else bool(lazy_rows)
        self._fresh = 0          # ticks for which the lazily advanced rows are up to date
        self._steps = [(sh.N + self.batch - 1) // self.batch for sh in shards]          # optimizer steps per epoch
        self.touch_mode = touch_plan(max(self._steps), self.d, self.batch, sum(sh.n_active for sh in shards) * self.d * 12, self.lazy_rows,
                                     snapshots, touch, final_only, epoch_reads)
        self.touch, self.ahead, self.index = self.touch_mode > 0, self.touch_mode == 2, self.touch_mode == 3
        # end-of-epoch snapshots: 'compact' keeps the n_active rows with interactions only (every other row is a_e * w0 and is
        # rebuilt where it is read: ure_eval_series_compact; needs lazy_rows), True / 'full' keeps complete tables
        self.snapshots = ('compact' if self.lazy_rows else 'full') if snapshots == 'compact' else ('full' if snapshots else False)
        # the small arrays of the job in one copy: the learning rates, then per shard the closed-form scalars its snapshots need
        # (lazy rows: SGD only) or its per-step Adam scalars (struct ure_shard: opt_sc)
        if optimizer == 'adam':
            per_shard = [adam.adam_scalars(self._lr_host, st_, self._beta1, self._beta2) for st_ in self._steps]
        elif self.snapshots:
            per_shard = [closed_form_scalars(self._lr_host, st_, float(np.float32(lam)), float(np.float32(momentum))) for st_ in self._steps]
        else:
            per_shard = []
        self._small = upload_many([self._lr_host] + per_shard, self.device)
        self.lr = self._small[0]
        self._opt_sc = self._small[1:] if optimizer == 'adam' else None
        self._snap_a = self._small[1:] if optimizer == 'sgd' and self.snapshots else None
        self._arrivals = []      # the rng.Arrival of every order that has one: run() waits for their chunks, check_tags() reads their flags
        self.wait_marks = None   # a list: run() adds an event pair around each wait of its stream for a chunk (bench.py)
        self._descs = (nv.UreShard * len(shards))()
        mark('job: start')
        cur = torch.cuda.current_stream(self.device) if torch.device(self.device).type == 'cuda' else None
        seen = set()             # the events this stream already waits for
        for sh in shards:
            if sh.ready is not None and id(sh.ready) not in seen:
                seen.add(id(sh.ready))
                cur.wait_event(sh.ready)
        self._allocate_pools()
        mark('job: pools')
        self._perms, self._init_src = [], []
        for s in range(len(shards)):
            self._init_src.append(self._adopt_start_tables(s, inits[s], cur, seen))       # (alive until the copy below has run)
            self._perms.append(self._adopt_order(s, perms[s], cur))
            self._fill_descriptor(s)
        self._copy_start_tables()
        self.state = _States(len(shards), self._state_of)
        mark('job: tables allocated, descriptors filled')
        self._job = ctypes.c_void_p()
        nv.check(nv.lib().ure_job_create(self._descs, len(shards), ctypes.byref(self._job)), 'ure_job_create')
        mark('job: ure_job_create')
        self.ticks, self.done = int(nv.lib().ure_job_ticks(self._job)), 0
        self.shard_steps = [int(nv.lib().ure_job_shard_steps(self._job, s)) for s in range(len(shards))]

    def _allocate_pools(self):
        """Every float table of every shard from ONE zero-filled allocation (a request of 16 shards made ~130 small allocations
        and fills here: 8-12 ms of host time beside 16 busy worker threads), the snapshots from another.  The descriptors are
        filled from ADDRESSES (_addr); the views of the tables are made when somebody asks for them (self.state), which a
        request does after its launches are queued."""
        self._regions, at, snap_at = [], 0, 0                        # per shard: (regions in _pool, regions in _snap_pool)
        for sh in self.shards:
            pool, snap, at, snap_at = shard_regions(sh.n_user, sh.n_item, sh.n_active, self.d, self.epochs, self.lazy_rows, self.snapshots, at, snap_at,
                                                    adam=self.optimizer == 'adam')
            self._regions.append((pool, snap))
        self._pool = torch.zeros(at, dtype=torch.float32, device=self.device)
        self._snap_pool = torch.empty(snap_at, dtype=torch.float32, device=self.device) if self.snapshots else None

    def _addr(self, s, name):
        """Device address of shard s's region `name` (shard_regions)."""
        pool, snap = self._regions[s]
        return self._pool.data_ptr() + 4 * pool[name][0] if name in pool else self._snap_pool.data_ptr() + 4 * snap[name][0]

    def _adopt_start_tables(self, s, init, cur, seen):
        """The start tables (U0, V0) of shard s as contiguous device tensors, safe to read on the stream `cur`."""
        sh, srcs = self.shards[s], []
        for t, n_rows in zip(init, (sh.n_user, sh.n_item)):
            ev = getattr(t, '_ure_event', None)
            if ev is not None and id(ev) not in seen:               # uploaded on a side stream (rng.shard_draws_async)
                seen.add(id(ev))
                cur.wait_event(ev)
            if ev is not None:
                t.record_stream(cur)
            t = torch.as_tensor(t, dtype=torch.float32)
            assert t.shape == (n_rows, self.k)
            if t.device != torch.device(self.device) or not t.is_contiguous():
                t = t.to(self.device, non_blocking=True).contiguous()
            srcs.append(t)
        return srcs

    def _adopt_order(self, s, perm, cur):
        """The epoch order of shard s on the device: int32 permutations [epochs, N], or -- int16 -- the batch tags made of them (rng.epoch_tags)."""
        from . import rng
        arrival = rng.Arrival.of(perm)                  # (before a conversion could make another tensor)
        if arrival is not None:
            self._arrivals.append(arrival)
            if arrival.whole:                           # uploaded on a side stream in one piece (rng.epoch_perms_async)
                arrival.wait(cur, self.epochs)
        perm = torch.as_tensor(perm)
        assert perm.shape == (self.epochs, self.shards[s].N), f'perm of shard {s} must be [epochs, N]'
        return perm.to(device=self.device, dtype=torch.int16 if perm.dtype == torch.int16 else torch.int32).contiguous()

    def _work_units(self, s):
        """The work of shard s's step kernel: -> (units_ptr, n_units, n_multi, n_split)."""
        sh = self.shards[s]
        if self.index:
            # no work units: the step's items come from the epoch's index.  Rows by weight class (slots per step on average)
            nnz, st_s = sh._sched_head[:min(sh.n_active, INDEX_HEAVY_MAX), 3], self._steps[s]
            n_multi = int(np.count_nonzero(nnz >= INDEX_HEAVY_SLOTS * st_s))
            return sh.ptr('sched'), 0, n_multi, min(n_multi, int(np.count_nonzero(nnz >= INDEX_SPLIT_SLOTS * st_s)))
        if self.touch:
            # epochs of several windows (more than 64 steps): a row of up to TOUCH_ROW_PASSES scan passes stays ONE work item -- its
            # lane group skips the passes without a slot of the step (csrc/mf_touch.h: pass masks) -- instead of one unit per pass
            long_epochs = max(self._steps) > 64
            units, n_units, n_multi = sh.units(self.d, touch=True, min_passes=TOUCH_ROW_PASSES if long_epochs else 1,
                                               unit_passes=TOUCH_UNIT_PASSES if long_epochs else 1)
            return nv.ptr(units), n_units, n_multi, 0
        units = sh.units(self.d)
        return nv.ptr(units), units.shape[0], 0, 0

    def _fill_descriptor(self, s):
        """struct ure_shard of shard s (include/ultrare_hip.h) from the layout's and the pools' addresses."""
        sh, D, d, perm = self.shards[s], self._descs[s], self.d, self._perms[s]
        for name in ('ent_oid', 'ent_r', 'ent_tag', 'ent_src', 'file_tag', 'inv_stage', 'inv_off', 'sched'):
            setattr(D, name, sh.ptr(name))
        D.units, D.n_units, D.n_multi, D.n_split = self._work_units(s)
        D.U[0], D.U[1] = self._addr(s, 'U'), self._addr(s, 'U') + 4 * sh.n_user * d
        D.V[0], D.V[1] = self._addr(s, 'V'), self._addr(s, 'V') + 4 * sh.n_item * d
        D.mU, D.mV, D.sse, D.lr = self._addr(s, 'mU'), self._addr(s, 'mV'), self._addr(s, 'sse'), nv.ptr(self.lr)
        D.perm, D.file_tags = (None, nv.ptr(perm)) if perm.dtype == torch.int16 else (nv.ptr(perm), None)
        D.N, D.n_user, D.n_item, D.d, D.n_active, D.n_slots = sh.N, sh.n_user, sh.n_item, d, sh.n_active, sh.n_slots
        D.batch, D.epochs, D.lam, D.mu, D.touch_mode = self.batch, self.epochs, self._lam, self._mu, self.touch_mode
        if self.snapshots:
            if self._snap_a is not None:
                D.snap_a = self._snap_a[s].data_ptr()
            if self.snapshots == 'compact':
                D.snap, D.row_slot = self._addr(s, 'snap'), sh.ptr('_row_slot')
            else:
                D.snapU, D.snapV = self._addr(s, 'snapU'), self._addr(s, 'snapV')
        if self.lazy_rows:
            D.U0, D.V0, D.lr_host, D.lazy_rows = self._addr(s, 'U0'), self._addr(s, 'V0'), self._lr_host.ctypes.data, 1
        if self.optimizer == 'adam':
            D.optimizer, D.beta1, D.beta2, D.eps = 1, self._beta1, self._beta2, self._eps
            D.vU, D.vV, D.opt_sc = self._addr(s, 'vU'), self._addr(s, 'vV'), self._opt_sc[s].data_ptr()

    def _copy_start_tables(self):
        """The start tables into buffer 0 (and the closed form's copy), every shard's in one launch."""
        src, dst, dst2, rows = zip(*[(t.data_ptr(), self._addr(s, name), self._addr(s, name + '0'), n_rows)
                                     for s, (sh, (U0, V0)) in enumerate(zip(self.shards, self._init_src))
                                     for t, name, n_rows in ((U0, 'U', sh.n_user), (V0, 'V', sh.n_item))])
        ptrs = lambda v: (ctypes.c_void_p * len(v))(*v)
        nv.check(nv.lib().ure_copy_rows_batch(len(src), ptrs(src), ptrs(dst), ptrs(dst2) if self.lazy_rows else None, (ctypes.c_int64 * len(rows))(*rows),
                                              self.k, self.d, nv.stream_handle()), 'ure_copy_rows_batch')
        self._init_src = None             # (allocator: their memory is reused only after the streams they were recorded on have passed this point)

    def _state_of(self, s):
        st = {'perm': self._perms[s]}
        for regions, mem in zip(self._regions[s], (self._pool, self._snap_pool)):
            for name, (first, n, shape) in regions.items():
                if n:                                   # (without lazy_rows a job keeps no U0, V0)
                    st[name] = mem[first:first + n].view(shape)
        if self._snap_a is not None:
            st['snap_a'] = self._snap_a[s]
        return st

    @property
    def chunk_wait_s(self):
        """Host seconds run() has waited for chunks of the orders to be queued."""
        return sum(a.waited_s for a in self._arrivals)

    def steps_per_epoch(self, s):
        return self.shard_steps[s] // self.epochs

    def run(self, n_ticks=None, stream=None):
        """Enqueue the next n_ticks optimizer steps of every shard (default: all)."""
        t1 = self.ticks if n_ticks is None else min(self.ticks, self.done + int(n_ticks))
        while t1 > self.done:
            t_next = t1
            if self._arrivals:
                # the launches of tick t read the order of the epoch AFTER the one a shard is in (the batch tags are prepared one epoch
                # ahead): wait for the chunks up to the one that holds it, and launch only up to where the next one is needed
                min_steps = min(self.steps_per_epoch(s) for s in range(len(self.shards)))
                lead = 2 if self.ahead else 1
                st = stream if stream is not None else torch.cuda.current_stream(self.device)
                horizon = min(a.wait(st, self.done // min_steps + lead, self.wait_marks) for a in self._arrivals)
                if horizon < self.epochs:
                    t_next = min(t_next, max(self.done + 1, (horizon - lead) * min_steps))
            nv.check(nv.lib().ure_job_train(self._job, self.done, t_next, nv.stream_handle(stream)), 'ure_job_train')
            self.done = t_next
        return self.done

    def run_profiled(self, n_ticks, stream=None):
        """Like run(), with every launch bracketed by HIP events (synchronises).
        -> (step kernel ms, launches, tag kernel ms, launches)."""
        t1 = min(self.ticks, self.done + int(n_ticks))
        sm, am = ctypes.c_double(), ctypes.c_double()
        ns, na = ctypes.c_int64(), ctypes.c_int64()
        nv.check(nv.lib().ure_job_train_profiled(self._job, self.done, t1, nv.stream_handle(stream), ctypes.byref(sm),
                                                 ctypes.byref(ns), ctypes.byref(am), ctypes.byref(na)),
                 'ure_job_train_profiled')
        self.done = t1
        return sm.value, ns.value, am.value, na.value

    def run_epochs(self, n_epochs, stream=None):
        """Single-shard convenience: advance by whole epochs."""
        assert len(self.shards) == 1
        return self.run(n_epochs * self.steps_per_epoch(0), stream)

    @staticmethod
    def snapshot_bytes(shards, epochs, d, mode):
        """Device bytes the end-of-epoch snapshots of `shards` need ('compact': active rows only)."""
        rows = sum((sh.n_active if mode == 'compact' else sh.n_user + sh.n_item) for sh in shards)
        return int(epochs) * rows * pad_dim(d) * 4

    def snapshot(self, s, epoch):
        """(U, V) of shard s as they were at the end of `epoch` (padded width; needs full snapshots)."""
        st = self.state[s]
        return st['snapU'][epoch], st['snapV'][epoch]

    def snapshots_of(self, s):
        """All end-of-epoch tables of shard s: (U [epochs, n_user, d], V [epochs, n_item, d]) (full snapshots)."""
        st = self.state[s]
        return st['snapU'], st['snapV']

    def own_scores(self, s, eval_set, stream=None):
        """own [epochs, n] float32: the score of every pair of `eval_set` under shard s's own model after every epoch, from the compact
        snapshots (ure_score_own_compact) -- the half of a series that does not depend on other shards; EvalSet.evaluate_series_own adds
        the fixed models and ranks.  After run()."""
        assert self.snapshots == 'compact' and self.done == self.ticks
        own = torch.empty(self.epochs, max(eval_set.n, 1), dtype=torch.float32, device=self.device)
        state, sh = self.state[s], self.shards[s]
        snap = state['snap']
        if eval_set.n:
            nv.check(nv.lib().ure_score_own_compact(nv.ptr(snap), snap.stride(0), nv.ptr(sh.row_slot()), nv.ptr(state['U0']), nv.ptr(state['V0']),
                                                    nv.ptr(state['snap_a']), sh.n_user, self.epochs, nv.ptr(eval_set.uid), nv.ptr(eval_set.iid), eval_set.n,
                                                    self.d, nv.ptr(own), nv.stream_handle(stream)), 'ure_score_own_compact')
        return own

    def evaluate_series(self, s, eval_set, fixed, out, stream=None, subset=None, lane=0):
        """scratch.py:83-97 for every epoch of shard s on `eval_set`: member e = the ensemble `fixed` + the shard's model
        after epoch e, from whichever kind of snapshots the job keeps.  out: device float64 [epochs, 3].
        subset = (EvalSet.subset_of plan, out_sub [epochs, 3]): the same numbers for a subset of the set's users as well."""
        st = self.state[s]
        if self.snapshots == 'compact':
            sh = self.shards[s]
            return eval_set.evaluate_series_compact(fixed, st['snap'], sh.row_slot(), st['U0'], st['V0'], st['snap_a'], sh.n_user, self.d, out, stream,
                                                    subset=subset, lane=lane)
        return eval_set.evaluate_series(fixed, st['snapU'], st['snapV'], self.d, out, stream, subset=subset, lane=lane)

    def evaluate_series_pair(self, s, test_ev, total_ev, fixed, out_test, out_total, stream=None, lane=0):
        """The two per-epoch series of scratch.py:83-97 -- the shard's own test set and the total test set.  Where the first is a subset of
        the second (the reference builds the total set from the shards' sets: config.py:144-148) ONE series on the total set yields both."""
        plan = test_ev.subset_of(total_ev)
        if plan is None:
            self.evaluate_series(s, test_ev, fixed, out_test, stream, lane=lane)
            return self.evaluate_series(s, total_ev, fixed, out_total, stream, lane=lane)
        return self.evaluate_series(s, total_ev, fixed, out_total, stream, subset=(plan, out_test), lane=lane)

    def materialize(self, stream=None):
        """Bring the lazily advanced rows (lazy_rows) up to date in the current tables."""
        if self.lazy_rows and self._fresh != self.done:
            nv.check(nv.lib().ure_job_materialize(self._job, self.done, nv.stream_handle(stream)), 'ure_job_materialize')
            self._fresh = self.done

    def tables(self, s):
        """Current (U, V) of shard s as device views [rows, k]."""
        U, V = self.padded_tables(s)
        return U[:, :self.k], V[:, :self.k]

    def padded_tables(self, s):
        self.materialize()
        cur = min(self.done, self.shard_steps[s]) & 1
        st = self.state[s]
        return st['U'][cur], st['V'][cur]

    def touch_rows_per_step(self):
        """Touch mode: rows the step kernel reads and rewrites per optimizer step, per shard (average over the shard's
        current window of up to 64 steps, from the window's row masks; synchronises).  None otherwise."""
        if not self.touch:
            return None
        out, win = np.zeros(len(self.shards), dtype=np.int64), np.zeros(len(self.shards), dtype=np.int64)
        nv.check(nv.lib().ure_job_touch_rows(self._job, out.ctypes.data, win.ctypes.data), 'ure_job_touch_rows')
        return [float(n) / max(int(w), 1) for n, w in zip(out, win)]

    _INDEX_ARRAYS = {'step_begin': (0, np.uint32, 1), 'step_item': (1, np.uint32, 1), 'items': (2, np.int32, 4), 'sslot': (3, np.uint32, 4),
                     'W': (4, np.uint64, 1), 'heavy_cnt': (5, np.uint32, 1), 'heavy_cum': (6, np.uint32, 257)}

    def index_array(self, s, name):
        """Test aid (touch_mode 3): one array of shard s's slot index of its current epoch as a host array (ure_job_index_read; synchronises)."""
        which, dtype, cols = self._INDEX_ARRAYS[name]
        n = ctypes.c_int64()
        nv.check(nv.lib().ure_job_index_read(self._job, s, which, None, 0, ctypes.byref(n)), 'ure_job_index_read')
        out = np.empty(n.value // np.dtype(dtype).itemsize, dtype=dtype)
        nv.check(nv.lib().ure_job_index_read(self._job, s, which, out.ctypes.data, out.nbytes, ctypes.byref(n)), 'ure_job_index_read')
        return out.reshape(-1, cols) if cols > 1 else out

    def epoch_sse(self, s):
        """Per-epoch sum of squared training errors (host float64 array; synchronises)."""
        return self.epoch_sse_queue([s]).cpu().numpy()[0]

    def epoch_sse_queue(self, which=None, out=None, stream=None):
        """epoch_sse of the shards `which` (default: all) as a DEVICE float64 tensor [n, epochs] (`out`, if given): one launch
        (ure_epoch_sse_batch: a fixed summation order, the same whoever asks), nothing synchronises."""
        which = list(range(len(self.shards))) if which is None else list(which)
        n = len(which)
        out = torch.empty(n, self.epochs, dtype=torch.float64, device=self.device) if out is None else out
        assert out.shape == (n, self.epochs) and out.dtype == torch.float64 and out.is_contiguous()
        ptrs = (ctypes.c_void_p * n)(*[self._addr(s, 'sse') for s in which])
        rows = (ctypes.c_int64 * n)(*[self.shards[s].n_user for s in which])
        nv.check(nv.lib().ure_epoch_sse_batch(n, ptrs, rows, self.epochs, out.data_ptr(), nv.stream_handle(stream)), 'ure_epoch_sse_batch')
        return out

    def epoch_sse_all(self):
        """epoch_sse of every shard, [n_shards, epochs] (host; synchronises once)."""
        return self.epoch_sse_queue().cpu().numpy()

    def check_tags(self):
        """Device-made batch tags (rng.device_tags): did a workgroup of perm_tags_kernel give up on a shuffle?  It cannot -- and its tags
        then match no batch, so nothing trained on a wrong permutation -- but a job that trained on fewer rows must not pass silently.
        Reads one small flag array (synchronises): called by close() and by callers right after they read a job's results."""
        seen = set()
        for a in self._arrivals:
            a.check(seen)

    def close(self):
        if self._job:
            nv.lib().ure_job_destroy(self._job)
            self._job = ctypes.c_void_p()
            try:
                self.check_tags()                 # (ure_job_destroy has waited for the device)
            finally:
                # the device memory goes back now: tables, snapshots, batch tags and what made them
                self._pool = self._snap_pool = self._small = self._opt_sc = self._snap_a = None
                self._perms, self._arrivals = [], []
                if isinstance(getattr(self, 'state', None), _States):
                    self.state._got.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_LOG2_TAB = np.log2(np.arange(2, 11)).astype(np.float64)      # utils.py:210
_IDCG = 1.0 + np.sum(np.ones(9) / _LOG2_TAB)                   # computeDCG(np.ones(10)), utils.py:207
_LOG2_TAB = np.concatenate([_LOG2_TAB, [_IDCG]])


class FixedBase:
    """The fixed models of a series given as their running sum on the set's pairs (ScoreCache.base): n models, base [n_pairs] float32."""

    def __init__(self, n, base):
        self.n, self.base = int(n), base

    def __len__(self):
        return self.n


class ScoreCache:
    """Score vectors of a request's models on ONE test set, each model scored once (ure_score with one model: what it adds to an ensemble's
    running sum), and an ensemble's base as their sum in list order (ure_sum_vectors) -- the additions ure_score makes over a list of
    tables, so a series evaluated from such a base has the same bits.  Everything is queued on the current stream."""
    LIMIT_BYTES = 4 << 30

    def __init__(self, eval_set, d):
        self.ev, self.d, self.vec = eval_set, int(d), {}

    def fits(self, n_vectors):
        return int(n_vectors) * 4 * self.ev.n <= self.LIMIT_BYTES

    def base(self, before):
        """before: [(key, get_tables, arg)] in the ensemble's order; get_tables(arg) -> padded (U, V) of the model `key` names.  -> FixedBase"""
        if not before:
            return FixedBase(0, None)
        for key, get, arg in before:
            if key not in self.vec:
                U, V = get(arg)
                self.vec[key] = self.ev.score_vector(U, V, self.d)
        out = torch.empty(max(self.ev.n, 1), dtype=torch.float32, device=self.ev.device)
        n = len(before)
        ptrs = (ctypes.c_void_p * n)(*[self.vec[key].data_ptr() for key, _, _ in before])
        nv.check(nv.lib().ure_sum_vectors(ptrs, n, self.ev.n, nv.ptr(out), nv.stream_handle()), 'ure_sum_vectors')
        return FixedBase(n, out)


def _ptr_arrays(tables, d):
    """-> (U pointers, V pointers) of a list of padded (U, V): contiguous device tables of row width d."""
    for U, V in tables:
        assert U.is_contiguous() and V.is_contiguous() and U.shape[1] == d and V.shape[1] == d
    n = max(len(tables), 1)
    return (ctypes.c_void_p * n)(*[U.data_ptr() for U, _ in tables]), (ctypes.c_void_p * n)(*[V.data_ptr() for _, V in tables])


def _fixed_args(fixed, d, own_base):
    """-> (U pointers, V pointers, n_fixed, base pointer) of a series call for `fixed` = a list of padded (U, V) or a FixedBase."""
    if isinstance(fixed, FixedBase):
        return None, None, fixed.n, (nv.ptr(fixed.base) if fixed.n else nv.ptr(own_base))
    return (*_ptr_arrays(fixed, d), len(fixed), nv.ptr(own_base))


class EvalSet:
    """Test interactions grouped by user (first-appearance order, utils.py:156-163)
    and resident on the device, plus the output buffers of the two eval kernels."""

    def __init__(self, uid, iid, rating, device=None):
        uid = np.ascontiguousarray(uid, dtype=np.int32)
        iid = np.ascontiguousarray(iid, dtype=np.int32)
        rating = np.ascontiguousarray(rating, dtype=np.float32)
        self.n = len(uid)
        self.device = device or _device()
        self.n_wide = self.n_half = 0
        if self.n:
            _, first = np.unique(uid, return_index=True)
            users = uid[np.sort(first)]                       # first-appearance order (utils.py:156-163) ...
            rank = np.empty(int(uid.max()) + 1, dtype=np.int64)
            rank[users] = np.arange(len(users))
            counts = np.bincount(rank[uid], minlength=len(users))
            # ... inside three classes: users with more than 32 test items first (a wavefront each in the ranking kernel), then those
            # with 17 .. 32 (two per wavefront), then the others (four per wavefront).  The metrics are means over users: their order
            # does not enter.
            klass = np.where(counts > 32, 0, np.where(counts > 16, 1, 2))
            self.n_wide, self.n_half = int((klass == 0).sum()), int((klass == 1).sum())
            cls = np.argsort(klass, kind='stable')
            users, counts = users[cls], counts[cls]
            rank[users] = np.arange(len(users))
            order = np.argsort(rank[uid], kind='stable')
        else:
            users, order, counts = np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64)
        off = np.zeros(len(users) + 1, dtype=np.int32)
        np.cumsum(counts, out=off[1:])
        self.users, self.n_users = users, len(users)
        dev = self.device
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.uid, self.iid, self.rating, self.off = to(uid[order]), to(iid[order]), to(rating[order]), to(off)
        self.pred = torch.zeros(max(self.n, 1), dtype=torch.float32, device=dev)
        self.hits = torch.zeros(max(self.n_users, 1), dtype=torch.int32, device=dev)
        self.ndcg = torch.zeros(max(self.n_users, 1), dtype=torch.float64, device=dev)
        self.sse = torch.zeros(SCORE_PARTIALS, dtype=torch.float64, device=dev)
        self.log2 = to(_LOG2_TAB)
        self.order = order
        # host copies in the set's own order: what subset_of() compares
        self._h_iid, self._h_rating, self._h_off = iid[order], rating[order], off
        self._subsets = {}
        # the ranking of the ratings is a property of the test set: once, here
        self.top_rating = torch.empty(max(self.n_users, 1) * 10, dtype=torch.int32, device=dev)
        if self.n_users:
            nv.check(nv.lib().ure_eval_rank_ratings(nv.ptr(self.off), self.n_users, nv.ptr(self.rating), nv.ptr(self.top_rating),
                                                    nv.stream_handle()), 'ure_eval_rank_ratings')

    def subset_of(self, total):
        """This set as a subset of `total`: -> {'users': device int32 [n_users] (this set's users as indices into total's user order), 'n': n_users,
        'pairs': device int32 [n] (its pairs as indices into total's pair order), 'n_pairs': n}
        when every user of this set is in `total` with exactly the same (item, rating) rows in the same order -- the reference's total test
        set is the shards' test sets side by side (config.py:144-148) --, else None.  Checked on the host once per pair of sets and kept
        (the sets live with their loaders).  With a plan, a series on `total` also yields this set's three numbers (ure_eval_subset)
        instead of a second series on the same models and pairs."""
        if total is self or self.n == 0 or total.n == 0:
            return None
        key = id(total)
        hit = self._subsets.get(key)
        if hit is not None and hit[0]() is total:
            return hit[1]
        import weakref
        plan = None
        pos = getattr(total, '_user_pos', None)
        if pos is None:
            pos = np.full(int(total.users.max()) + 1, -1, dtype=np.int64)
            pos[total.users] = np.arange(total.n_users)
            total._user_pos = pos
        mine = self.users.astype(np.int64)
        if mine.max() < len(pos):
            at = pos[mine]
            cnt = np.diff(self._h_off).astype(np.int64)
            if (at >= 0).all() and np.array_equal(cnt, np.diff(total._h_off).astype(np.int64)[at]):
                # the rows of every user, side by side in this set's order: equal items and ratings, in the same order
                src = np.repeat(total._h_off[at].astype(np.int64) - self._h_off[:-1].astype(np.int64), cnt) + np.arange(self.n, dtype=np.int64)
                if np.array_equal(total._h_iid[src], self._h_iid) and np.array_equal(total._h_rating[src], self._h_rating):
                    up = upload_many([at.astype(np.int32), src.astype(np.int32)], self.device)
                    plan = {'users': up[0], 'n': int(self.n_users), 'pairs': up[1], 'n_pairs': int(self.n)}
        self._subsets[key] = (weakref.ref(total), plan)
        return plan

    def _subset_after(self, subset, m, e0, st, b):
        """ure_eval_subset on the m members a series call just left in the scratch buffers b (subset = (plan of subset_of, out [E, 3]))."""
        plan, out_sub = subset
        nv.check(nv.lib().ure_eval_subset(nv.ptr(plan['users']), plan['n'], nv.ptr(plan['pairs']), plan['n_pairs'], nv.ptr(b['pred']), nv.ptr(self.rating),
                                          nv.ptr(b['hits']), nv.ptr(b['ndcg']), self.n, self.n_users, m, nv.ptr(out_sub[e0]), st), 'ure_eval_subset')

    def evaluate(self, models, d, stream=None, top_k=10, out=None, combiner=None):
        """baseTest (utils.py:115-187) for an ensemble: `models` = list of (U, V) device
        tensors with row stride d (the padded width).  Returns (rmse, ndcg, hr).
        combiner (a combine.Combiner, optional): the pairs are scored with its fitted weights (score_weighted) instead of the
        plain mean; the ranking and the reduction are the same calls on the same buffers."""
        assert top_k == 10, 'the kernel implements the reference default top_k=10'
        if combiner is not None and combiner.n_models != len(models):
            raise ValueError(f'the combiner was fitted on {combiner.n_models} models, not {len(models)}')
        if self.n == 0:
            if out is not None:
                return out.fill_(float('nan'))
            return float('nan'), float('nan'), float('nan')
        L, st = nv.lib(), nv.stream_handle(stream)
        S = len(models)
        if combiner is not None:
            W, gou = combiner.on_device(self.device, int(models[0][0].shape[0]))
            score_weighted(models, d, self.uid, self.iid, self.rating, combiner.link_code, W, gou, pred=self.pred, sse=self.sse, stream=stream)
        for c0 in (range(0, S, nv.MAX_MODELS_PER_CALL) if combiner is None else ()):
            chunk = models[c0:c0 + nv.MAX_MODELS_PER_CALL]
            Up, Vp = _ptr_arrays(chunk, d)
            nv.check(L.ure_score(Up, Vp, len(chunk), S, int(c0 == 0), int(c0 + len(chunk) >= S),
                                 nv.ptr(self.uid), nv.ptr(self.iid), nv.ptr(self.rating), self.n, d,
                                 nv.ptr(self.pred), nv.ptr(self.sse), st), 'ure_score')
        return self._rank_and_reduce(st, top_k, out)

    def evaluate_nmf(self, models, stream=None, top_k=10, out=None):
        """baseTest for an ensemble of NeuMF models: `models` = list of (U, V, dense, k, layers) (nmf.py's tables and dense vector
        on the device).  One ure_nmf_score call per model, in list order, under ure_score's protocol; the ranking and the reduction
        are evaluate's calls on the same buffers.  Returns (rmse, ndcg, hr), or `out`."""
        assert top_k == 10, 'the kernel implements the reference default top_k=10'
        if not models:
            raise ValueError('evaluate_nmf needs at least one model')
        if self.n == 0:
            if out is not None:
                return out.fill_(float('nan'))
            return float('nan'), float('nan'), float('nan')
        S = len(models)
        for s, (U, V, dense, k, layers) in enumerate(models):
            nmf_score(U, V, dense, k, layers, self.uid, self.iid, self.rating, self.pred, self.sse, S, s == 0, s == S - 1, stream)
        return self._rank_and_reduce(nv.stream_handle(stream), top_k, out)

    def _rank_and_reduce(self, st, top_k, out):
        """The per-user ranking and the reduction of what a scoring pass left in pred and sse."""
        L = nv.lib()
        nv.check(L.ure_eval_users(nv.ptr(self.off), self.n_users, nv.ptr(self.pred), nv.ptr(self.rating),
                                  nv.ptr(self.log2), nv.ptr(self.hits), nv.ptr(self.ndcg), nv.ptr(self.top_rating), self.n_wide, self.n_half, st),
                 'ure_eval_users')
        if out is not None:
            # queued evaluation: (rmse, ndcg, hr) land in `out` (device, 3 float64); nothing synchronises
            nv.check(L.ure_eval_reduce(nv.ptr(self.hits), nv.ptr(self.ndcg), self.n_users, nv.ptr(self.sse), self.n,
                                       nv.ptr(out), st), 'ure_eval_reduce')
            return out
        sse = float(self.sse.cpu().numpy().sum())
        hits = self.hits[:self.n_users].cpu().numpy()
        ndcg = self.ndcg[:self.n_users].cpu().numpy()
        rmse = float(np.sqrt(sse / self.n))
        return rmse, float(np.mean(ndcg)), float(np.mean(hits / top_k))

    def _series_buffers(self, E, lane=0):
        """Scratch of one series call (kept on the set): -> (buffers, members per call).  lane: series that run side by side on
        different streams (Sisa: the shards of a request) take a scratch of their own each; a lane belongs to ONE stream."""
        per_call = max(1, min(E, SERIES_SCRATCH_BYTES // (4 * self.n)))
        lanes = self.__dict__.setdefault('_series_lanes', {})
        if lanes.get(lane, (0, None))[0] < per_call:
            dev = self.device
            lanes[lane] = (per_call, {'base': torch.empty(self.n, dtype=torch.float32, device=dev),
                                      'pred': torch.empty(per_call, self.n, dtype=torch.float32, device=dev),
                                      'sse': torch.empty(per_call, SCORE_PARTIALS, dtype=torch.float64, device=dev),
                                      'hits': torch.empty(per_call, max(self.n_users, 1), dtype=torch.int32, device=dev),
                                      'ndcg': torch.empty(per_call, max(self.n_users, 1), dtype=torch.float64, device=dev)})
        return lanes[lane][1], per_call

    def score_vector(self, U, V, d, stream=None):
        """What the model (U, V) (padded, device) adds to an ensemble's running sum on this set's pairs: 0 + <u, v> per pair, float32
        [n] in the set's own order (ure_score with one model, first = 1, last = 0)."""
        Up, Vp = _ptr_arrays([(U, V)], d)
        out = torch.empty(max(self.n, 1), dtype=torch.float32, device=self.device)
        if self.n:
            nv.check(nv.lib().ure_score(Up, Vp, 1, 1, 1, 0, nv.ptr(self.uid), nv.ptr(self.iid), nv.ptr(self.rating), self.n, d, nv.ptr(out), None,
                                        nv.stream_handle(stream)), 'ure_score')
        return out

    def _series(self, E, fixed, d, out, stream, call, subset=None, lane=0, nan_if_empty=True):
        """The frame the three series routes share: out [E, 3] checked, the scratch of `lane`, the fixed models, then per chunk of
        members call(e0, m, head, tail) -- the route's native call for members e0 .. e0 + m, between the arguments every route starts
        (the fixed models) and ends with (the set, the scratch, out[e0], the stream) -- and the subset's numbers."""
        assert out.shape == (E, 3) and out.dtype == torch.float64 and out.is_contiguous()
        if nan_if_empty and self.n == 0:
            return out.fill_(float('nan'))
        st = nv.stream_handle(stream)
        b, per_call = self._series_buffers(E, lane)
        Up, Vp, n_fixed, base_ptr = _fixed_args(fixed, d, b['base'])
        for e0 in range(0, E, per_call):
            m = min(per_call, E - e0)
            call(e0, m, (Up, Vp, n_fixed),
                 (nv.ptr(self.uid), nv.ptr(self.iid), nv.ptr(self.rating), self.n, d, nv.ptr(self.off), self.n_users, nv.ptr(self.log2), base_ptr,
                  nv.ptr(b['pred']), nv.ptr(b['sse']), nv.ptr(b['hits']), nv.ptr(b['ndcg']), nv.ptr(out[e0]), nv.ptr(self.top_rating),
                  self.n_wide, self.n_half, st))
            if subset is not None:
                self._subset_after(subset, m, e0, st, b)
        return out

    def evaluate_series(self, fixed, U_series, V_series, d, out, stream=None, subset=None, lane=0):
        """scratch.py:83-97 for every epoch of a shard in four launches (ure_eval_series): member e of
        the series is the ensemble `fixed` + [(U_series[e], V_series[e])]; out[e] (device float64
        [E, 3]) receives its (rmse, ndcg, hr).  Nothing synchronises."""
        assert U_series.is_contiguous() and V_series.is_contiguous() and U_series.shape[2] == d and V_series.shape[2] == d
        call = lambda e0, m, head, tail: nv.check(nv.lib().ure_eval_series(
            *head, nv.ptr(U_series[e0]), nv.ptr(V_series[e0]), U_series.stride(0), V_series.stride(0), m, *tail), 'ure_eval_series')
        return self._series(int(U_series.shape[0]), fixed, d, out, stream, call, subset, lane)

    def evaluate_series_compact(self, fixed, snap, row_slot, U0, V0, snap_a, n_user_rows, d, out, stream=None, subset=None, lane=0):
        """evaluate_series on COMPACT snapshots (ure_eval_series_compact): snap [E, n_active, d] holds the rows with
        interactions in the shard, row_slot maps a row id to its place in it (-1: the row is snap_a[e] * (U0 | V0)[row])."""
        E = int(snap.shape[0])
        assert snap.is_contiguous() and snap.shape[2] == d and U0.is_contiguous() and V0.is_contiguous() and U0.shape[1] == d and V0.shape[1] == d
        assert row_slot.dtype == torch.int32 and row_slot.numel() == U0.shape[0] + V0.shape[0] and snap_a.numel() == E
        call = lambda e0, m, head, tail: nv.check(nv.lib().ure_eval_series_compact(
            *head, nv.ptr(snap[e0]), snap.stride(0), nv.ptr(row_slot), nv.ptr(U0), nv.ptr(V0), nv.ptr(snap_a[e0:]), int(n_user_rows), m, *tail),
            'ure_eval_series_compact')
        return self._series(E, fixed, d, out, stream, call, subset, lane)

    def evaluate_series_own(self, fixed, own, d, out, stream=None):
        """The second half of a series whose own scores own [E, n] exist (ure_eval_series_own)."""
        assert own.is_contiguous() and own.shape[1] == self.n
        call = lambda e0, m, head, tail: nv.check(nv.lib().ure_eval_series_own(*head, nv.ptr(own[e0]), m, *tail), 'ure_eval_series_own')
        return self._series(int(own.shape[0]), fixed, d, out, stream, call, nan_if_empty=False)

    def predictions(self):
        """Ensemble predictions of the last evaluate() in the caller's original row order."""
        out = np.empty(self.n, dtype=np.float32)
        out[self.order] = self.pred[:self.n].cpu().numpy()
        return out


def merge_rows(dst, src, rows, stream=None):
    """dst[rows] = src[rows] on the device (sisa.py:55-56)."""
    if not torch.is_tensor(rows):
        rows = to_device_async(np.asarray(rows, dtype=np.int64), dst.device)
    assert rows.dtype == torch.int64 and rows.device == dst.device
    assert dst.is_contiguous() and src.is_contiguous() and dst.shape == src.shape
    nv.check(nv.lib().ure_merge_rows(nv.ptr(dst), nv.ptr(src), nv.ptr(rows), rows.numel(), dst.shape[1],
                                     nv.stream_handle(stream)), 'ure_merge_rows')
    return dst


RECOMMEND_MAX_K = 128    # kRecMaxK of csrc/mf_recommend.hip


def exclusion_rows(csr, users):
    """The exclusion CSR of ure_recommend_topk for a batch of users: (off [n + 1] int64, items int32) with query row q holding
    the column indices of `csr`'s row users[q] (a scipy CSR with user ids as rows, as read.readSparseMat returns), sorted and
    unique.  Host only."""
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    indptr, indices = np.asarray(csr.indptr, dtype=np.int64), np.asarray(csr.indices)
    if users.size and (users.min() < 0 or users.max() >= len(indptr) - 1):
        raise ValueError(f'user ids outside the exclusion matrix\'s {len(indptr) - 1} rows')
    rows = [np.unique(indices[indptr[u]:indptr[u + 1]]).astype(np.int32) for u in users]
    off = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int32)).astype(np.int32)


def _ranking_weights(weights, S, what):
    """(link code, W, group_of_user) of the weights = (link, W, group_of_user or None) of a ranking call, checked as score_weighted
    checks them: W a device float64 [G, S + 1] tensor, group_of_user a device int32 tensor or None (row 0 for every user)."""
    if not isinstance(weights, (tuple, list)) or len(weights) != 3:
        raise ValueError(f'{what}: weights = (link, W, group_of_user or None)')
    link, W, gou = weights
    code = _link_code(link)
    if not 1 <= S <= nv.MAX_MODELS_PER_CALL:
        raise ValueError(f'{what} takes 1 .. {nv.MAX_MODELS_PER_CALL} models under weights, not {S}')
    if not (torch.is_tensor(W) and W.is_cuda and W.dtype == torch.float64 and W.dim() == 2 and W.shape[1] == S + 1 and W.shape[0] >= 1):
        raise ValueError(f'W must be a device float64 [G, {S + 1}] tensor')
    if gou is not None and not (torch.is_tensor(gou) and gou.is_cuda and gou.dtype == torch.int32 and gou.is_contiguous() and gou.numel() >= 1):
        raise ValueError('group_of_user must be a contiguous, non-empty device torch.int32 tensor')
    return code, W.contiguous(), gou


def recommend(tables, d, users, k, excl=None, stream=None, weights=None):
    """Top-k items of every user of `users` over the whole catalogue (ure_recommend_topk): tables = [(U, V)] device tensors of
    width d, the scores those of ure_score over the same list (the ensemble mean of baseTest), excl = (off, items) from
    exclusion_rows or None.  Returns (scores [n, k] float32, items [n, k] int64) on the device; padding is (NaN, -1).
    weights = (link, W, group_of_user or None) on the device: the scores are score_weighted's for the same pairs instead (the
    learned shard combiner, ure_recommend_topk_weighted; at most 32 models), ordered by the same key."""
    users = users.detach().cpu().numpy() if torch.is_tensor(users) else np.asarray(users)
    users = users.astype(np.int64).reshape(-1)
    if not tables:
        raise ValueError('recommend needs at least one model')
    n_user, n_item = int(tables[0][0].shape[0]), int(tables[0][1].shape[0])
    if not 1 <= int(k) <= RECOMMEND_MAX_K:
        raise ValueError(f'k = {k} outside [1, {RECOMMEND_MAX_K}]')
    if users.size == 0:
        raise ValueError('recommend needs at least one user')
    if users.min() < 0 or users.max() >= n_user:
        raise ValueError(f'user ids outside [0, {n_user})')
    if excl is not None:
        off, items = (np.asarray(excl[0], dtype=np.int64), np.asarray(excl[1], dtype=np.int32))
        if off.shape != (len(users) + 1,) or off[0] != 0 or off[-1] != len(items) or np.any(np.diff(off) < 0):
            raise ValueError('exclusion offsets do not describe one row per user')
        if items.size and (items.min() < 0 or items.max() >= n_item):
            raise ValueError(f'excluded items outside [0, {n_item})')
    for U, V in tables:
        if not (U.is_cuda and V.is_cuda):
            raise nv.NativeError('recommend runs on the HIP device only (no CPU fallback)')
        assert U.shape == (n_user, d) and V.shape == (n_item, d) and U.is_contiguous() and V.is_contiguous() and U.dtype == V.dtype == torch.float32
    dev = tables[0][0].device
    n, k = len(users), int(k)
    uid = to_device_async(users.astype(np.int32), dev)
    e_off = e_items = None
    if excl is not None:
        e_off = to_device_async(off, dev)
        e_items = to_device_async(items if items.size else np.zeros(1, dtype=np.int32), dev)
    L = nv.lib()
    if weights is not None:
        code, W, gou = _ranking_weights(weights, len(tables), 'recommend')
        nbytes = int(L.ure_recommend_weighted_scratch(n, n_item, k, d, len(tables), code, int(W.shape[0])))
        if nbytes < 0:
            raise ValueError(f'ure_recommend_weighted_scratch refused n_query = {n}, n_item = {n_item}, k = {k}, d = {d}')
    else:
        nbytes = int(L.ure_recommend_scratch(n, n_item, k))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    scores = torch.empty(n, k, dtype=torch.float32, device=dev)
    items_out = torch.empty(n, k, dtype=torch.int32, device=dev)
    Up = (ctypes.c_void_p * len(tables))(*[U.data_ptr() for U, _ in tables])
    Vp = (ctypes.c_void_p * len(tables))(*[V.data_ptr() for _, V in tables])
    if weights is not None:
        nv.check(L.ure_recommend_topk_weighted(Up, Vp, len(tables), nv.ptr(uid), n, n_item, d, nv.ptr(e_off), nv.ptr(e_items), k, nv.ptr(scores),
                                               nv.ptr(items_out), nv.ptr(scratch), scratch.numel(), nv.stream_handle(stream), code, nv.ptr(W),
                                               int(W.shape[0]), nv.ptr(gou), int(gou.numel()) if gou is not None else 0),
                 'ure_recommend_topk_weighted')
        return scores, items_out.long()
    nv.check(L.ure_recommend_topk(Up, Vp, len(tables), nv.ptr(uid), n, n_item, d, nv.ptr(e_off), nv.ptr(e_items), k, nv.ptr(scores),
                                  nv.ptr(items_out), nv.ptr(scratch), scratch.numel(), nv.stream_handle(stream)), 'ure_recommend_topk')
    return scores, items_out.long()


def _check_rows(off, items, n_rows, n_item, what):
    """(off int64 [n_rows + 1], items int32) of a per-query CSR, or ValueError: offsets from 0 to len(items), non-decreasing,
    items in [0, n_item)."""
    off, items = np.asarray(off, dtype=np.int64).reshape(-1), np.asarray(items).reshape(-1)
    if off.shape != (n_rows + 1,) or off[0] != 0 or off[-1] != len(items) or np.any(np.diff(off) < 0):
        raise ValueError(f'{what} offsets do not describe one row per user')
    if items.size and (items.min() < 0 or items.max() >= n_item):
        raise ValueError(f'{what} items outside [0, {n_item})')
    return off, items.astype(np.int32)


def rank_pairs(tables, d, users, targets, excl=None, stream=None, weights=None):
    """Exact full-catalogue rank of every (user, target item) pair (ure_rank_pairs): tables = [(U, V)] device tensors of width d,
    targets = (off [n + 1], items) with query row q's targets items[off[q]:off[q + 1]] (any order, duplicates, empty rows),
    excl = (off, items) from exclusion_rows or None.  rank = the number of non-excluded items whose (score, id) key beats the
    target's -- the position recommend would give it -- or -1 for an excluded target.  Returns ranks [len(items)] int32 on the
    device, in input order.  weights = (link, W, group_of_user or None) on the device: the ranks under score_weighted's scores,
    as recommend(..., weights=) orders them (ure_rank_pairs_weighted)."""
    users = users.detach().cpu().numpy() if torch.is_tensor(users) else np.asarray(users)
    users = users.astype(np.int64).reshape(-1)
    if not tables:
        raise ValueError('rank_pairs needs at least one model')
    n_user, n_item = int(tables[0][0].shape[0]), int(tables[0][1].shape[0])
    if users.size == 0:
        raise ValueError('rank_pairs needs at least one user')
    if users.min() < 0 or users.max() >= n_user:
        raise ValueError(f'user ids outside [0, {n_user})')
    t_off, t_items = _check_rows(*(t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in targets), len(users), n_item, 'target')
    if excl is not None:
        e_off_h, e_items_h = _check_rows(*(t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in excl), len(users), n_item, 'exclusion')
    for U, V in tables:
        if not (U.is_cuda and V.is_cuda):
            raise nv.NativeError('rank_pairs runs on the HIP device only (no CPU fallback)')
        assert U.shape == (n_user, d) and V.shape == (n_item, d) and U.is_contiguous() and V.is_contiguous() and U.dtype == V.dtype == torch.float32
    dev = tables[0][0].device
    n, n_t = len(users), len(t_items)
    if weights is not None:
        code, W, gou = _ranking_weights(weights, len(tables), 'rank_pairs')
    ranks = torch.empty(max(n_t, 1), dtype=torch.int32, device=dev)
    if n_t == 0:
        return ranks[:0]
    uid = to_device_async(users.astype(np.int32), dev)
    d_off, d_items = to_device_async(t_off, dev), to_device_async(t_items, dev)
    e_off = e_items = None
    if excl is not None:
        e_off = to_device_async(e_off_h, dev)
        e_items = to_device_async(e_items_h if e_items_h.size else np.zeros(1, dtype=np.int32), dev)
    L = nv.lib()
    nbytes = int(L.ure_rank_pairs_scratch(n, n_t, n_item, d) if weights is None else
                 L.ure_rank_pairs_weighted_scratch(n, n_t, n_item, d, len(tables), code, int(W.shape[0])))
    if nbytes < 0:
        raise ValueError(f'ure_rank_pairs_scratch refused n_query = {n}, n_targets = {n_t}, n_item = {n_item}, d = {d}')
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    Up = (ctypes.c_void_p * len(tables))(*[U.data_ptr() for U, _ in tables])
    Vp = (ctypes.c_void_p * len(tables))(*[V.data_ptr() for _, V in tables])
    if weights is not None:
        nv.check(L.ure_rank_pairs_weighted(Up, Vp, len(tables), nv.ptr(uid), n, n_item, d, nv.ptr(d_off), nv.ptr(d_items), nv.ptr(e_off),
                                           nv.ptr(e_items), nv.ptr(ranks), nv.ptr(scratch), nbytes, nv.stream_handle(stream), code, nv.ptr(W),
                                           int(W.shape[0]), nv.ptr(gou), int(gou.numel()) if gou is not None else 0), 'ure_rank_pairs_weighted')
        return ranks
    nv.check(L.ure_rank_pairs(Up, Vp, len(tables), nv.ptr(uid), n, n_item, d, nv.ptr(d_off), nv.ptr(d_items), nv.ptr(e_off), nv.ptr(e_items),
                              nv.ptr(ranks), nv.ptr(scratch), nbytes, nv.stream_handle(stream)), 'ure_rank_pairs')
    return ranks


# ---------------------------------------------------------------------------------------------------------------------
# Reductions of a user-by-user distance matrix (csrc/pair_dist.hip): the k-medoids, LPA and kNN comparison clusterers.
# metric None / 'given': src is the float32 n x n array D itself; 'euclidean' / 'cosine' / 'manhattan': src is X [n x d]
# and D is streamed from it, never materialised.  src may also be a CsrSet (below) with one of the three streamed metrics:
# the same D, bit for bit, from the sparse matrix (the CSR tile producer; the contract is sparse_pair.py), X never formed.
# ---------------------------------------------------------------------------------------------------------------------
PAIR_METRICS = {'given': 0, 'euclidean': 1, 'cosine': 2, 'manhattan': 3}


class _PairCall:
    """One source of D for the four reductions: the entry-name prefix, the leading arguments of the C call, n, the device."""

    def __init__(self, src, metric):
        if isinstance(src, CsrSet):
            from .sparse_pair import check_pair_metric
            code = PAIR_METRICS[check_pair_metric(metric)]
            _csr_has(src, 'CSR')
            if not src.row_off.is_cuda:
                raise nv.NativeError('pair distances run on the HIP device only (no CPU fallback)')
            for t, what in ((src.col, 'col'), (src.val, 'val')):
                _csr_same_device(src.row_off, t, what)
            self.prefix, self.n, self.device, self.keep = 'ure_csr_pair_', src.n, src.row_off.device, src
            self.head = (nv.ptr(src.row_off), nv.ptr(src.col), nv.ptr(src.val), src.n, src.n_item, code)
        else:
            t, n, d, code = pair_source(src, metric)
            self.prefix, self.n, self.device, self.keep = 'ure_pair_', n, t.device, t
            self.head = (nv.ptr(t), n, d, code)

    def __call__(self, name, *args, stream=None):
        entry = self.prefix + name
        nv.check(getattr(nv.lib(), entry)(*self.head, *args, nv.stream_handle(stream)), entry)


def pair_source(src, metric=None):
    """(device float32 tensor, n, d, metric code) of a distance source, or TypeError / ValueError: the given array must be a
    square float32 array (no silent cast), X a 2-D float array with n >= 1, d >= 1."""
    name = 'given' if metric is None else metric
    if name not in PAIR_METRICS:
        raise ValueError(f'metric must be None (a given n x n array) or one of euclidean / cosine / manhattan, not {metric!r}')
    if name == 'given':
        if (src.dtype != torch.float32) if torch.is_tensor(src) else (np.asarray(src).dtype != np.float32):
            raise TypeError('a given distance array must be float32 (n x n)')
        if tuple(src.shape)[:1] * 2 != tuple(src.shape) or src.shape[0] < 1:
            raise ValueError(f'a given distance array must be square, not {tuple(src.shape)}')
    elif len(src.shape) != 2 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError(f'the embedding must be 2-D with n, d >= 1, not {tuple(src.shape)}')
    if torch.is_tensor(src):
        if not src.is_cuda:
            raise nv.NativeError('pair distances run on the HIP device only (no CPU fallback)')
        t = src.to(torch.float32).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).to(_device())
    n, d = int(t.shape[0]), int(t.shape[1])
    return t, n, d, PAIR_METRICS[name]


def _index_tensor(ids, dev, hi, what):
    ids = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    ids = ids.astype(np.int64).reshape(-1)
    if ids.size == 0:
        raise ValueError(f'{what}: need at least one')
    if ids.min() < 0 or ids.max() >= hi:
        raise ValueError(f'{what} outside [0, {hi})')
    return to_device_async(ids.astype(np.int32), dev)


def pair_knn(src, n_nb, metric=None, query=None, splits=0, stream=None):
    """The n_nb nearest columns of each query row of D (ure_pair_knn; ure_csr_pair_knn for a CsrSet): query None = every row.
    Returns (dist [n_q, n_nb] float32, idx [n_q, n_nb] int64) on the device, ascending by (distance, column); the row itself
    is in its own list."""
    call = _PairCall(src, metric)
    n, dev = call.n, call.device
    n_nb = int(n_nb)
    if not 1 <= n_nb <= min(n, 128):
        raise ValueError(f'n_nb must be in [1, min(n, 128)] = [1, {min(n, 128)}], not {n_nb}')
    q = None if query is None else _index_tensor(query, dev, n, 'query rows')
    nq = n if q is None else int(q.numel())
    sizer = call.prefix + 'knn_scratch'
    nbytes = int(getattr(nv.lib(), sizer)(nq, n, n_nb, int(splits)))
    if nbytes < 0:
        raise ValueError(f'{sizer} refused n_query = {nq}, n = {n}, n_nb = {n_nb}, splits = {splits}')
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dist = torch.empty(nq, n_nb, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, n_nb, dtype=torch.int32, device=dev)
    call('knn', nv.ptr(q), nq, n_nb, int(splits), nv.ptr(dist), nv.ptr(idx), nv.ptr(scratch), nbytes, stream=stream)
    return dist, idx.long()


def pair_rowsum(src, metric=None, stream=None):
    """R[u] = sum_v D[u, v] [n] float32 on the device (ure_pair_rowsum / ure_csr_pair_rowsum), in np.sum(D, axis=1)'s
    pairwise order."""
    call = _PairCall(src, metric)
    R = torch.empty(call.n, dtype=torch.float32, device=call.device)
    call('rowsum', nv.ptr(R), stream=stream)
    return R


def pair_cols(src, cols, metric=None, stream=None):
    """D[:, cols] [n, m] float32 on the device (ure_pair_cols / ure_csr_pair_cols)."""
    call = _PairCall(src, metric)
    c = _index_tensor(cols, call.device, call.n, 'columns')
    out = torch.empty(call.n, int(c.numel()), dtype=torch.float32, device=call.device)
    call('cols', nv.ptr(c), int(c.numel()), nv.ptr(out), stream=stream)
    return out


def pair_label_expsum(src, label, k, metric=None, stream=None):
    """W[u, g] = sum over i with label[i] == g of exp(-D[i, u]) [n, k] float64 on the device (ure_pair_label_expsum /
    ure_csr_pair_label_expsum)."""
    call = _PairCall(src, metric)
    n = call.n
    k = int(k)
    if not 1 <= k <= 128:
        raise ValueError(f'k must be in [1, 128], not {k}')
    lab = label.detach().cpu().numpy() if torch.is_tensor(label) else np.asarray(label)
    lab = lab.astype(np.int64).reshape(-1)
    if lab.shape != (n,) or lab.min() < 0 or lab.max() >= k:
        raise ValueError(f'label must be n = {n} values in [0, {k})')
    lab_d = to_device_async(lab.astype(np.int32), call.device)
    W = torch.empty(n, k, dtype=torch.float64, device=call.device)
    call('label_expsum', nv.ptr(lab_d), k, nv.ptr(W), stream=stream)
    return W


SINKHORN_MAX_K = 1024


def check_sinkhorn_args(reg, num_iter_max, stop_thr):
    """The entropic solver's settings, checked before any device work (ValueError)."""
    if isinstance(reg, bool) or not isinstance(reg, (int, float, np.floating, np.integer)) or not (np.isfinite(reg) and reg > 0):
        raise ValueError(f'reg must be a finite number > 0, not {reg!r}')
    if isinstance(num_iter_max, bool) or not isinstance(num_iter_max, (int, np.integer)) or not 1 <= num_iter_max < 2 ** 31:
        raise ValueError(f'num_iter_max must be an integer >= 1, not {num_iter_max!r}')
    if not isinstance(stop_thr, (int, float, np.floating, np.integer)) or not stop_thr >= 0:
        raise ValueError(f'stop_thr must be a number >= 0, not {stop_thr!r}')


def ot_sinkhorn(dist, reg=1e-3, num_iter_max=1000, stop_thr=1e-9, want_u=True, want_cost_min=False, stream=None):
    """Log-domain Sinkhorn (ure_ot_sinkhorn) on a device cost matrix dist [k, n] float32 (ure_ot_cost's layout), uniform
    marginals.  Returns a dict of device tensors label [n] int32, v [k] float64, u [n] float64 (want_u) and cost_min [n]
    float32 (want_cost_min), and the host values iters (int) and err (float)."""
    check_sinkhorn_args(reg, num_iter_max, stop_thr)
    if not torch.is_tensor(dist) or not dist.is_cuda:
        raise nv.NativeError('ot_sinkhorn runs on the HIP device only (no CPU fallback)')
    if dist.dim() != 2 or dist.dtype != torch.float32:
        raise ValueError(f'dist must be a [k, n] float32 tensor, not {tuple(dist.shape)} {dist.dtype}')
    k, n = int(dist.shape[0]), int(dist.shape[1])
    if not (1 <= k <= SINKHORN_MAX_K and 1 <= n < 2 ** 31):
        raise ValueError(f'need 1 <= k <= {SINKHORN_MAX_K} and 1 <= n < 2^31, not k = {k}, n = {n}')
    dist = dist.contiguous()
    L, dev = nv.lib(), dist.device
    nbytes = int(L.ure_ot_sinkhorn_scratch(n, k))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = {'label': torch.empty(n, dtype=torch.int32, device=dev), 'v': torch.empty(k, dtype=torch.float64, device=dev)}
    if want_u:
        out['u'] = torch.empty(n, dtype=torch.float64, device=dev)
    if want_cost_min:
        out['cost_min'] = torch.empty(n, dtype=torch.float32, device=dev)
    iters, err = ctypes.c_int32(), ctypes.c_double()
    nv.check(L.ure_ot_sinkhorn(nv.ptr(dist), n, k, float(reg), int(num_iter_max), float(stop_thr), nv.ptr(out.get('u')), nv.ptr(out['v']),
                               nv.ptr(out['label']), nv.ptr(out.get('cost_min')), nv.ptr(scratch), nbytes, ctypes.byref(iters),
                               ctypes.byref(err), nv.stream_handle(stream)), 'ure_ot_sinkhorn')
    out['iters'], out['err'] = int(iters.value), float(err.value)
    return out


# ---------------------------------------------------------------------------
# The learned shard combiner (csrc/mf_combine.hip; the host side of the fit is combine.py)
# ---------------------------------------------------------------------------
def _table_ptrs(tables, d, what):
    """(U pointers, V pointers, S) of a list of padded device (U, V) for one call of the combiner kernels."""
    S = len(tables)
    if not 1 <= S <= nv.MAX_MODELS_PER_CALL:
        raise ValueError(f'{what} takes 1 .. {nv.MAX_MODELS_PER_CALL} models, not {S}')
    for U, V in tables:
        if not (torch.is_tensor(U) and U.is_cuda and V.is_cuda):
            raise nv.NativeError(f'{what} runs on the HIP device only (no CPU fallback)')
        assert U.dtype == torch.float32 and V.dtype == torch.float32 and U.shape[0] == tables[0][0].shape[0] and V.shape[0] == tables[0][1].shape[0]
    return (*_ptr_arrays(tables, d), S)


def _link_code(link):
    from .combine import link_code
    if isinstance(link, (int, np.integer)) and not isinstance(link, bool) and int(link) in (0, 1):
        return int(link)
    return link_code(link)


class PairSet:
    """Training pairs (uid int32, iid int32, rating float32 = rating / 5) resident on the device: a fit uploads them once
    and makes every Newton pass over the same tensors."""

    def __init__(self, uid, iid, rating, device=None):
        uid = np.ascontiguousarray(uid, dtype=np.int32)
        iid = np.ascontiguousarray(iid, dtype=np.int32)
        rating = np.ascontiguousarray(rating, dtype=np.float32)
        if not len(uid) == len(iid) == len(rating):
            raise ValueError('uid, iid and rating differ in length')
        self.n = len(uid)
        if self.n and (uid.min() < 0 or iid.min() < 0):
            raise ValueError('negative user or item id')
        self.max_uid, self.max_iid = (int(uid.max()), int(iid.max())) if self.n else (-1, -1)
        self.device = device or _device()
        self.uid, self.iid, self.rating = upload_many([uid, iid, rating], self.device) if self.n else (None, None, None)

    @classmethod
    def from_device(cls, uid, iid, rating):
        """Pairs that are on the device already (int32, int32, float32 tensors); the id range is read back once."""
        ps = cls.__new__(cls)
        ps.uid, ps.iid, ps.rating = uid.contiguous(), iid.contiguous(), rating.contiguous()
        assert ps.uid.dtype == torch.int32 and ps.iid.dtype == torch.int32 and ps.rating.dtype == torch.float32
        ps.n, ps.device = int(uid.numel()), uid.device
        if not ps.n == ps.iid.numel() == ps.rating.numel():
            raise ValueError('uid, iid and rating differ in length')
        if ps.n and (int(ps.uid.min()) < 0 or int(ps.iid.min()) < 0):
            raise ValueError('negative user or item id')
        ps.max_uid, ps.max_iid = (int(ps.uid.max()), int(ps.iid.max())) if ps.n else (-1, -1)
        return ps


def combine_stats(tables, d, pairs, link, w, stream=None, as_tensor=False):
    """One pass of ure_combine_stats: the float64 stats vector (n, loss, g, upper triangle of H: combine.unpack_stats) of
    `pairs` (a PairSet, or a (uid, iid, rating) triple that is uploaded for this call) at the weights w (S + 1 float64, host
    or device) for the padded device tables [(U, V)].  Returns a numpy vector (synchronises), or the device tensor."""
    code = _link_code(link)
    Up, Vp, S = _table_ptrs(tables, d, 'combine_stats')
    if not isinstance(pairs, PairSet):
        pairs = PairSet(*pairs, device=tables[0][0].device)
    if pairs.n < 1:
        raise ValueError('combine_stats needs at least one pair')
    if pairs.max_uid >= tables[0][0].shape[0] or pairs.max_iid >= tables[0][1].shape[0]:
        raise ValueError(f'pair ids up to ({pairs.max_uid}, {pairs.max_iid}) outside the tables {tuple(tables[0][0].shape)}, {tuple(tables[0][1].shape)}')
    dev = pairs.device
    if not torch.is_tensor(w):
        w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    if w.dtype != torch.float64 or w.numel() != S + 1 or not w.is_cuda:
        raise ValueError(f'w must hold {S + 1} float64 values on the device')
    L = nv.lib()
    nbytes = int(L.ure_combine_stats_scratch(pairs.n, S))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    combine_stats.last_scratch_bytes = nbytes
    out = torch.empty(int(L.ure_combine_stats_len(S)), dtype=torch.float64, device=dev)
    nv.check(L.ure_combine_stats(Up, Vp, S, nv.ptr(pairs.uid), nv.ptr(pairs.iid), nv.ptr(pairs.rating), pairs.n, d, code, nv.ptr(w.contiguous()),
                                 nv.ptr(out), nv.ptr(scratch), nbytes, nv.stream_handle(stream)), 'ure_combine_stats')
    if as_tensor:
        return out
    if stream is not None:
        stream.synchronize()
    return out.cpu().numpy()


def score_weighted(tables, d, uid, iid, rating, link, W, group_of_user=None, pred=None, sse=None, stream=None):
    """ure_score_weighted on device pairs (uid, iid int32; rating float32, needed for sse): pred[j] = (float)link(b + sum_s
    w[s] p[j, s]) with the row W[group_of_user[uid[j]]] of W (device float64 [G, S + 1]; row 0 without a map), and the
    squared-error partials ure_eval_reduce takes.  -> (pred float32 [n], sse float64 [SCORE_PARTIALS]); nothing synchronises."""
    code = _link_code(link)
    Up, Vp, S = _table_ptrs(tables, d, 'score_weighted')
    dev = tables[0][0].device
    n = int(uid.numel())
    if n < 1:
        raise ValueError('score_weighted needs at least one pair')
    if not (torch.is_tensor(W) and W.is_cuda and W.dtype == torch.float64 and W.dim() == 2 and W.shape[1] == S + 1 and W.shape[0] >= 1):
        raise ValueError(f'W must be a device float64 [G, {S + 1}] tensor')
    for t, dt, name in ((uid, torch.int32, 'uid'), (iid, torch.int32, 'iid'), (rating, torch.float32, 'rating'), (group_of_user, torch.int32, 'group_of_user')):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise ValueError(f'{name} must be a contiguous device {dt} tensor')
    if iid.numel() != n or (rating is not None and rating.numel() != n):
        raise ValueError('uid, iid and rating differ in length')
    if group_of_user is not None and group_of_user.numel() < 1:
        raise ValueError('an empty group map')
    if pred is None:
        pred = torch.empty(n, dtype=torch.float32, device=dev)
    if sse is None and rating is not None:
        sse = torch.empty(SCORE_PARTIALS, dtype=torch.float64, device=dev)
    assert pred.dtype == torch.float32 and pred.numel() >= n and pred.is_contiguous()
    assert sse is None or (sse.dtype == torch.float64 and sse.numel() >= SCORE_PARTIALS and sse.is_contiguous())
    nv.check(nv.lib().ure_score_weighted(Up, Vp, S, nv.ptr(uid), nv.ptr(iid), nv.ptr(rating), n, d, code, nv.ptr(W.contiguous()), int(W.shape[0]),
                                         nv.ptr(group_of_user), int(group_of_user.numel()) if group_of_user is not None else 0,
                                         nv.ptr(pred), nv.ptr(sse), nv.stream_handle(stream)), 'ure_score_weighted')
    return pred, sse


# ---------------------------------------------------------------------------
# Batched ridge solves (csrc/mf_ridge.hip; the contract and the CSR builder are ridge.py)
# ---------------------------------------------------------------------------
class SegmentSet:
    """A CSR of rating entries grouped by segment, resident on the device: segment s (a user, or an item) holds the ids of
    the fixed table's rows it rated and the ratings / 5, in the order given (a stable sort on the host).  The counterpart of
    PairSet for ridge_rows; `order` lists the segments longest first."""

    def __init__(self, seg_ids, other_ids, rating, n_seg, device=None):
        from .ridge import segment_csr
        off, idx, val, order = segment_csr(seg_ids, other_ids, rating, n_seg)
        self.m, self.nnz = int(n_seg), len(idx)
        self.max_other = int(idx.max()) if self.nnz else -1
        self.counts = np.diff(off)
        self.device = device or _device()
        self.off, self.order = upload_many([off, order], self.device)
        # (a kernel argument must not be NULL: an empty set keeps one unused entry)
        self.idx, self.val = upload_many([idx if self.nnz else np.zeros(1, np.int32), val if self.nnz else np.zeros(1, np.float32)], self.device)

    @classmethod
    def from_device(cls, off, idx, val):
        """A CSR that is on the device already (int64 [m + 1], int32, float32 tensors); no `order`.  The offsets and the id
        range are read back once."""
        ss = cls.__new__(cls)
        assert off.dtype == torch.int64 and idx.dtype == torch.int32 and val.dtype == torch.float32
        host = off.cpu().numpy()
        ss.m, ss.nnz = len(host) - 1, int(idx.numel())
        if ss.m < 0 or host[0] != 0 or host[-1] != ss.nnz or (np.diff(host) < 0).any() or val.numel() != ss.nnz:
            raise ValueError('off must rise from 0 to the number of entries')
        if ss.nnz and int(idx.min()) < 0:
            raise ValueError('negative id')
        ss.max_other = int(idx.max()) if ss.nnz else -1
        ss.counts, ss.device, ss.order = np.diff(host), off.device, None
        ss.off = off.contiguous()
        ss.idx = idx.contiguous() if ss.nnz else torch.zeros(1, dtype=torch.int32, device=off.device)
        ss.val = val.contiguous() if ss.nnz else torch.zeros(1, dtype=torch.float32, device=off.device)
        return ss


def ridge_rows(F, d, k, segs, l2, l2_n=0.0, stream=None, order='longest'):
    """ure_ridge_rows: X [m, d] float32, row s the ridge solution of segment s of `segs` (a SegmentSet) against the first k
    columns of the fixed device table F [n_fixed, d] at strength l2 + l2_n * n_s; columns k .. d - 1 are zero.  order:
    'longest' (the set's own longest-first list), None (index order) or an int32 list of segments; it changes no byte.  Reads
    the status words back (synchronises) and raises ValueError naming l2 and the first failing segment when a system was not
    positive definite; the exception carries X (the failed rows NaN), `failed` and `segment`."""
    from .ridge import MAX_D, check_ridge_args
    l2, l2_n = check_ridge_args(l2, l2_n)
    if d > MAX_D:
        raise ValueError(f'ridge_rows serves padded widths up to {MAX_D}: the float64 triangle of width {d} does not fit in LDS')
    if not 1 <= k <= d or d != pad_dim(d):
        raise ValueError(f'need 1 <= k <= d with d a padded width, not k = {k}, d = {d}')
    if not (torch.is_tensor(F) and F.is_cuda):
        raise nv.NativeError('ridge_rows runs on the HIP device only (no CPU fallback)')
    if not (F.dtype == torch.float32 and F.dim() == 2 and F.shape[1] == d and F.is_contiguous() and F.shape[0] >= 1):
        raise ValueError(f'F must be a contiguous float32 [n, {d}] tensor')
    if segs.max_other >= F.shape[0]:
        raise ValueError(f'ids up to {segs.max_other} outside the fixed table of {F.shape[0]} rows')
    dev = F.device
    if isinstance(order, str):
        if order != 'longest':
            raise ValueError(f"order must be 'longest', None or a list of segments, not {order!r}")
        order = segs.order
    elif order is not None and not torch.is_tensor(order):
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.shape != (segs.m,) or (np.sort(order) != np.arange(segs.m)).any():
            raise ValueError('order must list every segment once')
        order = torch.from_numpy(order).to(dev)
    X = torch.empty(segs.m, d, dtype=torch.float32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    nv.check(nv.lib().ure_ridge_rows(nv.ptr(F), int(F.shape[0]), d, k, nv.ptr(segs.off), nv.ptr(segs.idx), nv.ptr(segs.val), segs.m, nv.ptr(order),
                                     l2, l2_n, nv.ptr(X), nv.ptr(status), None, 0, nv.stream_handle(stream)), 'ure_ridge_rows')
    if stream is not None:
        stream.synchronize()
    failed, first = (int(v) for v in status.cpu().numpy())
    if failed:
        err = ValueError(f'ridge_rows: {failed} of {segs.m} systems are not positive definite, first segment {first} '
                         f'({int(segs.counts[first])} entries, width {k}) at l2 = {l2:g}, l2_n = {l2_n:g}: a larger l2 makes them definite')
        err.X, err.failed, err.segment = X, failed, first
        raise err
    return X


# ---------------------------------------------------------------------------
# Weighted matrix factorisation for implicit feedback (csrc/wmf.hip, include/ultrare_wmf.h; the contract is wmf.py)
# ---------------------------------------------------------------------------
def _fixed_table(F, d, k, who):
    from .ridge import MAX_D
    if d > MAX_D:
        raise ValueError(f'{who} serves padded widths up to {MAX_D}: the float64 triangle of width {d} does not fit in LDS')
    if not 1 <= k <= d or d != pad_dim(d):
        raise ValueError(f'need 1 <= k <= d with d a padded width, not k = {k}, d = {d}')
    if not (torch.is_tensor(F) and F.is_cuda):
        raise nv.NativeError(f'{who} runs on the HIP device only (no CPU fallback)')
    if not (F.dtype == torch.float32 and F.dim() == 2 and F.shape[1] == d and F.is_contiguous() and F.shape[0] >= 1):
        raise ValueError(f'F must be a contiguous float32 [n, {d}] tensor')


def gram(F, d, k, stream=None):
    """ure_gram: the Gram matrix of the first k columns of the device table F [n, d] as the packed upper triangle, float64
    [k (k + 1) / 2] on the device -- wmf.gram_ref's bytes (a two-level chain: 256-row chunks, then the chunks in order), on any
    stream.  wmf.tri_unpack gives the square matrix.  Nothing is read back."""
    _fixed_table(F, d, k, 'gram')
    n = int(F.shape[0])
    need = int(nv.lib().ure_gram_scratch(n, k))
    if need < 0:
        raise ValueError(f'gram: n = {n}, k = {k} is refused')
    G0 = torch.empty(k * (k + 1) // 2, dtype=torch.float64, device=F.device)
    scratch = torch.empty(need, dtype=torch.uint8, device=F.device)
    nv.check(nv.lib().ure_gram(nv.ptr(F), n, d, k, nv.ptr(G0), nv.ptr(scratch), need, nv.stream_handle(stream)), 'ure_gram')
    if stream is not None:
        scratch.record_stream(stream)
    return G0


def confidence(val, alpha):
    """(wg, wb) float32 on the device of the float32 ratings `val` -- wmf.confidence_ref's bytes: wg = fl32(alpha32 * r),
    wb = fl32(1 + wg); two elementwise float32 operations, each rounded once."""
    a = torch.tensor(float(alpha), dtype=torch.float32, device=val.device)
    wg = torch.mul(val, a)
    return wg, torch.add(wg, torch.ones((), dtype=torch.float32, device=val.device))


def wridge_rows(F, d, k, segs, wg, wb, G0, l2, l2_n=0.0, stream=None, order='longest'):
    """ure_wridge_rows: ridge_rows with a confidence per entry and a Gram matrix added to every system.  X [m, d] float32, row s
    the solution of (G0 + sum_j wg_j f_j f_j^T + (l2 + l2_n n_s) I) x = sum_j wb_j f_j over segment s of `segs` (a SegmentSet; its
    ratings are not read) against the first k columns of the fixed device table F [n_fixed, d].  wg, wb: float32 device tensors
    [nnz] in the set's CSR order (confidence(segs.val, alpha)); G0: gram()'s packed triangle, or None for no added matrix.  order,
    the status read-back and the ValueError of a failed segment are ridge_rows's."""
    from .ridge import check_ridge_args
    l2, l2_n = check_ridge_args(l2, l2_n)
    _fixed_table(F, d, k, 'wridge_rows')
    if segs.max_other >= F.shape[0]:
        raise ValueError(f'ids up to {segs.max_other} outside the fixed table of {F.shape[0]} rows')
    dev = F.device
    for name, w in (('wg', wg), ('wb', wb)):
        if not (torch.is_tensor(w) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 1 and w.is_contiguous() and w.numel() == segs.nnz):
            raise ValueError(f'{name} must be a contiguous float32 device tensor of {segs.nnz} values, one per entry in CSR order')
    if segs.nnz == 0:                                       # (a kernel argument must not be NULL)
        wg = wb = torch.zeros(1, dtype=torch.float32, device=dev)
    if G0 is not None and not (torch.is_tensor(G0) and G0.is_cuda and G0.dtype == torch.float64 and G0.is_contiguous() and G0.numel() == k * (k + 1) // 2):
        raise ValueError(f'G0 must be a contiguous float64 device tensor of {k * (k + 1) // 2} values (the packed triangle of width {k}), or None')
    if isinstance(order, str):
        if order != 'longest':
            raise ValueError(f"order must be 'longest', None or a list of segments, not {order!r}")
        order = segs.order
    elif order is not None and not torch.is_tensor(order):
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.shape != (segs.m,) or (np.sort(order) != np.arange(segs.m)).any():
            raise ValueError('order must list every segment once')
        order = torch.from_numpy(order).to(dev)
    X = torch.empty(segs.m, d, dtype=torch.float32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    nv.check(nv.lib().ure_wridge_rows(nv.ptr(F), int(F.shape[0]), d, k, nv.ptr(segs.off), nv.ptr(segs.idx), nv.ptr(wg), nv.ptr(wb), segs.m,
                                      nv.ptr(order), nv.ptr(G0), l2, l2_n, nv.ptr(X), nv.ptr(status), None, 0, nv.stream_handle(stream)),
             'ure_wridge_rows')
    if stream is not None:
        stream.synchronize()
    failed, first = (int(v) for v in status.cpu().numpy())
    if failed:
        err = ValueError(f'wridge_rows: {failed} of {segs.m} systems are not positive definite, first segment {first} '
                         f'({int(segs.counts[first])} entries, width {k}) at l2 = {l2:g}, l2_n = {l2_n:g}: a larger l2 makes them definite')
        err.X, err.failed, err.segment = X, failed, first
        raise err
    return X


# ---------------------------------------------------------------------------
# OT grouping on the sparse rating matrix (csrc/csr_group.hip; the contract is sparse_group.py)
# ---------------------------------------------------------------------------
class CsrSet:
    """The canonical CSR and CSC of a SciPy sparse matrix (sparse_group.canonical_csr) resident on the device, uploaded once
    per clustering call: the cost kernel walks the rows, the centroid kernel the columns.  n rows (users), n_item columns."""

    def __init__(self, sp_mat, device=None):
        from .sparse_group import canonical_csr
        self.csr, self.csc = canonical_csr(sp_mat)                # (raises ValueError before any device work)
        self.n, self.n_item = self.csr.shape
        self.nnz = self.csr.nnz
        self.device = device or _device()
        # (a kernel argument must not be NULL: an empty matrix keeps one unused entry)
        pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)
        # (plain copies: the pinned staging pool of upload_many is for small descriptors, these are 12 bytes per rating, twice)
        (self.row_off, self.col, self.val, self.col_off, self.row, self.cval) = [
            torch.from_numpy(a).to(self.device)
            for a in (self.csr.off, pad(self.csr.idx), pad(self.csr.val), self.csc.off, pad(self.csc.idx), pad(self.csc.val))]

    @classmethod
    def from_device(cls, n, n_item, row_off=None, col=None, val=None, col_off=None, row=None, cval=None):
        """Halves that are on the device already (int64 offsets, int32 indices, float32 values, at least one entry; the caller
        vouches for the index ranges), n rows by n_item columns; no host copy.  A half that is not given stays None."""
        S = cls.__new__(cls)
        halves = (row_off, col, val, col_off, row, cval)
        for half in (halves[:3], halves[3:]):
            if any(t is not None for t in half) and [getattr(t, 'dtype', None) for t in half] != [torch.int64, torch.int32, torch.float32]:
                raise ValueError('a CSR half is (int64 offsets, int32 indices, float32 values) tensors, all three')
        if row_off is None and col_off is None:
            raise ValueError('neither the CSR nor the CSC half is given')
        S.csr = S.csc = None
        S.n, S.n_item, S.nnz = int(n), int(n_item), int((cval if val is None else val).numel())
        S.device = (col_off if row_off is None else row_off).device
        S.row_off, S.col, S.val, S.col_off, S.row, S.cval = (None if t is None else t.contiguous() for t in halves)
        return S


def _csr_same_device(off, t, what):
    if t.device != off.device:
        raise ValueError(f'{what} is on {t.device} but the CsrSet was uploaded to {off.device}')


def _csr_has(S, half):
    if getattr(S, 'row_off' if half == 'CSR' else 'col_off') is None:
        raise ValueError(f'this CsrSet was made without the {half} half')


def _csr_held_for(stream, *tensors):
    """Tensors allocated here for a launch on a stream that is not torch's current one: the caching allocator may hand a block out
    again only after that stream's work."""
    if stream is not None:
        for t in tensors:
            t.record_stream(stream)


def _csr_k(k):
    from .sparse_group import MAX_K
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError(f'k must be an integer in 1 .. {MAX_K}, not {k!r}')
    return int(k)


def _csr_label(S, label, k, who):
    """label (n values in [0, k): a host array, or a device int32 tensor whose range is read back once) as a checked device
    int32 tensor."""
    if torch.is_tensor(label):
        if not label.is_cuda:
            raise nv.NativeError(f'{who} runs on the HIP device only (no CPU fallback)')
        if label.dtype != torch.int32 or label.shape != (S.n,) or int(label.min()) < 0 or int(label.max()) >= k:
            raise ValueError(f'label must be n = {S.n} int32 values in [0, {k})')
        _csr_has(S, 'CSC')
        _csr_same_device(S.col_off, label, 'label')
        return label.contiguous()
    lab = np.ascontiguousarray(label)
    if lab.shape != (S.n,) or lab.min() < 0 or lab.max() >= k:
        raise ValueError(f'label must be n = {S.n} values in [0, {k})')
    _csr_has(S, 'CSC')
    return to_device_async(lab.astype(np.int32), S.device)


def _csr_cost_call(entry, S, Ct, k, exact, dist_shape, stream):
    """Check Ct [n_item, >= k] (exact: [n_item, k]), size the scratch by `entry`_scratch, allocate dist and call `entry`
    (ure_csr_cost's argument list; without the stride when exact)."""
    if not (torch.is_tensor(Ct) and Ct.is_cuda):
        raise nv.NativeError(f'{entry[4:]} runs on the HIP device only (no CPU fallback)')
    if not (Ct.dtype == torch.float32 and Ct.dim() == 2 and Ct.is_contiguous() and Ct.shape[0] == S.n_item
            and (Ct.shape[1] == k if exact else Ct.shape[1] >= k)):
        raise ValueError(f"Ct must be a contiguous float32 [{S.n_item}, {'' if exact else '>= '}{k}] tensor, not {tuple(Ct.shape)} {Ct.dtype}")
    _csr_has(S, 'CSR')
    _csr_same_device(S.row_off, Ct, 'Ct')
    L, dev = nv.lib(), Ct.device
    nbytes = int(getattr(L, entry + '_scratch')(k))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dist = torch.empty(*dist_shape, dtype=torch.float32, device=dev)
    stride = () if exact else (int(Ct.shape[1]),)
    nv.check(getattr(L, entry)(nv.ptr(S.row_off), nv.ptr(S.col), nv.ptr(S.val), S.n, S.n_item, nv.ptr(Ct), *stride, k, nv.ptr(dist),
                               nv.ptr(scratch), nbytes, nv.stream_handle(stream)), entry)
    _csr_held_for(stream, scratch, dist)
    return dist


def csr_cost(S, Ct, k, stream=None):
    """ure_csr_cost: dist [k, n] float32 on the device (ure_ot_cost's layout) of the rows of S (a CsrSet) against the k
    centroids held transposed in the device tensor Ct [n_item, ldc] float32, ldc >= k.  Nothing synchronises."""
    k = _csr_k(k)
    return _csr_cost_call('ure_csr_cost', S, Ct, k, False, (k, S.n), stream)


def csr_centroids(S, label, k, ldc=None, stream=None):
    """ure_csr_centroids: (Ct [n_item, ldc] float32, counts [k] int32) on the device, the means of the users of every cluster
    of label (n values in [0, k): a host array, or a device int32 tensor whose range is read back once), transposed as
    csr_cost reads them.  ldc (default k) >= k; the padding columns are zero.  A cluster without members gives zeros and
    counts 0.  Nothing synchronises after the launch."""
    k = _csr_k(k)
    ldc = k if ldc is None else int(ldc)
    if ldc < k:
        raise ValueError(f'ldc = {ldc} < k = {k}')
    lab_d = _csr_label(S, label, k, 'csr_centroids')
    dev = lab_d.device
    Ct = (torch.empty if ldc == k else torch.zeros)(S.n_item, ldc, dtype=torch.float32, device=dev)
    counts = torch.empty(k, dtype=torch.int32, device=dev)
    nv.check(nv.lib().ure_csr_centroids(nv.ptr(S.col_off), nv.ptr(S.row), nv.ptr(S.cval), nv.ptr(lab_d), S.n, S.n_item, k, nv.ptr(Ct), ldc,
                                        nv.ptr(counts), nv.stream_handle(stream)), 'ure_csr_centroids')
    _csr_held_for(stream, lab_d, Ct, counts)
    return Ct, counts


# ---------------------------------------------------------------------------
# k-means / balanced k-means on the sparse rating matrix (csrc/csr_kmeans.hip; the contract is sparse_kmeans.py)
# ---------------------------------------------------------------------------
def csr_kmeans_cost(S, Ct, k, stream=None):
    """ure_csr_kmeans_cost: dist [n, k] float32 on the device (ure_kmeans_cost's layout) of the rows of S (a CsrSet) against
    the k centroids held transposed in the device tensor Ct [n_item, k] float32.  Nothing synchronises."""
    k = _csr_k(k)
    return _csr_cost_call('ure_csr_kmeans_cost', S, Ct, k, True, (S.n, k), stream)


def csr_kmeans_centroids(S, label, k, stream=None):
    """ure_csr_kmeans_centroids: (Ct [n_item, k] float32, counts [k] int32) on the device, scipy's sparse mean of the users of
    every cluster of label (n values in [0, k): a host array, or a device int32 tensor whose range is read back once),
    transposed as csr_kmeans_cost reads them.  A cluster without members gives zeros and counts 0.  Nothing synchronises
    after the launch."""
    k = _csr_k(k)
    lab_d = _csr_label(S, label, k, 'csr_kmeans_centroids')
    dev = lab_d.device
    Ct = torch.empty(S.n_item, k, dtype=torch.float32, device=dev)
    counts = torch.empty(k, dtype=torch.int32, device=dev)
    nv.check(nv.lib().ure_csr_kmeans_centroids(nv.ptr(S.col_off), nv.ptr(S.row), nv.ptr(S.cval), S.n_item, S.n, nv.ptr(lab_d), k, nv.ptr(Ct),
                                               nv.ptr(counts), nv.stream_handle(stream)), 'ure_csr_kmeans_centroids')
    _csr_held_for(stream, lab_d, Ct, counts)
    return Ct, counts


def balanced_fill(dist_d, capacity, stream=None):
    """ure_balanced_fill: (label int32 [n] on the device, rounds) from the device matrix dist_d [n, k] float32 --
    ure_host_kmeans_assign's labels without the copy, the sort and the walk.  capacity <= 0: the argmin (first minimum, the
    first NaN wins), rounds = 1.  capacity > 0: the balanced fill; the host reads a 4-byte flag once per round, so the call
    synchronises the stream `rounds` times."""
    if not (torch.is_tensor(dist_d) and dist_d.is_cuda):
        raise nv.NativeError('balanced_fill runs on the HIP device only (no CPU fallback)')
    if not (dist_d.dtype == torch.float32 and dist_d.dim() == 2 and dist_d.is_contiguous() and dist_d.numel() > 0):
        raise ValueError(f'dist must be a contiguous float32 [n, k] tensor, not {tuple(dist_d.shape)} {dist_d.dtype}')
    n, k = (int(v) for v in dist_d.shape)
    k = _csr_k(k)
    capacity = int(capacity)
    if n * k >= 2 ** 32:
        raise ValueError(f'n * k = {n} * {k} must stay below 2^32')
    if capacity > 0 and min(capacity, n) * k < n:
        raise ValueError(f'capacity {capacity} x {k} groups < {n} users')
    L, dev = nv.lib(), dist_d.device
    nbytes = int(L.ure_balanced_fill_scratch(n, k)) if capacity > 0 else 0
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    label = torch.empty(n, dtype=torch.int32, device=dev)
    rounds = ctypes.c_int64(0)
    nv.check(L.ure_balanced_fill(nv.ptr(dist_d), n, k, capacity, nv.ptr(label), ctypes.byref(rounds), nv.ptr(scratch), nbytes,
                                 nv.stream_handle(stream)), 'ure_balanced_fill')
    _csr_held_for(stream, scratch, label)
    return label, int(rounds.value)


# ---------------------------------------------------------------------------
# Attribute unlearning losses (csrc/mmd.hip; the contract and the argument checks are attr_unlearn.py)
# ---------------------------------------------------------------------------
class GroupRows:
    """The selected rows of two attribute groups on the device: rows int32 [n1 + n2], the first n1 the source group.
    Checked once on the host (attr_unlearn.check_groups) so that the calls of a fine-tune loop read nothing back."""

    def __init__(self, id1, id2, n_rows, device=None):
        from .attr_unlearn import check_groups
        self.host, self.n1, self.n2 = check_groups(id1, id2, n_rows)
        self.n_rows = int(n_rows)
        self.rows = to_device_async(self.host, device or _device())

    @classmethod
    def checked(cls, rows, n1, n2, n_rows, device):
        """From what attr_unlearn.check_groups returned already (rows int32 [n1 + n2]): nothing is checked again."""
        g = cls.__new__(cls)
        g.host, g.n1, g.n2, g.n_rows = rows, int(n1), int(n2), int(n_rows)
        g.rows = to_device_async(rows, device or _device())
        return g

    @classmethod
    def leading(cls, n1, n2, device):
        """Rows 0 .. n1 + n2 - 1 of a table that holds the source rows and then the target rows."""
        g = cls.__new__(cls)
        if n1 < 1 or n2 < 1:
            raise ValueError(f'both groups need at least one row, not {n1} and {n2}')
        g.host, g.n1, g.n2, g.n_rows = None, int(n1), int(n2), int(n1 + n2)
        g.rows = torch.arange(n1 + n2, dtype=torch.int32, device=device)
        return g

    @property
    def m(self):
        return self.n1 + self.n2


def _attr_table(X, groups, what):
    """(d, ld) of a device table the attribute kernels may read in place."""
    from .attr_unlearn import check_width
    if not (torch.is_tensor(X) and X.is_cuda):
        raise nv.NativeError(f'{what} runs on the HIP device only (no CPU fallback)')
    if not (X.dtype == torch.float32 and X.dim() == 2 and X.stride(1) == 1 and X.shape[0] >= groups.n_rows and X.stride(0) >= X.shape[1]):
        raise ValueError(f'{what}: X must be a float32 [>= {groups.n_rows}, d] device tensor with unit column stride, not {tuple(X.shape)} {X.dtype}')
    if X.device != groups.rows.device:
        raise ValueError(f'X is on {X.device} but the rows were uploaded to {groups.rows.device}')
    return check_width(X.shape[1], X.stride(0)), int(X.stride(0))


def _attr_scratch(m, d, dev, stream):
    nbytes = int(nv.lib().ure_mmd_scratch(m, d))
    if nbytes < 0:
        raise ValueError(f'ure_mmd_scratch refused m = {m}, d = {d}')
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _csr_held_for(stream, scratch)
    return scratch, nbytes


def mmd_bandwidth(X, groups, fix_sigma=None, check=False, stream=None):
    """The bandwidth of the selected rows as a 0-d float64 device tensor (ure_mmd_bandwidth), or fix_sigma put there.
    check: read it back and raise ValueError when it is not positive and finite (synchronises)."""
    d, ld = _attr_table(X, groups, 'mmd_bandwidth')
    if fix_sigma is not None:
        bw = torch.full((), float(fix_sigma), dtype=torch.float64, device=X.device)
    else:
        bw = torch.empty((), dtype=torch.float64, device=X.device)
        scratch, nbytes = _attr_scratch(groups.m, d, X.device, stream)
        nv.check(nv.lib().ure_mmd_bandwidth(X.data_ptr(), ld, d, nv.ptr(groups.rows), groups.n1, groups.n2, bw.data_ptr(), nv.ptr(scratch), nbytes,
                                            nv.stream_handle(stream)), 'ure_mmd_bandwidth')
    _csr_held_for(stream, bw)
    if check:
        from .attr_unlearn import check_bandwidth
        if stream is not None:
            stream.synchronize()
        check_bandwidth(float(bw.cpu()))
    return bw


def mmd_loss_grad(X, groups, bandwidth, kernel_mul=2.0, kernel_num=5, want_grad=True, stream=None):
    """ure_mmd_loss_grad on the selected rows of the device table X, read in place: (sums float64 [4] = the sums of the kernel
    matrix over S x S, T x T, S x T, T x S; grad float32 [m, d] or None), on the device.  bandwidth: the 0-d float64 device
    tensor of mmd_bandwidth.  Nothing synchronises."""
    from .attr_unlearn import check_mmd_args
    kernel_mul, kernel_num, _ = check_mmd_args(kernel_mul, kernel_num)
    d, ld = _attr_table(X, groups, 'mmd_loss_grad')
    if not (torch.is_tensor(bandwidth) and bandwidth.is_cuda and bandwidth.dtype == torch.float64 and bandwidth.numel() == 1):
        raise ValueError('bandwidth must be a float64 device tensor of one value (mmd_bandwidth)')
    dev = X.device
    scratch, nbytes = _attr_scratch(groups.m, d, dev, stream)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    grad = torch.empty(groups.m, d, dtype=torch.float32, device=dev) if want_grad else None
    nv.check(nv.lib().ure_mmd_loss_grad(X.data_ptr(), ld, d, nv.ptr(groups.rows), groups.n1, groups.n2, kernel_mul, kernel_num, bandwidth.data_ptr(),
                                        nv.ptr(sums), nv.ptr(grad), nv.ptr(scratch), nbytes, nv.stream_handle(stream)), 'ure_mmd_loss_grad')
    _csr_held_for(stream, sums, *([grad] if want_grad else []))
    return sums, grad


def mmd_loss_of(sums, groups):
    """The MMD loss (0-d float64 device tensor) from the four block sums."""
    n1, n2 = float(groups.n1), float(groups.n2)
    return sums[0] / (n1 * n1) + sums[1] / (n2 * n2) - sums[2] / (n1 * n2) - sums[3] / (n1 * n2)


def u2u_loss_grad(X, groups, want_grad=True, stream=None):
    """ure_u2u_loss_grad: (value 0-d float64, grad float32 [m, d] or None) on the device.  Nothing synchronises."""
    d, ld = _attr_table(X, groups, 'u2u_loss_grad')
    dev = X.device
    scratch, nbytes = _attr_scratch(groups.m, d, dev, stream)
    value = torch.empty((), dtype=torch.float64, device=dev)
    grad = torch.empty(groups.m, d, dtype=torch.float32, device=dev) if want_grad else None
    nv.check(nv.lib().ure_u2u_loss_grad(X.data_ptr(), ld, d, nv.ptr(groups.rows), groups.n1, groups.n2, value.data_ptr(), nv.ptr(grad),
                                        nv.ptr(scratch), nbytes, nv.stream_handle(stream)), 'ure_u2u_loss_grad')
    _csr_held_for(stream, value, *([grad] if want_grad else []))
    return value, grad


def mmd_matrix(X, groups, bandwidth, kernel_mul=2.0, kernel_num=5, stream=None):
    """ure_mmd_matrix: the kernel matrix K [m, m] float32 of the selected rows on the device, m <= 8192."""
    from .attr_unlearn import RBK_MAX_M, check_mmd_args
    kernel_mul, kernel_num, _ = check_mmd_args(kernel_mul, kernel_num)
    d, ld = _attr_table(X, groups, 'mmd_matrix')
    if groups.m > RBK_MAX_M:
        raise ValueError(f'the kernel matrix of {groups.m} rows is not formed (limit {RBK_MAX_M}): mmd_loss streams it')
    K = torch.empty(groups.m, groups.m, dtype=torch.float32, device=X.device)
    nv.check(nv.lib().ure_mmd_matrix(X.data_ptr(), ld, d, nv.ptr(groups.rows), groups.m, kernel_mul, kernel_num, bandwidth.data_ptr(), nv.ptr(K),
                                     nv.stream_handle(stream)), 'ure_mmd_matrix')
    _csr_held_for(stream, K)
    return K


# ---------------------------------------------------------------------------
# The attribute-inference attacker (csrc/attack.hip, include/ultrare_attack.h; the contract and the argument checks are attack.py)
# ---------------------------------------------------------------------------
class AttackFit:
    """A cross-validated probe on the device: params float32 [folds, P], stats float32 [folds, 2, d], fold_of int32 [m], scores
    float32 [m] (out of fold, by position of groups.rows), loss float64 [folds, epochs]; fold_host is fold_of on the host."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _attack_stream(stream):
    """Uploads go on torch's current stream: a launch stream of the caller's waits for them."""
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())


def attack_fit(X, groups, hidden=100, folds=5, epochs=None, lr=None, l2=1e-4, seed=0, stream=None, params0=None, fold_of=None):
    """Fit the probe of attack.py on the rows of `groups` (class 1 = the first group) of the device table X, read in place:
    ure_attack_standardize, ure_attack_train and ure_attack_score, back to back on one stream -> AttackFit.  The fold plan and the
    initial parameters come from attack.fold_plan / attack.init_params under `seed` (params0, fold_of: given ones, for tests).
    Nothing is read back and nothing synchronises."""
    run = _ProbeRun(X, groups, hidden, folds, epochs, lr, l2, seed, params0, fold_of, stream, 'attack_fit')
    dev, m = X.device, groups.m
    stats = torch.empty(run.folds, 2, run.d, dtype=torch.float32, device=dev)
    params = torch.empty(run.folds, run.P, dtype=torch.float32, device=dev)
    loss = torch.empty(run.folds, run.epochs, dtype=torch.float64, device=dev)
    scores = torch.empty(m, dtype=torch.float32, device=dev)
    run.standardize(X, stats)
    run.train(X, stats, run.p0, params, loss)
    nv.check(nv.lib().ure_attack_score(X.data_ptr(), run.ld, run.d, nv.ptr(groups.rows), nv.ptr(run.fold_of), m, run.folds, run.H, nv.ptr(stats),
                                       nv.ptr(params), nv.ptr(scores), run.st), 'ure_attack_score')
    _csr_held_for(stream, stats, params, loss, scores)
    return AttackFit(params=params, stats=stats, fold_of=run.fold_of, fold_host=run.fold_host, scores=scores, loss=loss, d=run.d, hidden=run.H,
                     folds=run.folds, epochs=run.epochs, lr=run.lr, l2=run.l2, seed=seed, n1=groups.n1, n2=groups.n2, fw=run.fw)


class _ProbeRun:
    """What every launch of a probe on fixed groups, folds and settings shares, checked and uploaded once: the fold plan, the initial
    parameters, the folds' class weights, Adam's scalars and ure_attack_train's scratch.  attack_fit runs it once, the round loop of
    adversarial_unlearn once per round."""

    def __init__(self, X, groups, hidden, folds, epochs, lr, l2, seed, params0, fold_of, stream, what):
        from . import adam, attack as A
        from .adv_unlearn import fold_weights
        self.d, self.ld = _attr_table(X, groups, what)
        self.groups, self.stream = groups, stream
        n1, n2, m, d = groups.n1, groups.n2, groups.m, self.d
        self.H, self.folds, self.epochs, self.lr, self.l2 = A.check_settings(d, n1, n2, hidden, folds, epochs, lr, l2)
        self.P = A.n_params(d, self.H)
        self.fold_host = A.fold_plan(n1, n2, self.folds, seed) if fold_of is None else np.ascontiguousarray(fold_of, dtype=np.int32)
        p0 = A.init_params(d, self.H, self.folds, seed) if params0 is None else np.ascontiguousarray(params0, dtype=np.float32)
        if self.fold_host.shape != (m,) or p0.shape != (self.folds, self.P):
            raise ValueError(f'fold_of must have shape ({m},) and params0 ({self.folds}, {self.P}), not {self.fold_host.shape} and {p0.shape}')
        fw = fold_weights(n1, self.fold_host, self.folds)
        if not np.isfinite(fw).all():
            raise ValueError('a fold trains on one class only: the fold plan must leave both classes in every training part')
        self.betas = adam.betas32(A.BETAS, A.EPS)
        dev = X.device
        self.nbytes = int(nv.lib().ure_attack_scratch(m, d, self.H, self.folds))
        if self.nbytes < 0:
            raise ValueError(f'ure_attack_scratch refused m = {m}, d = {d}, H = {self.H}, folds = {self.folds}')
        self.fold_of, self.p0, self.fw, self.sc = (to_device_async(a, dev) for a in (self.fold_host, p0, fw, A.scalars(self.epochs, self.lr)))
        _attack_stream(stream)
        self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.st = nv.stream_handle(stream)
        # (the caller's table and rows too: freed or rebound right after an asynchronous call, their blocks must not be handed out
        # again -- a small upload can land inside a freed table -- while the launch stream still reads them)
        _csr_held_for(stream, X, groups.rows, self.fold_of, self.p0, self.fw, self.sc, self.scratch)

    def standardize(self, X, stats):
        g = self.groups
        nv.check(nv.lib().ure_attack_standardize(X.data_ptr(), self.ld, self.d, nv.ptr(g.rows), nv.ptr(self.fold_of), g.m, self.folds, nv.ptr(stats),
                                                 self.st), 'ure_attack_standardize')

    def train(self, X, stats, p_in, p_out, loss):
        """`epochs` epochs from p_in into p_out (the same tensor will do), the losses into loss [folds, epochs]."""
        g = self.groups
        b1, b2, eps = self.betas
        nv.check(nv.lib().ure_attack_train(X.data_ptr(), self.ld, self.d, nv.ptr(g.rows), nv.ptr(self.fold_of), g.m, g.n1, self.folds, self.H,
                                           nv.ptr(stats), nv.ptr(self.fw), nv.ptr(self.sc), self.epochs, b1, b2, eps, float(np.float32(self.l2)),
                                           nv.ptr(p_in), nv.ptr(p_out), nv.ptr(loss), nv.ptr(self.scratch), self.nbytes, self.st), 'ure_attack_train')


def _adv_plan(fit, dev):
    """The fold groups of ure_adv_input_grad for a fit (adv_unlearn.fold_groups), made once and kept on it: from fold_host where the
    fit has one, else on the device from fold_of (a stable sort and counts on torch's current stream; nothing is read back)."""
    plan = getattr(fit, 'adv_plan', None)
    if plan is None:
        host = getattr(fit, 'fold_host', None)
        if host is not None:
            from .adv_unlearn import fold_groups
            perm, off = fold_groups(host, fit.folds)
            plan = (to_device_async(perm, dev), to_device_async(off, dev))
        else:
            fo = fit.fold_of.long()
            key = torch.where((fo >= 0) & (fo < fit.folds), fo, torch.full_like(fo, fit.folds))
            sizes = (key[:, None] == torch.arange(fit.folds + 1, device=dev)[None, :]).sum(0)         # (no bincount: it reads its size back)
            off = torch.zeros(fit.folds + 2, dtype=torch.int32, device=dev)
            off[1:] = torch.cumsum(sizes, 0)
            plan = (torch.argsort(key, stable=True).to(torch.int32), off)
        try:
            fit.adv_plan = plan
        except AttributeError:
            pass
    return plan


def _adv_target(target):
    t = np.asarray(target, dtype=np.float64).reshape(-1)
    if t.shape != (2,) or not np.isfinite(t).all():
        raise ValueError(f'target must be two finite numbers (the target p of class 0 and of class 1), not {target!r}')
    return float(np.float32(t[0])), float(np.float32(t[1]))


def attack_input_grad(fit, X, groups, target=(0.5, 0.5), want_p=True, stream=None):
    """ure_adv_input_grad: the gradient of every selected row's own term of the probe's loss with respect to the row, under the
    parameter set that held the row out -> (grad float32 [m, d], p float32 [m] or None) on the device.  fit: an AttackFit, or
    anything with its params, stats, fold_of (None: set 0 serves every row), fw, d, hidden and folds.  target = the p wanted of class
    0 and of class 1: (0, 1) is the attacker's own loss, (0.5, 0.5) the confusion target.  The contract is
    adv_unlearn.input_grad_ref.  Nothing is read back and nothing synchronises."""
    d, ld = _attr_table(X, groups, 'attack_input_grad')
    t0, t1 = _adv_target(target)
    P = fit.params.shape[-1]
    if d != fit.d or tuple(fit.params.shape) != (fit.folds, P) or tuple(fit.stats.shape) != (fit.folds, 2, d) or tuple(fit.fw.shape) != (fit.folds, 4):
        raise ValueError(f'attack_input_grad: the fit is of width {fit.d} with params {tuple(fit.params.shape)}, the table of width {d}')
    if fit.fold_of is not None and tuple(fit.fold_of.shape) != (groups.m,):
        raise ValueError(f'attack_input_grad: the fit holds {tuple(fit.fold_of.shape)} positions, the groups {groups.m}')
    dev, m = X.device, groups.m
    perm, off = _adv_plan(fit, dev) if fit.fold_of is not None else (None, None)
    _attack_stream(stream)
    grad = torch.empty(m, d, dtype=torch.float32, device=dev)
    p = torch.empty(m, dtype=torch.float32, device=dev) if want_p else None
    nv.check(nv.lib().ure_adv_input_grad(X.data_ptr(), ld, d, nv.ptr(groups.rows), nv.ptr(fit.fold_of), m, groups.n1, fit.folds, fit.hidden,
                                         nv.ptr(fit.stats), nv.ptr(fit.params), nv.ptr(fit.fw), t0, t1, nv.ptr(grad), nv.ptr(p), nv.ptr(perm),
                                         nv.ptr(off), nv.stream_handle(stream)), 'ure_adv_input_grad')
    _csr_held_for(stream, X, groups.rows, fit.params, fit.stats, fit.fw, grad, *([p] if want_p else []), *([] if perm is None else [fit.fold_of, perm, off]))
    return grad, p


def unlearn_row_step(X, at, start, grad, lr, eta, alpha):
    """x <- float32(x - lr (eta g + 2 alpha (x - x*))) on the rows `at` (int64) of the device table X, in place; x* = `start` (float64
    [m, d]), g = `grad` (float32 [m, d], left as it is).  The contract's float64 operations one by one, rounded once, written in place (four float64 [m, d] at the
    peak) -> (the new rows, float32; a float64 [m, d] buffer the caller may reuse).  utils.attribute_unlearn's step and the round of
    adversarial_unlearn."""
    cur = X.index_select(0, at).double()
    step = grad.double().mul_(eta)
    step.add_((cur - start).mul_(2.0 * alpha)).mul_(lr)
    new = cur.sub_(step).float()
    X.index_copy_(0, at, new)
    return new, step


def adversarial_unlearn(X, groups, hidden=32, folds=5, rounds=100, disc_epochs=5, disc_lr=1e-2, l2=1e-4, lr=0.1, eta=1.0, alpha=0.0,
                        target=(0.5, 0.5), seed=0, stream=None, params0=None, fold_of=None):
    """The round loop of adv_unlearn.adversarial_unlearn_ref on the rows of `groups` of the device table X, IN PLACE: per round
    ure_attack_standardize, ure_attack_train from the last round's parameters (disc_epochs epochs), ure_adv_input_grad, ure_auc_counts
    on its p, and the elementwise update, back to back on one stream.  Nothing is read back: -> AttackFit of the last round
    (params, stats, fold_of, fold_host, fw, scores = the last p) with the log on the device: loss float64 [rounds, folds, disc_epochs],
    counts int64 [rounds, 2] = (gt, eq), nan_flags int32 [rounds], reg float64 [rounds] (sum |x - x*|^2 after the round's update)."""
    from .adv_unlearn import check_loop
    rounds, disc_epochs, disc_lr, l2, lr, eta, alpha, _ = check_loop(rounds, disc_epochs, disc_lr, l2, lr, eta, alpha)
    t0, t1 = _adv_target(target)
    run = _ProbeRun(X, groups, hidden, folds, disc_epochs, disc_lr, l2, seed, params0, fold_of, stream, 'adversarial_unlearn')
    dev, m, n1, n2, L = X.device, groups.m, groups.n1, groups.n2, nv.lib()
    fit = AttackFit(params=run.p0.clone(), stats=torch.empty(run.folds, 2, run.d, dtype=torch.float32, device=dev), fold_of=run.fold_of,
                    fold_host=run.fold_host, fw=run.fw, d=run.d, hidden=run.H, folds=run.folds, epochs=disc_epochs, lr=disc_lr, l2=l2, seed=seed,
                    n1=n1, n2=n2)
    perm, off = _adv_plan(fit, dev)
    pos, neg = torch.arange(n1, dtype=torch.int32, device=dev), torch.arange(n1, m, dtype=torch.int32, device=dev)
    auc_bytes = int(L.ure_auc_scratch(n1, n2))
    auc_ws = torch.empty(auc_bytes, dtype=torch.uint8, device=dev)
    loss = torch.empty(rounds, run.folds, disc_epochs, dtype=torch.float64, device=dev)
    counts = torch.empty(rounds, 2, dtype=torch.int64, device=dev)
    flags = torch.empty(rounds, dtype=torch.int32, device=dev)
    reg = torch.empty(rounds, dtype=torch.float64, device=dev)
    grad = torch.empty(m, run.d, dtype=torch.float32, device=dev)
    p = torch.empty(m, dtype=torch.float32, device=dev)
    at = groups.rows.long()                 # (before the launch stream's wait below, and held for it: every round reads it there)
    _attack_stream(stream)
    _csr_held_for(stream, fit.params, fit.stats, perm, off, pos, neg, auc_ws, loss, counts, flags, reg, grad, p, at)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        start = X.index_select(0, at).double()
        for t in range(rounds):
            run.standardize(X, fit.stats)
            run.train(X, fit.stats, fit.params, fit.params, loss[t])
            nv.check(L.ure_adv_input_grad(X.data_ptr(), run.ld, run.d, nv.ptr(groups.rows), nv.ptr(run.fold_of), m, n1, run.folds, run.H,
                                          nv.ptr(fit.stats), nv.ptr(fit.params), nv.ptr(run.fw), t0, t1, nv.ptr(grad), nv.ptr(p), nv.ptr(perm),
                                          nv.ptr(off), run.st), 'ure_adv_input_grad')
            nv.check(L.ure_auc_counts(nv.ptr(p), nv.ptr(pos), n1, nv.ptr(neg), n2, counts[t].data_ptr(), flags[t].data_ptr(), nv.ptr(auc_ws), auc_bytes,
                                      run.st), 'ure_auc_counts')
            new, spare = unlearn_row_step(X, at, start, grad, lr, eta, alpha)
            delta = torch.sub(new, start, out=spare)
            reg[t] = delta.mul_(delta).sum()
    fit.scores, fit.loss, fit.counts, fit.nan_flags, fit.reg, fit.grad = p, loss, counts, flags, reg, grad
    return fit


def _index_list(idx, n, dev, name):
    """An index list into n scores as an int32 device tensor; every entry is checked to lie in [0, n) (a device tensor: on the
    device, which reads one flag back)."""
    if torch.is_tensor(idx) and idx.is_cuda:
        if idx.dtype not in (torch.int32, torch.int64) or idx.dim() != 1 or idx.numel() < 1:
            raise ValueError(f'{name} must be a non-empty 1-d integer tensor')
        if not bool(((idx >= 0) & (idx < n)).all()):
            raise ValueError(f'{name} holds indices outside [0, {n})')
        return idx.to(torch.int32).contiguous()
    a = np.asarray(idx.cpu().numpy() if torch.is_tensor(idx) else idx).reshape(-1)
    if a.size < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f'{name} must be a non-empty list of integer indices')
    if a.min() < 0 or a.max() >= n:
        raise ValueError(f'{name} holds indices outside [0, {n})')
    return to_device_async(a.astype(np.int32), dev)


def _scores_arg(scores, what):
    if not (torch.is_tensor(scores) and scores.is_cuda):
        raise nv.NativeError(f'{what} runs on the HIP device only (no CPU fallback)')
    if scores.dtype != torch.float32 or scores.dim() != 1 or not scores.is_contiguous() or not 1 <= scores.numel() < 2 ** 31:
        raise ValueError(f'{what}: scores must be a contiguous float32 [n] device tensor, not {tuple(scores.shape)} {scores.dtype}')
    return scores


def attack_scores(fit, X, rows, fold=0, stream=None):
    """ure_attack_score with ONE parameter set of a fit (its fold `fold`: weights and statistics) on the rows `rows` of a device
    table X -- fit on one table, score another -> float32 [len(rows)] on the device."""
    if not (torch.is_tensor(X) and X.is_cuda):
        raise nv.NativeError('attack_scores runs on the HIP device only (no CPU fallback)')
    if not (X.dtype == torch.float32 and X.dim() == 2 and X.stride(1) == 1 and X.shape[1] == fit.d and X.stride(0) >= fit.d):
        raise ValueError(f'attack_scores: X must be a float32 [n, {fit.d}] device tensor with unit column stride, not {tuple(X.shape)} {X.dtype}')
    fold = int(fold)
    if not 0 <= fold < fit.folds:
        raise ValueError(f'fold must be in 0 .. {fit.folds - 1}, not {fold!r}')
    rows_d = _index_list(rows, X.shape[0], X.device, 'rows')
    _attack_stream(stream)
    m = rows_d.numel()
    scores = torch.empty(m, dtype=torch.float32, device=X.device)
    nv.check(nv.lib().ure_attack_score(X.data_ptr(), int(X.stride(0)), fit.d, nv.ptr(rows_d), None, m, 1, fit.hidden, nv.ptr(fit.stats[fold]),
                                       nv.ptr(fit.params[fold]), nv.ptr(scores), nv.stream_handle(stream)), 'ure_attack_score')
    _csr_held_for(stream, rows_d, scores)
    return scores


def auc_counts(scores, pos, neg, stream=None):
    """ure_auc_counts: (counts int64 [2] = (pairs with s_p > s_n, pairs with s_p == s_n), nan_flag int32 [1]) on the device, for the
    index lists pos / neg into the float32 device tensor scores.  Never sorts; nothing of size n1 x n2 is written."""
    scores = _scores_arg(scores, 'auc_counts')
    dev = scores.device
    pos_d, neg_d = _index_list(pos, scores.numel(), dev, 'pos'), _index_list(neg, scores.numel(), dev, 'neg')
    _attack_stream(stream)
    n1, n2 = pos_d.numel(), neg_d.numel()
    nbytes = int(nv.lib().ure_auc_scratch(n1, n2))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    nv.check(nv.lib().ure_auc_counts(nv.ptr(scores), nv.ptr(pos_d), n1, nv.ptr(neg_d), n2, nv.ptr(counts), nv.ptr(flag), nv.ptr(scratch), nbytes,
                                     nv.stream_handle(stream)), 'ure_auc_counts')
    _csr_held_for(stream, pos_d, neg_d, scratch, counts, flag)
    return counts, flag


def confusion_counts(scores, pos, neg, thr=0.5, stream=None):
    """ure_confusion_counts: int64 [4] = (tp, fn, tn, fp) on the device; a score > thr predicts class 1."""
    scores = _scores_arg(scores, 'confusion_counts')
    thr = float(thr)
    if thr != thr:
        raise ValueError('thr is NaN')
    dev = scores.device
    pos_d, neg_d = _index_list(pos, scores.numel(), dev, 'pos'), _index_list(neg, scores.numel(), dev, 'neg')
    _attack_stream(stream)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    nv.check(nv.lib().ure_confusion_counts(nv.ptr(scores), nv.ptr(pos_d), pos_d.numel(), nv.ptr(neg_d), neg_d.numel(), thr, nv.ptr(counts),
                                           nv.stream_handle(stream)), 'ure_confusion_counts')
    _csr_held_for(stream, pos_d, neg_d, counts)
    return counts


# ---------------------------------------------------------------------------
# The LightGCN backbone (csrc/gcn.hip, include/ultrare_gcn.h; the contract is lightgcn.py)
# ---------------------------------------------------------------------------
class GcnGraph:
    """A shard's training triples as the bipartite graph LightGCN propagates over, resident on the device: the CSR (a user's
    items) and the CSC (an item's users) of lightgcn.Graph, s = 1 / sqrt(deg) of both sides, the ratings in CSR order and the
    position maps (pos: CSR entry -> file position, to_csr: CSC entry -> CSR position).  An index out of range, or no triple at
    all, raises ValueError before any device work."""

    def __init__(self, uid, iid, rating, n_user, n_item, device=None):
        from . import lightgcn
        rating = np.asarray(rating)
        if rating.shape != np.shape(uid):
            raise ValueError(f'rating has shape {rating.shape}, uid {np.shape(uid)}')
        self.host = g = lightgcn.Graph(uid, iid, n_user, n_item)
        if g.N == 0:
            raise ValueError('a graph needs at least one triple')
        self.n_user, self.n_item, self.N, self.nnz = g.n_user, g.n_item, g.N, g.N
        self.device = device or _device()
        names = ('off_u', 'col', 'row_u', 'pos', 'off_i', 'row', 'to_csr', 's_u', 's_i')
        arrays = [getattr(g, n) for n in names] + [rating.astype(np.float32)[g.pos]]
        # (plain copies, as CsrSet's: 28 bytes per rating)
        for n, a in zip(names + ('rating',), arrays):
            setattr(self, n, torch.from_numpy(np.ascontiguousarray(a)).to(self.device))

    def side(self, side):
        """(off, idx, s_src, s_dst, n_dst, n_src) device tensors of 'csr' (items -> users) or 'csc' (users -> items)."""
        if side == 'csr':
            return self.off_u, self.col, self.s_i, self.s_u, self.n_user, self.n_item
        if side == 'csc':
            return self.off_i, self.row, self.s_u, self.s_i, self.n_item, self.n_user
        raise ValueError(f"side {side!r}: 'csr' or 'csc'")


def _gcn_table(t, rows, d, what, dev):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise nv.NativeError('gcn_propagate runs on the HIP device only (no CPU fallback)')
    if not (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (rows, d)):
        raise ValueError(f'{what} must be a contiguous float32 [{rows}, {d}] tensor, not {tuple(t.shape)} {t.dtype}')
    if t.device != dev:
        raise ValueError(f'{what} is on {t.device} but the graph was uploaded to {dev}')
    return t


def _gcn_propagate(graph, side, X, add, sum, out, d, stream):
    """ure_gcn_propagate on checked tensors."""
    off, idx, s_src, s_dst, n_dst, n_src = graph.side(side)
    nv.check(nv.lib().ure_gcn_propagate(nv.ptr(off), nv.ptr(idx), n_dst, n_src, nv.ptr(s_src), nv.ptr(s_dst), nv.ptr(X), d, nv.ptr(add), nv.ptr(sum),
                                        nv.ptr(out), nv.stream_handle(stream)), 'ure_gcn_propagate')
    return out


def gcn_propagate(graph, side, X, add=None, sum=None, out=None, stream=None):
    """One LightGCN propagation (lightgcn.propagate_ref bit for bit): side 'csr' takes an item table X [n_item, d] to the users,
    'csc' a user table to the items.  out[r] = [add[r] +] s_dst[r] sum_j s_src[j] X[j]; sum (optional) is advanced in place by
    the rows stored; out (default: a new tensor) may be add, and must not overlap X.  d is a power of two in 4 .. 256.
    Nothing synchronises."""
    from . import lightgcn
    if not (torch.is_tensor(X) and X.is_cuda):
        raise nv.NativeError('gcn_propagate runs on the HIP device only (no CPU fallback)')
    _, _, _, _, n_dst, n_src = graph.side(side)
    d = lightgcn.check_width(int(X.shape[1]) if X.dim() == 2 else 0)
    _gcn_table(X, n_src, d, 'X', graph.device)
    for name, t in (('add', add), ('sum', sum), ('out', out)):
        if t is not None:
            _gcn_table(t, n_dst, d, name, graph.device)
    if out is None:
        out = torch.empty(n_dst, d, dtype=torch.float32, device=X.device)
        _csr_held_for(stream, out)
    return _gcn_propagate(graph, side, X, add, sum, out, d, stream)


def gcn_step_tags(graph, order, batch, stream=None):
    """The step of every CSR entry under one epoch's order (file positions in training order, batch t = order[t B : (t + 1) B]):
    the file-order tags are made on the host, the CSR-order tags by ure_gcn_gather_tags.  -> int32 [nnz] on the device."""
    order = np.asarray(order.cpu() if torch.is_tensor(order) else order).astype(np.int64)
    if order.shape != (graph.N,) or order.min() < 0 or order.max() >= graph.N or (np.bincount(order, minlength=graph.N) != 1).any():
        raise ValueError(f'the order is not a permutation of 0 .. {graph.N - 1}')
    file_tag = np.empty(graph.N, dtype=np.int32)
    file_tag[order] = np.arange(graph.N) // int(batch)
    file_tag = torch.from_numpy(file_tag).to(graph.device)
    tag = torch.empty(graph.nnz, dtype=torch.int32, device=graph.device)
    nv.check(nv.lib().ure_gcn_gather_tags(nv.ptr(file_tag), nv.ptr(graph.pos), graph.nnz, nv.ptr(tag), nv.stream_handle(stream)), 'ure_gcn_gather_tags')
    _csr_held_for(stream, file_tag, tag)
    return tag


def _gcn_mse_walks(graph, tag, step, U, V, d, err, pred, Gu, Gi, row_loss, st):
    """The residual pass and the two masked walks of an MSE step on checked tensors (pred may be None)."""
    g, L = graph, nv.lib()
    nv.check(L.ure_gcn_residual(nv.ptr(g.row_u), nv.ptr(g.col), nv.ptr(g.rating), nv.ptr(tag), g.nnz, int(step), nv.ptr(U), nv.ptr(V), g.n_user,
                                g.n_item, d, nv.ptr(err), nv.ptr(pred), st), 'ure_gcn_residual')
    nv.check(L.ure_gcn_grad(nv.ptr(g.off_u), nv.ptr(g.col), None, nv.ptr(tag), nv.ptr(err), g.n_user, g.n_item, g.nnz, int(step), nv.ptr(V), d,
                            nv.ptr(Gu), nv.ptr(row_loss), st), 'ure_gcn_grad')
    nv.check(L.ure_gcn_grad(nv.ptr(g.off_i), nv.ptr(g.row), nv.ptr(g.to_csr), nv.ptr(tag), nv.ptr(err), g.n_item, g.n_user, g.nnz, int(step), nv.ptr(U),
                            d, nv.ptr(Gi), None, st), 'ure_gcn_grad')


def gcn_loss_grad(graph, tag, step, U, V, want_pred=False, stream=None):
    """lightgcn.loss_grad_ref of the batch {CSR entries with tag == step} under the final tables (U, V) [rows, d]:
    -> (G_u [n_user, d], G_i [n_item, d], loss float64 [1] on the device, err [nnz], pred [nnz] or None -- both in CSR order, +0.0
    outside the batch).  Three launches and the loss fold; nothing synchronises."""
    from . import lightgcn
    if not (torch.is_tensor(U) and U.is_cuda and torch.is_tensor(V) and V.is_cuda):
        raise nv.NativeError('gcn_loss_grad runs on the HIP device only (no CPU fallback)')
    d = lightgcn.check_width(int(U.shape[1]) if U.dim() == 2 else 0)
    _gcn_table(U, graph.n_user, d, 'U', graph.device)
    _gcn_table(V, graph.n_item, d, 'V', graph.device)
    if not (torch.is_tensor(tag) and tag.dtype == torch.int32 and tag.shape == (graph.nnz,) and tag.device == graph.device and tag.is_contiguous()):
        raise ValueError(f'tag must be a contiguous int32 [{graph.nnz}] tensor on {graph.device}')
    g, L, dev, st = graph, nv.lib(), graph.device, nv.stream_handle(stream)
    err = torch.empty(g.nnz, dtype=torch.float32, device=dev)
    pred = torch.empty(g.nnz, dtype=torch.float32, device=dev) if want_pred else None
    Gu, Gi = torch.empty_like(U), torch.empty_like(V)
    row_loss, loss = torch.empty(g.n_user, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    _gcn_mse_walks(g, tag, step, U, V, d, err, pred, Gu, Gi, row_loss, st)
    nv.check(L.ure_gcn_step_loss(nv.ptr(row_loss), g.n_user, 1, nv.ptr(loss), st), 'ure_gcn_step_loss')
    _csr_held_for(stream, err, Gu, Gi, row_loss, loss, *([pred] if want_pred else []))
    return Gu, Gi, loss, err, pred


def gcn_sgd_step(w, m, g, lr, lam, mu, first, gscale=1.0, stream=None):
    """lightgcn.sgd_update_ref in place on the device tensors w and m (float32, contiguous, a multiple of 4 elements), with the
    gradient g * gscale.  Nothing synchronises."""
    for t in (w, m, g):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise nv.NativeError('gcn_sgd_step runs on the HIP device only (no CPU fallback)')
        if not (t.dtype == torch.float32 and t.is_contiguous() and t.shape == w.shape and t.numel() % 4 == 0 and t.numel() > 0):
            raise ValueError('w, m and g must be contiguous float32 tensors of one shape, a multiple of 4 elements')
    nv.check(nv.lib().ure_gcn_sgd_step(nv.ptr(w), nv.ptr(m), nv.ptr(g), w.numel(), float(gscale), float(np.float32(lr)), float(np.float32(lam)),
                                       float(np.float32(mu)), int(bool(first)), nv.stream_handle(stream)), 'ure_gcn_sgd_step')


# ---- BPR (csrc/bpr.hip, include/ultrare_bpr.h; the contract is bpr.py) ---------------------------------------------------------
def bpr_prepare(graph):
    """The users' distinct items of a GcnGraph on its device (graph.off_d, graph.col_d), made once per graph on the host.  A user
    with triples and no item left to draw raises ValueError before any device work."""
    if getattr(graph, 'off_d', None) is None:
        from . import bpr
        off_d, col_d = bpr.distinct_csr(graph.host)
        bpr.check_negatives(graph.host, off_d)
        graph.col_d = torch.from_numpy(col_d).to(graph.device)
        graph.off_d = torch.from_numpy(off_d).to(graph.device)
    return graph


def _bpr_sample(graph, key, epoch, neg, st):
    g = graph
    nv.check(nv.lib().ure_bpr_sample(nv.ptr(g.off_d), nv.ptr(g.col_d), g.col_d.numel(), nv.ptr(g.row_u), nv.ptr(g.pos), g.nnz, g.n_user, g.n_item,
                                     int(key) & 0xFFFFFFFFFFFFFFFF, int(epoch), nv.ptr(neg), st), 'ure_bpr_sample')


def _bpr_index(graph, neg, off_n, map_n, usr_n, scratch, st):
    nv.check(nv.lib().ure_bpr_index(nv.ptr(neg), nv.ptr(graph.row_u), graph.nnz, graph.n_item, nv.ptr(off_n), nv.ptr(map_n), nv.ptr(usr_n),
                                    nv.ptr(scratch), scratch.numel(), st), 'ure_bpr_index')


def _bpr_int_vector(t, graph, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise nv.NativeError(f'{what} must be on the HIP device (no CPU fallback)')
    if not (t.dtype == torch.int32 and t.shape == (graph.nnz,) and t.device == graph.device and t.is_contiguous()):
        raise ValueError(f'{what} must be a contiguous int32 [{graph.nnz}] tensor on {graph.device}')
    return t


def bpr_negatives(graph, key, epoch, stream=None):
    """bpr.sample_ref on the device: the negative item of every CSR entry in `epoch` under `key` (bpr.stream_key) -> int32 [nnz].
    Nothing synchronises."""
    if isinstance(epoch, bool) or not isinstance(epoch, (int, np.integer)) or not 0 <= epoch < 2 ** 31:
        raise ValueError(f'epoch must be an integer in 0 .. 2^31 - 1, not {epoch!r}')
    bpr_prepare(graph)
    neg = torch.empty(graph.nnz, dtype=torch.int32, device=graph.device)
    _bpr_sample(graph, key, epoch, neg, nv.stream_handle(stream))
    _csr_held_for(stream, neg)
    return neg


def bpr_neg_index(graph, neg, stream=None):
    """bpr.neg_index_ref on the device: -> (off_n int64 [n_item + 1], map_n int32 [nnz], usr_n int32 [nnz]).  Nothing synchronises."""
    _bpr_int_vector(neg, graph, 'neg')
    dev = graph.device
    off_n = torch.empty(graph.n_item + 1, dtype=torch.int64, device=dev)
    map_n, usr_n = torch.empty_like(neg), torch.empty_like(neg)
    scratch = torch.empty(int(nv.lib().ure_bpr_index_scratch(graph.nnz, graph.n_item)), dtype=torch.uint8, device=dev)
    _bpr_index(graph, neg, off_n, map_n, usr_n, scratch, nv.stream_handle(stream))
    _csr_held_for(stream, off_n, map_n, usr_n, scratch)
    return off_n, map_n, usr_n


def _bpr_walks(graph, tag, step, U, V, neg, index, w, x, d, Gu, Gi, row_loss, st):
    g, L = graph, nv.lib()
    off_n, map_n, usr_n = index
    nv.check(L.ure_bpr_grad_user(nv.ptr(g.off_u), nv.ptr(g.col), nv.ptr(neg), nv.ptr(tag), nv.ptr(w), nv.ptr(x), g.n_user, g.n_item, g.nnz, int(step),
                                 nv.ptr(V), d, nv.ptr(Gu), nv.ptr(row_loss), st), 'ure_bpr_grad_user')
    nv.check(L.ure_bpr_grad_item(nv.ptr(g.off_i), nv.ptr(g.row), nv.ptr(g.to_csr), nv.ptr(off_n), nv.ptr(map_n), nv.ptr(usr_n), nv.ptr(tag), nv.ptr(w),
                                 g.n_item, g.n_user, g.nnz, int(step), nv.ptr(U), d, nv.ptr(Gi), st), 'ure_bpr_grad_item')


def bpr_loss_grad(graph, tag, step, U, V, neg, index=None, coef=None, stream=None):
    """bpr.loss_grad_ref of the batch {CSR entries with tag == step} under the final tables (U, V) [rows, d], the epoch's negatives
    neg and their index (default: made here): -> (G_u, G_i, loss float64 [1] on the device, w, x, s_pos, s_neg -- [nnz] in CSR order,
    +0.0 outside the batch).  coef = (w, x): the walks run on these given arrays and the coefficient pass is left out (s_pos and
    s_neg are then None).  Nothing synchronises."""
    from . import lightgcn
    if not (torch.is_tensor(U) and U.is_cuda and torch.is_tensor(V) and V.is_cuda):
        raise nv.NativeError('bpr_loss_grad runs on the HIP device only (no CPU fallback)')
    d = lightgcn.check_width(int(U.shape[1]) if U.dim() == 2 else 0)
    _gcn_table(U, graph.n_user, d, 'U', graph.device)
    _gcn_table(V, graph.n_item, d, 'V', graph.device)
    _bpr_int_vector(tag, graph, 'tag')
    _bpr_int_vector(neg, graph, 'neg')
    g, L, dev, st = graph, nv.lib(), graph.device, nv.stream_handle(stream)
    if index is None:
        index = bpr_neg_index(graph, neg, stream)
    sp = sn = None
    if coef is None:
        w, x, sp, sn = (torch.empty(g.nnz, dtype=torch.float32, device=dev) for _ in range(4))
        nv.check(L.ure_bpr_coef(nv.ptr(g.row_u), nv.ptr(g.col), nv.ptr(neg), nv.ptr(tag), g.nnz, int(step), nv.ptr(U), nv.ptr(V), g.n_user, g.n_item, d,
                                nv.ptr(w), nv.ptr(x), nv.ptr(sp), nv.ptr(sn), st), 'ure_bpr_coef')
    else:
        w, x = coef
        for name, t in (('w', w), ('x', x)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.shape == (g.nnz,) and t.device == dev and t.is_contiguous()):
                raise ValueError(f'{name} must be a contiguous float32 [{g.nnz}] tensor on {dev}')
    Gu, Gi = torch.empty_like(U), torch.empty_like(V)
    row_loss, loss = torch.empty(g.n_user, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    _bpr_walks(g, tag, step, U, V, neg, index, w, x, d, Gu, Gi, row_loss, st)
    nv.check(L.ure_gcn_step_loss(nv.ptr(row_loss), g.n_user, 1, nv.ptr(loss), st), 'ure_gcn_step_loss')
    _csr_held_for(stream, Gu, Gi, row_loss, loss, w, x, *index, *([sp, sn] if coef is None else []))
    return Gu, Gi, loss, w, x, sp, sn


# ---- in-training attribute unlearning (csrc/attr_train.hip, include/ultrare_attr_train.h; the contract is attr_train.py) ----------
class StepGroups:
    """Two attribute groups of a shard's users for the per-batch term: group_of_user int8 [n_user] on the device (0, 1, 2) and the
    capacities cap1, cap2 -- the groups' sizes among the users WITH entries, which bound every step's counts.  Checked once on the
    host (attr_unlearn.check_groups); cap1 or cap2 may be 0 here (a shard without one group), which the callers decide about."""

    def __init__(self, graph, id1, id2):
        from .attr_unlearn import check_groups
        rows, n1, _ = check_groups(id1, id2, graph.n_user)
        self.graph, self.n_user, self.device = graph, graph.n_user, graph.device
        self.host = np.zeros(graph.n_user, dtype=np.int8)
        self.host[rows[:n1]], self.host[rows[n1:]] = 1, 2
        has = np.diff(graph.host.off_u) > 0
        self.cap1, self.cap2 = int((has & (self.host == 1)).sum()), int((has & (self.host == 2)).sum())
        self.group = to_device_async(self.host, self.device)

    @property
    def cap(self):
        return self.cap1 + self.cap2


def _attr_caps(cap1, cap2, who):
    cap1, cap2 = int(cap1), int(cap2)
    if cap1 < 1 or cap2 < 1:
        raise ValueError(f'{who}: both capacities must be at least 1, not {cap1} and {cap2}')
    return cap1, cap2


def _attr_words(steps):
    steps = int(steps)
    if steps < 1:
        raise ValueError(f'steps must be positive, not {steps}')
    return steps, (steps + 31) // 32


def _attr_masks(graph, tag, group, steps, masks, st):
    nv.check(nv.lib().ure_attr_step_masks(nv.ptr(graph.off_u), nv.ptr(tag), nv.ptr(group), graph.n_user, graph.nnz, steps, nv.ptr(masks), st),
             'ure_attr_step_masks')


def attr_step_masks(graph, tag, group, steps, stream=None):
    """ure_attr_step_masks: per user of the GcnGraph a bitset over an epoch's steps, uint32 [n_user, ceil(steps / 32)] (returned as
    int32 bit patterns) -- bit s set iff the user is in a group (group: int8 [n_user] device tensor, 0 / 1 / 2) and has a CSR entry
    with tag == s (tag: gcn_step_tags).  Nothing synchronises."""
    steps, words = _attr_words(steps)
    _bpr_int_vector(tag, graph, 'tag')
    if not (torch.is_tensor(group) and group.is_cuda and group.dtype == torch.int8 and group.shape == (graph.n_user,) and group.device == graph.device):
        raise ValueError(f'group must be an int8 [{graph.n_user}] tensor on {graph.device}')
    masks = torch.empty(graph.n_user, words, dtype=torch.int32, device=graph.device)
    _attr_masks(graph, tag, group, steps, masks, nv.stream_handle(stream))
    _csr_held_for(stream, masks)
    return masks


def _attr_select(masks, group, n_user, steps, step, cap1, cap2, rows, counts, scratch, st):
    nv.check(nv.lib().ure_attr_select(nv.ptr(masks), nv.ptr(group), n_user, steps, int(step), cap1, cap2, nv.ptr(rows), nv.ptr(counts), nv.ptr(scratch),
                                      scratch.numel(), st), 'ure_attr_select')


def attr_select(masks, group, steps, step, cap1, cap2, stream=None):
    """ure_attr_select: the step's rows, an ordered compaction of attr_step_masks -- (rows int32 [cap1 + cap2], counts int32 [2]) on the
    device, equal to attr_train.batch_groups_ref integer for integer (-1 behind the selected rows).  Nothing synchronises."""
    steps, words = _attr_words(steps)
    cap1, cap2 = _attr_caps(cap1, cap2, 'attr_select')
    if not (torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.int32 and masks.dim() == 2 and masks.shape[1] == words and masks.is_contiguous()):
        raise ValueError(f'masks must be a contiguous int32 [n_user, {words}] device tensor (attr_step_masks)')
    n_user = int(masks.shape[0])
    if not (torch.is_tensor(group) and group.dtype == torch.int8 and group.shape == (n_user,) and group.device == masks.device):
        raise ValueError(f'group must be an int8 [{n_user}] tensor on {masks.device}')
    if not 0 <= int(step) < steps:
        raise ValueError(f'step {step} outside 0 .. {steps - 1}')
    dev = masks.device
    rows = torch.empty(cap1 + cap2, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(nv.lib().ure_attr_select_scratch(n_user)), dtype=torch.uint8, device=dev)
    _attr_select(masks, group, n_user, steps, step, cap1, cap2, rows, counts, scratch, nv.stream_handle(stream))
    _csr_held_for(stream, rows, counts, scratch)
    return rows, counts


def _attr_step_table(X, rows, counts, cap1, cap2, what):
    from .attr_unlearn import check_width
    cap1, cap2 = _attr_caps(cap1, cap2, what)
    if not (torch.is_tensor(X) and X.is_cuda):
        raise nv.NativeError(f'{what} runs on the HIP device only (no CPU fallback)')
    if not (X.dtype == torch.float32 and X.dim() == 2 and X.stride(1) == 1 and X.stride(0) >= X.shape[1]):
        raise ValueError(f'{what}: X must be a float32 [rows, d] device tensor with unit column stride, not {tuple(X.shape)} {X.dtype}')
    if not (torch.is_tensor(rows) and rows.dtype == torch.int32 and rows.shape == (cap1 + cap2,) and rows.device == X.device and rows.is_contiguous()):
        raise ValueError(f'{what}: rows must be a contiguous int32 [{cap1 + cap2}] tensor on {X.device}')
    if not (torch.is_tensor(counts) and counts.dtype == torch.int32 and counts.shape == (2,) and counts.device == X.device):
        raise ValueError(f'{what}: counts must be an int32 [2] tensor on {X.device}')
    d = check_width(X.shape[1], X.stride(0))
    nbytes = int(nv.lib().ure_attr_scratch(cap1 + cap2, d))
    if nbytes < 0:
        raise ValueError(f'ure_attr_scratch refused cap = {cap1 + cap2}, d = {d}')
    return cap1, cap2, d, int(X.stride(0)), nbytes


def _attr_acc(t, dtype, what, dev):
    if t is not None and not (torch.is_tensor(t) and t.dtype == dtype and t.numel() == 1 and t.device == dev):
        raise ValueError(f'{what} must be a {dtype} device tensor of one value on {dev}')
    return t


def mmd_loss_grad_dev(X, rows, counts, cap1, cap2, kernel_mul=2.0, kernel_num=5, fix_sigma=None, acc=None, skipped=None, stream=None):
    """ure_attr_mmd_loss_grad: mmd_bandwidth + mmd_loss_grad at counts that live on the device (rows, counts: attr_select) ->
    (sums float64 [4], grad float32 [cap1 + cap2, d], valid int32 [1], bandwidth float64 0-d), all on the device; the loss is added
    to acc (float64 device tensor of one value) when the step is valid, skipped (int32) is advanced when it is not.  Nothing
    synchronises."""
    from .attr_unlearn import check_mmd_args
    kernel_mul, kernel_num, fix_sigma = check_mmd_args(kernel_mul, kernel_num, fix_sigma)
    cap1, cap2, d, ld, nbytes = _attr_step_table(X, rows, counts, cap1, cap2, 'mmd_loss_grad_dev')
    dev = X.device
    _attr_acc(acc, torch.float64, 'acc', dev)
    _attr_acc(skipped, torch.int32, 'skipped', dev)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sums, bw = torch.empty(4, dtype=torch.float64, device=dev), torch.empty((), dtype=torch.float64, device=dev)
    grad, valid = torch.empty(cap1 + cap2, d, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    nv.check(nv.lib().ure_attr_mmd_loss_grad(X.data_ptr(), ld, d, nv.ptr(rows), nv.ptr(counts), cap1, cap2, kernel_mul, kernel_num, fix_sigma or 0.0,
                                             bw.data_ptr(), nv.ptr(sums), nv.ptr(grad), nv.ptr(valid), nv.ptr(acc), nv.ptr(skipped), nv.ptr(scratch), nbytes,
                                             nv.stream_handle(stream)), 'ure_attr_mmd_loss_grad')
    _csr_held_for(stream, scratch, sums, bw, grad, valid)
    return sums, grad, valid, bw


def u2u_loss_grad_dev(X, rows, counts, cap1, cap2, acc=None, skipped=None, stream=None):
    """ure_attr_u2u_loss_grad: u2u_loss_grad at device counts -> (value float64 0-d, grad float32 [cap1 + cap2, d], valid int32 [1]) on
    the device; acc and skipped as mmd_loss_grad_dev's.  Nothing synchronises."""
    cap1, cap2, d, ld, nbytes = _attr_step_table(X, rows, counts, cap1, cap2, 'u2u_loss_grad_dev')
    dev = X.device
    _attr_acc(acc, torch.float64, 'acc', dev)
    _attr_acc(skipped, torch.int32, 'skipped', dev)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    value = torch.empty((), dtype=torch.float64, device=dev)
    grad, valid = torch.empty(cap1 + cap2, d, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    nv.check(nv.lib().ure_attr_u2u_loss_grad(X.data_ptr(), ld, d, nv.ptr(rows), nv.ptr(counts), cap1, cap2, value.data_ptr(), nv.ptr(grad), nv.ptr(valid),
                                             nv.ptr(acc), nv.ptr(skipped), nv.ptr(scratch), nbytes, nv.stream_handle(stream)), 'ure_attr_u2u_loss_grad')
    _csr_held_for(stream, scratch, value, grad, valid)
    return value, grad, valid


def _attr_add(G, ld, n_rows, d, rows, counts, cap, valid, grad, eta, st):
    nv.check(nv.lib().ure_attr_add_grad(nv.ptr(G), ld, n_rows, d, nv.ptr(rows), nv.ptr(counts), cap, nv.ptr(valid), nv.ptr(grad), float(np.float32(eta)), st),
             'ure_attr_add_grad')


def attr_add_grad(G, rows, counts, valid, grad, eta, stream=None):
    """ure_attr_add_grad, in place: G[rows[i]][c] = fl(G[rows[i]][c] + fl(eta grad[i][c])) for i < counts[0] + counts[1] and only when
    valid; every other byte of G (float32 [n_rows, >= d], unit column stride) keeps its value.  Nothing synchronises."""
    from .attr_train import check_eta
    eta = check_eta(eta)
    for t in (G, grad):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise nv.NativeError('attr_add_grad runs on the HIP device only (no CPU fallback)')
    cap, d = int(grad.shape[0]), int(grad.shape[1])
    if not (grad.dtype == torch.float32 and grad.is_contiguous() and G.dtype == torch.float32 and G.dim() == 2 and G.stride(1) == 1 and G.shape[1] >= d
            and G.stride(0) >= G.shape[1]):
        raise ValueError('G must be a float32 [n_rows, >= d] tensor with unit column stride and grad a contiguous float32 [cap, d] tensor')
    if not (rows.dtype == torch.int32 and rows.shape == (cap,) and counts.dtype == torch.int32 and counts.shape == (2,) and valid.dtype == torch.int32
            and valid.numel() == 1 and rows.device == counts.device == valid.device == grad.device == G.device):
        raise ValueError(f'rows int32 [{cap}], counts int32 [2] and valid int32 [1] must lie on {G.device}')
    _attr_add(G, int(G.stride(0)), int(G.shape[0]), d, rows, counts, cap, valid, grad, eta, nv.stream_handle(stream))
    return G


class _GraphJob:
    """What the trainers over a GcnGraph share (GcnJob, NmfJob): the checks of batch, epochs and orders, the float32 schedule and
    scalars, the epoch bookkeeping, and the three launches a step of either makes beside its own -- the gather of the epoch's table
    at its first step, the loss fold and the SGD update.  A subclass checks its init, allocates its buffers (_pool, _row_loss and
    _sse among them) and writes _step(e, s, stream)."""

    def _check_sizes(self, graph, batch, epochs):
        self.graph, self.batch, self.epochs, self.device = graph, int(batch), int(epochs), graph.device
        if self.batch < 1 or self.epochs < 0:
            raise ValueError(f'batch {batch!r} must be positive and epochs {epochs!r} not negative')

    def _plan(self, orders, lr, lam, momentum, lr_decay, lr_step):
        """-> int32 [epochs, N]: a triple's place in every epoch's order (the inverse permutations; place // batch is its step), every
        order checked once.  Sets the schedule, the scalars and the counters; no device work."""
        N = self.graph.N
        orders = np.asarray(orders.cpu() if torch.is_tensor(orders) else orders)
        if orders.shape != (self.epochs, N) or orders.dtype.kind not in 'iu':
            raise ValueError(f'orders must be integers of shape ({self.epochs}, {N}), not {orders.dtype} {orders.shape}')
        places = np.empty((self.epochs, N), dtype=np.int32)
        for e in range(self.epochs):
            o = orders[e].astype(np.int64)
            if o.min() < 0 or o.max() >= N or (np.bincount(o, minlength=N) != 1).any():
                raise ValueError(f'orders[{e}] is not a permutation of 0 .. {N - 1}')
            places[e, o] = np.arange(N, dtype=np.int32)
        # StepLR as engine.TrainJob makes it: float32 values
        self._lr_host = np.array([lr * (lr_decay ** (t // lr_step)) for t in range(self.epochs)], dtype=np.float32)
        self._lam, self._mu = float(np.float32(lam)), float(np.float32(momentum))
        self.steps = (N + self.batch - 1) // self.batch
        self.ticks = self.epochs * self.steps
        self.done = 0            # optimizer steps run
        return places

    # ---- the launches both jobs make ------------------------------------------------------------------------------------
    def _gather(self, table, out, st):
        """out [nnz] (CSR order) = one epoch's row of a file-order table."""
        g = self.graph
        nv.check(nv.lib().ure_gcn_gather_tags(nv.ptr(table), nv.ptr(g.pos), g.nnz, nv.ptr(out), st), 'ure_gcn_gather_tags')

    def _fold_loss(self, e, s, st):
        """The epoch's loss takes (step 0) or is advanced by the fold of the users' sums of this step."""
        nv.check(nv.lib().ure_gcn_step_loss(nv.ptr(self._row_loss), self.graph.n_user, int(s == 0), self._sse[e:].data_ptr(), st), 'ure_gcn_step_loss')

    def _sgd(self, e, w, m, g, gscale, st):
        """One update of every parameter at epoch e's rate; counts the step."""
        nv.check(nv.lib().ure_gcn_sgd_step(nv.ptr(w), nv.ptr(m), nv.ptr(g), w.numel(), gscale, float(self._lr_host[e]), self._lam, self._mu,
                                           int(self.done == 0), st), 'ure_gcn_sgd_step')
        self.done += 1

    # ---- what Scratch._train uses of a job -----------------------------------------------------------------------------
    def steps_per_epoch(self, s=0):
        return self.steps

    def run_epochs(self, n_epochs, stream=None):
        """Advance by whole epochs on `stream` (default: the current one).  Nothing synchronises."""
        assert self._pool is not None, 'the job is closed'
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(self.device))          # (the uploads and fills of __init__)
        e0 = self.done // self.steps
        assert self.done % self.steps == 0 and e0 + n_epochs <= self.epochs
        for e in range(e0, e0 + n_epochs):
            for s in range(self.steps):
                self._step(e, s, stream)
        return self.done

    def run(self, stream=None):
        return self.run_epochs(self.epochs - self.done // self.steps, stream)

    def epoch_sse(self, s=0):
        """Per-epoch sum of squared training errors (host float64 array; synchronises)."""
        assert s == 0
        return self._sse[:self.epochs].cpu().numpy()


class GcnJob(_GraphJob):
    """One shard trained with the LightGCN backbone (lightgcn.train_ref in float32, bit for bit): per step a forward of `layers`
    propagations per side, the residual pass and the two masked gradient walks, `layers` more propagations back, and one SGD
    update of every row of the parameters.  What Scratch._train uses of a TrainJob is here under the same names.
    loss='bpr' (bpr.train_ref in float32; bit for bit but for the coefficient w, which is held to one ulp) trains the pairwise BPR
    loss instead: the negatives (under `key`, bpr.stream_key) and their index are made on the device at each epoch's first step,
    and the coefficient pass and the two BPR walks stand where the residual pass and the masked walks stand.

    attr=(id1, id2) with dis_type 'd2d' / 'u2u' (attr_train.train_ref) adds eta times the MMD / Laplacian term over the
    batch's distinct users of the two groups to every step: the step masks are made at each epoch's first step, and the selection, the
    loss at device counts and the hand-off into the user gradient stand between the loss fold and the backward propagations.  The
    kernels of that term are held to bounds, not bits.  Without attr the job makes exactly the launches it made before.

    graph  : GcnGraph
    init   : (P0 [n_user, k], Q0 [n_item, k]) float32 numpy arrays or tensors
    orders : int32 [epochs, N] -- per epoch the file positions in training order (batch t = orders[e][t B : (t + 1) B])"""

    _TABLES = ('W', 'M', 'G', 'S', 'Xa', 'Xb', 'Star')

    def __init__(self, graph, init, orders, k, layers, batch, epochs, lr, lam, momentum, lr_decay=1.0, lr_step=50, loss='mse', key=0, attr=None,
                 dis_type='nor', eta=1.0, kernel_mul=2.0, kernel_num=5, fix_sigma=None):
        from . import attr_train, lightgcn
        if loss not in ('mse', 'bpr'):
            raise ValueError(f"loss {loss!r}: 'mse' or 'bpr'")
        if dis_type not in attr_train.DIS_TYPES:
            raise ValueError(f"dis_type {dis_type!r}: one of {attr_train.DIS_TYPES}")
        if (attr is None) != (dis_type == 'nor'):
            raise ValueError("attr=(id1, id2) goes with dis_type 'd2d' or 'u2u', attr=None with 'nor'")
        self.dis_type, self._attr = dis_type, None
        if attr is not None:
            if len(attr) != 2:
                raise ValueError('attr must be the pair (id1, id2)')
            _, _, self.eta, self._kernel_mul, self._kernel_num, self._fix_sigma = attr_train.check_train_args(
                graph.n_user, k, attr[0], attr[1], dis_type, eta, kernel_mul, kernel_num, fix_sigma)
        if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= key < 2 ** 64:
            raise ValueError(f'key must be an integer in 0 .. 2^64 - 1, not {key!r}')
        self.loss, self.key = loss, int(key)
        self.layers = lightgcn.check_layers(layers)
        self.k, self.d = int(k), pad_dim(int(k))
        self._check_sizes(graph, batch, epochs)
        P0, Q0 = (np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float32) for t in init)
        if P0.shape != (graph.n_user, self.k) or Q0.shape != (graph.n_item, self.k):
            raise ValueError(f'init tables have shapes {P0.shape}, {Q0.shape}: ({graph.n_user}, {self.k}) and ({graph.n_item}, {self.k}) are needed')
        file_tags = (self._plan(orders, lr, lam, momentum, lr_decay, lr_step).astype(np.int64) // self.batch).astype(np.int32)      # a triple's step
        if loss == 'bpr':
            bpr_prepare(graph)                              # (refuses a user without a negative)
        self._c = float(lightgcn.layer_scale(self.layers))
        dev, R = self.device, graph.n_user + graph.n_item
        self.rows = R
        self._pool = torch.zeros(len(self._TABLES), R, self.d, dtype=torch.float32, device=dev)
        self._t = dict(zip(self._TABLES, self._pool))
        start = np.zeros((R, self.d), dtype=np.float32)
        start[:graph.n_user, :self.k], start[graph.n_user:, :self.k] = P0, Q0
        self._t['W'].copy_(torch.from_numpy(start))
        self._file_tags = torch.from_numpy(file_tags).to(dev)
        self._tag = torch.zeros(graph.nnz, dtype=torch.int32, device=dev)
        self._err = torch.zeros(graph.nnz, dtype=torch.float32, device=dev)
        self._row_loss = torch.zeros(graph.n_user, dtype=torch.float64, device=dev)
        self._sse = torch.zeros(max(self.epochs, 1), dtype=torch.float64, device=dev)
        self._bpr = None
        if loss == 'bpr':        # 16 bytes per rating and 8 per item beside the job's own, and the sort's scratch
            ints = lambda: torch.zeros(graph.nnz, dtype=torch.int32, device=dev)
            self._bpr = dict(neg=ints(), map_n=ints(), usr_n=ints(), off_n=torch.zeros(graph.n_item + 1, dtype=torch.int64, device=dev),
                             w=torch.zeros(graph.nnz, dtype=torch.float32, device=dev),
                             scratch=torch.zeros(int(nv.lib().ure_bpr_index_scratch(graph.nnz, graph.n_item)), dtype=torch.uint8, device=dev))
        self._star_at = -1       # the step count Star belongs to
        if attr is not None:
            self._attr_buffers(StepGroups(graph, *attr))

    def _attr_buffers(self, groups):
        """The per-batch term's device memory: the step masks of one epoch, a step's rows, counts, gradient and validity word, the
        scratch of the loss entries (planned from the capacities), and per epoch the summed loss values and the skipped steps."""
        if groups.cap1 < 1 or groups.cap2 < 1:
            raise ValueError(f'the shard has {groups.cap1} users of group 1 and {groups.cap2} of group 2 with entries: both groups need one '
                             "(train such a shard with dis_type='nor')")
        dev, L, E = self.device, nv.lib(), max(self.epochs, 1)
        nbytes = int(L.ure_attr_scratch(groups.cap, self.k))
        if nbytes < 0:
            raise ValueError(f'ure_attr_scratch refused cap = {groups.cap}, d = {self.k}')
        a = dict(groups=groups, masks=torch.zeros(self.graph.n_user, (self.steps + 31) // 32, dtype=torch.int32, device=dev),
                 rows=torch.zeros(groups.cap, dtype=torch.int32, device=dev), counts=torch.zeros(2, dtype=torch.int32, device=dev),
                 grad=torch.zeros(groups.cap, self.k, dtype=torch.float32, device=dev), valid=torch.zeros(1, dtype=torch.int32, device=dev),
                 out=torch.zeros(4, dtype=torch.float64, device=dev), scratch=torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                 sel=torch.zeros(int(L.ure_attr_select_scratch(self.graph.n_user)), dtype=torch.uint8, device=dev),
                 dis=torch.zeros(E, dtype=torch.float64, device=dev), skipped=torch.zeros(E, dtype=torch.int32, device=dev))
        self._attr = a

    def _attr_term(self, e, s, U, Gu, st):
        """Gu[rows] += eta g of the step's MMD / u2u term on U[rows]: the selection, the loss at device counts, the hand-off."""
        a, g, L = self._attr, self._attr['groups'], nv.lib()
        if s == 0:
            _attr_masks(self.graph, self._tag, g.group, self.steps, a['masks'], st)
        _attr_select(a['masks'], g.group, self.graph.n_user, self.steps, s, g.cap1, g.cap2, a['rows'], a['counts'], a['sel'], st)
        front = (U.data_ptr(), self.d, self.k, nv.ptr(a['rows']), nv.ptr(a['counts']), g.cap1, g.cap2)
        back = (nv.ptr(a['grad']), nv.ptr(a['valid']), a['dis'][e:].data_ptr(), a['skipped'][e:].data_ptr(), nv.ptr(a['scratch']), a['scratch'].numel(), st)
        if self.dis_type == 'd2d':
            nv.check(L.ure_attr_mmd_loss_grad(*front, self._kernel_mul, self._kernel_num, self._fix_sigma or 0.0, None, nv.ptr(a['out']), *back),
                     'ure_attr_mmd_loss_grad')
        else:
            nv.check(L.ure_attr_u2u_loss_grad(*front, nv.ptr(a['out']), *back), 'ure_attr_u2u_loss_grad')
        _attr_add(Gu, self.d, self.graph.n_user, self.k, a['rows'], a['counts'], g.cap, a['valid'], a['grad'], self.eta, st)

    # ---- launches ------------------------------------------------------------------------------------------------------
    def _sides(self, t):
        n = self.graph.n_user
        return t[:n], t[n:]

    def _copy(self, src, c, dst, st):
        nv.check(nv.lib().ure_gcn_scale(nv.ptr(src), src.numel(), c, nv.ptr(dst), st), 'ure_gcn_scale')

    def _layer(self, src, dst, add, sum, stream):
        """dst = [add +] A src, both sides; sum += dst."""
        (src_u, src_i), (dst_u, dst_i) = self._sides(src), self._sides(dst)
        add_u, add_i = self._sides(add) if add is not None else (None, None)
        sum_u, sum_i = self._sides(sum) if sum is not None else (None, None)
        _gcn_propagate(self.graph, 'csr', src_i, add_u, sum_u, dst_u, self.d, stream)
        _gcn_propagate(self.graph, 'csc', src_u, add_i, sum_i, dst_i, self.d, stream)

    def _forward(self, stream=None):
        """Star = the layer mean of W and its propagations (skipped when Star is that of the current parameters)."""
        if self._star_at == self.done:
            return
        t, st = self._t, nv.stream_handle(stream)
        if self.layers:
            self._copy(t['W'], 1.0, t['S'], st)             # (x * 1.0f is x)
            src = t['W']
            for l in range(self.layers):
                dst = t['Xa'] if l % 2 == 0 else t['Xb']
                self._layer(src, dst, None, t['S'], stream)
                src = dst
        self._copy(t['S'] if self.layers else t['W'], self._c, t['Star'], st)
        self._star_at = self.done

    def _step(self, e, s, stream=None):
        g, t, st = self.graph, self._t, nv.stream_handle(stream)
        if s == 0:
            self._gather(self._file_tags[e], self._tag, st)
        self._forward(stream)
        U, V = self._sides(t['Star'])
        Gu, Gi = self._sides(t['G'])
        if self._bpr is not None:
            b = self._bpr
            index = (b['off_n'], b['map_n'], b['usr_n'])
            if s == 0:                                      # this epoch's negatives and their index
                _bpr_sample(g, self.key, e, b['neg'], st)
                _bpr_index(g, b['neg'], *index, b['scratch'], st)
            nv.check(nv.lib().ure_bpr_coef(nv.ptr(g.row_u), nv.ptr(g.col), nv.ptr(b['neg']), nv.ptr(self._tag), g.nnz, s, nv.ptr(U), nv.ptr(V), g.n_user,
                                           g.n_item, self.d, nv.ptr(b['w']), nv.ptr(self._err), None, None, st), 'ure_bpr_coef')
            _bpr_walks(g, self._tag, s, U, V, b['neg'], index, b['w'], self._err, self.d, Gu, Gi, self._row_loss, st)
        else:
            _gcn_mse_walks(g, self._tag, s, U, V, self.d, self._err, None, Gu, Gi, self._row_loss, st)
        self._fold_loss(e, s, st)
        if self._attr is not None:
            self._attr_term(e, s, U, Gu, st)
        src = t['G']
        for l in range(self.layers):                        # Horner: H^l = G + A H^(l-1)
            dst = t['Xa'] if l % 2 == 0 else t['Xb']
            self._layer(src, dst, t['G'], None, stream)
            src = dst
        self._sgd(e, t['W'], t['M'], src, self._c, st)

    # ---- what Scratch._train uses of a job, beside the base's ------------------------------------------------------------
    def padded_tables(self, s=0, stream=None):
        """The final tables (U*, V*) of the current parameters at the padded width: recomputed by a forward pass when read."""
        assert s == 0
        self._forward(stream)
        return self._sides(self._t['Star'])

    def tables(self, s=0, stream=None):
        U, V = self.padded_tables(s, stream)
        return U[:, :self.k], V[:, :self.k]

    def base_tables(self, padded=False):
        """The parameters (P, Q): layer 0."""
        P, Q = self._sides(self._t['W'])
        return (P, Q) if padded else (P[:, :self.k], Q[:, :self.k])

    def epoch_sse(self, s=0):
        """Per-epoch sum of squared training errors (host float64 array; synchronises)."""
        assert s == 0
        if self.loss != 'mse':
            raise ValueError(f"epoch_sse is the MSE job's: a loss={self.loss!r} job reports epoch_loss()")
        return super().epoch_sse(s)

    def epoch_loss(self, s=0):
        """Per-epoch sum of the steps' batch losses, whatever the loss (host float64 array; synchronises)."""
        return super().epoch_sse(s)

    def _attr_log(self, name):
        if self._attr is None:
            raise ValueError("the job trains without the attribute term (dis_type='nor')")
        return self._attr[name][:self.epochs].cpu().numpy()

    def epoch_dis(self, s=0):
        """Per epoch the sum of the applied steps' MMD / u2u values, before eta (host float64 array; synchronises)."""
        assert s == 0
        return self._attr_log('dis')

    def epoch_skipped(self, s=0):
        """Per epoch the steps whose term was skipped: a group absent from the batch, or no usable bandwidth (host array; synchronises)."""
        assert s == 0
        return self._attr_log('skipped').astype(np.int64)

    def close(self):
        self._pool = self._t = self._file_tags = self._tag = self._err = self._row_loss = self._sse = self._bpr = self._attr = None


# ---------------------------------------------------------------------------
# The NeuMF backbone (csrc/nmf.hip, include/ultrare_nmf.h; the contract is nmf.py)
# ---------------------------------------------------------------------------
def _nmf_layers(layers):
    """The stack as the host int32 array the entries take."""
    return np.ascontiguousarray(layers, dtype=np.int32)


def _nmf_tensor(t, shape, dtype, what, dev=None):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise nv.NativeError('nmf_score runs on the HIP device only (no CPU fallback)')
    if not (t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f'{what} must be a contiguous {dtype} {list(shape)} tensor, not {t.dtype} {list(t.shape)}')
    if dev is not None and t.device != dev:
        raise ValueError(f'{what} is on {t.device}, the tables on {dev}')
    return t


def nmf_score(U, V, dense, k, layers, uid, iid, rating=None, pred=None, sse=None, n_models_total=1, first=True, last=True, stream=None):
    """nmf.score_ref's step for ONE model (U [n_user, k + e], V [n_item, k + e], dense) at the pairs (uid, iid) int32 [n] on the
    device, under ure_score's protocol: pred (default: a new tensor; must be given unless `first`) receives the running sum, and
    on `last` the mean over n_models_total; sse (optional, float64 [SCORE_PARTIALS], with rating) the squared-error partials.
    -> pred.  Nothing synchronises."""
    from . import nmf
    S = nmf.Shape(k, layers)                                # (the ValueError of a bad stack comes before any device work)
    for t in (U, V, dense, uid, iid):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise nv.NativeError('nmf_score runs on the HIP device only (no CPU fallback)')
    dev, n = U.device, int(uid.numel())
    _nmf_tensor(U, (U.shape[0], S.wd), torch.float32, 'U')
    _nmf_tensor(V, (V.shape[0], S.wd), torch.float32, 'V', dev)
    _nmf_tensor(dense, (S.n_dense,), torch.float32, 'dense', dev)
    _nmf_tensor(uid, (n,), torch.int32, 'uid', dev)
    _nmf_tensor(iid, (n,), torch.int32, 'iid', dev)
    if n < 1:
        raise ValueError('nmf_score needs at least one pair')
    if pred is None:
        if not first:
            raise ValueError('pred holds the running sum of the models before: it must be given unless first')
        pred = torch.empty(n, dtype=torch.float32, device=dev)
        _csr_held_for(stream, pred)
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.numel() < n or pred.device != dev:
        raise ValueError(f'pred must be a contiguous float32 tensor of at least {n} elements on {dev}')
    if sse is not None:
        _nmf_tensor(sse, (SCORE_PARTIALS,), torch.float64, 'sse', dev)
        if rating is None:
            raise ValueError('sse needs the ratings')
    if rating is not None and (rating.dtype != torch.float32 or not rating.is_contiguous() or rating.numel() < n or rating.device != dev):
        raise ValueError(f'rating must be a contiguous float32 tensor of at least {n} elements on {dev}')
    lay = _nmf_layers(S.layers)
    nv.check(nv.lib().ure_nmf_score(nv.ptr(U), nv.ptr(V), nv.ptr(dense), S.k, nv.ptr(lay), len(lay), int(U.shape[0]), int(V.shape[0]),
                                    int(n_models_total), int(bool(first)), int(bool(last)), nv.ptr(uid), nv.ptr(iid), nv.ptr(rating), n, nv.ptr(pred),
                                    nv.ptr(sse), nv.stream_handle(stream)), 'ure_nmf_score')
    return pred


def _nmf_models(models, k, layers, who):
    """The checks every catalogue sweep makes of its ensemble: models = [(U, V, dense)] device tensors of ONE stack.
    -> (Shape, device, n_user, n_item, the three host pointer arrays, the host layers array)."""
    from . import nmf
    S = nmf.Shape(k, layers)                                # (the ValueError of a bad stack comes before any device work)
    models = list(models)
    if not models:
        raise ValueError(f'{who} needs at least one model')
    for m in models:
        if len(m) != 3:
            raise ValueError(f'{who}: a model is (U, V, dense), not {len(m)} tensors')
        for t in m:
            if not (torch.is_tensor(t) and t.is_cuda):
                raise nv.NativeError(f'{who} runs on the HIP device only (no CPU fallback)')
    dev, n_user, n_item = models[0][0].device, int(models[0][0].shape[0]), int(models[0][1].shape[0])
    for U, V, dense in models:
        _nmf_tensor(U, (n_user, S.wd), torch.float32, 'U', dev)
        _nmf_tensor(V, (n_item, S.wd), torch.float32, 'V', dev)
        _nmf_tensor(dense, (S.n_dense,), torch.float32, 'dense', dev)
    ptrs = tuple((ctypes.c_void_p * len(models))(*[m[j].data_ptr() for m in models]) for j in range(3))
    return S, dev, n_user, n_item, ptrs, _nmf_layers(S.layers)


def _query_users(users, n_user, who):
    users = users.detach().cpu().numpy() if torch.is_tensor(users) else np.asarray(users)
    users = users.astype(np.int64).reshape(-1)
    if users.size == 0:
        raise ValueError(f'{who} needs at least one user')
    if users.min() < 0 or users.max() >= n_user:
        raise ValueError(f'user ids outside [0, {n_user})')
    return users


def nmf_recommend(models, k, layers, users, top_k, excl=None, stream=None):
    """Top-k items of every user of `users` over the whole catalogue under a NeuMF ensemble (ure_nmf_recommend_topk; the contract
    is nmf.recommend_ref): models = [(U, V, dense)] device tensors of one (k, layers), the scores those a chain of nmf_score calls
    gives for the same pairs, bit for bit; excl = (off, items) from exclusion_rows or None.  Returns (scores [n, top_k] float32,
    items [n, top_k] int64) on the device; padding is (NaN, -1)."""
    S, dev, n_user, n_item, (Up, Vp, Dp), lay = _nmf_models(models, k, layers, 'nmf_recommend')
    if isinstance(top_k, bool) or not 1 <= int(top_k) <= RECOMMEND_MAX_K:
        raise ValueError(f'top_k = {top_k} outside [1, {RECOMMEND_MAX_K}]')
    users = _query_users(users, n_user, 'nmf_recommend')
    if excl is not None:
        off, items = _check_rows(*(t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in excl), len(users), n_item, 'exclusion')
    n, top_k = len(users), int(top_k)
    uid = to_device_async(users.astype(np.int32), dev)
    e_off = e_items = None
    if excl is not None:
        e_off = to_device_async(off, dev)
        e_items = to_device_async(items if items.size else np.zeros(1, dtype=np.int32), dev)
    L = nv.lib()
    nbytes = int(L.ure_nmf_recommend_scratch(n, n_item, top_k, len(models), S.k, nv.ptr(lay), len(lay)))
    if nbytes < 0:
        raise ValueError(f'ure_nmf_recommend_scratch refused n_query = {n}, n_item = {n_item}, top_k = {top_k}, k = {S.k}, layers = {S.layers}')
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    scores = torch.empty(n, top_k, dtype=torch.float32, device=dev)
    items_out = torch.empty(n, top_k, dtype=torch.int32, device=dev)
    _csr_held_for(stream, *(t for t in (uid, e_off, e_items, scratch, scores, items_out) if t is not None))
    nv.check(L.ure_nmf_recommend_topk(Up, Vp, Dp, len(models), S.k, nv.ptr(lay), len(lay), n_user, nv.ptr(uid), n, n_item, nv.ptr(e_off),
                                      nv.ptr(e_items), top_k, nv.ptr(scores), nv.ptr(items_out), nv.ptr(scratch), scratch.numel(),
                                      nv.stream_handle(stream)), 'ure_nmf_recommend_topk')
    return scores, items_out.long()


def nmf_rank_pairs(models, k, layers, users, targets, excl=None, stream=None):
    """Exact full-catalogue rank of every (user, target item) pair under a NeuMF ensemble (ure_nmf_rank_pairs; the contract is
    nmf.rank_ref): models as in nmf_recommend, targets = (off [n + 1], items) with query row q's targets items[off[q]:off[q + 1]]
    (any order, duplicates, empty rows), excl = (off, items) or None.  rank = the number of non-excluded items whose (score, id)
    key beats the target's -- the position nmf_recommend would give it -- or -1 for an excluded target.  Returns ranks
    [len(items)] int32 on the device, in input order."""
    S, dev, n_user, n_item, (Up, Vp, Dp), lay = _nmf_models(models, k, layers, 'nmf_rank_pairs')
    users = _query_users(users, n_user, 'nmf_rank_pairs')
    t_off, t_items = _check_rows(*(t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in targets), len(users), n_item, 'target')
    if excl is not None:
        e_off_h, e_items_h = _check_rows(*(t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in excl), len(users), n_item, 'exclusion')
    n, n_t = len(users), len(t_items)
    ranks = torch.empty(max(n_t, 1), dtype=torch.int32, device=dev)
    if n_t == 0:
        return ranks[:0]
    uid = to_device_async(users.astype(np.int32), dev)
    d_off, d_items = to_device_async(t_off, dev), to_device_async(t_items, dev)
    e_off = e_items = None
    if excl is not None:
        e_off = to_device_async(e_off_h, dev)
        e_items = to_device_async(e_items_h if e_items_h.size else np.zeros(1, dtype=np.int32), dev)
    L = nv.lib()
    nbytes = int(L.ure_nmf_rank_pairs_scratch(n, n_t, n_item, len(models), S.k, nv.ptr(lay), len(lay)))
    if nbytes < 0:
        raise ValueError(f'ure_nmf_rank_pairs_scratch refused n_query = {n}, n_targets = {n_t}, n_item = {n_item}, k = {S.k}, layers = {S.layers}')
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _csr_held_for(stream, *(t for t in (ranks, uid, d_off, d_items, e_off, e_items, scratch) if t is not None))
    nv.check(L.ure_nmf_rank_pairs(Up, Vp, Dp, len(models), S.k, nv.ptr(lay), len(lay), n_user, nv.ptr(uid), n, n_item, nv.ptr(d_off),
                                  nv.ptr(d_items), nv.ptr(e_off), nv.ptr(e_items), nv.ptr(ranks), nv.ptr(scratch), nbytes,
                                  nv.stream_handle(stream)), 'ure_nmf_rank_pairs')
    return ranks


class NmfJob(_GraphJob):
    """One shard trained with the NeuMF backbone (nmf.train_ref in float32, bit for bit): per step the forward / backward pass over
    the shard's entries (the batch's write their slot), the weight-gradient sums over the slots, the two masked row sums of the
    embedding gradients, the loss fold, and ONE SGD update of every parameter -- both tables and the dense vector are one
    contiguous run of floats, as are their momenta and gradients.  What Scratch._train uses of a TrainJob is here under the same
    names.

    graph  : GcnGraph
    init   : (U0 [n_user, k + e], V0 [n_item, k + e], dense0 [nmf.Shape(k, layers).n_dense]) float32 numpy arrays or tensors
    orders : int32 [epochs, N] -- per epoch the file positions in training order (batch t = orders[e][t B : (t + 1) B])"""

    def __init__(self, graph, init, orders, k, layers, batch, epochs, lr, lam, momentum, lr_decay=1.0, lr_step=50):
        from . import nmf
        self.shape = S = nmf.Shape(k, layers)
        self.k, self.layers = S.k, S.layers
        self._check_sizes(graph, batch, epochs)
        if len(init) != 3:
            raise ValueError('init is (U0, V0, dense0)')
        U0, V0, dense0 = (np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float32) for t in init)
        nmf.check_model(U0, V0, dense0, S.k, S.layers, graph.n_user, graph.n_item)
        file_rank = self._plan(orders, lr, lam, momentum, lr_decay, lr_step)
        self._lay = _nmf_layers(S.layers)
        dev, B = self.device, min(self.batch, graph.N)
        self._nu, self._ni = graph.n_user * S.wd, graph.n_item * S.wd
        self.n_params = self._nu + self._ni + S.n_dense
        # everything below is written before it is read (the momenta by the first step): torch.empty
        self._pool = torch.empty(3, self.n_params, dtype=torch.float32, device=dev)      # parameters, momenta, gradients
        self._pool[0].copy_(torch.from_numpy(np.concatenate([U0.reshape(-1), V0.reshape(-1), dense0])))
        self._file_rank = torch.from_numpy(file_rank).to(dev)
        self._rank = torch.empty(graph.nnz, dtype=torch.int32, device=dev)
        self._err = torch.empty(B, dtype=torch.float32, device=dev)
        self._act = torch.empty(B, S.A, dtype=torch.float32, device=dev)
        self._dlt = torch.empty(B, S.Dw, dtype=torch.float32, device=dev)
        self._emb = torch.empty(B, 2 * S.wd, dtype=torch.float32, device=dev)
        self._scratch_bytes = int(nv.lib().ure_nmf_weight_grad_scratch(B, S.k, nv.ptr(self._lay), len(self._lay)))
        self._scratch = torch.empty(self._scratch_bytes, dtype=torch.uint8, device=dev)
        self._row_loss = torch.empty(graph.n_user, dtype=torch.float64, device=dev)
        self._sse = torch.zeros(max(self.epochs, 1), dtype=torch.float64, device=dev)

    def _part(self, which):
        """(U, V, dense) views of the parameters (0), the momenta (1) or the gradients (2)."""
        g, S, t = self.graph, self.shape, self._pool[which]
        return t[:self._nu].view(g.n_user, S.wd), t[self._nu:self._nu + self._ni].view(g.n_item, S.wd), t[self._nu + self._ni:]

    def _step(self, e, s, stream=None):
        g, S, L, st = self.graph, self.shape, nv.lib(), nv.stream_handle(stream)
        if s == 0:
            self._gather(self._file_rank[e], self._rank, st)
        lo = s * self.batch
        n_slots = min(self.batch, g.N - lo)
        (U, V, dense), (gU, gV, gd) = self._part(0), self._part(2)
        lay, m = nv.ptr(self._lay), len(self._lay)
        nv.check(L.ure_nmf_forward_backward(nv.ptr(g.row_u), nv.ptr(g.col), nv.ptr(g.rating), nv.ptr(self._rank), g.nnz, lo, n_slots, U.data_ptr(),
                                            V.data_ptr(), g.n_user, g.n_item, dense.data_ptr(), S.k, lay, m, nv.ptr(self._err), None, nv.ptr(self._act),
                                            nv.ptr(self._dlt), nv.ptr(self._emb), st), 'ure_nmf_forward_backward')
        nv.check(L.ure_nmf_weight_grad(nv.ptr(self._err), nv.ptr(self._act), nv.ptr(self._dlt), n_slots, S.k, lay, m, gd.data_ptr(),
                                       nv.ptr(self._scratch), self._scratch_bytes, 0, st), 'ure_nmf_weight_grad')
        nv.check(L.ure_nmf_row_sum(nv.ptr(g.off_u), None, nv.ptr(self._rank), g.n_user, g.nnz, lo, n_slots, nv.ptr(self._emb), 2 * S.wd, 0, S.wd,
                                   nv.ptr(self._err), gU.data_ptr(), nv.ptr(self._row_loss), st), 'ure_nmf_row_sum')
        nv.check(L.ure_nmf_row_sum(nv.ptr(g.off_i), nv.ptr(g.to_csr), nv.ptr(self._rank), g.n_item, g.nnz, lo, n_slots, nv.ptr(self._emb), 2 * S.wd,
                                   S.wd, S.wd, None, gV.data_ptr(), None, st), 'ure_nmf_row_sum')
        self._fold_loss(e, s, st)
        self._sgd(e, *self._pool, 1.0, st)                  # (the pool's rows: parameters, momenta, gradients)

    def params(self):
        """(U [n_user, k + e], V [n_item, k + e], dense): views of the job's current parameters."""
        return self._part(0)

    def close(self):
        self._pool = self._file_rank = self._rank = self._err = self._act = self._dlt = self._emb = self._scratch = self._row_loss = self._sse = None


# ---------------------------------------------------------------------------
# Newton-step (influence) unlearning (csrc/influence.hip, include/ultrare_influence.h; the contract is influence.py)
# ---------------------------------------------------------------------------
def _inf_on(stream):
    import contextlib
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _inf_tables(graph, U, V, who):
    """The checks of the two float32 tables of a shard: -> d."""
    from . import lightgcn
    if not (torch.is_tensor(U) and U.is_cuda and torch.is_tensor(V) and V.is_cuda):
        raise nv.NativeError(f'{who} runs on the HIP device only (no CPU fallback)')
    d = lightgcn.check_width(int(U.shape[1]) if U.dim() == 2 else 0)
    _gcn_table(U, graph.n_user, d, 'U', graph.device)
    _gcn_table(V, graph.n_item, d, 'V', graph.device)
    return d


def _inf_f64(t, shape, what, dev):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise nv.NativeError('the influence entries run on the HIP device only (no CPU fallback)')
    if not (t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.device == dev):
        raise ValueError(f'{what} must be a contiguous float64 {list(shape)} tensor on {dev}, not {tuple(t.shape)} {t.dtype} on {t.device}')
    return t


def _inf_active(graph, active):
    """active None, or (active_u, active_i) masks (numpy or tensors; None in a slot: all rows) -> two uint8 device tensors or None."""
    if active is None:
        return None, None
    if not (isinstance(active, (tuple, list)) and len(active) == 2):
        raise ValueError('active must be None or (active_u, active_i)')
    out = []
    for a, n, what in ((active[0], graph.n_user, 'active_u'), (active[1], graph.n_item, 'active_i')):
        if a is None:
            out.append(None)
            continue
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint8)))
        if a.shape != (n,):
            raise ValueError(f'{what} must have {n} entries, not {tuple(a.shape)}')
        out.append(a.to(device=graph.device, dtype=torch.uint8).contiguous())
    return out[0], out[1]


def inf_coef(graph, U, V, P=None, Q=None, out=None, stream=None):
    """influence.coef_ref on the device: the residuals e [nnz] float64 of the CSR entries, or with a float64 direction (P, Q) the
    tangents t.  Nothing synchronises."""
    d = _inf_tables(graph, U, V, 'inf_coef')
    if (P is None) != (Q is None):
        raise ValueError('a direction is both P and Q')
    if P is not None:
        _inf_f64(P, (graph.n_user, d), 'P', graph.device)
        _inf_f64(Q, (graph.n_item, d), 'Q', graph.device)
    with _inf_on(stream):
        if out is None:
            out = torch.empty(graph.nnz, dtype=torch.float64, device=graph.device)
        _inf_f64(out, (graph.nnz,), 'out', graph.device)
        nv.check(nv.lib().ure_inf_coef(nv.ptr(graph.row_u), nv.ptr(graph.col), nv.ptr(graph.rating), graph.nnz, nv.ptr(U), nv.ptr(V), nv.ptr(P), nv.ptr(Q),
                                       graph.n_user, graph.n_item, d, nv.ptr(out), nv.stream_handle(stream)), 'ure_inf_coef')
    return out


def _inf_walks(graph, d, a, U, V, b, DU, DV, reg, XU, XV, act, outU, outV, stream):
    """Both sides of one walk: the users' rows over the CSR against (V, DV), the items' rows over the CSC against (U, DU)."""
    g, L, st = graph, nv.lib(), nv.stream_handle(stream)
    nv.check(L.ure_inf_walk(nv.ptr(g.off_u), nv.ptr(g.col), None, nv.ptr(a), nv.ptr(V), nv.ptr(b), nv.ptr(DV) if b is not None else None, float(reg),
                            nv.ptr(XU), nv.ptr(act[0]), g.n_user, g.n_item, g.nnz, d, nv.ptr(outU), st), 'ure_inf_walk')
    nv.check(L.ure_inf_walk(nv.ptr(g.off_i), nv.ptr(g.row), nv.ptr(g.to_csr), nv.ptr(a), nv.ptr(U), nv.ptr(b), nv.ptr(DU) if b is not None else None,
                            float(reg), nv.ptr(XV), nv.ptr(act[1]), g.n_item, g.n_user, g.nnz, d, nv.ptr(outV), st), 'ure_inf_walk')


def _inf_reg(l2, damping, curvature):
    from . import influence
    if curvature not in influence.CURVATURES:
        raise ValueError(f"curvature must be 'full' or 'gn', not {curvature!r}")
    l2, damping = float(l2), float(damping)
    if not (np.isfinite(l2) and l2 > 0 and np.isfinite(damping) and damping >= 0):
        raise ValueError(f'need l2 > 0 and damping >= 0, both finite, not {l2!r}, {damping!r}')
    return l2 + damping


def inf_matvec(graph, U, V, P, Q, l2, damping=0.0, curvature='full', active=None, e=None, stream=None):
    """influence.matvec_ref bit for bit: (H + 2 damping I)(P, Q) -> (HU, HV) float64 for the float32 tables (U, V) of a shard, its
    GcnGraph of the remaining triples and a float64 direction.  e: the residuals (inf_coef) when the caller holds them.  Three
    launches (four without e under 'full'); nothing synchronises."""
    d = _inf_tables(graph, U, V, 'inf_matvec')
    reg = _inf_reg(l2, damping, curvature)
    _inf_f64(P, (graph.n_user, d), 'P', graph.device)
    _inf_f64(Q, (graph.n_item, d), 'Q', graph.device)
    act = _inf_active(graph, active)
    with _inf_on(stream):
        b = None
        if curvature == 'full':
            b = inf_coef(graph, U, V, stream=stream) if e is None else _inf_f64(e, (graph.nnz,), 'e', graph.device)
        t = inf_coef(graph, U, V, P, Q, stream=stream)
        HU, HV = torch.empty_like(P), torch.empty_like(Q)
        _inf_walks(graph, d, t, U, V, b, P, Q, reg, P, Q, act, HU, HV, stream)
    return HU, HV


def inf_grad(graph, U, V, l2, active=None, e=None, stream=None):
    """influence.grad_ref bit for bit: grad F -> (gU, gV) float64, +0.0 on inactive and emptied rows."""
    d = _inf_tables(graph, U, V, 'inf_grad')
    reg = _inf_reg(l2, 0.0, 'gn')
    act = _inf_active(graph, active)
    with _inf_on(stream):
        if e is None:
            e = inf_coef(graph, U, V, stream=stream)
        _inf_f64(e, (graph.nnz,), 'e', graph.device)
        U64, V64 = U.double(), V.double()
        gU, gV = torch.empty_like(U64), torch.empty_like(V64)
        _inf_walks(graph, d, e, U, V, None, None, None, reg, U64, V64, act, gU, gV, stream)
    return gU, gV


def inf_dot(x, y, out=None, stream=None):
    """influence.dot_ref bit for bit on two float64 device tensors of one size -> float64 [1] on the device (out: where to leave
    it).  Nothing synchronises."""
    n = x.numel()
    _inf_f64(x, x.shape, 'x', x.device)
    _inf_f64(y, x.shape, 'y', x.device)
    with _inf_on(stream):
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=x.device)
        L = nv.lib()
        nbytes = L.ure_inf_dot_scratch(n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        nv.check(L.ure_inf_dot(nv.ptr(x), nv.ptr(y), n, nv.ptr(scratch), nbytes, nv.ptr(out), nv.stream_handle(stream)), 'ure_inf_dot')
    return out


def inf_objective(graph, U, V, l2, e=None, stream=None):
    """The two sums of influence.objective_ref on the device -> float64 [2] = (dot(e, e), dot(theta, theta)); F = [0] + l2 * [1]."""
    _inf_tables(graph, U, V, 'inf_objective')
    with _inf_on(stream):
        if e is None:
            e = inf_coef(graph, U, V, stream=stream)
        th = torch.cat([U.reshape(-1), V.reshape(-1)]).double()
        out = torch.empty(2, dtype=torch.float64, device=graph.device)
        inf_dot(e, e, out[0:1], stream)
        inf_dot(th, th, out[1:2], stream)
    return out


def inf_solve(graph, U, V, bU, bV, l2, damping=0.0, curvature='full', active=None, e=None, iters=512, tol=1e-8, stream=None):
    """influence.solve_ref on the device: conjugate gradients on (H + 2 damping I) x = (bU, bV) from x = 0 -> (xU, xV, log) with
    log = {'rr': the float64 residual norms per iteration, 'flag', 'iters_run', 'status'} (0 out of iterations, 1 converged, 2
    non-positive curvature).  The scalars stay on the device (ure_inf_cg_*); the host reads the flags of the log once per
    influence.LOG_BLOCK iterations to stop launching, and the rr history once at the end."""
    from . import influence
    influence.check_args(curvature, damping, 1, iters, tol, l2)              # (refuses the undamped full Hessian)
    d = _inf_tables(graph, U, V, 'inf_solve')
    reg = _inf_reg(l2, damping, curvature)
    g, dev, L, st = graph, graph.device, nv.lib(), nv.stream_handle(stream)
    _inf_f64(bU, (g.n_user, d), 'bU', dev)
    _inf_f64(bV, (g.n_item, d), 'bV', dev)
    act = _inf_active(graph, active)
    nu, n = g.n_user * d, (g.n_user + g.n_item) * d
    sides = lambda v: (v[:nu].view(g.n_user, d), v[nu:].view(g.n_item, d))
    with _inf_on(stream):
        b = None
        if curvature == 'full':
            b = inf_coef(graph, U, V, stream=stream) if e is None else _inf_f64(e, (g.nnz,), 'e', dev)
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        r = torch.cat([bU.reshape(-1), bV.reshape(-1)])
        p, Ap = r.clone(), torch.empty_like(r)
        t = torch.empty(g.nnz, dtype=torch.float64, device=dev)
        state = torch.zeros(8, dtype=torch.float64, device=dev)
        log_rr, log_flag = torch.zeros(iters, dtype=torch.float64, device=dev), torch.zeros(iters, dtype=torch.int32, device=dev)
        nbytes = L.ure_inf_dot_scratch(n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        (pU, pV), (ApU, ApV) = sides(p), sides(Ap)

        def dot(a, c, slot):
            nv.check(L.ure_inf_dot(nv.ptr(a), nv.ptr(c), n, nv.ptr(scratch), nbytes, state.data_ptr() + 8 * slot, st), 'ure_inf_dot')

        dot(r, r, 0)
        nv.check(L.ure_inf_cg_start(nv.ptr(state), float(tol), st), 'ure_inf_cg_start')
        ran, status = iters, influence.RUNNING
        for it in range(iters):
            inf_coef(graph, U, V, pU, pV, out=t, stream=stream)
            _inf_walks(graph, d, t, U, V, b, pU, pV, reg, pU, pV, act, ApU, ApV, stream)
            dot(p, Ap, 1)
            nv.check(L.ure_inf_cg_xr(nv.ptr(state), nv.ptr(x), nv.ptr(r), nv.ptr(p), nv.ptr(Ap), n, st), 'ure_inf_cg_xr')
            dot(r, r, 2)
            nv.check(L.ure_inf_cg_beta(nv.ptr(state), nv.ptr(log_rr), nv.ptr(log_flag), it, iters, st), 'ure_inf_cg_beta')
            nv.check(L.ure_inf_cg_p(nv.ptr(state), nv.ptr(p), nv.ptr(r), n, st), 'ure_inf_cg_p')
            if (it + 1) % influence.LOG_BLOCK == 0 or it + 1 == iters:
                a0 = it + 1 - ((it % influence.LOG_BLOCK) + 1)
                flags = log_flag[a0:it + 1].cpu().numpy()                      # the one read of the loop: a block of flags
                hit = np.flatnonzero(flags)
                if len(hit):
                    ran, status = a0 + int(hit[0]) + 1, int(flags[hit[0]])
                    break
        rr = log_rr[:ran].cpu().numpy()
        flag = log_flag[:ran].cpu().numpy()
    xU, xV = sides(x)
    return xU, xV, {'rr': rr, 'flag': flag, 'iters_run': ran, 'status': status}
