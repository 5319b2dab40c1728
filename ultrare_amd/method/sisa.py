"""Sisa.learn / unlearn / test with the reference's signatures (method/sisa.py:7-118).

Two execution modes, same final models and log0 (training of a shard is deterministic
and isolated, and the RNG stream is consumed in the reference's order in both):

  sequential (default)  shard after shard, with the reference's per-epoch group / total
                        tests that average the models trained so far (scratch.py:83-97).
  parallel              `param.parallel = True` (CLI --parallel 1): all shards of the
                        call share every launch (engine.TrainJob) and, when
                        torch.distributed is initialised, are spread over the ranks
                        (one process per GPU, no collective while training; trained
                        tables are exchanged once over RCCL).  The reference's per-epoch
                        test logs depend on the sequential order (they average the models
                        trained before the shard); they are rebuilt afterwards from
                        end-of-epoch snapshots (`param.epoch_logs`, default on while the
                        snapshots fit URE_SNAPSHOT_LIMIT_GB).
"""
import numpy as np
import torch
from torch import nn

from .. import engine
from ..read import as_loader
from .scratch import PERM_THREADS, Scratch, prepare_shard, snapshot_limit
from . import utils
from .utils import MF, baseTest, fit_combiner, padded_tables, rank_eval, recommend, seed_all




def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


def assign_shards(sizes, world):
    """Longest-processing-time-first placement of shards on ranks."""
    load = [0] * world
    owner = [0] * len(sizes)
    for s in sorted(range(len(sizes)), key=lambda i: (-sizes[i], i)):
        r = min(range(world), key=lambda q: (load[q], q))
        owner[s] = r
        load[r] += sizes[s]
    return owner


def prepare_owned(ids, owner, rank, train_dlist, n_user, n_item, k, epochs, on_device=True):
    """Host part of a parallel call.  Every rank walks the WHOLE RNG stream in shard
    order (the draws are data independent: 4 fills + 4 seeds per epoch per shard,
    SURVEY.md 3.4) but DRAWS only for its own shards: the generator is moved past everything
    a shard of another rank would draw (ure_host_mt_advance), so shard i starts from exactly
    the state it would have in a sequential single-process run and no rank makes a normal it
    does not train on.  (Round 3 drew the full U0 of every foreign shard on every rank -- the
    reference's per-epoch logs need the earlier shards' full user tables -- ; those now come
    from their owners with the path's one exchange: exchange_tables(full_u=True).)"""
    from .. import rng
    prepared = {}
    # the HBM layouts of the owned shards -- which training needs first -- are built at once on a worker: ONE native call for
    # all of them, side by side on host threads into pinned staging, uploaded asynchronously, plus the work units of this
    # table width (a layout a loader already holds is returned as it is)
    layouts = None
    own_ids = [i for pos, i in enumerate(ids) if owner[pos] == rank]

    def start_layouts(allocate=True):
        from ..read import plan_shard_layouts
        finish = plan_shard_layouts([as_loader(train_dlist[i]) for i in own_ids], n_user, n_item, engine._device(), k)
        fut = rng.worker_pool().submit(finish)               # (the native builder starts now ...
        if allocate:
            finish.allocate()                                #  ... and the device allocations are made beside it)
        engine.mark('layouts planned')
        return fut, finish.allocate
    # the layouts first: their native builder runs on a thread of the library's own from this call on (engine.LayoutPlan), the worker below
    # only joins it and queues the copy
    allocate_layouts = None
    if on_device:
        layouts, allocate_layouts = start_layouts(allocate=False)
    streams = rng.shard_streams(len(ids), n_user, n_item, k, epochs, True, want_seeds=True) if on_device else None
    engine.mark('streams')
    if on_device and streams is None:
        allocate_layouts()
    if streams is not None:
        # every shard's start state by skip-ahead; then, in the order of what the job waits for longest: the owned shards' model inits
        # (a worker each, started at once: rng.start_inits), the layouts (one native call on a worker, the device allocations beside
        # it), and last the permutations' buffers and chunk workers (rng.draws_batch_async: seeds by skip-ahead, chunks round robin)
        starts, end, seeds = streams
        torch.set_rng_state(end)
        futures = {}
        specs, order = [], []
        # permutation chunks: 8 epochs each for a few shards (a 5-shard call: 8 -> 13.8 / 11.7 ms learn / unlearn, 17 -> 19.7 /
        # 14.2), larger ones when many shards make many chunk uploads (16 shards: 8 -> 21.6 / 23.2, 13 -> 20.9 / 20.1;
        # ab_host.py medians, a script since removed: see git history): about 64 chunks per call.
        n_owned = sum(1 for pos in range(len(ids)) if owner[pos] == rank)
        chunk_epochs = max(8, -(-epochs * n_owned // 64))
        for pos, i in enumerate(ids):
            loader = as_loader(train_dlist[i])
            base = dict(start_state=starts[pos], n_user=n_user, n_item=n_item, k=k, epochs=epochs, with_total_test=True, seeds=seeds[pos])
            if owner[pos] == rank:
                specs.append(dict(base, n_rows=len(loader.dataset), shuffle=loader.shuffle, device=engine._device(),
                                  tags_batch=rng.tags_batch_for(len(loader.dataset), loader.batch_size),
                                  chunk_epochs=chunk_epochs))
                order.append(i)
        tasks = rng.start_inits(specs)
        engine.mark('inits started')
        # (the layouts' builder is running); the epochs' batch tags are put on their way (rng.draws_batch_async: made on the device from the
        # seeds, or by host workers); the layouts' device allocations -- which the builder's worker needs only when it is done -- come last
        # few workers, several shards each (rng.draws_batch_async): the expansion threads of a worker's native calls share
        # the rank's CPUs
        W = max(1, min(len(specs), max(2, rng.host_cpus() // 2)))
        for sp in specs:
            sp['threads'] = max(2, PERM_THREADS // W)
        allocate_layouts()                               # (the builder's worker queues the layouts' copy as soon as both are done)
        engine.mark('layouts allocated')
        futures = dict(zip(order, rng.draws_batch_async(specs, W, tasks=tasks)))
        engine.mark('draws submitted')
        shards = dict(zip(own_ids, layouts.result()))
        engine.mark('layouts')
        for pos, i in enumerate(ids):
            if i not in futures:
                continue
            prepared[i] = (shards[i], futures[i].init(), futures[i].perms())         # the permutations may still be arriving (chunks)
        engine.mark('inits')
        return prepared
    if layouts is not None:
        layouts.result()                # (tables too small to skip ahead in the stream: the draws below run one after the other)
    for pos, i in enumerate(ids):
        if owner[pos] == rank:
            if on_device:
                prepared[i] = prepare_shard(train_dlist[i], n_user, n_item, k, epochs, True, defer=True)
            else:   # host-only (tests): same draws, no HBM layout
                U0, V0 = rng.mf_init(n_user, n_item, k)
                seeds = rng.epoch_seeds(epochs, True)
                n = len(as_loader(train_dlist[i]).dataset)
                prepared[i] = (None, (U0, V0), rng.epoch_perms(seeds, n))
        else:
            rng.skip_model(n_user, n_item, k, epochs, True)
    for i, (shard, init, perms) in list(prepared.items()):      # permutations expanded in the background: collect
        if hasattr(perms, 'result'):
            prepared[i] = (shard, init, perms.result())
    return prepared


def exchange_plan(ids, owner, group_sizes, n_item, k, world):
    """Layout of the path's one collective.  A rank's segment holds, for each shard it owns (in `ids`
    order), that shard's OWN user rows [len(group_index[i]), k] followed by its item table
    [n_item, k]; segments are padded to the longest (all-gather-v as one all_gather_into_tensor).
    With full user tables (exchange_tables(full_u=True)) pass n_user for every group size.
    -> ({shard: (rank, offset in floats)}, floats per segment)."""
    fill = [0] * world
    where = {}
    for pos, i in enumerate(ids):
        r = owner[pos]
        where[i] = (r, fill[r])
        fill[r] += (group_sizes[pos] + n_item) * k
    return where, max(max(fill), 1)


def exchange_tables(models, ids, owner, rank, rows, n_item, k, device, dist, full_u=0):
    """After isolated training: ONE all-gather over RCCL/xGMI.  Every rank contributes, per shard it
    owns, the rows of U_i that belong to the shard's own users (sisa.py:55-56 reads nothing else of
    U_i) and V_i (utils.py:140-145 needs every model's item table); payloads are padded to the
    longest segment.  `rows[i]` = device int64 tensor of group_index[i].
    full_u = n_user: the WHOLE pre-merge user table of every shard travels instead of its own rows --
    what the reference's per-epoch logs (scratch.py:83-86 averages the earlier models as they are) and
    user_mat{id}.npy need of a foreign shard.  S x n_user x k floats in all: 3.9 MB at ml-1m / 5 shards,
    2.6 GB at BASELINE.json configs[3] (~30 ms on a ring of 8 over xGMI), against 28 x 20.7 M normals
    drawn per rank to rebuild them from the init stream (round 3).
    -> {shard: (U rows of its own users [len(rows[i]), k] | U [n_user, k], V [n_item, k])}, device tensors."""
    world = dist.get_world_size()
    sizes = [int(full_u) if full_u else int(rows[i].numel()) for i in ids]
    where, seg = exchange_plan(ids, owner, sizes, n_item, k, world)
    send = torch.zeros(seg, dtype=torch.float32, device=device)
    for pos, i in enumerate(ids):
        if owner[pos] == rank:
            U, V = models[i]
            o = where[i][1]
            nu = sizes[pos] * k
            send[o:o + nu] = (U if full_u else U.index_select(0, rows[i])).reshape(-1)
            send[o + nu:o + nu + n_item * k] = V.reshape(-1)
    recv = torch.empty(world * seg, dtype=torch.float32, device=device)
    if dist.get_backend() == 'nccl':
        dist.all_gather_into_tensor(recv, send)
    else:       # rehearsal transports (gloo): staged through the host
        host = torch.empty(world * seg, dtype=torch.float32)
        dist.all_gather_into_tensor(host, send.cpu())
        recv.copy_(host)
    out = {}
    for pos, i in enumerate(ids):
        r, o = where[i]
        base = r * seg + o
        nu = sizes[pos] * k
        out[i] = (recv[base:base + nu].view(sizes[pos], k), recv[base + nu:base + nu + n_item * k].view(n_item, k))
    return out


class Sisa(Scratch):
    def __init__(self, param={}, model_type='mf', n_group=5, group_index=[]):
        super(Sisa, self).__init__(param, model_type)
        self.n_group = n_group
        self.group_index = group_index
        self.parallel = bool(getattr(param, 'parallel', False))
        if self.model_type in ('lightgcn', 'nmf', 'wmf'):
            self._gcn_one_rank()
            if self.parallel:           # a GcnJob / NmfJob / WmfSweeps holds one shard: the shards train one after the other
                import warnings
                warnings.warn(f"model_type={self.model_type!r} trains its shards one after the other: parallel is ignored")
                self.parallel = False
        self.epoch_logs = bool(getattr(param, 'epoch_logs', True))   # parallel mode: rebuild the per-epoch test logs
        self.model_list = []
        self.combiner = None
        self.folded = {}                # user -> group of the users fold_in added since the last learn

    def _gcn_one_rank(self):
        dist = _dist()
        if self.model_type in ('lightgcn', 'nmf', 'wmf') and dist is not None and dist.get_world_size() > 1:
            raise ValueError(f"model_type={self.model_type!r} runs on one rank, not {dist.get_world_size()}")

    def _refuse_nmf(self, who):
        """`who` is defined for models scored as the dot product of two tables."""
        if getattr(self, 'model_type', 'mf') == 'nmf':
            raise ValueError(f"Sisa.{who} needs a model scored as the dot product of two tables ('mf' or 'lightgcn'), not the 'nmf' backbone")

    def test(self, test_data, verbose, save_dir):
        dist = _dist()
        if dist is not None and self.parallel:
            # several ranks hold the same merged models: rank 0 tests, the three numbers travel (every rank ran this test in round 3)
            box = [baseTest(test_data, self.model_list, nn.MSELoss(reduction='sum'), self.device, verbose) if dist.get_rank() == 0 else None]
            dist.broadcast_object_list(box, src=0)
            rmse, ndcg, hr = box[0]
        else:
            rmse, ndcg, hr = baseTest(test_data, self.model_list, nn.MSELoss(reduction='sum'), self.device, verbose)
        log = {'total_rmse': rmse,
               'total_ndcg': ndcg,
               'total_hr': hr}
        if len(save_dir) > 0:
            np.save(save_dir + '/log0', log)
        self.log0 = log

    def fit_combiner(self, train_dlist, link='linear', l2=0.0, per_group=True):
        """Fit the weights that combine the shard models (utils.fit_combiner over self.model_list) on the CURRENT training
        loaders and keep them in self.combiner.  per_group: one weight row per shard's user group (loader g holds group g's
        pairs, as learn takes them), else one row for all.  learn and unlearn drop the combiner: its weights were fitted on
        ratings a deletion removes, so it is refitted on the post-deletion train_dlist.  Every rank of a parallel run holds
        the merged models and fits its own (bitwise the same)."""
        from ..combine import check_fit_args
        self._refuse_nmf('fit_combiner')
        check_fit_args(link, l2, 25, 1e-10)
        if len(train_dlist) != self.n_group:
            raise ValueError(f'{len(train_dlist)} training loaders for {self.n_group} groups')
        if not self.model_list:
            raise ValueError('fit_combiner needs trained models: call learn first')
        self.combiner = fit_combiner(self.model_list, list(train_dlist), link, l2, groups=self.group_index if per_group else None)
        return self.combiner

    def test_combined(self, test_data, verbose, save_dir):
        """Sisa.test with the fitted weights: (rmse, ndcg, hr), kept in self.log0c and saved as log0c.npy beside log0.npy.
        Sisa.test and log0 stay the mean's."""
        self._refuse_nmf('test_combined')
        self._need_combiner()
        rmse, ndcg, hr = baseTest(test_data, self.model_list, nn.MSELoss(reduction='sum'), self.device, verbose, combiner=self.combiner)
        self.log0c = {'total_rmse': rmse, 'total_ndcg': ndcg, 'total_hr': hr}
        if len(save_dir) > 0:
            np.save(save_dir + '/log0c', self.log0c)
        return rmse, ndcg, hr

    # ------------------------------------------------------------------ helpers
    def _need_combiner(self):
        """self.combiner, or the ValueError of every call that scores with the fitted weights."""
        if getattr(self, 'combiner', None) is None:
            raise ValueError('no combiner: call fit_combiner after learn / unlearn (a deletion drops the fitted weights)')
        return self.combiner

    def _rows_dev(self, i):
        """group_index[i] as a device int64 tensor; all groups go up together, once per (group_index object, its group sizes, device):
        the reference reads self.group_index at every merge (sisa.py:55-56), so a reassigned list or another current device must not
        find the rows of the old one.  (Groups edited in place at equal length are not detected: call forget_rows().)"""
        dev = engine._device()
        key = (id(self.group_index), tuple(len(g) for g in self.group_index), str(dev))
        if getattr(self, '_group_rows_key', None) != key:
            self._group_rows = engine.upload_many([np.asarray(g, dtype=np.int64) for g in self.group_index], dev)
            self._group_rows_key = key
        return self._group_rows[i]

    def forget_rows(self):
        self._group_rows_key = None

    def _check_closed(self):
        """The job of the last request is destroyed on a worker (ure_job_destroy waits for the device); a failure there surfaces at the
        start of the next request or here."""
        fut, self._closing = getattr(self, '_closing', None), None
        if fut is not None:
            fut.result()

    def _merge(self, merged, ids):
        """sisa.py:52-58 / 107-113: merged[group_index[i]] = U_i[group_index[i]]; for 'nmf' both user tables (sisa.py:39-50, 92-104),
        merged = {attribute name: table}."""
        if self.model_type == 'nmf':
            for name, table in merged.items():
                for i in ids:
                    engine.merge_rows(table, getattr(self.model_list[i], name).weight.detach().contiguous(), self._rows_dev(i))
                for m in self.model_list:
                    getattr(m, name).weight = nn.Parameter(table, requires_grad=False)
            return
        for i in ids:
            src = self.model_list[i].user_mat.weight.detach().contiguous()
            engine.merge_rows(merged, src, self._rows_dev(i))
        for m in self.model_list:
            m.user_mat.weight = nn.Parameter(merged, requires_grad=False)

    def _train_parallel(self, ids, train_dlist, test_dlist, test_data, verbose, save_dir, unlearning=False):
        """Train the shards `ids` side by side (and across ranks).  With epoch_logs the tables of
        every epoch end are kept on the device and the reference's per-epoch group / total tests
        (scratch.py:83-97: mean of the models trained BEFORE this shard + this shard's model of
        that epoch) are computed afterwards, so log{id}.npy carries the same series as a
        sequential run."""
        seed_all(self.seed)
        self._check_closed()
        engine.mark('start')
        # The shards' worker threads (draws, permutation chunks, uploads) run short pieces of Python between native calls; with
        # CPython's default switch interval (5 ms) this thread can wait that long for the GIL every time it comes back from a
        # native call of its own -- 10 ms between two marks of a 16-shard call.  A short interval for the duration of the call.
        import sys
        switch = sys.getswitchinterval()
        sys.setswitchinterval(2e-4)
        from .. import rng
        try:
            with rng.torch_threads():
                return self._train_parallel_body(ids, train_dlist, test_dlist, test_data, verbose, save_dir, unlearning)
        finally:
            sys.setswitchinterval(switch)

    def _train_parallel_body(self, ids, train_dlist, test_dlist, test_data, verbose, save_dir, unlearning):
        dist = _dist()
        world = dist.get_world_size() if dist else 1
        rank = dist.get_rank() if dist else 0
        sizes = [len(as_loader(train_dlist[i]).dataset) for i in ids]
        owner = assign_shards(sizes, world)
        # full pre-merge user tables of other ranks' shards are needed for the reference's per-epoch logs
        # (scratch.py:83-86 averages the earlier models as they are) and for user_mat{id}.npy on rank 0
        want_full = bool(dist) and (self.epoch_logs or len(save_dir) > 0)          # (the same on every rank: it sizes the collective)
        prepared = prepare_owned(ids, owner, rank, train_dlist, self.n_user, self.n_item, self.k, self.epochs)
        mine = [i for pos, i in enumerate(ids) if owner[pos] == rank]
        snap_mode = self._snap_mode()
        snap_bytes = engine.TrainJob.snapshot_bytes([prepared[i][0] for i in mine], self.epochs, self.k, snap_mode)
        keep_logs = self.epoch_logs and snap_bytes <= snapshot_limit()
        if self.epoch_logs and not keep_logs:
            import warnings
            warnings.warn(f'per-epoch test logs of this call are NaN: {snap_bytes / 2**30:.1f} GiB of end-of-epoch snapshots '
                          f'exceed URE_SNAPSHOT_LIMIT_GB ({snapshot_limit() / 2**30:.3g}); train_loss and log0 are complete')
        models, job = {}, None
        if mine:
            batch = as_loader(train_dlist[mine[0]]).batch_size
            job = engine.TrainJob([prepared[i][0] for i in mine], [prepared[i][1] for i in mine],
                                  [prepared[i][2] for i in mine], self.k, batch, self.epochs, self.lr, self.lam,
                                  self.momentum, self.lr_decay, snapshots=snap_mode if keep_logs else False,
                                  final_only=True, **self._optimizer_args())       # (the tables are read once, after the last epoch)
            from .. import rng
            engine.mark('job_created')
            job.run()
            self._rows_dev(mine[0])             # (the merge's row lists go up while the device works through the launches)
            engine.mark(f'launched (waited {job.chunk_wait_s * 1e3:.2f} ms for permutation chunks)')
            for i in mine:
                rng.release(prepared[i][2])                 # uploaded: host buffers go back to the pool

        # ---- the per-epoch test series, shard after shard in the reference's order (one dict for all shards)
        out, queued = {}, {}
        # the results of all series of the call in one device tensor: read with ONE copy below
        # (and the per-epoch training losses behind them: ONE device tensor, ONE copy to the host for the whole call)
        n_res = len(mine) * 6 * self.epochs if keep_logs else 0
        flat = torch.zeros(n_res + len(mine) * self.epochs, dtype=torch.float64, device=engine._device()) if mine else None
        res_all = flat[:n_res].view(len(mine), 2, self.epochs, 3) if (mine and keep_logs) else None
        if mine:
            job.epoch_sse_queue(out=flat[n_res:].view(len(mine), self.epochs))         # (one launch, right behind the last step)

        def queue_series(fixed_of):
            """Every shard's two test series (scratch.py:83-97) go into the queue, all on the current stream (the shards' series on four
            streams were measured: the events cost more than such short chains overlap -- NOTES r4 6); fixed_of(j) = the padded (U, V) of
            shard j's final model.
            Member e of shard i's series is the mean over an ensemble of FIXED models -- learn: the shards trained before i
            (scratch.py:83-86); unlearn: every shard's model, retrained if it came before i in this call, else the old one (sisa.py:89) --
            and i's own model after epoch e.  The fixed models' share is the same sum for every epoch and nearly the same for every
            shard: each distinct model is scored ONCE on the total test set (engine.ScoreCache) and a shard's base is the sum of
            those vectors in the ensemble's order -- the additions ure_score makes, so every number of every series is unchanged --
            instead of scoring i models again for shard i: S instead of S^2 / 2 table passes (S^2 when unlearning), which at
            BASELINE.json configs[3] (32 shards, 2.5 M test pairs, d = 128) was 1.3 TB of gathers per learn."""
            if not keep_logs:
                return
            total_ev = as_loader(test_data).eval_set()
            cache = engine.ScoreCache(total_ev, job.d)
            old = {}

            def old_tables(j):
                if j not in old:
                    old[j] = padded_tables(self.model_list[j])[:2]
                return old[j]
            for i in mine:
                test_ev = as_loader(test_dlist[i]).eval_set()
                if unlearning:                              # sisa.py:89: the shards before i in the retraining order are already replaced
                    replaced = set(ids[:ids.index(i)])
                    before = [(('new', j), fixed_of, j) if j in replaced else (('old', j), old_tables, j) for j in range(len(self.model_list))]
                else:
                    before = [(('new', j), fixed_of, j) for j in ids[:ids.index(i)]]
                pos = mine.index(i)
                res = res_all[pos]
                if test_ev.subset_of(total_ev) is not None and cache.fits(len({key for key, _, _ in before}) + len(cache.vec)):
                    fixed = cache.base(before)
                else:                                       # (the shard's own set is not the total set's rows of its users: two series, models scored per series)
                    fixed = [get(j) for _, get, j in before]
                job.evaluate_series_pair(pos, test_ev, total_ev, fixed, res[0], res[1])
                queued[i] = pos

        if mine and not dist:
            # one process: every final model is in the job's own tables -- the series are queued from THOSE, right behind the last
            # launch, and the copies the caller keeps are made while the device works through them (made first, the device sat idle for
            # 0.7 ms of a 5-shard request between its last step and its first series)
            queue_series(lambda j: job.padded_tables(mine.index(j)))
            engine.mark('series_queued')
        if mine:
            for pos, i in enumerate(mine):
                U, V = job.tables(pos)
                models[i] = (U.clone().contiguous(), V.clone().contiguous())
        if dist:
            # the only exchange of the path (sisa.py:52-58): own user rows + item table of every shard, one all-gather
            dev = engine._device()
            rows = {i: self._rows_dev(i) for i in ids}
            got = exchange_tables(models, ids, owner, rank, rows, self.n_item, self.k, dev, dist, full_u=self.n_user if want_full else 0)
            for pos, i in enumerate(ids):
                if owner[pos] == rank:
                    continue
                Ur, V = got[i]
                if want_full:      # the owner's whole pre-merge table (rows of other shards' users included: they only decayed there)
                    U = Ur.clone()
                else:              # only the shard's own rows are ever read again (merge + final test)
                    U = torch.zeros(self.n_user, self.k, dtype=torch.float32, device=dev)
                    U.index_copy_(0, rows[i], Ur)
                models[i] = (U, V.clone())
        out.update({i: MF.from_tables(*models[i]) for i in ids})
        engine.mark('models')
        logs = {}
        if dist:
            queue_series(lambda j: padded_tables(out[j])[:2])
            engine.mark('series_queued')
        # two copies for the whole call (a copy per shard and kind was a synchronisation each; medians of 6 of ab_host.py,
        # since removed:
        # 13.5 / 12.2 -> 12.1 / 12.2 ms learn / unlearn at 5 shards, within the noise at 16)
        if mine:
            from .. import rng
            stage = rng.SMALL.take((flat.numel(),), torch.float64)
            stage.copy_(flat, non_blocking=True)
            if stage.is_pinned():
                torch.cuda.current_stream(engine._device()).synchronize()
            host = stage.numpy().copy()
            rng.SMALL.give(stage)
            rng.device_tags_check([prepared[i][2] for i in mine])       # (the device is idle here: one tiny read)
            res_host = host[:n_res].reshape(len(mine), 2, self.epochs, 3) if keep_logs else None
            sse_host = host[n_res:].reshape(len(mine), self.epochs)
        for pos, i in enumerate(mine):
            entry = {'train_loss': np.sqrt(sse_host[pos] / prepared[i][0].N).tolist()}
            if keep_logs:
                for c, key in enumerate(('test_rmse', 'test_ndcg', 'test_hr')):
                    entry[key] = res_host[pos, 0, :, c].tolist()
                for c, key in enumerate(('total_rmse', 'total_ndcg', 'total_hr')):
                    entry[key] = res_host[pos, 1, :, c].tolist()
            else:
                nan = [float('nan')] * self.epochs
                for key in ('test_rmse', 'test_ndcg', 'test_hr', 'total_rmse', 'total_ndcg', 'total_hr'):
                    entry[key] = list(nan)
            logs[i] = entry
        engine.mark('logs_read')
        if job is not None:
            # the job's device memory is returned by a worker: ure_job_destroy waits for the device and takes 0.2-0.4 ms, and
            # nothing below needs it (the models are copies, the logs are on the host)
            from .. import rng
            self._closing = rng.worker_pool().submit(job.close)
        engine.mark('job_closed')
        if dist:
            gathered = [None] * world
            dist.all_gather_object(gathered, logs)
            logs = {k: v for part in gathered for k, v in part.items()}
        for i in ids:
            if rank == 0 and verbose in (1, 2):
                # the lines the sequential path prints while it trains (scratch.py:99-118), shard after shard in the reference's order
                from .scratch import print_epoch
                print('Using device:', self.device)
                e = logs[i]
                for t in range(self.epochs):
                    print_epoch(verbose, t, self.epochs, e['train_loss'][t], (e['test_rmse'][t], e['test_ndcg'][t], e['test_hr'][t]),
                                (e['total_rmse'][t], e['total_ndcg'][t], e['total_hr'][t]), True, '00:00:00')
            for key, vals in logs[i].items():
                self.log[key] += vals
            self.log['time'] += ['00:00:00'] * self.epochs
            if rank == 0:
                self.save(out[i], save_dir, i + 1)
        engine.mark('logs_appended')
        return out

    # ------------------------------------------------------------------ learn
    def learn(self, train_dlist, test_dlist, test_data, verbose, save_dir):
        '''
        train_dlist:   list of dataloader[n_group]
        '''
        self._gcn_one_rank()
        self.combiner = None            # fitted on the models this call replaces
        self.folded = {}                # the folded rows are replaced with the tables
        assert len(train_dlist) == self.n_group
        assert len(test_dlist) == self.n_group

        if self.parallel:
            trained = self._train_parallel(list(range(self.n_group)), train_dlist, test_dlist, test_data, verbose, save_dir)
            self.model_list = [trained[i] for i in range(self.n_group)]
        else:
            for i in range(self.n_group):
                given_model = ''
                model = super(Sisa, self).train(train_dlist[i], test_dlist[i], test_data, verbose, save_dir, i + 1, given_model)
                self.model_list.append(model)

        # merge user mat (sisa.py:52-58)
        merged = self._merge_target(self.model_list[0], zero=True)
        self._merge(merged, range(self.n_group))
        engine.mark('merged')

        # total test
        self.test(test_data, verbose, save_dir)
        engine.mark('tested')
        return self.model_list

    def _merge_target(self, model, zero=False):
        """What _merge writes into: a new table shaped as (zero) or copied from `model`'s user table -- for 'nmf' one per user table."""
        make = (lambda t: torch.zeros_like(t.detach()).contiguous()) if zero else (lambda t: t.detach().clone().contiguous())
        if self.model_type == 'nmf':
            return {name: make(getattr(model, name).weight) for name in ('user_mat_mf', 'user_mat_mlp')}
        return make(model.user_mat.weight)

    # ------------------------------------------------------------------ fold-in
    def _merged_table(self):
        """The one merged user table, with every model pointed at it (models handed to unlearn may be copies)."""
        merged = self.model_list[0].user_mat.weight.detach()
        if not merged.is_contiguous():
            merged = merged.contiguous()
        for m in self.model_list:
            if m.user_mat.weight.data_ptr() != merged.data_ptr():
                m.user_mat.weight = nn.Parameter(merged, requires_grad=False)
        return merged

    def _set_rows(self, users, rows=None):
        """merged[users] = rows (zero without rows) through engine.merge_rows."""
        merged = self._merged_table()
        at = engine.to_device_async(np.asarray(users, dtype=np.int64), merged.device)
        src = torch.zeros_like(merged)
        if rows is not None:
            src.index_copy_(0, at, rows)
        engine.merge_rows(merged, src, at)

    def fold_in(self, data, l2, groups=None, l2_n=0.0, against='home'):
        """Add the users of `data` (a loader, or a (uid, iid, rating / 5) triple) between retrainings, without training: each
        gets the ridge row of its ratings against frozen item tables (utils.fold_in; utils.trainer_l2 gives the l2 of the
        trainer's own fixed point).  groups: one group id per distinct user, in ascending user id; None sends each user, in
        ascending id, to the currently smallest group (lowest id on ties), which keeps the balance the grouping bought.
        against='home': the item table of the user's group -- how every trained user's row came to be, so the row behaves like
        its neighbours under the mean and under any combiner; 'ensemble': the mean item table, which minimises the error of the
        score actually served.  The rows go into the merged user table all models share, the users are appended to
        group_index[g] and recorded in self.folded[user] = g, and a fitted combiner is dropped (its group lists no longer cover
        the users).  A user that a group already lists, or with an id >= n_user (the tables do not grow), is refused with
        ValueError before any device work.  Returns (users ascending int64, their groups int64).  forget_folded deletes them
        exactly."""
        from ..ridge import check_ridge_args
        self._refuse_nmf('fold_in')
        check_ridge_args(l2, l2_n)
        if against not in ('home', 'ensemble'):
            raise ValueError(f"against must be 'home' or 'ensemble', not {against!r}")
        if not self.model_list:
            raise ValueError('fold_in needs trained models: call learn first')
        uid, iid, r = utils._rating_triple(data)
        users = np.unique(uid)
        if len(users) == 0:
            raise ValueError('fold_in needs at least one rating')
        if users[0] < 0 or users[-1] >= self.n_user:
            raise ValueError(f'users {users[(users < 0) | (users >= self.n_user)].tolist()} outside [0, {self.n_user}): the tables do not grow')
        if len(iid) and (iid.min() < 0 or iid.max() >= self.n_item):
            raise ValueError(f'items outside [0, {self.n_item})')
        listed = np.zeros(self.n_user, dtype=bool)
        for g in self.group_index:
            ids = np.asarray(g, dtype=np.int64)
            listed[ids[(ids >= 0) & (ids < self.n_user)]] = True
        if listed[users].any():
            raise ValueError(f'users {users[listed[users]].tolist()} are already in a group: unlearn them first')
        if groups is None:
            sizes = [len(g) for g in self.group_index]
            home = np.empty(len(users), dtype=np.int64)
            for q in range(len(users)):
                g = min(range(self.n_group), key=lambda c: (sizes[c], c))
                home[q] = g
                sizes[g] += 1
        else:
            home = np.asarray(groups).reshape(-1)
            if len(home) != len(users):
                raise ValueError(f'{len(home)} group ids for {len(users)} distinct users')
            if not np.issubdtype(home.dtype, np.integer) or (home < 0).any() or (home >= self.n_group).any():
                raise ValueError(f'group ids must be integers in 0 .. {self.n_group - 1}')
            home = home.astype(np.int64)
        # ---- device work
        if against == 'ensemble':
            got, rows = utils.fold_in(self.model_list, (uid, iid, r), l2, l2_n, 'mean')
            assert np.array_equal(got, users)
            self._set_rows(users, rows)
        else:
            of_user = np.full(self.n_user, -1, dtype=np.int64)
            of_user[users] = home
            for g in np.unique(home):
                pick = of_user[uid] == g
                got, rows = utils.fold_in(self.model_list, (uid[pick], iid[pick], r[pick]), l2, l2_n, int(g))
                self._set_rows(got, rows)
        for g in np.unique(home):
            self.group_index[g] = list(self.group_index[g]) + users[home == g].tolist()
        self.forget_rows()
        self.folded.update({int(u): int(g) for u, g in zip(users, home)})
        self.combiner = None
        return users, home

    def forget_folded(self, users):
        """Exact deletion of users that fold_in added, without retraining: a folded row depends on nothing but frozen item
        tables and the user's own ratings, and no other parameter depends on it.  Zeroes their rows, removes them from their
        group's list and from self.folded, and drops a fitted combiner.  ValueError (before any change) when some user was not
        folded in, listing those that need unlearn."""
        users = np.unique(np.asarray(list(users), dtype=np.int64).reshape(-1))
        trained = [int(u) for u in users if int(u) not in self.folded]
        if trained:
            raise ValueError(f'users {trained} were not folded in: deleting them needs unlearn')
        if len(users) == 0:
            return
        self._set_rows(users)
        gone = set(users.tolist())
        for g in sorted({self.folded[int(u)] for u in users}):
            self.group_index[g] = [u for u in self.group_index[g] if int(u) not in gone]
        for u in users:
            del self.folded[int(u)]
        self.forget_rows()
        self.combiner = None

    # ------------------------------------------------------------------ attribute unlearning
    def _own_sides(self, rows, n1):
        """(s, sa, sb) per shard: the users of rows[:n1] and of rows[n1:] that group_index[s] lists, in the order given."""
        a, b = rows[:n1].astype(np.int64), rows[n1:].astype(np.int64)
        for s in range(self.n_group):
            own = np.zeros(self.n_user, dtype=bool)
            ids = np.asarray(self.group_index[s], dtype=np.int64)
            own[ids[(ids >= 0) & (ids < self.n_user)]] = True
            yield s, a[own[a]], b[own[b]]

    def attribute_unlearn(self, id1, id2, **kw):
        """Make the user rows of the attribute groups id1 and id2 indistinguishable, shard by shard, without retraining
        (utils.attribute_unlearn; its keywords pass through).  Shard s fine-tunes the rows of its OWN users only --
        group_index[s] & id1 against group_index[s] & id2, in the order id1 / id2 list them -- in the merged user table all
        models share, so a row is moved by the shard that trained it and by no other; users no shard lists are not touched.
        A shard where either side is empty is skipped.  Returns one entry per shard: utils.attribute_unlearn's log plus
        'rows' (n1, n2), or {'skipped': reason, 'rows': (n1, n2)}.  A fitted combiner is dropped (its weights were fitted on
        the rows this call moves); test, recommend, rank_eval and unlearn read the table itself and see the new rows.
        ValueError before any device work for groups that are empty, overlap, repeat a user or leave the table."""
        from ..attr_unlearn import check_groups
        self._refuse_nmf('attribute_unlearn')
        if not self.model_list:
            raise ValueError('attribute_unlearn needs trained models: call learn first')
        rows, n1, _ = check_groups(id1, id2, self.n_user)
        utils.attribute_unlearn_check(**kw)
        self._merged_table()
        logs = []
        for s, sa, sb in self._own_sides(rows, n1):
            if len(sa) == 0 or len(sb) == 0:
                logs.append({'skipped': f'shard {s} holds {len(sa)} users of id1 and {len(sb)} of id2: both sides need one', 'rows': (len(sa), len(sb))})
                continue
            log = utils.attribute_unlearn(self.model_list[s], sa, sb, **kw)
            log['rows'] = (len(sa), len(sb))
            logs.append(log)
        self.forget_rows()
        self.combiner = None
        return logs

    def adversarial_unlearn(self, id1, id2, **kw):
        """Adversarial attribute unlearning, shard by shard on the merged user table (utils.adversarial_unlearn; its keywords pass
        through), exactly as attribute_unlearn goes: shard s plays the game on the rows of its OWN users only -- group_index[s] & id1
        against group_index[s] & id2 -- so a row is moved by the shard that trained it and by no other, and retraining another
        shard later stays exact.  A shard with fewer than `folds` users on either side is skipped with a reason (every held-out
        part needs both classes).  Returns one entry per shard: utils.adversarial_unlearn's log plus 'rows' (n1, n2), or
        {'skipped': reason, 'rows': (n1, n2)}.  A fitted combiner is dropped, also when a shard raises after rows have moved (a NaN
        p is found at a shard's end: the shards before it keep their moved rows).  ValueError before any device work for bad groups
        or settings."""
        from ..adv_unlearn import DEFAULTS, check_loop
        from ..attack import MAX_FOLDS, MAX_H, _int
        from ..attr_unlearn import check_groups
        self._refuse_nmf('adversarial_unlearn')
        if not self.model_list:
            raise ValueError('adversarial_unlearn needs trained models: call learn first')
        unknown = set(kw) - set(DEFAULTS)
        if unknown:
            raise TypeError(f'adversarial_unlearn got unexpected keywords {sorted(unknown)}')
        want = {**DEFAULTS, **kw}
        check_loop(want['rounds'], want['disc_epochs'], want['disc_lr'], want['l2'], want['lr'], want['eta'], want['alpha'], want['target'])
        _int('hidden', want['hidden'], 0, MAX_H)
        folds = _int('folds', want['folds'], 2, MAX_FOLDS)
        rows, n1, _ = check_groups(id1, id2, self.n_user)
        self._merged_table()
        logs = []
        try:
            for s, sa, sb in self._own_sides(rows, n1):
                if min(len(sa), len(sb)) < folds:
                    logs.append({'skipped': f'shard {s} holds {len(sa)} users of id1 and {len(sb)} of id2: both sides need folds = {folds}',
                                 'rows': (len(sa), len(sb))})
                    continue
                log = utils.adversarial_unlearn(self.model_list[s], sa, sb, **kw)
                log['rows'] = (len(sa), len(sb))
                logs.append(log)
        finally:            # (a shard that raises at its end -- a NaN p -- has moved rows already, as may the shards before it)
            self.forget_rows()
            self.combiner = None
        return logs

    def attribute_attack(self, id1, id2, **kw):
        """How well an adversary tells the attribute groups id1 and id2 apart from the merged user table (utils.attribute_attack; its
        keywords pass through): the cross-validated probe's out-of-fold AUC / BAcc / F1.  It changes no state: the tables keep their
        bytes, no forget_rows, and a fitted combiner is kept.  The 'nmf' backbone has two user tables: pass one (or a torch.cat of
        both) to utils.attribute_attack."""
        if not self.model_list:
            raise ValueError('attribute_attack needs trained models: call learn first')
        return Scratch.attribute_attack(self, self.model_list[0], id1, id2, **kw)

    # ------------------------------------------------------------------ unlearn
    def recommend(self, users, top_k=10, exclude=None, combined=False):
        """Top-k items per user from the current ensemble (utils.recommend over self.model_list): after unlearn it answers
        from the retrained shards.  Every rank of a parallel run holds the merged models and answers its own queries.
        The 'nmf' backbone is answered by recommend_nmf.  combined=True ranks under self.combiner's weights (the ensemble
        test_combined reports) and raises test_combined's ValueError without one: learn, unlearn, fold_in and
        attribute_unlearn drop it."""
        self._refuse_nmf('recommend')
        return recommend(self.model_list, users, top_k, exclude, combiner=self._need_combiner() if combined else None)

    def recommend_nmf(self, users, top_k=10, exclude=None):
        """recommend for the 'nmf' backbone (utils.recommend_nmf over self.model_list): the same return values and padding, the
        scores those baseTest gives a NeuMF ensemble; after unlearn it answers from the retrained shards."""
        return utils.recommend_nmf(self.model_list, users, top_k, exclude)

    def rank_eval(self, test_data, exclude=None, ks=(10, 20), combined=False):
        """Full-ranking HR@K / Recall@K / NDCG@K / MRR of the current ensemble on a test loader (utils.rank_eval over
        self.model_list): after unlearn it evaluates the retrained shards.  Every rank of a parallel run holds the merged models
        and answers for itself.  The 'nmf' backbone is evaluated by rank_eval_nmf.  combined=True: under self.combiner's
        weights, as recommend(combined=True)."""
        self._refuse_nmf('rank_eval')
        return rank_eval(self.model_list, test_data, exclude, ks, combiner=self._need_combiner() if combined else None)

    def rank_eval_nmf(self, test_data, exclude=None, ks=(10, 20)):
        """rank_eval for the 'nmf' backbone (utils.rank_eval_nmf over self.model_list): the same metrics over the whole catalogue;
        after unlearn it evaluates the retrained shards."""
        return utils.rank_eval_nmf(self.model_list, test_data, exclude, ks)

    def unlearn(self, model_list, train_dlist, test_dlist, test_data, del_user, verbose, save_dir):
        '''
        train_dlist:   list of dataloader[n_group]

        A user that fold_in added is deleted exactly and without retraining by forget_folded.  Passed here, it retrains its
        home shard like any other user; the folded users of every retrained shard leave self.folded, since their rows now
        come from that shard's training.
        '''
        self._gcn_one_rank()
        self.combiner = None            # fitted on the deleted users' ratings: refit on the post-deletion loaders
        self.model_list = model_list

        assert len(train_dlist) == self.n_group
        assert len(test_dlist) == self.n_group

        # find deletion (sisa.py:76-81: the first group that lists the user)
        first_group = np.full(max(self.n_user, 1 + max((int(max(g)) for g in self.group_index if len(g)), default=0)), -1, dtype=np.int64)
        for i in reversed(range(self.n_group)):
            first_group[np.asarray(self.group_index[i], dtype=np.int64)] = i
        users = np.asarray(list(del_user), dtype=np.int64).reshape(-1)
        users = users[(users >= 0) & (users < len(first_group))]
        retrain_gid = set(int(g) for g in np.unique(first_group[users]) if g >= 0)
        self.folded = {u: g for u, g in getattr(self, 'folded', {}).items() if g not in retrain_gid}

        model_before_unlearn = model_list[0]
        merged = self._merge_target(model_before_unlearn)

        if self.parallel:
            ids = list(retrain_gid)
            trained = self._train_parallel(ids, train_dlist, test_dlist, test_data, verbose, save_dir, unlearning=True) if ids else {}
            for i in ids:
                self.model_list[i] = trained[i]
        else:
            for i in retrain_gid:
                given_model = ''
                model = super(Sisa, self).train(train_dlist[i], test_dlist[i], test_data, verbose, save_dir, i + 1, given_model)
                self.model_list[i] = model

        # merge user mat (sisa.py:107-113): only the retrained shards' rows change
        self._merge(merged, list(retrain_gid))

        # total test
        self.test(test_data, verbose, save_dir)
        self.retrained = sorted(retrain_gid)
        return self.model_list

    def unlearn_influence(self, model_list, train_dlist, test_data, del_user, verbose, save_dir, **kw):
        '''
        Approximate unlearning without retraining: every shard that holds a deleted user -- found exactly as unlearn
        finds them -- takes utils.newton_unlearn's damped Newton steps on its post-deletion loader train_dlist[i], over its OWN rows
        of the merged user table and its item table; the rows go back into the merged table, where the deleted users' rows are zero.
        kw: newton_unlearn's keywords (l2 None: trainer_l2 of the shard's remaining ratings with the trainer's batch and lam).
        self.influenced lists the updated shards and self.influence_logs their per-step logs; self.retrained is empty; a fitted
        combiner is dropped and folded is kept as unlearn keeps it.  More than one rank and model_type='lightgcn' (or loss='bpr') are
        refused before any device work.  unlearn itself is untouched and may follow.
        '''
        from ..influence import check_model
        if getattr(self, 'dis_type', 'nor') != 'nor':
            raise ValueError(f"unlearn_influence takes Newton steps on the plain MSE objective: dis_type={self.dis_type!r} is not supported with it")
        check_model(self.model_type, getattr(self, 'loss', 'mse'))
        dist = _dist()
        if dist is not None and dist.get_world_size() > 1:
            raise ValueError(f'unlearn_influence runs on one rank, not {dist.get_world_size()}')
        assert len(train_dlist) == self.n_group
        kw = dict(kw)
        if kw.get('l2') is None:
            kw.setdefault('batch', self.batch)
            kw.setdefault('lam', self.lam)
        first_group = np.full(max(self.n_user, 1 + max((int(max(g)) for g in self.group_index if len(g)), default=0)), -1, dtype=np.int64)
        for i in reversed(range(self.n_group)):
            first_group[np.asarray(self.group_index[i], dtype=np.int64)] = i
        users = np.asarray(list(del_user), dtype=np.int64).reshape(-1)
        users = users[(users >= 0) & (users < len(first_group))]
        gids = sorted(int(g) for g in np.unique(first_group[users]) if g >= 0)
        for i in gids:                  # every setting of every affected shard, before any device work or change
            n = len(utils._rating_triple(train_dlist[i])[0])
            if n == 0:
                raise ValueError(f'shard {i} has no rating left: nothing to take a Newton step on (unlearn retrains it)')
            utils.newton_unlearn_check(self.model_type, 'mse', n_rows=n, **{k: v for k, v in kw.items() if k != 'scope'})
        self.combiner = None
        self.model_list = model_list
        self.folded ={u: g for u, g in getattr(self, 'folded', {}).items() if g not in set(gids)}

        merged = model_list[0].user_mat.weight.detach().clone().contiguous()
        self.influence_logs = {}
        for i in gids:
            # the shard's view: a copy of the merged user table (the rows of other shards' users have no entry in this loader; only
            # group_index[i]'s rows are merged back) and its own item table, updated in place
            shard = MF.from_tables(merged.clone(), self.model_list[i].item_mat.weight.detach().clone().contiguous())
            self.influence_logs[i] = utils.newton_unlearn(shard, train_dlist[i], **kw)
            self.model_list[i] = shard
        self._merge(merged, gids)

        self.test(test_data, verbose, save_dir)
        self.influenced = gids
        self.retrained = []
        return self.model_list
