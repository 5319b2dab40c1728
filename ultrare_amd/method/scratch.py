"""Scratch.train with the reference's signature (method/scratch.py:11-148), driving
the HBM-resident engine: the shard is uploaded once, every epoch is `steps` fused
kernel launches, and the two per-epoch tests run on the device.

RNG: the reference draws, per Scratch.train call, four normal fills (model init) and
per epoch three or four int64 seeds from torch's global CPU generator.
The draws are data independent, so they are all taken up front in the same order;
the epoch permutations are then expanded from their own generators.
"""
import os
import time

import numpy as np
import torch
from torch import nn

from .. import engine, rng
from ..read import as_loader
from . import utils
from .utils import MF, NMF, padded_tables, seed_all

PERM_THREADS = rng.perm_threads()
# end-of-epoch snapshots kept on the device for the per-epoch test series (per job).  They hold the rows with interactions in
# the shard only (engine: 'compact'): 5 GiB for 5 epochs of BASELINE.json configs[3] (32 shards, d = 128) on a 288 GB card.
def snapshot_limit():
    return int(float(os.environ.get('URE_SNAPSHOT_LIMIT_GB', '64')) * 2 ** 30)


def _is_empty(x):
    return isinstance(x, (list, tuple)) and len(x) == 0


def prepare_shard(train_loader, n_user, n_item, k, epochs, has_total, given_model='', defer=False):
    """Host part of one Scratch.train call: consume the RNG stream exactly like the
    reference (model init, then per-epoch seeds) and expand the permutations.  defer=True returns
    the permutations as a future (rng.epoch_perms_async): the expansion then runs beside the
    caller's next draws."""
    loader = as_loader(train_loader)
    if _is_empty(given_model) or given_model == '':
        # the stream of MF(...): 2 discarded + 2 kept fills (utils.py:31-40); big tables are made on the device
        U0, V0 = rng.mf_init(n_user, n_item, k, device=engine._device())
    else:
        U0 = given_model.user_mat.weight.detach().float().cpu()
        V0 = given_model.item_mat.weight.detach().float().cpu()
    seeds = rng.epoch_seeds(epochs, has_total)
    n = len(loader.dataset)
    # the permutations go to the device as batch tags (rng.epoch_tags; struct ure_shard: file_tags): half the bytes, and the device
    # does not partition them (rng.tags_batch_for: URE_HOST_TAGS=0, too many steps or rows -- as permutations)
    tags = rng.tags_batch_for(n, loader.batch_size)
    on_dev = None
    if loader.shuffle and tags:
        # ... and they are MADE on the device (rng.epoch_tags_device -> csrc/perm_chain.hip / perm_tags.hip): no sequential Fisher-Yates per
        # epoch on the host in front of the device's epochs (22.5 M rows per epoch for config.py:182-188's run at the 25 M shape)
        on_dev = rng.epoch_tags_device(seeds, n, tags, engine._device())
    if on_dev is not None:
        perms = on_dev
    elif loader.shuffle and defer:
        perms = rng.epoch_perms_async(seeds, n, threads=PERM_THREADS, pooled=True, device=engine._device(), tags_batch=tags)
    elif loader.shuffle and tags:
        perms = rng.epoch_tags(seeds, n, tags, threads=PERM_THREADS)
    elif loader.shuffle:
        perms = rng.epoch_perms(seeds, n, threads=PERM_THREADS, pooled=True)
    else:
        perms = torch.arange(n, dtype=torch.int32).repeat(epochs, 1)
    return loader.shard_data(n_user, n_item), (U0, V0), perms


def print_epoch(verbose, t, epochs, train_loss, test, total, has_total, epoch_time):
    """The per-epoch lines of scratch.py:99-118 (verbose 1 and 2).  test / total = (rmse, ndcg, hr)."""
    if verbose == 2:
        print(f'Epoch: [{t+1:>3d}/{epochs:>3d}] --------------------')
        print(f'Test - RMSE: {test[0]:>.4f}, NDCG: {test[1]:>.3f}, HR: {test[2]:>.3f}')
        print('Time:', epoch_time)
    elif verbose == 1:
        msg = (f'Epoch: [{t+1:>2d}/{epochs:>2d}]' + f' train loss: {train_loss:>.9f},' +
               f' train RMSE: {train_loss:>.4f},' + f' test RMSE: {test[0]:>.4f},')
        if has_total:
            msg += f' total RMSE: {total[0]:>.4f},'
        print(msg + ' time:', epoch_time)


class Scratch(object):
    def __init__(self, param, model_type):
        # model param
        self.n_user = param.n_user
        self.n_item = param.n_item
        self.k = param.k
        self.lam = param.lam
        self.model_type = model_type

        # training param
        self.seed = param.seed
        self.lr = param.lr
        self.lr_decay = param.lr_decay
        self.momentum = param.momentum
        self.epochs = param.epochs
        self.batch = getattr(param, 'batch', 30000)
        # the optimizer of every training job this object makes: 'sgd' (the reference's, scratch.py:64-69) or 'adam' (engine.TrainJob)
        self.optimizer = getattr(param, 'optimizer', 'sgd')
        if self.optimizer not in ('sgd', 'adam'):
            raise ValueError(f"optimizer {self.optimizer!r}: 'sgd' or 'adam'")
        self.betas = tuple(getattr(param, 'betas', (0.9, 0.999)))
        self.eps = getattr(param, 'eps', 1e-8)
        self.device = 'cuda'
        # the reference's InsParam never sets dis_type / attr.  'nor' is the plain loss; 'd2d' / 'u2u' add the per-batch
        # MMD / Laplacian term of utils.py:66-81 over the attribute groups attr = (id1, id2) (ultrare_amd/attr_train.py), on the
        # 'lightgcn' backbone (gcn_layers = 0 is plain MF); checked below, once the backbone is known
        self.dis_type = getattr(param, 'dis_type', 'nor')
        self.attr = []

        # log (one dict per object, appended by every shard it trains)
        self.log = {'train_loss': [],
                    'test_rmse': [],
                    'test_ndcg': [],
                    'test_hr': [],
                    'total_rmse': [],
                    'total_ndcg': [],
                    'total_hr': [],
                    'time': []}

        if self.model_type not in ('mf', 'lightgcn', 'nmf', 'wmf'):
            raise NotImplementedError("model_type is 'mf' on the published path (config.py:185-199), 'lightgcn' (ultrare_amd/lightgcn.py), 'nmf' "
                                      "(ultrare_amd/nmf.py) or 'wmf' (ultrare_amd/wmf.py)")
        if self.model_type == 'wmf':
            # weighted MF for implicit feedback (utils.WmfSweeps): alternating least squares, `epochs` counts sweeps; no optimizer, no
            # other loss, no per-batch term (refused by name before the generic checks below)
            from ..wmf import DEFAULT_ALPHA, DEFAULT_L2, check_backbone, check_wmf_args
            check_backbone(self.optimizer, getattr(param, 'loss', 'mse'), getattr(param, 'unlearn', 'retrain'), self.dis_type)
            self.wmf_alpha, self.wmf_l2, _, _ = check_wmf_args(getattr(param, 'wmf_alpha', DEFAULT_ALPHA), getattr(param, 'wmf_l2', DEFAULT_L2), 0.0,
                                                               self.epochs)
        if self.model_type == 'nmf':
            # the neural backbone (engine.NmfJob): SGD on the MSE loss only; `layers` is the MLP stack [L0, .., Lm]
            from ..nmf import check_layers as check_stack
            if self.optimizer != 'sgd':
                raise ValueError(f"model_type='nmf' trains with optimizer='sgd' only, not {self.optimizer!r}")
            if getattr(param, 'loss', 'mse') != 'mse':
                raise ValueError(f"model_type='nmf' trains with loss='mse' only, not {param.loss!r}")
            self.k, self.layers = check_stack(self.k, getattr(param, 'layers', None))
        if self.model_type == 'lightgcn':
            # the graph backbone (engine.GcnJob): SGD only, gcn_layers propagations per side
            from ..lightgcn import check_layers
            if self.optimizer != 'sgd':
                raise ValueError(f"model_type='lightgcn' trains with optimizer='sgd' only, not {self.optimizer!r}")
            self.gcn_layers = check_layers(getattr(param, 'gcn_layers', 2))
        # the training loss: 'mse' (the reference's), or 'bpr' -- pairwise, negatives drawn on the device (ultrare_amd/bpr.py)
        self.loss = getattr(param, 'loss', 'mse')
        if self.loss not in ('mse', 'bpr'):
            raise ValueError(f"loss {self.loss!r}: 'mse' or 'bpr'")
        if self.loss == 'bpr' and self.model_type != 'lightgcn':
            raise ValueError("loss='bpr' trains with model='lightgcn' only: --model lightgcn --gcn-layers 0 is BPR-MF")
        self._check_dis_type(param)
        self.loss_fn = nn.MSELoss(reduction='sum')
        self.is_rmse = True

    def _check_dis_type(self, param):
        from ..attr_train import DIS_TYPES, check_eta, check_k
        from ..attr_unlearn import check_groups
        if self.dis_type not in DIS_TYPES:
            raise ValueError(f"dis_type {self.dis_type!r}: one of {DIS_TYPES}")
        if self.dis_type == 'nor':
            return
        if self.model_type == 'mf':
            raise NotImplementedError(f"dis_type={self.dis_type!r} trains with model='lightgcn' only (utils.py:66-81 reads a table the MF model "
                                      "does not have): --model lightgcn --gcn-layers 0 is plain MF with the term")
        if self.model_type == 'nmf':
            raise ValueError(f"dis_type={self.dis_type!r} trains with model='lightgcn' only, not the 'nmf' backbone")
        attr = getattr(param, 'attr', [])
        if len(attr) != 2:
            raise ValueError(f"dis_type={self.dis_type!r} needs attr = (id1, id2), two groups of user ids")
        rows, n1, _ = check_groups(attr[0], attr[1], self.n_user)
        check_k(self.k)
        self.attr = (rows[:n1].astype(np.int64), rows[n1:].astype(np.int64))
        self.dis_eta = check_eta(getattr(param, 'dis_eta', 1.0))

    def attribute_attack(self, model, id1, id2, **kw):
        """The attribute-inference attacker on the user table of a model this object trained (utils.attribute_attack; its keywords
        pass through).  It changes nothing.  The 'nmf' backbone has two user tables: pass one (or a torch.cat of both) to
        utils.attribute_attack."""
        if not hasattr(model, 'user_mat'):
            raise ValueError("attribute_attack reads model.user_mat; for the 'nmf' backbone pass user_mat_mf.weight, user_mat_mlp.weight or a "
                             "torch.cat of both (at most 128 columns) to utils.attribute_attack")
        return utils.attribute_attack(model, id1, id2, **kw)

    def adversarial_unlearn(self, model, id1, id2, **kw):
        """Adversarial attribute unlearning of the user table of a model this object trained, in place (utils.adversarial_unlearn; its
        keywords pass through) -> its log.  The 'nmf' backbone, with two user tables, is refused."""
        return utils.adversarial_unlearn(model, id1, id2, **kw)

    def _optimizer_args(self):
        """What a TrainJob of this object takes beyond the reference's parameters."""
        return dict(optimizer=self.optimizer, betas=self.betas, eps=self.eps)

    def _snap_mode(self):
        """The end-of-epoch snapshots its jobs keep: compact ones need the closed form of lazy rows, which Adam has not."""
        return 'compact' if engine.LAZY_ROWS and self.optimizer == 'sgd' else 'full'

    def _models_before(self):
        return list(getattr(self, 'model_list', [])) if self.__class__.__name__ == 'Sisa' else []

    def train(self, train_data, test_data, test_total=[], verbose=1, save_dir='', id=0, given_model=''):
        with rng.torch_threads():          # (torch's intra-op pool capped for the duration of the request, restored afterwards)
            return self._train(train_data, test_data, test_total, verbose, save_dir, id, given_model)

    def _train(self, train_data, test_data, test_total, verbose, save_dir, id, given_model):
        print('Using device:', self.device)
        seed_all(self.seed)                                 # scratch.py:54
        has_total = not _is_empty(test_total)
        # verbose 0: nothing is printed per epoch, so the epochs run back to back, every epoch end is kept
        # on the device (snapshots) and the two test series of scratch.py:83-97 are computed afterwards
        # in four launches each (ure_eval_series); otherwise each epoch synchronises to print
        queued = verbose == 0
        if self.model_type == 'lightgcn':
            job, series = self._gcn_job(train_data, has_total, given_model, id), False     # (the per-epoch branch: no queued series)
            n_train, device = job.graph.N, job.device
        elif self.model_type == 'nmf':
            return self._train_nmf(train_data, test_data, test_total, has_total, verbose, save_dir, id, given_model)
        elif self.model_type == 'wmf':
            return self._train_wmf(train_data, test_data, test_total, has_total, verbose, save_dir, id, given_model)
        else:
            shard, init, perms = prepare_shard(train_data, self.n_user, self.n_item, self.k, self.epochs, has_total, given_model)
            batch = as_loader(train_data).batch_size
            snap_mode = self._snap_mode()
            series = queued and engine.TrainJob.snapshot_bytes([shard], self.epochs, self.k, snap_mode) <= snapshot_limit()
            job = engine.TrainJob([shard], [init], [perms], self.k, batch, self.epochs, self.lr, self.lam, self.momentum,
                                  self.lr_decay, snapshots=snap_mode if series else False, final_only=series, epoch_reads=True,       # (tables are read at epoch ends only)
                                  **self._optimizer_args())
            rng.release(perms)                                  # uploaded: the host buffer goes back to the pool
            n_train, device = shard.N, shard.device
        test_ev = as_loader(test_data).eval_set()
        total_ev = as_loader(test_total).eval_set() if has_total else None
        before = [padded_tables(m)[:2] for m in self._models_before()]

        res = torch.zeros(self.epochs, 2, 3, dtype=torch.float64, device=device) if queued else None
        times = []
        if series:
            sets = (test_ev, total_ev if has_total else test_ev)
            job.run()
            res = torch.zeros(2, self.epochs, 3, dtype=torch.float64, device=device)
            if has_total:
                job.evaluate_series_pair(0, sets[0], sets[1], before, res[0], res[1])
            else:
                for which, ev in enumerate(sets):
                    job.evaluate_series(0, ev, before, res[which])
            res = res.transpose(0, 1).contiguous()
            times = ['00:00:00'] * self.epochs
        for t in range(0 if not series else self.epochs, self.epochs):
            epoch_start = time.time()
            job.run_epochs(1)                               # baseTrain (utils.py:46-111) + scheduler.step()
            models = before + [job.padded_tables(0)]        # scratch.py:83-86
            if queued:
                test_ev.evaluate(models, job.d, out=res[t, 0])
                (total_ev if has_total else test_ev).evaluate(models, job.d, out=res[t, 1])
                times.append(time.strftime('%H:%M:%S', time.gmtime(time.time() - epoch_start)))
                continue
            test_rmse, test_ndcg, test_hr = test_ev.evaluate(models, job.d)
            if has_total:
                total_rmse, total_ndcg, total_hr = total_ev.evaluate(models, job.d)
            else:
                total_rmse, total_ndcg, total_hr = test_rmse, test_ndcg, test_hr
            train_loss = float(self._train_loss(job, n_train)[t])
            epoch_time = time.strftime('%H:%M:%S', time.gmtime(time.time() - epoch_start))
            print_epoch(verbose, t, self.epochs, train_loss, (test_rmse, test_ndcg, test_hr), (total_rmse, total_ndcg, total_hr), has_total, epoch_time)

            self.log['train_loss'].append(train_loss)
            self.log['test_rmse'].append(test_rmse)
            self.log['test_ndcg'].append(test_ndcg)
            self.log['test_hr'].append(test_hr)
            self.log['time'].append(epoch_time)
            if has_total:
                self.log['total_rmse'].append(total_rmse)
                self.log['total_ndcg'].append(total_ndcg)
                self.log['total_hr'].append(total_hr)

        if queued:
            res = res.cpu().numpy()
            self.log['train_loss'] += [float(x) for x in self._train_loss(job, n_train)]
            for c, key in enumerate(('test_rmse', 'test_ndcg', 'test_hr')):
                self.log[key] += [float(x) for x in res[:, 0, c]]
            self.log['time'] += times
            if has_total:
                for c, key in enumerate(('total_rmse', 'total_ndcg', 'total_hr')):
                    self.log[key] += [float(x) for x in res[:, 1, c]]

        U, V = job.tables(0)
        model = MF.from_tables(U.clone().contiguous(), V.clone().contiguous())
        if self.model_type == 'lightgcn':                   # the tables above are the layer mean; the parameters travel with the model
            model.base = tuple(t.clone().contiguous() for t in job.base_tables())
        job.close()
        self.save(model, save_dir, id)
        return model

    def _nmf_job(self, train_data, has_total, given_model):
        """The job of a NeuMF request: the model's draws (utils.NMF, on the CPU after seed_all), then the epochs' seeds as an MF
        request draws them; the orders are the epochs' permutations as file positions."""
        if not (_is_empty(given_model) or given_model == ''):
            raise ValueError("given_model is not supported with model_type='nmf': the job starts from NMF's own init")
        loader = as_loader(train_data)
        init = tuple(t.numpy() for t in NMF(self.n_user, self.n_item, self.k, self.layers).tables())
        seeds = rng.epoch_seeds(self.epochs, has_total)
        n = len(loader.dataset)
        orders = rng.epoch_perms(seeds, n, threads=PERM_THREADS) if loader.shuffle else torch.arange(n, dtype=torch.int32).repeat(self.epochs, 1)
        graph = engine.GcnGraph(*loader.dataset.triples(), self.n_user, self.n_item)
        return engine.NmfJob(graph, init, orders, self.k, self.layers, loader.batch_size, self.epochs, self.lr, self.lam, self.momentum, self.lr_decay)

    def _train_nmf(self, train_data, test_data, test_total, has_total, verbose, save_dir, id, given_model):
        """_train for the 'nmf' backbone: the per-epoch branch (no queued series), every epoch's two tests through
        EvalSet.evaluate_nmf on the models trained before (Sisa) and the job's current parameters."""
        job = self._nmf_job(train_data, has_total, given_model)
        test_ev = as_loader(test_data).eval_set()
        total_ev = as_loader(test_total).eval_set() if has_total else None
        before = [m.tables() + (m.k, m.layers) for m in self._models_before()]
        for t in range(self.epochs):
            epoch_start = time.time()
            job.run_epochs(1)
            models = before + [job.params() + (self.k, self.layers)]
            test = test_ev.evaluate_nmf(models)
            total = total_ev.evaluate_nmf(models) if has_total else test
            train_loss = float(np.sqrt(job.epoch_sse(0) / job.graph.N)[t])
            epoch_time = time.strftime('%H:%M:%S', time.gmtime(time.time() - epoch_start))
            print_epoch(verbose, t, self.epochs, train_loss, test, total, has_total, epoch_time)
            self.log['train_loss'].append(train_loss)
            for c, key in enumerate(('test_rmse', 'test_ndcg', 'test_hr')):
                self.log[key].append(test[c])
            self.log['time'].append(epoch_time)
            if has_total:
                for c, key in enumerate(('total_rmse', 'total_ndcg', 'total_hr')):
                    self.log[key].append(total[c])
        model = NMF.from_tables(*(t.clone() for t in job.params()), self.k, self.layers)
        job.close()
        self.save(model, save_dir, id)
        return model

    def _train_wmf(self, train_data, test_data, test_total, has_total, verbose, save_dir, id, given_model):
        """_train for the 'wmf' backbone: `epochs` sweeps of implicit ALS (utils.WmfSweeps) from the MF request's own draws
        (rng.mf_init, as the 'lightgcn' backbone takes them); no other draw is made, and nothing depends on a schedule or a learning
        rate, so a retrained shard is a function of its remaining data and the seed alone.  After every sweep the two tests of
        scratch.py:83-97 on the models trained before (Sisa) and the current tables; train_loss is the objective over all pairs
        (wmf.objective_ref).  The test RMSE compares a preference score with rating / 5 and means little, as under BPR: judge the
        model with rank_eval."""
        if not (_is_empty(given_model) or given_model == ''):
            raise ValueError("given_model is not supported with model_type='wmf': the sweeps start from rng.mf_init")
        U0, V0 = rng.mf_init(self.n_user, self.n_item, self.k, device=engine._device())
        dev = engine._device()
        U, V, d = padded_tables(MF.from_tables(U0.to(dev), V0.to(dev)))
        job = utils.WmfSweeps(U, V, d, self.k, utils._rating_triple(train_data), self.wmf_alpha, self.wmf_l2, 0.0)
        test_ev = as_loader(test_data).eval_set()
        total_ev = as_loader(test_total).eval_set() if has_total else None
        before = [padded_tables(m)[:2] for m in self._models_before()]
        for t in range(self.epochs):
            epoch_start = time.time()
            job.sweep()
            models = before + [(job.U, job.V)]
            test = test_ev.evaluate(models, d)
            total = total_ev.evaluate(models, d) if has_total else test
            train_loss = job.objective()
            epoch_time = time.strftime('%H:%M:%S', time.gmtime(time.time() - epoch_start))
            print_epoch(verbose, t, self.epochs, train_loss, test, total, has_total, epoch_time)
            self.log['train_loss'].append(train_loss)
            for c, key in enumerate(('test_rmse', 'test_ndcg', 'test_hr')):
                self.log[key].append(test[c])
            self.log['time'].append(epoch_time)
            if has_total:
                for c, key in enumerate(('total_rmse', 'total_ndcg', 'total_hr')):
                    self.log[key].append(total[c])
        model = MF.from_tables(*job.tables())
        self.save(model, save_dir, id)
        return model

    def _train_loss(self, job, n_train):
        """The train_loss series of a job: sqrt(sse / N) (utils.py:101-103), or under BPR the reference's is_rmse == False
        reporting, loss_sum / N (utils.py:104-106)."""
        dis = self.dis_eta * job.epoch_dis() if getattr(job, 'dis_type', 'nor') != 'nor' else 0.0      # utils.py:78-82: the term is part of the loss
        if self.loss == 'bpr':
            return (job.epoch_loss(0) + dis) / n_train
        return np.sqrt(np.maximum(job.epoch_sse(0) + dis, 0.0) / n_train)

    def _gcn_job(self, train_data, has_total, given_model, id=0):
        """prepare_shard and the job of a LightGCN request: the RNG stream is the MF request's (rng.mf_init, then the epochs' seeds),
        the orders are the epochs' permutations as file positions.  Under BPR the negatives' key is bpr.stream_key(seed, id): the
        shard's number, so a retrained shard draws under its own key from its post-deletion graph."""
        if not (_is_empty(given_model) or given_model == ''):
            raise ValueError("given_model is not supported with model_type='lightgcn': the job starts from rng.mf_init")
        loader = as_loader(train_data)
        init = rng.mf_init(self.n_user, self.n_item, self.k, device=engine._device())
        seeds = rng.epoch_seeds(self.epochs, has_total)
        n = len(loader.dataset)
        orders = rng.epoch_perms(seeds, n, threads=PERM_THREADS) if loader.shuffle else torch.arange(n, dtype=torch.int32).repeat(self.epochs, 1)
        graph = engine.GcnGraph(*loader.dataset.triples(), self.n_user, self.n_item)
        extra = {}
        if self.loss == 'bpr':
            from ..bpr import stream_key
            extra = dict(loss='bpr', key=stream_key(self.seed, id))
        if self.dis_type != 'nor':
            groups = engine.StepGroups(graph, *self.attr)
            if groups.cap1 < 1 or groups.cap2 < 1:          # (a SISA shard may hold one group only)
                import warnings
                warnings.warn(f"shard {id}: {groups.cap1} users of group 1 and {groups.cap2} of group 2 have ratings here: dis_type={self.dis_type!r} "
                              "needs both, so this shard trains as dis_type='nor' does")
            else:
                extra.update(attr=self.attr, dis_type=self.dis_type, eta=self.dis_eta)
        return engine.GcnJob(graph, init, orders, self.k, self.gcn_layers, loader.batch_size, self.epochs, self.lr, self.lam, self.momentum,
                             self.lr_decay, **extra)

    def save(self, model, save_dir, id):
        """scratch.py:131-144: model{id}.pth, user_mat{id}.npy, item_mat{id}.npy, log{id}.npy; a LightGCN model's parameters beside
        them as base_user_mat{id}.npy and base_item_mat{id}.npy.  An NMF model: model{id}.pth, user_mat_mf{id}.npy, user_mat_mlp{id}.npy,
        item_mat_mf{id}.npy, item_mat_mlp{id}.npy, log{id}.npy."""
        from .utils import dist_rank
        if isinstance(model, NMF):                          # the reference's attribute names (method/sisa.py:39-50) as file names
            if len(save_dir) > 0 and dist_rank()[0] == 0:
                torch.save(model.state_dict(), save_dir + '/model' + str(id) + '.pth')
                for name in ('user_mat_mf', 'user_mat_mlp', 'item_mat_mf', 'item_mat_mlp'):
                    np.save(save_dir + '/' + name + str(id), getattr(model, name).weight.detach().cpu().numpy())
                np.save(save_dir + '/log' + str(id), self.log)
            return
        if len(save_dir) > 0 and dist_rank()[0] == 0:       # several ranks running the same call: one set of files
            torch.save(model.state_dict(), save_dir + '/model' + str(id) + '.pth')
            np.save(save_dir + '/user_mat' + str(id), model.user_mat.weight.detach().cpu().numpy())
            np.save(save_dir + '/item_mat' + str(id), model.item_mat.weight.detach().cpu().numpy())
            np.save(save_dir + '/log' + str(id), self.log)
            if getattr(model, 'base', None) is not None:
                np.save(save_dir + '/base_user_mat' + str(id), model.base[0].cpu().numpy())
                np.save(save_dir + '/base_item_mat' + str(id), model.base[1].cpu().numpy())
