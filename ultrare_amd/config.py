"""InsParam / Instance with the reference's names, arguments and artifact layout
(config.py:16-200), running on the MI355X engine.

Differences from the reference, all defect fixes or optional additions:
  D1  n_del = int(del_per / 100 * n_user)   (the shipped formula asks for 12,080 of 6,040 users)
  D2  dis_type = 'nor', attr = []            (set here; Scratch needs them)
  D5  data / result roots are configurable   ($ULTRARE_DATA_DIR, $ULTRARE_SAVE_DIR, default ./data, ./result)
  +   InsParam(..., k=16, parallel=False)    optional embedding width and shard-parallel mode
  +   InsParam(..., optimizer='sgd', lr=None) optional optimizer ('adam': engine.TrainJob) and learning rate (None: 0.001)
  +   InsParam(..., model='mf', gcn_layers=2) optional backbone ('lightgcn': engine.GcnJob, artifacts under LightGCN_*) and its layers
  +   InsParam(..., model='nmf', layers=[64, 32]) optional neural backbone (NeuMF: engine.NmfJob, artifacts under NMF_*); `layers` is its MLP
                                             stack [L0, .., Lm] (ultrare_amd/nmf.py); optimizer='sgd' and loss='mse' only
  +   InsParam(..., loss='mse')              optional training loss ('bpr': pairwise, negatives drawn on the device; needs model='lightgcn';
                                             artifacts under LightGCN_bpr_*)
  +   InsParam(..., unlearn='retrain')       optional unlearning route of runGroup ('influence': Sisa.unlearn_influence, Newton steps on the
                                             affected shards instead of retraining them; model='mf' with loss='mse' only)
  +   InsParam(..., dis_type='nor', attr=[], dis_eta=1.0) optional in-training attribute unlearning ('d2d' / 'u2u': the per-batch MMD /
                                             Laplacian term over the user groups attr = (id1, id2), ultrare_amd/attr_train.py; needs
                                             model='lightgcn', gcn_layers=0 being plain MF; artifacts under LightGCN_<dis_type>_*)
  +   InsParam(..., model='wmf', wmf_alpha=40.0, wmf_l2=0.1) optional implicit-feedback backbone (weighted MF by alternating least squares,
                                             ultrare_amd/wmf.py, csrc/wmf.hip; artifacts under WMF_*): `epochs` counts sweeps, every triple is an
                                             observation of confidence 1 + wmf_alpha * rating / 5, wmf_l2 is the ridge; both defaults are
                                             UNTUNED.  optimizer='adam', loss='bpr', unlearn='influence', dis_type != 'nor', more than one rank
                                             and given_model are refused; parallel=True warns and trains the shards one after the other
  +   dataset 'toy' is usable end to end     (the reference only has its batch size)
"""
import os
import warnings
from os import mkdir
from os.path import exists

import numpy as np

from .group import DATA_DIR, SAVE_DIR, Group
from .method.scratch import Scratch
from .method.sisa import Sisa
from .method.utils import atomic_save, dist_rank, saveObject
from .read import RatingData, loadData, readRating, readSparseMat

DATASETS = {
    # name: (train csv, test csv, n_user, n_item)   relative to DATA_DIR   (config.py:40-44)
    'ml1m': ('ml1m/squ0_train.csv', 'ml1m/squ0_test.csv', 6040, 3416),
    'toy': ('toy/0_train.csv', 'toy/0_test.csv', 1508, 2071),
}


class InsParam(object):
    def __init__(self, dataset='toy', epochs=50, n_worker=24, layers=[32], n_group=2, del_per=2, del_type='test',
                 k=16, parallel=False, data_dir=None, optimizer='sgd', lr=None, model='mf', gcn_layers=2, loss='mse', unlearn='retrain',
                 dis_type='nor', attr=[], dis_eta=1.0, wmf_alpha=40.0, wmf_l2=0.1):
        if unlearn not in ('retrain', 'influence'):
            raise ValueError(f"unlearn {unlearn!r}: 'retrain' or 'influence'")
        from .attr_train import DIS_TYPES
        if dis_type not in DIS_TYPES:
            raise ValueError(f"dis_type {dis_type!r}: one of {DIS_TYPES}")
        from .wmf import DEFAULT_ALPHA, DEFAULT_L2, check_backbone, check_wmf_args
        if model == 'wmf':                      # implicit-feedback ALS (ultrare_amd/wmf.py): what it cannot be combined with, by name
            if optimizer not in ('sgd', 'adam'):
                raise ValueError(f"optimizer {optimizer!r}: 'sgd' or 'adam'")
            if loss not in ('mse', 'bpr'):
                raise ValueError(f"loss {loss!r}: 'mse' or 'bpr'")
            check_backbone(optimizer, loss, unlearn, dis_type)
            wmf_alpha, wmf_l2, _, _ = check_wmf_args(wmf_alpha, wmf_l2, 0.0, epochs if isinstance(epochs, int) and epochs >= 0 else 0)
            if wmf_alpha != DEFAULT_ALPHA:      # (set only off the defaults, as the other options are)
                self.wmf_alpha = wmf_alpha
            if wmf_l2 != DEFAULT_L2:
                self.wmf_l2 = wmf_l2
        elif wmf_alpha != DEFAULT_ALPHA or wmf_l2 != DEFAULT_L2:
            raise ValueError(f"wmf_alpha and wmf_l2 go with model='wmf', not model={model!r}")
        if unlearn == 'influence' and dis_type != 'nor':
            raise ValueError(f"unlearn='influence' takes Newton steps on the plain MSE objective: dis_type={dis_type!r} is not supported with it")
        if unlearn == 'influence':
            from .influence import check_model
            check_model(model, loss)
            self.unlearn = unlearn              # (set only off the default: the saved param of a plain run keeps its bytes)
        # model param
        self.k = k  # dimension of embedding (config.py:19 hard-codes 16)
        self.lam = 0.1  # regularization coefficient
        self.layers = layers  # the MLP stack [L0, .., Lm] of model='nmf' (the reference's "structure of FC layers"); unused by 'mf' and 'lightgcn'

        # training param
        self.seed = 42
        self.n_worker = n_worker
        self.batch = 3000 if dataset == 'toy' else 30000
        self.lr = 0.001 if lr is None else float(lr)
        self.lr_decay = 0.95
        self.momentum = 0.9
        self.epochs = epochs
        self.n_group = n_group
        self.dis_type = 'nor'   # D2
        self.attr = []          # D2
        self.parallel = parallel
        if optimizer not in ('sgd', 'adam'):
            raise ValueError(f"optimizer {optimizer!r}: 'sgd' or 'adam'")
        self.optimizer = optimizer  # 'adam': momentum is not used; betas / eps are torch.optim.Adam's defaults
        self.betas = (0.9, 0.999)
        self.eps = 1e-8
        if model not in ('mf', 'lightgcn', 'nmf', 'wmf'):
            raise ValueError(f"model {model!r}: 'mf', 'lightgcn', 'nmf' or 'wmf'")
        if model == 'nmf':
            from .nmf import check_layers as check_stack
            if optimizer != 'sgd':
                raise ValueError(f"model='nmf' trains with optimizer='sgd' only, not {optimizer!r}")
            if loss != 'mse':
                raise ValueError(f"model='nmf' trains with loss='mse' only, not {loss!r}")
            self.k, self.layers = check_stack(k, layers)
        if model == 'lightgcn' and optimizer != 'sgd':
            raise ValueError(f"model='lightgcn' trains with optimizer='sgd' only, not {optimizer!r}")
        if loss not in ('mse', 'bpr'):
            raise ValueError(f"loss {loss!r}: 'mse' or 'bpr'")
        if loss == 'bpr' and model != 'lightgcn':
            raise ValueError("loss='bpr' trains with model='lightgcn' only: --model lightgcn --gcn-layers 0 is BPR-MF")
        self.loss = loss                        # 'mse' (the reference's), or 'bpr' (ultrare_amd/bpr.py)
        from .lightgcn import check_layers
        self.model = model                      # the backbone: 'mf', 'lightgcn' (ultrare_amd/lightgcn.py), 'nmf' (ultrare_amd/nmf.py) or 'wmf' (ultrare_amd/wmf.py)
        self.gcn_layers = check_layers(gcn_layers)   # propagations per side of the 'lightgcn' backbone (`layers` above is the 'nmf' backbone's stack)

        if dis_type != 'nor':                   # the per-batch attribute term (ultrare_amd/attr_train.py); the groups are checked below
            from .attr_train import check_eta, check_k
            if model == 'mf':
                raise NotImplementedError(f"dis_type={dis_type!r} trains with model='lightgcn' only (utils.py:66-81 reads a table the MF model "
                                          "does not have): --model lightgcn --gcn-layers 0 is plain MF with the term")
            if model == 'nmf':
                raise ValueError(f"dis_type={dis_type!r} trains with model='lightgcn' only, not model='nmf'")
            check_k(k)
            self.dis_eta = check_eta(dis_eta)   # (set only off the default: the saved param of a plain run keeps its bytes)
        elif len(attr):
            raise ValueError("attr goes with dis_type 'd2d' or 'u2u': dis_type='nor' trains without it")

        # dataset-varied param
        self.del_rating = []  # 2d array/list [[uid, iid], ...]
        self.dataset = dataset
        self.max_rating = 5
        self.del_per = del_per
        self.del_type = del_type
        self.del_user = []

        if dataset in DATASETS:
            root = data_dir or DATA_DIR
            tr, te, self.n_user, self.n_item = DATASETS[dataset]
            self.train_dir = root + '/' + tr
            self.test_dir = root + '/' + te
            if self.del_type == 'rand':
                np.random.seed(0)
                n_del = int(self.del_per / 100 * self.n_user)            # D1
                self.del_user = np.random.choice(self.n_user, n_del, replace=False)
        else:
            raise ValueError(f'unknown dataset {dataset!r}; known: {sorted(DATASETS)}')
        if dis_type != 'nor':
            from .attr_unlearn import check_groups
            if len(attr) != 2:
                raise ValueError(f"dis_type={dis_type!r} needs attr = (id1, id2), two groups of user ids")
            rows, n1, _ = check_groups(attr[0], attr[1], self.n_user)
            self.dis_type, self.attr = dis_type, [rows[:n1].tolist(), rows[n1:].tolist()]

    def info(self):
        print(self.dataset, '-----------')
        print('Path of training data:', self.train_dir)
        print('Path of testing data:', self.test_dir)
        print('Number of users:', self.n_user)
        print('Number of items:', self.n_item)


class Instance(object):
    def __init__(self, param, save_dir=None):
        self.param = param
        self.save_root = save_dir or SAVE_DIR
        prefix = '/test/' if self.param.del_type == 'test' else '/' + str(self.param.del_per) + '/' + self.param.del_type + '/'
        self.name = prefix + self.param.dataset + '_g' + str(self.param.n_group)
        param_dir = self.save_root + self.name
        os.makedirs(param_dir, exist_ok=True)
        rank, dist = dist_rank()
        if rank == 0:          # several ranks (torch.distributed.run) run the same Instance: one of them writes
            # save param
            saveObject(param_dir + '/param', self.param)  # loadObject(dir + '/param')
            # save deletion
            deletion = [self.param.del_user, self.param.del_rating]
            arr = np.empty(2, dtype=object)
            arr[0], arr[1] = deletion

            def write(tmp):
                with warnings.catch_warnings(), open(tmp, 'wb') as f:
                    warnings.simplefilter('ignore')
                    np.save(f, arr)  # np.load('deletion.npy', allow_pickle=True)
            atomic_save(param_dir + '/deletion.npy', write)
        if dist is not None:
            dist.barrier()

    # read raw data (config.py:80-96)
    def _read(self, is_del=False, n_group=1, group_index=[]):
        del_user = self.param.del_user if is_del else []
        del_rating = self.param.del_rating if is_del else []
        train_rating, train_index = readRating(self.param.train_dir, self.param.n_user, self.param.max_rating,
                                               del_user, del_rating, n_group, group_index, 'a')
        # no deletion for testing data
        test_rating, _ = readRating(self.param.test_dir, self.param.n_user, self.param.max_rating,
                                    [], [], n_group, train_index)
        return train_rating, train_index, test_rating

    def _save_dir(self, is_save, saving_name):
        if not is_save:
            return ''
        save_dir = self.save_root + self.name + '/' + saving_name
        os.makedirs(save_dir, exist_ok=True)
        return save_dir

    def _attack(self, run, save_dir, id=0):
        """main.py --attack: self.attack = dict(id1, id2, hidden, folds), set by the caller after construction (it is no part of the
        saved parameters).  The attribute-inference attacker (utils.attribute_attack) on the final user table of the stage: its AUC /
        BAcc / F1 are printed and, with a save_dir, the dict is stored as attack<id>.npy beside log<id>.npy.  Without it nothing runs."""
        a = getattr(self, 'attack', None)
        if a is None:
            return None
        res = run(a)
        print('attribute attacker (hidden %d, %d folds): AUC %.4f  BAcc %.4f  F1 %.4f' % (res['settings']['hidden'], res['settings']['folds'],
                                                                                        res['auc'], res['bacc'], res['f1']))
        if save_dir and dist_rank()[0] == 0:      # (every rank holds the merged models and computes the same dict; one writes it)
            np.save(save_dir + '/attack' + str(id), res)
        self.last_attack = res
        return res

    def _adv(self, table, run, attack_run, save_dir, id=0, owner=None):
        """main.py --adv-unlearn: self.adv = dict(id1, id2, rounds, hidden), set by the caller after construction.  Adversarial
        attribute unlearning (utils.adversarial_unlearn) on the final user table of the stage: run(adv) -> the list of logs, table()
        -> the user table it moves.  A one-line summary is printed and, with a save_dir, adv<id>.npy is stored beside log<id>.npy:
        the logs, the moved rows (ids, rows) and -- with --attack -- the attacker's result from before the move; attack<id>.npy is
        then the attacker on the moved table.  The stage's table gets its trained bytes back afterwards: the saved model files
        are training's and the next stage starts from the trained rows; a combiner fitted on them, which
        Sisa.adversarial_unlearn drops, is put back on `owner` with them.  Without self.adv this is _attack alone."""
        v = getattr(self, 'adv', None)
        if v is None:
            return self._attack(attack_run, save_dir, id)
        import torch
        a = getattr(self, 'attack', None)
        before = attack_run(a) if a is not None else None
        kept = table().detach().clone()
        combiner = getattr(owner, 'combiner', None)
        logs = run(v)
        T = table().detach()
        moved = [g for g in logs if 'skipped' not in g]
        n = sum(sum(g['rows']) for g in moved)
        first, last = (sum(g['auc'][k] * sum(g['rows']) for g in moved) / max(n, 1) for k in (0, -1))
        rms = float(np.sqrt(sum(g['reg'][-1] for g in moved) / max(n, 1)))
        print('adversarial unlearning (hidden %d, %d rounds): %d of %d parts moved, in-loop AUC %.4f -> %.4f, RMS row movement %.4f'
              % (v['hidden'], v['rounds'], len(moved), len(logs), first, last, rms))
        ids = np.concatenate([np.asarray(v['id1']), np.asarray(v['id2'])]).astype(np.int64)
        res = dict(logs=logs, attack_before=before, ids=ids, rows=T[torch.from_numpy(ids).to(T.device)].cpu().numpy())
        if save_dir and dist_rank()[0] == 0:
            np.save(save_dir + '/adv' + str(id), res)
        self._attack(attack_run, save_dir, id)
        T.copy_(kept)
        if combiner is not None:
            owner.combiner = combiner
        self.last_adv = res
        return res

    # sub function of self.runFull (config.py:99-120)
    def _full(self, is_save, saving_name, model_type='mf', is_del=False, verbose=1):
        print(self.name, saving_name, 'begin:')
        train_rating, _, test_rating = self._read(is_del)
        train_data = loadData(RatingData(train_rating[0]), self.param.batch, self.param.n_worker)
        test_data = loadData(RatingData(test_rating[0]), self.param.batch, self.param.n_worker, False)
        save_dir = self._save_dir(is_save, saving_name)
        model = Scratch(self.param, model_type)
        trained = model.train(train_data, test_data, [], verbose, save_dir)
        self._adv(lambda: trained.user_mat.weight,
                  lambda v: [dict(model.adversarial_unlearn(trained, v['id1'], v['id2'], hidden=v['hidden'], rounds=v['rounds']),
                                  rows=(len(v['id1']), len(v['id2'])))],
                  lambda a: model.attribute_attack(trained, a['id1'], a['id2'], hidden=a['hidden'], folds=a['folds']), save_dir)
        print('End of training', self.name, saving_name)
        print()
        return trained

    def _full_user_mat(self):
        """config.py:132 loads result/2/rand/ml1m_g0/MF_full_train/user_mat0.npy -- the
        product of an earlier `--group 0` run.  Look beside this instance first."""
        p = self.param
        cands = [f'{self.save_root}/{p.del_per}/{p.del_type}/{p.dataset}_g0/MF_full_train/user_mat0.npy',
                 f'{self.save_root}/2/rand/ml1m_g0/MF_full_train/user_mat0.npy']
        for c in cands:
            if exists(c):
                return np.load(c, allow_pickle=True)
        raise FileNotFoundError(f'{cands[0]} not found: run the full-MF stage first (main.py --group 0), '
                                'its user matrix is the embedding the OT grouping clusters (config.py:132)')

    # sub function of self.runGroup (config.py:123-174)
    def _group(self, model_list, is_save, learn_type, saving_name, model_type='mf',
               is_del=False, group_type='uniform', n_group=5, verbose=1):
        print(self.name, saving_name, 'begin:')
        if group_type == 'uniform':
            group_index = []
        else:
            val_mat = readSparseMat(self.param.train_dir, self.param.n_user, self.param.n_item) \
                if group_type.startswith('rating') else None
            user_mat = None if group_type.startswith('rating') else self._full_user_mat()       # the ratings need no finished full-MF run
            rank, dist = dist_rank()
            grouper = Group(val_mat, self.param.dataset, user_mat)
            kw = dict(verbose=False, data_dir=os.path.dirname(os.path.dirname(self.param.train_dir)))
            if dist is None:
                group_index = grouper.grouping(self.param.dataset, n_group, group_type, **kw)
            else:               # rank 0 clusters and writes the label cache (atomically); the others read it after the barrier
                if rank == 0:
                    group_index = grouper.grouping(self.param.dataset, n_group, group_type, **kw)
                dist.barrier()
                if rank != 0:
                    group_index = grouper.grouping(self.param.dataset, n_group, group_type, **kw)

        train_rating, train_index, test_rating = self._read(is_del, n_group, group_index)

        train_dlist, test_dlist = [], []
        assert learn_type in ['sisa']
        for i in range(n_group):
            train_dlist.append(loadData(RatingData(train_rating[i]), self.param.batch, self.param.n_worker))
            test_dlist.append(loadData(RatingData(test_rating[i]), self.param.batch, self.param.n_worker, False))
        test_total = np.hstack(test_rating)
        test_data = loadData(RatingData(test_total), self.param.batch, self.param.n_worker, False)

        save_dir = self._save_dir(is_save, saving_name)

        model = Sisa(self.param, model_type, n_group, train_index)
        if not is_del:
            model.learn(train_dlist, test_dlist, test_data, verbose, save_dir)
        else:
            del_user = list(self.param.del_user)
            for rating in self.param.del_rating:
                if rating[0] not in del_user:
                    del_user.append(rating[0])
            if getattr(self.param, 'unlearn', 'retrain') == 'influence':
                model.unlearn_influence(model_list, train_dlist, test_data, del_user, verbose, save_dir)
            else:
                model.unlearn(model_list, train_dlist, test_dlist, test_data, del_user, verbose, save_dir)
        self._adv(lambda: model._merged_table(),
                  lambda v: model.adversarial_unlearn(v['id1'], v['id2'], hidden=v['hidden'], rounds=v['rounds']),
                  lambda a: model.attribute_attack(a['id1'], a['id2'], hidden=a['hidden'], folds=a['folds']), save_dir, owner=model)
        self.last = model
        return model.model_list

    #########################
    # runFull, runGroup
    #########################
    def _model(self):
        """(model_type, artifact prefix) of the backbone the parameters name."""
        model = getattr(self.param, 'model', 'mf')
        prefix = {'mf': 'MF_', 'lightgcn': 'LightGCN_', 'nmf': 'NMF_', 'wmf': 'WMF_'}[model]
        prefix += 'bpr_' if getattr(self.param, 'loss', 'mse') == 'bpr' else ''
        dis_type = getattr(self.param, 'dis_type', 'nor')
        return model, prefix + (dis_type + '_' if dis_type != 'nor' else '')

    def runFull(self, is_save=True, verbose=1):
        '''model MF (or the backbone of param.model)'''
        model, prefix = self._model()
        # full train without deletion
        self._full(is_save, prefix + 'full_train', model, False, verbose)
        # retrain from scratch after deletion
        self._full(is_save, prefix + 'retrain', model, True, verbose)

    def runGroup(self, is_save=True, learn_type='seq', group_type='uniform', n_group=5, verbose=1):
        '''model MF (or the backbone of param.model)'''
        if learn_type == 'seq':
            learn_type = 'sisa'      # the published tree only ships the SISA learner (main.py:45)
        model, prefix = self._model()
        saving_name = prefix + group_type + '_' + learn_type + '_learn'
        model_list = self._group([], is_save, learn_type, saving_name, model, False, group_type, n_group, verbose)
        saving_name = prefix + group_type + '_' + learn_type + '_unlearn'
        return self._group(model_list, is_save, learn_type, saving_name, model, True, group_type, n_group, verbose)
