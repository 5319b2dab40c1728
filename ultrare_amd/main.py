"""Command line of the reference (main.py:5-72) on the MI355X engine.

Same flags, defaults and assertions; additions are optional:
  --k N          embedding width (the reference hard-codes 16, config.py:19)
  --parallel 0   train the shards of a SISA call one after the other, testing after every epoch as the reference does.  The default
                 (1) trains them side by side (and across ranks when launched with torch.distributed.run, one process per GPU) and
                 rebuilds the per-epoch tests from end-of-epoch snapshots: models, log0 and every log series are bit-identical
                 (tests/test_gpu_surface.py::test_parallel_equals_sequential_bitwise), the same lines are printed -- after the
                 call instead of during it -- and a 5-shard ml-1m learn takes 10 ms instead of 50.  One exception to
                 "bit-identical": a shard's own test_rmse comes from the total set's predictions (ure_eval_subset) when the shard's test
                 set is the total set's rows of its users, and is then summed pair by pair in double instead of by float wave partials --
                 equal to rounding (1e-12 relative), not to the bit, with a run that evaluates the shard's set on its own (another test
                 set, URE_EVAL_SUBSET=0, snapshots beyond URE_SNAPSHOT_LIMIT_GB); NDCG and HR are the same bits on both routes
  --dataset toy  the small rating set shipped with the reference (data/toy)
  --group-type   'emb-ot' (the reference's only route), 'uniform', or 'rating-ot': the reference's documented alternative, OT groups on
                 the sparse rating matrix (csrc/csr_group.hip), which needs no user matrix of an earlier --group 0 run;
                 'rating-bkmeans': the balanced k-means the reference compares OT grouping against, on the same sparse matrix
                 (csrc/csr_kmeans.hip); 'rating-bkmedoids' / 'rating-blpa': balanced k-medoids / label propagation on
                 the euclidean distances of the sparse rows, streamed (the CSR tile producer of csrc/pair_dist.hip).
                 The plain 'rating-kmeans' / '-kmedoids' / '-lpa' stay with Group.grouping: their shards are not balanced
  --optimizer    'sgd' (default: the reference's SGD with momentum 0.9) or 'adam' (torch.optim.Adam with weight_decay, fused into the step
                 kernel: DESIGN 4.21) -- the one that trains wide tables (--k 128) the reference's summed-loss SGD diverges on
  --lr           learning rate (default 0.001, config.py:27)
  --model        'mf' (default) or 'lightgcn': the graph backbone (ultrare_amd/lightgcn.py, csrc/gcn.hip), trained shard after
                 shard whatever --parallel says, artifacts under LightGCN_* with the parameters as base_user_mat / base_item_mat
  --gcn-layers   propagations per side of the 'lightgcn' backbone, 0 .. 8 (default 2)
  --model nmf    the NeuMF backbone (ultrare_amd/nmf.py, csrc/nmf.hip): GMF of width --k beside an MLP whose stack is
                 --layer L0 L1 .. Lm (the reference's "setting of layers"; powers of two, 1 .. 4 fully connected layers), trained shard
                 after shard with SGD on the MSE loss, artifacts under NMF_* with the four tables as user_mat_mf / user_mat_mlp /
                 item_mat_mf / item_mat_mlp.  'mf' and 'lightgcn' do not read --layer
  --model wmf    weighted matrix factorisation for implicit feedback by alternating least squares (ultrare_amd/wmf.py, csrc/wmf.hip,
                 DESIGN 4.32): every rating is an observation of confidence 1 + --wmf-alpha * rating / 5 (default 40, UNTUNED), every other
                 pair counts with confidence 1 and preference 0; --wmf-l2 is the ridge (default 0.1, UNTUNED); --epoch counts sweeps.
                 Trained shard after shard, artifacts under WMF_*; train_loss is the objective over all pairs, the RMSE columns mean
                 little (a preference score against rating / 5): judge the result with rank_eval.  Refuses --optimizer adam, --loss bpr,
                 --unlearn influence, --dis-type d2d / u2u and more than one rank
  --loss         'mse' (default: the reference's MSELoss(sum) on the rating) or 'bpr': the pairwise BPR loss, one negative per triple and
                 epoch drawn on the device (ultrare_amd/bpr.py, csrc/bpr.hip).  Needs --model lightgcn (--gcn-layers 0 is
                 BPR-MF); artifacts under LightGCN_bpr_*; train_loss is the mean batch loss; judge the result with rank_eval
  --unlearn      'retrain' (default: the affected shards are retrained, Sisa.unlearn) or 'influence': damped Newton steps on the remaining
                 data of every affected shard, no retraining (Sisa.unlearn_influence, ultrare_amd/influence.py, csrc/influence.hip,
                 DESIGN 4.25): approximate.  Needs --model mf --loss mse
  --attack       after every stage, the attribute-inference attacker (utils.attribute_attack, csrc/attack.hip) on the stage's
                 final user table over the two groups of --attr-file (refused without one): a cross-validated MLP probe of
                 --attack-hidden units (default 100; 0 is logistic regression) and --attack-folds folds (default 5).  Prints its AUC /
                 BAcc / F1 and saves attack<id>.npy beside log<id>.npy; without the flag no file appears and no artifact changes
  --adv-unlearn  after every stage, adversarial attribute unlearning (utils.adversarial_unlearn, csrc/adv.hip) of the two groups of
                 --attr-file (refused without one, and with --model nmf) on the stage's final user table: --adv-rounds rounds (default
                 100) against a cross-validated discriminator of --adv-hidden units (default 32).  Prints a one-line summary and saves
                 adv<id>.npy (the log, the moved rows and, with --attack, the attacker's result from BEFORE the move; attack<id>.npy is
                 then the one after) beside log<id>.npy.  The saved model files are written by training and are NOT rewritten, and the
                 next stage starts from the trained rows: the moved rows are in adv<id>.npy.  Without the flag no file appears and no
                 artifact changes
  --data-dir / --save-dir  roots of data/ and result/ (default: ./data, ./result)
"""
import argparse
import os

parser = argparse.ArgumentParser()
parser.add_argument('--dataset', type=str, default='ml1m', help='dataset name')
parser.add_argument('--epoch', type=int, default=50, help='number of epochs')
parser.add_argument('--worker', type=int, default=24, help='number of CPU workers (accepted, unused: no DataLoader workers)')
parser.add_argument('--verbose', type=int, default=1, help='verbose type')
parser.add_argument('--group', type=int, default=2, help='number of groups')
parser.add_argument('--layer', nargs='+', default=[64, 32], help='setting of layers')
parser.add_argument('--learn', type=str, default='sisa', help='type of learning and unlearning')
parser.add_argument('--delper', type=int, default=2, help='deleted user proportion')
parser.add_argument('--deltype', type=str, default='rand', help='deletion type')
parser.add_argument('--k', type=int, default=16, help='embedding width')
parser.add_argument('--parallel', type=int, default=1, help='1 (default): shards side by side / across GPUs; 0: one after the other')
parser.add_argument('--group-type', type=str, default='emb-ot', help="'emb-ot' (reference), 'uniform', or 'rating-ot' (OT groups), 'rating-bkmeans', 'rating-bkmedoids', 'rating-blpa' (balanced k-means / k-medoids / label propagation groups) on the sparse rating matrix, no --group 0 run needed")
parser.add_argument('--optimizer', type=str, default='sgd', choices=['sgd', 'adam'], help="'sgd' (reference) or 'adam'")
parser.add_argument('--lr', type=float, default=None, help='learning rate (default 0.001)')
parser.add_argument('--model', type=str, default='mf', choices=['mf', 'lightgcn', 'nmf', 'wmf'], help="'mf' (reference), 'lightgcn', 'nmf' (NeuMF; its MLP is --layer) or 'wmf' (implicit-feedback ALS; --epoch counts sweeps)")
parser.add_argument('--wmf-alpha', type=float, default=40.0, help="confidence slope of --model wmf: c = 1 + alpha * rating / 5 (default 40: untuned)")
parser.add_argument('--wmf-l2', type=float, default=0.1, help="ridge strength of --model wmf, > 0 (default 0.1: untuned)")
parser.add_argument('--gcn-layers', type=int, default=2, help="propagations per side of the 'lightgcn' backbone (0 .. 8)")
parser.add_argument('--loss', type=str, default='mse', choices=['mse', 'bpr'], help="'mse' (reference) or 'bpr' (needs --model lightgcn)")
parser.add_argument('--unlearn', type=str, default='retrain', choices=['retrain', 'influence'], help="'retrain' (reference) or 'influence' (Newton steps, no retraining; --model mf --loss mse)")
parser.add_argument('--dis-type', type=str, default='nor', choices=['nor', 'd2d', 'u2u'], help="'nor' (plain loss), or the per-batch attribute term 'd2d' (MMD) / 'u2u' (Laplacian); needs --attr-file and --model lightgcn (--gcn-layers 0 is plain MF)")
parser.add_argument('--attr-file', type=str, default=None, help="an .npz with id1 and id2: the global user ids of the two attribute groups of --dis-type")
parser.add_argument('--dis-eta', type=float, default=1.0, help='weight of the --dis-type term')
parser.add_argument('--attack', action='store_true', help="after every stage, run the attribute-inference attacker on the final user table over the groups of --attr-file (needs it); prints AUC / BAcc / F1, saves attack<id>.npy")
parser.add_argument('--attack-hidden', type=int, default=100, help='hidden units of the --attack probe (0: logistic regression)')
parser.add_argument('--attack-folds', type=int, default=5, help='cross-validation folds of the --attack probe')
parser.add_argument('--adv-unlearn', action='store_true', help="after every stage, adversarial attribute unlearning of the groups of --attr-file (needs it) on the final user table; prints a summary, saves adv<id>.npy with the moved rows.  The saved model files are written by training and are not rewritten")
parser.add_argument('--adv-rounds', type=int, default=100, help='rounds of --adv-unlearn')
parser.add_argument('--adv-hidden', type=int, default=32, help='hidden units of the --adv-unlearn discriminator (0: logistic regression)')
parser.add_argument('--data-dir', type=str, default=None)
parser.add_argument('--save-dir', type=str, default=None)


def layer_ints(layer):
    """--layer as integers for the 'nmf' backbone (ValueError names the value that is none)."""
    try:
        return [int(i) for i in layer]
    except ValueError:
        raise ValueError(f'--layer takes integers, not {layer!r}') from None


def attr_groups(dis_type, attr_file):
    """--attr-file as InsParam's attr: [] under 'nor' (a file is then refused), else [id1, id2] of the .npz."""
    import numpy as np
    if dis_type == 'nor':
        if attr_file is not None:
            raise ValueError("--attr-file goes with --dis-type d2d or u2u")
        return []
    if attr_file is None:
        raise ValueError(f'--dis-type {dis_type} needs --attr-file (an .npz with id1 and id2)')
    with np.load(attr_file) as z:
        if 'id1' not in z.files or 'id2' not in z.files:
            raise ValueError(f'{attr_file} must hold the arrays id1 and id2, not {sorted(z.files)}')
        return [z['id1'], z['id2']]


def attack_setting(attack, attr_file, hidden=100, folds=5):
    """--attack as Instance.attack: None without the flag, else dict(id1, id2, hidden, folds) of --attr-file (refused without one)."""
    import numpy as np
    if not attack:
        return None
    if attr_file is None:
        raise ValueError('--attack needs --attr-file (an .npz with id1 and id2): the two attribute groups the attacker tells apart')
    from .attack import MAX_FOLDS, MAX_H, _int
    hidden, folds = _int('--attack-hidden', hidden, 0, MAX_H), _int('--attack-folds', folds, 2, MAX_FOLDS)
    with np.load(attr_file) as z:
        if 'id1' not in z.files or 'id2' not in z.files:
            raise ValueError(f'{attr_file} must hold the arrays id1 and id2, not {sorted(z.files)}')
        return dict(id1=z['id1'], id2=z['id2'], hidden=hidden, folds=folds)


def adv_setting(adv, attr_file, model='mf', rounds=100, hidden=32):
    """--adv-unlearn as Instance.adv: None without the flag, else dict(id1, id2, rounds, hidden) of --attr-file (refused without one,
    and with --model nmf)."""
    import numpy as np
    if not adv:
        return None
    if attr_file is None:
        raise ValueError('--adv-unlearn needs --attr-file (an .npz with id1 and id2): the two attribute groups to make indistinguishable')
    if model == 'nmf':
        raise ValueError('--adv-unlearn moves one user table: --model nmf has two (not supported)')
    from .attack import MAX_H, _int
    rounds, hidden = _int('--adv-rounds', rounds, 1, 1 << 20), _int('--adv-hidden', hidden, 0, MAX_H)
    with np.load(attr_file) as z:
        if 'id1' not in z.files or 'id2' not in z.files:
            raise ValueError(f'{attr_file} must hold the arrays id1 and id2, not {sorted(z.files)}')
        return dict(id1=z['id1'], id2=z['id2'], rounds=rounds, hidden=hidden)


def main(argv=None):
    args = parser.parse_args(argv)
    attack = attack_setting(args.attack, args.attr_file, args.attack_hidden, args.attack_folds)
    if attack is not None and args.model == 'nmf':
        raise ValueError("--attack reads one user table: with --model nmf pass one of its two tables to utils.attribute_attack instead")
    adv = adv_setting(args.adv_unlearn, args.attr_file, args.model, args.adv_rounds, args.adv_hidden)

    assert args.dataset in ['ml1m', 'toy']
    assert args.epoch > 0
    assert args.worker > 0
    assert args.verbose in [0, 1, 2]
    assert args.group >= 0
    if args.model == 'nmf':          # values given on the command line arrive as strings; the other models see them as they came
        args.layer = layer_ints(args.layer)
    for i in args.layer:
        assert type(i) == int
    assert args.learn in ['sisa']
    assert args.delper in [2, 5]
    assert args.deltype in ['rand']
    assert args.group_type in ['emb-ot', 'uniform', 'rating-ot', 'rating-bkmeans', 'rating-bkmedoids', 'rating-blpa']

    import torch
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        import torch.distributed as dist
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        dist.init_process_group(os.environ.get('URE_DIST_BACKEND', 'nccl'), device_id=torch.device('cuda', local)
                                if os.environ.get('URE_DIST_BACKEND', 'nccl') == 'nccl' else None)
        if args.group > 0 and not args.parallel:
            # one process per GPU only makes sense with the shards spread over the ranks: without it every rank would train
            # every shard and write the same files
            if dist.get_rank() == 0:
                print('WORLD_SIZE > 1: --parallel 1 implied (shards placed over the ranks)')
            args.parallel = 1

    from .config import InsParam, Instance

    torch.manual_seed(42)   # the reference never seeds the CPU generator; a fixed run needs it
    param = InsParam(args.dataset, args.epoch, args.worker, args.layer, args.group, args.delper, args.deltype,
                     k=args.k, parallel=bool(args.parallel), data_dir=args.data_dir, optimizer=args.optimizer, lr=args.lr,
                     model=args.model, gcn_layers=args.gcn_layers, loss=args.loss, unlearn=args.unlearn,
                     dis_type=args.dis_type, attr=attr_groups(args.dis_type, None if (attack is not None or adv is not None) and args.dis_type == 'nor' else args.attr_file),
                     dis_eta=args.dis_eta, wmf_alpha=args.wmf_alpha, wmf_l2=args.wmf_l2)
    if attack is not None:
        # the groups against the table the attacker will read, before any training: a bad file costs no run
        from .attack import check_attack_args
        check_attack_args(param.n_user, args.k, attack['id1'], attack['id2'], attack['hidden'], attack['folds'])
    if adv is not None:
        from .adv_unlearn import DEFAULTS, check_adv_args
        check_adv_args(param.n_user, args.k, adv['id1'], adv['id2'], adv['hidden'], DEFAULTS['folds'], adv['rounds'])
    ins = Instance(param, save_dir=args.save_dir)
    if attack is not None:
        ins.attack = attack
    if adv is not None:
        ins.adv = adv

    if args.group == 0:
        ins.runFull(is_save=True, verbose=args.verbose)
    else:
        ins.runGroup(is_save=True, learn_type=args.learn, group_type=args.group_type, n_group=args.group,
                     verbose=args.verbose)


if __name__ == '__main__':
    main()
