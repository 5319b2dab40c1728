"""In-training attribute unlearning through the surface: Scratch against a direct job, Sisa.learn / unlearn with a shard that lacks a
group, the artifact names of an Instance (tests/golden/attr_train_artifacts.json), dis_type='nor' against a plain request, and the
operator."""
import copy
import json
import os
import shutil
import warnings

import numpy as np
import pytest
import torch

from test_gpu_lightgcn import N_ITEM, N_USER, TEST, TRAIN, Param, _bytes, _loaders

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
ARTIFACT_RUNS = {'lightgcn_d2d_g2': dict(dis_type='d2d', loss='mse'), 'lightgcn_bpr_u2u_g2': dict(dis_type='u2u', loss='bpr')}


def _param(epochs, dis_type, attr, dis_eta=1.0, **kw):
    p = Param(epochs, **kw)
    p.dis_type, p.attr, p.dis_eta = dis_type, attr, dis_eta
    return p


def _halves(users):
    users = np.sort(np.asarray(users, dtype=np.int64))
    return users[0::2], users[1::2]


def test_scratch_train_gives_the_tables_of_a_direct_job_with_the_term():
    from ultrare_amd import engine, rng
    from ultrare_amd.method.scratch import Scratch
    from ultrare_amd.method.utils import seed_all
    _, trd, ted, _ = _loaders(1)
    attr = _halves(np.arange(0, N_USER, 3))
    p = _param(2, 'd2d', attr, dis_eta=0.5, k=20, gcn_layers=1)
    sc = Scratch(p, 'lightgcn')
    torch.manual_seed(42)
    model = sc.train(trd[0], ted[0], [], 0, '')
    torch.manual_seed(42)
    seed_all(p.seed)
    init = rng.mf_init(N_USER, N_ITEM, p.k)
    n = len(trd[0].dataset)
    orders = rng.epoch_perms(rng.epoch_seeds(p.epochs, False), n)
    graph = engine.GcnGraph(*trd[0].dataset.triples(), N_USER, N_ITEM)
    args = (graph, init, orders, p.k, 1, 3000, p.epochs, p.lr, p.lam, p.momentum, p.lr_decay)
    job = engine.GcnJob(*args, attr=attr, dis_type='d2d', eta=0.5)
    job.run()
    U, V = job.tables(0)
    assert _bytes(model.user_mat.weight) == _bytes(U.contiguous()) and _bytes(model.item_mat.weight) == _bytes(V.contiguous())
    dis, skipped = job.epoch_dis(), job.epoch_skipped()
    assert (dis > 0).all() and not skipped.any()
    assert sc.log['train_loss'] == [float(x) for x in np.sqrt((job.epoch_sse(0) + 0.5 * dis) / n)]           # utils.py:108
    job.close()
    plain = engine.GcnJob(*args)
    plain.run()
    assert _bytes(plain.tables(0)[0].contiguous()) != _bytes(model.user_mat.weight)                           # the term moved the tables
    plain.close()


def test_dis_type_nor_through_scratch_gives_the_bytes_of_a_plain_request():
    from ultrare_amd.method.scratch import Scratch
    _, trd, ted, _ = _loaders(1)
    out = []
    for p in (Param(1), _param(1, 'nor', [])):
        torch.manual_seed(42)
        sc = Scratch(p, 'lightgcn')
        m = sc.train(trd[0], ted[0], [], 0, '')
        out.append((_bytes(m.user_mat.weight), _bytes(m.item_mat.weight), _bytes(m.base[0]), sc.log['train_loss']))
    assert out[0] == out[1]


def test_sisa_learns_and_unlearns_with_a_shard_that_lacks_a_group():
    from ultrare_amd.method.sisa import Sisa
    idx, trd, ted, tot = _loaders(3)
    id1 = np.sort(np.concatenate([np.asarray(g, dtype=np.int64)[0::4] for g in idx]))                          # every shard
    id2 = np.sort(np.concatenate([np.asarray(g, dtype=np.int64)[1::4] for g in idx[:2]]))                      # shards 0 and 1 only
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        s = Sisa(_param(1, 'u2u', (id1, id2)), 'lightgcn', 3, idx)
        torch.manual_seed(42)
        ml = s.learn(trd, ted, tot, 0, '')
    assert sum("trains as dis_type='nor' does" in str(w.message) for w in caught) == 1
    nor = Sisa(Param(1), 'lightgcn', 3, idx)
    torch.manual_seed(42)
    ml_nor = nor.learn(trd, ted, tot, 0, '')
    shard = lambda m: (_bytes(m.item_mat.weight), _bytes(m.base[0]), _bytes(m.base[1]))
    assert shard(ml[2]) == shard(ml_nor[2])                                                                   # the shard without group 2
    assert shard(ml[0]) != shard(ml_nor[0]) and shard(ml[1]) != shard(ml_nor[1])
    assert all(np.isfinite(v).all() for k, v in s.log.items() if k != 'time')
    del_user = [int(u) for u in idx[1][:5]]
    idx2, trd2, ted2, tot2 = _loaders(3, del_user)
    keep = lambda ids: ids[~np.isin(ids, del_user)]
    s2 = Sisa(_param(1, 'u2u', (keep(id1), keep(id2))), 'lightgcn', 3, idx2)
    torch.manual_seed(42)
    before = [shard(m) for m in ml]
    ml2 = s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, '')
    assert s2.retrained == [1]
    after = [shard(m) for m in ml2]
    assert after[0] == before[0] and after[2] == before[2] and after[1] != before[1]
    assert np.isfinite([s2.log0['total_rmse'], s2.log0['total_ndcg'], s2.log0['total_hr']]).all()


def artifact_names(root, dis_type, loss):
    """One runGroup of the toy set with the term -> the sorted relative paths of every file it wrote."""
    from ultrare_amd.config import InsParam, Instance
    data = os.path.join(root, 'data')
    os.makedirs(os.path.join(data, 'toy'))
    shutil.copy(TRAIN, os.path.join(data, 'toy', '0_train.csv'))
    shutil.copy(TEST, os.path.join(data, 'toy', '0_test.csv'))
    save = os.path.join(root, 'result')
    torch.manual_seed(42)
    attr = _halves(np.arange(0, N_USER, 2))
    p = InsParam('toy', 1, 24, [32], 2, 2, 'rand', data_dir=data, model='lightgcn', gcn_layers=0, loss=loss, dis_type=dis_type, attr=attr)
    models = Instance(p, save_dir=save).runGroup(is_save=True, learn_type='sisa', group_type='uniform', n_group=2, verbose=0)
    assert len(models) == 2
    return sorted(os.path.relpath(os.path.join(d, f), save).replace(os.sep, '/') for d, _, files in os.walk(save) for f in files)


@pytest.mark.parametrize('run', sorted(ARTIFACT_RUNS))
def test_instance_writes_the_artifacts_under_the_dis_type_names(tmp_path, run):
    with open(os.path.join(G, 'attr_train_artifacts.json')) as f:
        want = json.load(f)[run]
    got = artifact_names(str(tmp_path), **ARTIFACT_RUNS[run])
    assert got == want
    prefix = 'LightGCN_' + ('bpr_' if ARTIFACT_RUNS[run]['loss'] == 'bpr' else '') + ARTIFACT_RUNS[run]['dis_type'] + '_uniform_sisa_'
    assert any(prefix + 'learn/' in n for n in got) and any(prefix + 'unlearn/log0.npy' in n for n in got)
    assert not any('/MF_' in n or '/LightGCN_uniform' in n for n in got)


def test_the_op_equals_the_wrapper_and_raises_on_cpu_tensors():
    from ultrare_amd import _native as nv, engine, ops  # noqa: F401
    rs = np.random.RandomState(3)
    n_user, steps = 300, 40
    group = torch.from_numpy(rs.randint(0, 3, n_user).astype(np.int8)).cuda()
    masks = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, (n_user, 2)).astype(np.int32)).cuda()
    rows, counts = torch.ops.ultrare.attr_select(masks, group, steps, 37, n_user, n_user)
    want = engine.attr_select(masks, group, steps, 37, n_user, n_user)
    assert _bytes(rows) == _bytes(want[0]) and _bytes(counts) == _bytes(want[1]) and int(counts.sum()) > 0
    with pytest.raises(nv.NativeError, match='HIP device only'):
        torch.ops.ultrare.attr_select(masks.cpu(), group.cpu(), steps, 37, n_user, n_user)
