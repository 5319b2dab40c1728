"""The numpy contract of in-training attribute unlearning (ultrare_amd/attr_train.py) against torch restatements of the reference's
literal lines, the skip rule, the argument checks before any device work, and the surface (InsParam / Scratch / main).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attr_train_cases as AC
from ultrare_amd import attr_train, lightgcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ------------------------------------------------------------------ selection
@pytest.mark.parametrize('seed', range(4))
def test_batch_groups_equal_unique_and_isin(seed):
    rs = np.random.RandomState(seed)
    n_user, N = 37, 150
    uid, iid = rs.randint(0, n_user, N), rs.randint(0, 9, N)
    ids = rs.permutation(n_user)
    id1, id2 = ids[:11], ids[11:25]                              # unsorted on purpose; 12 users in neither
    in_batch = rs.rand(N) < (0.05, 0.3, 0.6, 1.0)[seed]
    user = torch.from_numpy(uid[in_batch])
    u1, u2 = AC.torch_groups(user, torch.from_numpy(id1), torch.from_numpy(id2))
    for src in ((uid, iid), lightgcn.Graph(uid, iid, n_user, 9)):
        rows, n1, n2 = attr_train.batch_groups_ref(src, in_batch, id1, id2)
        assert rows.dtype == np.int32 and (n1, n2) == (len(u1), len(u2))
        assert rows.tolist() == u1.tolist() + u2.tolist()
    rows, n1, n2 = attr_train.batch_groups_ref((uid, iid), np.zeros(N, dtype=bool), id1, id2)
    assert (len(rows), n1, n2) == (0, 0, 0)
    with pytest.raises(ValueError, match='in_batch'):
        attr_train.batch_groups_ref((uid, iid), in_batch[:-1], id1, id2)


def test_step_valid_states_the_skip_rule():
    V = attr_train.step_valid
    assert V(1, 1, 'u2u') and V(3, 2, 'd2d', 0.5) and V(1, 1, 'd2d', 1e-300)
    assert not V(0, 5, 'u2u') and not V(5, 0, 'd2d', 1.0) and not V(0, 0, 'u2u')
    for bw in (0.0, -1.0, float('nan'), float('inf'), None):
        assert not V(2, 2, 'd2d', bw)
    with pytest.raises(ValueError, match='var'):
        V(1, 1, 'nor')


# ------------------------------------------------------------------ training against torch float64 autograd of the literal loss
@pytest.mark.parametrize('case', AC.CPU_CASES, ids=repr)
def test_train_ref_equals_torch_float64_autograd_of_the_literal_loss(case):
    """Both are float64 restatements of one formula: 1e-10 relative on tables and losses."""
    ref = AC.reference(case)['f64']
    assert ref['counts'].min() >= 1 and not ref['skipped'].any()             # no case passes by skipping everything
    t64 = AC.torch_train(case, torch.float64)
    for k in ('U', 'V', 'P', 'Q'):
        assert np.abs(t64[k] - ref[k]).max() <= 1e-10 * np.abs(ref[k]).max(), k
    for k in ('loss', 'dis'):
        assert np.abs(t64[k] / ref[k] - 1.0).max() <= 1e-10, k
    assert t64['skipped'].tolist() == ref['skipped'].tolist()
    assert ref['loss'].tolist() == np.sqrt((ref['sse'] + case.eta * ref['dis']) / case.N).tolist()
    plain = lightgcn.train_ref(case.uid, case.iid, case.rating, case.U0, case.V0, case.orders, case.B, case.lr_host, case.lam, case.mu, case.layers)
    assert np.abs(plain['U'] - ref['U']).max() > 1e-6                       # the term is not a no-op


def _planted(var):
    """24 users, one epoch of 4 steps; group 2 = the users 9 and 11, whose triples all sit in step 0: steps 1 .. 3 have an empty group."""
    case = AC.Case(24, 16, 8, 200, 64, 1, 1, seed=75, var=var, no_u=2, no_i=1)
    case.id2 = np.array([9, 11])
    mine, rest = np.flatnonzero(np.isin(case.uid, case.id2)), np.flatnonzero(~np.isin(case.uid, case.id2))
    assert 0 < len(mine) <= case.B
    case.orders = np.concatenate([mine, rest])[None, :].astype(case.orders.dtype)
    return case


@pytest.mark.parametrize('var', ('d2d', 'u2u'))
def test_a_step_with_an_empty_group_is_skipped(var):
    case = _planted(var)
    ref = case.train_ref()
    assert ref['counts'][0, :, 1].tolist() == [2, 0, 0, 0] and ref['counts'][0, :, 0].min() >= 1
    assert ref['skipped'].tolist() == [3]
    # the tables equal a run with eta = 0 on those steps: applying the term there at eta = 0 is the same run
    same = case.train_ref(eta_of_step=lambda e, t: case.eta if t == 0 else 0.0)
    t64 = AC.torch_train(case, torch.float64)
    for k in ('U', 'V', 'P', 'Q'):
        assert same[k].tobytes() == ref[k].tobytes()
        assert np.abs(t64[k] - ref[k]).max() <= 1e-10 * np.abs(ref[k]).max(), k
    assert t64['skipped'].tolist() == [3] and abs(t64['dis'][0] / ref['dis'][0] - 1) <= 1e-10
    # and differ from the plain run by step 0's term alone
    none = case.train_ref(eta_of_step=lambda e, t: 0.0)
    assert np.abs(none['U'] - ref['U']).max() > 1e-9


def test_a_step_whose_selected_rows_are_all_equal_is_skipped_under_d2d():
    """Zero bandwidth: layers = 0 and equal parameter rows for every group member.  Step 0 is skipped; the plain gradient then
    separates the rows, so the later steps apply."""
    case = AC.Case(24, 16, 8, 200, 64, 1, 0, seed=76, var='d2d', no_u=2, no_i=1)
    members = np.concatenate([case.id1, case.id2])
    case.U0[members] = case.U0[members[0]]
    ref = case.train_ref()
    assert ref['counts'].min() >= 1
    assert ref['skipped'].tolist() == [1] and np.isfinite(ref['U']).all() and np.isfinite(ref['dis']).all()
    same = case.train_ref(eta_of_step=lambda e, t: 0.0 if t == 0 else case.eta)
    for k in ('U', 'V', 'P', 'Q'):
        assert same[k].tobytes() == ref[k].tobytes()
    case.var = 'u2u'                                                        # no bandwidth: the Laplacian term applies (value 0 at step 0)
    assert case.train_ref()['skipped'].tolist() == [0]
    case.var, case.fix_sigma = 'd2d', 2.0                                   # fix_sigma counts as the bandwidth
    assert case.train_ref()['skipped'].tolist() == [0]


def test_float32_execution_is_close_and_argument_checks_name_the_argument():
    case = AC.CPU_CASES[1]
    ref = AC.reference(case)
    assert 0 < ref['E_y'] < 1e-5 and ref['f32']['U'].dtype == np.float32
    args = (case.uid, case.iid, case.rating, case.U0, case.V0, case.orders, case.B, case.lr_host, case.lam, case.mu, 1)
    for kw, msg in ((dict(var='nor'), 'var'), (dict(eta=float('nan')), 'eta'), (dict(kernel_num=17), 'kernel_num'), (dict(kernel_mul=0.0), 'kernel_mul'),
                    (dict(fix_sigma=-1.0), 'fix_sigma'), (dict(id1=[]), 'id1 is empty'), (dict(id2=[1, 1]), 'more than once'), (dict(id2=case.id1), 'disjoint'),
                    (dict(id1=[99]), 'outside')):
        a = dict(id1=case.id1, id2=case.id2, var='d2d')
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            attr_train.train_ref(*args, a.pop('id1'), a.pop('id2'), a.pop('var'), **a)
    wide = (case.uid, case.iid, case.rating, np.zeros((24, 129), np.float32), np.zeros((16, 129), np.float32)) + args[5:]
    with pytest.raises(ValueError, match='k = 129'):
        attr_train.train_ref(*wide, case.id1, case.id2, 'u2u')


# ------------------------------------------------------------------ the C ABI
def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_attr_train.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.ATTR_TRAIN_EXPORTS) and len(declared) == 8
    for other in (nv.EXPORTS, nv.CSR_PAIR_EXPORTS, nv.GCN_EXPORTS, nv.BPR_EXPORTS, nv.INF_EXPORTS, nv.NMF_EXPORTS, nv.NMF_RANK_EXPORTS, nv.COMBINE_RANK_EXPORTS):
        assert not declared & set(other)
    assert '#include "ultrare_attr_train.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    assert nv.ABI_VERSION == 15 and nv.lib().ure_abi_version() == 15
    L = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
        assert getattr(nv.lib(), name).argtypes == nv._ATTR_TRAIN_PROTOTYPES[name][1]
    from ultrare_amd import build
    assert 'attr_train.hip' in build.SOURCES and not {'attr_train.hip', 'mmd_tile.h'} & set(build.STEP_KERNEL_FILES)
    for name, (res, args) in nv._ATTR_TRAIN_PROTOTYPES.items():
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    # the tile arithmetic is written once: mmd.hip and attr_train.hip both take it from mmd_tile.h
    for src in ('mmd.hip', 'attr_train.hip'):
        text = open(os.path.join(ROOT, 'ultrare_amd', 'csrc', src)).read()
        assert '#include "mmd_tile.h"' in text and 'void mmd_pair' not in text and 'void mmd_stage' not in text


def test_the_new_kernels_do_not_spill(nv):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_report
    rows = [r for r in isa_report.kernels(nv.LIB_PATH) if '_dev_kernel' in r['name'] or r['name'].startswith(('attr_masks', 'attr_sel_', 'attr_add_grad'))]
    names = {r['name'] for r in rows}
    assert {'mmd_dev_kernel<1>', 'mmd_dev_kernel<2>', 'mmd_dev_kernel<8>', 'attr_masks_kernel', 'attr_sel_scatter_kernel'} <= names     # d = 8, 32, 128
    for r in rows:
        assert (r['vgpr_spill'], r['sgpr_spill'], r['scratch']) == (0, 0, 0), r


BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.addressof(BUF)


def _bad_calls():
    far = P + 32768
    step = lambda **kw: [kw.get(k, v) for k, v in (('X', P), ('ld', 8), ('d', 8), ('rows', P), ('counts', P), ('cap1', 4), ('cap2', 4))]
    mmd = lambda **kw: ('ure_attr_mmd_loss_grad', step(**kw) + [kw.get(k, v) for k, v in (('kernel_mul', 2.0), ('kernel_num', 5), ('fix_sigma', 0.0), ('bw', None),
                        ('sums', far), ('grad', far), ('valid', far), ('acc', None), ('skipped', None), ('ws', far), ('bytes', 1 << 14), ('stream', None))])
    u2u = lambda **kw: ('ure_attr_u2u_loss_grad', step(**kw) + [kw.get(k, v) for k, v in (('value', far), ('grad', far), ('valid', far), ('acc', None),
                        ('skipped', None), ('ws', far), ('bytes', 1 << 14), ('stream', None))])
    bw = lambda **kw: ('ure_attr_bandwidth', step(**kw) + [kw.get(k, v) for k, v in (('fix_sigma', 0.0), ('bw', far), ('valid', far), ('ws', far), ('bytes', 1 << 14),
                       ('stream', None))])
    masks = lambda **kw: ('ure_attr_step_masks', [kw.get(k, v) for k, v in (('off', P), ('tag', P), ('group', P), ('n_user', 4), ('nnz', 9), ('steps', 3),
                          ('masks', far), ('stream', None))])
    sel = lambda **kw: ('ure_attr_select', [kw.get(k, v) for k, v in (('masks', P), ('group', P), ('n_user', 4), ('steps', 3), ('step', 0), ('cap1', 2), ('cap2', 2),
                        ('rows', far), ('counts', far), ('ws', far), ('bytes', 64), ('stream', None))])
    add = lambda **kw: ('ure_attr_add_grad', [kw.get(k, v) for k, v in (('G', far), ('ldg', 8), ('n_rows', 4), ('d', 8), ('rows', P), ('counts', P), ('cap', 4),
                        ('valid', P), ('grad', P), ('eta', 1.0), ('stream', None))])
    return [mmd(d=129), mmd(d=0), mmd(cap1=0), mmd(cap2=0), mmd(ld=7), mmd(X=None), mmd(counts=None), mmd(kernel_num=17), mmd(kernel_num=0), mmd(kernel_mul=0.0),
            mmd(fix_sigma=float('nan')), mmd(sums=None), mmd(grad=None), mmd(valid=None), mmd(ws=None), mmd(bytes=8),
            u2u(d=200), u2u(cap1=0), u2u(rows=None), u2u(value=None), u2u(bytes=8), bw(bw=None), bw(cap2=1 << 31), bw(bytes=0),
            masks(steps=0), masks(n_user=0), masks(nnz=0), masks(masks=None), masks(off=None),
            sel(step=3), sel(step=-1), sel(cap1=0), sel(bytes=4), sel(rows=None), sel(n_user=0),
            add(d=129), add(ldg=7), add(eta=float('inf')), add(G=None), add(cap=0), add(n_rows=0)]


@pytest.mark.parametrize('entry,args', _bad_calls(), ids=lambda v: v if isinstance(v, str) else '')
def test_entries_check_their_arguments_before_any_hip_call(nv, entry, args):
    """Through ctypes on a machine without a device: -1 and the check's own message, and the 'device' memory is untouched."""
    ctypes.memset(P, 0x5A, len(BUF))
    assert getattr(nv.lib(), entry)(*args) == -1
    assert b'argument check failed' in nv.lib().ure_last_error()
    assert BUF.raw == b'\x5a' * len(BUF)


def test_sizers_refuse_what_the_entries_refuse(nv):
    L = nv.lib()
    assert L.ure_attr_scratch(1, 8) == -1 and L.ure_attr_scratch(10, 129) == -1 and L.ure_attr_scratch(10, 0) == -1 and L.ure_attr_scratch(2 ** 31, 8) == -1
    assert L.ure_attr_scratch(200, 32) == L.ure_mmd_scratch(200, 32) > 0
    assert L.ure_attr_scratch(10 ** 6, 128) < 17 * 10 ** 6 * 128 * 8 + 2 ** 20                              # never quadratic in the capacity
    assert L.ure_attr_select_scratch(0) == -1 and L.ure_attr_select_scratch(1) == 8 and L.ure_attr_select_scratch(2049) == 16


# ------------------------------------------------------------------ surface
def test_surface_refusals_and_defaults(tmp_path):
    from ultrare_amd.config import InsParam, Instance
    from ultrare_amd.main import attr_groups, parser
    from ultrare_amd.method.scratch import Scratch
    data = os.path.join(ROOT, 'tests', 'golden')
    id1, id2 = [0, 2, 4], [1, 3]
    plain = InsParam('toy', 2, data_dir=data)
    nor = InsParam('toy', 2, data_dir=data, dis_type='nor', attr=[], dis_eta=1.0)
    assert vars(nor).keys() == vars(plain).keys() and (nor.dis_type, nor.attr) == ('nor', []) and not hasattr(nor, 'dis_eta')
    for k in vars(plain):
        a, b = getattr(plain, k), getattr(nor, k)
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, k
    q = InsParam('toy', 2, data_dir=data, model='lightgcn', gcn_layers=0, dis_type='d2d', attr=(id1, np.array(id2)), dis_eta=0.25)
    assert (q.dis_type, q.attr, q.dis_eta, q.gcn_layers) == ('d2d', [id1, id2], 0.25, 0)
    lg = dict(model='lightgcn')
    with pytest.raises(NotImplementedError, match='--model lightgcn --gcn-layers 0'):
        InsParam('toy', 2, data_dir=data, dis_type='d2d', attr=(id1, id2))
    for kw, msg in ((dict(dis_type='mmd'), 'dis_type'), (dict(model='nmf', dis_type='u2u', attr=(id1, id2), layers=[64, 32]), "model='nmf'"),
                    (dict(lg, dis_type='u2u'), 'attr'), (dict(lg, dis_type='u2u', attr=(id1, [])), 'id2 is empty'),
                    (dict(lg, dis_type='u2u', attr=(id1, [1508])), 'outside'), (dict(lg, dis_type='u2u', attr=(id1, [4, 5])), 'disjoint'),
                    (dict(lg, dis_type='d2d', attr=(id1, [1.5])), 'integer'), (dict(lg, dis_type='d2d', attr=(id1, id2), dis_eta=float('inf')), 'eta'),
                    (dict(lg, dis_type='d2d', attr=(id1, id2), k=256), 'k = 256'), (dict(lg, attr=(id1, id2)), "dis_type='nor'"),
                    (dict(unlearn='influence', dis_type='d2d', attr=(id1, id2)), "dis_type='d2d'")):
        with pytest.raises(ValueError, match=msg):
            InsParam('toy', 2, data_dir=data, **kw)
    sc = Scratch(q, 'lightgcn')
    assert (sc.dis_type, sc.dis_eta) == ('d2d', 0.25) and sc.attr[0].tolist() == id1 and sc.attr[1].tolist() == id2
    assert Scratch(plain, 'lightgcn').dis_type == 'nor' and Scratch(plain, 'mf').attr == []
    with pytest.raises(NotImplementedError, match='--model lightgcn --gcn-layers 0'):
        Scratch(q, 'mf')
    q.layers = [64, 32]
    with pytest.raises(ValueError, match="'nmf' backbone"):
        Scratch(q, 'nmf')
    q.attr = [id1]
    with pytest.raises(ValueError, match='attr'):
        Scratch(q, 'lightgcn')
    q.attr, q.dis_type = [id1, id2], 'mmd'
    with pytest.raises(ValueError, match='dis_type'):
        Scratch(q, 'lightgcn')
    q.dis_type = 'u2u'
    from ultrare_amd.method.sisa import Sisa
    with pytest.raises(ValueError, match="dis_type='u2u'"):
        Sisa(q, 'lightgcn', 3, []).unlearn_influence([], [None] * 3, None, [], 0, '')
    ins = Instance.__new__(Instance)
    ins.param = q
    assert ins._model() == ('lightgcn', 'LightGCN_u2u_')
    q.loss = 'bpr'
    assert ins._model() == ('lightgcn', 'LightGCN_bpr_u2u_')
    ins.param = plain
    assert ins._model() == ('mf', 'MF_')
    args = parser.parse_args([])
    assert (args.dis_type, args.attr_file, args.dis_eta) == ('nor', None, 1.0)
    args = parser.parse_args(['--dis-type', 'u2u', '--attr-file', 'a.npz', '--dis-eta', '0.5'])
    assert (args.dis_type, args.attr_file, args.dis_eta) == ('u2u', 'a.npz', 0.5)
    with pytest.raises(SystemExit):
        parser.parse_args(['--dis-type', 'mmd'])
    path = str(tmp_path / 'attr.npz')
    np.savez(path, id1=np.array(id1), id2=np.array(id2))
    got = attr_groups('d2d', path)
    assert got[0].tolist() == id1 and got[1].tolist() == id2 and attr_groups('nor', None) == []
    np.savez(path, id1=np.array(id1))
    for a, msg in ((('d2d', None), '--attr-file'), (('nor', path), '--attr-file'), (('u2u', path), 'id1 and id2')):
        with pytest.raises(ValueError, match=msg):
            attr_groups(*a)


def test_device_wrappers_refuse_host_tensors_by_name():
    from ultrare_amd import _native, engine
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.mmd_loss_grad_dev(z(4, 8), i32(4), i32(2), 2, 2)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.u2u_loss_grad_dev(z(4, 8), i32(4), i32(2), 2, 2)
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.attr_add_grad(z(4, 8), i32(4), i32(2), i32(1), z(4, 8), 1.0)
    with pytest.raises(ValueError, match='capacities'):
        engine.attr_select(i32(4, 1), torch.zeros(4, dtype=torch.int8), 3, 0, 0, 2)
