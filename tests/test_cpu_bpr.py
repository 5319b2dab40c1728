"""The BPR contract on the CPU (ultrare_amd/bpr.py): the selection rule IS the r-th missing item, the draws are uniform and never a
user's own item, the loss gradient and whole training are torch float64 autograd's, the plants are told apart, and every refusal of the
new surface comes before any device work.  tests/test_gpu_bpr.py holds the kernels to these functions."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import bpr_cases as B
import lightgcn_cases as C
from ultrare_amd import bpr, lightgcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHI2_9_001 = 27.88                                   # the 0.1 % critical value of chi-square with 9 degrees of freedom


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ------------------------------------------------------------------ 1. the selection rule and the draw
def test_selection_rule_is_the_rth_missing_item():
    """select_ref against np.setdiff1d for every r, n_item in 1 .. 64: random rows, an empty row, a row missing exactly one item."""
    rs = np.random.RandomState(1)
    for n_item in range(1, 65):
        rows = [np.zeros(0, np.int64), np.delete(np.arange(n_item), rs.randint(n_item))]
        rows += [np.sort(rs.choice(n_item, rs.randint(0, n_item), replace=False)) for _ in range(4)]
        for c in rows:
            missing = np.setdiff1d(np.arange(n_item), c)
            assert len(missing) == n_item - len(c) >= 1
            assert [bpr.select_ref(c, n_item, r) for r in range(len(missing))] == list(missing)


def _one_user_graph(items, n_item, copies=1):
    """A graph of ONE user with the given items (each `copies` times), and a second user without a triple."""
    iid = np.repeat(np.asarray(items, dtype=np.int64), copies)
    return lightgcn.Graph(np.zeros(len(iid), np.int64), iid, 2, n_item)


def test_sample_ref_is_the_selection_rule_with_repeated_pairs():
    """sample_ref draws r < m_u and maps it by select_ref -- also when the user's pairs repeat (the distinct-item CSR is then not the
    graph's), and never draws one of the user's items; every missing item is drawn."""
    rs = np.random.RandomState(2)
    for n_item in (2, 3, 7, 33, 64):
        for copies in (1, 3):
            items = np.sort(rs.choice(n_item, rs.randint(1, n_item), replace=False))
            g = _one_user_graph(items, n_item, copies)
            off_d, col_d = bpr.distinct_csr(g)
            assert list(col_d) == list(items) and list(off_d) == [0, len(items), len(items)]
            assert (copies == 1) == (len(col_d) == g.N)
            missing = np.setdiff1d(np.arange(n_item), items)
            seen = set()
            for epoch in range(40):
                neg = bpr.sample_ref(g, off_d, col_d, 5, epoch)
                assert np.isin(neg, missing).all()
                seen |= set(neg.tolist())
            assert seen == set(missing.tolist())


@pytest.mark.parametrize('key', B.KEYS)
@pytest.mark.parametrize('epoch', B.EPOCHS)
def test_draws_are_uniform(key, epoch):
    """100,000 draws of one user over the 1,000 items it has none of, 10 buckets: chi-square (9 degrees of freedom) <= 27.88, the
    0.1 % critical value; r < m_u always."""
    n, held = 100_000, 24
    g = lightgcn.Graph(np.zeros(n, np.int64), np.arange(n) % held, 1, 1000 + held)           # the user holds items 0 .. 23, each many times
    off_d, col_d = bpr.distinct_csr(g)
    assert len(col_d) == held
    neg = bpr.sample_ref(g, off_d, col_d, key, epoch).astype(np.int64)
    assert neg.min() >= held and neg.max() < 1000 + held                     # r = neg - 24 < m_u = 1000; never an item of the user's
    count = np.bincount((neg - held) // 100, minlength=10)
    chi2 = float(((count - n / 10) ** 2 / (n / 10)).sum())
    print(f'key {key} epoch {epoch}: chi-square {chi2:.2f}')
    assert chi2 <= CHI2_9_001


@pytest.mark.parametrize('case', B.SMALL_CASES[:3], ids=repr)
def test_no_negative_is_one_of_the_users_items(case):
    g, off_d, col_d = case.host()
    mine = set(zip(case.uid.tolist(), case.iid.tolist()))
    for epoch in (0, 1, 7):
        neg = bpr.sample_ref(g, off_d, col_d, case.key, epoch)
        assert not mine & set(zip(g.row_u.tolist(), neg.tolist()))
        assert neg.min() >= 0 and neg.max() < case.n_item
    assert (case.uid[0], case.iid[0]) == (case.uid[-1], case.iid[-1])        # a repeated pair
    any_item = bpr.sample_ref(g, off_d, col_d, case.key, 0, plant='any_item')
    assert mine & set(zip(g.row_u.tolist(), any_item.tolist()))              # (the plant does draw them)


def test_a_user_without_a_negative_is_refused_by_name():
    g = lightgcn.Graph([0, 0, 0, 1, 2, 2], [0, 1, 2, 1, 0, 0], 4, 3)
    with pytest.raises(ValueError, match='user 0 has a triple for every one of the 3 items'):
        bpr.check_negatives(g, bpr.distinct_csr(g)[0])
    with pytest.raises(ValueError, match='no negative to draw'):
        bpr.train_ref([0, 0, 0, 1], [0, 1, 2, 1], np.zeros((2, 4), np.float32), np.zeros((3, 4), np.float32), np.arange(4)[None], 2,
                      [1e-3], 0.1, 0.9, 1, 0)
    ok = lightgcn.Graph([0, 0, 1, 2, 2], [0, 1, 1, 0, 0], 4, 3)              # user 3 has no triple and never draws
    bpr.check_negatives(ok, bpr.distinct_csr(ok)[0])
    from ultrare_amd import engine
    host = types.SimpleNamespace(host=g, device='cuda', off_d=None)
    with pytest.raises(ValueError, match='no negative to draw'):            # (before any device work: no device is visible here)
        engine.bpr_prepare(host)


def test_the_epoch_and_the_key_move_the_draws_and_the_blind_plant_does_not():
    case = B.SMALL_CASES[1]
    g, off_d, col_d = case.host()
    a, b = (bpr.sample_ref(g, off_d, col_d, case.key, e) for e in (0, 1))
    assert not np.array_equal(a, b)
    blind = [bpr.sample_ref(g, off_d, col_d, case.key, e, plant='epoch_blind') for e in (0, 1)]
    assert np.array_equal(blind[0], blind[1]) and np.array_equal(blind[0], a)
    assert not np.array_equal(a, bpr.sample_ref(g, off_d, col_d, case.key + 1, 0))
    # the draw goes by the FILE position: the same triples in another file order give every triple the negative of its new position
    perm = np.random.RandomState(3).permutation(case.N)
    g2 = lightgcn.Graph(case.uid[perm], case.iid[perm], case.n_user, case.n_item)
    by_file, by_file2 = np.empty(case.N, np.int64), np.empty(case.N, np.int64)
    by_file[g.pos], by_file2[g2.pos] = a, bpr.sample_ref(g2, *bpr.distinct_csr(g2), case.key, 0)
    assert not np.array_equal(by_file[perm], by_file2)
    assert bpr.stream_key(42, 1) != bpr.stream_key(42, 2) != bpr.stream_key(43, 1) and 0 <= bpr.stream_key(2 ** 70, 3) < 2 ** 64
    assert bpr.stream_key(42, 1) == bpr.stream_key(42, 1)


def test_the_negative_index_is_the_stable_sort():
    rs = np.random.RandomState(4)
    neg = rs.randint(0, 9, 500)
    neg[neg == 3] = 4                                                        # item 3 is nobody's negative
    row_u = rs.randint(0, 40, 500).astype(np.int32)
    off_n, map_n, usr_n = bpr.neg_index_ref(neg, row_u, 11)
    assert map_n.tobytes() == np.argsort(neg, kind='stable').astype(np.int32).tobytes() and np.array_equal(usr_n, row_u[map_n])
    assert off_n[0] == 0 and off_n[-1] == 500 and off_n[3] == off_n[4] and off_n[9] == off_n[10] == off_n[11]
    for i in range(11):
        q = map_n[off_n[i]:off_n[i + 1]]
        assert (neg[q] == i).all() and (np.diff(q) > 0).all()


# ------------------------------------------------------------------ 2. the contract is BPR
def test_loss_gradient_equals_torch_autograd_in_float64():
    """loss_grad_ref(float64) against torch float64 autograd of sum -logsigmoid(x) with respect to the final tables: within 1e-9
    (the figure tests/test_cpu_lightgcn.py holds the MSE contract to).  The batch is partial, an item is positive and negative in it."""
    case = B.SMALL_CASES[1]
    g, off_d, col_d = case.host()
    rs = np.random.RandomState(5)
    U, V = rs.standard_normal((case.n_user, case.d)) * 0.5, rs.standard_normal((case.n_item, case.d)) * 0.5
    neg = bpr.sample_ref(g, off_d, col_d, case.key, 0)
    index = bpr.neg_index_ref(neg, g.row_u, g.n_item)
    batch = case.orders[0][2 * case.B:]
    assert 0 < len(batch) < case.B
    Gu, Gi, loss, w, x = bpr.loss_grad_ref(g, index, U, V, neg, batch, dtype=np.float64)
    neg_file = np.empty(case.N, np.int64)
    neg_file[g.pos] = neg
    Ut, Vt = torch.from_numpy(U).requires_grad_(True), torch.from_numpy(V).requires_grad_(True)
    u, i, j = (torch.from_numpy(a[batch].astype(np.int64)) for a in (case.uid, case.iid, neg_file))
    want = -torch.nn.functional.logsigmoid((Ut[u] * Vt[i]).sum(1) - (Ut[u] * Vt[j]).sum(1)).sum()
    want.backward()
    assert abs(loss - float(want.detach())) <= 1e-9 and np.abs(Gu - Ut.grad.numpy()).max() <= 1e-9 and np.abs(Gi - Vt.grad.numpy()).max() <= 1e-9
    assert set(case.iid[batch]) & set(neg_file[batch]) and set(neg_file[batch]) - set(case.iid[batch])      # positive and negative; negative only
    in_csr = bpr.in_batch_csr(g, batch)
    assert in_csr.sum() == len(batch) and not w[~in_csr].any() and not x[~in_csr].any() and (w[in_csr] < 0).all()


@pytest.mark.parametrize('case', B.SMALL_CASES, ids=repr)
def test_contract_equals_torch_autograd_in_float64(case):
    """train_ref(float64) against torch float64 autograd on the dense adjacency, -logsigmoid, SGD(momentum, weight_decay): within
    1e-9 over both final tables, both parameter tables and the epoch losses.  L = 0, 1, 2, 3; a repeated pair."""
    ref, yard = case.train_ref(), B.torch_bpr(case, torch.float64)
    for k in ('U', 'V', 'P', 'Q', 'loss'):
        assert np.isfinite(ref[k]).all() and np.isfinite(yard[k]).all(), k
    assert B.distance(yard, ref) <= 1e-9
    assert (case.uid[0], case.iid[0]) == (case.uid[-1], case.iid[-1])
    assert np.array_equal(ref['loss'], ref['loss_sum'] / case.N) and 'sse' not in ref
    assert np.array_equal(ref['U'][-1], ref['P'][-1]) == (case.layers == 0)


def test_cases_cover_the_shapes():
    assert [(c.n_user, c.n_item, c.d, c.N, c.B, c.epochs, c.layers) for c in B.WHOLE_STEP_CASES[:5]] == \
        [(c.n_user, c.n_item, c.d, c.N, c.B, c.epochs, c.layers) for c in C.WHOLE_STEP_CASES]
    assert B.WHOLE_STEP_CASES[5].layers == 0 and {c.layers for c in B.SMALL_CASES} == {0, 1, 2, 3}


@pytest.mark.parametrize('plant', bpr.PLANTS)
@pytest.mark.parametrize('case', B.WHOLE_STEP_CASES, ids=repr)
def test_every_plant_lies_outside_the_bound_of_the_device_test(case, plant):
    """The bound tests/test_gpu_bpr.py holds the job to -- 4 max(E_y, ulp32(max |w|)), E_y from two float32 CPU executions -- tells
    every plant apart on every whole-training case."""
    ref = B.reference(case)
    planted = B.plant_distance(case, plant)
    print(f'{case!r} {plant}: {planted:.3g} against the bound {ref["bound"]:.3g}')
    assert ref['E_y'] > 0 and planted > 100 * ref['bound'], (plant, planted, ref['bound'])


def test_the_contract_learns():
    """On the learnable case the last epoch's mean loss is below the first's, which starts near log 2 (tables of small entries)."""
    loss = B.LEARNABLE.train_ref()['loss']
    print(loss)
    assert abs(loss[0] - np.log(2)) < 0.05 and loss[-1] < 0.75 * loss[0]


def test_the_coefficient_is_stable_at_both_ends():
    x = np.array([0.0, 100.0, -100.0, 88.0, -88.0, 1e-8], np.float32)
    w = bpr.coef_w(x)
    assert w.dtype == np.float32 and w[0] == np.float32(-0.5) and np.isfinite(w).all() and w[2] == np.float32(-1) and -1e-40 < w[1] < 0
    t = bpr.loss_terms(x)
    assert np.isfinite(t).all() and t[0] == np.log(2) and abs(t[2] - 100) < 1e-12 and 0 < t[1] < 1e-40


# ------------------------------------------------------------------ 3. refusals and wiring
def test_job_refusals_come_before_any_device_work():
    from ultrare_amd import engine
    g = types.SimpleNamespace(n_user=3, n_item=4, N=5, nnz=5, device='cuda')
    P, Q = np.zeros((3, 8), np.float32), np.zeros((4, 8), np.float32)
    orders = np.stack([np.arange(5), np.arange(5)[::-1]]).astype(np.int32)
    make = lambda **kw: engine.GcnJob(**{**dict(graph=g, init=(P, Q), orders=orders, k=8, layers=2, batch=2, epochs=2, lr=1e-3, lam=0.1, momentum=0.9), **kw})
    for kw, msg in ((dict(loss='bce'), "'mse' or 'bpr'"), (dict(loss='bpr', key=-1), 'key must be'), (dict(loss='bpr', key=2 ** 64), 'key must be'),
                    (dict(loss='bpr', key=1.5), 'key must be'), (dict(loss='bpr', layers=9), 'layers')):
        with pytest.raises(ValueError, match=msg):
            make(**kw)
    g.host, g.off_d = lightgcn.Graph([0, 0, 0, 0, 1], [0, 1, 2, 3, 1], 3, 4), None
    with pytest.raises(ValueError, match='no negative to draw'):
        make(loss='bpr')


def test_surface_refusals_and_defaults():
    from ultrare_amd.config import InsParam, Instance
    from ultrare_amd.main import parser
    from ultrare_amd.method.scratch import Scratch
    data = os.path.join(ROOT, 'tests', 'golden')
    p = InsParam('toy', 2, data_dir=data)
    assert p.loss == 'mse' and Scratch(p, 'mf').loss == 'mse'
    q = InsParam('toy', 2, data_dir=data, model='lightgcn', gcn_layers=0, loss='bpr')
    assert (q.loss, q.model, q.gcn_layers) == ('bpr', 'lightgcn', 0) and Scratch(q, 'lightgcn').loss == 'bpr'
    for kw, msg in ((dict(loss='bpr'), '--model lightgcn --gcn-layers 0 is BPR-MF'), (dict(loss='bce', model='lightgcn'), "'mse' or 'bpr'"),
                    (dict(loss='bpr', model='lightgcn', optimizer='adam'), "optimizer='sgd' only")):
        with pytest.raises(ValueError, match=msg):
            InsParam('toy', 2, data_dir=data, **kw)
    with pytest.raises(ValueError, match='--model lightgcn --gcn-layers 0 is BPR-MF'):
        Scratch(q, 'mf')
    with pytest.raises(ValueError, match='given_model'):
        Scratch(q, 'lightgcn')._gcn_job(None, False, object(), 1)
    q.optimizer = 'adam'
    with pytest.raises(ValueError, match="optimizer='sgd' only"):
        Scratch(q, 'lightgcn')
    q.optimizer = 'sgd'
    args = parser.parse_args(['--model', 'lightgcn', '--gcn-layers', '0', '--loss', 'bpr'])
    assert (args.model, args.gcn_layers, args.loss) == ('lightgcn', 0, 'bpr') and parser.parse_args([]).loss == 'mse'
    with pytest.raises(SystemExit):
        parser.parse_args(['--loss', 'bce'])
    ins = Instance.__new__(Instance)
    ins.param = q
    assert ins._model() == ('lightgcn', 'LightGCN_bpr_')
    ins.param = InsParam('toy', 2, data_dir=data, model='lightgcn')
    assert ins._model() == ('lightgcn', 'LightGCN_')
    ins.param = p
    assert ins._model() == ('mf', 'MF_')


def test_ops_refuse_cpu_tensors():
    from ultrare_amd import _native, engine, ops  # noqa: F401
    z = torch.zeros
    with pytest.raises(_native.NativeError, match='HIP device only'):
        torch.ops.ultrare.bpr_negatives(z(3, dtype=torch.int64), z(2, dtype=torch.int32), z(2, dtype=torch.int32), z(2, dtype=torch.int32), 4, 0, 0)
    g = types.SimpleNamespace(n_user=2, n_item=2, nnz=2, device='cuda')
    with pytest.raises(_native.NativeError, match='HIP device only'):
        engine.bpr_loss_grad(g, z(2, dtype=torch.int32), 0, z(2, 4), z(2, 4), z(2, dtype=torch.int32))
    with pytest.raises(_native.NativeError, match='HIP device'):
        engine.bpr_neg_index(g, z(2, dtype=torch.int32))
    with pytest.raises(ValueError, match='epoch must be'):
        engine.bpr_negatives(g, 0, -1)


def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_bpr.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.BPR_EXPORTS)
    assert not declared & (set(nv.EXPORTS) | set(nv.CSR_PAIR_EXPORTS) | set(nv.GCN_EXPORTS))
    assert '#include "ultrare_bpr.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    L = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    from ultrare_amd import build
    assert 'bpr.hip' in build.SOURCES and not {'bpr.hip', 'gcn_ops.h'} & set(build.STEP_KERNEL_FILES)
    import inspect
    assert "'ultrare_bpr.h'" in inspect.getsource(build.source_hash)                 # the header is part of the library's identity
    for name, (res, args) in nv._BPR_PROTOTYPES.items():
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    assert nv.lib().ure_bpr_index_scratch(0, 5) == 0 and nv.lib().ure_bpr_index_scratch(5, 0) == 0
    assert nv.lib().ure_bpr_index_scratch(1, 2) == 3 * 256 + 1024 and nv.lib().ure_bpr_index_scratch(1025, 70000) == 3 * 4352 + 2048


BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.addressof(BUF)


def _bad_calls():
    """(entry, arguments) that each entry must refuse: host addresses stand in for device memory -- nothing may touch them."""
    far, mid = P + 32768, P + 16384
    sample = lambda **kw: ('ure_bpr_sample', [kw.get(k, v) for k, v in (('off_d', P), ('col_d', P + 1024), ('nnz_d', 9), ('row_u', P + 2048), ('pos', P + 3072),
                                                                       ('nnz', 9), ('n_user', 4), ('n_item', 4), ('key', 1), ('epoch', 0), ('neg', far), ('stream', None))])
    index = lambda **kw: ('ure_bpr_index', [kw.get(k, v) for k, v in (('neg', P), ('row_u', P + 1024), ('nnz', 9), ('n_item', 4), ('off_n', P + 2048),
                                                                     ('map_n', P + 3072), ('usr_n', P + 4096), ('scratch', far), ('bytes', 3 * 256 + 1024), ('stream', None))])
    coef = lambda **kw: ('ure_bpr_coef', [kw.get(k, v) for k, v in (('row', P), ('col', P), ('neg', P), ('tag', P), ('nnz', 9), ('step', 0), ('U', P), ('V', P),
                                                                   ('n_user', 4), ('n_item', 4), ('d', 8), ('w', far), ('x', mid), ('sp', None), ('sn', None), ('stream', None))])
    user = lambda **kw: ('ure_bpr_grad_user', [kw.get(k, v) for k, v in (('off', P), ('col', P), ('neg', P), ('tag', P), ('w', P), ('x', P), ('n_user', 4), ('n_item', 4),
                                                                        ('nnz', 9), ('step', 0), ('V', P), ('d', 8), ('G', far), ('row_loss', None), ('stream', None))])
    item = lambda **kw: ('ure_bpr_grad_item', [kw.get(k, v) for k, v in (('off_i', P), ('row', P), ('to_csr', P), ('off_n', P), ('map_n', P), ('usr_n', P), ('tag', P),
                                                                        ('w', P), ('n_item', 4), ('n_user', 4), ('nnz', 9), ('step', 0), ('U', P), ('d', 8), ('G', far),
                                                                        ('stream', None))])
    return [sample(nnz=0), sample(nnz=1 << 31), sample(nnz_d=0), sample(nnz_d=10), sample(n_user=0), sample(n_item=0), sample(epoch=-1), sample(neg=None),
            sample(neg=P + 2048 + 16), sample(off_d=None),
            index(nnz=0), index(n_item=0), index(bytes=3 * 256 + 1023), index(scratch=None), index(map_n=P + 4096), index(off_n=P + 8), index(scratch=P + 4096),
            index(usr_n=None),
            coef(d=6), coef(d=512), coef(nnz=0), coef(step=-1), coef(w=None), coef(x=far + 8), coef(n_user=0), coef(neg=None),
            user(d=24), user(nnz=0), user(step=-1), user(G=P), user(V=None), user(n_user=0), user(w=None),
            item(d=3), item(nnz=1 << 31), item(step=-1), item(G=P), item(U=None), item(n_item=0), item(off_n=None)]


@pytest.mark.parametrize('entry,args', _bad_calls(), ids=lambda v: v if isinstance(v, str) else '')
def test_entries_check_their_arguments_before_any_hip_call(nv, entry, args):
    """Through ctypes on a machine without a device: -1 and the check's own message, and the 'device' memory is untouched."""
    ctypes.memset(P, 0x5A, len(BUF))
    assert getattr(nv.lib(), entry)(*args) == -1
    assert b'argument check failed' in nv.lib().ure_last_error()
    assert BUF.raw == b'\x5a' * len(BUF)
