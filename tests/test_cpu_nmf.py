"""The NeuMF contract on the CPU (ultrare_amd/nmf.py): it IS NeuMF -- torch float64 autograd is the yardstick --, every planted
defect moves it further than the bound the GPU comparison uses, and every refusal of the new surface comes before any device
work.  tests/test_gpu_nmf.py holds the kernels to these functions bit for bit."""
import ctypes
import functools
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch

import nmf_cases as C
from ultrare_amd import nmf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import build
    build.build()
    from ultrare_amd import _native
    return _native


# ------------------------------------------------------------------ 1. the contract is NeuMF
@pytest.mark.parametrize('case', C.WHOLE_CASES, ids=repr)
def test_contract_equals_torch_autograd_in_float64(case):
    """train_ref(float64) against torch float64 autograd (embedding lookups, F.linear, relu, MSELoss(sum), SGD(momentum,
    weight_decay) over every parameter) after whole training: both tables, the dense vector and the epoch losses agree within
    1e-12 of the largest magnitude compared -- a derived cap: fewer than 1e4 float64 operations feed any number.  Measured:
    1.2e-16 .. 4.0e-16 over the five cases."""
    ref, yard = case.train_ref(), C.torch_nmf(case, torch.float64)
    worst = 0.0
    for name in ('U', 'V', 'dense', 'loss'):
        assert np.isfinite(ref[name]).all() and np.isfinite(yard[name]).all(), name
        assert ref[name].shape == yard[name].shape
        worst = max(worst, float(np.abs(ref[name] - yard[name]).max() / np.abs(yard[name]).max()))
    print(f'{case!r}: {worst:.3g}')
    assert worst <= 1e-12
    assert (case.uid[0], case.iid[0]) == (case.uid[-1], case.iid[-1])
    assert set(range(case.no_u)).isdisjoint(case.uid) and set(range(case.no_i)).isdisjoint(case.iid)
    assert case.N % case.B and len(set(case.lr_host.tolist())) == case.epochs          # a partial last step; lr changes every epoch
    assert np.bincount(case.iid)[-1] >= case.N // 4 - 1                                 # a quarter of the ratings on one item (less the repeated pair's)
    assert not np.array_equal(ref['dense'][-1], case.dense0) and not np.array_equal(ref['U'][-1], case.U0)


def test_cases_are_the_issue_s():
    got = [(c.n_user, c.n_item, c.k, c.layers, c.N, c.B, c.epochs) for c in C.WHOLE_CASES]
    assert got == [(40, 30, 8, [16, 8], 500, 200, 3), (50, 45, 32, [64, 32], 700, 300, 3), (33, 21, 16, [64, 32, 16, 8], 400, 150, 3),
                   (45, 35, 64, [128, 64], 450, 200, 2), (30, 40, 4, [8, 4], 420, 200, 2)]
    assert C.STAGE_SHAPES == [(4, [8, 4]), (8, [16, 8]), (32, [64, 32]), (16, [64, 32, 16, 8]), (64, [128, 64]), (16, [32, 128, 4])]


# ------------------------------------------------------------------ 2. told apart from near misses
@pytest.mark.parametrize('plant', nmf.PLANTS)
@pytest.mark.parametrize('case', C.WHOLE_CASES, ids=repr)
def test_every_plant_is_beyond_the_bound_of_the_gpu_comparison(case, plant):
    """distance (every parameter and the losses) of each planted defect from the float64 contract exceeds the bound that
    tests/test_gpu_nmf.py holds NmfJob to: the GPU comparison can see each of them."""
    ref = C.reference(case)
    planted = C.distance(ref['f64'], case.train_ref(plant=plant))
    assert 3e-8 <= ref['E_y'] <= 3e-6                                      # (the yardstick is not degenerate)
    assert planted > ref['bound'], (plant, planted, ref['bound'])
    assert C.distance(ref['f64'], ref['f32']) <= ref['bound']


def test_stage_model_plants_zero_preactivations():
    k, layers = 8, [16, 8]
    U, V, dense = C.stage_model(k, layers, 9, 7, seed=1)
    S = nmf.Shape(k, layers)
    W, b, _, _ = S.unpack(dense)
    assert not W[0][:2].any() and b[0][:2].tobytes() == np.array([0.0, -0.0], np.float32).tobytes()
    uid, iid = np.arange(9) % 9, np.arange(9) % 7
    pred, act = nmf.forward_ref(U, V, dense, k, layers, uid, iid)
    a1 = act[:, S.a_at[1]:S.a_at[1] + 2]
    assert a1.tobytes() == bytes(a1.nbytes)
    dlt, _ = nmf.backward_ref(U, V, dense, k, layers, uid, iid, act, pred - np.float32(0.5))
    assert dlt[:, :2].tobytes() == bytes(9 * 8) and dlt[:, 2:].any()
    leak, _ = nmf.backward_ref(U, V, dense, k, layers, uid, iid, act, pred - np.float32(0.5), plant='relu_leak')
    assert leak[:, :2].any()


def test_squared_error_partials_are_one_per_workgroup():
    """sse_ref: min(ceil(n / 4), 2048) partials, zeros behind, each the float64 sum of four float32 fmaf chains; their total is the
    squared error to float32 rounding, and differs in its bits from a plain float64 sum (the chain is what is stated)."""
    rs = np.random.RandomState(8)
    for n in (1, 5, 257, 10000):
        pred, r = rs.standard_normal(n).astype(np.float32), rs.rand(n).astype(np.float32)
        sse = nmf.sse_ref(pred, r)
        blocks = min(-(-n // 4), nmf.SCORE_PARTIALS)
        assert sse.shape == (2048,) and sse.dtype == np.float64 and not sse[blocks:].any() and (sse[:blocks] > 0).all()
        exact = float(((pred.astype(np.float64) - r) ** 2).sum())
        assert abs(sse.sum() - exact) <= 1e-5 * exact
    assert sse.sum() != exact


def test_weight_gradient_chunks_are_told_apart_from_one_chain():
    """The two-level chain (chunks of 256 slots) is what the contract states: one chain over all slots gives other bytes."""
    k, layers = 4, [8, 4]
    S, rs = nmf.Shape(k, layers), np.random.RandomState(3)
    n = 515
    err, act, dlt = (rs.standard_normal(s).astype(np.float32) for s in ((n,), (n, S.A), (n, S.Dw)))
    got = nmf.weight_grad_ref(err, act, dlt, k, layers)
    one = np.zeros(S.layers[1], np.float32)
    for s in range(n):
        one = one + dlt[s, :S.layers[1]]
    assert not np.array_equal(got[S.b_at[0]:S.b_at[0] + S.layers[1]], one)
    f64 = nmf.weight_grad_ref(err, act, dlt, k, layers, dtype=np.float64)
    assert np.abs(got - f64).max() <= 515 * 2.0 ** -24 * np.abs(f64).max() * 4
    assert got[S.n_real:].tobytes() == bytes(4 * (S.n_dense - S.n_real))


# ------------------------------------------------------------------ 3. refusals and wiring
BAD_STACKS = [(8, [16]), (8, [16, 8, 8, 8, 8, 8]), (3, [16, 8]), (8, [4, 4]), (8, [16, 12]), (8, [16, 2]), (256, [16, 8]), (8, [256, 8]),
              (8, [16, 8.0]), (True, [16, 8]), (8, 'x'), (8, None), (128, [128, 128]), (8, [128, 128, 128, 128, 128])]


@pytest.mark.parametrize('k,layers', BAD_STACKS, ids=lambda v: str(v).replace(' ', ''))
def test_check_layers_refuses_before_any_device_call(k, layers):
    """No device is visible to this test: a ValueError (not the NativeError of a missing device) shows the order."""
    from ultrare_amd import engine
    with pytest.raises(ValueError, match='nmf'):
        nmf.check_layers(k, layers)
    g = types.SimpleNamespace(n_user=3, n_item=4, N=5, nnz=5, device='cuda')
    with pytest.raises(ValueError, match='nmf'):
        engine.NmfJob(g, (None, None, None), np.zeros((1, 5), np.int32), k, layers, 2, 1, 1e-3, 0.1, 0.9)
    z = torch.zeros
    with pytest.raises(ValueError, match='nmf'):
        engine.nmf_score(z(3, 8), z(3, 8), z(8), k, layers, z(2, dtype=torch.int32), z(2, dtype=torch.int32))


def test_check_layers_accepts_the_issue_s_shapes():
    for k, layers in C.STAGE_SHAPES + [(32, [64, 32]), (128, [128, 64])]:
        assert nmf.check_layers(k, layers) == (k, layers)
        assert nmf.lds_bytes(k, layers) <= nmf.LDS_BYTES
    assert nmf.check_layers(np.int64(8), (np.int32(16), 8)) == (8, [16, 8])
    assert nmf.lds_bytes(32, [64, 32]) < 16384


def test_job_refusals_come_before_any_device_work():
    from ultrare_amd import engine
    g = types.SimpleNamespace(n_user=3, n_item=4, N=5, nnz=5, device='cuda')
    k, layers = 4, [8, 4]
    S = nmf.Shape(k, layers)
    U, V, dense = np.zeros((3, S.wd), np.float32), np.zeros((4, S.wd), np.float32), np.zeros(S.n_dense, np.float32)
    orders = np.stack([np.arange(5), np.arange(5)[::-1]]).astype(np.int32)
    make = lambda **kw: engine.NmfJob(**{**dict(graph=g, init=(U, V, dense), orders=orders, k=k, layers=layers, batch=2, epochs=2, lr=1e-3, lam=0.1,
                                                momentum=0.9), **kw})
    for kw, msg in ((dict(batch=0), 'batch'), (dict(init=(U[:2], V, dense)), 'U has shape'), (dict(init=(U, V[:, :4], dense)), 'V has shape'),
                    (dict(init=(U, V, dense[:-4])), 'dense has shape'), (dict(init=(U, V)), 'init is'), (dict(orders=orders[:1]), 'orders must be'),
                    (dict(orders=orders.astype(np.float32)), 'orders must be'), (dict(orders=np.zeros((2, 5), np.int32)), 'not a permutation')):
        with pytest.raises(ValueError, match=msg):
            make(**kw)


def test_header_binding_and_library_agree(nv):
    header = open(os.path.join(ROOT, 'include', 'ultrare_nmf.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(ure_[a-z0-9_]+)\s*\(', header))
    assert declared == set(nv.NMF_EXPORTS) and len(declared) == 6
    for other in (nv.EXPORTS, nv.CSR_PAIR_EXPORTS, nv.GCN_EXPORTS, nv.BPR_EXPORTS, nv.INF_EXPORTS):
        assert not declared & set(other)
    assert len(nv.EXPORTS) == 96
    assert '#include "ultrare_nmf.h"' in open(os.path.join(ROOT, 'include', 'ultrare_hip.h')).read()
    L = ctypes.CDLL(nv.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
        assert getattr(nv.lib(), name).argtypes == nv._NMF_PROTOTYPES[name][1]          # NMF_EXPORTS is bound
    from ultrare_amd import build
    import inspect
    assert 'nmf.hip' in build.SOURCES and 'nmf.hip' not in build.STEP_KERNEL_FILES
    assert "'ultrare_nmf.h'" in inspect.getsource(build.source_hash)
    for name, (res, args) in nv._NMF_PROTOTYPES.items():
        proto = re.search(r'(?:int|int64_t)\s+' + name + r'\s*\((.*?)\);', header, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    assert (nmf.CHUNK, nmf.LDS_BYTES, nmf.MAX_FC) == tuple(int(re.search(r'#define ' + n + r' (\d+)', header).group(1))
                                                           for n in ('URE_NMF_CHUNK', 'URE_NMF_LDS_BYTES', 'URE_NMF_MAX_FC'))


def test_sizers_agree_with_the_contract(nv):
    L = nv.lib()
    for k, layers in C.STAGE_SHAPES:
        lay = np.array(layers, np.int32)
        S = nmf.Shape(k, layers)
        assert L.ure_nmf_dense_size(k, nv.ptr(lay), len(lay)) == S.n_dense
        for n in (1, 256, 257):
            assert L.ure_nmf_weight_grad_scratch(n, k, nv.ptr(lay), len(lay)) == -(-n // nmf.CHUNK) * S.n_dense * 4
    assert L.ure_nmf_weight_grad_scratch(2 ** 31 - 1, 4, nv.ptr(LAY), 2) == -1 and L.ure_nmf_weight_grad_scratch(0, 4, nv.ptr(LAY), 2) == -1
    assert L.ure_nmf_weight_grad_scratch(2 ** 31 - 257, 4, nv.ptr(LAY), 2) == -(-(2 ** 31 - 257) // 256) * nmf.Shape(4, [8, 4]).n_dense * 4        # (no 32-bit sum)
    for k, layers in [(k, l) for k, l in BAD_STACKS if isinstance(l, list) and all(isinstance(v, int) for v in l) and isinstance(k, int) and k is not True]:
        lay = np.array(layers, np.int32)
        assert L.ure_nmf_dense_size(k, nv.ptr(lay), len(lay)) == -1, (k, layers)          # the library refuses what check_layers refuses


BUF = ctypes.create_string_buffer(1 << 16)
P = ctypes.addressof(BUF)
LAY = np.array([8, 4], np.int32)
BAD_LAY = np.array([8, 3], np.int32)


def _bad_calls():
    """(entry, arguments) that each entry must refuse: host addresses stand in for device memory -- nothing may touch them."""
    far, lay, bad = P + 32768, LAY.ctypes.data, BAD_LAY.ctypes.data
    order = dict(
        ure_nmf_forward_backward=('row', 'col', 'rating', 'rank', 'nnz', 'lo', 'n_slots', 'U', 'V', 'n_user', 'n_item', 'dense', 'k', 'layers', 'n_layers',
                                  'err', 'pred', 'act', 'dlt', 'emb', 'stream'),
        ure_nmf_weight_grad=('err', 'act', 'dlt', 'n_slots', 'k', 'layers', 'n_layers', 'g', 'scratch', 'bytes', 'blocks', 'stream'),
        ure_nmf_row_sum=('off', 'map', 'rank', 'n_rows', 'nnz', 'lo', 'n_slots', 'E', 'ld', 'col0', 'width', 'err', 'G', 'row_loss', 'stream'),
        ure_nmf_score=('U', 'V', 'dense', 'k', 'layers', 'n_layers', 'n_user', 'n_item', 'total', 'first', 'last', 'uid', 'iid', 'rating', 'n', 'pred', 'sse',
                       'stream'))
    base = dict(row=P, col=P, rating=P, rank=P, nnz=9, lo=0, n_slots=4, U=P, V=P, n_user=4, n_item=4, dense=P, k=4, layers=lay, n_layers=2, err=far,
                pred=None, act=far, dlt=far, emb=far, stream=None, g=far, scratch=far + 4096, bytes=1 << 12, blocks=0, off=P, map=None, n_rows=4, E=P, ld=16,
                col0=4, width=8, G=far, row_loss=None, total=1, first=1, last=1, uid=P, iid=P, n=5, sse=None)
    call = lambda entry, **kw: (entry, [{**base, **kw}[name] for name in order[entry]])
    fb, wg, rs, sc = (functools.partial(call, entry) for entry in order)
    return [fb(k=3), fb(layers=bad), fb(layers=None), fb(n_layers=1), fb(n_layers=6), fb(nnz=0), fb(nnz=1 << 31), fb(n_slots=0), fb(lo=-1), fb(lo=6),
            fb(n_user=0), fb(n_item=1 << 31), fb(U=None), fb(dense=None), fb(err=None), fb(act=None), fb(dlt=None), fb(emb=None), fb(rank=None),
            wg(k=12), wg(layers=bad), wg(n_slots=0), wg(n_slots=2 ** 31 - 1), wg(n_slots=2 ** 31 - 256), wg(bytes=16), wg(scratch=None), wg(g=None), wg(blocks=-1), wg(scratch=far + 16), wg(err=None),
            rs(width=6), rs(width=260), rs(width=0), rs(col0=2), rs(ld=18), rs(ld=8), rs(n_rows=0), rs(nnz=0), rs(n_slots=0), rs(lo=8), rs(E=None),
            rs(G=None), rs(G=P), rs(off=None), rs(rank=None), rs(row_loss=far + 8192, err=None),
            sc(k=2), sc(layers=bad), sc(n=0), sc(n=1 << 31), sc(n_user=0), sc(total=0), sc(pred=None), sc(uid=None), sc(dense=None), sc(sse=far, rating=None)]


@pytest.mark.parametrize('entry,args', _bad_calls(), ids=lambda v: v if isinstance(v, str) else '')
def test_entries_check_their_arguments_before_any_hip_call(nv, entry, args):
    """Through ctypes on a machine without a device: -1 and the check's own message, and the 'device' memory is untouched."""
    ctypes.memset(P, 0x5A, len(BUF))
    assert getattr(nv.lib(), entry)(*args) == -1
    assert b'argument check failed' in nv.lib().ure_last_error()
    assert BUF.raw == b'\x5a' * len(BUF)


# ------------------------------------------------------------------ 4. the surface without a device
def test_insparam_cli_and_artifact_names(monkeypatch):
    from ultrare_amd.config import InsParam, Instance
    from ultrare_amd.main import layer_ints, parser
    from ultrare_amd.method import sisa
    from ultrare_amd.method.scratch import Scratch
    data = os.path.join(ROOT, 'tests', 'golden')
    p = InsParam('toy', 2, data_dir=data, model='nmf', layers=[64, 32], k=32)
    assert (p.model, p.k, p.layers) == ('nmf', 32, [64, 32])
    for kw, msg in ((dict(layers=[32]), 'nmf: layers must hold'), (dict(layers=[64, 30]), 'power of two'), (dict(layers=['64', '32']), 'power of two'),
                    (dict(layers=[64, 32], optimizer='adam'), "optimizer='sgd' only"), (dict(layers=[64, 32], loss='bpr'), "loss='mse' only"),
                    (dict(layers=[64, 32], unlearn='influence'), "model='mf' only, not 'nmf'"), (dict(layers=[64, 32], k=12), 'k must be')):
        with pytest.raises(ValueError, match=msg):
            InsParam('toy', 2, data_dir=data, model='nmf', **kw)
    # the other backbones see `layers` as it came, and a plain parameter object keeps its pickle
    assert InsParam('toy', 2, data_dir=data, layers=['64', '32']).layers == ['64', '32']
    plain = InsParam('toy', 2, data_dir=data)
    assert sorted(vars(plain)) == sorted(vars(p)) and pickle.dumps(plain) == pickle.dumps(InsParam('toy', 2, data_dir=data))
    args = parser.parse_args(['--model', 'nmf', '--layer', '64', '32', '--k', '32'])
    assert (args.model, args.layer, layer_ints(args.layer)) == ('nmf', ['64', '32'], [64, 32])
    with pytest.raises(ValueError, match='--layer takes integers'):
        layer_ints(['64', 'x'])
    with pytest.raises(SystemExit):
        parser.parse_args(['--model', 'dmf'])
    ins = Instance.__new__(Instance)
    ins.param = p
    assert ins._model() == ('nmf', 'NMF_')
    s = Scratch(p, 'nmf')
    assert (s.k, s.layers) == (32, [64, 32])
    with pytest.raises(ValueError, match='nmf: layers'):
        Scratch(plain, 'nmf')                                                # (layers=[32] is no stack)
    with pytest.raises(ValueError, match='given_model'):
        s._nmf_job(None, False, object())
    for attr, value, msg in (('optimizer', 'adam', "optimizer='sgd' only"), ('loss', 'bpr', "loss='mse' only")):
        q = InsParam('toy', 2, data_dir=data, model='nmf', layers=[64, 32])
        setattr(q, attr, value)
        with pytest.raises(ValueError, match=msg):
            Scratch(q, 'nmf')
    p.parallel = True
    with pytest.warns(UserWarning, match='one after the other'):
        model = sisa.Sisa(p, 'nmf', 3, [])
    assert model.parallel is False
    two = types.SimpleNamespace(get_world_size=lambda: 2)
    monkeypatch.setattr(sisa, '_dist', lambda: two)
    with pytest.raises(ValueError, match="'nmf' runs on one rank, not 2"):
        sisa.Sisa(p, 'nmf', 3, [])
    with pytest.raises(ValueError, match='one rank, not 2'):
        model.learn([None] * 3, [None] * 3, None, 0, '')
    with pytest.raises(ValueError, match='one rank, not 2'):
        model.unlearn([], [None] * 3, [None] * 3, None, [], 0, '')


def _cpu_model(k=8, layers=(16, 8), n_user=11, n_item=7, seed=5):
    from ultrare_amd.method.utils import NMF
    torch.manual_seed(seed)
    return NMF(n_user, n_item, k, list(layers))


def test_module_init_and_from_tables_draw_nothing_extra():
    from ultrare_amd.method.utils import NMF
    m = _cpu_model()
    assert [n for n, _ in m.named_parameters()] == ['user_mat_mf.weight', 'item_mat_mf.weight', 'user_mat_mlp.weight', 'item_mat_mlp.weight',
                                                    'fc.0.weight', 'fc.0.bias', 'head.weight', 'head.bias']
    assert m.user_mat_mf.weight.shape == (11, 8) and m.user_mat_mlp.weight.shape == (11, 8) and m.head.weight.shape == (1, 16)
    for emb in (m.user_mat_mf, m.item_mat_mf, m.user_mat_mlp, m.item_mat_mlp):
        assert 0.003 < float(emb.weight.detach().std()) < 0.03                      # normal_(std=0.01)
    assert float(m.fc[0].weight.detach().abs().max()) <= 0.25 + 1e-6                 # torch's default: |w| <= 1 / sqrt(16)
    # the draws, in order: the four embeddings' normal fills (nothing drawn and thrown away before them), then the layers, the head last
    torch.manual_seed(5)
    for emb in (m.user_mat_mf, m.item_mat_mf, m.user_mat_mlp, m.item_mat_mlp):
        assert torch.equal(torch.empty_like(emb.weight).normal_(std=0.01), emb.weight.detach())
    assert torch.equal(torch.nn.Linear(16, 8).weight, m.fc[0].weight) and torch.equal(torch.nn.Linear(16, 1).weight, m.head.weight)
    again = _cpu_model()
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), again.parameters()))
    U, V, dense = m.tables()
    S = nmf.check_model(U.numpy(), V.numpy(), dense.numpy(), 8, [16, 8], 11, 7)
    W, b, h, c = S.unpack(dense.numpy())
    assert np.array_equal(W[0], m.fc[0].weight.detach().numpy()) and np.array_equal(h, m.head.weight.detach().numpy()[0]) and c == float(m.head.bias.detach())
    state = torch.get_rng_state()
    back = NMF.from_tables(U, V, dense, 8, [16, 8])
    assert torch.equal(torch.get_rng_state(), state)                         # wrapping draws nothing
    assert all(torch.equal(a, b) for a, b in zip(back.tables(), (U, V, dense)))
    # the packed form is kept until a parameter changes
    assert all(a is b for a, b in zip(back.tables(), back.tables()))
    with torch.no_grad():
        back.head.bias.add_(1.0)
    assert float(back.tables()[2][S.c_at]) == float(dense[S.c_at] + 1.0)
    back.user_mat_mf.weight = torch.nn.Parameter(torch.zeros(11, 8), requires_grad=False)
    assert not back.tables()[0][:, :8].any() and torch.equal(back.tables()[0][:, 8:], U[:, 8:])
    assert set(back.state_dict()) == set(m.state_dict())
    with pytest.raises(ValueError, match='nmf'):
        NMF(11, 7, 8, [16])


def test_refusal_table():
    """Everything that needs a two-table dot model names the backbone in a ValueError (no AttributeError, no device work)."""
    from ultrare_amd import _native
    from ultrare_amd.config import InsParam
    from ultrare_amd.method import sisa, utils
    m = _cpu_model()
    loader = (np.array([0, 1]), np.array([0, 1]), np.array([0.2, 0.4], np.float32))
    calls = {
        'recommend': lambda: utils.recommend([m], [0, 1]),
        'rank_eval': lambda: utils.rank_eval([m], None),
        'fit_combiner': lambda: utils.fit_combiner([m], None),
        'fold_in': lambda: utils.fold_in([m], loader, 0.1),
        'als_sweeps': lambda: utils.als_sweeps(m, loader, 0.1),
        'attribute_unlearn': lambda: utils.attribute_unlearn(m, [0], [1]),
        'newton_unlearn': lambda: utils.newton_unlearn(m, loader, l2=0.1),
        'padded_tables': lambda: utils.padded_tables(m),
        'baseTest\\(combiner=\\)': lambda: utils.baseTest(None, [m], combiner=object()),
    }
    for who, call in calls.items():
        with pytest.raises(ValueError, match=who + ".*'nmf' backbone"):
            call()
    with pytest.raises(ValueError, match='one backbone'):
        utils.baseTest(None, [m, utils.MF(11, 7, 8)])
    with pytest.raises(_native.NativeError, match='HIP device'):
        m(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
    p = InsParam('toy', 2, data_dir=os.path.join(ROOT, 'tests', 'golden'), model='nmf', layers=[16, 8], k=8)
    s = sisa.Sisa(p, 'nmf', 2, [[0], [1]])
    s.model_list = [m, m]
    for who, call in (('recommend', lambda: s.recommend([0])), ('rank_eval', lambda: s.rank_eval(None)), ('fit_combiner', lambda: s.fit_combiner([None, None])),
                      ('test_combined', lambda: s.test_combined(None, 0, '')), ('fold_in', lambda: s.fold_in(loader, 0.1)),
                      ('attribute_unlearn', lambda: s.attribute_unlearn([0], [1]))):
        with pytest.raises(ValueError, match=f"Sisa.{who} .*'nmf' backbone"):
            call()
    with pytest.raises(ValueError, match="model='mf' only, not 'nmf'"):
        s.unlearn_influence([m, m], [None, None], None, [0], 0, '')


def test_ops_refuse_cpu_tensors_and_bad_stacks():
    from ultrare_amd import _native, ops  # noqa: F401
    z = torch.zeros
    S = nmf.Shape(8, [16, 8])
    args = (z(3, S.wd), z(4, S.wd), z(S.n_dense))
    with pytest.raises(_native.NativeError, match='HIP device only'):
        torch.ops.ultrare.nmf_score(*args, 8, [16, 8], z(2, dtype=torch.int64), z(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='nmf'):
        torch.ops.ultrare.nmf_score(*args, 8, [16, 6], z(2, dtype=torch.int64), z(2, dtype=torch.int64))
