"""Adversarial attribute unlearning on the device (-m gpu): csrc/adv.hip held to the numpy contract of ultrare_amd/adv_unlearn.py.

  bit for bit   the device's own p is handed to input_grad_ref(..., p = p_dev, dtype = float32): everything after the sigmoid is
                pure float32, so grad must then be the contract's bytes.  p_dev itself is the contract's float32 p or one float32
                ulp away (the float64 exp's last bit: the family's stated exception).
  by the rule   without the hand-over, with E_k the device's distance from the float64 contract and E_y the float32 contract's, both
                relative to the largest float64 magnitude of the array: E_k <= 4 max(E_y, ulp32) -- the rule and factor of
                tests/test_gpu_sgd.py and tests/test_gpu_attack.py.  Three whole rounds of the game under the same rule; the pair
                counts within what the score bound allows (only a pair whose float64 p are closer than twice the bound can be ordered
                differently).  No long run is compared: the game amplifies last-bit differences.
  the outcome   the default fine-tune on the planted table, judged by a fresh attacker: AUC <= 0.65 after, >= 0.98 before.
"""
import os

import numpy as np
import pytest
import torch

import adv_cases as D
import attack_cases as C
from abi_arena import Arena, run_prefills, verdict
from ultrare_amd import adv_unlearn as V
from ultrare_amd import attack as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
ULP32 = 2.0 ** -24
TARGETS = [(0.0, 1.0), (0.5, 0.5)]
N_USER, N_ITEM = 1508, 2071


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import _native
    return _native


def _wide(x, ld, seed, fill=float('nan')):
    """tests/test_gpu_attack.py's construction: the rows of x at an unsorted selection of a wider table, `fill` everywhere else."""
    m, d = x.shape
    rs = np.random.RandomState(seed)
    rows = rs.permutation(2 * m + 7)[:m]
    W = np.full((2 * m + 7, ld), fill, dtype=np.float32)
    W[rows, :d] = x
    return W, rows


def _rel(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def _grad_raw(nv, c, H, target, W=None, rows=None, fold_of='own', want_p=True, stream=None, junk=None):
    """ure_adv_input_grad through the C ABI on the case c (adv_cases.probe) -> (grad, p or None) on the host."""
    m, d = c['x'].shape
    if W is None:
        W, rows = _wide(c['x'], d + 3, m + d)
    dev = torch.device('cuda')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fo = c['fold_of'] if isinstance(fold_of, str) else fold_of
    Wt, rows_d, params, stats, fw = up(W), up(rows.astype(np.int32)), up(c['params']), up(c['stats']), up(c['fw'])
    fo_d = perm_d = off_d = None
    if fo is not None:
        perm, off = V.fold_groups(fo, len(c['params']))
        fo_d, perm_d, off_d = up(fo.astype(np.int32)), up(perm), up(off)
    grad = torch.empty(m, d, dtype=torch.float32, device=dev)
    p = torch.empty(m, dtype=torch.float32, device=dev) if want_p else None
    if junk is not None:
        grad.view(torch.uint8).fill_(junk)
        if want_p:
            p.view(torch.uint8).fill_(junk)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    nv.check(nv.lib().ure_adv_input_grad(Wt.data_ptr(), Wt.stride(0), d, rows_d.data_ptr(), nv.ptr(fo_d), m, c['n1'], len(c['params']), H, stats.data_ptr(),
                                         params.data_ptr(), fw.data_ptr(), target[0], target[1], grad.data_ptr(), nv.ptr(p), nv.ptr(perm_d), nv.ptr(off_d),
                                         nv.stream_handle(stream)), 'ure_adv_input_grad')
    torch.cuda.synchronize()
    return grad.cpu().numpy(), (p.cpu().numpy() if want_p else None)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


M_OF = lambda folds: (folds, 255, 256, 257, 773)


@pytest.mark.parametrize('H', [0, 1, 7, 64, 100, 128])
@pytest.mark.parametrize('d', [1, 17, 32, 128])
def test_gradient_bit_for_bit_from_the_device_p_and_by_the_rule(nv, H, d):
    """Every m of M_OF under 2, 5 and 16 folds and both targets at this (H, d): unsorted rows of a wider NaN-filled table, ld > d."""
    for k, folds in [(k, folds) for k in range(5) for folds in (2, 5, 16)]:
        m = M_OF(folds)[k]
        c = D.probe(m, d, H, folds, 1000 * H + 10 * d + k)
        args = (c['params'], c['stats'], c['x'], c['y'], c['fold_of'], c['fw'])
        for target in TARGETS:
            g, p = _grad_raw(nv, c, H, target)
            g32, p32 = V.input_grad_ref(*args, target, H, dtype=np.float32)
            assert _ulps(p, p32).max() <= 1, (m, folds, target)
            want = V.input_grad_ref(*args, target, H, dtype=np.float32, p=p)[0]
            assert np.array_equal(g.view(np.int32), want.view(np.int32)), (m, folds, target)
            g64, p64 = V.input_grad_ref(*args, target, H, dtype=np.float64)
            e_k, e_y = _rel(g, g64), _rel(g32, g64)
            print(f'H {H} d {d} m {m} folds {folds} target {target}: E_k {e_k:.3g} E_y {e_y:.3g}, p within {int(_ulps(p, p32).max())} ulp')
            assert e_k <= 4 * max(e_y, ULP32), (m, folds, target)
            assert np.abs(p - p64).max() <= 4 * max(np.abs(p32 - p64).max(), ULP32)


def test_edges(nv):
    H, d, folds, m = 7, 17, 5, 300
    c = D.probe(m, d, H, folds, 3)
    args = (c['params'], c['stats'], c['x'], c['y'])
    # a fold_of entry outside [0, folds) gives a NaN row; a fold with no held-out position (3) is simply not met
    fo = c['fold_of'].copy()
    fo[fo == 3] = 1
    fo[[0, 44, 299]] = [folds, -1, 1 << 20]
    g, p = _grad_raw(nv, c, H, (0.5, 0.5), fold_of=fo)
    bad = np.zeros(m, dtype=bool)
    bad[[0, 44, 299]] = True
    assert np.isnan(g[bad]).all() and np.isnan(p[bad]).all() and np.isfinite(g[~bad]).all() and np.isfinite(p[~bad]).all()
    want = V.input_grad_ref(*args, fo, c['fw'], (0.5, 0.5), H, p=p)[0]
    assert np.array_equal(g.view(np.int32), want.view(np.int32))         # (NaN rows: the same quiet NaN)
    # fold_of NULL: set 0 serves every position (no plan is read)
    g0, p0 = _grad_raw(nv, c, H, (0.0, 1.0), fold_of=None)
    want = V.input_grad_ref(*args, None, c['fw'], (0.0, 1.0), H, p=p0)[0]
    assert np.array_equal(g0.view(np.int32), want.view(np.int32)) and np.isfinite(g0).all()
    # p_out NULL: the same gradient
    g1, none = _grad_raw(nv, c, H, (0.5, 0.5), want_p=False)
    g2, _ = _grad_raw(nv, c, H, (0.5, 0.5))
    assert none is None and g1.tobytes() == g2.tobytes()
    # n1 = 1 and n1 = 0 / m (one class only)
    for n1 in (1, 0, m):
        c1 = dict(c, n1=n1, y=(np.arange(m) < n1).astype(np.int64))
        g, p = _grad_raw(nv, c1, H, (0.0, 1.0))
        want = V.input_grad_ref(c['params'], c['stats'], c['x'], c1['y'], c['fold_of'], c['fw'], (0.0, 1.0), H, p=p)[0]
        assert np.array_equal(g.view(np.int32), want.view(np.int32)), n1
    # p is ure_attack_score's
    W, rows = _wide(c['x'], d + 3, m + d)
    Wt = torch.from_numpy(W).cuda()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    scores = torch.empty(m, dtype=torch.float32, device='cuda')
    held = [up(rows.astype(np.int32)), up(c['fold_of']), up(c['stats']), up(c['params'])]         # (kept alive across the launch)
    nv.check(nv.lib().ure_attack_score(Wt.data_ptr(), Wt.stride(0), d, held[0].data_ptr(), held[1].data_ptr(), m, folds, H, held[2].data_ptr(),
                                       held[3].data_ptr(), scores.data_ptr(), nv.stream_handle(None)), 'score')
    torch.cuda.synchronize()
    assert scores.cpu().numpy().tobytes() == _grad_raw(nv, c, H, (0.5, 0.5))[1].tobytes()


def test_equal_bytes_on_streams_calls_and_junk(nv):
    H, d, folds, m = 100, 33, 3, 600
    c = D.probe(m, d, H, folds, 8)
    W, rows = _wide(c['x'], d + 3, 9)
    W2 = _wide(c['x'], d + 3, 9, fill=1e30)[0]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    runs = [_grad_raw(nv, c, H, (0.5, 0.5), W, rows), _grad_raw(nv, c, H, (0.5, 0.5), W, rows, stream=s1, junk=0xFF),
            _grad_raw(nv, c, H, (0.5, 0.5), W2, rows, stream=s2, junk=0x00), _grad_raw(nv, c, H, (0.5, 0.5), W, rows, junk=0x5A)]
    for r in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], r))
    # the engine call and the torch op give the same bytes
    from ultrare_amd import engine
    import ultrare_amd.ops  # noqa: F401
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Wt = up(W)
    groups = engine.GroupRows(rows[:c['n1']], rows[c['n1']:], len(W), Wt.device)
    fit = engine.AttackFit(params=up(c['params']), stats=up(c['stats']), fw=up(c['fw']), fold_of=up(c['fold_of']), d=d, hidden=H, folds=folds)
    for stream in (None, s1):
        g, p = engine.attack_input_grad(fit, Wt[:, :d], groups, stream=stream)
        torch.cuda.synchronize()
        assert g.cpu().numpy().tobytes() == runs[0][0].tobytes() and p.cpu().numpy().tobytes() == runs[0][1].tobytes()
    assert engine.attack_input_grad(fit, Wt[:, :d], groups, want_p=False)[1] is None
    g, p = torch.ops.ultrare.attack_input_grad(Wt[:, :d], up(rows.astype(np.int32)), c['n1'], fit.fold_of, fit.params, fit.stats, fit.fw, H, 0.5, 0.5)
    assert g.cpu().numpy().tobytes() == runs[0][0].tobytes() and p.cpu().numpy().tobytes() == runs[0][1].tobytes()
    # the asymmetric target (0, 1) through the engine call and the op: a swapped pair would show; the op's fit has no host copy of
    # the folds, so its plan is built on the device -- with entries outside [0, folds) too
    raw01 = _grad_raw(nv, c, H, (0.0, 1.0), W, rows)
    assert raw01[0].tobytes() != runs[0][0].tobytes() and raw01[0].tobytes() != _grad_raw(nv, c, H, (1.0, 0.0), W, rows)[0].tobytes()
    g, p = engine.attack_input_grad(fit, Wt[:, :d], groups, target=(0.0, 1.0))
    assert g.cpu().numpy().tobytes() == raw01[0].tobytes() and p.cpu().numpy().tobytes() == raw01[1].tobytes()
    g, p = torch.ops.ultrare.attack_input_grad(Wt[:, :d], up(rows.astype(np.int32)), c['n1'], fit.fold_of, fit.params, fit.stats, fit.fw, H, 0.0, 1.0)
    assert g.cpu().numpy().tobytes() == raw01[0].tobytes() and p.cpu().numpy().tobytes() == raw01[1].tobytes()
    fo = c['fold_of'].copy()
    fo[[5, 77, 599]] = [folds, -3, 1 << 20]
    raw_bad = _grad_raw(nv, c, H, (0.0, 1.0), W, rows, fold_of=fo)
    g, p = torch.ops.ultrare.attack_input_grad(Wt[:, :d], up(rows.astype(np.int32)), c['n1'], up(fo), fit.params, fit.stats, fit.fw, H, 0.0, 1.0)
    assert np.isnan(raw_bad[1][[5, 77, 599]]).all() and int(np.isnan(raw_bad[1]).sum()) == 3
    assert g.cpu().numpy().tobytes() == raw_bad[0].tobytes() and p.cpu().numpy().tobytes() == raw_bad[1].tobytes()
    with pytest.raises(ValueError, match='params'):
        torch.ops.ultrare.attack_input_grad(Wt[:, :d], up(rows.astype(np.int32)), c['n1'], fit.fold_of, fit.params[:, :-1], fit.stats, fit.fw, H, 0.5, 0.5)
    with pytest.raises(ValueError, match='target'):
        engine.attack_input_grad(fit, Wt[:, :d], groups, target=(0.5, float('nan')))


# ---- the memory contract ------------------------------------------------------------------------------------------------------------
def _arena_case(nv, want_p):
    L = nv.lib()
    m, d, H, folds = 300, 17, 7, 3
    c = D.probe(m, d, H, folds, 4)
    W, rows = _wide(c['x'], d + 3, 1)
    perm, off = V.fold_groups(c['fold_of'], folds)
    ar = Arena('cuda')
    st = nv.stream_handle(None)
    ar.input('X', W), ar.input('rows', rows.astype(np.int32)), ar.input('fold_of', c['fold_of']), ar.input('stats', c['stats'])
    ar.input('params', c['params']), ar.input('fw', c['fw']), ar.input('perm', perm), ar.input('off', off)
    ar.output('grad', 4 * m * d)
    if want_p:
        ar.output('p', 4 * m)
    return ar, lambda a: nv.check(L.ure_adv_input_grad(a.addr('X'), W.shape[1], d, a.addr('rows'), a.addr('fold_of'), m, c['n1'], folds, H, a.addr('stats'),
                                                       a.addr('params'), a.addr('fw'), 0.5, 0.5, a.addr('grad'), a.addr('p') if want_p else None,
                                                       a.addr('perm'), a.addr('off'), st), 'ure_adv_input_grad')


@pytest.mark.parametrize('want_p', [True, False])
def test_the_entry_on_dirty_memory_inside_guard_zones(nv, want_p):
    arena, call = _arena_case(nv, want_p)
    reports = run_prefills(arena, call, sync=torch.cuda.synchronize)
    assert verdict(reports) == []
    assert set(nv.ADV_EXPORTS) == {'ure_adv_input_grad'}          # every entry of the header is run above; there is no sizer


# ---- three rounds of the game -------------------------------------------------------------------------------------------------------
def test_three_rounds_within_the_float32_yardstick():
    from ultrare_amd import engine
    X, id1, id2 = C.table(True)
    s = D.SHORT
    m64, log64, rows, n1, n2, fold_of, p0, _ = D.play(X, id1, id2, np.float64, **s)
    m32, log32 = D.play(X, id1, id2, np.float32, **s)[:2]
    runs = []
    for stream in (None, torch.cuda.Stream()):
        Xt = torch.from_numpy(X).cuda()
        groups = engine.GroupRows(id1, id2, len(X), Xt.device)
        fit = engine.adversarial_unlearn(Xt, groups, s['hidden'], s['folds'], s['rounds'], s['disc_epochs'], s['disc_lr'], s['l2'], s['lr'], s['eta'],
                                         s['alpha'], (0.5, 0.5), s['seed'], stream=stream)
        torch.cuda.synchronize()
        runs.append((Xt.cpu().numpy(), fit))
    got, fit = runs[0]
    assert np.array_equal(fit.fold_host, fold_of)
    assert got.tobytes() == runs[1][0].tobytes() and torch.equal(fit.params, runs[1][1].params) and torch.equal(fit.counts, runs[1][1].counts)
    other = np.setdiff1d(np.arange(len(X)), rows)
    assert np.array_equal(got[other], X[other])
    for name, dev, a32, a64 in (('rows', got[rows], m32[rows], m64[rows].astype(np.float64)),
                                ('params', fit.params.cpu().numpy(), log32['params'], log64['params']),
                                ('grad', fit.grad.cpu().numpy(), log32['grad'], log64['grad']),
                                ('stats', fit.stats.cpu().numpy(), log32['stats'], log64['stats'])):
        e_k, e_y = _rel(dev, a64), _rel(a32, a64)
        print(f'{name}: E_k {e_k:.3g} E_y {e_y:.3g}')
        assert e_k <= 4 * max(e_y, ULP32), name
    p_dev = fit.scores.cpu().numpy()
    bound = 4 * max(np.abs(log32['p'] - log64['p']).max(), ULP32)
    assert np.abs(p_dev - log64['p']).max() <= bound
    # the pair counts: equal to the counts of the device's own p, and within what the score bound allows of the float64 contract's
    counts = fit.counts.cpu().numpy()
    assert not fit.nan_flags.cpu().numpy().any()
    assert tuple(counts[-1]) == A.auc_counts_ref(p_dev, np.arange(n1), np.arange(n1, n1 + n2))
    for t in range(s['rounds']):
        p64 = log64['p_rounds'][t]
        b = 4 * max(np.abs(log32['p_rounds'][t] - p64).max(), ULP32)
        close = int((np.abs(p64[:n1, None] - p64[None, n1:]) < 2 * b).sum())
        gt64, eq64 = int((p64[:n1, None] > p64[None, n1:]).sum()), int((p64[:n1, None] == p64[None, n1:]).sum())
        print(f'round {t}: device {tuple(counts[t])} float64 {(gt64, eq64)}, {close} close pairs')
        assert abs(int(counts[t, 0]) - gt64) <= close and abs(int(counts[t, 0] + counts[t, 1]) - (gt64 + eq64)) <= close
    loss = fit.loss.cpu().numpy()
    assert loss.shape == (s['rounds'], s['folds'], s['disc_epochs'])
    assert np.abs(loss[:, :, 0] - log64['loss_first']).max() <= 1e-5 * log64['loss_first'].max()
    assert np.abs(loss[:, :, -1] - log64['loss_last']).max() <= 1e-5 * log64['loss_last'].max()
    assert np.allclose(fit.reg.cpu().numpy(), log64['reg'], rtol=1e-5)


# ---- the outcome on the device ------------------------------------------------------------------------------------------------------
def test_the_default_fine_tune_leaves_a_fresh_attacker_near_chance():
    from ultrare_amd.method import utils
    X, id1, id2 = C.table(True)
    rs = np.random.RandomState(0)
    V0 = torch.from_numpy(rs.randn(9, X.shape[1]).astype(np.float32)).cuda()
    model = utils.MF.from_tables(torch.from_numpy(X).cuda(), V0.clone())
    before = utils.attribute_attack(model, id1, id2, **C.SETTINGS)
    log = utils.adversarial_unlearn(model, id1, id2)
    after = utils.attribute_attack(model, id1, id2, **C.SETTINGS)
    rms = np.sqrt(log['reg'][-1] / (len(id1) + len(id2)))
    print(f"fresh attacker's AUC {before['auc']:.4f} -> {after['auc']:.4f}; in-loop AUC {log['auc'][0]:.4f} -> {log['auc'][-1]:.4f}; RMS row movement {rms:.3f}")
    assert before['auc'] >= 0.98
    assert after['auc'] <= D.AUC_CAP
    got = model.user_mat.weight.detach().cpu().numpy()
    other = np.setdiff1d(np.arange(len(X)), np.concatenate([id1, id2]))
    assert np.array_equal(got[other], X[other]) and torch.equal(model.item_mat.weight.detach(), V0)
    assert not np.array_equal(got[id1], X[id1])
    assert set(log) == {'disc_loss', 'auc', 'counts', 'reg', 'settings'} and len(log['auc']) == len(log['reg']) == 100
    assert np.array(log['disc_loss']['first']).shape == (100, 5) and log['settings']['hidden'] == 32 and log['settings']['target'] == 'confuse'
    with pytest.raises(ValueError, match='diverges'):
        utils.adversarial_unlearn(model, id1, id2, target='reverse')
    with pytest.raises(ValueError, match='at least folds'):
        utils.adversarial_unlearn(model, id1[:2], id2)
    from ultrare_amd import _native
    with pytest.raises(_native.NativeError):
        utils.adversarial_unlearn(utils.MF.from_tables(torch.from_numpy(X), V0.cpu()), id1, id2)
    assert np.array_equal(model.user_mat.weight.detach().cpu().numpy(), got)            # a refusal moves nothing
    bad = utils.MF.from_tables(torch.from_numpy(X).cuda(), V0.clone())
    bad.user_mat.weight.data[int(id1[0]), 0] = float('inf')
    with pytest.raises(ValueError, match='NaN'):
        utils.adversarial_unlearn(bad, id1, id2, rounds=1)


# ---- the surface --------------------------------------------------------------------------------------------------------------------
class Param:
    def __init__(self):
        self.k, self.lam, self.seed, self.batch = 16, 0.1, 42, 3000
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, 2
        self.n_user, self.n_item, self.parallel = N_USER, N_ITEM, True


def test_sisa_adversarial_unlearn_moves_own_shard_rows_only_and_unlearn_replaces_a_shard():
    import copy
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import MF
    from ultrare_amd.read import RatingData, loadData, readRating
    g = np.load(os.path.join(G, 'sisa_toy.npz'))
    U = torch.from_numpy(g['S3_learn_Umerged']).cuda()
    groups = [g[f'S3_index{i}'].tolist() for i in range(3)]
    sisa = Sisa(Param(), 'mf', 3, groups)
    with pytest.raises(ValueError, match='learn first'):
        sisa.adversarial_unlearn([0, 1], [2, 3])
    sisa.model_list = [MF.from_tables(U, torch.from_numpy(g[f'S3_learn_V{i}']).cuda()) for i in range(3)]
    sisa.combiner = object()
    sisa._group_rows_key = 'stale'
    before = U.clone()
    V_before = [m.item_mat.weight.detach().clone() for m in sisa.model_list]
    # id1 from every shard, id2 from shards 0 and 1 only: shard 2 is short of one side
    id1 = groups[0][:40] + groups[1][:30] + groups[2][:20]
    id2 = groups[0][40:90] + groups[1][30:75] + groups[2][20:22]
    kw = dict(hidden=4, folds=3, rounds=4, lr=0.5)
    with pytest.raises(ValueError, match='rounds'):
        sisa.adversarial_unlearn(id1, id2, rounds=0)
    with pytest.raises(TypeError, match='unexpected'):
        sisa.adversarial_unlearn(id1, id2, steps=3)
    assert torch.equal(sisa.model_list[0].user_mat.weight.detach(), before) and sisa.combiner is not None
    logs = sisa.adversarial_unlearn(id1, id2, **kw)
    assert len(logs) == 3 and 'skipped' in logs[2] and logs[2]['rows'] == (20, 2) and 'folds = 3' in logs[2]['skipped']
    assert logs[0]['rows'] == (40, 50) and logs[1]['rows'] == (30, 45) and len(logs[0]['auc']) == 4 and logs[0]['settings']['hidden'] == 4
    assert sisa.combiner is None and sisa._group_rows_key is None
    after = sisa.model_list[0].user_mat.weight.detach()
    assert all(m.user_mat.weight.data_ptr() == after.data_ptr() for m in sisa.model_list)
    changed = set(torch.nonzero((after != before).any(dim=1)).reshape(-1).tolist())
    own = (set(groups[0]) | set(groups[1])) & (set(id1) | set(id2))
    assert changed and changed <= own and not changed & set(groups[2]) and len(changed) > len(own) // 2
    for m, V0 in zip(sisa.model_list, V_before):
        assert torch.equal(m.item_mat.weight.detach(), V0)
    # a following unlearn of users of shard 1 retrains that shard: its rows are replaced, the moved rows of shard 0 stay
    moved = after.clone()
    del_user = [int(u) for u in groups[1][100:105]]
    train, test = os.path.join(G, 'toy', '0_train.csv'), os.path.join(G, 'toy', '0_test.csv')
    tr, idx = readRating(train, N_USER, 5, del_user, [], 3, groups)
    te, _ = readRating(test, N_USER, 5, [], [], 3, idx)
    trd = [loadData(RatingData(a), 3000, 24) for a in tr]
    ted = [loadData(RatingData(a), 3000, 24, False) for a in te]
    tot = loadData(RatingData(np.hstack(te)), 3000, 24, False)
    s2 = Sisa(Param(), 'mf', 3, idx)
    torch.manual_seed(42)
    ml2 = s2.unlearn([copy.deepcopy(m) for m in sisa.model_list], trd, ted, tot, del_user, 0, '')
    assert s2.retrained == [1]
    final = ml2[0].user_mat.weight.detach()
    keep0 = torch.tensor(sorted(set(groups[0]) & changed), device='cuda')
    redo1 = torch.tensor(sorted(set(idx[1]) & changed), device='cuda')
    assert len(keep0) and len(redo1)
    assert torch.equal(final[keep0], moved[keep0]) and bool((final[redo1] != moved[redo1]).any(dim=1).all())


def _toy_cli(tmp_path, name, extra):
    """main.py on the toy set, 2 uniform shards, one epoch -> (save dir, the sorted relative paths of every file it wrote)."""
    import shutil
    from ultrare_amd import main
    data = tmp_path / 'data' / 'toy'
    if not data.exists():
        os.makedirs(data)
        for f in ('0_train.csv', '0_test.csv'):
            shutil.copy(os.path.join(G, 'toy', f), data / f)
    save = str(tmp_path / name)
    torch.manual_seed(42)
    main.main(['--dataset', 'toy', '--epoch', '1', '--verbose', '0', '--group', '2', '--group-type', 'uniform', '--parallel', '0',
               '--data-dir', str(tmp_path / 'data'), '--save-dir', save] + extra)
    return save, sorted(os.path.relpath(os.path.join(d, f), save).replace(os.sep, '/') for d, _, files in os.walk(save) for f in files)


def _same_file(a, b):
    with open(a, 'rb') as fa, open(b, 'rb') as fb:
        return fa.read() == fb.read()


def test_main_adv_unlearn_writes_its_files_and_changes_no_other_artifact(tmp_path, capsys):
    attr = str(tmp_path / 'groups.npz')
    np.savez(attr, id1=np.arange(0, 1508, 2), id2=np.arange(1, 1508, 2))
    plain_dir, plain = _toy_cli(tmp_path, 'plain', [])
    capsys.readouterr()
    save, got = _toy_cli(tmp_path, 'adv', ['--adv-unlearn', '--adv-rounds', '3', '--adv-hidden', '4', '--attack', '--attack-hidden', '4', '--attack-folds', '3',
                                           '--attr-file', attr])
    out = capsys.readouterr().out
    assert out.count('adversarial unlearning (hidden 4, 3 rounds): 2 of 2 parts moved') == 2 and out.count('attribute attacker (hidden 4, 3 folds)') == 2
    added = sorted(set(got) - set(plain))
    assert not set(plain) - set(got) and len(added) == 4          # learn and unlearn: adv0.npy and attack0.npy each
    assert sum(n.endswith('/adv0.npy') for n in added) == 2 and sum(n.endswith('/attack0.npy') for n in added) == 2
    tables = [n for n in plain if os.path.basename(n).startswith(('user_mat', 'item_mat')) or os.path.basename(n) == 'log0.npy']
    assert len(tables) >= 6         # (log<id>.npy holds wall-clock times: not compared)
    for n in tables:                # the saved tables are training's, and the unlearn stage started from the trained rows
        assert _same_file(os.path.join(plain_dir, n), os.path.join(save, n)), n
    for n in added:
        if n.endswith('/adv0.npy'):
            assert os.path.exists(os.path.join(save, os.path.dirname(n), 'log0.npy'))
            res = np.load(os.path.join(save, n), allow_pickle=True).item()
            after = np.load(os.path.join(save, os.path.dirname(n), 'attack0.npy'), allow_pickle=True).item()
            assert set(res) == {'logs', 'attack_before', 'ids', 'rows'} and len(res['logs']) == 2 and res['rows'].shape == (1508, 16)
            assert res['attack_before']['settings'] == after['settings'] and res['attack_before']['counts'] != after['counts']
            assert all(len(g['auc']) == 3 for g in res['logs'])
    assert not any('adv0' in n for n in plain)
    # without --attack: adv<id>.npy alone
    _, alone = _toy_cli(tmp_path, 'alone', ['--adv-unlearn', '--adv-rounds', '2', '--adv-hidden', '0', '--attr-file', attr])
    extra = sorted(set(alone) - set(plain))
    assert len(extra) == 2 and all(n.endswith('/adv0.npy') for n in extra)
    with pytest.raises(ValueError, match='--adv-unlearn needs --attr-file'):
        _toy_cli(tmp_path, 'refused', ['--adv-unlearn'])
    assert not os.path.exists(tmp_path / 'refused')
