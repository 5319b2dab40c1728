"""The attribute-inference attacker on the device (-m gpu): csrc/attack.hip held to the numpy contract of ultrare_amd/attack.py.

  pair counts   equal integers to attack.auc_counts_ref / confusion_ref.  The tile geometry is 256 positives per workgroup
                (URE_AUC_TILE_POS), 1024 negatives per LDS tile (URE_AUC_TILE_NEG) and at most 128 splits of the negatives: the sizes
                cross every one of these edges.
  statistics    bit for bit.
  one epoch     the gradient chunk sums and the updated parameters within the float32-execution yardstick: with E_k the device's
                distance from the float64 contract and E_y the float32 contract's, both relative to the largest float64 magnitude of
                the array, E_k <= 4 max(E_y, ulp32) -- the rule and factor of tests/test_gpu_sgd.py.  The kernel offers no hook that
                replaces exp by a table, so the bit-for-bit half of that comparison is not made here.  (p is the float64 sigmoid of
                the float32 logit rounded once, on the device and in the contract: with expf in the kernel the case H = 128, d = 32,
                m = 773, folds = 5 missed this rule by a factor of 1.2 at the parameters after one Adam step.)
  training      the same rule on the out-of-fold scores (absolute: they lie in [0, 1]) of the planted, null and logistic cases, and
                the device's AUC within the bound derived from it.
  recorded      the bytes of tests/probe_cases.py's cases (training, scoring, the input gradient) equal to the digests recorded in
                tests/golden/probe_parent_bytes.json before attack.hip and adv.hip shared probe.h: the rule above bounds an error,
                this pins the summation orders.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import attack_cases as C
from abi_arena import Arena, run_prefills, verdict
from ultrare_amd import attack as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
ULP32 = 2.0 ** -24
AUC_POS, AUC_NEG, AUC_SPLITS = 256, 1024, 128


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import _native
    return _native


def _wide(x, ld, seed, fill=float('nan')):
    """(table [2 m + 7, ld] with the rows of x at an unsorted selection and `fill` in every other row and padding column, rows)."""
    m, d = x.shape
    rs = np.random.RandomState(seed)
    rows = rs.permutation(2 * m + 7)[:m]
    W = np.full((2 * m + 7, ld), fill, dtype=np.float32)
    W[rows, :d] = x
    return W, rows


# ---- pair counts --------------------------------------------------------------------------------------------------------------------
def _counts(scores, pos, neg, stream=None):
    from ultrare_amd import engine
    s = torch.from_numpy(np.ascontiguousarray(scores)).cuda()
    counts, flag = engine.auc_counts(s, np.asarray(pos), np.asarray(neg), stream=stream)
    conf = engine.confusion_counts(s, np.asarray(pos), np.asarray(neg), stream=stream)
    torch.cuda.synchronize()
    return tuple(counts.tolist()), int(flag), tuple(conf.tolist())


@pytest.mark.parametrize('name', sorted(C.score_cases()))
def test_pair_counts_on_the_cpu_cases(name):
    scores, pos, neg = C.score_cases()[name]
    got, flag, conf = _counts(scores, pos, neg)
    assert got == A.auc_counts_ref(scores, pos, neg) and flag == 0
    assert got != A.auc_counts_ref(scores, pos, neg, plant='ties_as_wins') or name in ('random', 'one_positive', 'one_negative')
    assert conf == A.confusion_ref(scores, pos, neg)


def test_pair_counts_cross_every_tile_edge():
    """pos / neg are unsorted index lists into a wider NaN-filled score array; the scores are quantised so that ties are common."""
    sizes = (1, 63, 64, 65, 255, 256, 257, 1025)
    rs = np.random.RandomState(5)
    n = 2 * 1025 + 50
    wide = np.full(n, np.nan, dtype=np.float32)
    pick = rs.permutation(n)[:2 * 1025]
    wide[pick] = (np.floor(rs.rand(2 * 1025) * 64) / 64).astype(np.float32)
    assert AUC_POS in sizes and 1025 > AUC_NEG
    for n1 in sizes:
        for n2 in sizes:
            pos, neg = pick[:n1], pick[1025:1025 + n2]
            got, flag, conf = _counts(wide, pos, neg)
            assert got == A.auc_counts_ref(wide, pos, neg) and flag == 0, (n1, n2)
            assert conf == A.confusion_ref(wide, pos, neg), (n1, n2)
    # more negative tiles than splits: a workgroup walks several
    n2 = AUC_NEG * AUC_SPLITS + AUC_NEG + 1
    big = (np.floor(rs.rand(n2 + 3) * 16) / 16).astype(np.float32)
    pos, neg = np.array([n2, n2 + 2, n2 + 1]), rs.permutation(n2)
    got, flag, _ = _counts(big, pos, neg)
    assert got == A.auc_counts_ref(big, pos, neg) and flag == 0


def test_a_selected_nan_raises_the_flag():
    s = np.array([0.1, np.nan, 0.3, 0.2], dtype=np.float32)
    assert _counts(s, [0], [2, 3])[1] == 0
    assert _counts(s, [1], [2, 3])[1] == 1 and _counts(s, [0, 2], [3, 1])[1] == 1
    from ultrare_amd import engine
    with pytest.raises(ValueError, match='outside'):
        engine.auc_counts(torch.from_numpy(s).cuda(), [0], [4])
    with pytest.raises(ValueError, match='outside'):
        engine.confusion_counts(torch.from_numpy(s).cuda(), torch.tensor([-1]).cuda(), [1])


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def _standardize(nv, Wt, d, rows, fold_of, folds, stream=None):
    dev = Wt.device
    rows_d, fold_d = torch.from_numpy(rows.astype(np.int32)).to(dev), torch.from_numpy(fold_of.astype(np.int32)).to(dev)
    stats = torch.full((folds, 2, d), float('nan'), dtype=torch.float32, device=dev)
    nv.check(nv.lib().ure_attack_standardize(Wt.data_ptr(), Wt.stride(0), d, rows_d.data_ptr(), fold_d.data_ptr(), len(rows), folds, stats.data_ptr(),
                                             nv.stream_handle(stream)), 'ure_attack_standardize')
    torch.cuda.synchronize()
    return stats.cpu().numpy()


@pytest.mark.parametrize('d', [1, 3, 16, 17, 32, 33, 64, 127, 128])
def test_standardize_bit_for_bit(nv, d):
    rs = np.random.RandomState(d)
    for m, folds in ((2 * 16, 16), (300, 5), (513, 2)):
        x = (rs.randn(m, d) * (1 + rs.rand(d) * 4) + rs.randn(d) * 3).astype(np.float32)
        if d > 1:
            x[:, d - 1] = np.float32(0.7)           # a zero-variance column
        W, rows = _wide(x, d + 5, d + m)
        fold_of = A.fold_plan(m // 3, m - m // 3, folds, d)
        got = _standardize(nv, torch.from_numpy(W).cuda(), d, rows, fold_of, folds)
        want = A.standardize_ref(W[:, :d], rows, fold_of, folds)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (m, folds)
        if d > 1:
            assert not got[:, 1, d - 1].any()


# ---- one epoch from given parameters ------------------------------------------------------------------------------------------------
def _train_raw(nv, W, d, rows, n1, fold_of, p0, H, epochs, lr, l2, stream=None, junk=None):
    """ure_attack_standardize + ure_attack_train through the C ABI with a scratch of this test's own -> (params, loss, grad sums of
    the LAST epoch per fold, rebuilt from the chunk sums in the scratch: the header's layout)."""
    from ultrare_amd import adam, engine
    Wt = torch.from_numpy(W).cuda() if not torch.is_tensor(W) else W
    dev, L = Wt.device, nv.lib()
    m, folds, P = len(rows), len(p0), A.n_params(d, H)
    y = np.arange(m) < n1
    fw = np.zeros((folds, 4), dtype=np.float32)
    for f in range(folds):
        cw, mt = A.class_weights(y, fold_of != f)
        fw[f, :2], fw[f, 2] = cw, mt
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows_d, fold_d, fw_d, sc_d, p0_d = up(rows.astype(np.int32)), up(fold_of.astype(np.int32)), up(fw), up(A.scalars(epochs, lr)), up(p0.astype(np.float32))
    nbytes = int(L.ure_attack_scratch(m, d, H, folds))
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    scratch.fill_(0xFF if junk is None else junk)
    stats = torch.empty(folds, 2, d, dtype=torch.float32, device=dev)
    params = torch.empty(folds, P, dtype=torch.float32, device=dev)
    loss = torch.empty(folds, epochs, dtype=torch.float64, device=dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    st = nv.stream_handle(stream)
    b1, b2, eps = adam.betas32(A.BETAS, A.EPS)
    nv.check(L.ure_attack_standardize(Wt.data_ptr(), Wt.stride(0), d, rows_d.data_ptr(), fold_d.data_ptr(), m, folds, stats.data_ptr(), st), 'standardize')
    nv.check(L.ure_attack_train(Wt.data_ptr(), Wt.stride(0), d, rows_d.data_ptr(), fold_d.data_ptr(), m, n1, folds, H, stats.data_ptr(), fw_d.data_ptr(),
                                sc_d.data_ptr(), epochs, b1, b2, eps, float(np.float32(l2)), p0_d.data_ptr(), params.data_ptr(), loss.data_ptr(),
                                scratch.data_ptr(), nbytes, st), 'ure_attack_train')
    torch.cuda.synchronize()
    chunks = -(-m // A.CHUNK)
    raw = scratch.cpu().numpy()
    off = 8 * folds * chunks + 8 * folds
    part = raw[off:off + 4 * folds * chunks * P].view(np.float32).reshape(folds, chunks, P)
    g = part[:, 0].copy()
    for j in range(1, chunks):
        g = g + part[:, j]
    return params.cpu().numpy(), loss.cpu().numpy(), g


def _rel(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


M_OF = lambda folds: (2 * folds, A.CHUNK - 1, A.CHUNK, A.CHUNK + 1, 3 * A.CHUNK + 5)


@pytest.mark.parametrize('H', [0, 1, 7, 64, 100, 128])
@pytest.mark.parametrize('d', [1, 17, 32, 128])
def test_one_epoch_from_given_parameters(nv, H, d):
    """Every m of M_OF under both fold counts at this (H, d)."""
    rs = np.random.RandomState(1000 * H + d)
    for k, folds in [(k, folds) for k in range(5) for folds in (2, 5)]:
        m = M_OF(folds)[k]
        n1 = max(folds, m // 3)
        x = rs.randn(m, d).astype(np.float32)
        x[:n1] += np.float32(0.5)
        W, rows = _wide(x, d + 3, m + d)
        fold_of = A.fold_plan(n1, m - n1, folds, k)
        p0 = (A.init_params(d, H, folds, k) + rs.uniform(-0.05, 0.05, (folds, A.n_params(d, H)))).astype(np.float32)      # (biases off zero)
        params, loss, g = _train_raw(nv, W, d, rows, n1, fold_of, p0, H, 1, 1e-2, 1e-3)
        ref = {T: A.train_ref(W[:, :d], rows, n1, fold_of, p0, H, 1, 1e-2, 1e-3, dtype=T, keep_first_grad=True) for T in (np.float32, np.float64)}
        for name, got in (('grad0', g), ('params', params)):
            e_k, e_y = _rel(got, ref[np.float64][name]), _rel(ref[np.float32][name], ref[np.float64][name])
            print(f'H {H} d {d} m {m} folds {folds} {name}: E_k {e_k:.3g} E_y {e_y:.3g}')
            assert e_k <= 4 * max(e_y, ULP32), (name, m, folds)
        assert np.abs(loss - ref[np.float64]['loss']).max() <= 1e-5 * np.abs(ref[np.float64]['loss']).max()


# ---- whole training -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained():
    """{case: (device fit, float64 contract, float32 contract, n1, n2, fold_of)} -- computed once, shared, left unchanged."""
    from ultrare_amd import engine
    out = {}
    for case, planted, settings in (('planted', True, C.SETTINGS), ('null', False, C.SETTINGS), ('logistic', True, C.LOGISTIC)):
        X, id1, id2 = C.table(planted)
        r64, rows, n1, n2, fold_of, p0 = C.fit_contract(X, id1, id2, settings, np.float64)
        r32 = C.fit_contract(X, id1, id2, settings, np.float32)[0]
        Xt = torch.from_numpy(X).cuda()
        s = settings
        fit = engine.attack_fit(Xt, engine.GroupRows(id1, id2, len(X), Xt.device), s['hidden'], s['folds'], s['epochs'], s['lr'], s['l2'], s['seed'])
        torch.cuda.synchronize()
        assert np.array_equal(fit.fold_host, fold_of)
        out[case] = (fit, r64, r32, n1, n2, fold_of)
    return out


@pytest.mark.parametrize('case', ['planted', 'null', 'logistic'])
def test_whole_training_within_the_float32_yardstick(trained, case):
    fit, r64, r32, n1, n2, fold_of = trained[case]
    scores = fit.scores.cpu().numpy()
    e_k, e_y = np.abs(scores - r64['scores']).max(), np.abs(r32['scores'] - r64['scores']).max()
    print(f'{case}: E_k {e_k:.3g} E_y {e_y:.3g}')
    assert e_k <= 4 * max(e_y, ULP32)
    assert np.array_equal(fit.stats.cpu().numpy().view(np.int32), r32['stats'].view(np.int32))
    assert _rel(fit.params.cpu().numpy(), r64['params']) <= 4 * max(_rel(r32['params'], r64['params']), ULP32)
    loss = fit.loss.cpu().numpy()
    assert loss.shape == r64['loss'].shape and np.abs(loss - r64['loss']).max() <= 1e-5 * r64['loss'].max()


@pytest.mark.parametrize('case', ['planted', 'null', 'logistic'])
def test_device_auc_within_the_derived_bound(trained, case):
    """Only a pair whose float64 scores are closer than twice the score bound can be ordered differently by the device."""
    from ultrare_amd import engine
    fit, r64, r32, n1, n2, fold_of = trained[case]
    bound = 4 * max(np.abs(r32['scores'] - r64['scores']).max(), ULP32)
    s64 = r64['scores']
    close = int((np.abs(s64[:n1, None] - s64[None, n1:]) < 2 * bound).sum())
    pos, neg = np.arange(n1), np.arange(n1, n1 + n2)
    counts, flag = engine.auc_counts(fit.scores, pos, neg)
    gt, eq = counts.tolist()
    assert int(flag) == 0 and (gt, eq) == A.auc_counts_ref(fit.scores.cpu().numpy(), pos, neg)
    auc_dev = (gt + eq / 2.0) / (n1 * n2)
    gt64 = int((s64[:n1, None] > s64[None, n1:]).sum())
    eq64 = int((s64[:n1, None] == s64[None, n1:]).sum())
    auc64 = (gt64 + eq64 / 2.0) / (n1 * n2)
    print(f'{case}: AUC device {auc_dev:.6f} float64 {auc64:.6f}, {close} close pairs')
    assert abs(auc_dev - auc64) <= close / (n1 * n2)


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------
def test_equal_bytes_on_streams_calls_and_junk(nv):
    rs = np.random.RandomState(2)
    m, d, H, folds, n1 = 300, 17, 7, 3, 120
    x = rs.randn(m, d).astype(np.float32)
    fold_of, p0 = A.fold_plan(n1, m - n1, folds, 0), A.init_params(d, H, folds, 0)
    W, rows = _wide(x, d + 3, 9)
    W2 = _wide(x, d + 3, 9, fill=1e30)[0]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    runs = [_train_raw(nv, W, d, rows, n1, fold_of, p0, H, 3, 1e-2, 1e-3),
            _train_raw(nv, W, d, rows, n1, fold_of, p0, H, 3, 1e-2, 1e-3, stream=s1),
            _train_raw(nv, W, d, rows, n1, fold_of, p0, H, 3, 1e-2, 1e-3, stream=s2, junk=0x00),
            _train_raw(nv, W2, d, rows, n1, fold_of, p0, H, 3, 1e-2, 1e-3, junk=0x5A)]
    for r in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], r))
    from ultrare_amd import engine
    fits = []
    for Wx, stream in ((W, None), (W2, s1), (W, s2)):
        Wt = torch.from_numpy(Wx).cuda()
        g = engine.GroupRows(rows[:n1], rows[n1:], len(Wx), Wt.device)
        fits.append(engine.attack_fit(Wt[:, :d], g, H, folds, 3, 1e-2, 1e-3, seed=0, stream=stream))
    torch.cuda.synchronize()
    for f in fits[1:]:
        assert torch.equal(f.scores, fits[0].scores) and torch.equal(f.params, fits[0].params) and torch.equal(f.loss, fits[0].loss)
    assert fits[0].params.cpu().numpy().tobytes() == runs[0][0].tobytes()
    # transfer: one parameter set on other rows is attack.score_ref within the rule's floor
    got = engine.attack_scores(fits[0], torch.from_numpy(W).cuda()[:, :d], rows[::-1].copy(), fold=1).cpu().numpy()
    want = A.score_ref(W[:, :d], rows[::-1], None, fits[0].params.cpu().numpy()[1:2], fits[0].stats.cpu().numpy()[1:2], H)
    assert np.abs(got - want).max() <= 4 * ULP32


def test_probe_bytes_are_the_recorded_ones(nv):
    """Every case of tests/probe_cases.py gives the bytes recorded in tests/golden/probe_parent_bytes.json from the commit before
    attack.hip and adv.hip shared probe.h: a refactor of the probe's kernels that reorders a chain shows here, not under the rule above."""
    import json
    import probe_cases as PC
    with open(os.path.join(G, 'probe_parent_bytes.json')) as f:
        want = json.load(f)
    assert sorted(want['cases']) == sorted(PC.name(case) for case in PC.CASES)
    off = []
    for case in PC.CASES:
        got = PC.digests(nv, _train_raw, case)
        assert set(got) == set(want['cases'][PC.name(case)])
        off += [(PC.name(case), k) for k in sorted(got) if got[k] != want['cases'][PC.name(case)][k]]
    assert not off, f"recorded under HIP {want['torch_version_hip']}, run under {torch.version.hip}: {off}"


# ---- the memory contract ------------------------------------------------------------------------------------------------------------
def _arena_case(nv, entry):
    """(arena, call) of one entry at a small shape with an odd width and a tail chunk."""
    L = nv.lib()
    rs = np.random.RandomState(4)
    m, d, H, folds, n1, epochs = 300, 17, 7, 3, 120, 2
    W, rows = _wide(rs.randn(m, d).astype(np.float32), d + 3, 1)
    fold_of, p0 = A.fold_plan(n1, m - n1, folds, 0), A.init_params(d, H, folds, 0)
    stats = A.standardize_ref(W[:, :d], rows, fold_of, folds)
    P = A.n_params(d, H)
    fw = np.zeros((folds, 4), dtype=np.float32)
    for f in range(folds):
        cw, mt = A.class_weights(np.arange(m) < n1, fold_of != f)
        fw[f, :2], fw[f, 2] = cw, mt
    ar = Arena('cuda')
    st = nv.stream_handle(None)
    if entry in ('ure_attack_standardize', 'ure_attack_train', 'ure_attack_score'):
        ar.input('X', W), ar.input('rows', rows.astype(np.int32)), ar.input('fold_of', fold_of.astype(np.int32))
        head = lambda a: (a.addr('X'), W.shape[1], d, a.addr('rows'), a.addr('fold_of'), m)
    if entry == 'ure_attack_standardize':
        ar.output('stats', 4 * folds * 2 * d)
        return ar, lambda a: nv.check(L.ure_attack_standardize(*head(a), folds, a.addr('stats'), st), entry)
    if entry == 'ure_attack_train':
        from ultrare_amd import adam
        b1, b2, eps = adam.betas32(A.BETAS, A.EPS)
        ar.input('stats', stats), ar.input('fw', fw), ar.input('sc', A.scalars(epochs, 1e-2)), ar.input('p0', p0)
        ar.output('params', 4 * folds * P), ar.output('loss', 8 * folds * epochs)
        ar.scratch('ws', L.ure_attack_scratch(m, d, H, folds))
        return ar, lambda a: nv.check(L.ure_attack_train(*head(a), n1, folds, H, a.addr('stats'), a.addr('fw'), a.addr('sc'), epochs, b1, b2, eps, 1e-3,
                                                         a.addr('p0'), a.addr('params'), a.addr('loss'), a.addr('ws'), a.size('ws'), st), entry)
    if entry == 'ure_attack_score':
        ar.input('stats', stats), ar.input('params', p0)
        ar.output('scores', 4 * m)
        return ar, lambda a: nv.check(L.ure_attack_score(*head(a), folds, H, a.addr('stats'), a.addr('params'), a.addr('scores'), st), entry)
    scores = (np.floor(rs.rand(2500) * 32) / 32).astype(np.float32)
    idx = rs.permutation(2500).astype(np.int32)
    n1, n2 = 300, 1100
    ar.input('scores', scores), ar.input('pos', idx[:n1]), ar.input('neg', idx[n1:n1 + n2])
    if entry == 'ure_auc_counts':
        ar.output('counts', 16), ar.output('flag', 4)
        ar.scratch('ws', L.ure_auc_scratch(n1, n2))
        return ar, lambda a: nv.check(L.ure_auc_counts(a.addr('scores'), a.addr('pos'), n1, a.addr('neg'), n2, a.addr('counts'), a.addr('flag'), a.addr('ws'),
                                                       a.size('ws'), st), entry)
    assert entry == 'ure_confusion_counts'
    ar.output('counts', 32)
    return ar, lambda a: nv.check(L.ure_confusion_counts(a.addr('scores'), a.addr('pos'), n1, a.addr('neg'), n2, 0.5, a.addr('counts'), st), entry)


SIZERS = {'ure_attack_scratch', 'ure_auc_scratch'}
COVERED = ['ure_attack_standardize', 'ure_attack_train', 'ure_attack_score', 'ure_auc_counts', 'ure_confusion_counts']


@pytest.mark.parametrize('entry', COVERED)
def test_entries_on_dirty_memory_inside_guard_zones(nv, entry):
    arena, call = _arena_case(nv, entry)
    reports = run_prefills(arena, call, sync=torch.cuda.synchronize)
    assert verdict(reports) == []


def test_every_entry_is_covered(nv):
    assert set(COVERED) == set(nv.ATTACK_EXPORTS) - SIZERS


# ---- the surface --------------------------------------------------------------------------------------------------------------------
def _check_result(res, n1, n2, settings):
    c = res['counts']
    assert set(res) == {'auc', 'bacc', 'f1', 'fold_auc', 'counts', 'loss', 'settings'}
    assert c['tp'] + c['fn'] == n1 and c['tn'] + c['fp'] == n2 and 0 <= c['gt'] + c['eq'] <= n1 * n2
    assert res['auc'] == (c['gt'] + c['eq'] / 2.0) / (n1 * n2) and res == {**res, **A.metrics(c['gt'], c['eq'], c['tp'], c['fn'], c['tn'], c['fp'])}
    assert len(res['fold_auc']) == settings['folds'] == len(c['folds']) and sum(f['gt'] for f in c['folds']) <= c['gt']
    assert sum(f['n1'] for f in c['folds']) == n1 and sum(f['n2'] for f in c['folds']) == n2
    assert len(res['loss']['first']) == settings['folds'] and all(b < a for a, b in zip(res['loss']['first'], res['loss']['last']))
    assert {k: res['settings'][k] for k in settings} == settings


def test_attribute_attack_on_a_model_and_on_a_tensor(trained):
    from ultrare_amd.method import utils
    X, id1, id2 = C.table(True)
    Xt = torch.from_numpy(X).cuda()
    V = torch.zeros(5, X.shape[1], device='cuda')
    s = C.SETTINGS
    results = [utils.attribute_attack(src, id1, id2, **s) for src in (utils.MF.from_tables(Xt.clone(), V), Xt)]
    assert results[0] == results[1]
    _check_result(results[0], len(id1), len(id2), s)
    fit, r64, _, n1, n2, fold_of = trained['planted']
    gt, eq = A.auc_counts_ref(fit.scores.cpu().numpy(), np.arange(n1), np.arange(n1, n1 + n2))
    assert (results[0]['counts']['gt'], results[0]['counts']['eq']) == (gt, eq)
    assert torch.equal(Xt, torch.from_numpy(X).cuda())
    null = utils.attribute_attack(torch.from_numpy(C.table(False)[0]).cuda(), id1, id2, **s)
    assert null['auc'] < results[0]['auc']
    with pytest.raises(ValueError, match='at least folds'):
        utils.attribute_attack(Xt, id1[:1], id2, **s)
    with pytest.raises(nv_error()):
        utils.attribute_attack(torch.from_numpy(X), id1, id2, **s)
    wide = torch.zeros(10, 129, device='cuda')
    with pytest.raises(ValueError, match='width'):
        utils.attribute_attack(wide, [0, 1], [2, 3], folds=2)


def nv_error():
    from ultrare_amd import _native
    return _native.NativeError


class Param:
    def __init__(self):
        self.k, self.lam, self.seed, self.batch = 16, 0.1, 42, 3000
        self.lr, self.lr_decay, self.momentum, self.epochs = 0.001, 0.95, 0.9, 3
        self.n_user, self.n_item, self.parallel = 1508, 2071, True


def test_sisa_attribute_attack_changes_nothing():
    from ultrare_amd.method.sisa import Sisa
    from ultrare_amd.method.utils import MF
    g = np.load(os.path.join(G, 'sisa_toy.npz'))
    U = torch.from_numpy(g['S3_learn_Umerged']).cuda()
    groups = [g[f'S3_index{i}'].tolist() for i in range(3)]
    sisa = Sisa(Param(), 'mf', 3, groups)
    with pytest.raises(ValueError, match='learn first'):
        sisa.attribute_attack([0, 1], [2, 3], folds=2)
    sisa.model_list = [MF.from_tables(U, torch.from_numpy(g[f'S3_learn_V{i}']).cuda()) for i in range(3)]
    marker = object()
    sisa.combiner = marker
    sisa._group_rows_key = 'kept'
    before = [(m.user_mat.weight.detach().clone(), m.item_mat.weight.detach().clone()) for m in sisa.model_list]
    ptrs = [m.user_mat.weight.data_ptr() for m in sisa.model_list]
    id1 = groups[0][:40] + groups[1][:30] + groups[2][:20]
    id2 = groups[0][40:90] + groups[1][30:75]
    s = dict(hidden=4, folds=3, epochs=10, lr=1e-2, l2=1e-4, seed=1)
    res = sisa.attribute_attack(id1, id2, **s)
    _check_result(res, len(id1), len(id2), s)
    assert sisa.combiner is marker and sisa._group_rows_key == 'kept'
    assert ptrs == [m.user_mat.weight.data_ptr() for m in sisa.model_list]
    for m, (U0, V0) in zip(sisa.model_list, before):
        assert torch.equal(m.user_mat.weight.detach(), U0) and torch.equal(m.item_mat.weight.detach(), V0)
    assert res == sisa.attribute_attack(id1, id2, **s)


def test_the_two_ops(trained):
    import ultrare_amd.ops  # noqa: F401
    fit, r64, r32, n1, n2, fold_of = trained['planted']
    pos, neg = torch.arange(n1, device='cuda'), torch.arange(n1, n1 + n2, device='cuda', dtype=torch.int32)
    counts, flag = torch.ops.ultrare.auc_counts(fit.scores, pos, neg)
    assert tuple(counts.tolist()) == A.auc_counts_ref(fit.scores.cpu().numpy(), np.arange(n1), np.arange(n1, n1 + n2)) and int(flag) == 0
    X, id1, id2 = C.table(True)
    Xt = torch.from_numpy(X).cuda()
    held = np.flatnonzero(fold_of == 1)
    rows = torch.from_numpy(np.concatenate([id1, id2])[held]).cuda()
    got = torch.ops.ultrare.attack_scores(Xt, rows, fit.params[1], fit.stats[1], C.SETTINGS['hidden'])
    assert torch.equal(got, fit.scores[torch.from_numpy(held).cuda()])
    with pytest.raises(ValueError, match='params'):
        torch.ops.ultrare.attack_scores(Xt, rows, fit.params[1][:-1], fit.stats[1], C.SETTINGS['hidden'])


def _toy_cli(tmp_path, name, extra):
    """main.py on the toy set, 2 uniform shards, one epoch -> the sorted relative paths of every file it wrote."""
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


def test_main_attack_writes_its_file_beside_the_log_and_nothing_else_changes(tmp_path, capsys):
    attr = str(tmp_path / 'groups.npz')
    np.savez(attr, id1=np.arange(0, 1508, 2), id2=np.arange(1, 1508, 2))
    _, plain = _toy_cli(tmp_path, 'plain', [])
    capsys.readouterr()
    save, got = _toy_cli(tmp_path, 'attack', ['--attack', '--attack-hidden', '4', '--attack-folds', '3', '--attr-file', attr])
    assert 'attribute attacker (hidden 4, 3 folds): AUC' in capsys.readouterr().out
    added = sorted(set(got) - set(plain))
    assert not set(plain) - set(got) and len(added) == 2 and all(n.endswith('/attack0.npy') for n in added)          # learn and unlearn
    for n in added:
        assert os.path.exists(os.path.join(save, os.path.dirname(n), 'log0.npy'))
        res = np.load(os.path.join(save, n), allow_pickle=True).item()
        assert res['settings']['hidden'] == 4 and res['settings']['folds'] == 3 and 0.0 <= res['auc'] <= 1.0
    assert not any('attack' in n for n in plain)
    # a bad group file is refused before anything is trained or written
    bad = str(tmp_path / 'bad.npz')
    np.savez(bad, id1=np.arange(0, 10), id2=np.arange(5, 2000))
    with pytest.raises(ValueError, match='outside'):
        _toy_cli(tmp_path, 'bad', ['--attack', '--attr-file', bad])
    assert not os.path.exists(tmp_path / 'bad')
    with pytest.raises(ValueError, match='width'):
        _toy_cli(tmp_path, 'wide', ['--attack', '--attr-file', attr, '--k', '256'])
    assert not os.path.exists(tmp_path / 'wide')


def test_main_attack_without_attr_file_is_refused(tmp_path):
    from ultrare_amd import main
    with pytest.raises(ValueError, match='--attack needs --attr-file'):
        main.main(['--dataset', 'toy', '--attack', '--save-dir', str(tmp_path)])
    assert not os.listdir(tmp_path)
