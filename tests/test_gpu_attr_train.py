"""In-training attribute unlearning on the device (csrc/attr_train.hip, engine.GcnJob(attr=...)) against its numpy contract
(ultrare_amd/attr_train.py, ultrare_amd/attr_unlearn.py): the selection integer for integer, the device-counted losses inside the
derived bounds of mmd_ref / u2u_ref on dirty memory in guard zones, the hand-off bit for bit, whole training against the float64
restatement with two float32 CPU executions as the yardstick, and the bytes of a job without the term."""
import numpy as np
import pytest
import torch

import attr_train_cases as AC
from abi_arena import Arena, run_prefills, verdict
from ultrare_amd import attr_train, attr_unlearn, lightgcn

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _engine():
    from ultrare_amd import engine
    return engine


def _lib():
    from ultrare_amd import _native as nv
    return nv, nv.lib(), nv.stream_handle()


# ------------------------------------------------------------------ 1. selection
def _selection_case(n_user, steps):
    """Triples with a step tag each (by file position): users without entries, a user with one entry, a user with 300 entries (longer
    than a staged tile), group members at the ids 0 and n_user - 1; with two steps or more, group 1 is absent from the last step;
    with three or more, the step before it holds one triple."""
    rs = np.random.RandomState(1000 * n_user + steps)
    group = np.zeros(n_user, dtype=np.int8)
    group[0], group[-1] = 1, (2 if n_user > 1 else 1)
    for u in range(1, n_user - 1):
        group[u] = (0, 1, 2, 2, 1)[u % 5]
    long_user, one_user = 0, (n_user - 1 if n_user > 1 else None)
    empty = set(range(3, n_user - 1, 7))
    uid = [long_user] * 300 + ([one_user] if one_user is not None else [])
    for u in range(1, n_user - 1):
        if u not in empty:
            uid += [u] * int(rs.randint(1, 6))
    uid = np.array(uid, dtype=np.int64)
    rs.shuffle(uid)
    N = len(uid)
    iid = rs.randint(0, 50, size=N)
    tag = rs.randint(0, steps, size=N).astype(np.int32)
    tag[:steps] = np.arange(steps)                         # every step has a triple
    if steps >= 2:
        tag[(tag == steps - 1) & (group[uid] == 1)] = 0
    if steps >= 3:
        at = np.flatnonzero(tag == steps - 2)
        at = at[np.argsort(group[uid[at]] == 0, kind='stable')]        # (a group member's triple first, where there is one)
        tag[at[1:]] = 0
    return uid, iid, tag, group


@pytest.mark.parametrize('steps', (1, 3, 32, 33, 65))
@pytest.mark.parametrize('n_user', (1, 63, 64, 65, 257, 1000))
def test_selection_equals_the_contract_integer_for_integer(n_user, steps):
    E = _engine()
    uid, iid, file_tag, group = _selection_case(n_user, steps)
    graph = E.GcnGraph(uid, iid, np.ones(len(uid), np.float32), n_user, 50)
    id1, id2 = np.flatnonzero(group == 1), np.flatnonzero(group == 2)
    has = np.bincount(uid, minlength=n_user) > 0
    assert (~has).sum() >= (1 if n_user > 4 else 0) and np.bincount(uid).max() >= 300
    cap1, cap2 = max(1, int((has & (group == 1)).sum())), max(1, int((has & (group == 2)).sum()))
    tag = _dev(file_tag[graph.host.pos])
    gdev = _dev(group)
    masks = E.attr_step_masks(graph, tag, gdev, steps)
    want_masks = np.zeros((n_user, (steps + 31) // 32), dtype=np.uint32)
    for u, t in zip(uid, file_tag):
        if group[u]:
            want_masks[u, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    got = [E.attr_select(masks, gdev, steps, s, cap1, cap2) for s in range(steps)]
    torch.cuda.synchronize()
    assert masks.cpu().numpy().view(np.uint32).tolist() == want_masks.tolist()
    seen = []
    for s, (rows, counts) in enumerate(got):
        want, n1, n2 = attr_train.batch_groups_ref((uid, iid), file_tag == s, id1, id2)
        rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
        assert counts.tolist() == [n1, n2], (s, counts, n1, n2)
        assert rows[:n1 + n2].tolist() == want.tolist(), s
        assert (rows[n1 + n2:] == -1).all()
        seen.append((n1, n2))
    if steps >= 2 and n_user > 1:
        assert seen[-1][0] == 0                            # group 1 absent
    if steps >= 3:
        assert sum(seen[-2]) <= 1                          # at most one user selected
    assert max(a + b for a, b in seen) >= 1


def test_the_selection_entries_keep_the_memory_contract_on_dirty_memory():
    """ure_attr_step_masks and ure_attr_select in one arena: guard zones, the sizer's scratch, three prefills, the wrapper's bytes."""
    E = _engine()
    n_user, steps, step = 257, 33, 32
    uid, iid, file_tag, group = _selection_case(n_user, steps)
    g = lightgcn.Graph(uid, iid, n_user, 50)
    tag = np.ascontiguousarray(file_tag[g.pos].astype(np.int32))
    has = np.bincount(uid, minlength=n_user) > 0
    cap1, cap2 = int((has & (group == 1)).sum()), int((has & (group == 2)).sum())
    A = Arena('cuda:0')
    A.input('off', g.off_u)
    A.input('tag', tag)
    A.input('group', group)
    A.output('masks', n_user * 2 * 4)
    A.output('rows', (cap1 + cap2) * 4)
    A.output('counts', 8)
    A.scratch('ws', int(_lib()[1].ure_attr_select_scratch(n_user)))

    def call(A):
        nv, L, st = _lib()
        nv.check(L.ure_attr_step_masks(A.addr('off'), A.addr('tag'), A.addr('group'), n_user, g.N, steps, A.addr('masks'), st), 'masks')
        nv.check(L.ure_attr_select(A.addr('masks'), A.addr('group'), n_user, steps, step, cap1, cap2, A.addr('rows'), A.addr('counts'), A.addr('ws'),
                                   A.size('ws'), st), 'select')
    reports = run_prefills(A, call, sync=torch.cuda.synchronize)
    found = verdict(reports)
    assert not found, '\n  '.join(found)
    graph = E.GcnGraph(uid, iid, np.ones(len(uid), np.float32), n_user, 50)
    masks = E.attr_step_masks(graph, _dev(tag), _dev(group), steps)
    rows, counts = E.attr_select(masks, _dev(group), steps, step, cap1, cap2)
    torch.cuda.synchronize()
    out = reports[0].outputs
    assert out['masks'] == masks.cpu().numpy().tobytes() and out['rows'] == rows.cpu().numpy().tobytes() and out['counts'] == counts.cpu().numpy().tobytes()
    assert 0 < int(counts.sum()) < cap1 + cap2                     # a strict subset: the tail of -1 is there


def test_the_bandwidth_entry_keeps_the_memory_contract_and_takes_fix_sigma():
    (n1, n2), (cap1, cap2), d = (65, 63), (70, 70), 32
    X, ld, rows, counts = _loss_inputs(n1, n2, cap1, cap2, d)
    want = attr_unlearn.mmd_ref(X[:, :d], rows[:n1 + n2], n1)[2]
    for fix_sigma, bw in ((0.0, want), (2.5, 2.5)):
        A = Arena('cuda:0')
        A.input('X', X)
        A.input('rows', rows)
        A.input('counts', counts)
        A.output('bw', 8)
        A.output('valid', 4)
        A.scratch('ws', int(_lib()[1].ure_attr_scratch(cap1 + cap2, d)))

        def call(A):
            nv, L, st = _lib()
            nv.check(L.ure_attr_bandwidth(A.addr('X'), ld, d, A.addr('rows'), A.addr('counts'), cap1, cap2, fix_sigma, A.addr('bw'), A.addr('valid'),
                                          A.addr('ws'), A.size('ws'), st), 'bandwidth')
        reports = run_prefills(A, call, sync=torch.cuda.synchronize)
        assert not verdict(reports)
        got = np.frombuffer(reports[0].outputs['bw'], dtype=np.float64)[0]
        assert abs(got / bw - 1.0) <= 1e-12 and np.frombuffer(reports[0].outputs['valid'], dtype=np.int32)[0] == 1


# ------------------------------------------------------------------ 2. device-counted losses
# ((n1, n2), (cap1, cap2)); (64, 64) runs two column splits, (300, 250) two column-sum workgroups (d = 8 only)
COUNTS = (((1, 1), (1, 1)), ((1, 5), (3, 5)), ((64, 64), (64, 64)), ((65, 63), (70, 70)), ((3, 4), (120, 80)))
WIDTHS = (1, 8, 32, 100, 128)
LOSS_CASES = [(c, d) for c in COUNTS for d in WIDTHS] + [(((300, 250), (300, 300)), 8)]


def _loss_inputs(n1, n2, cap1, cap2, d, equal=False):
    """X [n_rows, ld] float32 with ld > d, rows [cap] (the entries behind m name row 0) and counts."""
    rs = np.random.RandomState(7 * n1 + 13 * n2 + d)
    n_rows, ld = cap1 + cap2 + 9, d + 3
    X = rs.randn(n_rows, ld).astype(np.float32)
    X[:, d:] = 1e30                                        # the padding columns are never read
    if equal:
        X[:, :d] = X[0, :d]
    rows = np.zeros(cap1 + cap2, dtype=np.int32)
    rows[:n1 + n2] = rs.permutation(n_rows)[:n1 + n2]
    rows[:n1].sort()
    rows[n1:n1 + n2].sort()
    return X, ld, rows, np.array([n1, n2], dtype=np.int32)


def _arena(var, X, ld, rows, counts, cap1, cap2, d):
    nv, L, _ = _lib()
    A = Arena('cuda:0')
    A.input('X', X)
    A.input('rows', rows)
    A.input('counts', counts)
    A.output('out', 32 if var == 'd2d' else 8)
    A.output('grad', (cap1 + cap2) * d * 4)
    A.output('valid', 4)
    if var == 'd2d':
        A.output('bw', 8)
    nbytes = int(L.ure_attr_scratch(cap1 + cap2, d))
    assert nbytes == int(L.ure_mmd_scratch(cap1 + cap2, d)) > 0
    A.scratch('ws', nbytes)

    def call(A):
        nv, L, st = _lib()
        front = (A.addr('X'), ld, d, A.addr('rows'), A.addr('counts'), cap1, cap2)
        if var == 'd2d':
            rc = L.ure_attr_mmd_loss_grad(*front, 2.0, 5, 0.0, A.addr('bw'), A.addr('out'), A.addr('grad'), A.addr('valid'), None, None, A.addr('ws'),
                                          A.size('ws'), st)
        else:
            rc = L.ure_attr_u2u_loss_grad(*front, A.addr('out'), A.addr('grad'), A.addr('valid'), None, None, A.addr('ws'), A.size('ws'), st)
        nv.check(rc, var)
    return A, call


def _wrapper(var, X, ld, d, rows, counts, cap1, cap2, acc=None, skipped=None, stream=None):
    """The same call through the engine's wrapper (torch.empty memory) -> the outputs' bytes by the arena's names."""
    E = _engine()
    Xd = _dev(X)[:, :d]
    if var == 'd2d':
        sums, grad, valid, bw = E.mmd_loss_grad_dev(Xd, _dev(rows), _dev(counts), cap1, cap2, acc=acc, skipped=skipped, stream=stream)
        out = dict(out=sums, grad=grad, valid=valid, bw=bw)
    else:
        value, grad, valid = E.u2u_loss_grad_dev(Xd, _dev(rows), _dev(counts), cap1, cap2, acc=acc, skipped=skipped, stream=stream)
        out = dict(out=value, grad=grad, valid=valid)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in out.items()}


@pytest.mark.parametrize('var', ('d2d', 'u2u'))
@pytest.mark.parametrize('case', LOSS_CASES, ids=lambda c: f'{c[0][0][0]}x{c[0][0][1]}-cap{c[0][1][0]}x{c[0][1][1]}-d{c[1]}')
def test_device_counted_losses_stay_inside_the_derived_bounds_on_dirty_memory(case, var):
    ((n1, n2), (cap1, cap2)), d = case
    m = n1 + n2
    X, ld, rows, counts = _loss_inputs(n1, n2, cap1, cap2, d)
    A, call = _arena(var, X, ld, rows, counts, cap1, cap2, d)
    reports = run_prefills(A, call, sync=torch.cuda.synchronize)
    found = verdict(reports)
    assert not found, '\n  '.join(found)
    out = reports[0].outputs
    grad = np.frombuffer(out['grad'], dtype=np.float32).reshape(cap1 + cap2, d)
    assert np.frombuffer(out['valid'], dtype=np.int32)[0] == 1
    assert not np.frombuffer(out['grad'], dtype=np.uint8).reshape(cap1 + cap2, d * 4)[m:].any()          # +0.0, every byte
    if var == 'd2d':
        loss, g, bw, b_loss, b_grad = attr_unlearn.mmd_ref(X[:, :d], rows[:m], n1)
        s = np.frombuffer(out['out'], dtype=np.float64)
        got = s[0] / (n1 * n1) + s[1] / (n2 * n2) - s[2] / (n1 * n2) - s[3] / (n1 * n2)
        got_bw = np.frombuffer(out['bw'], dtype=np.float64)[0]
        print(f'loss err {abs(got - loss):.3g} bound {b_loss:.3g}; grad err/bound {np.max(np.abs(grad[:m] - g) / b_grad):.3g}; bw rel {abs(got_bw / bw - 1):.3g}')
        # the closed form adds float64 sums of float32 data shifted by the first row: (m + d + 8) 2^-53 of the magnitudes added,
        # 2 m sum |t|^2 + 2 |sum t|^2 <= 4 m sum |t|^2, over m^2 - m
        t = X[rows[:m].astype(np.int64), :d].astype(np.float64) - X[rows[0], :d].astype(np.float64)
        assert abs(got_bw - bw) <= (m + d + 8) * attr_unlearn.U64 * 4 * m * (t * t).sum() / (m * m - m)
        assert abs(got - loss) <= b_loss
    else:
        value, g, b_value, b_grad = attr_unlearn.u2u_ref(X[:, :d], rows[:m], n1)
        got = np.frombuffer(out['out'], dtype=np.float64)[0]
        print(f'value err {abs(got - value):.3g} bound {b_value:.3g}; grad err/bound {np.max(np.abs(grad[:m] - g) / b_grad):.3g}')
        assert abs(got - value) <= b_value
    assert (np.abs(grad[:m] - g) <= b_grad).all()
    # the wrapper's call, a repeat of it and one on a side stream give the arena's bytes
    first = _wrapper(var, X, ld, d, rows, counts, cap1, cap2)
    assert first == out
    assert _wrapper(var, X, ld, d, rows, counts, cap1, cap2) == out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert _wrapper(var, X, ld, d, rows, counts, cap1, cap2, stream=side) == out


@pytest.mark.parametrize('var', ('d2d', 'u2u'))
def test_the_accumulator_takes_the_loss_of_a_valid_step(var):
    (n1, n2), (cap1, cap2), d = (3, 4), (120, 80), 8
    X, ld, rows, counts = _loss_inputs(n1, n2, cap1, cap2, d)
    acc, skipped = torch.full((1,), 2.5, dtype=torch.float64, device='cuda'), torch.full((1,), 7, dtype=torch.int32, device='cuda')
    _wrapper(var, X, ld, d, rows, counts, cap1, cap2, acc=acc, skipped=skipped)
    want = attr_unlearn.mmd_ref(X[:, :d], rows[:7], n1)[0] if var == 'd2d' else attr_unlearn.u2u_ref(X[:, :d], rows[:7], n1)[0]
    assert abs(float(acc) - 2.5 - want) <= 1e-6 * abs(want) + 1e-6 and int(skipped) == 7


@pytest.mark.parametrize('var', ('d2d', 'u2u'))
@pytest.mark.parametrize('what', ('empty-group', 'all-equal'))
def test_a_step_without_a_group_or_a_bandwidth_is_skipped_without_nan(var, what):
    d, (cap1, cap2) = 8, (6, 6)
    n1, n2 = (0, 5) if what == 'empty-group' else (3, 3)
    X, ld, rows, counts = _loss_inputs(n1, n2, cap1, cap2, d, equal=what == 'all-equal')
    A, call = _arena(var, X, ld, rows, counts, cap1, cap2, d)
    reports = run_prefills(A, call, sync=torch.cuda.synchronize)
    assert not verdict(reports)
    out = reports[0].outputs
    acc, skipped = torch.full((1,), 2.5, dtype=torch.float64, device='cuda'), torch.full((1,), 7, dtype=torch.int32, device='cuda')
    assert _wrapper(var, X, ld, d, rows, counts, cap1, cap2, acc=acc, skipped=skipped) == out
    valid = np.frombuffer(out['valid'], dtype=np.int32)[0]
    if var == 'u2u' and what == 'all-equal':               # the Laplacian term has no bandwidth: valid, value 0
        assert attr_train.step_valid(n1, n2, var) and valid == 1 and int(skipped) == 7
        assert np.frombuffer(out['out'], dtype=np.float64)[0] == 0.0 and float(acc) == 2.5
    else:
        assert not attr_train.step_valid(n1, n2, var, 0.0) and valid == 0
        assert float(acc) == 2.5 and int(skipped) == 8                                                    # unchanged accumulator
        assert not np.frombuffer(out['out'], dtype=np.uint8).any()
    for name in out:
        if name != 'valid':
            assert np.isfinite(np.frombuffer(out[name], dtype=np.float32 if name == 'grad' else np.float64)).all(), name
    assert not np.frombuffer(out['grad'], dtype=np.uint8).any()


def test_refusals_before_any_device_work():
    E = _engine()
    nv, L, _ = _lib()
    assert L.ure_attr_scratch(1, 8) == -1 and L.ure_attr_scratch(10, 129) == -1 and L.ure_attr_scratch(10, 0) == -1
    assert L.ure_attr_scratch(10 ** 5, 128) < 17 * 10 ** 5 * 128 * 8 + 2 ** 20                            # never quadratic
    assert L.ure_attr_select_scratch(0) == -1
    X, ld, rows, counts = _loss_inputs(2, 2, 2, 2, 8)
    with pytest.raises(nv.NativeError):
        E.mmd_loss_grad_dev(torch.from_numpy(X), _dev(rows), _dev(counts), 2, 2)
    with pytest.raises(ValueError):
        E.mmd_loss_grad_dev(_dev(X)[:, :8], _dev(rows), _dev(counts), 0, 4)
    with pytest.raises(ValueError):
        E.u2u_loss_grad_dev(_dev(X)[:, :8], _dev(rows)[:3], _dev(counts), 2, 2)
    with pytest.raises(ValueError):
        E.attr_add_grad(_dev(X), _dev(rows), _dev(counts), _dev(np.ones(1, np.int32)), _dev(np.zeros((4, 8), np.float32)), float('nan'))


# ------------------------------------------------------------------ 3. the hand-off
@pytest.mark.parametrize('valid', (1, 0))
def test_the_hand_off_is_the_numpy_formula_bit_for_bit_and_touches_nothing_else(valid):
    E = _engine()
    rs = np.random.RandomState(5)
    n_rows, ld, d, cap, n1, n2 = 50, 16, 11, 20, 4, 9
    G = rs.randn(n_rows, ld).astype(np.float32)
    rows = np.full(cap, -1, dtype=np.int32)
    rows[:n1 + n2] = rs.permutation(n_rows)[:n1 + n2]
    sel = rows[:n1 + n2].astype(np.int64)
    poison = np.ones((n_rows, ld), dtype=bool)
    poison[sel, :d] = False
    G.view(np.uint32)[poison] = 0xFFC0DEAD                 # NaN patterns in every float the call must not touch
    grad = rs.randn(cap, d).astype(np.float32)
    eta = np.float32(0.37)
    want = G.copy()
    if valid:
        want[sel, :d] = G[sel, :d] + eta * grad[:n1 + n2]
    Gd = _dev(G)
    E.attr_add_grad(Gd, _dev(rows), _dev(np.array([n1, n2], np.int32)), _dev(np.array([valid], np.int32)), _dev(grad), float(eta))
    torch.cuda.synchronize()
    assert Gd.cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------ 4. whole training
def _run(job, case):
    job.run()
    U, V = job.tables(0)
    P, Q = job.base_tables()
    dis, base = job.epoch_dis(), job.epoch_loss(0)
    loss = np.sqrt((base + case.eta * dis) / job.graph.N) if case.loss == 'mse' else (base + case.eta * dis) / job.graph.N
    return dict(U=[U.cpu().numpy()], V=[V.cpu().numpy()], P=[P.cpu().numpy()], Q=[Q.cpu().numpy()], loss=loss, dis=dis, skipped=job.epoch_skipped())


def _job_bytes(job):
    return [t.cpu().numpy().tobytes() for t in (*job.padded_tables(0), *job.base_tables(padded=True), job._t['M'])] + [job.epoch_loss(0).tobytes()]


@pytest.mark.parametrize('case', AC.GPU_CASES, ids=repr)
def test_whole_training_with_the_term_is_as_close_to_float64_as_the_float32_executions(case):
    """E_k = distance of the job from attr_train.train_ref(float64) (lightgcn_cases.distance: both final and both parameter tables,
    the epoch losses); E_y = the larger such distance of two float32 CPU executions, train_ref(float32) and torch float32 autograd
    of the literal loss.  E_k <= 4 max(E_y, ulp32(max |w|)), the rule of tests/test_gpu_lightgcn.py."""
    ref = AC.reference(case)
    f64 = ref['f64']
    assert f64['counts'].min() >= 1 and not f64['skipped'].any()                                          # no test passes by skipping
    job = case.job()
    run = _run(job, case)
    want = _job_bytes(job)
    job.close()
    E_k = AC.distance(f64, run)
    print(f'{case!r}: E_k {E_k:.3g} E_y {ref["E_y"]:.3g} bound {ref["bound"]:.3g} dis {run["dis"]} ref {f64["dis"]}')
    assert ref['E_y'] > 0
    assert E_k <= ref['bound'], (E_k, ref['E_y'], ref['bound'])
    assert np.abs(run['dis'] / f64['dis'] - 1.0).max() <= 1e-5
    assert run['skipped'].tolist() == f64['skipped'].tolist()
    again = case.job()
    again.run()
    assert _job_bytes(again) + [again.epoch_dis().tobytes()] == want + [run['dis'].tobytes()]
    again.close()


def test_skipped_steps_are_counted_and_leave_the_step_plain():
    """Every user of group 2 sits in ONE batch of the first epoch's order only: the other steps of that epoch are skipped."""
    case = AC.Case(40, 24, 8, 600, 128, 1, 1, seed=91, var='d2d', no_i=2)
    case.id2 = np.array([9, 11])
    rest = np.flatnonzero(~np.isin(case.uid, case.id2))
    mine = np.flatnonzero(np.isin(case.uid, case.id2))
    assert 0 < len(mine) <= case.B
    case.orders = np.concatenate([mine, rest])[None, :].astype(case.orders.dtype)
    both = AC.reference(case)
    ref = both['f64']
    assert ref['skipped'].tolist() == [case.steps - 1] and ref['counts'][0, 0].min() >= 1
    job = case.job()
    run = _run(job, case)
    job.close()
    assert run['skipped'].tolist() == [case.steps - 1]
    assert abs(run['dis'][0] / ref['dis'][0] - 1.0) <= 1e-5
    assert AC.distance(ref, run) <= both['bound']


# ------------------------------------------------------------------ 5. existing behaviour
@pytest.mark.parametrize('loss', ('mse', 'bpr'))
def test_a_job_without_the_term_gives_the_bytes_of_a_job_built_without_the_arguments(loss):
    case = AC.GPU_CASES[3 if loss == 'bpr' else 2]
    E = _engine()
    graph = case.graph()
    args = (graph, (case.U0, case.V0), case.orders, case.d, case.layers, case.B, case.epochs, AC.C.LR, case.lam, case.mu, case.lr_decay, case.lr_step)
    plain = E.GcnJob(*args, loss=loss, key=case.key)
    plain.run()
    want = _job_bytes(plain)
    plain.close()
    nor = E.GcnJob(*args, loss=loss, key=case.key, attr=None, dis_type='nor', eta=3.0, fix_sigma=2.0)
    nor.run()
    assert _job_bytes(nor) == want
    with pytest.raises(ValueError):
        nor.epoch_dis()
    nor.close()
    with pytest.raises(ValueError, match='k = 256'):
        E.GcnJob(graph, (np.zeros((case.n_user, 256), np.float32), np.zeros((case.n_item, 256), np.float32)), case.orders, 256, 0, case.B, case.epochs,
                 1e-3, 0.1, 0.9, attr=(case.id1, case.id2), dis_type='d2d')
    with pytest.raises(ValueError):
        E.GcnJob(*args, attr=(case.id1, case.id2), dis_type='nor')
    with pytest.raises(ValueError):
        E.GcnJob(*args, attr=(case.id1[:0], case.id2), dis_type='u2u')
