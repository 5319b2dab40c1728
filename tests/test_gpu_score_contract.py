"""The scoring path of csrc/mf_eval.hip against its contract, bit for bit, at every row width (run with -m gpu on an MI355X).

ure_score is what the recommend, rank and combiner tests take as their expected value; here it is compared with the CPU
restatement of DESIGN.md's "The ure_score contract" (oracle/mf_oracle.c: ure_oracle_score_contract, ure_oracle_score_sse), the
three series routes with single evaluations, and the reductions, the row merge and the per-user ranking with numpy.  Every
comparison is an equality: no tolerance appears in this file.  Straight through the C ABI, no training: tables of 97 users x 61
items of mixed signs and magnitudes (tests/test_cpu_score_contract.py shows that on such tables the contract differs from the
near-miss orders), pairs drawn with repetition."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

N_USER, N_ITEM = 97, 61
WIDTHS = (4, 8, 16, 32, 64, 128, 256)
CHUNK = 32                                     # URE_MAX_MODELS_PER_CALL


def tables(seed, d, S):
    """As in tests/test_cpu_score_contract.py: a normal value times a log-normal scale."""
    rs = np.random.RandomState(seed)
    mk = lambda n: (rs.standard_normal((n, d)) * np.exp(1.5 * rs.standard_normal((n, d)))).astype(np.float32)
    return [(mk(N_USER), mk(N_ITEM)) for _ in range(S)]


def pairs(seed, n):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, N_USER, n).astype(np.int32), rs.randint(0, N_ITEM, n).astype(np.int32),
            rs.choice([0.2, 0.4, 0.6, 0.8, 1.0], n).astype(np.float32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def native():
    from ultrare_amd import _native as nv
    return nv, nv.lib(), nv.stream_handle()


def gpu_score(models, n_total, uid, iid, rating, n, d, pred, sse, first=True, last=True):
    """ure_score over a model list of any length: chunks of 32 with first / last, as every caller does."""
    nv, L, st = native()
    for c0 in range(0, len(models), CHUNK):
        chunk = models[c0:c0 + CHUNK]
        end = c0 + CHUNK >= len(models)
        nv.check(L.ure_score(ptrs([m[0] for m in chunk]), ptrs([m[1] for m in chunk]), len(chunk), n_total, int(first and c0 == 0), int(last and end),
                             nv.ptr(uid), nv.ptr(iid), nv.ptr(rating), n, d, nv.ptr(pred), nv.ptr(sse) if end else None, st), 'ure_score')


@pytest.mark.parametrize('d', WIDTHS)
def test_score_equals_the_contract_at_every_width_count_and_model_count(d):
    """pred and all 2048 sse doubles of ure_score against the contract for n = 1, G - 1, G, G + 1, 4G - 1, 4G + 1 (one wavefront,
    one workgroup, their edges), 8192 G - 1, 8192 G, 8192 G + 1 (the cap of 2048 workgroups: the first pair of the grid stride) and
    2 * 8192 G + G + 3 (two to three strides, ragged), crossed with S = 1, 3, 4, 5 (the unroll by four and its tail), 32, 33, 35 (the
    callers' chunks with first / last).  The running sum after m models does not depend on S, so the oracle adds the 35 models once."""
    G = 64 // (d // 4)
    sizes = sorted({1, max(G - 1, 1), G, G + 1, 4 * G - 1, 4 * G + 1, 8192 * G - 1, 8192 * G, 8192 * G + 1, 2 * 8192 * G + G + 3})
    counts = (1, 3, 4, 5, 32, 33, 35)
    host = tables(300 + d, d, 35)
    uid, iid, r = pairs(d, sizes[-1])
    want, run = {}, None
    for m in range(35):
        if m + 1 in counts:
            want[m + 1] = O.score_contract(host[m:m + 1], uid, iid, n_total=m + 1, first=m == 0, last=True, running=run)
        run = O.score_contract(host[m:m + 1], uid, iid, first=m == 0, last=False, running=run)
    models = [(dev(U), dev(V)) for U, V in host]
    d_uid, d_iid, d_r = dev(uid), dev(iid), dev(r)
    pred = torch.empty(sizes[-1], dtype=torch.float32, device='cuda')
    sse = torch.empty(O.SCORE_PARTIALS, dtype=torch.float64, device='cuda')
    for n in sizes:
        for S in counts:
            pred.fill_(-7.0)
            sse.fill_(-7.0)
            gpu_score(models[:S], S, d_uid, d_iid, d_r, n, d, pred, sse)
            got, got_sse = pred.cpu().numpy(), sse.cpu().numpy()
            assert np.array_equal(got[:n], want[S][:n]), (n, S)
            assert (got[n:] == -7.0).all(), (n, S)                                          # nothing written past n
            assert np.array_equal(got_sse, O.score_sse_partials(want[S][:n], r[:n], d)), (n, S)
    # n_models_total > n_models; sse = NULL; rating = NULL with sse = NULL; last = 0 (the running sum, sse left alone)
    n = 4 * G + 1
    for kw, total, last in (({}, 7, True), ({'sse': None}, 5, True), ({'sse': None, 'rating': None}, 5, True), ({}, 5, False)):
        pred.fill_(-7.0)
        sse.fill_(-7.0)
        nv, L, st = native()
        nv.check(L.ure_score(ptrs([m[0] for m in models[:5]]), ptrs([m[1] for m in models[:5]]), 5, total, 1, int(last), nv.ptr(d_uid), nv.ptr(d_iid),
                             nv.ptr(kw.get('rating', d_r)), n, d, nv.ptr(pred), nv.ptr(kw.get('sse', sse)), st), 'ure_score')
        ref = O.score_contract(host[:5], uid[:n], iid[:n], n_total=total, last=last)
        assert np.array_equal(pred.cpu().numpy()[:n], ref), (kw, total, last)
        if last and 'sse' not in kw:
            assert np.array_equal(sse.cpu().numpy(), O.score_sse_partials(ref, r[:n], d))
        else:
            assert (sse == -7.0).all()


def single_evaluations(ev, fixed, members, n, d):
    """-> (out [E, 3], pred [E, n], sse [E, 2048]) of ure_score + ure_eval_users + ure_eval_reduce, one member at a time."""
    nv, L, st = native()
    E = len(members)
    out = torch.zeros(E, 3, dtype=torch.float64, device='cuda')
    pred = torch.zeros(E, n, dtype=torch.float32, device='cuda')
    sse = torch.zeros(E, O.SCORE_PARTIALS, dtype=torch.float64, device='cuda')
    for e, model in enumerate(members):
        gpu_score(fixed + [model], len(fixed) + 1, ev.uid, ev.iid, ev.rating, n, d, pred[e], sse[e])
        nv.check(L.ure_eval_users(nv.ptr(ev.off), ev.n_users, nv.ptr(pred[e]), nv.ptr(ev.rating), nv.ptr(ev.log2), nv.ptr(ev.hits), nv.ptr(ev.ndcg),
                                  nv.ptr(ev.top_rating), ev.n_wide, ev.n_half, st), 'ure_eval_users')
        nv.check(L.ure_eval_reduce(nv.ptr(ev.hits), nv.ptr(ev.ndcg), ev.n_users, nv.ptr(sse[e]), n, nv.ptr(out[e]), st), 'ure_eval_reduce')
    return out, pred, sse


@pytest.mark.parametrize('d', WIDTHS)
def test_series_routes_equal_single_evaluations_at_every_width(d):
    """ure_eval_series, ure_eval_series_compact and ure_score_own_compact + ure_eval_series_own (in place and out of place) against
    ure_score + ure_eval_users + ure_eval_reduce per member on the same full tables: out, pred and sse to the last bit.  n below 4 G,
    and on both sides of 8192 G (above it series_combine_kernel restates score_kernel's grid stride thread by thread); n_series
    1, 3, 4, 5, 9 (the four epochs in flight and the clamp to the last member; 3 and 5 at d = 4, which keeps the scratch under
    50 MB); 0, 2 and 33 fixed models, given as tables or as a base made by ure_sum_vectors.  The compact snapshot's full tables are
    built on the host as the snapshot stores them: a row without a slot is float32(snap_a[e]) * w0, elementwise; the slots make
    every combination of a stored / unstored user and item occur, and user 0 has slot 0."""
    from ultrare_amd import engine
    nv, L, st = native()
    G = 64 // (d // 4)
    E_max = 5 if d == 4 else 9
    series = (3, 5) if d == 4 else (1, 3, 4, 5, 9)
    rs = np.random.RandomState(400 + d)
    fixed_host = tables(500 + d, d, 33)
    fixed_all = [(dev(U), dev(V)) for U, V in fixed_host]
    (U0, V0), = tables(600 + d, d, 1)
    # compact snapshots: half of the rows stored, in a shuffled slot order that gives user 0 slot 0
    n_rows = N_USER + N_ITEM
    stored = rs.rand(n_rows) < 0.5
    stored[0] = True
    ids = np.flatnonzero(stored)
    ids = np.concatenate([[0], rs.permutation(ids[1:])])
    row_slot = np.full(n_rows, -1, np.int32)
    row_slot[ids] = np.arange(len(ids), dtype=np.int32)
    assert row_slot[0] == 0 and (row_slot[:N_USER] < 0).any() and (row_slot[N_USER:] < 0).any() and (row_slot[N_USER:] >= 0).any()
    snap = (rs.standard_normal((E_max, len(ids), d)) * np.exp(1.5 * rs.standard_normal((E_max, len(ids), d)))).astype(np.float32)
    snap_a = (0.5 + rs.rand(E_max)).astype(np.float32)
    W0 = np.concatenate([U0, V0])
    full = np.empty((E_max, n_rows, d), np.float32)
    for e in range(E_max):
        full[e] = np.float32(snap_a[e]) * W0
        full[e][ids] = snap[e]
    U_ser, V_ser = dev(full[:, :N_USER]), dev(full[:, N_USER:])
    members = [(U_ser[e], V_ser[e]) for e in range(E_max)]
    d_snap, d_slot, d_U0, d_V0, d_a = dev(snap), dev(row_slot), dev(U0), dev(V0), dev(snap_a)
    for n in (4 * G - 1, 8192 * G - 1, 8192 * G + 4 * G + 3):
        uid, iid, r = pairs(700 + d, n)
        if n > 100:
            su, si = row_slot[uid] >= 0, row_slot[N_USER + iid] >= 0
            assert all(((su == a) & (si == b)).any() for a in (False, True) for b in (False, True))
        ev = engine.EvalSet(uid, iid, r)
        new = lambda *shape, dt=torch.float32: torch.full(shape, -7, dtype=dt, device='cuda')
        for n_fixed in (0, 2, 33):
            fixed = fixed_all[:n_fixed]
            want = single_evaluations(ev, fixed, members, n, d)
            # the fixed models as a cached base: every model scored alone (first = 1, last = 0), the vectors added in list order
            base_made = None
            if n_fixed:
                vec = torch.empty(n_fixed, n, dtype=torch.float32, device='cuda')
                for m, model in enumerate(fixed):
                    gpu_score([model], 1, ev.uid, ev.iid, ev.rating, n, d, vec[m], None, last=False)
                base_made = new(n)
                nv.check(L.ure_sum_vectors(ptrs(list(vec)), n_fixed, n, nv.ptr(base_made), st), 'ure_sum_vectors')
            for as_base in ((False,) if n_fixed == 0 else (False, True)):
                Uf = None if as_base or not n_fixed else ptrs([m[0] for m in fixed])
                Vf = None if as_base or not n_fixed else ptrs([m[1] for m in fixed])
                for E in series:
                    for route in ('series', 'compact', 'own', 'own_in_place'):
                        base = base_made.clone() if as_base else new(n)
                        pred, sse, out = new(E, n), new(E, O.SCORE_PARTIALS, dt=torch.float64), new(E, 3, dt=torch.float64)
                        hits, ndcg = new(E, ev.n_users, dt=torch.int32), new(E, ev.n_users, dt=torch.float64)
                        tail = (nv.ptr(ev.off), ev.n_users, nv.ptr(ev.log2), nv.ptr(base), nv.ptr(pred), nv.ptr(sse), nv.ptr(hits), nv.ptr(ndcg), nv.ptr(out),
                                nv.ptr(ev.top_rating), ev.n_wide, ev.n_half, st)
                        test = (nv.ptr(ev.uid), nv.ptr(ev.iid), nv.ptr(ev.rating), n, d)
                        compact = (nv.ptr(d_snap), len(ids) * d, nv.ptr(d_slot), nv.ptr(d_U0), nv.ptr(d_V0), nv.ptr(d_a), N_USER, E)
                        if route == 'series':
                            nv.check(L.ure_eval_series(Uf, Vf, n_fixed, nv.ptr(U_ser), nv.ptr(V_ser), N_USER * d, N_ITEM * d, E, *test, *tail), route)
                        elif route == 'compact':
                            nv.check(L.ure_eval_series_compact(Uf, Vf, n_fixed, *compact, *test, *tail), route)
                        else:
                            own = pred if route == 'own_in_place' else new(E, n)
                            nv.check(L.ure_score_own_compact(*compact, nv.ptr(ev.uid), nv.ptr(ev.iid), n, d, nv.ptr(own), st), 'ure_score_own_compact')
                            nv.check(L.ure_eval_series_own(Uf, Vf, n_fixed, nv.ptr(own), E, *test, *tail), route)
                        what = (n, n_fixed, as_base, E, route)
                        assert torch.equal(pred, want[1][:E]), what
                        assert torch.equal(sse, want[2][:E]), what
                        assert torch.equal(out, want[0][:E]), what
        # and the single evaluations themselves are the contract's (the last n_fixed of the loop: 33 models + the member)
        for e in (0, E_max - 1):
            ref = O.score_contract(fixed_host + [(full[e, :N_USER], full[e, N_USER:])], uid[ev.order], iid[ev.order])
            assert np.array_equal(want[1][e].cpu().numpy(), ref), (n, e)
            assert np.array_equal(want[2][e].cpu().numpy(), O.score_sse_partials(ref, r[ev.order], d)), (n, e)


def test_sum_vectors_is_the_sequential_float32_sum():
    """ure_sum_vectors for 1, 32, 33 and 70 vectors (chunks of 32: the `first` flag) and n = 1, 255, 257 and 8192 * 256 + 5 (the
    grid's cap: the stride loop) against the vectors added one after another in float32.  (Seven buffers, listed in turn.)"""
    nv, L, st = native()
    rs = np.random.RandomState(8)
    n_max = 8192 * 256 + 5
    host = [(rs.standard_normal(n_max) * np.exp(1.5 * rs.standard_normal(n_max))).astype(np.float32) for _ in range(7)]
    bufs = [dev(v) for v in host]
    out = torch.empty(n_max, dtype=torch.float32, device='cuda')
    for count in (1, 32, 33, 70):
        order = [(3 * k) % 7 for k in range(count)]
        want = O.sum_vectors([host[k] for k in order])
        for n in (1, 255, 257, n_max):
            out.fill_(-7.0)
            nv.check(L.ure_sum_vectors(ptrs([bufs[k] for k in order]), count, n, nv.ptr(out), st), 'ure_sum_vectors')
            got = out.cpu().numpy()
            assert np.array_equal(got[:n], want[:n]) and (got[n:] == -7.0).all(), (count, n)


def test_reduce_and_subset_orders():
    """ure_eval_reduce and ure_eval_subset against tree_1024 (oracle/cpu_ref.py): 1024 strided accumulators, then the tree
    o = 512 ... 1, in float64 and int64, for n_users / n_sub = 0, 1, 63, 1023, 1024, 1025, 5000 and n_pairs = 0, 1, 1024 * 24 -+ 1,
    60001 (one round of 24 pairs per thread and the next), on values of mixed magnitude: the three numbers with np.array_equal."""
    nv, L, st = native()
    rs = np.random.RandomState(9)
    mixed = lambda n: rs.standard_normal(n) * np.exp(3 * rs.standard_normal(n))
    sizes = (0, 1, 63, 1023, 1024, 1025, 5000)
    out = torch.empty(2, 3, dtype=torch.float64, device='cuda')
    for n_users in sizes:
        hits, ndcg = rs.randint(0, 11, max(n_users, 1)).astype(np.int32), np.abs(mixed(max(n_users, 1)))
        sse = np.abs(mixed(O.SCORE_PARTIALS))
        out.fill_(-7.0)
        d_hits, d_ndcg, d_sse = dev(hits), dev(ndcg), dev(sse)
        nv.check(L.ure_eval_reduce(nv.ptr(d_hits), nv.ptr(d_ndcg), n_users, nv.ptr(d_sse), 60001, nv.ptr(out), st), 'ure_eval_reduce')
        assert np.array_equal(out[0].cpu().numpy(), O.eval_reduce(hits[:n_users], ndcg[:n_users], sse, 60001)), n_users
    n_all, n_total = 5000, 70000
    hits, ndcg = rs.randint(0, 11, (2, n_all)).astype(np.int32), np.abs(mixed(2 * n_all)).reshape(2, n_all)
    pred, r = mixed(2 * n_total).astype(np.float32).reshape(2, n_total), rs.choice([0.2, 0.4, 0.6, 0.8, 1.0], n_total).astype(np.float32)
    d_hits, d_ndcg, d_pred, d_r = dev(hits), dev(ndcg), dev(pred), dev(r)
    for n_sub in sizes:
        for n_pairs in (0, 1, 1024 * 24 - 1, 1024 * 24 + 1, 60001):
            users = rs.permutation(n_all)[:n_sub].astype(np.int32)
            sel = rs.permutation(n_total)[:n_pairs].astype(np.int32)
            out.fill_(-7.0)
            d_users, d_sel = dev(np.append(users, 0).astype(np.int32)), dev(np.append(sel, 0).astype(np.int32))
            nv.check(L.ure_eval_subset(nv.ptr(d_users), n_sub, nv.ptr(d_sel), n_pairs,
                                       nv.ptr(d_pred), nv.ptr(d_r), nv.ptr(d_hits), nv.ptr(d_ndcg), n_total, n_all, 2, nv.ptr(out), st), 'ure_eval_subset')
            got = out.cpu().numpy()
            for m in range(2):
                assert np.array_equal(got[m], O.eval_subset(users, sel, pred[m], r, hits[m], ndcg[m])), (n_sub, n_pairs, m)


@pytest.mark.parametrize('d', (1, 3, 4, 6, 16))
def test_merge_rows_copies_the_listed_rows_and_nothing_else(d):
    """ure_merge_rows with dst / src 16-byte aligned (the float4 path when d % 4 == 0) and each offset by one float (the scalar
    path), duplicate row indices and n_rows = 0: the listed rows are src's, every other row keeps its bits."""
    nv, L, st = native()
    rs = np.random.RandomState(d)
    n_rows = 301
    for off_dst, off_src in ((0, 0), (1, 0), (0, 1)):
        a = rs.standard_normal(n_rows * d + 1).astype(np.float32)
        b = rs.standard_normal(n_rows * d + 1).astype(np.float32)
        for rows in (np.zeros(0, np.int64), rs.randint(0, n_rows, 500).astype(np.int64), np.array([n_rows - 1, 0, 0, n_rows - 1], np.int64)):
            buf_dst, buf_src = dev(a), dev(b)
            dst, src = buf_dst[off_dst:off_dst + n_rows * d], buf_src[off_src:off_src + n_rows * d]
            assert dst.data_ptr() % 16 == 4 * off_dst and src.data_ptr() % 16 == 4 * off_src
            d_rows = dev(np.append(rows, 0))
            nv.check(L.ure_merge_rows(dst.data_ptr(), src.data_ptr(), nv.ptr(d_rows), len(rows), d, st), 'ure_merge_rows')
            want = a.copy()
            w, s = want[off_dst:off_dst + n_rows * d].reshape(n_rows, d), b[off_src:off_src + n_rows * d].reshape(n_rows, d)
            w[rows] = s[rows]
            assert np.array_equal(buf_dst.cpu().numpy().view(np.int32), want.view(np.int32)), (off_dst, off_src, len(rows))
            assert np.array_equal(buf_src.cpu().numpy().view(np.int32), b.view(np.int32))


LENGTHS = list(range(1, 17)) + [17, 32, 33, 64, 65, 128, 129, 512, 513, 700]
FLT_MAX = np.finfo(np.float32).max


def segment_class(cnt):
    """Which code ranks a segment: a quarter wave, a half wave, a lane per entry, several entries per lane, from memory."""
    return 0 if cnt <= 16 else 1 if cnt <= 32 else 2 if cnt <= 64 else 3 if cnt <= 512 else 4


def ranking_set():
    rs = np.random.RandomState(12)
    lengths = LENGTHS * 3 + list(rs.randint(1, 90, 150))
    uid = np.repeat(rs.permutation(len(lengths)), lengths).astype(np.int32)
    uid = uid[rs.permutation(len(uid))]                         # interleaved: first-appearance order is not sorted order
    n = len(uid)
    r = rs.choice([0.2, 0.4, 0.6, 0.8, 1.0], n).astype(np.float32)
    # family 4: every user mixes NaN, +inf, -inf, +-0.0, FLT_MAX and finite ties.  The numbers of NaN and +inf go through six
    # scenarios inside every segment class (longest segments first), so that the two fall inside the first ten together, and each
    # of them across the boundary of the tenth rank (asserted in the test below)
    pool = np.array([-np.inf, 0.0, -0.0, FLT_MAX, -FLT_MAX, 0.5, 0.5, -1.0, 1.0, 1e-40], np.float32)
    scenarios = ((2, 3), (4, 9), (12, 3), (0, 5), (5, 0), (1, 1))
    special = pool[rs.randint(0, len(pool), n)]
    cnt = np.bincount(uid)
    turn = [0] * 5
    for u in np.argsort(-cnt, kind='stable'):
        at = rs.permutation(np.flatnonzero(uid == u))
        n_nan, n_inf = scenarios[turn[segment_class(cnt[u])] % len(scenarios)]
        turn[segment_class(cnt[u])] += 1
        special[at[:n_nan]] = np.nan
        special[at[n_nan:n_nan + n_inf]] = np.inf
    families = {'ties': rs.choice(np.linspace(-1, 1, 7), n).astype(np.float32),
                'distinct': rs.standard_normal(n).astype(np.float32),
                'nan': np.where(rs.rand(n) < 0.2, np.nan, rs.choice(np.linspace(-1, 1, 5), n)).astype(np.float32),
                'special': special}
    return uid, r, families


@pytest.fixture(scope='module')
def ranking():
    uid, r, families = ranking_set()
    return uid, r, families, {name: O.eval_users_from_pred(uid, r, p) for name, p in families.items()}


def test_special_family_has_nan_and_inf_inside_and_across_the_tenth_rank(ranking):
    """The inputs of the test below do what the issue of the ranking order needs: users whose NaN and +inf predictions all fall
    inside the first ten, users where the +inf run crosses the tenth rank and users where the NaN run does, in segments of every
    class (<= 16, <= 32, <= 64, several entries per lane, from memory); real -inf in segments shorter than a quarter wave."""
    uid, _, families, _ = ranking
    p = families['special']
    seen = set()
    for u in np.unique(uid):
        v = p[uid == u]
        n_nan, n_inf, cnt = int(np.isnan(v).sum()), int(np.isposinf(v).sum()), len(v)
        klass = segment_class(cnt)
        if n_nan and n_inf and n_nan + n_inf <= 10:
            seen.add(('inside', klass))
        if n_nan and n_nan < 10 < n_nan + n_inf:
            seen.add(('inf across', klass))
        if n_inf and n_nan > 10:
            seen.add(('nan across', klass))
        if cnt < 16 and np.isneginf(v).any():
            seen.add(('-inf padded', klass))
    assert {(what, k) for what in ('inside', 'inf across', 'nan across') for k in range(5)} <= seen and ('-inf padded', 0) in seen, sorted(seen)


@pytest.mark.parametrize('family', ('ties', 'distinct', 'nan', 'special'))
@pytest.mark.parametrize('cached', (True, False))
def test_per_user_ranking_equals_numpy(ranking, family, cached):
    """hits and NDCG of every user from ure_eval_users, in both launch forms (cached ranking of the ratings: eval_rank_kernel +
    eval_metrics_kernel; none: eval_users_kernel), against numpy's stable argsort read backwards (oracle/cpu_ref.py
    eval_users_from_pred) with np.array_equal: the keys order as -inf < finite < +inf < NaN, -0.0 == +0.0, ties by position, and
    NDCG is the same float64 arithmetic in the same order."""
    from ultrare_amd import engine
    nv, L, st = native()
    uid, r, families, want = ranking
    pred = families[family]
    ev = engine.EvalSet(uid, np.zeros(len(uid), np.int32), r)
    ev.pred.copy_(torch.from_numpy(pred[ev.order]))
    ev.hits.fill_(-7)
    ev.ndcg.fill_(-7.0)
    nv.check(L.ure_eval_users(nv.ptr(ev.off), ev.n_users, nv.ptr(ev.pred), nv.ptr(ev.rating), nv.ptr(ev.log2), nv.ptr(ev.hits), nv.ptr(ev.ndcg),
                              nv.ptr(ev.top_rating) if cached else None, ev.n_wide, ev.n_half, st), 'ure_eval_users')
    users, hits, ndcg = want[family]
    at = {int(u): k for k, u in enumerate(users)}
    sel = [at[int(u)] for u in ev.users]
    assert np.array_equal(ev.hits.cpu().numpy(), np.asarray(hits, np.int64)[sel])
    assert np.array_equal(ev.ndcg.cpu().numpy(), np.asarray(ndcg, np.float64)[sel])
