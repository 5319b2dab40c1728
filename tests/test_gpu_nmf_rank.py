"""NeuMF catalogue sweeps on the device (csrc/nmf_rank.hip): ure_nmf_recommend_topk and ure_nmf_rank_pairs against the scores
engine.nmf_score gives the same pairs and a key sort over them (nmf.rank_keys, held to a brute-force lexsort by
tests/test_cpu_nmf_rank.py), against nmf.recommend_ref / rank_ref in numpy on the smallest cases, on dirty memory inside guard
zones, through the operators and through Sisa.  Every comparison is bitwise: int32 views of scores, equal integers for items and
ranks."""
import ctypes

import numpy as np
import pytest
import torch

import nmf_cases as C
from abi_arena import Arena, run_prefills, verdict
from ultrare_amd import nmf

pytestmark = pytest.mark.gpu

# (k, layers, S, n_item, top_k, n_query): the issue's; the last is one more whose top-k runs two item splits and their merge
# (at top_k = 100 a split holds 16 top_k = 1,600 items at least, so 1,100 items stay one split there; the ranks split at 512)
CASES = [(4, [8, 4], 1, 1, 1, 1), (32, [32, 16], 5, 63, 10, 7), (8, [16, 128, 4], 3, 65, 65, 7), (32, [64, 32], 5, 3416, 10, 1000),
         (16, [16, 8, 8, 4, 4], 33, 130, 128, 7), (128, [128, 64], 2, 1100, 100, 3), (32, [32, 16], 2, 1100, 10, 3)]


@pytest.fixture(scope='module')
def nv():
    from ultrare_amd import _native
    _native.lib()
    torch.cuda.set_device(0)
    return _native


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32).view(np.int32)


def ints(a):
    return a.detach().cpu().numpy().astype(np.int64)


def make_models(k, layers, S, n_user, n_item, seed):
    """S models of one stack as numpy triples (every model its own tables, as the kernel's loads are general)."""
    return [C.model_init(np.random.RandomState(seed + 17 * s), n_user, n_item, k, layers) for s in range(S)]


def on_device(models):
    return [tuple(torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).cuda() for t in m) for m in models]


def device_scores(dev, k, layers, users, n_item):
    """[n, n_item] float32: the ensemble mean engine.nmf_score writes for every (user, item) pair, one call per model."""
    from ultrare_amd import engine
    uid = torch.from_numpy(np.repeat(np.asarray(users, dtype=np.int32), n_item)).cuda()
    iid = torch.from_numpy(np.tile(np.arange(n_item, dtype=np.int32), len(users))).cuda()
    pred = None
    for m, (U, V, dense) in enumerate(dev):
        pred = engine.nmf_score(U, V, dense, k, layers, uid, iid, pred=pred, n_models_total=len(dev), first=m == 0, last=m == len(dev) - 1)
    return pred.cpu().numpy().reshape(len(users), n_item)


def random_excl(rs, n_query, n_item, share):
    rows = [np.flatnonzero(rs.random_sample(n_item) < share).astype(np.int32) for _ in range(n_query)]
    off = np.zeros(n_query + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, (np.concatenate(rows) if rows else np.zeros(0, np.int32)).astype(np.int32)


def csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)


def oracle_topk(sc, top_k, excl):
    """The key sort over a score matrix: (score bits [n, top_k] int32, items [n, top_k]) with padding (NaN, -1)."""
    n, n_item = sc.shape
    keys = nmf.rank_keys(sc.reshape(-1), np.tile(np.arange(n_item), n)).reshape(n, n_item)
    if excl is not None:
        keys[np.repeat(np.arange(n), np.diff(excl[0])), excl[1]] = 0
    order = np.argsort(keys, axis=1)[:, ::-1][:, :top_k]
    live = np.take_along_axis(keys, order, axis=1) != 0
    items = np.full((n, top_k), -1, dtype=np.int64)
    s = np.full((n, top_k), np.nan, dtype=np.float32)
    items[:, :order.shape[1]][live] = order[live]
    s[:, :order.shape[1]][live] = np.take_along_axis(sc, order, axis=1)[live]
    return s, items


def same_topk(got, want, what=''):
    (gs, gi), (ws, wi) = got, want
    gi = ints(gi)
    assert np.array_equal(gi, wi), what
    pad = wi < 0
    assert np.array_equal(bits(gs)[~pad], bits(ws)[~pad]) and np.isnan(gs.cpu().numpy()[pad]).all(), what


# ------------------------------------------------------------------ 1. top-k
@pytest.mark.parametrize('excluded', [False, True], ids=['all', 'excl'])
@pytest.mark.parametrize('k,layers,S,n_item,top_k,n_query', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_topk_equals_the_scores_sorted(nv, k, layers, S, n_item, top_k, n_query, excluded):
    from ultrare_amd import engine
    n_user = n_query + 3
    models = make_models(k, layers, S, n_user, n_item, seed=k + n_item)
    dev = on_device(models)
    rs = np.random.RandomState(n_item)
    users = rs.permutation(n_user)[:n_query]
    excl = random_excl(rs, n_query, n_item, 0.05) if excluded else None
    if excluded and n_item == 1:
        excl = (np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32))          # the one item excluded: a row of padding
    sc = device_scores(dev, k, layers, users, n_item)
    got = engine.nmf_recommend(dev, k, layers, users, top_k, excl)
    assert got[0].shape == got[1].shape == (n_query, top_k) and got[0].dtype == torch.float32 and got[1].dtype == torch.int64
    same_topk(got, oracle_topk(sc, top_k, excl))
    if n_item <= 63:                                                                 # the two smallest: the whole contract in numpy
        assert np.array_equal(bits(nmf.catalogue_scores_ref(models, k, layers, users, n_item)), bits(sc))
        same_topk(got, nmf.recommend_ref(models, k, layers, users, n_item, top_k, excl))


# ------------------------------------------------------------------ 2. ties, NaN, +inf, padding
def special_case():
    """(8, [16, 8]) x 2 models over 1,100 items (two item splits of 576 at top_k = 10): duplicated item rows across the tile
    boundary 63 | 64 and the split boundary 575 | 576, a NaN and a +inf score, a row with three eligible items and one with none."""
    k, layers, n_user, n_item = 8, [16, 8], 9, 1100
    models = make_models(k, layers, 2, n_user, n_item, seed=5)
    hpos = nmf.Shape(k, layers).h_at
    for U, V, dense in models:
        V[[63, 64, 575, 576]] = V[10]
        V[20, k] = np.nan
        V[21, 0] = np.inf
        U[:, 0] = np.abs(U[:, 0]) + 0.1
        dense[hpos] = abs(dense[hpos]) + 0.1
    users = np.array([0, 1, 2, 3, 4, 5, 6])
    rows = [[], [10, 64], [21], np.setdiff1d(np.arange(n_item), [63, 576, 20]), np.arange(n_item), [20], [5, 6]]
    return k, layers, models, users, n_item, csr(rows)


def test_ties_special_values_and_padding(nv):
    from ultrare_amd import engine
    k, layers, models, users, n_item, excl = special_case()
    dev = on_device(models)
    sc = device_scores(dev, k, layers, users, n_item)
    assert np.isnan(sc[:, 20]).all() and np.isposinf(sc[:, 21]).all()
    for t in (63, 64, 575, 576):
        assert np.array_equal(bits(sc[:, t]), bits(sc[:, 10]))
    for ex in (None, excl):
        for top_k in (10, 128):
            same_topk(engine.nmf_recommend(dev, k, layers, users, top_k, ex), oracle_topk(sc, top_k, ex), (top_k, ex is not None))
    s, it = engine.nmf_recommend(dev, k, layers, users, 10, excl)
    it = ints(it)
    assert it[0, 0] == 21 and it[2, 0] != 21                                          # +inf first, unless excluded
    assert it[4].tolist() == [-1] * 10 and np.isnan(s[4].cpu().numpy()).all()            # everything excluded
    assert it[3, :3].tolist() == [63, 576, 20] and it[3, 3:].tolist() == [-1] * 7         # the tie by id, the NaN last, then padding
    assert np.isnan(s[3, 2].item())
    # the five tied items stand together, in id order, in a full row
    full = ints(engine.nmf_recommend(dev, k, layers, users[:1], 128)[1])[0].tolist()
    if 10 in full[:120]:
        at = full.index(10)
        assert full[at:at + 5] == [10, 63, 64, 575, 576]


# ------------------------------------------------------------------ 3. ranks
def test_ranks_equal_counting_over_the_scores(nv):
    from ultrare_amd import engine
    k, layers, n_user, n_item = 8, [16, 8], 8, 600
    models = make_models(k, layers, 2, n_user, n_item, seed=9)
    for U, V, dense in models:
        V[[70, 300]] = V[7]                                                             # equal scores, told apart by the id
    dev = on_device(models)
    rs = np.random.RandomState(3)
    users = np.array([5, 0, 3, 7, 3])
    long_row = rs.randint(0, n_item, 4097)                                               # > 4,096 targets: the row counts in global memory
    rows = [rs.permutation(n_item)[:50].tolist() + [7, 70, 300, 7], [], long_row, [4, 9, 9, 250], np.arange(n_item)]
    targets = csr(rows)
    excl = csr([[1, 2, 3], [5], np.unique(rs.randint(0, n_item, 40)), [9, 100], []])
    sc = device_scores(dev, k, layers, users, n_item)
    for ex in (None, excl):
        got = engine.nmf_rank_pairs(dev, k, layers, users, targets, ex)
        assert got.dtype == torch.int32 and got.shape == (len(targets[1]),)
        want = nmf.rank_ref(None, k, layers, users, targets, ex, scores=sc, n_item=n_item)
        assert np.array_equal(ints(got), want)
        got = ints(got)
        # every rank r < top_k is position r of nmf_recommend under the same exclusion
        _, items = engine.nmf_recommend(dev, k, layers, users, 128, ex)
        items = ints(items)
        row = np.repeat(np.arange(len(users)), np.diff(targets[0]))
        low = (got >= 0) & (got < 128)
        assert low.sum() > 200 and np.array_equal(items[row[low], got[low]], targets[1][low])
    assert ints(engine.nmf_rank_pairs(dev, k, layers, users, targets, excl))[targets[0][3] + 1] == -1          # the excluded target
    assert engine.nmf_rank_pairs(dev, k, layers, users, csr([[], [], [], [], []])).numel() == 0


@pytest.mark.parametrize('k,layers,S,n_item,top_k,n_query', CASES[1:], ids=lambda v: str(v).replace(' ', ''))
def test_ranks_at_every_stack(nv, k, layers, S, n_item, top_k, n_query):
    from ultrare_amd import engine
    n_query = min(n_query, 40)
    n_user = n_query + 3
    models = make_models(k, layers, S, n_user, n_item, seed=k + n_item)
    dev = on_device(models)
    rs = np.random.RandomState(n_item + 1)
    users = rs.permutation(n_user)[:n_query]
    targets = csr([rs.randint(0, n_item, rs.randint(0, 9)) for _ in range(n_query)])
    excl = random_excl(rs, n_query, n_item, 0.05)
    sc = device_scores(dev, k, layers, users, n_item)
    for ex in (None, excl):
        got = ints(engine.nmf_rank_pairs(dev, k, layers, users, targets, ex))
        assert np.array_equal(got, nmf.rank_ref(None, k, layers, users, targets, ex, scores=sc, n_item=n_item))
    if n_item <= 63:
        assert np.array_equal(got, nmf.rank_ref(models, k, layers, users, targets, excl))


# (k, layers) -> the (QW, passes' shift) the top-k (top_k = 10) and the rank entries run it at (nmf.rank_plan: the header's list): every
# instantiation and every pass count; the last two hold 192 activation columns a lane, so the pair scorer runs in two passes as well
NARROW = [((4, [8, 4, 32, 4]), (2, 0), (2, 0)), ((128, [8, 8, 64, 4]), (1, 0), (1, 0)), ((4, [128, 4, 128, 4]), (1, 1), (1, 1)),
          ((128, [128, 4, 64, 128, 8]), (1, 2), (1, 2)), ((128, [128, 4, 64, 128, 16]), (1, 2), (1, 3))]


@pytest.mark.parametrize('stack,plan_topk,plan_rank', NARROW, ids=lambda v: str(v).replace(' ', ''))
def test_stacks_that_need_fewer_users_or_lanes_at_a_time(nv, stack, plan_topk, plan_rank):
    from ultrare_amd import engine
    k, layers = stack
    assert (nmf.rank_plan(k, layers, 10), nmf.rank_plan(k, layers, None)) == (plan_topk, plan_rank)
    n_user, n_item, n_query = 9, 130, 6
    dev = on_device(make_models(k, layers, 2, n_user, n_item, seed=k + len(layers)))
    rs = np.random.RandomState(k)
    users = rs.permutation(n_user)[:n_query]
    excl = random_excl(rs, n_query, n_item, 0.05)
    targets = csr([rs.randint(0, n_item, rs.randint(0, 9)) for _ in range(n_query)])
    sc = device_scores(dev, k, layers, users, n_item)
    assert len(np.unique(bits(sc))) > n_item                                           # (the stack does not score everything alike)
    for ex in (None, excl):
        same_topk(engine.nmf_recommend(dev, k, layers, users, 10, ex), oracle_topk(sc, 10, ex))
        got = ints(engine.nmf_rank_pairs(dev, k, layers, users, targets, ex))
        assert np.array_equal(got, nmf.rank_ref(None, k, layers, users, targets, ex, scores=sc, n_item=n_item))


# ------------------------------------------------------------------ 4. reproducibility
def test_rows_do_not_depend_on_the_batch_or_the_stream(nv):
    from ultrare_amd import engine
    k, layers, n_user, n_item = 32, [64, 32], 70, 700
    dev = on_device(make_models(k, layers, 3, n_user, n_item, seed=21))
    rs = np.random.RandomState(4)
    users = rs.permutation(n_user)[:37]
    users[20] = users[3]                                                              # a user twice in one batch
    excl = random_excl(rs, len(users), n_item, 0.05)
    excl = (excl[0], excl[1])
    targets = csr([rs.randint(0, n_item, 6) for _ in users])
    s, it = engine.nmf_recommend(dev, k, layers, users, 10)
    r = engine.nmf_rank_pairs(dev, k, layers, users, targets)
    assert np.array_equal(bits(s[20]), bits(s[3])) and np.array_equal(ints(it[20]), ints(it[3]))
    for q in (3, 36):                                                                 # alone: another tile, another grid
        s1, it1 = engine.nmf_recommend(dev, k, layers, users[q:q + 1], 10)
        assert np.array_equal(bits(s1[0]), bits(s[q])) and np.array_equal(ints(it1[0]), ints(it[q]))
        t1 = (np.array([0, 6]), targets[1][6 * q:6 * q + 6])
        assert np.array_equal(ints(engine.nmf_rank_pairs(dev, k, layers, users[q:q + 1], t1)), ints(r[6 * q:6 * q + 6]))
    torch.cuda.synchronize()
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            s2, it2 = engine.nmf_recommend(dev, k, layers, users, 10, excl, stream=stream)
            r2 = engine.nmf_rank_pairs(dev, k, layers, users, targets, excl, stream=stream)
        stream.synchronize()
        s0, it0 = engine.nmf_recommend(dev, k, layers, users, 10, excl)
        assert np.array_equal(bits(s2), bits(s0)) and np.array_equal(ints(it2), ints(it0))
        assert np.array_equal(ints(r2), ints(engine.nmf_rank_pairs(dev, k, layers, users, targets, excl)))


# ------------------------------------------------------------------ 5. the raw ABI on dirty memory inside guard zones
def test_raw_abi_in_guard_zones(nv):
    """Both entries at exactly the sizer's scratch under the three prefills (0x00, 0xFF, 0x5A): guards and inputs intact, every
    output byte written and equal under every prefill, and equal to the engine's clean run."""
    from ultrare_amd import engine
    k, layers, n_user, n_item, top_k = 8, [16, 8, 4], 12, 1100, 10
    models = make_models(k, layers, 2, n_user, n_item, seed=33)
    rs = np.random.RandomState(8)
    users = np.array([4, 0, 11, 7, 4], dtype=np.int32)
    excl = random_excl(rs, len(users), n_item, 0.05)
    targets = csr([rs.randint(0, n_item, 5) for _ in users[:-1]] + [[]])
    lay = np.array(layers, np.int32)
    L = nv.lib()
    n, n_t = len(users), len(targets[1])
    dev = on_device(models)
    want_s, want_i = engine.nmf_recommend(dev, k, layers, users, top_k, excl)
    want_r = engine.nmf_rank_pairs(dev, k, layers, users, targets, excl)

    def arena(outputs, scratch_bytes):
        A = Arena('cuda')
        for m, (U, V, dense) in enumerate(models):
            A.input(f'U{m}', U), A.input(f'V{m}', V), A.input(f'D{m}', dense)
        A.input('users', users), A.input('excl_off', excl[0]), A.input('excl_items', excl[1])
        A.input('tgt_off', targets[0]), A.input('tgt_items', targets[1])
        for name, nbytes in outputs:
            A.output(name, nbytes)
        A.scratch('ws', scratch_bytes)
        return A

    tabs = lambda A: [(ctypes.c_void_p * len(models))(*[A.addr(f'{c}{m}') for m in range(len(models))]) for c in 'UVD']
    need = L.ure_nmf_recommend_scratch(n, n_item, top_k, len(models), k, nv.ptr(lay), len(lay))
    assert need == n * 2 * top_k * 12                                                 # two splits: the merge runs
    A = arena([('scores', n * top_k * 4), ('items', n * top_k * 4)], need)

    def call_rec(A):
        Up, Vp, Dp = tabs(A)
        nv.check(L.ure_nmf_recommend_topk(Up, Vp, Dp, len(models), k, nv.ptr(lay), len(lay), n_user, A.addr('users'), n, n_item, A.addr('excl_off'),
                                          A.addr('excl_items'), top_k, A.addr('scores'), A.addr('items'), A.addr('ws'), A.size('ws'),
                                          nv.stream_handle()), 'ure_nmf_recommend_topk')
    reports = run_prefills(A, call_rec, sync=torch.cuda.synchronize)
    assert verdict(reports) == []
    assert np.array_equal(np.frombuffer(reports[0].outputs['scores'], np.int32), bits(want_s).reshape(-1))
    assert np.array_equal(np.frombuffer(reports[0].outputs['items'], np.int32), ints(want_i).reshape(-1))

    need = L.ure_nmf_rank_pairs_scratch(n, n_t, n_item, len(models), k, nv.ptr(lay), len(lay))
    assert need == n_t * 24
    A = arena([('ranks', n_t * 4)], need)

    def call_rank(A):
        Up, Vp, Dp = tabs(A)
        nv.check(L.ure_nmf_rank_pairs(Up, Vp, Dp, len(models), k, nv.ptr(lay), len(lay), n_user, A.addr('users'), n, n_item, A.addr('tgt_off'),
                                      A.addr('tgt_items'), A.addr('excl_off'), A.addr('excl_items'), A.addr('ranks'), A.addr('ws'), A.size('ws'),
                                      nv.stream_handle()), 'ure_nmf_rank_pairs')
    reports = run_prefills(A, call_rank, sync=torch.cuda.synchronize)
    assert verdict(reports) == []
    assert np.array_equal(np.frombuffer(reports[0].outputs['ranks'], np.int32), ints(want_r))


# ------------------------------------------------------------------ 6. the operators
def test_ops_match_the_engine(nv):
    from ultrare_amd import engine, ops  # noqa: F401
    k, layers, n_user, n_item = 16, [32, 16], 20, 150
    dev = on_device(make_models(k, layers, 3, n_user, n_item, seed=2))
    rs = np.random.RandomState(6)
    users = np.arange(0, 20, 2)
    excl = random_excl(rs, len(users), n_item, 0.05)
    targets = csr([rs.randint(0, n_item, 4) for _ in users])
    Us, Vs, Ds = ([m[j] for m in dev] for j in range(3))
    t = lambda a: torch.from_numpy(np.asarray(a)).cuda()
    for ex in (None, excl):
        e_off, e_items = (None, None) if ex is None else (t(ex[0]), t(ex[1]))
        s, it = torch.ops.ultrare.nmf_recommend_topk(Us, Vs, Ds, k, layers, t(users), e_off, e_items, 7)
        ws, wi = engine.nmf_recommend(dev, k, layers, users, 7, ex)
        assert np.array_equal(bits(s), bits(ws)) and np.array_equal(ints(it), ints(wi)) and it.dtype == torch.int64
        r = torch.ops.ultrare.nmf_rank_pairs(Us, Vs, Ds, k, layers, t(users), t(targets[0]), t(targets[1]), e_off, e_items)
        assert np.array_equal(ints(r), ints(engine.nmf_rank_pairs(dev, k, layers, users, targets, ex))) and r.dtype == torch.int32


# ------------------------------------------------------------------ 7. Sisa
def test_sisa_recommends_and_ranks_before_and_after_unlearning(nv):
    import scipy.sparse as sp
    import test_gpu_nmf as T
    from ultrare_amd import engine
    from ultrare_amd.method import utils
    ml, ml2, s, s2 = T.sisa_request()
    idx, trd, ted, tot = T.synthetic_loaders()
    del_user = idx[1][:5]
    _, trd2, _, tot2 = T.synthetic_loaders(del_user)

    def train_csr(loaders):
        u = np.concatenate([np.asarray(d.dataset.users, dtype=np.int64) for d in loaders])
        i = np.concatenate([np.asarray(d.dataset.items, dtype=np.int64) for d in loaders])
        return sp.csr_matrix((np.ones(len(u), np.float32), (u, i)), shape=(T.SYN_USER, T.SYN_ITEM))
    users = np.arange(T.SYN_USER)
    keys = set(utils.rank_metrics(np.array([0, 1]), np.array([0])))
    out = []
    for sisa, models, loaders, test in ((s, ml, trd, tot), (s2, ml2, trd2, tot2)):
        excl = train_csr(loaders)
        got = sisa.recommend_nmf(users, 10, excl)
        want = utils.recommend_nmf(models, users, 10, excl)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(ints(got[1]), ints(want[1]))
        # ... and they are the scores the models' own forward gives, sorted
        sc = device_scores([m.tables() for m in models], models[0].k, models[0].layers, users, T.SYN_ITEM)
        same_topk(got, oracle_topk(sc, 10, engine.exclusion_rows(excl, users)))
        metrics = sisa.rank_eval_nmf(test, excl)
        assert metrics == utils.rank_eval_nmf(models, test, excl) and set(metrics) == keys
        ds = test.dataset
        distinct = len(set(zip(np.asarray(ds.users).tolist(), np.asarray(ds.items).tolist())))
        assert sisa.rank_eval_nmf(test)['n_pairs'] == distinct                       # nothing excluded: every distinct test pair counts
        assert 0 < metrics['n_pairs'] <= distinct and 0.0 <= metrics['hr@10'] <= 1.0
        out.append((bits(got[0]).copy(), ints(got[1]).copy(), metrics))
    assert not np.array_equal(out[0][0], out[1][0]) and out[0][2] != out[1][2]          # unlearning moved the answers
