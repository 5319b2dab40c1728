"""The ure_score contract on the CPU (oracle/mf_oracle.c: ure_oracle_score_contract, ure_oracle_score_sse; DESIGN.md "The ure_score
contract"): it is a dot product within float32's error, and it is told apart from the summation orders a wrong kernel would compute
-- otherwise the device tests of tests/test_gpu_score_contract.py, which compare with it bit for bit, would prove nothing about
order.  Also the numpy restatements of the fixed reduction orders and the key order of the prediction ranking."""
import numpy as np
import pytest

from oracle import cpu_ref as O

N_USER, N_ITEM = 97, 61
WIDTHS = (4, 8, 16, 32, 64, 128, 256)


def tables(seed, d, S, n_user=N_USER, n_item=N_ITEM):
    """S models of mixed signs and magnitudes (a normal value times a log-normal scale): sums whose rounding depends on the order."""
    rs = np.random.RandomState(seed)
    mk = lambda n: (rs.standard_normal((n, d)) * np.exp(1.5 * rs.standard_normal((n, d)))).astype(np.float32)
    return [(mk(n_user), mk(n_item)) for _ in range(S)]


def all_pairs():
    uid, iid = np.divmod(np.arange(N_USER * N_ITEM, dtype=np.int32), np.int32(N_ITEM))
    return uid.astype(np.int32), iid.astype(np.int32)


def tree(part, swap_level=None):
    """Balanced tree of adjacent pairs over the last axis in float32; swap_level = l: at level l element j is paired with j + 2 w
    instead of j + w (w = 2^l), the pairing a butterfly with one exchanged step computes."""
    part = part.copy()
    level = 0
    while part.shape[-1] > 1:
        if level == swap_level and part.shape[-1] >= 4:
            q = part.reshape(part.shape[:-1] + (-1, 4))
            part = np.stack([q[..., 0] + q[..., 2], q[..., 1] + q[..., 3]], axis=-1).reshape(part.shape[:-1] + (-1,))
        else:
            part = part[..., 0::2] + part[..., 1::2]
        level += 1
    return part[..., 0]


@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('S', (1, 4, 5, 33))
def test_contract_is_a_dot_product_within_float32_error(d, S):
    """|contract - float64 dot| <= k 2^-24 sum_m sum_c |u_c v_c| / S with k = (3 + log2(d/4)) + (S - 1) + 1.
    Derivation (first order in 2^-24, every operation rounds once, an intermediate sum is at most the sum of the absolute terms
    that entered it): inside a group of four columns a product passes the fmaf chain, three roundings; the d/4 partials pass
    log2(d/4) levels of the tree: depth 3 + log2(d/4) per model; the models are added with S - 1 roundings (the first addition,
    to zero, is exact); the division rounds once.  (The first product of a chain has a rounding of its own in front of the three
    fmaf, so the strict worst case is one more than k; k is the tighter figure and the one held here.)"""
    models = tables(100 + d, d, S)
    uid, iid = all_pairs()
    got = O.score_contract(models, uid, iid).astype(np.float64)
    exact, mag = np.zeros(len(uid)), np.zeros(len(uid))
    for U, V in models:
        t = U[uid].astype(np.float64) * V[iid].astype(np.float64)           # float32 products are exact in float64
        exact += t.sum(axis=1)
        mag += np.abs(t).sum(axis=1)
    k = (3 + int(np.log2(d // 4))) + (S - 1) + 1
    bound = k * 2.0 ** -24 * mag / S
    err = np.abs(got - exact / S)
    assert (err <= bound).all(), float((err / bound).max())
    assert err.max() > 0                                                     # (a float32 result: it does round)


@pytest.mark.parametrize('d', WIDTHS)
def test_contract_is_told_apart_from_the_near_misses(d):
    """On these inputs the contract differs in at least one bit from: the sequential dot (products rounded, added left to right:
    ure_oracle_score); every tree with one level's pairing swapped (d >= 16: there is a level with two pairs); the models added
    lane by lane before the lane sum (d >= 8: more than one lane).  And it IS the tree of the partials, rebuilt here in numpy."""
    S = 5
    models = tables(200 + d, d, S)
    uid, iid = all_pairs()
    want = O.score_contract(models, uid, iid)
    parts = np.stack([O.score_partials(U, V, uid, iid) for U, V in models])          # [S, n, d/4]
    acc = np.zeros(len(uid), np.float32)
    for m in range(S):
        acc = acc + tree(parts[m])
    assert np.array_equal(acc / np.float32(S), want)
    assert not np.array_equal(O.score(models, uid, iid), want)
    for level in range(int(np.log2(d // 4)) - 1):
        acc = np.zeros(len(uid), np.float32)
        for m in range(S):
            acc = acc + tree(parts[m], swap_level=level)
        assert not np.array_equal(acc / np.float32(S), want), level
    if d >= 8:
        lanes = np.zeros(parts.shape[1:], np.float32)
        for m in range(S):
            lanes = lanes + parts[m]
        assert not np.array_equal(tree(lanes) / np.float32(S), want)
    # a model added twice, or one left out, of course differs too; and the running form equals the one-call form
    run = O.score_contract(models[:2], uid, iid, n_total=S, last=False)
    assert np.array_equal(O.score_contract(models[2:], uid, iid, n_total=S, first=False, running=run), want)
    assert not np.array_equal(O.score_contract(models[1:], uid, iid, n_total=S, first=False, running=run), want)


@pytest.mark.parametrize('d', WIDTHS)
def test_sse_partials_layout_and_order(d):
    """ure_oracle_score_sse: slots past `blocks` are zero, the total is the squared error within float32's error, and below the cap
    (one pair per accumulator) every slot is the butterfly of its 4 G squared errors -- rebuilt here in numpy; above the cap the
    strided accumulation differs from adding the same pairs slot by slot."""
    G = 64 // (d // 4)
    rs = np.random.RandomState(d)
    for n in (1, G + 1, 4 * G + 1, 8192 * G + G + 3):
        pred = (rs.standard_normal(n) * np.exp(rs.standard_normal(n))).astype(np.float32)
        r = rs.choice([0.2, 0.4, 0.6, 0.8, 1.0], n).astype(np.float32)
        sse = O.score_sse_partials(pred, r, d)
        blocks = min(-(-(-(-n // G)) // 4), O.SCORE_PARTIALS)
        assert sse.shape == (O.SCORE_PARTIALS,) and not sse[blocks:].any() and (sse[:blocks] > 0).all()
        e = (pred - r).astype(np.float32)
        sq = (e * e).astype(np.float32)                                    # fmaf(e, e, 0) = the rounded square
        np.testing.assert_allclose(sse.sum(), (e.astype(np.float64) ** 2).sum(), rtol=1e-6)
        if n <= 8192 * G:
            pad = np.zeros(blocks * 4 * G, np.float32)
            pad[:n] = sq
            want = tree(pad.reshape(blocks, 4, G)).astype(np.float64)
            assert np.array_equal(want[:, 0] + want[:, 1] + want[:, 2] + want[:, 3], sse[:blocks])
        else:
            n_acc = blocks * 4 * G
            first = np.zeros(n_acc, np.float32)
            first[:] = sq[:n_acc]
            second = np.zeros(n_acc, np.float32)
            second[:n - n_acc] = sq[n_acc:]
            apart = tree(first.reshape(blocks, 4, G)).astype(np.float64).sum(axis=1) + tree(second.reshape(blocks, 4, G)).astype(np.float64).sum(axis=1)
            assert not np.array_equal(apart, sse[:blocks])


def test_reduction_orders_are_told_apart_from_plain_sums():
    """tree_1024 (ure_eval_reduce / ure_eval_subset) and the sequential float32 sum (ure_sum_vectors) against the exact sums, and
    against numpy's own order, which they are not."""
    rs = np.random.RandomState(5)
    for n in (0, 1, 63, 1023, 1024, 1025, 5000):
        x = rs.standard_normal(n) * np.exp(3 * rs.standard_normal(n))
        got = O.tree_1024(x)
        assert abs(got - float(np.sum(x.astype(np.longdouble)))) <= 14 * 2.0 ** -53 * np.abs(x).sum()
        h = rs.randint(0, 11, n).astype(np.int64)
        assert O.tree_1024(h) == h.sum() and O.tree_1024(h).dtype == np.int64
    x = rs.standard_normal(5000) * np.exp(3 * rs.standard_normal(5000))
    assert O.tree_1024(x) != np.sum(x) and O.tree_1024(x) != sum(x.tolist())
    vec = [(rs.standard_normal(257) * np.exp(rs.standard_normal(257))).astype(np.float32) for _ in range(70)]
    got = O.sum_vectors(vec)
    assert got.dtype == np.float32 and not np.array_equal(got, np.sum(np.stack(vec), axis=0, dtype=np.float64).astype(np.float32))
    np.testing.assert_allclose(got, np.sum(np.stack(vec), axis=0, dtype=np.float64), rtol=0, atol=70 * 2.0 ** -24 * np.abs(np.stack(vec)).sum(axis=0).max())


def test_ranking_key_order_is_numpys():
    """The order the prediction ranking must give (np.argsort: -inf < finite < +inf < NaN, -0.0 == +0.0, ties by position) on the
    issue's example: NaN ordered AS +inf would give 4 3 1 0 2 5."""
    p = np.array([np.nan, np.inf, 1, np.inf, np.nan, -np.inf], np.float32)
    assert list(np.argsort(p, kind='stable')[::-1]) == [4, 0, 3, 1, 2, 5]
    uid = np.zeros(6, np.int32)
    r = np.array([1.0, 0.2, 1.0, 0.2, 0.2, 1.0], np.float32)
    users, hits, ndcg = O.eval_users_from_pred(uid, r, p)
    assert list(users) == [0] and list(hits) == [3]
    # eval_from_pred is the mean of the per-user numbers
    rmse, n, h = O.eval_from_pred(uid, r, np.nan_to_num(p, posinf=9, neginf=-9), 4)
    assert n == float(np.mean(O.eval_users_from_pred(uid, r, np.nan_to_num(p, posinf=9, neginf=-9))[2])) and h == 0.3
