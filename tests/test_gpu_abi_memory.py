"""The memory contract of the stateless device entry points (DESIGN.md "The memory contract of the C ABI"), entry by entry
through the raw C ABI (_native.lib(), not engine): every buffer of a call is carved out of one guarded arena
(tests/abi_arena.py), the scratch is exactly the entry's own sizer's size, and the call runs three times with outputs and
scratch prefilled with 0x00, 0xFF and 0x5A.  Asserted, on bytes (NaN and -0.0 by pattern):

  * the three runs give the same output bytes -- with complementary prefills also the proof that every byte was written
    and that nothing was computed from stale outputs or scratch;
  * no guard byte and no input byte changed;
  * the outputs are what the existing wrapper (engine.*, the torch op, or the numpy statement the suite already holds
    the kernel to) returns for the same inputs, which ties the raw call to the references of the other test modules and
    catches a case that passes its arguments wrongly three times alike;
  * bytes an in-place entry must not write (rows not named, padding columns) still hold the prefill.

Shapes are the smallest that leave a ragged tail in every tiled dimension and take more than one workgroup or split;
the derivation from the constants of the sources stands beside each case, with the result of reading the entry's kernels
for reads before writes ("audit:").  INVENTORY classifies every bound name; tests/test_cpu_abi_arena.py fails when a
name is in no class, and runs the sizers of these very cases on the host.
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

from abi_arena import PREFILLS, Arena, run_prefills, verdict

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p

# ---------------------------------------------------------------------------------------------------------------------
# Every name of ultrare_amd/_native.py's signature table, in one of five classes.
# ---------------------------------------------------------------------------------------------------------------------
_SCORE = 'tests/test_gpu_score_contract.py::'
INVENTORY = {
    # host-only: no device memory of the caller's
    'ure_abi_version': ('host', ''), 'ure_source_hash': ('host', ''), 'ure_last_error': ('host', ''), 'ure_device_info': ('host', ''),
    'ure_host_randperm': ('host', ''), 'ure_host_randperm_tags': ('host', ''), 'ure_host_mt_advance': ('host', ''),
    'ure_host_mt_jump_blocks': ('host', ''), 'ure_host_mt_jump_support': ('host', ''), 'ure_host_mt_charpoly': ('host', ''),
    'ure_host_draw_int64': ('host', ''), 'ure_host_mf_init': ('host', ''), 'ure_host_mf_init_batch': ('host', ''),
    'ure_host_normal_blocks': ('host', ''), 'ure_host_normal_blocks_scalar': ('host', ''), 'ure_host_read_csv': ('host', ''),
    'ure_host_free': ('host', ''), 'ure_host_partition': ('host', ''), 'ure_host_partition64': ('host', ''),
    'ure_host_build_layout': ('host', ''), 'ure_host_build_layouts': ('host', ''), 'ure_host_build_layouts_units': ('host', ''),
    'ure_host_build_layouts_units_start': ('host', ''), 'ure_host_build_layouts_units_wait': ('host', ''), 'ure_host_build_units': ('host', ''),
    'ure_host_assign_desc_f64': ('host', ''), 'ure_host_kmeans_assign': ('host', ''),
    'ure_ot_assign': ('host', 'the exact LP: host memory in and out'), 'ure_ot_assign_warm': ('host', 'the exact LP: host memory in and out'),
    'ure_ot_potentials': ('host', 'reads a device matrix; its outputs are host memory and its device state is its own allocation'),
    # stateful: the job's memory comes from csrc/block_cache.cpp and keeps the job's rule of DESIGN 4.20 (whole jobs on poisoned memory)
    **{n: ('stateful', 'tests/test_gpu_job_memory.py::test_a_job_gives_the_same_bytes_on_memory_of_every_fill') for n in (
        'ure_job_create', 'ure_job_destroy', 'ure_job_shard_steps', 'ure_job_ticks', 'ure_job_train', 'ure_job_materialize',
        'ure_job_touch_rows', 'ure_job_index_read', 'ure_job_train_profiled')},
    # sizers: host code, run by tests/test_cpu_abi_arena.py on the shapes of the cases below
    **{n: ('sizer', '') for n in (
        'ure_device_randperm_tags_scratch', 'ure_device_shuffle_tags_scratch', 'ure_device_shuffle_tags_flag', 'ure_device_mf_init_scratch',
        'ure_recommend_scratch', 'ure_rank_pairs_scratch', 'ure_pair_knn_scratch', 'ure_ot_sinkhorn_scratch', 'ure_combine_stats_len',
        'ure_combine_stats_scratch', 'ure_ridge_rows_scratch', 'ure_csr_cost_scratch', 'ure_csr_kmeans_cost_scratch',
        'ure_balanced_fill_scratch', 'ure_mmd_scratch', 'ure_mmd_splits')},
    # already run on prefilled outputs elsewhere (the scoring path: every output filled with -7 before the call)
    'ure_score': ('prefilled', _SCORE + 'test_score_equals_the_contract_at_every_width_count_and_model_count'),
    'ure_eval_series': ('prefilled', _SCORE + 'test_series_routes_equal_single_evaluations_at_every_width'),
    'ure_eval_series_compact': ('prefilled', _SCORE + 'test_series_routes_equal_single_evaluations_at_every_width'),
    'ure_score_own_compact': ('prefilled', _SCORE + 'test_series_routes_equal_single_evaluations_at_every_width'),
    'ure_eval_series_own': ('prefilled', _SCORE + 'test_series_routes_equal_single_evaluations_at_every_width'),
    'ure_eval_users': ('prefilled', _SCORE + 'test_per_user_ranking_equals_numpy'),
    'ure_eval_reduce': ('prefilled', _SCORE + 'test_reduce_and_subset_orders'),
    'ure_eval_subset': ('prefilled', _SCORE + 'test_reduce_and_subset_orders'),
    'ure_device_shuffle_tags': ('prefilled', 'tests/test_gpu_shuffle.py::test_shuffle_tags_equal_the_hosts'),
    # arena cases: CASES below
    **{n: ('arena', '') for n in (
        'ure_copy_rows_batch', 'ure_epoch_sse_batch', 'ure_device_randperm_tags', 'ure_device_mf_init', 'ure_eval_rank_ratings', 'ure_sum_vectors',
        'ure_merge_rows', 'ure_recommend_topk', 'ure_rank_pairs', 'ure_pair_knn', 'ure_pair_rowsum', 'ure_pair_cols', 'ure_pair_label_expsum',
        'ure_ot_cost', 'ure_ot_cost_mfma', 'ure_ot_centroids', 'ure_ot_centroids_members', 'ure_kmeans_cost', 'ure_kmeans_centroids',
        'ure_ot_sinkhorn', 'ure_combine_stats', 'ure_score_weighted', 'ure_ridge_rows', 'ure_csr_cost', 'ure_csr_centroids',
        'ure_csr_kmeans_cost', 'ure_csr_kmeans_centroids', 'ure_balanced_fill', 'ure_mmd_bandwidth', 'ure_mmd_loss_grad', 'ure_u2u_loss_grad',
        'ure_mmd_matrix')},
}
CLASSES = ('arena', 'sizer', 'host', 'stateful', 'prefilled')

# The shapes each sizer must refuse with -1 (tests/test_cpu_abi_arena.py): k = 0, k = 257 for the CSR calls, d = 129 for
# ure_mmd_scratch, n k >= 2^32 for ure_balanced_fill_scratch.
SIZER_REFUSALS = [
    ('ure_csr_cost_scratch', (0,)), ('ure_csr_cost_scratch', (257,)),
    ('ure_csr_kmeans_cost_scratch', (0,)), ('ure_csr_kmeans_cost_scratch', (257,)),
    ('ure_balanced_fill_scratch', (320, 0)), ('ure_balanced_fill_scratch', (320, 257)), ('ure_balanced_fill_scratch', (1 << 30, 4)),
    ('ure_mmd_scratch', (129, 129)), ('ure_mmd_splits', (129, 129)),
    ('ure_recommend_scratch', (3, 70, 0)), ('ure_pair_knn_scratch', (130, 130, 0, 0)), ('ure_ot_sinkhorn_scratch', (257, 0)),
    ('ure_combine_stats_scratch', (65, 0)), ('ure_combine_stats_len', (0,)), ('ure_ridge_rows_scratch', (5, 0)),
]


class Plan:
    """One case, built without touching a device: the arena's buffers are declared, `call(A)` makes the raw call, `want()`
    (device only) returns {output name: numpy array} from the existing wrapper, `keep` marks the output bytes the call must
    leave alone, `sizers` lists the (sizer, args, value) the case asked."""

    def __init__(self, A):
        self.A, self.call, self.want, self.keep, self.sizers, self.host = A, None, None, {}, [], {}

    def sizer(self, name, *args):
        from ultrare_amd import _native as nv
        v = int(getattr(nv.lib(), name)(*args))
        self.sizers.append((name, args, v))
        assert v >= 0, (name, args, v)
        return v


def _lib():
    from ultrare_amd import _native as nv
    return nv, nv.lib(), nv.stream_handle()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptrs(A, names):
    return (_vp * len(names))(*[A.addr(n) for n in names])


def _check(rc, what):
    from ultrare_amd import _native as nv
    nv.check(rc, what)


def _tables(P, rs, S, n_user, n_item, d):
    """S models' padded tables as arena inputs 'U0', 'V0', ... -> [(U, V)] numpy."""
    out = []
    for s in range(S):
        U, V = rs.standard_normal((n_user, d)).astype(np.float32), rs.standard_normal((n_item, d)).astype(np.float32)
        P.A.input(f'U{s}', U)
        P.A.input(f'V{s}', V)
        out.append((U, V))
    return out


def _dev_tables(tables):
    return [(_dev(U), _dev(V)) for U, V in tables]


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mmd.hip.  64-row tiles; DQ = 1, 2, 4, 8 for d <= 16, 32, 64, 128; splits = min(row tiles, 16) at these sizes;
# column-sum workgroups = m / 256.  (65, 64, 17): m = 129 -> 3 row tiles, 3 splits, a 1-row tile, DQ = 2.  (40, 30, 40):
# DQ = 4.  (300, 300, 5): m = 600 -> two column-sum workgroups, 10 tiles.  ld = d + 3; the unselected rows and the padding
# columns are NaN (never read).
# audit: attr_colsum writes partial[b][0..3][f < d] and attr_stats reads exactly those, then writes stats[0], [1] and the
# three column blocks for f < d (all u2u_grad reads); mmd_kernel writes part_sums of every (tile, split) and part_grad of
# every (split, row < m, f < d) before mmd_sums / mmd_grad_combine read them.  Nothing is read before it is written.
# ---------------------------------------------------------------------------------------------------------------------
MMD_SHAPES = [(65, 64, 17), (40, 30, 40), (300, 300, 5)]


def _mmd_inputs(P, n1, n2, d):
    rs = np.random.RandomState(n1 * 1000 + d)
    m, ld, extra = n1 + n2, d + 3, 7
    X = np.full((m + extra, ld), np.nan, dtype=np.float32)
    rows = rs.permutation(m + extra)[:m].astype(np.int32)
    X[rows, :d] = rs.standard_normal((m, d)).astype(np.float32) * 0.5
    P.A.input('X', X)
    P.A.input('rows', rows)
    return X, rows, m, ld


def _mmd_wrapper_args(X, rows, n1, d):
    from ultrare_amd import engine
    Xd = _dev(X)
    return Xd[:, :d], engine.GroupRows(rows[:n1], rows[n1:], X.shape[0], Xd.device)


def _bandwidth_value(X, rows, d):
    x = X[rows, :d].astype(np.float64)
    m = len(rows)
    return np.array([(2 * m * (x * x).sum() - 2 * (x.sum(0) ** 2).sum()) / (m * m - m)], dtype=np.float64)


def case_mmd_bandwidth(A, n1, n2, d):
    P = Plan(A)
    X, rows, m, ld = _mmd_inputs(P, n1, n2, d)
    A.output('bw', 8)
    A.scratch('ws', P.sizer('ure_mmd_scratch', m, d))

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_mmd_bandwidth(A.addr('X'), ld, d, A.addr('rows'), n1, n2, A.addr('bw'), A.addr('ws'), A.size('ws'), st), 'ure_mmd_bandwidth')

    def want():
        from ultrare_amd import engine
        return {'bw': engine.mmd_bandwidth(*_mmd_wrapper_args(X, rows, n1, d)).cpu().numpy()}
    P.call, P.want = call, want
    return P


def case_mmd_loss_grad(A, n1, n2, d, grad):
    P = Plan(A)
    X, rows, m, ld = _mmd_inputs(P, n1, n2, d)
    bw = _bandwidth_value(X, rows, d)
    A.input('bw', bw)
    A.output('sums', 32)
    if grad:
        A.output('grad', m * d * 4)
    A.scratch('ws', P.sizer('ure_mmd_scratch', m, d))
    P.sizer('ure_mmd_splits', m, d)

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_mmd_loss_grad(A.addr('X'), ld, d, A.addr('rows'), n1, n2, 2.0, 5, A.addr('bw'), A.addr('sums'), A.addr('grad' if grad else None),
                                   A.addr('ws'), A.size('ws'), st), 'ure_mmd_loss_grad')

    def want():
        from ultrare_amd import engine
        sums, g = engine.mmd_loss_grad(*_mmd_wrapper_args(X, rows, n1, d), _dev(bw).reshape(()), 2.0, 5, want_grad=grad)
        return {'sums': sums.cpu().numpy(), **({'grad': g.cpu().numpy()} if grad else {})}
    P.call, P.want = call, want
    return P


def case_u2u(A, n1, n2, d, grad):
    P = Plan(A)
    X, rows, m, ld = _mmd_inputs(P, n1, n2, d)
    A.output('value', 8)
    if grad:
        A.output('grad', m * d * 4)
    A.scratch('ws', P.sizer('ure_mmd_scratch', m, d))

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_u2u_loss_grad(A.addr('X'), ld, d, A.addr('rows'), n1, n2, A.addr('value'), A.addr('grad' if grad else None), A.addr('ws'),
                                   A.size('ws'), st), 'ure_u2u_loss_grad')

    def want():
        from ultrare_amd import engine
        v, g = engine.u2u_loss_grad(*_mmd_wrapper_args(X, rows, n1, d), want_grad=grad)
        return {'value': v.cpu().numpy(), **({'grad': g.cpu().numpy()} if grad else {})}
    P.call, P.want = call, want
    return P


def case_mmd_matrix(A, n1, n2, d):
    # audit: no scratch; every K[gi][gj] with gi, gj < m is stored by its tile's thread
    P = Plan(A)
    X, rows, m, ld = _mmd_inputs(P, n1, n2, d)
    bw = _bandwidth_value(X, rows, d)
    A.input('bw', bw)
    A.output('K', m * m * 4)

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_mmd_matrix(A.addr('X'), ld, d, A.addr('rows'), m, 2.0, 5, A.addr('bw'), A.addr('K'), st), 'ure_mmd_matrix')

    def want():
        from ultrare_amd import engine
        return {'K': engine.mmd_matrix(*_mmd_wrapper_args(X, rows, n1, d), _dev(bw).reshape(()), 2.0, 5).cpu().numpy()}
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mf_recommend.hip.  64 items per tile, 64 candidate slots, splits = min(1024 / user tiles, n_item / max(512, 16 k)),
# k <= 128.  (d, S, n_item, k, n_query) = (4, 1, 70, 100, 3): one split, two item tiles (64 + 6), 70 candidates < k, so
# the (NaN, -1) padding of 30 places per row must be written, and the scratch is 0 bytes (given fenced, and as NULL).  (8, 2, 1100, 10, 3): 2 splits
# (1100 / 512), span 576, a ragged last tile, exclusions, user 1 excluding the whole catalogue.
# audit: tk / ts / thr / cnt are cleared in LDS by the kernel; every (row, split, place < k) of pkey / pscore is written by
# rec_topk_kernel before rec_merge_splits_kernel reads it; scores / items get all k places of every row (padding from the
# cleared list).  The model table is the library's own stream-ordered allocation.
# ---------------------------------------------------------------------------------------------------------------------
def case_recommend(A, d, S, n_item, k, n_query, with_excl, null_scratch=False):
    P = Plan(A)
    rs = np.random.RandomState(n_item + k)
    n_user = 9
    tables = _tables(P, rs, S, n_user, n_item, d)
    users = np.array([5, 0, 8], dtype=np.int32)[:n_query]
    A.input('users', users)
    excl = None
    if with_excl:
        lists = [np.sort(rs.choice(n_item, 37, replace=False)), np.arange(n_item), np.zeros(0, dtype=np.int64)][:n_query]
        off = np.zeros(n_query + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=off[1:])
        excl = (off, np.concatenate(lists).astype(np.int32))
        A.input('excl_off', excl[0])
        A.input('excl_items', excl[1])
    A.output('scores', n_query * k * 4)
    A.output('items', n_query * k * 4)
    A.scratch('ws', P.sizer('ure_recommend_scratch', n_query, n_item, k))
    assert not (null_scratch and A.size('ws'))               # (0 bytes: the scratch may be NULL)

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_recommend_topk(_ptrs(A, [f'U{s}' for s in range(S)]), _ptrs(A, [f'V{s}' for s in range(S)]), S, A.addr('users'), n_query, n_item, d,
                                    A.addr('excl_off' if with_excl else None), A.addr('excl_items' if with_excl else None), k, A.addr('scores'),
                                    A.addr('items'), A.addr(None if null_scratch else 'ws'), A.size('ws'), st), 'ure_recommend_topk')

    def want():
        from ultrare_amd import engine
        scores, items = engine.recommend(_dev_tables(tables), d, users, k, excl)
        got_items = items.cpu().numpy()
        if with_excl:
            assert (got_items[1] == -1).all()               # the user who excludes everything: padding only
        else:
            assert (got_items[:, n_item:] == -1).all() and (got_items[:, :n_item] >= 0).all()
        return {'scores': scores.cpu().numpy(), 'items': got_items.astype(np.int32)}
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mf_rank.hip.  A workgroup keeps 4,096 sorted target keys in LDS; rows beyond count in global memory.  One user with
# 4,100 targets (over the LDS budget: the global path) over 5,000 items (9 item splits), beside users with 0 and 1
# targets (the LDS path); duplicates among the targets; excluded targets give -1.
# audit: rank_keys_kernel writes tkey, ranks (0 / -1) and bucket = 0 for every target before rank_sort reads tkey and
# writes spos / skey; excl / stream only add to written buckets; scan and gather read what those wrote.  The scratch
# holds no index or counter that is read before it is written.
# ---------------------------------------------------------------------------------------------------------------------
def case_rank_pairs(A):
    P = Plan(A)
    rs = np.random.RandomState(11)
    d, S, n_user, n_item = 4, 1, 6, 5000
    tables = _tables(P, rs, S, n_user, n_item, d)
    users = np.array([4, 1, 2], dtype=np.int32)
    t_rows = [rs.randint(0, n_item, 4100), np.zeros(0, dtype=np.int64), np.array([77])]
    e_rows = [np.unique(np.concatenate([t_rows[0][:40], rs.choice(n_item, 60)])), np.array([3, 9]), np.array([5])]
    t_off, e_off = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    np.cumsum([len(x) for x in t_rows], out=t_off[1:])
    np.cumsum([len(x) for x in e_rows], out=e_off[1:])
    t_items, e_items = np.concatenate(t_rows).astype(np.int32), np.concatenate(e_rows).astype(np.int32)
    n_t = len(t_items)
    for name, a in (('users', users), ('t_off', t_off), ('t_items', t_items), ('e_off', e_off), ('e_items', e_items)):
        A.input(name, a)
    A.output('ranks', n_t * 4)
    A.scratch('ws', P.sizer('ure_rank_pairs_scratch', 3, n_t, n_item, d))

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_rank_pairs(_ptrs(A, ['U0']), _ptrs(A, ['V0']), S, A.addr('users'), 3, n_item, d, A.addr('t_off'), A.addr('t_items'),
                                A.addr('e_off'), A.addr('e_items'), A.addr('ranks'), A.addr('ws'), A.size('ws'), st), 'ure_rank_pairs')

    def want():
        from ultrare_amd import engine
        ranks = engine.rank_pairs(_dev_tables(tables), d, users, (t_off, t_items), (e_off, e_items)).cpu().numpy()
        assert (ranks[:40] == -1).all() and ranks[-1] >= 0
        return {'ranks': ranks}
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/pair_dist.hip.  64-row tiles, 16-feature chunks; n = 130 (two full tiles and a 2-row one), d = 17 (one chunk and
# one feature), n_nb = 10.  kNN: splits 0 (automatic: 3 column tiles -> 3) and forced 3, streamed (euclidean) and given
# source, with and without a query list.
# audit: pair_knn_kernel writes all n_nb places of every (split, query) list (fillers ~0) before the merge reads them; the
# merge writes every place < n_nb of every query exactly once (keys are unique, n_nb <= n).  rowsum / cols / label_expsum
# have no scratch and store every element of their outputs under the tile bounds.
# ---------------------------------------------------------------------------------------------------------------------
PAIR_N, PAIR_D = 130, 17


def _pair_source(P, metric):
    rs = np.random.RandomState(5)
    X = rs.standard_normal((PAIR_N, PAIR_D)).astype(np.float32)
    if metric is None:
        D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
        D[3, 7] = D[3, 9]                                  # an exact tie inside a row
        P.A.input('src', D)
        return D, PAIR_N, PAIR_N
    P.A.input('src', X)
    return X, PAIR_N, PAIR_D


def case_pair_knn(A, metric, splits, with_query):
    P = Plan(A)
    from ultrare_amd import engine
    src, n, d = _pair_source(P, metric)
    n_nb = 10
    query = np.array([129, 0, 64, 63, 5, 5], dtype=np.int32) if with_query else None
    nq = n if query is None else len(query)
    if with_query:
        A.input('query', query)
    A.output('dist', nq * n_nb * 4)
    A.output('idx', nq * n_nb * 4)
    A.scratch('ws', P.sizer('ure_pair_knn_scratch', nq, n, n_nb, splits))
    code = engine.PAIR_METRICS[metric or 'given']

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_pair_knn(A.addr('src'), n, d, code, A.addr('query' if with_query else None), nq, n_nb, splits, A.addr('dist'), A.addr('idx'),
                              A.addr('ws'), A.size('ws'), st), 'ure_pair_knn')

    def want():
        dist, idx = engine.pair_knn(_dev(src), n_nb, metric, query, splits)
        return {'dist': dist.cpu().numpy(), 'idx': idx.cpu().numpy().astype(np.int32)}
    P.call, P.want = call, want
    return P


def case_pair_rowsum(A, metric):
    P = Plan(A)
    from ultrare_amd import engine
    src, n, d = _pair_source(P, metric)
    A.output('R', n * 4)
    code = engine.PAIR_METRICS[metric or 'given']

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_pair_rowsum(A.addr('src'), n, d, code, A.addr('R'), st), 'ure_pair_rowsum')
    P.call, P.want = call, lambda: {'R': engine.pair_rowsum(_dev(src), metric).cpu().numpy()}
    return P


def case_pair_cols(A, metric):
    P = Plan(A)
    from ultrare_amd import engine
    src, n, d = _pair_source(P, metric)
    cols = np.array([129, 0, 64], dtype=np.int32)
    A.input('cols', cols)
    A.output('out', n * 3 * 4)
    code = engine.PAIR_METRICS[metric or 'given']

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_pair_cols(A.addr('src'), n, d, code, A.addr('cols'), 3, A.addr('out'), st), 'ure_pair_cols')
    P.call, P.want = call, lambda: {'out': engine.pair_cols(_dev(src), cols, metric).cpu().numpy()}
    return P


def case_pair_label_expsum(A, metric):
    P = Plan(A)
    from ultrare_amd import engine
    src, n, d = _pair_source(P, metric)
    k = 3
    label = (np.arange(n) % k).astype(np.int32)
    A.input('label', label)
    A.output('W', n * k * 8)
    code = engine.PAIR_METRICS[metric or 'given']

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_pair_label_expsum(A.addr('src'), n, d, code, A.addr('label'), k, A.addr('W'), st), 'ure_pair_label_expsum')
    P.call, P.want = call, lambda: {'W': engine.pair_label_expsum(_dev(src), label, k, metric).cpu().numpy()}
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/ot_sinkhorn.hip.  256 points per workgroup: (n, k) = (257, 3) is two workgroups, the second with one point, k below
# the 4 waves of the column pass; (255, 33) is one ragged workgroup and k over 32.  30 iterations at most (one batch of
# 10 and one of 20 between host reads), with and without u and cost_min.
# audit: the 16-byte state is cleared by hipMemsetAsync before the first kernel reads its stop word; pm / ps are written
# for every (column, workgroup) by each pass before the combine reads them; v[0] is written by the first combine before
# the first iteration reads it; u (the caller's, or the scratch's) is written before the label pass.  An internal u goes
# to the scratch, so the result cannot depend on whether u is asked for.
# ---------------------------------------------------------------------------------------------------------------------
def case_sinkhorn(A, n, k, want_u, want_cost_min):
    P = Plan(A)
    rs = np.random.RandomState(n + k)
    dist = rs.rand(k, n).astype(np.float32)
    A.input('dist', dist)
    A.output('v', k * 8)
    A.output('label', n * 4)
    if want_u:
        A.output('u', n * 8)
    if want_cost_min:
        A.output('cost_min', n * 4)
    A.scratch('ws', P.sizer('ure_ot_sinkhorn_scratch', n, k))
    reg, cap, thr = 0.05, 30, 1e-9

    def call(A):
        nv, L, st = _lib()
        iters, err = ctypes.c_int32(), ctypes.c_double()
        _check(L.ure_ot_sinkhorn(A.addr('dist'), n, k, reg, cap, thr, A.addr('u' if want_u else None), A.addr('v'), A.addr('label'),
                                 A.addr('cost_min' if want_cost_min else None), A.addr('ws'), A.size('ws'), ctypes.byref(iters), ctypes.byref(err), st),
               'ure_ot_sinkhorn')
        P.host.setdefault('iters_err', []).append((int(iters.value), float(err.value)))

    def want():
        from ultrare_amd import engine
        r = engine.ot_sinkhorn(_dev(dist), reg, cap, thr, want_u=want_u, want_cost_min=want_cost_min)
        assert all(x == (r['iters'], r['err']) for x in P.host['iters_err']), (P.host['iters_err'], r['iters'], r['err'])
        return {name: r[name].cpu().numpy() for name in ('v', 'label') + (('u',) if want_u else ()) + (('cost_min',) if want_cost_min else ())}
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mf_combine.hip.  64 pairs per tile, one workgroup per tile (at most 2,048), URE_SCORE_PARTIALS = 2,048 partials.
# n = 65 (a full tile and a 1-pair tile) and 129 (three workgroups), S = 2 and 5 (phase A takes the models four at a
# time: one ragged group, and a full group with a ragged one), d = 8, both links.
# audit: combine_stats_kernel writes partial[b][1 .. len) of every workgroup (word 0 is never written and never read);
# combine_reduce_kernel writes out[1 .. len) and out[0].  score_weighted_kernel writes pred[j] for every pair, sse[b] for
# every workgroup, and workgroup 0 zeroes sse[grid .. 2048).
# ---------------------------------------------------------------------------------------------------------------------
def _pairs(P, rs, n, n_user, n_item):
    uid, iid = rs.randint(0, n_user, n).astype(np.int32), rs.randint(0, n_item, n).astype(np.int32)
    rating = (rs.randint(1, 6, n) / 5.0).astype(np.float32)
    for name, a in (('uid', uid), ('iid', iid), ('rating', rating)):
        P.A.input(name, a)
    return uid, iid, rating


def case_combine_stats(A, n, S, link):
    P = Plan(A)
    rs = np.random.RandomState(n + S)
    d, n_user, n_item = 8, 20, 30
    tables = _tables(P, rs, S, n_user, n_item, d)
    uid, iid, rating = _pairs(P, rs, n, n_user, n_item)
    w = (rs.standard_normal(S + 1) * 0.3).astype(np.float64)
    A.input('w', w)
    A.output('out', P.sizer('ure_combine_stats_len', S) * 8)
    A.scratch('ws', P.sizer('ure_combine_stats_scratch', n, S))

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_combine_stats(_ptrs(A, [f'U{s}' for s in range(S)]), _ptrs(A, [f'V{s}' for s in range(S)]), S, A.addr('uid'), A.addr('iid'),
                                   A.addr('rating'), n, d, link, A.addr('w'), A.addr('out'), A.addr('ws'), A.size('ws'), st), 'ure_combine_stats')

    def want():
        from ultrare_amd import engine
        return {'out': engine.combine_stats(_dev_tables(tables), d, (uid, iid, rating), link, w)}
    P.call, P.want = call, want
    return P


def case_score_weighted(A, n, S, link, with_sse, with_groups):
    P = Plan(A)
    from ultrare_amd import engine
    rs = np.random.RandomState(n + S + link)
    d, n_user, n_item, G = 8, 20, 30, 3
    tables = _tables(P, rs, S, n_user, n_item, d)
    uid, iid, rating = _pairs(P, rs, n, n_user, n_item)
    W = (rs.standard_normal((G, S + 1)) * 0.3).astype(np.float64)
    A.input('W', W)
    gou = None
    if with_groups:
        gou = rs.randint(0, G, n_user).astype(np.int32)
        if link == 0:
            gou[uid[0]] = -1                               # in no group: the mean ensemble (link 0 only: callers refuse it under link 1)
        A.input('gou', gou)
    A.output('pred', n * 4)
    if with_sse:
        A.output('sse', engine.SCORE_PARTIALS * 8)

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_score_weighted(_ptrs(A, [f'U{s}' for s in range(S)]), _ptrs(A, [f'V{s}' for s in range(S)]), S, A.addr('uid'), A.addr('iid'),
                                    A.addr('rating' if with_sse else None), n, d, link, A.addr('W'), G, A.addr('gou' if with_groups else None),
                                    n_user if with_groups else 0, A.addr('pred'), A.addr('sse' if with_sse else None), st), 'ure_score_weighted')

    def want():
        pred, sse = engine.score_weighted(_dev_tables(tables), d, _dev(uid), _dev(iid), _dev(rating) if with_sse else None, link, _dev(W),
                                          _dev(gou) if with_groups else None)
        out = {'pred': pred.cpu().numpy()}
        if with_sse:
            out['sse'] = sse.cpu().numpy()
            grid = (n + 63) // 64
            assert not out['sse'][grid:].view(np.uint64).any()          # the partials beyond the grid: +0.0, bit for bit
        return out
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mf_ridge.hip.  A workgroup per segment, tiles of 64 entries for d <= 32.  d = 8, k = 5 (three padding columns),
# segment lengths [0, 1, 5, 65, 0]: empty segments at both ends, one entry, one tile and a tile with one entry more.
# The zero rows, the zero padding columns and both status words must be written.  The sizer returns 0 bytes: the case
# runs with a fenced zero-byte scratch and `order`, and with scratch = NULL and no `order`.
# audit: status is set to (0, -1) by two hipMemsetAsync before the launch; an empty segment stores all d zeros; every
# other segment stores all d columns (NaN or the solution below k, 0 from k on).  No scratch is touched.
# ---------------------------------------------------------------------------------------------------------------------
def case_ridge(A, with_order):
    P = Plan(A)
    rs = np.random.RandomState(8)
    d, k, n_fixed = 8, 5, 40
    lens = [0, 1, 5, 65, 0]
    m = len(lens)
    off = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    idx = rs.randint(0, n_fixed, off[-1]).astype(np.int32)
    val = (rs.randint(1, 6, off[-1]) / 5.0).astype(np.float32)
    F = rs.standard_normal((n_fixed, d)).astype(np.float32)
    order = np.array([3, 2, 1, 0, 4], dtype=np.int32)
    for name, a in (('F', F), ('off', off), ('idx', idx), ('val', val)) + ((('order', order),) if with_order else ()):
        A.input(name, a)
    A.output('X', m * d * 4)
    A.output('status', 8)
    A.scratch('ws', P.sizer('ure_ridge_rows_scratch', m, k))
    assert A.size('ws') == 0

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_ridge_rows(A.addr('F'), n_fixed, d, k, A.addr('off'), A.addr('idx'), A.addr('val'), m, A.addr('order' if with_order else None),
                                0.1, 0.01, A.addr('X'), A.addr('status'), A.addr('ws' if with_order else None), 0, st), 'ure_ridge_rows')

    def want():
        from ultrare_amd import engine
        segs = engine.SegmentSet.from_device(_dev(off), _dev(idx), _dev(val))
        X = engine.ridge_rows(_dev(F), d, k, segs, 0.1, 0.01, order=order if with_order else None).cpu().numpy()
        assert not X[[0, 4]].view(np.uint32).any() and not X[:, k:].view(np.uint32).any() and X[1:4, :k].all()
        return {'X': X, 'status': np.array([0, -1], dtype=np.int32)}         # (ridge_rows raises on any other status)
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/csr_group.hip, csrc/csr_kmeans.hip.  Lane groups of the power of two >= k (up to 64): k = 5 -> groups of 8 lanes
# with three idle, k = 65 -> two passes of a 64-lane group, the second with one lane; the squared norms by 256 lanes.  The
# matrices are the crafted() ones of the two sparse test modules (130 x 257: one item past the 256 lanes; 203 x 97), one
# cluster without members.  ure_csr_centroids also with ldc = k + 3: the padding columns are not written.
# audit: cc / csq are written for all k centroids by the first small launch before the cost kernel reads them; counts is
# cleared by hipMemsetAsync before csr_counts_kernel adds to it; every Ct[j][c < k] and every dist entry is stored.
# ---------------------------------------------------------------------------------------------------------------------
def _crafted(which):
    if which == 'ot':
        from test_gpu_sparse_group import crafted
        return crafted('rows')
    from test_gpu_sparse_kmeans import crafted
    return crafted()


def _labels_with_a_gap(rs, n, k):
    label = rs.randint(0, k - 1, n).astype(np.int32)
    label[label >= 3] += 1                                  # cluster 3 has no members
    return label


def case_csr_cost(A, which, k):
    P = Plan(A)
    halves = _crafted(which)
    csr = halves[0]
    n, n_item = csr.shape
    rs = np.random.RandomState(k)
    ldc = k + 3 if which == 'ot' else k
    Ct = rs.rand(n_item, ldc).astype(np.float32)
    for name, a in (('off', csr.off), ('col', csr.idx), ('val', csr.val), ('Ct', Ct)):
        A.input(name, a)
    A.output('dist', n * k * 4)
    entry = 'ure_csr_cost' if which == 'ot' else 'ure_csr_kmeans_cost'
    A.scratch('ws', P.sizer(entry + '_scratch', k))

    def call(A):
        nv, L, st = _lib()
        head = (A.addr('off'), A.addr('col'), A.addr('val'), n, n_item, A.addr('Ct'))
        if which == 'ot':
            _check(L.ure_csr_cost(*head, ldc, k, A.addr('dist'), A.addr('ws'), A.size('ws'), st), entry)
        else:
            _check(L.ure_csr_kmeans_cost(*head, k, A.addr('dist'), A.addr('ws'), A.size('ws'), st), entry)

    def want():
        from ultrare_amd import engine
        S = engine.CsrSet(halves)
        return {'dist': (engine.csr_cost if which == 'ot' else engine.csr_kmeans_cost)(S, _dev(Ct), k).cpu().numpy()}
    P.call, P.want = call, want
    return P


def case_csr_centroids(A, which, k, pad):
    P = Plan(A)
    halves = _crafted(which)
    csc = halves[1]
    n, n_item = halves[0].shape
    label = _labels_with_a_gap(np.random.RandomState(k + 1), n, k)
    ldc = k + pad
    for name, a in (('off', csc.off), ('row', csc.idx), ('val', csc.val), ('label', label)):
        A.input(name, a)
    A.output('Ct', n_item * ldc * 4)
    A.output('counts', k * 4)
    if pad:
        mask = np.zeros((n_item, ldc, 4), dtype=bool)
        mask[:, k:] = True
        P.keep['Ct'] = mask.reshape(-1)

    def call(A):
        nv, L, st = _lib()
        if which == 'ot':
            _check(L.ure_csr_centroids(A.addr('off'), A.addr('row'), A.addr('val'), A.addr('label'), n, n_item, k, A.addr('Ct'), ldc, A.addr('counts'), st),
                   'ure_csr_centroids')
        else:
            _check(L.ure_csr_kmeans_centroids(A.addr('off'), A.addr('row'), A.addr('val'), n_item, n, A.addr('label'), k, A.addr('Ct'), A.addr('counts'), st),
                   'ure_csr_kmeans_centroids')

    def want():
        from ultrare_amd import engine
        S = engine.CsrSet(halves)
        Ct, counts = engine.csr_centroids(S, label, k, ldc) if which == 'ot' else engine.csr_kmeans_centroids(S, label, k)
        Ct, counts = Ct.cpu().numpy(), counts.cpu().numpy()
        assert counts[3] == 0 and not Ct[:, 3].view(np.uint32).any()      # the cluster without members: count 0, +0.0 centroid
        return {'Ct': Ct, 'counts': counts}
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/csr_kmeans.hip: the balanced fill.  Workspace = a 4,096-byte head (256 thresholds, 256 counts, a flag) + n keys.
# (n, k, capacity) = (320, 5, 64): two workgroups of 256 users, every group exactly full, distances on a coarse grid so
# that keys tie in the float and differ in the index.  (37, 5, 0): the argmin path, no workspace (NULL, 0 bytes).
# audit: thr is set to ~0 by hipMemsetAsync once, cnt and the flag are cleared before every round; fill_choose_kernel
# writes label and ckey of every user before fill_select_kernel reads them.
# ---------------------------------------------------------------------------------------------------------------------
def case_balanced_fill(A, n, k, capacity):
    P = Plan(A)
    rs = np.random.RandomState(n)
    dist = (rs.randint(0, 12, (n, k)) / 4.0).astype(np.float32)
    A.input('dist', dist)
    A.output('label', n * 4)
    if capacity > 0:
        A.scratch('ws', P.sizer('ure_balanced_fill_scratch', n, k))

    def call(A):
        nv, L, st = _lib()
        rounds = ctypes.c_int64(0)
        _check(L.ure_balanced_fill(A.addr('dist'), n, k, capacity, A.addr('label'), ctypes.byref(rounds), A.addr('ws' if capacity > 0 else None),
                                   A.size('ws') if capacity > 0 else 0, st), 'ure_balanced_fill')
        P.host.setdefault('rounds', []).append(int(rounds.value))

    def want():
        from ultrare_amd import engine
        label, rounds = engine.balanced_fill(_dev(dist), capacity)
        assert P.host['rounds'] == [rounds] * len(P.host['rounds'])
        return {'label': label.cpu().numpy()}
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/ot.hip.  ure_ot_cost stages 64 rows in LDS while 64 (d + 1) floats fit in 64 KiB - 256, i.e. up to d = 254, and
# runs untiled from d = 255; the MFMA form takes 32 rows per wave (128 per workgroup) and 32 centroids per pass; the
# centroid kernels run one thread per (cluster, column).  (n, k, d) = (70, 3, 20): two row tiles, the second of 6 rows.
# (65, 2, 255): the untiled kernel, an odd d for the two-feature MFMA step, a 1-row tile.  The last cluster has no members;
# counts given and NULL.
# audit: no scratch anywhere; every dist[c][i] / dist[i][c] and every C[c][j] is stored under the bounds tests, counts[c]
# by the thread of column 0.  A cluster without members gives 0 / 0 = NaN rows in the OT means and +0.0 rows in k-means.
# ---------------------------------------------------------------------------------------------------------------------
OT_SHAPES = [(70, 3, 20), (65, 2, 255)]


def _ot_inputs(P, n, k, d, labels=False):
    rs = np.random.RandomState(n + d)
    X = (rs.standard_normal((n, d)) * (rs.rand(n, d) < 0.7)).astype(np.float32)
    P.A.input('X', X)
    if labels:
        label = rs.randint(0, k - 1, n).astype(np.int32)      # cluster k - 1 has no members
        return X, label
    C = X[rs.choice(n, k, replace=False)].copy()
    P.A.input('C', C)
    return X, C


def case_dense_cost(A, entry, n, k, d):
    P = Plan(A)
    X, C = _ot_inputs(P, n, k, d)
    A.output('dist', n * k * 4)

    def call(A):
        nv, L, st = _lib()
        _check(getattr(L, entry)(A.addr('X'), A.addr('C'), n, k, d, A.addr('dist'), st), entry)

    def want():
        if entry == 'ure_kmeans_cost':                      # [n][k]; the numpy statement tests/test_gpu_surface.py holds the kernel to
            from oracle import cpu_ref as O
            return {'dist': O.kmeans_dist(X, C)}
        from ultrare_amd import ops
        return {'dist': (ops.ot_cost if entry == 'ure_ot_cost' else ops.ot_cost_mfma)(_dev(X), _dev(C)).cpu().numpy()}
    P.call, P.want = call, want
    return P


def case_dense_centroids(A, entry, n, k, d, with_counts):
    P = Plan(A)
    X, label = _ot_inputs(P, n, k, d, labels=True)
    members = entry == 'ure_ot_centroids_members'
    if members:
        order = np.argsort(label, kind='stable').astype(np.int32)
        off = np.zeros(k + 1, dtype=np.int64)
        np.cumsum(np.bincount(label, minlength=k), out=off[1:])
        A.input('order', order)
        A.input('off', off)
    else:
        A.input('label', label)
    A.output('C', k * d * 4)
    if with_counts:
        A.output('counts', k * 4)

    def call(A):
        nv, L, st = _lib()
        tail = (n, k, d, A.addr('C'), A.addr('counts' if with_counts else None), st)
        if members:
            _check(L.ure_ot_centroids_members(A.addr('X'), A.addr('order'), A.addr('off'), *tail), entry)
        else:
            _check(getattr(L, entry)(A.addr('X'), A.addr('label'), *tail), entry)

    def want():
        if entry == 'ure_kmeans_centroids':                 # oracle/cpu_ref.py: kmeans_centroids, a cluster without members = zeros
            C = np.zeros((k, d), dtype=np.float32)
            for c in range(k):
                rows = np.flatnonzero(label == c)
                inv = np.float32(1.0 / len(rows)) if len(rows) else np.float32(0)
                for i in rows:
                    C[c] += X[i] * inv
        else:                                               # (the member-list kernel computes the same means: include/ultrare_hip.h)
            from ultrare_amd import ops
            C = ops.ot_centroids(_dev(X), _dev(label), k).cpu().numpy()
            assert np.isnan(C[k - 1]).all()
        out = {'C': C}
        if with_counts:
            out['counts'] = np.bincount(label, minlength=k).astype(np.int32)
        return out
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mf_init.hip, csrc/perm_tags.hip, as their own tests: 2 shards of (16, 16) (the smallest fill) and (1616, 41) (a
# re-drawn tail: 41 is no multiple of 16) table rows; permutations of 5 and 4,099 rows (one over 4,096 pending swaps).
# audit: mf_init uploads the plan (descriptors, supports, block 0 of every shard) over the head of the scratch, copies
# block 0 into the segment states and, with more than one segment, clears the others by hipMemsetAsync before the jump
# kernels add into them; one segment here.  perm_tags writes z[0 .. n - 2] and inv[n - 1] before the swaps read them, and
# a swap reads inv[j] only after swap j (or the identity store of n - 1) wrote it; the reservation words are in LDS, and
# the give-up flags behind the scratch are only ever written.
# ---------------------------------------------------------------------------------------------------------------------
def _gen_states(n):
    g = torch.Generator()
    g.manual_seed(1234)
    torch.empty(333, dtype=torch.int32).random_(generator=g)         # the middle of a generator block
    out = []
    for _ in range(n):
        out.append(g.get_state().clone())
        torch.empty(5000).normal_(generator=g)
    return out


def case_mf_init(A, nu, nv_):
    P = Plan(A)
    S = 2
    states = _gen_states(S)
    for s in range(S):
        A.output(f'U{s}', nu * 4)
        A.output(f'V{s}', nv_ * 4)
    A.scratch('ws', 4 * P.sizer('ure_device_mf_init_scratch', S, nu, nv_))

    def call(A):
        nv, L, st = _lib()
        mine = [s.clone() for s in states]
        _check(L.ure_device_mf_init(S, (_vp * S)(*[x.data_ptr() for x in mine]), mine[0].numel(), (ctypes.c_int64 * S)(0, 0),
                                    _ptrs(A, [f'U{s}' for s in range(S)]), nu, _ptrs(A, [f'V{s}' for s in range(S)]), nv_, A.addr('ws'), A.size('ws') // 4, 1,
                                    st), 'ure_device_mf_init')
        P.host.setdefault('end', []).append(mine)

    def want():
        from ultrare_amd import rng
        mine = [s.clone() for s in states]
        got = rng.mf_init_device(mine, nu, nv_, 0, torch.device('cuda', 0))
        torch.cuda.synchronize()
        for end in P.host['end']:
            assert all(torch.equal(a, b) for a, b in zip(end, mine))         # the host states end where the wrapper's do
        out = {}
        for s, (U, V) in enumerate(got):
            out[f'U{s}'], out[f'V{s}'] = U.cpu().numpy(), V.cpu().numpy()
        return out
    P.call, P.want = call, want
    return P


def case_randperm_tags(A, groups):
    P = Plan(A)
    from ultrare_amd import rng
    perms = [(5, 2, 0x1234567890abcdef >> 2), (4099, 1000, 77), (5, 5, 3)]
    n_max = 4099
    for i, (n, _, _) in enumerate(perms):
        A.output(f'tags{i}', n * 2)

    def table(A):
        tab = np.zeros(len(perms), dtype=rng.PERM_DTYPE)
        for i, (n, batch, seed) in enumerate(perms):
            tab[i] = (seed, A.addr(f'tags{i}'), n, batch)
        return tab.view(np.uint8)
    A.input('table', table, nbytes=len(perms) * rng.PERM_DTYPE.itemsize)
    A.scratch('ws', 4 * P.sizer('ure_device_randperm_tags_scratch', n_max, groups))

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_device_randperm_tags(A.addr('table'), len(perms), n_max, A.addr('ws'), A.size('ws') // 4, groups, st), 'ure_device_randperm_tags')

    def want():                                             # ure_host_randperm_tags, what tests/test_gpu_engine.py holds the kernel to
        nv, L, st = _lib()
        out = {}
        for i, (n, batch, seed) in enumerate(perms):
            host = np.empty(n, dtype=np.uint16)
            _check(L.ure_host_randperm_tags(np.array([seed], dtype=np.int64).ctypes.data, 1, n, batch, host.ctypes.data, 1), 'ure_host_randperm_tags')
            out[f'tags{i}'] = host
        return out
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mf_eval.hip, csrc/job_io.hip: the small table entries.  3 rows of 50 x 16; 2 vectors of 65.
# audit: no scratch.  merge_rows stores only the rows it names; copy_rows_batch only columns [0, k) of dst / dst2;
# sum_vectors starts from 0 in its first chunk (it reads `out` only from the second chunk of 32 vectors on, after it
# wrote it); epoch_sse stores one double per (shard, epoch); eval_rank_ratings stores ten positions per user.
# ---------------------------------------------------------------------------------------------------------------------
def case_merge_rows(A):
    P = Plan(A)
    rs = np.random.RandomState(1)
    n, d = 50, 16
    src = rs.standard_normal((n, d)).astype(np.float32)
    rows = np.array([49, 0, 17], dtype=np.int64)
    A.input('src', src)
    A.input('rows', rows)
    A.output('dst', n * d * 4)                               # in place: the rows not named must still hold the prefill
    mask = np.ones((n, d * 4), dtype=bool)
    mask[rows] = False
    P.keep['dst'] = mask.reshape(-1)

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_merge_rows(A.addr('dst'), A.addr('src'), A.addr('rows'), len(rows), d, st), 'ure_merge_rows')

    def want():
        from ultrare_amd import engine
        return {'dst': engine.merge_rows(torch.zeros(n, d, device='cuda'), _dev(src), rows).cpu().numpy()}
    P.call, P.want = call, want
    return P


def case_copy_rows_batch(A, with_dst2):
    P = Plan(A)
    rs = np.random.RandomState(2)
    k, d, rows = 5, 16, [50, 3]
    srcs = [rs.standard_normal((r, k)).astype(np.float32) for r in rows]
    outs = ['dst0', 'dst1'] + (['dst2_0'] if with_dst2 else [])
    for i, s in enumerate(srcs):
        A.input(f'src{i}', s)
    for name in outs:
        r = rows[int(name[-1])]
        A.output(name, r * d * 4)
        mask = np.zeros((r, d, 4), dtype=bool)
        mask[:, k:] = True                                  # columns [k, d) are not written
        P.keep[name] = mask.reshape(-1)

    def call(A):
        nv, L, st = _lib()
        dst2 = (_vp * 2)(A.addr('dst2_0'), None) if with_dst2 else None
        _check(L.ure_copy_rows_batch(2, _ptrs(A, ['src0', 'src1']), _ptrs(A, ['dst0', 'dst1']), dst2, (ctypes.c_int64 * 2)(*rows), k, d, st),
               'ure_copy_rows_batch')

    def want():                                             # a copy: the source itself in the first k columns
        out = {}
        for name in outs:
            s = srcs[int(name[-1])]
            full = np.zeros((len(s), d), dtype=np.float32)
            full[:, :k] = s
            out[name] = full
        return out
    P.call, P.want = call, want
    return P


def case_sum_vectors(A):
    P = Plan(A)
    rs = np.random.RandomState(3)
    vec = [rs.standard_normal(65).astype(np.float32) for _ in range(2)]
    for i, v in enumerate(vec):
        A.input(f'v{i}', v)
    A.output('out', 65 * 4)

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_sum_vectors(_ptrs(A, ['v0', 'v1']), 2, 65, A.addr('out'), st), 'ure_sum_vectors')

    def want():
        from oracle import cpu_ref as O
        return {'out': np.asarray(O.sum_vectors(vec), dtype=np.float32)}
    P.call, P.want = call, want
    return P


def case_epoch_sse(A):
    P = Plan(A)
    rs = np.random.RandomState(4)
    users, E = [65, 300], 3
    sse = [(rs.rand(E, u) * 3).astype(np.float32) for u in users]
    for i, s in enumerate(sse):
        A.input(f'sse{i}', s)
    A.output('out', 2 * E * 8)

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_epoch_sse_batch(2, _ptrs(A, ['sse0', 'sse1']), (ctypes.c_int64 * 2)(*users), E, A.addr('out'), st), 'ure_epoch_sse_batch')

    def want():                                             # csrc/job_io.hip: thread t adds elements t, t + 256, ... in double, then a pairwise fold
        out = np.zeros((2, E), dtype=np.float64)
        for i, s in enumerate(sse):
            for e in range(E):
                part = np.zeros(256, dtype=np.float64)
                for j in range(s.shape[1]):
                    part[j % 256] += np.float64(s[e, j])
                w = 128
                while w:
                    part[:w] += part[w:2 * w]
                    w //= 2
                out[i, e] = part[0]
        return {'out': out}
    P.call, P.want = call, want
    return P


def case_eval_rank_ratings(A):
    P = Plan(A)
    rs = np.random.RandomState(6)
    counts = [70, 40, 33, 20, 17, 5, 1]                      # EvalSet's own order: over 32 entries, 17 .. 32, the rest
    uid = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    rating = (rs.randint(1, 6, len(uid)) / 5.0).astype(np.float32)
    off = np.zeros(len(counts) + 1, dtype=np.int32)
    np.cumsum(counts, out=off[1:])
    A.input('off', off)
    A.input('rating', rating)
    A.output('top', len(counts) * 10 * 4)

    def call(A):
        nv, L, st = _lib()
        _check(L.ure_eval_rank_ratings(A.addr('off'), len(counts), A.addr('rating'), A.addr('top'), st), 'ure_eval_rank_ratings')

    def want():
        from ultrare_amd import engine
        ev = engine.EvalSet(uid, np.zeros_like(uid), rating)
        assert np.array_equal(ev.off.cpu().numpy(), off) and np.array_equal(ev.rating.cpu().numpy(), rating)
        return {'top': ev.top_rating.cpu().numpy()}
    P.call, P.want = call, want
    return P


# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'id entry build')


def _cases():
    c = []
    add = lambda cid, entry, fn, *args: c.append(Case(cid, entry, lambda A: fn(A, *args)))
    for n1, n2, d in MMD_SHAPES:
        tag = f'{n1}x{n2}x{d}'
        add(f'mmd_bandwidth-{tag}', 'ure_mmd_bandwidth', case_mmd_bandwidth, n1, n2, d)
        for grad in (True, False):
            add(f'mmd_loss_grad-{"grad" if grad else "sums"}-{tag}', 'ure_mmd_loss_grad', case_mmd_loss_grad, n1, n2, d, grad)
            add(f'u2u_loss_grad-{"grad" if grad else "value"}-{tag}', 'ure_u2u_loss_grad', case_u2u, n1, n2, d, grad)
        add(f'mmd_matrix-{tag}', 'ure_mmd_matrix', case_mmd_matrix, n1, n2, d)
    add('recommend-padding', 'ure_recommend_topk', case_recommend, 4, 1, 70, 100, 3, False)
    add('recommend-padding-null', 'ure_recommend_topk', case_recommend, 4, 1, 70, 100, 3, False, True)
    add('recommend-splits-excl', 'ure_recommend_topk', case_recommend, 8, 2, 1100, 10, 3, True)
    add('rank_pairs', 'ure_rank_pairs', case_rank_pairs)
    for metric, splits, q in (('euclidean', 0, False), ('euclidean', 3, True), (None, 3, False), (None, 0, True)):
        add(f'pair_knn-{metric or "given"}-s{splits}-{"query" if q else "all"}', 'ure_pair_knn', case_pair_knn, metric, splits, q)
    for metric in ('euclidean', None):
        add(f'pair_rowsum-{metric or "given"}', 'ure_pair_rowsum', case_pair_rowsum, metric)
        add(f'pair_cols-{metric or "given"}', 'ure_pair_cols', case_pair_cols, metric)
        add(f'pair_label_expsum-{metric or "given"}', 'ure_pair_label_expsum', case_pair_label_expsum, metric)
    for n, k, u, cm in ((257, 3, True, True), (257, 3, False, False), (255, 33, True, False), (255, 33, False, True)):
        add(f'ot_sinkhorn-{n}x{k}-{"u" if u else "nou"}-{"cmin" if cm else "nocmin"}', 'ure_ot_sinkhorn', case_sinkhorn, n, k, u, cm)
    for n, S, link in ((65, 2, 0), (129, 5, 1), (65, 5, 1), (129, 2, 0)):
        add(f'combine_stats-n{n}-S{S}-link{link}', 'ure_combine_stats', case_combine_stats, n, S, link)
    for n, S, link, sse, gou in ((65, 2, 0, True, True), (129, 5, 1, False, False), (129, 5, 0, True, False), (65, 2, 1, False, True),
                                 (129, 2, 1, True, True)):
        add(f'score_weighted-n{n}-S{S}-link{link}-{"sse" if sse else "nosse"}-{"groups" if gou else "nogroups"}', 'ure_score_weighted',
            case_score_weighted, n, S, link, sse, gou)
    add('ridge_rows-order-scratch', 'ure_ridge_rows', case_ridge, True)
    add('ridge_rows-plain-null', 'ure_ridge_rows', case_ridge, False)
    for k in (5, 65):
        add(f'csr_cost-k{k}', 'ure_csr_cost', case_csr_cost, 'ot', k)
        add(f'csr_kmeans_cost-k{k}', 'ure_csr_kmeans_cost', case_csr_cost, 'kmeans', k)
        add(f'csr_centroids-k{k}', 'ure_csr_centroids', case_csr_centroids, 'ot', k, 0)
        add(f'csr_centroids-k{k}-ldc{k + 3}', 'ure_csr_centroids', case_csr_centroids, 'ot', k, 3)
        add(f'csr_kmeans_centroids-k{k}', 'ure_csr_kmeans_centroids', case_csr_centroids, 'kmeans', k, 0)
    add('balanced_fill-320x5-cap64', 'ure_balanced_fill', case_balanced_fill, 320, 5, 64)
    add('balanced_fill-37x5-argmin', 'ure_balanced_fill', case_balanced_fill, 37, 5, 0)
    for n, k, d in OT_SHAPES:
        tag = f'{n}x{k}x{d}'
        for entry in ('ure_ot_cost', 'ure_ot_cost_mfma', 'ure_kmeans_cost'):
            add(f'{entry[4:]}-{tag}', entry, case_dense_cost, entry, n, k, d)
        for entry in ('ure_ot_centroids', 'ure_ot_centroids_members', 'ure_kmeans_centroids'):
            for counts in (True, False):
                add(f'{entry[4:]}-{tag}-{"counts" if counts else "nocounts"}', entry, case_dense_centroids, entry, n, k, d, counts)
    add('device_mf_init-16x16', 'ure_device_mf_init', case_mf_init, 16, 16)
    add('device_mf_init-1616x41', 'ure_device_mf_init', case_mf_init, 1616, 41)
    add('device_randperm_tags-1group', 'ure_device_randperm_tags', case_randperm_tags, 1)
    add('device_randperm_tags-2groups', 'ure_device_randperm_tags', case_randperm_tags, 2)
    add('merge_rows', 'ure_merge_rows', case_merge_rows)
    add('copy_rows_batch-dst2', 'ure_copy_rows_batch', case_copy_rows_batch, True)
    add('copy_rows_batch', 'ure_copy_rows_batch', case_copy_rows_batch, False)
    add('sum_vectors', 'ure_sum_vectors', case_sum_vectors)
    add('epoch_sse_batch', 'ure_epoch_sse_batch', case_epoch_sse)
    add('eval_rank_ratings', 'ure_eval_rank_ratings', case_eval_rank_ratings)
    return c


CASES = _cases()


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_entry_keeps_the_memory_contract(case):
    P = case.build(Arena('cuda:0'))
    reports = run_prefills(P.A, P.call, sync=torch.cuda.synchronize)
    found = verdict(reports, keep=P.keep)
    assert not found, f'{case.entry}:\n  ' + '\n  '.join(found)
    want = P.want()
    torch.cuda.synchronize()
    assert set(want) == set(reports[0].outputs), (sorted(want), sorted(reports[0].outputs))
    for name, arr in want.items():
        got = np.frombuffer(reports[0].outputs[name], dtype=np.uint8)
        ref = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8)
        assert got.size == ref.size, (case.entry, name, got.size, ref.size)
        diff = got != ref
        if name in P.keep:
            diff &= ~P.keep[name]
        bad = np.flatnonzero(diff)
        assert bad.size == 0, (f'{case.entry}: output {name!r} differs from the wrapper\'s in {bad.size} byte(s), first at offset {int(bad[0])} '
                               f'({got[bad[0]]:#04x} vs {ref[bad[0]]:#04x})')
