"""The masked row walks of the graph kernels (csrc/row_walk.h: gcn_grad, bpr_grad_user, bpr_grad_item, inf_walk) at the edges of their
tiles, bit for bit against the numpy contracts, on both sides of a graph.

Graph A is bpr_cases.long_row_triples(): 67 users x 2,000 items whose USERS' rows -- the unmapped side -- run through every length of
lightgcn_cases.ROW_LENGTHS (0 .. 300: one less than, exactly and one more than a tile of every group width, 129 = two tiles of 64 and
one entry) and one row of 1,500.  Graph T is the same triples transposed: the ITEMS' rows -- the side walked through to_csr -- have
those lengths.  One epoch's order of three steps puts the first 128 entries of the long row, in its own side's walk order, into step
1: at G = 64 two whole tiles lie outside steps 0 and 2 and inside step 1, at every narrower width more of them, and the rest of the
row is mixed."""
import functools
import types

import numpy as np
import pytest
import torch

import bpr_cases as B
import lightgcn_cases as C
from test_cpu_score_contract import tables as mixed_tables
from ultrare_amd import bpr, influence, lightgcn

pytestmark = pytest.mark.gpu
WIDTHS = lightgcn.WIDTHS
STEPS, KEY, L2 = 3, 20240608, 0.2
FULL_TILES = 128                                        # two tiles of the widest group


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want):
    got = _np(got)
    want = np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _zero_rows(t, rows):
    a = _np(t)[rows]
    return a.tobytes() == bytes(a.nbytes)


def _engine():
    from ultrare_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _case(name):
    """Graph 'A' or 'T' on the host and on the device, the epoch's order and tags, the contract's negatives and their index."""
    E = _engine()
    uid, iid, n_user, n_item = B.long_row_triples()
    if name == 'T':
        uid, iid, n_user, n_item = iid, uid, n_item, n_user
    N = len(uid)
    rs = np.random.RandomState(7200 + ord(name))
    rating = rs.uniform(0.2, 1.0, N).astype(np.float32)
    host = lightgcn.Graph(uid, iid, n_user, n_item)
    off, file_pos = (host.off_u, host.pos) if name == 'A' else (host.off_i, host.pos[host.to_csr])
    lengths = np.diff(off)
    long_row = int(lengths.argmax())
    assert lengths[long_row] == C.LONG_ROW and set(C.ROW_LENGTHS) <= set(lengths.tolist())
    batch = -(-N // STEPS)
    first = file_pos[off[long_row]:off[long_row] + FULL_TILES].astype(np.int64)
    perm = rs.permutation(N)
    rest = perm[~np.isin(perm, first)]
    order = np.concatenate([rest[:batch], first, rest[batch:]]).astype(np.int32)
    assert FULL_TILES <= batch and sorted(order.tolist()) == list(range(N))
    file_tag = np.empty(N, np.int32)
    file_tag[order] = np.arange(N) // batch
    row_tags = file_tag[file_pos[off[long_row]:off[long_row + 1]]]
    assert (row_tags[:FULL_TILES] == 1).all()
    for t0 in range(FULL_TILES, C.LONG_ROW - 64, 64):                  # every later tile of 64 holds more than one step
        assert len(set(row_tags[t0:t0 + 64].tolist())) > 1
    off_d, col_d = bpr.distinct_csr(host)
    bpr.check_negatives(host, off_d)
    neg = bpr.sample_ref(host, off_d, col_d, KEY, 0)
    index = bpr.neg_index_ref(neg, host.row_u, n_item)
    short_row = int(np.flatnonzero(lengths == 33)[0])
    active = [m.copy() for m in influence.active_rows(host)[:2]]
    side = 0 if name == 'A' else 1
    assert active[side][long_row] and active[side][short_row]
    active[side][long_row] = active[side][short_row] = False
    g = E.GcnGraph(uid, iid, rating, n_user, n_item)
    return types.SimpleNamespace(name=name, host=host, g=g, n_user=n_user, n_item=n_item, N=N, batch=batch, order=order, rating=rating, r=rating[host.pos],
                                 tag=E.gcn_step_tags(g, order, batch), neg=neg, index=index, neg_d=_dev(neg), index_d=tuple(_dev(a) for a in index),
                                 active=tuple(active), frozen=(side, np.array([long_row, short_row])), long_row=long_row)


def _tables(c, d):
    (U, V), = mixed_tables(7300 + d, d, 1, n_user=c.n_user, n_item=c.n_item)
    return (U * np.float32(0.25)).astype(np.float32), (V * np.float32(0.25)).astype(np.float32)


CASES = [(name, d) for name in 'AT' for d in WIDTHS]
IDS = [f'{name}-d{d}' for name, d in CASES]


@pytest.mark.parametrize('name,d', CASES, ids=IDS)
def test_mse_walks_equal_the_contract_at_every_tile_edge(name, d):
    """engine.gcn_loss_grad at every step: G_u and G_i are lightgcn.loss_grad_ref's bytes, the loss is within 1e-12 relative, rows
    without an entry in the step are +0.0 in every byte."""
    E, c = _engine(), _case(name)
    U, V = _tables(c, d)
    Ud, Vd = _dev(U), _dev(V)
    for step in range(STEPS):
        batch = c.order[step * c.batch:(step + 1) * c.batch]
        Gu, Gi, loss, _ = lightgcn.loss_grad_ref(c.host, U, V, c.rating, batch)
        got_u, got_i, got_loss, _, _ = E.gcn_loss_grad(c.g, c.tag, step, Ud, Vd)
        assert _same(got_u, Gu) and _same(got_i, Gi), (name, d, step)
        got_loss = float(got_loss.cpu()[0])
        assert abs(got_loss - loss) <= 1e-12 * abs(loss), (got_loss, loss)
        in_csr = bpr.in_batch_csr(c.host, batch)
        idle_u = np.setdiff1d(np.arange(c.n_user), c.host.row_u[in_csr])
        idle_i = np.setdiff1d(np.arange(c.n_item), c.host.col[in_csr])
        assert len(idle_u) and len(idle_i) and _zero_rows(got_u, idle_u) and _zero_rows(got_i, idle_i)


@pytest.mark.parametrize('name,d', CASES, ids=IDS)
def test_bpr_walks_equal_the_contract_at_every_tile_edge(name, d):
    """engine.bpr_loss_grad with the contract's negatives and index at every step: on the device's own w and x, G_u and G_i are
    bpr.walks_ref's bytes and the loss is within 1e-12 relative of lightgcn.fold_256(row_loss); a user without an entry in the step,
    and an item that is neither an entry's item nor its negative there, is +0.0 in every byte."""
    E, c = _engine(), _case(name)
    U, V = _tables(c, d)
    Ud, Vd = _dev(U), _dev(V)
    for step in range(STEPS):
        in_csr = bpr.in_batch_csr(c.host, c.order[step * c.batch:(step + 1) * c.batch])
        got_u, got_i, loss, w, x, _, _ = E.bpr_loss_grad(c.g, c.tag, step, Ud, Vd, c.neg_d, c.index_d)
        Gu, Gi, row_loss = bpr.walks_ref(c.host, c.index, U, V, c.neg, _np(w), _np(x), in_csr)
        assert _same(got_u, Gu) and _same(got_i, Gi), (name, d, step)
        got_loss, want_loss = float(loss.cpu()[0]), lightgcn.fold_256(row_loss)
        assert abs(got_loss - want_loss) <= 1e-12 * want_loss, (got_loss, want_loss)
        idle_u = np.setdiff1d(np.arange(c.n_user), c.host.row_u[in_csr])
        idle_i = np.setdiff1d(np.arange(c.n_item), np.concatenate([c.host.col[in_csr], c.neg[in_csr]]))
        assert len(idle_u) and _zero_rows(got_u, idle_u) and _zero_rows(got_i, idle_i)
        assert len(idle_i) or name == 'T'                              # (67 items: every one is somebody's negative in a step)


@pytest.mark.parametrize('name,d', CASES, ids=IDS)
def test_influence_walks_equal_the_contract_at_every_tile_edge(name, d):
    """engine.inf_matvec ('full' with damping 0.07, and 'gn') and engine.inf_grad, with every row active and with the long row and a
    row of 33 entries frozen: influence.matvec_ref's / grad_ref's bytes, frozen rows +0.0 in every byte."""
    E, c = _engine(), _case(name)
    U, V = _tables(c, d)
    Ud, Vd = _dev(U), _dev(V)
    rs = np.random.RandomState(7400 + d)
    P, Q = rs.standard_normal(U.shape), rs.standard_normal(V.shape)
    Pd, Qd = _dev(P), _dev(Q)
    side, frozen = c.frozen
    for active in (None, c.active):
        got = [E.inf_grad(c.g, Ud, Vd, L2, active)]
        want = [influence.grad_ref(c.host, U, V, c.r, L2, active)]
        for curvature, damping in (('full', 0.07), ('gn', 0.0)):
            got.append(E.inf_matvec(c.g, Ud, Vd, Pd, Qd, L2, damping, curvature, active))
            want.append(influence.matvec_ref(c.host, U, V, c.r, P, Q, L2, damping, curvature, active))
        for k, ((gU, gV), (wU, wV)) in enumerate(zip(got, want)):
            assert _same(gU, wU) and _same(gV, wV), (name, d, active is None, k)
            if active is not None:
                assert _zero_rows((gU, gV)[side], frozen)
