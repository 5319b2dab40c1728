"""The two host-only decisions of TrainJob setup, stated without a device: which step kernel a job runs (engine.touch_plan) and where a
shard's tables live in the job's two device pools (engine.shard_regions)."""
from types import SimpleNamespace

import pytest

from ultrare_amd import engine

BIG = (256 << 20) + 1            # live rows just beyond the Infinity Cache (the comparison is strict) ...
SMALL = 256 << 20                # ... and just inside it

# (touch, live_bytes, final_only, epoch_reads, steps, d, whatever differs from: empty environment, lazy_rows=True, snapshots=False, batch=3000, mode)
PLAN_ROWS = [
    (None, SMALL, True, False, 27, 64, {}, 0),
    (None, BIG, False, False, 27, 64, {}, 0),
    (None, BIG, True, False, 27, 64, {}, 3),
    (None, BIG, True, False, 27, 128, {}, 2),
    (None, BIG, True, False, 27, 128, dict(snapshots=True), 1),
    (None, BIG, False, True, 27, 128, {}, 1),
    (None, BIG, False, True, 27, 64, {}, 3),
    (None, BIG, True, False, 27, 64, dict(URE_TOUCH_INDEX='0'), 2),
    (None, BIG, True, False, 27, 16, dict(URE_TOUCH='1'), 2),
    (None, BIG, True, False, 27, 64, dict(URE_TOUCH='0'), 0),
    (True, 0, False, False, 27, 16, {}, 1),
    (True, 0, True, False, 63, 16, {}, 2),
    (True, 0, True, False, 64, 16, {}, 3),
    (True, 0, True, False, 27, 16, dict(snapshots='compact'), 2),
    (True, 0, True, False, 27, 16, dict(snapshots='full'), 1),
    (True, 0, True, False, 27, 16, dict(URE_TOUCH_AHEAD='0'), 1),
    (True, 0, True, False, 27, 16, dict(URE_TOUCH_INDEX='2'), 3),
    (True, 0, False, False, 74, 16, {}, 3),
    (True, 0, False, False, 74, 16, dict(URE_TOUCH_INDEX='0'), 1),
    (True, 0, False, False, 1008, 16, {}, 3),
    (True, 0, False, False, 1009, 16, {}, 1),
    (True, 0, False, False, 64, 16, dict(batch=200001), 1),
    (True, 0, False, False, 32000, 16, {}, 1),
    (True, 0, False, False, 32001, 16, {}, 0),
    (True, 0, False, False, 27, 16, dict(lazy_rows=False), 0),
    ('index', 0, True, False, 27, 16, {}, 3),
    ('index', 0, False, False, 1009, 16, {}, 1),
    (False, BIG, True, False, 27, 64, dict(URE_TOUCH='1'), 0),
]


def _plan(touch, live, final_only, epoch_reads, steps, d, extra, env=None):
    args = dict(lazy_rows=True, snapshots=False, batch=3000)
    args.update({k: v for k, v in extra.items() if not k.startswith('URE_')})
    return engine.touch_plan(steps, d, args['batch'], live, args['lazy_rows'], args['snapshots'], touch, final_only, epoch_reads, env)


@pytest.mark.parametrize('row', PLAN_ROWS, ids=lambda r: '-'.join(str(x) for x in r[:6]) + ''.join(f'-{k}={v}' for k, v in r[6].items()))
def test_touch_plan_table(row):
    *args, extra, mode = row
    env = {k: v for k, v in extra.items() if k.startswith('URE_')}
    assert _plan(*args, extra, env=env) == mode
    if args[0] is not None or args[2]:           # epoch_reads does not enter: the caller said touch, or reads after the last epoch only
        assert _plan(*args[:3], True, *args[4:], extra, env=env) == mode


def test_touch_plan_reads_the_environment_when_called(monkeypatch):
    row = (None, BIG, True, False, 27, 64, {})
    for name in ('URE_TOUCH', 'URE_TOUCH_INDEX', 'URE_TOUCH_AHEAD'):
        monkeypatch.delenv(name, raising=False)
    assert _plan(*row) == 3
    monkeypatch.setenv('URE_TOUCH_INDEX', '0')
    assert _plan(*row) == 2
    monkeypatch.setenv('URE_TOUCH_AHEAD', '0')
    assert _plan(*row) == 1
    monkeypatch.setenv('URE_TOUCH', '0')
    assert _plan(*row) == 0
    assert _plan(*row, env={}) == 3              # a given environment replaces the process's


def test_float_pool_regions():
    pool, snap, end, snap_end = engine.shard_regions(5, 6, 4, 8, 4, True, False)
    assert list(pool) == ['U', 'V', 'mU', 'mV', 'sse', 'U0', 'V0']
    assert [pool[n][0] for n in pool] == [0, 128, 256, 320, 384, 448, 512]
    assert [pool[n][1:] for n in pool] == [(80, (2, 5, 8)), (96, (2, 6, 8)), (40, (5, 8)), (48, (6, 8)), (20, (4, 5)), (40, (5, 8)), (48, (6, 8))]
    assert (end, snap, snap_end) == (576, {}, 0)
    # a second identical shard: the same regions, 576 floats on
    pool2, _, end2, _ = engine.shard_regions(5, 6, 4, 8, 4, True, False, end, 0)
    assert pool2 == {n: (576 + at, size, shape) for n, (at, size, shape) in pool.items()} and end2 == 2 * 576


def test_float_pool_regions_without_lazy_rows():
    pool, _, end, _ = engine.shard_regions(5, 6, 4, 8, 4, False, False)
    assert pool['U0'][1] == 0 and pool['V0'][1] == 0
    assert [pool[n][0] for n in ('U', 'V', 'mU', 'mV', 'sse')] == [0, 128, 256, 320, 384] and end == 448
    assert engine.shard_regions(5, 6, 4, 8, 4, False, False, end, 0)[0]['U'][0] == 448


@pytest.mark.parametrize('mode, want', [
    ('full', {'snapU': (0, 4 * 5 * 8, (4, 5, 8)), 'snapV': (4 * 5 * 8, 4 * 6 * 8, (4, 6, 8))}),
    ('compact', {'snap': (0, 4 * 3 * 8, (4, 3, 8))}),
    (False, {}),
])
def test_snapshot_pool_regions(mode, want):
    n_user, n_item, n_active, d, epochs = 5, 6, 3, 8, 4
    _, snap, _, snap_end = engine.shard_regions(n_user, n_item, n_active, d, epochs, True, mode)
    assert snap == want
    used = sum(size for _, size, _ in snap.values())
    assert snap_end == (used + 63) // 64 * 64 and snap_end % 64 == 0            # (352 -> 384 floats, 96 -> 128, 0)
    # the next shard's snapshots start on the rounded boundary
    _, snap2, _, snap_end2 = engine.shard_regions(n_user, n_item, n_active, d, epochs, True, mode, 576, snap_end)
    assert snap2 == {n: (snap_end + at, size, shape) for n, (at, size, shape) in want.items()} and snap_end2 == 2 * snap_end
    if mode:
        shards = [SimpleNamespace(n_user=n_user, n_item=n_item, n_active=n_active)] * 2
        assert engine.TrainJob.snapshot_bytes(shards, epochs, d, mode) == 2 * 4 * used
