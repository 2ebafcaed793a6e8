"""grouped_acc_global against exact numpy, and the engine sites that use it."""
import numpy as np
import pytest
import torch

import sail_amd
import sail_amd.engine.aggregates as agg_mod
from sail_amd.engine import types as T
from sail_amd.engine.column import Table
from sail_amd.ops import kernels

pytestmark = pytest.mark.gpu

SUM, FSUM, COUNT, MIN, MAX = 0, 1, 2, 3, 4
SLOTS = 1024  # cache slots of a launch of up to 4 columns (512 above)

# (op, column dtype); float columns hold small integers: op 1 is exact too
ALL_OPS = [(SUM, np.int32), (FSUM, np.float32), (COUNT, None), (MIN, np.int16),
           (MAX, np.int64)]
ONE = [(FSUM, np.float64)]
TEN = [(SUM, np.int64), (FSUM, np.int32), (COUNT, None), (MIN, np.int8), (MAX, np.uint8),
       (SUM, np.bool_), (FSUM, np.float64), (MIN, np.int64), (MAX, np.int32), (SUM, np.int16)]


@pytest.fixture(scope="module")
def ext():
    return kernels.require()


def _gids(rng, kind, n, G):
    if kind == "random":
        return rng.integers(0, G, n)
    if kind == "ascending":
        return np.sort(rng.integers(0, G, n))
    if kind.startswith("runs"):          # runs<len>@<offset of the first run>
        length, start = map(int, kind[4:].split("@"))
        return ((np.arange(n) + length - start) // length) % G
    if kind == "last":
        return np.full(n, G - 1)
    if kind == "third":
        return rng.integers(0, (G + 2) // 3, n) * 3
    if kind == "hot":                    # one group holds about 90 % of the rows
        return np.where(rng.random(n) < 0.9, 7, rng.integers(0, G, n))
    assert kind == "collide"             # two hot groups of one cache slot
    return np.where(np.arange(n) % 2 == 0, 5, 5 + SLOTS)


def _check(ext, gid, mask, specs, G, gid_dtype, seed=0):
    """Random columns per `specs`; every cell against numpy's at-reductions."""
    rng = np.random.default_rng(seed)
    n = len(gid)
    live = (gid >= 0) & (gid < G) & (np.ones(n, bool) if mask is None else mask.astype(bool))
    vals, want = [], []
    for op, dt in specs:
        if dt is None:
            col = np.ones(n, np.int64)
        elif dt == np.bool_:
            col = rng.random(n) < 0.4
        elif np.issubdtype(dt, np.floating):
            col = rng.integers(-(1 << 20), 1 << 20, n).astype(dt)
        else:
            info = np.iinfo(dt)
            col = rng.integers(max(info.min, -(1 << 40)), min(info.max, 1 << 40), n).astype(dt)
        vals.append(None if dt is None else torch.from_numpy(col).cuda())
        init = {MIN: np.iinfo(np.int64).max, MAX: np.iinfo(np.int64).min}.get(op, 0)
        acc = np.full(G, init, np.float64 if op == FSUM else np.int64)
        at = {MIN: np.minimum.at, MAX: np.maximum.at}.get(op, np.add.at)
        at(acc, gid[live], col[live].astype(acc.dtype))
        want.append(acc.view(np.int64))
    out = ext.grouped_acc_global(torch.from_numpy(gid.astype(gid_dtype)).cuda(),
                                 None if mask is None else torch.from_numpy(mask).cuda(),
                                 vals, [op for op, _ in specs], G)
    assert tuple(out.shape) == (len(specs), G) and out.dtype == torch.int64
    got = out.cpu().numpy()
    for c, w in enumerate(want):
        bad = np.flatnonzero(got[c] != w)
        assert bad.size == 0, (c, specs[c], bad[:5], got[c][bad[:5]], w[bad[:5]])


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 769, 3 * 4096 + 1]
KINDS = ["random", "ascending", "runs64@0", "runs64@1", "runs65@0", "runs65@1",
         "runs128@0", "runs128@1", "last", "third", "hot", "collide"]


@pytest.mark.parametrize("gid_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("G", [4097, 5000, 70_001])
def test_sizes_patterns_and_masks(ext, G, gid_dtype):
    """Each size and each pattern with live rows, unmasked and under a random
    mask (a masked row must not glue its neighbours' runs); all five ops."""
    rng = np.random.default_rng(G)
    rand = [lambda n: rng.random(n) < 0.6, lambda n: (rng.random(n) < 0.6).astype(np.uint8)]
    cases = [("runs64@0", n) for n in SIZES] + [("random", n) for n in SIZES] \
        + [(kind, 20_001) for kind in KINDS]
    for j, (kind, n) in enumerate(cases):
        gid = _gids(rng, kind, n, G)
        _check(ext, gid, None, ALL_OPS, G, gid_dtype, seed=j)
        _check(ext, gid, rand[j % 2](n), ALL_OPS, G, gid_dtype, seed=j)
    _check(ext, gid, np.zeros(len(gid), bool), ALL_OPS, G, gid_dtype)   # every row masked out


@pytest.mark.parametrize("specs", [ONE, TEN], ids=["1col", "10col"])
@pytest.mark.parametrize("kind", ["random", "ascending", "hot", "collide"])
def test_one_and_ten_columns(ext, specs, kind):
    rng = np.random.default_rng(len(specs))
    _check(ext, _gids(rng, kind, 20_001, 5000), rng.random(20_001) < 0.7, specs, 5000, np.int64)


def test_capped_grid_loops_over_tiles(ext):
    # more rows than 2048 workgroups of 16 tiles: a workgroup's chunk grows
    gid = _gids(np.random.default_rng(9), "hot", 2048 * 4096 * 2 + 257, 70_001)
    _check(ext, gid, None, [(SUM, np.int32), (COUNT, None)], 70_001, np.int32)


@pytest.mark.parametrize("kind", ["random", "last"])
def test_int64_sums_wrap(ext, kind):
    """Values near 2^62, in one run and in one cache slot: sums wrap modulo 2^64."""
    G, n = 5000, 512
    gid = np.full(n, 11) if kind == "last" else np.arange(n) % 8
    col = (np.int64(1) << 62) - np.arange(n, dtype=np.int64)
    want = np.zeros(G, np.uint64)
    np.add.at(want, gid, col.astype(np.uint64))
    out = ext.grouped_acc_global(torch.from_numpy(gid).cuda(), None,
                                 [torch.from_numpy(col).cuda()], [SUM], G)
    assert np.array_equal(out.cpu().numpy()[0], want.view(np.int64))


def test_out_of_range_gid_is_dropped(ext):
    G = 4097
    gid = np.random.default_rng(3).integers(0, G, 1000)
    gid[[0, 63, 64, 500]] = [-1, G, -1, G]
    for dt in (np.int32, np.int64):
        _check(ext, gid, None, ALL_OPS, G, dt)


def test_refusals(ext):
    gid = torch.zeros(64, dtype=torch.int64).cuda()
    v = torch.ones(64, dtype=torch.int64).cuda()
    f = torch.ones(64, dtype=torch.float64).cuda()
    for args in ([[v], [SUM], 0], [[v], [SUM], 1 << 31], [[v] * 11, [SUM] * 11, 5000],
                 [[f], [SUM], 5000], [[f], [MIN], 5000], [[f], [MAX], 5000],
                 [[v[:63]], [SUM], 5000]):
        with pytest.raises(RuntimeError):
            ext.grouped_acc_global(gid, None, *args)


@pytest.fixture(scope="module")
def sessions():
    rng = np.random.default_rng(50)
    n = 12_000
    data = {"id": list(range(n)),
            "a": rng.integers(0, 90, n).tolist(), "b": rng.integers(-40, 40, n).tolist(),
            "v": rng.integers(-(1 << 40), 1 << 40, n).tolist(),
            "d": (rng.integers(-(1 << 20), 1 << 20, n) / 4.0).tolist(),
            "bo": (rng.random(n) < 0.5).tolist(),
            "nl": [None if r < 0.3 else int(x) for r, x in
                   zip(rng.random(n), rng.integers(-1000, 1000, n))]}
    schema = {"id": T.I64, "a": T.I64, "b": T.I64, "v": T.I64, "d": T.F64, "bo": T.BOOL,
              "nl": T.I64}
    tbl = Table.from_pydict(data, schema, device="cpu")
    cpu, dev = sail_amd.SessionContext(device="cpu"), sail_amd.SessionContext(device="cuda")
    cpu.catalog.register_table("t", tbl)
    dev.catalog.register_table("t", tbl.to("cuda"))
    return cpu, dev


def test_group_by_5000_groups_runs_on_the_kernel(ext, sessions, monkeypatch):
    cpu, dev = sessions
    calls = []
    real = ext.grouped_acc_global
    monkeypatch.setattr(ext, "grouped_acc_global", lambda *a: calls.append(
        (a[0].dtype, int(a[4]), len(a[3]))) or real(*a))
    q = ("SELECT k, sum(v), sum(d), count(*), max(v), min(b), avg(nl), "
         "sum(v) FILTER (WHERE bo) FROM (SELECT id % 5000 AS k, * FROM t) x "
         "GROUP BY k ORDER BY k")
    got = dev.sql(q).collect()
    monkeypatch.undo()
    assert calls and all(c == (torch.int64, 5000, c[2]) and c[2] <= 4 for c in calls), calls
    assert got == cpu.sql(q).collect()


@pytest.mark.parametrize("switch", ["on", "off"])
def test_direct_aggregate_on_and_off(ext, sessions, monkeypatch, switch):
    cpu, dev = sessions   # two dense keys, 90 x 80 slots
    calls = []
    real = ext.grouped_acc_global
    monkeypatch.setattr(ext, "grouped_acc_global",
                        lambda *a: calls.append(int(a[4])) or real(*a))
    monkeypatch.setenv("SAIL_EXEC_AGG_GLOBAL", switch)
    monkeypatch.setattr(agg_mod, "DIRECT_MIN_ROWS", 1000)
    q = ("SELECT a, b, sum(v), avg(d), count(*), count_if(bo), sum(nl), avg(nl), "
         "count(nl), sum(v) FILTER (WHERE bo) FROM t GROUP BY a, b ORDER BY a, b")
    got = dev.sql(q).collect()
    want = cpu.sql(q).collect()   # the same path on the host, through index_add_
    monkeypatch.undo()
    assert len(want) > 4096 and got == want
    assert (len(calls) > 0 and all(g == 90 * 80 for g in calls)) if switch == "on" else not calls
