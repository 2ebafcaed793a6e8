"""distinct_acc (ops/csrc/distinct_agg.hip) against Python sets, and the engine
sites that use it (`sail.exec.distinct_hash`)."""
import pytest
import torch

import sail_amd
import sail_amd.engine.aggregates as A
from sail_amd.engine import types as T
from sail_amd.engine.column import Column, Table
from sail_amd.ops import kernels

gpu = pytest.mark.gpu
TILE = 256                 # rows per tile = threads per workgroup
CHUNK = 16 * TILE          # the fewest rows a workgroup walks
LDS_GROUPS = 1024          # LDS counters up to here, global atomics above
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
EMPTY_MARKER = -(1 << 63) + 1   # 0x8000000000000001, the ng == 1 table's empty slot
SIZES = [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 3 * CHUNK + 5]
KINDS = ["same", "distinct", "value_across_groups", "values_in_group", "sorted", "random8"]
# (ng, gid dtype); None: no gid, the key-table variant
GROUPS = [(1, None), (1, torch.int64), (7, torch.int32), (LDS_GROUPS, torch.int64),
          (LDS_GROUPS + 1, torch.int32)]


@pytest.fixture(scope="module")
def ext():
    return kernels.require()


def _pairs(kind, n, ng):
    i = torch.arange(n)
    if kind == "same":
        return torch.full((n,), ng - 1), torch.full((n,), 7)
    if kind == "distinct":
        return i % ng, i - n // 2
    if kind == "value_across_groups":
        return i % ng, torch.full((n,), 5)
    if kind == "values_in_group":
        return torch.full((n,), ng // 2), i * 3
    g = torch.Generator().manual_seed(n + ng)
    idx = torch.randint(0, max(n // 8, 1), (n,), generator=g)   # about 8 copies of each
    if kind == "sorted":
        idx = idx.sort().values
    return idx % ng, idx * 2654435761 - (1 << 40)


def _check(ext, gid, keys, mask, ng, gid_dtype, **kw):
    """Every shipped flag combination (variant 0..3) against sets, exactly."""
    sets = [set() for _ in range(ng)]
    keep = [1] * len(keys) if mask is None else mask.tolist()
    for g, k, m in zip(gid.tolist(), keys.tolist(), keep):
        if m:
            sets[g].add(k)
    cnt = [len(s) for s in sets]
    tot = [(sum(s) + (1 << 63)) % (1 << 64) - (1 << 63) for s in sets]
    dg = None if gid_dtype is None else gid.to(gid_dtype).cuda()
    dm = None if mask is None else mask.cuda()
    for variant in range(4):
        out = ext.distinct_acc(dg, keys.cuda(), dm, ng, True, variant=variant, **kw)
        assert out.dtype == torch.int64 and out.tolist() == [cnt, tot], (variant, kw)
    out = ext.distinct_acc(dg, keys.cuda(), dm, ng, False, **kw)
    assert out.tolist() == [cnt, [0] * ng]


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_pair_structure(ext, n, kind):
    for ng, gid_dtype in GROUPS:   # groups above n receive no row
        gid, keys = _pairs(kind, n, ng)
        _check(ext, gid, keys, None, ng, gid_dtype)


@gpu
@pytest.mark.parametrize("ng,gid_dtype", GROUPS)
@pytest.mark.parametrize("mask", ["zero", "random_bool", "random_uint8"])
def test_masks(ext, mask, ng, gid_dtype):
    n = 3 * CHUNK + 5
    gid, keys = _pairs("random8", n, ng)
    m = torch.rand(n, generator=torch.Generator().manual_seed(5)) < 0.5
    m = {"zero": torch.zeros(n, dtype=torch.bool), "random_bool": m,
         "random_uint8": m.to(torch.uint8) * 3}[mask]   # non-zero keeps a row
    _check(ext, gid, keys, m, ng, gid_dtype)


@gpu
@pytest.mark.parametrize("ng,gid_dtype", GROUPS)
def test_edge_keys_once_each_and_wrapping_sum(ext, ng, gid_dtype):
    keys = torch.tensor([I64_MIN, I64_MIN + 1, -1, 0, I64_MAX, EMPTY_MARKER, I64_MAX - 1] * 40)
    gid = (torch.arange(keys.numel()) // 7) % min(ng, 3)
    _check(ext, gid, keys, None, ng, gid_dtype)


@gpu
@pytest.mark.parametrize("ng,gid_dtype", GROUPS)
def test_nearly_full_table(ext, ng, gid_dtype):
    gid, keys = _pairs("distinct", 1000, ng)
    _check(ext, gid, keys, None, ng, gid_dtype, table_slots=1024)
    for slots in (512, 1000, 1536):   # <= n, or no power of two
        with pytest.raises(RuntimeError):
            ext.distinct_acc(None, keys.cuda(), None, 1, True, table_slots=slots)


ROWS = 3000
QUERIES = {
    "grouped": "SELECT k, count(DISTINCT v), sum(DISTINCT v), avg(DISTINCT v) FROM t "
               "GROUP BY k ORDER BY k",
    "global": "SELECT count(DISTINCT v), sum(DISTINCT v), avg(DISTINCT v) FROM t",
    "filter": "SELECT k, count(DISTINCT v) FILTER (WHERE b), sum(DISTINCT v) FILTER (WHERE b), "
              "avg(DISTINCT v) FILTER (WHERE b) FROM t GROUP BY k ORDER BY k",
    "filter_global": "SELECT count(DISTINCT v) FILTER (WHERE b), "
                     "avg(DISTINCT v) FILTER (WHERE b) FROM t",
    "string": "SELECT k, count(DISTINCT s) FROM t GROUP BY k ORDER BY k",
    "decimal": "SELECT k, count(DISTINCT d), sum(DISTINCT d), avg(DISTINCT d) FROM t "
               "GROUP BY k ORDER BY k",
    "approx": "SELECT k, approx_count_distinct(v) FROM t GROUP BY k ORDER BY k",
    "q10": "SELECT k, sum(w), count(*), avg(w), count(DISTINCT v) FROM t GROUP BY k ORDER BY k",
}


@pytest.fixture(scope="module")
def sessions():
    r = torch.randint(0, 1 << 30, (4, ROWS), generator=torch.Generator().manual_seed(1)).tolist()
    data = {"k": [x % 13 for x in r[0]],
            "v": [None if x % 5 == 0 else x % 101 - 50 for x in r[1]],
            "w": [x % 1000 for x in r[2]], "b": [x % 3 != 0 for x in r[3]],
            "s": [f"name{x % 40}" for x in r[2]], "d": [(x % 37) / 4.0 for x in r[3]]}
    schema = {"k": T.I64, "v": T.I64, "w": T.I64, "b": T.BOOL, "s": T.STRING,
              "d": T.DecimalType(12, 2)}
    tbl = Table.from_pydict(data, schema, device="cpu")
    cpu, dev = sail_amd.SessionContext(device="cpu"), sail_amd.SessionContext(device="cuda")
    cpu.catalog.register_table("t", tbl)
    dev.catalog.register_table("t", tbl.to("cuda"))
    return cpu, dev


@gpu
@pytest.mark.parametrize("name", list(QUERIES))
def test_engine_hash_and_sort_agree_with_the_cpu(sessions, monkeypatch, name):
    cpu, dev = sessions
    fused = []
    real = A.fused_agg_batch
    monkeypatch.setattr(A, "fused_agg_batch", lambda *a: fused.append(real(*a)) or fused[-1])
    want = cpu.sql(QUERIES[name]).collect()
    assert len(want) == (1 if "global" in name else 13)
    for switch, path in (("on", "hash"), ("off", "sort")):
        monkeypatch.setenv("SAIL_EXEC_DISTINCT_HASH", switch)
        A.LAST_DISTINCT_PATH = None
        assert dev.sql(QUERIES[name]).collect() == want
        assert A.LAST_DISTINCT_PATH == path
        if name == "q10":   # the plain aggregates stay on the fused launches
            assert (fused[-1] is not None) == (switch == "on")


def test_switch_default_and_cpu_columns_sort(monkeypatch):
    from sail_amd.config import DEFAULTS

    monkeypatch.delenv("SAIL_EXEC_DISTINCT_HASH", raising=False)
    assert DEFAULTS["sail.exec.distinct_hash"] == "on" and A.distinct_hash_enabled()
    monkeypatch.setenv("SAIL_EXEC_DISTINCT_HASH", "off")
    assert not A.distinct_hash_enabled()
    monkeypatch.setenv("SAIL_EXEC_DISTINCT_HASH", "on")
    before = dict(A.DISTINCT_PATHS)
    col = Column.from_values([4, 4, 9, None, 9, 2], T.I64)
    out = A.agg_eval("count", [col], torch.tensor([0, 0, 0, 1, 1, 1]), 2, distinct=True)
    assert out.data.tolist() == [2, 2] and A.LAST_DISTINCT_PATH == "sort"
    assert A.DISTINCT_PATHS == {"hash": before["hash"], "sort": before["sort"] + 1}
