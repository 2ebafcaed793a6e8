"""grouped_select (ops/csrc/grouped_select.hip) against a per-group sorted()
reference, and the engine sites that use it (`sail.exec.percentile_select`)."""
import math

import numpy as np
import pytest
import torch

import sail_amd
import sail_amd.engine.aggregates as A
from sail_amd.engine import types as T
from sail_amd.engine.column import Table
from sail_amd.ops import kernels

gpu = pytest.mark.gpu
TILE = 256                 # rows per tile = threads per workgroup
CHUNK = 16 * TILE          # the fewest rows a workgroup walks
SIZES = [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 3 * CHUNK + 5]
# (ng, gid dtype); None: no gid. 32 groups is the last LDS histogram, 33 the first global one
GROUPS = [(1, None), (1, torch.int64), (7, torch.int32), (32, torch.int64), (33, torch.int32),
          (1000, torch.int64)]
QS = [0, 0.25, 0.5, 0.9, 1]
KINDS = ["equal", "low_byte", "top_byte", "random8", "sorted", "half_in_one"]
# one value per top byte or sign, the ends of the number line included
EDGES = [math.inf, -math.inf, 0.0, -0.0, 5e-324, -5e-324, 2.5e-310] + \
        [s * 2.0 ** e for s in (1, -1) for e in (-1000, -48, -16, 0, 16, 48, 1000)]


@pytest.fixture(scope="module")
def ext():
    return kernels.require()


def _rows(kind, n, ng):
    """(vals float64, gid int64) on the host."""
    i = torch.arange(n)
    gid = i * 13 % ng
    if kind == "equal":
        return torch.full((n,), 7.5, dtype=torch.float64), gid
    if kind == "low_byte":   # the passes 0..6 all tie
        return (torch.tensor(1.5, dtype=torch.float64).view(torch.int64) + i * 37 % 256) \
            .view(torch.float64), gid
    if kind == "top_byte":
        return torch.tensor(EDGES, dtype=torch.float64)[i * 7 % len(EDGES)], gid
    g = torch.Generator().manual_seed(n + ng)
    v = torch.randint(0, max(n // 8, 1), (n,), generator=g).double() * 0.37 - 3.0   # 8 copies
    if kind == "sorted":
        v = v.sort().values
    if kind == "half_in_one":
        gid = torch.where(i % 2 == 0, torch.zeros_like(gid), gid)
    return v, gid


def _check(ext, vals, gid, mask, ng, gid_dtype):
    """lo, hi, count, row and flag of every q and mode against sorted(), exactly
    (as text: -0.0 and nan compare by what they are)."""
    keep = [1] * len(vals) if mask is None else mask.tolist()
    groups = [[] for _ in range(ng)]
    for i, (v, g, m) in enumerate(zip(vals.tolist(), gid.tolist(), keep)):
        if m:   # NaNs last, -0.0 before 0.0, equal values by row
            groups[g].append((v != v, 0.0 if v != v else v, v != v or math.copysign(1, v), i))
    first = []  # per group and sorted position: the smallest row of that value
    for s in groups:
        s.sort()
        f = [e[3] for e in s]
        for k in range(1, len(s)):
            if s[k][:3] == s[k - 1][:3]:
                f[k] = f[k - 1]
        first.append(f)
    value = lambda e: math.nan if e[0] else e[1]
    dv, dm = vals.cuda(), None if mask is None else mask.cuda()
    dg = None if gid_dtype is None else gid.to(gid_dtype).cuda()
    for q in QS:
        for mode in (0, 1, 2):
            lo, hi, cnt, row, flag = ([0.0] * ng, [0.0] * ng, [0] * ng, [-1] * ng, [0] * ng)
            for j, s in enumerate(groups):
                if not s:
                    continue
                last = len(s) - 1
                k = math.floor(q * last) if mode == 0 else \
                    max(0, min(last, math.ceil(q * len(s)) - 1))
                k = last - k if mode == 2 else k
                lo[j], hi[j] = value(s[k]), value(s[min(k + 1, last)])
                cnt[j], row[j], flag[j] = len(s), first[j][k], int(s[-1][0])
            lo_hi, meta = ext.grouped_select(dv, dg, dm, ng, q, mode)
            assert lo_hi.dtype == torch.float64 and meta.dtype == torch.int64
            assert str(lo_hi.tolist()) == str([lo, hi]), (q, mode)
            assert meta.tolist() == [cnt, row, flag], (q, mode)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_value_structure(ext, n, kind):
    for ng, gid_dtype in GROUPS:   # groups above n receive no row
        vals, gid = _rows(kind, n, ng)
        _check(ext, vals, gid, None, ng, gid_dtype)


@gpu
@pytest.mark.parametrize("ng,gid_dtype", GROUPS)
@pytest.mark.parametrize("mask", ["zero", "random_bool", "random_uint8"])
def test_masks(ext, mask, ng, gid_dtype):
    n = 3 * CHUNK + 5
    vals, gid = _rows("random8", n, ng)
    m = torch.rand(n, generator=torch.Generator().manual_seed(5)) < 0.5
    m = {"zero": torch.zeros(n, dtype=torch.bool), "random_bool": m,
         "random_uint8": m.to(torch.uint8) * 3}[mask]   # non-zero keeps a row
    _check(ext, vals, gid, m, ng, gid_dtype)


@gpu
@pytest.mark.parametrize("ng,gid_dtype", GROUPS)
def test_one_nan_flags_its_group_only(ext, ng, gid_dtype):
    vals, gid = _rows("random8", 3 * TILE + 5, ng)
    vals[300] = -math.nan   # a negative NaN still sorts last
    _check(ext, vals, gid, None, ng, gid_dtype)


@gpu
def test_refused_inputs(ext):
    v = torch.arange(512, dtype=torch.float64, device="cuda")
    g = torch.zeros(512, dtype=torch.int64, device="cuda")
    for vals, gid, mask, ng in [(v.float(), None, None, 1), (v[::2], None, None, 1),
                                (v, g[:100], None, 2), (v, g[::2], None, 2), (v, None, None, 2),
                                (v, g.double(), None, 2), (v, g, g, 2), (v, g, None, 0)]:
        with pytest.raises(RuntimeError):
            ext.grouped_select(vals, gid, mask, ng, 0.5, 0)
    for q, mode in [(1.5, 0), (-0.1, 1), (0.5, 3)]:
        with pytest.raises(RuntimeError):
            ext.grouped_select(v, None, None, 1, q, mode)


ROWS = 3000
SHAPES = {"global": ("", "", ""), "grouped": ("k, ", "", " GROUP BY k ORDER BY k"),
          "filter": ("k, ", " FILTER (WHERE b)", " GROUP BY k ORDER BY k")}


@pytest.fixture(scope="module")
def sessions():
    r = torch.randint(0, 1 << 30, (4, ROWS), generator=torch.Generator().manual_seed(1)).tolist()
    data = {"k": [x % 13 for x in r[0]],
            "a": [None if x % 5 == 0 else x % 101 - 50 for x in r[1]],   # integer, nullable
            "x": [float(x % 64 - 32) for x in r[2]], "b": [x % 3 != 0 for x in r[3]],
            "d": [(x % 37) / 4.0 for x in r[3]]}
    schema = {"k": T.I64, "a": T.I64, "x": T.F64, "b": T.BOOL, "d": T.DecimalType(12, 2)}
    tbl = Table.from_pydict(data, schema, device="cpu")
    dev = sail_amd.SessionContext(device="cuda")
    dev.catalog.register_table("t", tbl.to("cuda"))
    return data, dev


@gpu
@pytest.mark.parametrize("q", [0, 0.25, 0.5, 0.75, 1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_engine_select_sort_host_and_numpy_agree(sessions, monkeypatch, shape, q):
    data, dev = sessions
    keys, flt, tail = SHAPES[shape]
    sql = (f"SELECT {keys}median(a){flt}, percentile(x, {q}){flt}, "
           f"percentile_cont({q}) WITHIN GROUP (ORDER BY d){flt}, "
           f"percentile_cont({q}) WITHIN GROUP (ORDER BY a DESC){flt}, "
           f"percentile_disc({q}) WITHIN GROUP (ORDER BY a){flt}, "
           f"percentile_disc({q}) WITHIN GROUP (ORDER BY x DESC){flt}, "
           f"percentile_disc({q}) WITHIN GROUP (ORDER BY d){flt} FROM t{tail}")
    want = []
    for k in sorted(set(data["k"])) if keys else [None]:
        col = {c: sorted(v for v, kk, b in zip(data[c], data["k"], data["b"])
                         if v is not None and k in (None, kk) and (b or not flt)) for c in "axd"}
        disc = lambda s: s[max(0, min(len(s) - 1, math.ceil(q * len(s)) - 1))]
        want.append(((k,) if keys else ()) + (
            np.percentile(col["a"], 50), np.percentile(col["x"], q * 100),
            np.percentile(col["d"], q * 100), np.percentile(col["a"], (1 - q) * 100),
            disc(col["a"]), disc(col["x"][::-1]), disc(col["d"])))
    for switch, budget, path in (("on", A.PERCENTILE_HIST_BUDGET, "select"), ("on", 0, "sort"),
                                 ("off", 0, "host")):
        monkeypatch.setenv("SAIL_EXEC_PERCENTILE_SELECT", switch)
        monkeypatch.setattr(A, "PERCENTILE_HIST_BUDGET", budget)
        A.LAST_PERCENTILE_PATH = None
        assert dev.sql(sql).collect() == want, path
        assert A.LAST_PERCENTILE_PATH == path


def test_switch_default_and_environment(monkeypatch):
    from sail_amd.config import DEFAULTS

    monkeypatch.delenv("SAIL_EXEC_PERCENTILE_SELECT", raising=False)
    assert DEFAULTS["sail.exec.percentile_select"] == "on" and A.percentile_select_enabled()
    monkeypatch.setenv("SAIL_EXEC_PERCENTILE_SELECT", "off")
    assert not A.percentile_select_enabled()
