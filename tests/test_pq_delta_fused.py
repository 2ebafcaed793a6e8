"""pq_delta_values (ops/csrc/parquet_delta.hip): DELTA_BINARY_PACKED pages
to final int64 / int32 values in one pass.

One case table, two backends, the shape of tests/test_pq_kernels.py. A
builder encodes values of its own choosing with tests/pq_encode.py; the
expectation is those values (plus the page's aux, wrapped to the output
width), never the output of a simulator or of a kernel. Every comparison is
exact. Every case runs for int64 and for int32 output, with the first page
at output row 0 and at output row 3 (odd: the int64 destination is then
only 8-byte aligned and the int32 one only 4-byte aligned).

* CPU half: each case through tests/pq_delta_sim.py, which composes the
  simulator's pq_delta_decode and pq_segscan and the cast.
* GPU half (`gpu` mark): the same cases through the HIP extension, compared
  with the expectation and, bit for bit, with the old path (pq_delta_decode,
  pq_segscan, cast) of the same extension on the same buffer.

Sizes: the kernel works in tiles of 2048 deltas per 256-thread workgroup
and stages at most 17 KB of a page at a time; 40,000 values of 41-bit
deltas (about 205 KB) is the case that needs many windows and tiles, 8,200
pages the one that makes the grid stride.

The file-level tests write a parquet file with stock pq.ParquetWriter and
read it through datasource/gpu_parquet.py with SAIL_IO_GPU_DELTA_FUSED on
and off; the cache test checks that a second scan reuses the page table."""
import functools
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from sail_amd.datasource import gpu_parquet as G
from sail_amd.datasource import parquet_io

import pq_delta_sim as S
import pq_encode as E

FIRST_ROWS = (0, 3)


class Case:
    def __init__(self, buf, rows, expected, total):
        self.buf = buf
        self.pages = E.page_table(rows)
        self.expected = expected      # list of python ints, rows [first:]
        self.total = total
        self.first = rows[0][3]


def _rng(seed):
    return np.random.default_rng(seed)


def _from_deltas(first, adj, min_delta=0):
    """Values whose deltas are min_delta + adj[i], wrapping."""
    vals = [int(first)]
    for a in adj:
        vals.append(E.wrap64(vals[-1] + int(min_delta) + int(a)))
    return vals


def _pack(first_row, pages):
    """pages: (values, payload, skew, aux[, n_values]) in output order, back
    to back from `first_row`. n_values defaults to len(values); when larger,
    the extra slots repeat the last value."""
    lay = E.Layout()
    rows, exp, base = [], [], first_row
    for pg in pages:
        vals, payload, skew, aux = pg[:4]
        n = pg[4] if len(pg) > 4 else len(vals)
        off = lay.add(payload, skew)
        assert off % 4 == skew
        rows.append((off, len(payload), n, base, aux, 0))
        page_exp = [E.wrap64(v + aux) for v in vals]
        page_exp += page_exp[-1:] * (n - len(vals))
        assert len(page_exp) == n
        exp += page_exp
        base += n
    return Case(lay.finish(), rows, exp, base)


# -- builders ---------------------------------------------------------------

def _b_bit_widths(first_row):
    """Every width 0-64, one page of 300 values each (two full blocks and a
    third with two used and two empty miniblocks)."""
    rng = _rng(1)
    pages = []
    for bw in range(65):
        top = (1 << bw) - 1
        adj = [int.from_bytes(rng.bytes(8), "little") & top for _ in range(299)]
        adj[::32] = [top] * len(adj[::32])     # every miniblock uses the width
        adj[1::32] = [0] * len(adj[1::32])     # ... above the block's minimum
        # deltas span [-2^(bw-1), 2^(bw-1)): no wrap below width 64, the
        # whole int64 range at 64
        vals = _from_deltas(int(rng.integers(-10**9, 10**9)), adj,
                            min_delta=-(1 << bw >> 1) if bw else 7)
        payload, used = E.delta_binary_packed(vals, forced_bw=bw)
        assert set(used) == {bw}
        pages.append((vals, payload, bw % 4, 0))
    return _pack(first_row, pages)


def _b_page_sizes(first_row):
    rng = _rng(2)
    pages = []
    for k, n in enumerate((1, 2, 32, 33, 128, 129, 130, 257)):
        vals = [int(x) for x in rng.integers(-10**15, 10**15, n)]
        payload, _ = E.delta_binary_packed(vals)
        pages.append((vals, payload, (k + 1) % 4, (-7, 0, 10**12)[k % 3]))
    return _pack(first_row, pages)


def _b_wrap(first_row):
    alt = [E.INT64_MIN, E.INT64_MAX] * 75
    p1, _ = E.delta_binary_packed(alt)
    # deltas INT64_MIN (the block's min_delta), 5 and -3
    vals = [0]
    for i in range(199):
        vals.append(E.wrap64(vals[-1] + (E.INT64_MIN, 5, -3)[i % 3]))
    p2, used = E.delta_binary_packed(vals)
    assert 64 in used
    return _pack(first_row, [(alt, p1, 1, 0), (vals, p2, 3, 1)])


def _b_large_page(first_row):
    rng = _rng(4)
    adj = rng.integers(0, 1 << 41, 39_999)
    vals = np.concatenate([[12345], 12345 + np.cumsum(adj)]).tolist()
    payload, used = E.delta_binary_packed(vals)
    assert min(used) >= 40 and len(payload) > 200_000
    return _pack(first_row, [(vals, payload, 1, 0)])


def _b_source_skew(first_row):
    rng = _rng(5)
    pages = []
    for skew in range(4):
        vals = [int(x) for x in rng.integers(-10**6, 10**6, 70)]
        pages.append((vals, E.delta_binary_packed(vals)[0], skew, 0))
    return _pack(first_row, pages)


def _b_many_pages(first_row):
    v = _rng(6).integers(-10**9, 10**9, (8200, 3)).tolist()
    return _pack(first_row, [(vals, E.delta_binary_packed(vals)[0], p % 4, 0)
                             for p, vals in enumerate(v)])


def _b_geometries(first_row):
    rng = _rng(7)
    pages = []
    # 256/8 has more than four miniblocks per block: the kernel then reads
    # the width bytes one at a time
    for k, (block, mbpb) in enumerate(((256, 4), (128, 1), (256, 4), (128, 1),
                                       (256, 8), (256, 8))):
        n = (700, 700, 65, 129, 700, 33)[k]
        vals = [int(x) for x in rng.integers(-10**10, 10**10, n)]
        payload, _ = E.delta_binary_packed(vals, block=block, mbpb=mbpb)
        pages.append((vals, payload, (k + 2) % 4, 0))
    return _pack(first_row, pages)


def _b_empty_pages(first_row):
    """A, 32 empty pages whose out_row is B's, B, then an empty page with
    out_row == total. The empty pages carry a real header with a first
    value that must not land anywhere."""
    rng = _rng(8)
    a = [int(x) for x in rng.integers(-10**6, 10**6, 45)]
    b = [int(x) for x in rng.integers(-10**6, 10**6, 200)]
    empty = E.delta_header(0, 0x5A5A5A5A)
    pages = [(a, E.delta_binary_packed(a)[0], 1, 0)]
    pages += [([], empty, k % 4, 0) for k in range(32)]
    pages += [(b, E.delta_binary_packed(b)[0], 3, 0), ([], empty, 2, 0)]
    case = _pack(first_row, pages)
    assert case.pages[-1, 3] == case.total and case.pages[1, 3] == \
        case.pages[33, 3]
    return case


def _b_short_count(first_row):
    """The header counts 100 values, the descriptor 130: slots 100-129
    repeat value 99. The page after it starts right behind."""
    rng = _rng(9)
    a = [int(x) for x in rng.integers(-10**6, 10**6, 100)]
    b = [int(x) for x in rng.integers(-10**6, 10**6, 40)]
    return _pack(first_row, [(a, E.delta_binary_packed(a)[0], 1, 4, 130),
                             (b, E.delta_binary_packed(b)[0], 2, 0)])


CASES = [
    ("bit_widths_0_to_64_300_values_each", _b_bit_widths),
    ("page_sizes_1_2_32_33_128_129_130_257", _b_page_sizes),
    ("wrap_int64_min_max_and_min_delta_int64_min", _b_wrap),
    ("large_page_40000_values_41_bit_deltas", _b_large_page),
    ("source_skew_0_to_3_70_values", _b_source_skew),
    ("many_pages_8200_of_3_values", _b_many_pages),
    ("geometries_256_4_128_1_and_256_8", _b_geometries),
    ("empty_pages_32_between_two_and_one_trailing", _b_empty_pages),
    ("short_header_count_100_of_130", _b_short_count),
]
_BUILDERS = dict(CASES)
NAMES = [n for n, _ in CASES]
assert len(_BUILDERS) == len(CASES)
PARAMS = [(n, f, i32) for n in NAMES for f in FIRST_ROWS for i32 in (False, True)]


@functools.lru_cache(maxsize=None)
def _case(name, first_row):
    return _BUILDERS[name](first_row)


@functools.lru_cache(maxsize=None)
def _sim_out(name, first_row):
    """int64 simulator output of a case: computed once, shared."""
    c = _case(name, first_row)
    return S.pq_delta_values(c.buf, c.pages, c.total, False)


def _expected(case, as_int32):
    t = torch.tensor(case.expected, dtype=torch.int64)
    return t.to(torch.int32) if as_int32 else t


def _check(got, case, as_int32, what):
    want = _expected(case, as_int32)
    g = got.cpu()[case.first:]
    assert got.dtype == want.dtype and got.numel() == case.total, what
    if not torch.equal(g, want):
        bad = torch.nonzero(g != want).flatten()[:8].tolist()
        raise AssertionError(f"{what}: mismatches, first at {bad}: got "
                             f"{g[bad].tolist()} want {want[bad].tolist()}")


@pytest.mark.parametrize("name,first_row,as_int32", PARAMS)
def test_sim_case(name, first_row, as_int32):
    out = _sim_out(name, first_row)
    _check(out.to(torch.int32) if as_int32 else out, _case(name, first_row),
           as_int32, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,first_row,as_int32", PARAMS)
def test_gpu_case(name, first_row, as_int32):
    from sail_amd.ops import kernels

    ext = kernels.require()
    case = _case(name, first_row)
    buf, pages = case.buf.to("cuda:0"), case.pages.to("cuda:0")
    got = ext.pq_delta_values(buf, pages, case.total, as_int32)
    _check(got, case, as_int32, name)
    old, _ = ext.pq_delta_decode(buf, pages, case.total)
    ext.pq_segscan(old, pages)
    if as_int32:
        old = old.to(torch.int32)
    assert torch.equal(got[case.first:], old[case.first:]), name


@pytest.mark.gpu
def test_gpu_wrapper_checks_its_arguments():
    from sail_amd.ops import kernels

    fn = kernels.require().pq_delta_values
    case = _case("source_skew_0_to_3_70_values", 0)
    buf, pages = case.buf.to("cuda:0"), case.pages.to("cuda:0")
    with pytest.raises(RuntimeError, match="device tensor"):
        fn(case.buf, pages, 0, False)
    with pytest.raises(RuntimeError, match="contiguous uint8"):
        fn(buf.to(torch.int32), pages, 0, False)
    with pytest.raises(RuntimeError, match=r"int64 \[n,6\]"):
        fn(buf, pages[:, :5].contiguous(), 0, False)
    with pytest.raises(RuntimeError, match="negative"):
        fn(buf, pages, -1, False)
    assert fn(buf, pages[:0], 0, True).dtype == torch.int32
    assert fn(buf, pages[:0], 5, False).shape == (5,)


def test_entry_point_is_registered_with_its_own_table():
    """pq_delta_values is registered in the split form that
    tests/test_pq_kernels.py leaves to other case tables."""
    src = os.path.join(os.path.dirname(G.__file__), "..", "ops", "csrc",
                       "module.cpp")
    with open(src) as f:
        registered = set(re.findall(r'm\.def\(\s*\n\s*"(pq_\w+)"', f.read()))
    assert "pq_delta_values" in registered
    assert callable(S.SIM.pq_delta_values)


# ---------------------------------------------------------------------------
# files written by pyarrow, through datasource/gpu_parquet.py
# ---------------------------------------------------------------------------

NROWS = 50_000


def _write_file(path):
    rng = _rng(21)
    days = rng.integers(8000, 12000, NROWS).astype("datetime64[D]")
    t = pa.table({
        "k64": pa.array(np.cumsum(rng.integers(0, 1 << 20, NROWS)) - 10**12),
        "v64": pa.array(rng.integers(-2**62, 2**62, NROWS),
                        mask=rng.random(NROWS) < 0.05),
        "i32": pa.array(rng.integers(-2**31, 2**31 - 1, NROWS)
                        .astype(np.int32)),
        "d32": pa.array(days, pa.date32()),
    })
    w = pq.ParquetWriter(path, t.schema, compression="NONE",
                         use_dictionary=False, data_page_size=4096,
                         data_page_version="1.0",
                         column_encoding={n: "DELTA_BINARY_PACKED"
                                          for n in t.schema.names})
    try:
        w.write_table(t, row_group_size=20_000)
    finally:
        w.close()
    return pq.read_table(path)


def _assert_table(out, want):
    assert list(out.columns) == want.schema.names
    for name in want.schema.names:
        col = out.columns[name]
        arr = want.column(name).combine_chunks()
        valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), bool)
        got_valid = (np.ones(len(arr), bool) if col.validity is None
                     else col.validity.cpu().numpy().astype(bool))
        assert np.array_equal(got_valid, valid), name
        if pa.types.is_date32(arr.type):
            arr = arr.cast(pa.int32())
        exp = arr.fill_null(0).to_numpy(zero_copy_only=False)
        got = col.data.cpu().numpy()
        assert got.dtype == exp.dtype and len(got) == len(exp), name
        assert np.array_equal(got[valid], exp[valid]), name


def _file_roundtrip(tmp_path, monkeypatch, read):
    p = str(tmp_path / "delta.parquet")
    want = _write_file(p)
    idx = G.file_index(p)
    assert idx.meta.num_row_groups == 3
    for ci in range(len(idx.schema)):
        chunks = idx.chunks(ci)
        assert {pg.enc for ch in chunks for pg in ch.pages} == \
            {G.DELTA_BINARY_PACKED}
        assert all(len(ch.pages) >= 3 for ch in chunks)
        assert chunks[-1].pages[-1].nvals < chunks[-1].pages[0].nvals
    for switch in ("on", "off", "on"):
        monkeypatch.setenv("SAIL_IO_GPU_DELTA_FUSED", switch)
        _assert_table(read(p, None), want)
    win = pq.ParquetFile(p).read_row_groups([1, 2])
    _assert_table(read(p, (1, 3)), win)


class _Recording:
    """Wraps an extension object; records every call's name and arguments."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def call(*a, **kw):
            self.calls.append((name, a))
            return fn(*a, **kw)
        return call


@pytest.fixture()
def sim(monkeypatch):
    rec = _Recording(S.SIM)
    monkeypatch.setattr(G, "_ext", lambda: rec)
    monkeypatch.setattr(G, "_ALLOW_CPU", True)
    yield rec


def test_sim_file_matches_pyarrow_switch_on_and_off(tmp_path, monkeypatch, sim):
    schema = [(n, None) for n in ("k64", "v64", "i32", "d32")]
    _file_roundtrip(tmp_path, monkeypatch,
                    lambda p, win: G.read_gpu([p], schema, "cpu", rg_window=win))
    names = [n for n, _ in sim.calls]
    # three whole-file reads of four columns, the middle one on the old path
    assert names.count("pq_delta_values") == 4 * 3
    assert names.count("pq_delta_decode") == 4 and names.count("pq_segscan") == 4
    flags = {a[3] for n, a in sim.calls if n == "pq_delta_values"}
    assert flags == {True, False}


def test_sim_old_extension_without_the_entry_keeps_working(tmp_path,
                                                           monkeypatch):
    """tests/pq_sim.py has no pq_delta_values: the two-call path runs with
    the switch at its default."""
    import pq_sim

    monkeypatch.setattr(G, "_ext", lambda: pq_sim)
    monkeypatch.setattr(G, "_ALLOW_CPU", True)
    monkeypatch.delenv("SAIL_IO_GPU_DELTA_FUSED", raising=False)
    p = str(tmp_path / "delta.parquet")
    want = _write_file(p).select(["k64", "d32"])
    _assert_table(G.read_gpu([p], [("k64", None), ("d32", None)], "cpu"), want)


@pytest.mark.gpu
def test_gpu_file_matches_pyarrow_switch_on_and_off(tmp_path, monkeypatch):
    monkeypatch.setenv("SAIL_IO_GPU_PARQUET", "force")
    schema = None

    def read(p, win):
        nonlocal schema
        if win is not None:
            return G.read_gpu([p], schema, "cuda:0", rg_window=win)
        schema = schema or parquet_io.infer_schema([p])
        return parquet_io.read([p], schema, "cuda:0", {})

    _file_roundtrip(tmp_path, monkeypatch, read)


def _cache_checks(tmp_path, rec, device):
    p = str(tmp_path / "cache.parquet")
    want = _write_file(p).select(["k64"])
    schema = [("k64", None)]

    def tables():
        return [a[1] for n, a in rec.calls if n == "pq_delta_values"]

    _assert_table(G.read_gpu([p], schema, device), want)
    _assert_table(G.read_gpu([p], schema, device), want)
    first, second = tables()
    assert second is first                    # no rebuild, no upload
    win = pq.ParquetFile(p).read_row_groups([0, 1]).select(["k64"])
    _assert_table(G.read_gpu([p], schema, device, rg_window=(0, 2)), win)
    assert tables()[2] is not first
    _assert_table(G.read_gpu([p], schema, device), want)
    assert tables()[3] is first
    held = sum(t.nbytes for t in G.file_index(p)._tables.values())
    assert 0 < held <= G.TABLE_CACHE_CAP

    # the same path rewritten: a fresh index, so a fresh table
    t2 = pa.table({"k64": pa.array(np.arange(30_000, dtype=np.int64) * 3)})
    pq.write_table(t2, p, compression="NONE", use_dictionary=False,
                   column_encoding={"k64": "DELTA_BINARY_PACKED"})
    _assert_table(G.read_gpu([p], schema, device), pq.read_table(p))
    assert tables()[4] is not first


def test_sim_page_table_is_cached_per_window(tmp_path, sim):
    _cache_checks(tmp_path, sim, "cpu")


@pytest.mark.gpu
def test_gpu_page_table_is_cached_per_window(tmp_path, monkeypatch):
    from sail_amd.ops import kernels

    rec = _Recording(kernels.require())
    monkeypatch.setattr(G, "_ext", lambda: rec)
    _cache_checks(tmp_path, rec, "cuda:0")


def test_sim_nulls_in_v1_pages_bypass_the_cache(tmp_path, sim):
    """v1 pages with nulls state no dense count: the table depends on the
    decoded levels, so it is rebuilt on every scan."""
    p = str(tmp_path / "nulls.parquet")
    want = _write_file(p).select(["v64"])
    for _ in range(2):
        _assert_table(G.read_gpu([p], [("v64", None)], "cpu"), want)
    a, b = [a[1] for n, a in sim.calls if n == "pq_delta_values"]
    assert a is not b and torch.equal(a, b)
    assert not G.file_index(p)._tables
