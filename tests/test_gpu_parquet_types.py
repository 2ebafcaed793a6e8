"""BOOLEAN, INT96, BYTE_STREAM_SPLIT and v2 data pages through
datasource/gpu_parquet.py: the host orchestration against the kernel
simulator (CPU) and the same files through the HIP kernels (GPU).

Files are written by pyarrow; the expectation is pq.read_table on the same
file (INT96 coerced to microseconds). Every comparison is exact; floats are
compared by bit pattern. 3000 rows; 30-byte pages and 64-row write batches
so that even the bit-packed boolean column is cut into several pages per
column chunk (asserted through the page index).

Layouts: (a) v1 stock, (b) v1 PLAIN, (c) v2 stock with a small dictionary
limit (dictionary pages, then PLAIN fallback, RLE booleans), (d) v2 with
DELTA encodings, (e) BYTE_STREAM_SPLIT, (f) layout (a) under Snappy with
the device-Snappy switch on, (g) an all-null column and a zero-row file.
Layouts (a), (c) and (e) raised Unsupported before these decoders
existed."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from sail_amd.datasource import gpu_parquet as G
from sail_amd.datasource import parquet_io
from sail_amd.engine import types as T

import pq_types_sim

NROWS = 3000
_US_1700 = int(np.datetime64("1700-01-01", "us").astype(np.int64))
_US_2200 = int(np.datetime64("2200-01-01", "us").astype(np.int64))
_DAY = 86_400_000_000


def _table(nulls, nrows=NROWS):
    rng = np.random.default_rng(5)

    def col(values, typ=None):
        mask = (rng.random(nrows) < 0.1) if nulls else None
        return pa.array(values, typ, mask=mask)

    ts = rng.integers(_US_1700, _US_2200, nrows)
    ts_low = _US_1700 + rng.integers(0, 40, nrows) * 4000 * _DAY + 1_000_001
    f64 = rng.standard_normal(nrows)
    f32 = rng.standard_normal(nrows).astype(np.float32)
    for a in (f64, f32):
        a[3], a[4], a[5], a[6] = np.nan, -0.0, np.inf, -np.inf
    f64[7:9] = np.array([0x7FF8000000000123, 0xFFF0000000000001],
                        dtype=np.uint64).view(np.float64)   # NaN payloads
    return pa.table({
        "b": col(rng.random(nrows) < 0.5),
        "ts": col(ts.astype("datetime64[us]"), pa.timestamp("us")),
        "ts_low": col(ts_low.astype("datetime64[us]"), pa.timestamp("us")),
        "i64": col(rng.integers(-10**12, 10**12, nrows)),
        "i32": col(rng.integers(-2**31, 2**31 - 1, nrows).astype(np.int32)),
        "f64": col(f64),
        "f32": col(f32),
        "mode": col(np.array(["AIR", "FOB", "MAIL", "RAIL"])[
            rng.integers(0, 4, nrows)]),
        "tag": col(np.array([f"t{v:03d}" for v in
                             rng.integers(0, 300, nrows)])),
    })


COMMON = dict(data_page_size=30, write_batch_size=64,
              use_deprecated_int96_timestamps=True)

#: layout -> (pq.write_table arguments, columns, encodings a column must show)
LAYOUTS = {
    "a_v1_stock": (dict(compression="NONE", data_page_version="1.0"), None,
                   {"b": {G.PLAIN}, "ts": {G.RLE_DICTIONARY}}),
    "b_v1_plain": (dict(compression="NONE", data_page_version="1.0",
                        use_dictionary=False), None,
                   {"b": {G.PLAIN}, "ts": {G.PLAIN}}),
    "c_v2_stock": (dict(compression="NONE", data_page_version="2.0",
                        dictionary_pagesize_limit=4000), None,
                   {"b": {G.RLE}, "ts": {G.RLE_DICTIONARY, G.PLAIN},
                    "ts_low": {G.RLE_DICTIONARY},
                    "f64": {G.RLE_DICTIONARY, G.PLAIN}}),
    "d_v2_delta": (dict(compression="NONE", data_page_version="2.0",
                        use_dictionary=False,
                        column_encoding={"i64": "DELTA_BINARY_PACKED",
                                         "i32": "DELTA_BINARY_PACKED",
                                         "mode": "DELTA_LENGTH_BYTE_ARRAY",
                                         "tag": "DELTA_LENGTH_BYTE_ARRAY"}),
                   ["b", "ts", "i64", "i32", "mode", "tag"],
                   {"i64": {G.DELTA_BINARY_PACKED},
                    "tag": {G.DELTA_LENGTH_BYTE_ARRAY}, "b": {G.RLE}}),
    "e_bss": (dict(compression="NONE", data_page_version="1.0",
                   use_dictionary=False,
                   column_encoding={c: "BYTE_STREAM_SPLIT" for c in
                                    ("f64", "f32", "i64", "i32")}),
              ["f64", "f32", "i64", "i32", "b"],
              {c: {G.BYTE_STREAM_SPLIT} for c in ("f64", "f32", "i64", "i32")}),
    "f_v1_snappy": (dict(compression="snappy", data_page_version="1.0"), None,
                    {}),
}


def _write(layout, path, nulls, row_groups):
    kw, cols, _ = LAYOUTS[layout]
    t = _table(nulls)
    if cols:
        t = t.select(cols)
    pq.write_table(t, path, row_group_size=NROWS // row_groups,
                   **COMMON, **kw)
    return pq.read_table(path, coerce_int96_timestamp_unit="us")


def _check_index(layout, path, row_groups, snappy):
    """Every column chunk has at least 3 data pages, v2 files really hold
    v2 pages, and the columns show the encodings the layout is about."""
    idx = G.file_index(path)
    assert idx.meta.num_row_groups == row_groups
    want_enc = LAYOUTS[layout][2]
    for ci in range(len(idx.schema)):
        name = idx.schema.column(ci).name
        chunks = idx.chunks(ci, snappy)
        assert len(chunks) == row_groups
        for ch in chunks:
            assert len(ch.pages) >= 3, (name, len(ch.pages))
            if "_v2_" in layout:
                assert all(p.ndense is not None for p in ch.pages), name
        if name in want_enc:
            assert {p.enc for ch in chunks for p in ch.pages} == \
                want_enc[name], name


def _np(t):
    return t.cpu().numpy()


def _assert_equal(out, want: pa.Table):
    assert list(out.columns) == want.schema.names
    for name in want.schema.names:
        col = out.columns[name]
        arr = want.column(name).combine_chunks()
        at = arr.type
        if pa.types.is_string(at):
            assert col.to_pylist() == arr.to_pylist(), name
            continue
        valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False),
                           dtype=bool)
        got_valid = (np.ones(len(arr), dtype=bool) if col.validity is None
                     else _np(col.validity).astype(bool))
        assert len(col) == len(arr), name
        assert np.array_equal(got_valid, valid), name
        got = _np(col.data)
        if pa.types.is_boolean(at):
            assert col.dtype == T.BOOL and col.data.dtype == torch.bool, name
            exp = arr.fill_null(False).to_numpy(zero_copy_only=False)
        elif pa.types.is_timestamp(at):
            assert col.dtype == T.TIMESTAMP and got.dtype == np.int64, name
            exp = arr.cast(pa.int64()).fill_null(0).to_numpy(
                zero_copy_only=False)
        else:
            exp = arr.fill_null(0).to_numpy(zero_copy_only=False)
            assert got.dtype == exp.dtype, name
            if exp.dtype.kind == "f":     # by bit pattern
                as_int = np.int32 if exp.dtype.itemsize == 4 else np.int64
                got, exp = got.view(as_int), exp.view(as_int)
        assert np.array_equal(got[valid], exp[valid]), name


def _roundtrip(tmp_path, layout, nulls, row_groups, device):
    p = str(tmp_path / f"{layout}.parquet")
    want = _write(layout, p, nulls, row_groups)
    snappy = layout == "f_v1_snappy"
    _check_index(layout, p, row_groups, snappy)
    schema = [(f.name, None) for f in want.schema]
    _assert_equal(G.read_gpu([p], schema, device, snappy=snappy), want)
    # second read: page layout and dictionaries now come from the caches
    _assert_equal(G.read_gpu([p], schema, device, snappy=snappy), want)
    if row_groups == 3:
        win = pq.ParquetFile(p, coerce_int96_timestamp_unit="us") \
            .read_row_groups([1, 2])
        got = G.read_gpu([p], schema, device, rg_window=(1, 3), snappy=snappy)
        _assert_equal(got, win)


@pytest.fixture()
def sim(monkeypatch):
    monkeypatch.setattr(G, "_ext", lambda: pq_types_sim.SIM)
    monkeypatch.setattr(G, "_ALLOW_CPU", True)
    yield


PARAMS = [(layout, nulls, rgs) for layout in LAYOUTS
          for nulls in (False, True) for rgs in (1, 3)]


@pytest.mark.parametrize("layout,nulls,row_groups", PARAMS)
def test_sim_file_matches_pyarrow(tmp_path, sim, layout, nulls, row_groups):
    _roundtrip(tmp_path, layout, nulls, row_groups, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("layout,nulls,row_groups", PARAMS)
def test_gpu_file_matches_pyarrow(tmp_path, layout, nulls, row_groups):
    _roundtrip(tmp_path, layout, nulls, row_groups, "cuda:0")


# ---------------------------------------------------------------------------
# (g) an all-null column and a zero-row file, v2
# ---------------------------------------------------------------------------

def _all_null_and_empty(tmp_path, device):
    t = _table(True, 600)
    nothing = {"b": pa.bool_(), "ts": pa.timestamp("us"), "i64": pa.int64(),
               "f64": pa.float64(), "mode": pa.string()}
    for name, typ in nothing.items():
        t = t.set_column(t.schema.get_field_index(name), name,
                         pa.nulls(600, typ))
    p = str(tmp_path / "nulls.parquet")
    pq.write_table(t, p, compression="NONE", data_page_version="2.0",
                   row_group_size=200, **COMMON)
    want = pq.read_table(p, coerce_int96_timestamp_unit="us")
    assert want.column("ts").null_count == 600
    schema = [(f.name, None) for f in want.schema]
    for _ in range(2):
        _assert_equal(G.read_gpu([p], schema, device), want)

    p0 = str(tmp_path / "empty.parquet")
    pq.write_table(_table(False, 600).slice(0, 0), p0, compression="NONE",
                   data_page_version="2.0", **COMMON)
    want0 = pq.read_table(p0, coerce_int96_timestamp_unit="us")
    assert want0.num_rows == 0
    _assert_equal(G.read_gpu([p0], schema, device), want0)


def test_sim_all_null_column_and_zero_rows(tmp_path, sim):
    _all_null_and_empty(tmp_path, "cpu")


@pytest.mark.gpu
def test_gpu_all_null_column_and_zero_rows(tmp_path):
    _all_null_and_empty(tmp_path, "cuda:0")


# ---------------------------------------------------------------------------
# still refused
# ---------------------------------------------------------------------------

def test_still_unsupported_layouts(tmp_path, sim):
    import decimal

    t = pa.table({"s": pa.array([f"k{i}" for i in range(500)])})
    p1 = str(tmp_path / "dba.parquet")
    pq.write_table(t, p1, compression="NONE", use_dictionary=False,
                   column_encoding={"s": "DELTA_BYTE_ARRAY"})
    with pytest.raises(G.Unsupported, match=r"s: encodings \{7\}"):
        G.read_gpu([p1], [("s", None)], "cpu")

    d = pa.table({"d": pa.array([decimal.Decimal(i) / 100 for i in range(500)],
                                pa.decimal128(12, 2))})
    p2 = str(tmp_path / "bss_flba.parquet")
    pq.write_table(d, p2, compression="NONE", use_dictionary=False,
                   column_encoding={"d": "BYTE_STREAM_SPLIT"})
    assert pq.ParquetFile(p2).schema.column(0).physical_type == \
        "FIXED_LEN_BYTE_ARRAY"
    with pytest.raises(G.Unsupported, match=r"d: encodings \{9\}"):
        G.read_gpu([p2], [("d", None)], "cpu")

    p3 = str(tmp_path / "v2sn.parquet")
    pq.write_table(_table(False, 500), p3, compression="snappy",
                   data_page_version="2.0", **COMMON)
    with pytest.raises(G.Unsupported, match="page type 3"):
        G.read_gpu([p3], [("b", None)], "cpu", snappy=True)
    with pytest.raises(G.Unsupported, match="compression SNAPPY"):
        G.read_gpu([p3], [("b", None)], "cpu", snappy=False)


class _Counting:
    """Wraps an extension object; records the name of every call."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)

        def call(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return call


#: (layout, column, encoding of its pages, shrunk val_len for c values)
SHRINK = [("b_v1_plain", "b", G.PLAIN, lambda c, w: (c + 7) // 8 - 1),
          ("b_v1_plain", "ts", G.PLAIN, lambda c, w: 12 * c - 1),
          ("c_v2_stock", "b", G.RLE, lambda c, w: 3),
          ("e_bss", "f64", G.BYTE_STREAM_SPLIT, lambda c, w: w - 1),
          ("e_bss", "i32", G.BYTE_STREAM_SPLIT, lambda c, w: w + 1)]


def _shrunk_page(tmp_path, ext, device, monkeypatch, layout, column, enc,
                 bad_len):
    """A page whose value region is too short for its values (val_len
    changed on the cached page index) raises Unsupported naming column and
    page before any kernel is launched. No nulls: no validity launch."""
    p = str(tmp_path / "short.parquet")
    want = _write(layout, p, False, 1)
    idx = G.file_index(p)
    pages = idx.chunks(idx.column_index(column))[0].pages
    page = pages[1]
    assert page.enc == enc and page.nvals > 8
    good = G.read_gpu([p], [(column, None)], device)
    _assert_equal(good, want.select([column]))
    page.val_len = bad_len(page.nvals, page.val_len)
    counting = _Counting(ext)
    monkeypatch.setattr(G, "_ext", lambda: counting)
    with pytest.raises(G.Unsupported, match=rf"^{column}: page 1: "):
        G.read_gpu([p], [(column, None)], device)
    assert counting.calls == []


@pytest.mark.parametrize("layout,column,enc,bad_len", SHRINK)
def test_sim_short_page_raises_before_launch(tmp_path, sim, monkeypatch,
                                             layout, column, enc, bad_len):
    _shrunk_page(tmp_path, pq_types_sim.SIM, "cpu", monkeypatch, layout,
                 column, enc, bad_len)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,column,enc,bad_len", SHRINK)
def test_gpu_short_page_raises_before_launch(tmp_path, monkeypatch, layout,
                                             column, enc, bad_len):
    from sail_amd.ops import kernels

    _shrunk_page(tmp_path, kernels.require(), "cuda:0", monkeypatch, layout,
                 column, enc, bad_len)


# ---------------------------------------------------------------------------
# parity with the host path, and the engine
# ---------------------------------------------------------------------------

def _assert_same_tables(dev_t, host_t):
    assert list(dev_t.columns) == list(host_t.columns)
    for name in dev_t.columns:
        a, b = dev_t.columns[name], host_t.columns[name]
        assert a.dtype == b.dtype, name
        assert len(a) == len(b), name
        if a.dtype == T.STRING:
            assert a.to_pylist() == b.to_pylist(), name
            continue
        n = len(a)
        va = (np.ones(n, bool) if a.validity is None
              else _np(a.validity).astype(bool))
        vb = (np.ones(n, bool) if b.validity is None
              else _np(b.validity).astype(bool))
        assert np.array_equal(va, vb), name
        assert a.data.dtype == b.data.dtype, name
        da, db = _np(a.data), _np(b.data)
        if da.dtype.kind == "f":
            as_int = np.int32 if da.dtype.itemsize == 4 else np.int64
            da, db = da.view(as_int), db.view(as_int)
        assert np.array_equal(da[va], db[va]), name


@pytest.mark.parametrize("layout", ["a_v1_stock", "c_v2_stock"])
def test_sim_matches_host_path(tmp_path, sim, layout):
    """The decoder's table against parquet_io's host path (gpuDecode=off):
    names, engine types, values, validity."""
    p = str(tmp_path / "par.parquet")
    _write(layout, p, True, 3)
    schema = parquet_io.infer_schema([p])
    assert dict(schema)["b"] == T.BOOL and dict(schema)["ts"] == T.TIMESTAMP
    host = parquet_io.read([p], schema, "cpu", {"gpuDecode": "off"})
    _assert_same_tables(G.read_gpu([p], schema, "cpu"), host)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["a_v1_stock", "c_v2_stock"])
def test_gpu_force_matches_off(tmp_path, layout):
    """parquet_io.read with gpuDecode=force (no host fallback allowed)
    against gpuDecode=off on the same file."""
    p = str(tmp_path / "par.parquet")
    _write(layout, p, True, 3)
    schema = parquet_io.infer_schema([p])
    dev_t = parquet_io.read([p], schema, "cuda:0", {"gpuDecode": "force"})
    host = parquet_io.read([p], schema, "cuda:0", {"gpuDecode": "off"})
    assert dev_t.columns["b"].dtype == T.BOOL
    assert dev_t.columns["ts"].dtype == T.TIMESTAMP
    _assert_same_tables(dev_t, host)
    batches = list(parquet_io.scan_batches(
        [p], schema, "cuda:0", {"gpuDecode": "force"}, target_rows=1000))
    assert [b.num_rows for b in batches] == [1000, 1000, 1000]


@pytest.mark.gpu
def test_gpu_sql_filter_bool_group_by_int96(tmp_path, gpu_session, session,
                                            monkeypatch):
    """Filter on the boolean column, group by the INT96 timestamp truncated
    to the year, over a v2 file; decode forced onto the device. Equal to
    the same query on a CPU session."""
    p = str(tmp_path / "q.parquet")
    _write("c_v2_stock", p, True, 3)
    q = (f"SELECT date_trunc('year', ts) AS y, COUNT(*), SUM(i64), "
         f"COUNT(ts_low) FROM parquet.`{p}` WHERE b GROUP BY "
         "date_trunc('year', ts) ORDER BY y")
    want = session.sql(q).collect()
    monkeypatch.setenv("SAIL_IO_GPU_PARQUET", "force")
    got = gpu_session.sql(q).collect()
    assert len(want) > 100 and got == want
