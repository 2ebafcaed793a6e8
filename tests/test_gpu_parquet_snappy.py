"""Opt-in device decode of SNAPPY parquet files (datasource/gpu_parquet.py
+ ops/csrc/snappy.hip): the switch, the host orchestration against the
kernel simulator (CPU), and the same files through the HIP kernels (GPU).

Two kinds of file, 3000 rows and 600-byte pages each, with and without
nulls, in 1 and 3 row groups: the mixed-encoding table of
tests/test_gpu_parquet.py written with compression="snappy", and a file
written by pq.write_table with no encoding arguments at all (Snappy,
RLE_DICTIONARY with PLAIN fallback), which is what other writers hand us.
The expectation is always pq.read_table on the same file."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from sail_amd.datasource import gpu_parquet as G
from sail_amd.datasource import parquet_io

import snappy_encode
from test_gpu_parquet import _write_mixed

NROWS = 3000
PAGE = 600


def _write_stock(path, nulls=False, row_groups=1):
    """pyarrow defaults: no compression or encoding argument."""
    rng = np.random.default_rng(11)

    def _mask(arr):
        if not nulls:
            return pa.array(arr)
        return pa.array(arr, mask=rng.random(NROWS) < 0.1)

    t = pa.table({
        "qty": _mask(rng.integers(1, 51, NROWS)),
        "mode": _mask(np.array(["AIR", "FOB", "MAIL", "RAIL", "SHIP",
                                "TRUCK", "REG AIR"])[
            rng.integers(0, 7, NROWS)]),
        "uid": _mask(np.array([f"order-{i:06d}-{int(v)}" for i, v in
                               enumerate(rng.integers(0, 10**9, NROWS))])),
        "price": _mask(rng.standard_normal(NROWS) * 1000.0),
    })
    pq.write_table(t, path, data_page_size=PAGE,
                   row_group_size=max(NROWS // row_groups, 1))
    return t


def _write(kind, path, nulls, row_groups):
    if kind == "mixed":
        _write_mixed(path, nrows=NROWS, page_size=PAGE, nulls=nulls,
                     compression="snappy", row_groups=row_groups)
    else:
        _write_stock(path, nulls=nulls, row_groups=row_groups)
    md = pq.ParquetFile(path).metadata
    assert md.num_row_groups >= row_groups
    for ci in range(md.num_columns):
        assert md.row_group(0).column(ci).compression == "SNAPPY"
    return pq.read_table(path)


def _assert_equal(out, t: pa.Table):
    assert list(out.columns) == t.schema.names
    for name in t.schema.names:
        exp = t.column(name).to_pylist()
        got = out.columns[name].to_pylist()
        at = t.schema.field(name).type
        if pa.types.is_decimal(at):
            # the engine hands decimals back as floats of the exact scaled
            # integer; same comparison as tests/test_gpu_parquet.py
            exp = [None if v is None else float(v) for v in exp]
            assert got == pytest.approx(exp), name
        elif pa.types.is_date32(at):
            assert [x if x is None else x.isoformat() for x in got] == \
                [x if x is None else x.isoformat() for x in exp], name
        else:
            assert got == exp, name


def _roundtrip(tmp_path, kind, nulls, row_groups, device):
    p = str(tmp_path / f"{kind}.parquet")
    t = _write(kind, p, nulls, row_groups)
    schema = [(f.name, None) for f in t.schema]
    out = G.read_gpu([p], schema, device, snappy=True)
    _assert_equal(out, t)
    # second read: page layout and dictionaries now come from the caches
    _assert_equal(G.read_gpu([p], schema, device, snappy=True), t)
    if row_groups == 3:
        # the row-group window the streaming scan uses
        lo, hi = 1, 3
        want = pq.ParquetFile(p).read_row_groups(list(range(lo, hi)))
        win = G.read_gpu([p], schema, device, rg_window=(lo, hi), snappy=True)
        _assert_equal(win, want)


@pytest.fixture()
def sim(monkeypatch):
    monkeypatch.setattr(G, "_ext", lambda: snappy_encode.SIM)
    monkeypatch.setattr(G, "_ALLOW_CPU", True)
    yield


# ---------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------

def test_switch_spellings_and_default(monkeypatch):
    from sail_amd.config import DEFAULTS

    assert DEFAULTS["sail.io.gpu_snappy"] == "off"
    monkeypatch.delenv("SAIL_IO_GPU_SNAPPY", raising=False)
    assert G.snappy_enabled() is False
    assert G.snappy_enabled({}) is False
    assert G.snappy_enabled({"gpuSnappy": "on"}) is True
    assert G.snappy_enabled({"gpuSnappy": "off"}) is False
    monkeypatch.setenv("SAIL_IO_GPU_SNAPPY", "on")
    assert G.snappy_enabled() is True
    assert G.snappy_enabled({"gpuSnappy": "off"}) is False   # option wins


@pytest.mark.parametrize("kind", ["mixed", "stock"])
def test_switch_off_snappy_file_unsupported(tmp_path, sim, monkeypatch, kind):
    """Off (the default): Unsupported names the codec, as before; and an
    index asked with the switch off does not answer for the switch on, nor
    the other way round."""
    monkeypatch.delenv("SAIL_IO_GPU_SNAPPY", raising=False)
    p = str(tmp_path / "off.parquet")
    t = _write(kind, p, False, 1)
    schema = [(f.name, None) for f in t.schema]
    idx = G.file_index(p)
    with pytest.raises(G.Unsupported, match="compression SNAPPY"):
        idx.chunks(0)
    with pytest.raises(G.Unsupported, match="compression SNAPPY"):
        G.read_gpu([p], schema, "cpu")
    _assert_equal(G.read_gpu([p], schema, "cpu", snappy=True), t)
    with pytest.raises(G.Unsupported, match="compression SNAPPY"):
        G.read_gpu([p], schema, "cpu")
    with pytest.raises(G.Unsupported, match="compression SNAPPY"):
        G.read_gpu([p], schema, "cpu", snappy=False)
    monkeypatch.setenv("SAIL_IO_GPU_SNAPPY", "on")
    _assert_equal(G.read_gpu([p], schema, "cpu"), t)


def test_other_codecs_and_v2_pages_stay_unsupported(tmp_path, sim):
    t = pa.table({"a": pa.array(range(500), pa.int64())})
    p1 = str(tmp_path / "gz.parquet")
    pq.write_table(t, p1, compression="gzip")
    with pytest.raises(G.Unsupported, match="compression GZIP"):
        G.read_gpu([p1], [("a", None)], "cpu", snappy=True)
    p2 = str(tmp_path / "v2.parquet")
    pq.write_table(t, p2, compression="snappy", data_page_version="2.0")
    with pytest.raises(G.Unsupported, match="page type 3"):
        G.read_gpu([p2], [("a", None)], "cpu", snappy=True)


def test_rejected_page_raises_unsupported(tmp_path, sim, monkeypatch):
    """A non-zero kernel status becomes Unsupported naming column, page
    and code (auto mode then falls back to pyarrow, force mode raises)."""
    p = str(tmp_path / "bad.parquet")
    t = _write("stock", p, False, 1)

    class Rejecting(snappy_encode.SimExt):
        @staticmethod
        def pq_snappy_decompress(buf, pages, out):
            st = snappy_encode.pq_snappy_decompress(buf, pages, out)
            st[2] = snappy_encode.BAD_OFFSET
            return st

    monkeypatch.setattr(G, "_ext", lambda: Rejecting())
    with pytest.raises(G.Unsupported, match=r"qty: snappy page 2 .*status 4"):
        G.read_gpu([p], [("qty", None)], "cpu", snappy=True)


# ---------------------------------------------------------------------------
# whole files
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("row_groups", [1, 3])
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("kind", ["mixed", "stock"])
def test_sim_snappy_file_matches_pyarrow(tmp_path, sim, kind, nulls,
                                         row_groups):
    _roundtrip(tmp_path, kind, nulls, row_groups, "cpu")


def test_sim_stock_file_has_dictionary_and_plain_pages(tmp_path, sim):
    """The stock file reaches what it is meant to: dictionary-encoded
    pages behind definition levels, and a unique string column."""
    p = str(tmp_path / "s.parquet")
    _write("stock", p, True, 1)
    idx = G.file_index(p)
    G.read_gpu([p], [("mode", None), ("uid", None)], "cpu", snappy=True)
    mode = idx.chunks(idx.column_index("mode"), True)[0]
    assert mode.compressed and mode.dict_off is not None
    assert len(mode.pages) > 1
    assert all(pg.resolved and pg.enc == G.RLE_DICTIONARY and pg.bw0 == 3
               and not pg.all_valid and pg.def_len > 0 for pg in mode.pages)


@pytest.mark.gpu
@pytest.mark.parametrize("row_groups", [1, 3])
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("kind", ["mixed", "stock"])
def test_gpu_snappy_file_matches_pyarrow(tmp_path, kind, nulls, row_groups):
    _roundtrip(tmp_path, kind, nulls, row_groups, "cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mixed", "stock"])
def test_gpu_snappy_read_options_force(tmp_path, kind):
    """parquet_io.read with gpuDecode=force + gpuSnappy=on decodes on the
    device (force allows no host fallback); with the switch off, force
    raises."""
    p = str(tmp_path / "o.parquet")
    t = _write(kind, p, True, 3)
    schema = parquet_io.infer_schema([p])
    out = parquet_io.read([p], schema, "cuda:0",
                          {"gpuDecode": "force", "gpuSnappy": "on"})
    _assert_equal(out, t)
    with pytest.raises(G.Unsupported, match="compression SNAPPY"):
        parquet_io.read([p], schema, "cuda:0",
                        {"gpuDecode": "force", "gpuSnappy": "off"})
    batches = list(parquet_io.scan_batches(
        [p], schema, "cuda:0", {"gpuDecode": "force", "gpuSnappy": "on"},
        target_rows=1000))
    assert len(batches) == 3
    assert sum(b.num_rows for b in batches) == NROWS


@pytest.mark.gpu
def test_gpu_snappy_sql_query(tmp_path, gpu_session, monkeypatch):
    """One SQL query over a stock Snappy file, decode forced to the GPU."""
    p = str(tmp_path / "q.parquet")
    t = _write("stock", p, True, 3)
    monkeypatch.setenv("SAIL_IO_GPU_PARQUET", "force")
    monkeypatch.setenv("SAIL_IO_GPU_SNAPPY", "on")
    rows = gpu_session.sql(
        f"SELECT mode, COUNT(*), SUM(qty), COUNT(uid) FROM parquet.`{p}` "
        "WHERE mode IS NOT NULL GROUP BY mode ORDER BY mode").collect()
    exp = {}
    for m, q, u in zip(t.column("mode").to_pylist(),
                       t.column("qty").to_pylist(),
                       t.column("uid").to_pylist()):
        if m is None:
            continue
        c, sq, cu = exp.get(m, (0, 0, 0))
        exp[m] = (c + 1, sq + (q or 0), cu + (u is not None))
    assert rows == [(m,) + exp[m] for m in sorted(exp)]
