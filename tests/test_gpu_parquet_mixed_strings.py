"""String columns whose dictionary outgrew the writer's limit: the chunk
starts with RLE_DICTIONARY pages and goes on with PLAIN pages. Files come
from stock pq.write_table; the expectation is pq.read_table of the same
file; every comparison is exact.

6,000 rows, data_page_size=4096, dictionary_pagesize_limit=8192, every 11th
row null in the variants with nulls. Three data layouts:

* `one_rg`: 3,300 rows that cycle through 600 short values, then distinct
  URLs 'http://host/%06d/' + 'x' * (i % 40). The indices of the first 3,072
  rows fill a data page before the dictionary overflows, so the one chunk
  holds two RLE_DICTIONARY pages and then PLAIN pages.
* `three_rg`: row groups of 2,000; the first cycles through 23 URLs and
  stays all-dictionary, the other two overflow at once.
* `distinct`: the 6,000 distinct URLs alone, one row group. The stock writer
  then emits exactly one RLE_DICTIONARY page (it flushes the buffered
  indices when it falls back) in front of the PLAIN pages; asserted as
  that.

Every test first asserts, through the page index, that its file has the
layout it is about. All of them raised `mixed string encodings` before the
decoder learnt this layout.

CPU tests run the host orchestration against tests/pq_bytearray_sim.py;
`gpu` tests run the same files through the HIP kernels."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from sail_amd.datasource import gpu_parquet as G
from sail_amd.datasource import parquet_io
from sail_amd.engine import types as T

import pq_bytearray_sim
import pq_types_sim

NROWS = 6000
BASE = dict(data_page_size=4096, dictionary_pagesize_limit=8192)


def _url(i):
    return "http://host/%06d/" % i + "x" * (i % 40)


def _values(layout):
    if layout == "distinct":
        return [_url(i) for i in range(NROWS)]
    if layout == "one_rg":
        return ["h/%03d" % (i % 600) if i < 3300 else _url(i)
                for i in range(NROWS)]
    if layout == "three_rg":
        return [_url(i % 23) if i < 2000 else _url(i) for i in range(NROWS)]
    raise ValueError(layout)


def _write(path, layout, version="1.0", nulls=False, typ="string",
           compression="NONE"):
    vals = _values(layout)
    if typ == "binary":
        vals = [v.encode() for v in vals]
    mask = (np.arange(NROWS) % 11 == 0) if nulls else None
    arr = pa.array(vals, pa.binary() if typ == "binary" else pa.string(),
                   mask=mask)
    t = pa.table({"s": arr, "k": pa.array(np.arange(NROWS, dtype=np.int64))})
    pq.write_table(t, path, compression=compression,
                   data_page_version=version,
                   row_group_size=2000 if layout == "three_rg" else NROWS,
                   **BASE)
    return pq.read_table(path)


def _assert_layout(path, layout, snappy=False):
    """The file really mixes: at least two RLE_DICTIONARY and two PLAIN
    pages in the column, in one chunk for the one-row-group layouts."""
    idx = G.file_index(path)
    chunks = idx.chunks(idx.column_index("s"), snappy)
    per_chunk = [[p.enc for p in ch.pages] for ch in chunks]
    n_dict = [e.count(G.RLE_DICTIONARY) for e in per_chunk]
    n_plain = [e.count(G.PLAIN) for e in per_chunk]
    assert all(set(e) <= {G.RLE_DICTIONARY, G.PLAIN} for e in per_chunk)
    if layout == "three_rg":
        assert len(chunks) == 3
        assert n_plain[0] == 0 and n_dict[0] >= 1       # stays dictionary
        assert all(d >= 1 and p >= 1 for d, p in zip(n_dict[1:], n_plain[1:]))
        assert sum(n_dict) >= 2 and sum(n_plain) >= 2
    elif layout == "one_rg":
        assert len(chunks) == 1
        assert n_dict[0] >= 2 and n_plain[0] >= 2, per_chunk
    else:
        # the stock writer's answer to 6,000 distinct values: one page of
        # indices, flushed at the fallback, then PLAIN
        assert len(chunks) == 1
        assert n_dict[0] == 1 and n_plain[0] >= 2, per_chunk
    assert all(ch.dict_off is not None and ch.dict_nvals > 0 for ch in chunks)


def _assert_equal(out, want: pa.Table, coded=()):
    assert list(out.columns) == want.schema.names
    for name in want.schema.names:
        col = out.columns[name]
        arr = want.column(name).combine_chunks()
        assert len(col) == len(arr), name
        if pa.types.is_integer(arr.type):
            assert col.data.cpu().tolist() == arr.to_pylist(), name
            continue
        assert (col.codes is not None) == (name in coded), name
        # every BYTE_ARRAY path of the decoder returns T.STRING, for
        # pa.binary() too: all windows of a column agree on its type
        assert col.dtype == T.STRING, name
        got = col.to_pylist()
        want_list = arr.to_pylist()
        if pa.types.is_binary(arr.type):
            want_list = [None if w is None else w.decode() for w in want_list]
        assert got == want_list, name
        valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), bool)
        got_valid = (np.ones(len(arr), bool) if col.validity is None
                     else col.validity.cpu().numpy().astype(bool))
        assert np.array_equal(got_valid, valid), name


SCHEMA = [("s", None), ("k", None)]


def _roundtrip(tmp_path, device, layout, version, nulls, typ,
               compression="NONE"):
    p = str(tmp_path / "mixed.parquet")
    want = _write(p, layout, version, nulls, typ, compression)
    snappy = compression != "NONE"
    _assert_layout(p, layout, snappy)
    for _ in range(2):      # the second read finds the page index cached
        _assert_equal(G.read_gpu([p], SCHEMA, device, snappy=snappy), want)
    if layout == "three_rg":
        pf = pq.ParquetFile(p)
        for lo, hi in ((1, 3), (0, 2), (0, 1), (2, 3)):
            got = G.read_gpu([p], SCHEMA, device, rg_window=(lo, hi),
                             snappy=snappy)
            # window (0, 1) is all-dictionary: it keeps its coded form
            _assert_equal(got, pf.read_row_groups(list(range(lo, hi))),
                          coded=("s",) if (lo, hi) == (0, 1) else ())


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


@pytest.fixture()
def sim(monkeypatch):
    counting = _Counting(pq_bytearray_sim.SIM)
    monkeypatch.setattr(G, "_ext", lambda: counting)
    monkeypatch.setattr(G, "_ALLOW_CPU", True)
    monkeypatch.delenv("SAIL_IO_GPU_BYTEARRAY_FAST", raising=False)
    yield counting


@pytest.fixture()
def gpu_ext(monkeypatch):
    from sail_amd.ops import kernels

    counting = _Counting(kernels.require())
    monkeypatch.setattr(G, "_ext", lambda: counting)
    monkeypatch.delenv("SAIL_IO_GPU_BYTEARRAY_FAST", raising=False)
    yield counting


MATRIX = [(layout, version, nulls, typ)
          for layout in ("one_rg", "three_rg") for version in ("1.0", "2.0")
          for nulls in (False, True) for typ in ("string", "binary")]
DISTINCT_FILE = [("distinct", version, nulls, "string")
              for version in ("1.0", "2.0") for nulls in (False, True)]


@pytest.mark.parametrize("layout,version,nulls,typ", MATRIX + DISTINCT_FILE)
def test_sim_mixed_file_matches_pyarrow(tmp_path, sim, layout, version, nulls,
                                        typ):
    _roundtrip(tmp_path, "cpu", layout, version, nulls, typ)
    assert "pq_bytearray_index" in sim.calls and "pq_gather_bytes" in sim.calls
    assert "pq_bytearray_walk" not in sim.calls


@pytest.mark.gpu
@pytest.mark.parametrize("layout,version,nulls,typ", MATRIX + DISTINCT_FILE)
def test_gpu_mixed_file_matches_pyarrow(tmp_path, gpu_ext, layout, version,
                                        nulls, typ):
    _roundtrip(tmp_path, "cuda:0", layout, version, nulls, typ)
    assert "pq_bytearray_index" in gpu_ext.calls
    assert "pq_gather_bytes" in gpu_ext.calls
    assert "pq_bytearray_walk" not in gpu_ext.calls


@pytest.mark.parametrize("layout,nulls", [("one_rg", True), ("three_rg", False)])
def test_sim_snappy_v1_mixed_file(tmp_path, sim, layout, nulls):
    _roundtrip(tmp_path, "cpu", layout, "1.0", nulls, "string", "snappy")
    assert "pq_snappy_decompress" in sim.calls


@pytest.mark.gpu
@pytest.mark.parametrize("layout,nulls", [("one_rg", True), ("three_rg", False)])
def test_gpu_snappy_v1_mixed_file(tmp_path, gpu_ext, layout, nulls):
    _roundtrip(tmp_path, "cuda:0", layout, "1.0", nulls, "string", "snappy")
    assert "pq_snappy_decompress" in gpu_ext.calls


# ---------------------------------------------------------------------------
# the switch, and extensions without the new entry points
# ---------------------------------------------------------------------------

def _old_pair_when_off(tmp_path, monkeypatch, counting, device):
    p = str(tmp_path / "switch.parquet")
    want = _write(p, "three_rg", "1.0", True)
    _assert_layout(p, "three_rg")
    on = G.read_gpu([p], SCHEMA, device)
    _assert_equal(on, want)
    assert {"pq_bytearray_index", "pq_gather_bytes"} <= set(counting.calls)
    del counting.calls[:]
    for off in ("off", "0", "false"):
        monkeypatch.setenv("SAIL_IO_GPU_BYTEARRAY_FAST", off)
        got = G.read_gpu([p], SCHEMA, device)
        _assert_equal(got, want)
        for a, b in ((got.columns["s"].offsets, on.columns["s"].offsets),
                     (got.columns["s"].bytes_, on.columns["s"].bytes_)):
            assert torch.equal(a, b)
    assert {"pq_bytearray_walk", "pq_gather_strings"} <= set(counting.calls)
    assert not {"pq_bytearray_index", "pq_gather_bytes"} & set(counting.calls)


def test_sim_switch_off_runs_the_old_pair(tmp_path, monkeypatch, sim):
    _old_pair_when_off(tmp_path, monkeypatch, sim, "cpu")


@pytest.mark.gpu
def test_gpu_switch_off_runs_the_old_pair(tmp_path, monkeypatch, gpu_ext):
    _old_pair_when_off(tmp_path, monkeypatch, gpu_ext, "cuda:0")


def test_sim_extension_without_the_entries_keeps_working(tmp_path,
                                                         monkeypatch):
    """pq_types_sim.SIM has neither new entry point: the old pair decodes
    the mixed column with the switch at its default."""
    assert not hasattr(pq_types_sim.SIM, "pq_bytearray_index")
    monkeypatch.setattr(G, "_ext", lambda: pq_types_sim.SIM)
    monkeypatch.setattr(G, "_ALLOW_CPU", True)
    monkeypatch.delenv("SAIL_IO_GPU_BYTEARRAY_FAST", raising=False)
    p = str(tmp_path / "old.parquet")
    want = _write(p, "one_rg", "2.0", True)
    _assert_equal(G.read_gpu([p], SCHEMA, "cpu"), want)


def test_switch_defaults_on_and_recognises_off(monkeypatch):
    from sail_amd import config

    assert config.DEFAULTS["sail.io.gpu_bytearray_fast"] == "on"
    monkeypatch.delenv("SAIL_IO_GPU_BYTEARRAY_FAST", raising=False)
    assert G.bytearray_fast_enabled()
    for v in ("off", "0", "false", "OFF", "False"):
        monkeypatch.setenv("SAIL_IO_GPU_BYTEARRAY_FAST", v)
        assert not G.bytearray_fast_enabled(), v
    for v in ("on", "1", "true"):
        monkeypatch.setenv("SAIL_IO_GPU_BYTEARRAY_FAST", v)
        assert G.bytearray_fast_enabled(), v


# ---------------------------------------------------------------------------
# single-encoding string files through the new pair
# ---------------------------------------------------------------------------

def _single_encoding_files(tmp_path, counting, device):
    vals = _values("distinct")
    mask = np.arange(NROWS) % 11 == 0
    t = pa.table({"s": pa.array(vals, mask=mask)})
    p1 = str(tmp_path / "plain.parquet")
    pq.write_table(t, p1, compression="NONE", use_dictionary=False,
                   data_page_size=4096, row_group_size=2500)
    idx = G.file_index(p1)
    assert {pg.enc for ch in idx.chunks(0) for pg in ch.pages} == {G.PLAIN}
    _assert_equal(G.read_gpu([p1], [("s", None)], device), pq.read_table(p1))

    few = pa.table({"s": pa.array([_url(i % 300) for i in range(NROWS)],
                                  mask=mask)})
    p2 = str(tmp_path / "dict.parquet")
    pq.write_table(few, p2, compression="NONE", data_page_size=4096,
                   row_group_size=2500)
    idx = G.file_index(p2)
    assert {pg.enc for ch in idx.chunks(0) for pg in ch.pages} == \
        {G.RLE_DICTIONARY}
    got = G.read_gpu([p2], [("s", None)], device)
    _assert_equal(got, pq.read_table(p2), coded=("s",))
    # code order is byte order: the merged dictionary is sorted
    d = got.columns["s"]
    entries = [bytes(d.bytes_[a:b].cpu().tolist())
               for a, b in zip(d.offsets[:-1].tolist(), d.offsets[1:].tolist())]
    assert entries == sorted(set(entries)) and len(entries) == 300
    assert counting.calls.count("pq_bytearray_index") == 1 + 3
    assert "pq_bytearray_walk" not in counting.calls
    assert "pq_gather_strings" not in counting.calls


def test_sim_plain_only_and_dictionary_only_files(tmp_path, sim):
    _single_encoding_files(tmp_path, sim, "cpu")


@pytest.mark.gpu
def test_gpu_plain_only_and_dictionary_only_files(tmp_path, gpu_ext):
    _single_encoding_files(tmp_path, gpu_ext, "cuda:0")


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def _codes_out_of_range(device):
    limits = torch.tensor([3, 3, 3, 5, 5], dtype=torch.int64, device=device)

    def codes(*v):
        return torch.tensor(v, dtype=torch.int32, device=device)

    G._check_dict_codes(codes(0, 2, 1, 4, 0), limits, "s")
    G._check_dict_codes(codes(), limits[:0], "s")
    with pytest.raises(G.Unsupported, match=r"^s: dictionary code 3 at dense "
                                            r"value 1 outside a dictionary "
                                            r"of 3 entries"):
        G._check_dict_codes(codes(0, 3, 1, 4, 0), limits, "s")
    with pytest.raises(G.Unsupported, match="code 5 at dense value 4"):
        G._check_dict_codes(codes(0, 2, 1, 4, 5), limits, "s")
    with pytest.raises(G.Unsupported, match="code -1 at dense value 0"):
        G._check_dict_codes(codes(-1, 2, 1, 4, 0), limits, "s")


def test_dictionary_codes_out_of_range_are_refused():
    _codes_out_of_range("cpu")


@pytest.mark.gpu
def test_gpu_dictionary_codes_out_of_range_are_refused():
    _codes_out_of_range("cuda:0")


def _bad_file_refusals(tmp_path, device):
    p = str(tmp_path / "bad.parquet")
    want = _write(p, "one_rg", "1.0", False)
    idx = G.file_index(p)
    ch = idx.chunks(idx.column_index("s"))[0]
    _assert_equal(G.read_gpu([p], SCHEMA, device), want)

    # a chunk whose codes exceed its dictionary: the index says 600 entries,
    # claim 100
    nvals, ch.dict_nvals = ch.dict_nvals, 100
    with pytest.raises(G.Unsupported, match=r"^s: dictionary code 100 "):
        G.read_gpu([p], SCHEMA, device)
    # more entries than the dictionary page holds: the page is rejected
    ch.dict_nvals = nvals + 1
    with pytest.raises(G.Unsupported,
                       match=r"^s: dictionary page of row group 0 rejected, "
                             r"status 2"):
        G.read_gpu([p], SCHEMA, device)
    ch.dict_nvals = nvals

    # a PLAIN page cut short by one byte: its last length runs past it
    plain = [pg for pg in ch.pages if pg.enc == G.PLAIN]
    plain[1].val_len -= 1
    with pytest.raises(G.Unsupported,
                       match=rf"^s: plain page 1 of {len(plain)} rejected, "
                             r"status 1"):
        G.read_gpu([p], SCHEMA, device)
    plain[1].val_len += 1

    # dictionary-coded pages without a dictionary page
    off, ch.dict_off = ch.dict_off, None
    with pytest.raises(G.Unsupported, match="dict-encoded page, no dict"):
        G.read_gpu([p], SCHEMA, device)
    ch.dict_off = off
    _assert_equal(G.read_gpu([p], SCHEMA, device), want)

    # a mix that involves DELTA_LENGTH_BYTE_ARRAY stays refused (no writer
    # produces it: the page index is edited, on a window of its own so that
    # no cached page list answers)
    p2 = str(tmp_path / "dlba.parquet")
    _write(p2, "three_rg", "1.0", False)
    idx2 = G.file_index(p2)
    pages = idx2.chunks(idx2.column_index("s"))[1].pages
    pages[-1].enc = G.DELTA_LENGTH_BYTE_ARRAY
    with pytest.raises(G.Unsupported, match="s: mixed string encodings"):
        G.read_gpu([p2], SCHEMA, device, rg_window=(1, 2))


def test_sim_bad_files_are_refused(tmp_path, sim):
    _bad_file_refusals(tmp_path, "cpu")


@pytest.mark.gpu
def test_gpu_bad_files_are_refused(tmp_path, gpu_ext):
    _bad_file_refusals(tmp_path, "cuda:0")


# ---------------------------------------------------------------------------
# parity with the host path, batches, and the engine
# ---------------------------------------------------------------------------

def _assert_same_tables(dev_t, host_t):
    assert list(dev_t.columns) == list(host_t.columns)
    for name in dev_t.columns:
        a, b = dev_t.columns[name], host_t.columns[name]
        assert a.dtype == b.dtype, name
        assert len(a) == len(b), name
        if isinstance(a.dtype, T.StringType):
            assert a.to_pylist() == b.to_pylist(), name
        else:
            assert torch.equal(a.data.cpu(), b.data.cpu()), name


def test_sim_matches_host_path(tmp_path, sim):
    """Strings only: the host path has no binary columns."""
    p = str(tmp_path / "par.parquet")
    _write(p, "three_rg", "2.0", True)
    schema = parquet_io.infer_schema([p])
    host = parquet_io.read([p], schema, "cpu", {"gpuDecode": "off"})
    _assert_same_tables(G.read_gpu([p], schema, "cpu"), host)


@pytest.mark.gpu
def test_gpu_force_matches_off_and_batches(tmp_path, gpu_ext):
    p = str(tmp_path / "par.parquet")
    _write(p, "three_rg", "2.0", True)
    _assert_layout(p, "three_rg")
    schema = parquet_io.infer_schema([p])
    dev_t = parquet_io.read([p], schema, "cuda:0", {"gpuDecode": "force"})
    host = parquet_io.read([p], schema, "cuda:0", {"gpuDecode": "off"})
    _assert_same_tables(dev_t, host)
    assert "pq_bytearray_index" in gpu_ext.calls
    batches = list(parquet_io.scan_batches(
        [p], schema, "cuda:0", {"gpuDecode": "force"}, target_rows=1000))
    assert [b.num_rows for b in batches] == [2000, 2000, 2000]
    got = [v for b in batches for v in b.columns["s"].to_pylist()]
    assert got == host.columns["s"].to_pylist()


@pytest.mark.gpu
def test_gpu_sql_like_and_group_by_on_the_mixed_column(tmp_path, gpu_session,
                                                       session, monkeypatch):
    """LIKE filter and GROUP BY on the mixed column (no dictionary codes:
    the grouping goes through exact string codes); decode forced onto the
    device. Equal to the same query on a CPU session."""
    p = str(tmp_path / "q.parquet")
    _write(p, "three_rg", "1.0", True)
    _assert_layout(p, "three_rg")
    q = (f"SELECT s, COUNT(*), SUM(k) FROM parquet.`{p}` "
         "WHERE s LIKE 'http://host/0000%' GROUP BY s ORDER BY s")
    want = session.sql(q).collect()
    monkeypatch.setenv("SAIL_IO_GPU_PARQUET", "force")
    got = gpu_session.sql(q).collect()
    assert len(want) == 23 and got == want
