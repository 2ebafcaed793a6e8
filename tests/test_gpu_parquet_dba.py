"""DELTA_BYTE_ARRAY string and binary columns of pyarrow-written files
through the scan (datasource/gpu_parquet.py + parquet_delta_bytearray.hip):
on the device under SAIL_IO_GPU_PARQUET=force, and on the host path when the
switch is off or there is no device. Bytes, lengths and validity are compared
exactly with pq.read_table."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from sail_amd.datasource import gpu_parquet as G
from sail_amd.datasource import parquet_io

NROWS = 3000


def _write(path, version, nulls, **kw):
    rng = np.random.default_rng(23)
    mask = (rng.random(NROWS) < 0.15) if nulls else None
    urls = sorted(f"https://example.org/{a:02d}/item/{b:07d}?p={'é' * (b % 3)}"
                  for a, b in zip(rng.integers(0, 20, NROWS),
                                  rng.integers(0, 10**7, NROWS)))
    blobs = [rng.bytes(int(k)) for k in rng.integers(0, 24, NROWS)]
    t = pa.table({"url": pa.array(urls, pa.string(), mask=mask),
                  "blob": pa.array(blobs, pa.binary(), mask=mask)})
    args = dict(compression="NONE", use_dictionary=False, data_page_size=4096,
                write_batch_size=64, data_page_version=version,
                column_encoding={"url": "DELTA_BYTE_ARRAY",
                                 "blob": "DELTA_BYTE_ARRAY"})
    args.update(kw)
    pq.write_table(t, path, **args)
    return pq.read_table(path)


def _assert_equal(out, want):
    for name in want.schema.names:
        col = out.columns[name]
        exp = want.column(name).combine_chunks().cast(pa.binary()).to_pylist()
        offs = col.offsets.cpu().tolist()
        blob = col.bytes_.cpu().numpy().tobytes()
        valid = [True] * len(exp) if col.validity is None else \
            col.validity.cpu().to(bool).tolist()
        got = [blob[offs[i]:offs[i + 1]] if v else None
               for i, v in enumerate(valid)]
        assert got == exp, name
        assert offs[-1] == len(blob), name      # null rows hold no bytes


@pytest.mark.gpu
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("nulls", [False, True])
def test_gpu_force_scan_equals_pyarrow(tmp_path, monkeypatch, version, nulls):
    monkeypatch.setenv("SAIL_IO_GPU_PARQUET", "force")
    monkeypatch.delenv("SAIL_IO_GPU_DELTA_BYTEARRAY", raising=False)
    p = str(tmp_path / "dba.parquet")
    want = _write(p, version, nulls)
    idx = G.file_index(p)
    for ci in range(2):
        pages = idx.chunks(ci, False)[0].pages
        assert len(pages) >= 3 and {pg.enc for pg in pages} == {G.DELTA_BYTE_ARRAY}
    schema = [(f.name, None) for f in want.schema]
    _assert_equal(parquet_io.read([p], schema, "cuda:0", {}), want)


@pytest.mark.gpu
def test_gpu_snappy_v1_chunk_expands_then_decodes(tmp_path, monkeypatch):
    monkeypatch.setenv("SAIL_IO_GPU_PARQUET", "force")
    p = str(tmp_path / "dba_snappy.parquet")
    want = _write(p, "1.0", True, compression="snappy")
    schema = [(f.name, None) for f in want.schema]
    _assert_equal(parquet_io.read([p], schema, "cuda:0", {"gpuSnappy": "on"}),
                  want)


@pytest.mark.gpu
def test_gpu_switch_off_refuses_the_encoding(tmp_path, monkeypatch):
    monkeypatch.setenv("SAIL_IO_GPU_DELTA_BYTEARRAY", "off")
    p = str(tmp_path / "dba.parquet")
    want = _write(p, "1.0", False)
    schema = [(f.name, None) for f in want.schema]
    with pytest.raises(G.Unsupported, match="url: encodings"):
        G.read_gpu([p], schema, "cuda:0")
    # outside force mode the same read falls back to the host, which has
    # no binary type
    _assert_equal(parquet_io.read([p], schema[:1], "cuda:0", {}),
                  want.select(["url"]))


@pytest.mark.parametrize("switch", ["on", "off"])
def test_host_path_equals_pyarrow(tmp_path, monkeypatch, switch):
    monkeypatch.setenv("SAIL_IO_GPU_DELTA_BYTEARRAY", switch)
    monkeypatch.delenv("SAIL_IO_GPU_PARQUET", raising=False)
    assert G.delta_bytearray_enabled() == (switch == "on")
    p = str(tmp_path / "dba.parquet")
    want = _write(p, "2.0", True)
    schema = [(f.name, None) for f in want.schema]
    # the host path has no binary type: the string column alone
    _assert_equal(parquet_io.read([p], schema[:1], "cpu", {}),
                  want.select(["url"]))


def test_mixed_chunk_is_refused_by_column_name(tmp_path, monkeypatch):
    """One chunk with DELTA_BYTE_ARRAY pages and pages of another encoding
    (parquet-java's v2 dictionary fallback looks like this)."""
    monkeypatch.delenv("SAIL_IO_GPU_DELTA_BYTEARRAY", raising=False)
    p = str(tmp_path / "dba.parquet")
    _write(p, "1.0", False)
    idx = G.file_index(p)
    idx.chunks(0, False)[0].pages[0].enc = G.RLE_DICTIONARY
    monkeypatch.setattr(G, "_ALLOW_CPU", True)
    with pytest.raises(G.Unsupported, match="url: mixed string encodings"):
        G._ColumnDecoder(idx, "url", "cpu")
