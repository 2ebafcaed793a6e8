"""The device half of the pipelined column-chunk reader
(ops/csrc/scan_reader.hip, pq_read_ranges) against the Python reader of
datasource/gpu_parquet.py.

The ring is set to 4 KB slices and 2 slots, so a 100 KB file gives up to 26
slices and every slot is reused many times within a call. The expected
device buffer is always what _upload_ranges returns with the switch off:
the concatenated bytes followed by 16 zero bytes. The host half has its own
stand-alone check (tests/native/scan_reader_check.cpp, run by
tests/test_scan_reader_host.py); the switch and range coalescing are also
checked here without a GPU."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from sail_amd.datasource import gpu_parquet as G

FILE_BYTES = 100 * 1024 + 37
SLICE = 4096


def _range_shapes():
    rng = np.random.default_rng(5)
    fifty = []
    for i in range(50):
        n = (0, int(rng.integers(1, 100)), SLICE, int(rng.integers(1, 3000)),
             SLICE + int(rng.integers(1, 6000)))[i % 5]
        s = int(rng.integers(0, FILE_BYTES - n))
        fifty.append((s, s + n))
    return {
        "single": [(100, 9000)],
        "fifty_uneven_with_empty": fifty,
        "smaller_than_a_slice": [(7777, 7877)],
        "spans_many_slices": [(3, FILE_BYTES)],
        "exact_multiple": [(10, 10 + 3 * SLICE), (50000, 50000 + 2 * SLICE)],
        "one_byte_over": [(10, 10 + 3 * SLICE), (50000, 50000 + 2 * SLICE + 1)],
        "adjacent": [(100, 5000), (5000, 5001), (5001, 20000), (20000, 20000),
                     (20000, 33333), (40000, 41000), (41000, 47000)],
        "out_of_file_order": [(5000, 9000), (100, 5000)],
        "empty": [],
    }


SHAPES = _range_shapes()


def test_coalesce_keeps_the_bytes_and_the_order():
    assert G._coalesce(SHAPES["adjacent"]) == [(100, 33333), (40000, 47000)]
    assert G._coalesce(SHAPES["out_of_file_order"]) == SHAPES["out_of_file_order"]
    assert G._coalesce([(5, 5)]) == []
    for rs in SHAPES.values():
        merged = G._coalesce(rs)
        assert sum(e - s for s, e in merged) == sum(e - s for s, e in rs)
        assert all(e > s for s, e in merged)


def test_switch_defaults_on_and_cpu_keeps_the_python_reader(monkeypatch):
    from sail_amd.config import DEFAULTS

    assert DEFAULTS["sail.io.native_reader"] == "on"
    monkeypatch.delenv("SAIL_IO_NATIVE_READER", raising=False)
    assert G.native_reader_enabled()
    for v in ("off", "0", "false", "OFF"):
        monkeypatch.setenv("SAIL_IO_NATIVE_READER", v)
        assert not G.native_reader_enabled()
    monkeypatch.setenv("SAIL_IO_NATIVE_READER", "on")
    assert G._native_reader("cpu") is None


def test_cpu_upload_is_the_python_reader(tmp_path, monkeypatch):
    monkeypatch.delenv("SAIL_IO_NATIVE_READER", raising=False)
    p = str(tmp_path / "bytes.bin")
    body = np.random.default_rng(3).integers(0, 256, 20000, dtype=np.uint8)
    body.tofile(p)
    buf, offs = G._upload_ranges(p, [(10, 5000), (9000, 9100)], "cpu")
    want = np.concatenate([body[10:5000], body[9000:9100], np.zeros(16, np.uint8)])
    assert offs == [0, 4990] and np.array_equal(buf.numpy(), want)


# ---------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def seeded_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("native_reader") / "bytes.bin")
    np.random.default_rng(11).integers(0, 256, FILE_BYTES, dtype=np.uint8).tofile(p)
    return p


@pytest.fixture()
def small_ring():
    from sail_amd.ops import kernels

    ext = kernels.require()
    torch.cuda.synchronize()
    ext.pq_reader_configure(threads=8, slice_bytes=SLICE, slots=2)
    yield ext
    torch.cuda.synchronize()
    ext.pq_reader_configure()  # back to the environment's


def _python_upload(monkeypatch, path, ranges):
    monkeypatch.setenv("SAIL_IO_NATIVE_READER", "off")
    buf, offs = G._upload_ranges(path, ranges, "cuda:0")
    torch.cuda.synchronize()
    return buf.cpu(), offs


@pytest.mark.gpu
def test_gpu_range_shapes_match_the_python_reader(seeded_file, small_ring, monkeypatch):
    want = {k: _python_upload(monkeypatch, seeded_file, rs) for k, rs in SHAPES.items()}
    monkeypatch.setenv("SAIL_IO_NATIVE_READER", "on")
    assert G._native_reader("cuda:0") is small_ring
    for k, rs in SHAPES.items():
        buf, offs = G._upload_ranges(seeded_file, rs, "cuda:0")
        torch.cuda.synchronize()
        exp, exp_offs = want[k]
        assert offs == exp_offs, k
        assert buf.dtype == torch.uint8 and buf.numel() == exp.numel(), k
        assert torch.equal(buf.cpu(), exp), k
        assert not buf[-16:].any().item(), k
    info = small_ring.pq_reader_info()
    assert info == [8, SLICE, 2, 2 * SLICE]  # the pinned footprint is the ring


@pytest.mark.gpu
def test_gpu_two_calls_without_a_synchronize_reuse_the_slots(seeded_file, small_ring,
                                                            monkeypatch):
    a, b = [(3, FILE_BYTES)], [(20000, 90000), (5, 4000)]
    want_a, _ = _python_upload(monkeypatch, seeded_file, a)
    want_b, _ = _python_upload(monkeypatch, seeded_file, b)
    cs = torch.cuda.Stream()
    da = torch.full((want_a.numel(),), 0xAB, dtype=torch.uint8, device="cuda:0")
    db = torch.full((want_b.numel(),), 0xAB, dtype=torch.uint8, device="cuda:0")
    cs.wait_stream(torch.cuda.current_stream())
    n_a = small_ring.pq_read_ranges(seeded_file, a, da, cs.cuda_stream)
    n_b = small_ring.pq_read_ranges(seeded_file, b, db, cs.cuda_stream)
    cs.synchronize()
    assert n_a == want_a.numel() - 16 and n_b == want_b.numel() - 16
    assert torch.equal(da.cpu(), want_a)
    assert torch.equal(db.cpu(), want_b)


@pytest.mark.gpu
def test_gpu_errors_leave_the_reader_usable(seeded_file, small_ring, monkeypatch):
    cs = torch.cuda.Stream()
    dst = torch.zeros(40000 + 16, dtype=torch.uint8, device="cuda:0")
    cs.wait_stream(torch.cuda.current_stream())
    with pytest.raises(RuntimeError, match="end of file"):
        small_ring.pq_read_ranges(seeded_file, [(FILE_BYTES - 30000, FILE_BYTES + 10000)],
                                  dst, cs.cuda_stream)
    with pytest.raises(RuntimeError, match="cannot open"):
        small_ring.pq_read_ranges(seeded_file + ".missing", [(0, 10)], dst, cs.cuda_stream)
    with pytest.raises(RuntimeError, match="dst holds"):
        small_ring.pq_read_ranges(seeded_file, [(0, 40001)], dst, cs.cuda_stream)
    with pytest.raises(RuntimeError, match="bad range"):
        small_ring.pq_read_ranges(seeded_file, [(10, 5)], dst, cs.cuda_stream)
    cs.synchronize()
    want, _ = _python_upload(monkeypatch, seeded_file, [(100, 9000)])
    monkeypatch.setenv("SAIL_IO_NATIVE_READER", "on")
    buf, _ = G._upload_ranges(seeded_file, [(100, 9000)], "cuda:0")
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), want)


@pytest.mark.gpu
def test_gpu_replaced_file_is_read_anew(tmp_path, small_ring, monkeypatch):
    monkeypatch.setenv("SAIL_IO_NATIVE_READER", "on")
    p = str(tmp_path / "swap.bin")
    for fill in (1, 2):
        np.full(9000, fill, np.uint8).tofile(p)
        small_ring.pq_reader_invalidate(os.path.abspath(p))
        buf, _ = G._upload_ranges(p, [(0, 9000)], "cuda:0")
        torch.cuda.synchronize()
        assert int(buf[:9000].min()) == fill and int(buf[:9000].max()) == fill


def _write_parquet(path):
    rng = np.random.default_rng(17)
    n = 20_000
    words = np.array(["alpha", "beta", "gamma", "delta", "epsilon", ""])
    t = pa.table({
        "k64": pa.array(np.cumsum(rng.integers(0, 1 << 20, n)) - 10**12),
        "d32": pa.array(rng.integers(8000, 12000, n).astype("datetime64[D]"),
                        pa.date32()),
        "s": pa.array(words[rng.integers(0, len(words), n)],
                      mask=rng.random(n) < 0.1),
    })
    w = pq.ParquetWriter(path, t.schema, compression="NONE",
                         use_dictionary=["s"], data_page_size=4096,
                         data_page_version="1.0",
                         column_encoding={"k64": "DELTA_BINARY_PACKED",
                                          "d32": "DELTA_BINARY_PACKED"})
    try:
        w.write_table(t, row_group_size=10_000)
    finally:
        w.close()
    return t


def _tensors(col):
    return {k: getattr(col, k) for k in ("data", "validity", "offsets", "bytes_", "codes")
            if getattr(col, k, None) is not None}


@pytest.mark.gpu
def test_gpu_parquet_file_equal_with_the_switch_on_and_off(tmp_path, small_ring,
                                                           monkeypatch):
    p = str(tmp_path / "small.parquet")
    src = _write_parquet(p)
    assert pq.ParquetFile(p).metadata.num_row_groups == 2
    schema = [(n, None) for n in src.schema.names]
    tables = {}
    for switch in ("off", "on"):
        monkeypatch.setenv("SAIL_IO_NATIVE_READER", switch)
        tables[switch] = G.read_gpu([p], schema, "cuda:0")
        torch.cuda.synchronize()
    for name in src.schema.names:
        off, on = _tensors(tables["off"].columns[name]), _tensors(tables["on"].columns[name])
        assert set(off) == set(on), name
        for k in off:
            assert off[k].dtype == on[k].dtype and torch.equal(off[k], on[k]), (name, k)
    got = tables["on"].columns["k64"].data.cpu().numpy()
    assert np.array_equal(got, src.column("k64").to_numpy())
    assert tables["on"].columns["s"].to_pylist() == src.column("s").to_pylist()
