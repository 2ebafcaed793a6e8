"""Measurement: device decode against the host path for the page layouts
that used to fall back — BOOLEAN, INT96 timestamps, BYTE_STREAM_SPLIT and
v2 data pages.

Writes one uncompressed parquet file with data_page_version="2.0":

  flag   BOOLEAN (RLE in v2 pages), 5 % nulls
  ts     INT96 timestamp (Spark's default), dictionary then PLAIN fallback
  price  DOUBLE, BYTE_STREAM_SPLIT
  key    INT64, stock encoding (dictionary, then PLAIN fallback)
  mode   low-cardinality string, RLE_DICTIONARY, 5 % nulls

and times scans of it into device memory with gpuDecode=force (the page
decoders) and gpuDecode=off (pyarrow on the host, then upload), for the
whole table and for each column alone, so a layout where the device path
loses shows by name.

Method: page cache warm (the file is read once first), --warmup scans,
then the median of --runs scans, device synchronised before the clock
starts and before it stops. Before timing, the two paths' tables are
compared exactly.

Usage: python tools/parquet_types_scan_bench.py [--rows 4000000] [--runs 7]
Prints one JSON line last.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sail_amd.datasource import gpu_parquet as G  # noqa: E402
from sail_amd.datasource import parquet_io  # noqa: E402
from sail_amd.engine.column import StringColumn  # noqa: E402

DEV = "cuda:0"


def _write(path, nrows):
    rng = np.random.default_rng(17)
    lo = int(np.datetime64("1990-01-01", "us").astype(np.int64))
    hi = int(np.datetime64("2030-01-01", "us").astype(np.int64))
    modes = np.array(["AIR", "FOB", "MAIL", "RAIL", "SHIP", "TRUCK", "REG AIR"])
    t = pa.table({
        "flag": pa.array(rng.random(nrows) < 0.5,
                         mask=rng.random(nrows) < 0.05),
        "ts": pa.array(rng.integers(lo, hi, nrows).astype("datetime64[us]"),
                       pa.timestamp("us")),
        "price": pa.array(np.round(rng.random(nrows) * 1e5, 2)),
        "key": pa.array(rng.integers(0, 10**12, nrows)),
        "mode": pa.array(modes[rng.integers(0, len(modes), nrows)],
                         mask=rng.random(nrows) < 0.05),
    })
    pq.write_table(t, path, compression="NONE", data_page_version="2.0",
                   use_deprecated_int96_timestamps=True,
                   use_dictionary=["ts", "key", "mode"],
                   column_encoding={"price": "BYTE_STREAM_SPLIT"})


def _layout(path):
    """Per column: physical type, pages, encodings seen (from the index)."""
    idx = G.file_index(path)
    out = {}
    for ci in range(len(idx.schema)):
        sc = idx.schema.column(ci)
        pages = [p for ch in idx.chunks(ci) for p in ch.pages]
        out[sc.name] = {"physical": sc.physical_type, "pages": len(pages),
                        "v2": all(p.ndense is not None for p in pages),
                        "encodings": sorted({p.enc for p in pages})}
    return out


def _timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def _same(a, b):
    if len(a) != len(b) or a.dtype != b.dtype:
        return False
    if isinstance(a, StringColumn):
        idx = torch.from_numpy(
            np.random.default_rng(3).integers(0, len(a), 20_000)).to(DEV)
        return a.gather(idx).to_pylist() == b.gather(idx).to_pylist()
    va = None if a.validity is None else a.validity.to(torch.bool)
    vb = None if b.validity is None else b.validity.to(torch.bool)
    if (va is None) != (vb is None) or (va is not None
                                        and not torch.equal(va, vb)):
        return False
    da, db = a.data, b.data
    if da.dtype != db.dtype:
        return False
    if da.dtype.is_floating_point:
        da, db = da.view(torch.int64), db.view(torch.int64)
    if va is not None:
        da, db = da[va], db[va]
    return bool(torch.equal(da, db))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("parquet_types_scan_bench needs a GPU: timings "
                         "taken anywhere else say nothing about the scan path")
    out_dir = args.dir or tempfile.mkdtemp(prefix="sail_types_bench_")
    path = os.path.join(out_dir, "types-v2.parquet")
    _write(path, args.rows)
    with open(path, "rb") as f:          # warm the page cache
        while f.read(64 << 20):
            pass
    layout = _layout(path)
    schema_all = parquet_io.infer_schema([path])
    print(f"rows {args.rows}; file {os.path.getsize(path) / 1e6:.1f} MB; "
          f"layout {layout}", flush=True)

    def scan(schema, mode):
        return parquet_io.read([path], schema, DEV, {"gpuDecode": mode})

    dev_t, host_t = scan(schema_all, "force"), scan(schema_all, "off")
    for name, _ in schema_all:
        if not _same(dev_t.columns[name], host_t.columns[name]):
            raise SystemExit(f"column {name}: device decode differs from "
                             "the host path")
    del dev_t, host_t
    torch.cuda.empty_cache()

    res = {}
    for label, schema in [("all", schema_all)] + [
            (n, [(n, t)]) for n, t in schema_all]:
        row = {}
        for mode in ("force", "off"):
            med, lo, hi = _timed(lambda: scan(schema, mode), args.warmup,
                                 args.runs)
            row[mode] = {"median_ms": round(med * 1e3, 2),
                         "min_ms": round(lo * 1e3, 2),
                         "max_ms": round(hi * 1e3, 2)}
        row["host_over_device"] = round(
            row["off"]["median_ms"] / row["force"]["median_ms"], 2)
        res[label] = row
        print(f"{label:6s} device {row['force']['median_ms']:8.2f} ms "
              f"({row['force']['min_ms']:.2f}-{row['force']['max_ms']:.2f})  "
              f"host {row['off']['median_ms']:8.2f} ms "
              f"({row['off']['min_ms']:.2f}-{row['off']['max_ms']:.2f})  "
              f"host/device {row['host_over_device']:.2f}x", flush=True)

    print(json.dumps({
        "tool": "parquet_types_scan_bench", "rows": args.rows,
        "runs": args.runs, "warmup": args.warmup,
        "file_mb": round(os.path.getsize(path) / 1e6, 1),
        "layout": layout, "scan_ms": res,
        "device_loses": [k for k, v in res.items()
                         if v["host_over_device"] < 1.0],
    }))


if __name__ == "__main__":
    main()
