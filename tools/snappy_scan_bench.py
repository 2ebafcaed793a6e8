"""Measurement: what does the opt-in device Snappy path (sail.io.gpu_snappy)
buy on a stock pyarrow file?

Writes TPC-H `lineitem` twice, as the project's uncompressed shard
(datagen/tpch.py encodings) and as pq.write_table(table, path) with no
arguments (Snappy, dictionary with PLAIN fallback), then times three scans
of the same columns into device memory:

  host   stock file, switch off: GPU decode refuses the codec and the scan
         falls back to pyarrow + upload (what happens without the switch)
  snappy stock file, gpuDecode=force + gpuSnappy=on
  plain  uncompressed shard, gpuDecode=force (context)

Method: page cache warm (each file is read once first), 2 warm-up scans,
then the median of --runs scans, device synchronised before the clock
starts and before it stops. The Snappy kernel's own rate comes from a
separate scan with device events around every pq_snappy_decompress call
(decompressed bytes / summed kernel-call time). Columns the GPU path cannot
decode from the stock file are listed and left out of all three scans.

Usage: python tools/snappy_scan_bench.py [--sf 1] [--runs 5] [--dir DIR]
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
import pyarrow.parquet as pq
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sail_amd.datagen.tpch import TpchGenerator, write_tpch_parquet  # noqa: E402
from sail_amd.datasource import gpu_parquet as G  # noqa: E402
from sail_amd.datasource import parquet_io  # noqa: E402
from sail_amd.engine.column import StringColumn  # noqa: E402

DEV = "cuda:0"


class _TimedExt:
    """The kernel extension with device events around pq_snappy_decompress."""

    def __init__(self, ext):
        self._ext = ext
        self.events = []
        self.out_bytes = 0
        self.in_bytes = 0

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def pq_snappy_decompress(self, buf, pages, out):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        st = self._ext.pq_snappy_decompress(buf, pages, out)
        b.record()
        self.events.append((a, b))
        self.out_bytes += out.numel() - 16
        self.in_bytes += int(pages[:, 1].sum().item())
        return st


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


def _same(gpu_col, host_col, rng):
    if len(gpu_col) != len(host_col):
        return False
    if isinstance(gpu_col, StringColumn):
        idx = torch.from_numpy(rng.integers(0, len(gpu_col), 20_000)).to(DEV)
        return gpu_col.gather(idx).to_pylist() == host_col.gather(idx).to_pylist()
    return bool(torch.equal(gpu_col.data, host_col.data.to(gpu_col.data.dtype)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--full", action="store_true",
                    help="include l_comment (the benchmark's --full shards)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("snappy_scan_bench needs a GPU: timings taken "
                         "anywhere else say nothing about the scan path")
    out_dir = args.dir or tempfile.mkdtemp(prefix="sail_snappy_bench_")

    gen = TpchGenerator(sf=args.sf, device=DEV, seed=42, rank=0, world=1,
                        full=args.full)
    shard = write_tpch_parquet({"lineitem": gen.lineitem()}, out_dir)["lineitem"]
    del gen
    torch.cuda.empty_cache()
    stock = os.path.join(out_dir, "lineitem-stock.parquet")
    pq.write_table(pq.read_table(shard), stock)
    md = pq.ParquetFile(stock).metadata
    assert md.row_group(0).column(0).compression == "SNAPPY"
    nrows = md.num_rows

    # which columns the device path takes from the stock file, and that it
    # decodes them to what pyarrow reads
    rng = np.random.default_rng(3)
    schema_all = parquet_io.infer_schema([stock])
    schema, skipped = [], {}
    for name, typ in schema_all:
        try:
            g = G.read_gpu([stock], [(name, typ)], DEV, snappy=True)
        except G.Unsupported as e:
            skipped[name] = str(e)
            continue
        h = parquet_io.read([stock], [(name, typ)], DEV, {"gpuDecode": "off"})
        if not _same(g.columns[name], h.columns[name], rng):
            raise SystemExit(f"column {name}: device decode differs from pyarrow")
        schema.append((name, typ))
    del g, h
    torch.cuda.empty_cache()
    print(f"rows {nrows}; timed columns {len(schema)}/{len(schema_all)}; "
          f"skipped {skipped}", flush=True)

    def host():
        return parquet_io.read([stock], schema, DEV, {"gpuSnappy": "off"})

    def snappy():
        return parquet_io.read([stock], schema, DEV,
                               {"gpuDecode": "force", "gpuSnappy": "on"})

    def plain():
        return parquet_io.read([shard], schema, DEV, {"gpuDecode": "force"})

    res = {}
    for label, fn in (("host", host), ("snappy", snappy), ("plain", plain)):
        med, lo, hi = _timed(fn, args.warmup, args.runs)
        res[label] = {"median_s": round(med, 4), "min_s": round(lo, 4),
                      "max_s": round(hi, 4)}
        print(f"{label:7s} median {med * 1e3:8.1f} ms  "
              f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)

    # the kernel alone
    timed = _TimedExt(G._ext())
    real = G._ext
    G._ext = lambda: timed
    try:
        snappy()
        torch.cuda.synchronize()
    finally:
        G._ext = real
    ms = sum(a.elapsed_time(b) for a, b in timed.events)
    gbps = timed.out_bytes / (ms * 1e-3) / 1e9 if ms else 0.0
    print(f"kernel  {len(timed.events)} launches, {timed.in_bytes / 1e6:.1f} MB"
          f" -> {timed.out_bytes / 1e6:.1f} MB in {ms:.2f} ms = {gbps:.1f} "
          "GB/s decompressed", flush=True)

    print(json.dumps({
        "tool": "snappy_scan_bench", "sf": args.sf, "rows": nrows,
        "runs": args.runs, "warmup": args.warmup,
        "columns": [n for n, _ in schema], "skipped": skipped,
        "stock_file_mb": round(os.path.getsize(stock) / 1e6, 1),
        "shard_file_mb": round(os.path.getsize(shard) / 1e6, 1),
        "scan": res,
        "kernel": {"launches": len(timed.events),
                   "compressed_mb": round(timed.in_bytes / 1e6, 1),
                   "decompressed_mb": round(timed.out_bytes / 1e6, 1),
                   "ms": round(ms, 3), "decompressed_gb_s": round(gbps, 2),
                   "launch_ms": [round(a.elapsed_time(b), 2)
                                 for a, b in timed.events]},
    }))


if __name__ == "__main__":
    main()
