"""Measurement: the fused DELTA_BINARY_PACKED decode (pq_delta_values)
against the path it replaces (pq_delta_decode + pq_segscan + cast), on the
lineitem shard the benchmark writes.

Generates TPC-H at --sf (default 10: 60M lineitem rows), writes the
lineitem shard as bench.py does, and for l_orderkey (narrow deltas),
l_extendedprice (wide) and l_shipdate (INT32):

1. Kernel A/B in one process: the column's chunks are uploaded once and
   both paths decode that same buffer with the same page table, timed with
   device events, alternating old and new: --warmup rounds, then the median
   and min-max of --runs. Outputs are compared exactly first. Bytes are
   computed from shapes: the new path reads the packed pages and writes the
   values once; the old one also zero-fills, writes and re-reads the int64
   deltas, and casts INT32 columns. GB/s is those bytes over the median;
   the share is against 6.3 TB/s.
2. Whole-column scans (file read, upload, decode), host clock around a
   device synchronise, page cache warm: SAIL_IO_GPU_DELTA_FUSED on and off,
   page-table cache warm and cold (cold: the tables are dropped before every
   scan). The upload alone (file read + H2D) is timed too, so the host time
   outside it can be read off.

Usage: python tools/delta_scan_bench.py [--sf 10] [--runs 7] [--warmup 2]
Prints one JSON line last.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sail_amd.datasource import gpu_parquet as G  # noqa: E402

DEV = "cuda:0"
HBM = 6.3e12
COLUMNS = ("l_orderkey", "l_extendedprice", "l_shipdate")


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 3),
            "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (time.perf_counter() - t0) * 1e3


def _kernel_ab(ext, idx, name, warmup, runs):
    dec = G._ColumnDecoder(idx, name, DEV)
    dec.upload()
    tabs, validity = dec._tables()
    assert validity is None and len(tabs.rows["delta"]) == tabs.n_pages
    table, total = tabs.dev["delta"], tabs.delta_total
    i32 = dec.physical == "INT32"

    def old():
        vals, _ = ext.pq_delta_decode(dec.buf, table, total)
        ext.pq_segscan(vals, table)
        return vals.to(torch.int32) if i32 else vals

    def new():
        return ext.pq_delta_values(dec.buf, table, total, i32)

    if not torch.equal(old(), new()):
        raise SystemExit(f"{name}: fused decode differs from the old path")
    for _ in range(warmup):
        _event_ms(old)
        _event_ms(new)
    t_old, t_new = [], []
    for _ in range(runs):
        t_old.append(_event_ms(old))
        t_new.append(_event_ms(new))
    packed = int(tabs.rows["delta"][:, 1].sum())
    w = 4 if i32 else 8
    new_bytes = packed + total * w
    # fill 8N, deltas out 8N, scan in and out 16N, cast in 8N and out 4N
    old_bytes = packed + total * (32 + (12 if i32 else 0))
    row = {"pages": tabs.n_pages, "values": total, "packed_bytes": packed,
           "old": _stats(t_old), "new": _stats(t_new),
           "old_bytes": old_bytes, "new_bytes": new_bytes}
    for k, nbytes in (("old", old_bytes), ("new", new_bytes)):
        rate = nbytes / (row[k]["median_ms"] * 1e-3)
        row[k]["gb_s"] = round(rate / 1e9, 1)
        row[k]["share_of_6.3_tb_s"] = round(rate / HBM, 3)
    row["speedup"] = round(row["old"]["median_ms"] / row["new"]["median_ms"], 2)
    return row


def _scans(idx, path, name, warmup, runs):
    schema = [(name, None)]

    def scan():
        return G.read_gpu([path], schema, DEV)

    def cold_scan():
        idx._tables.clear()
        idx._windows.clear()
        return scan()

    def upload():
        dec = G._ColumnDecoder(idx, name, DEV)
        dec.upload()
        return dec.buf

    out = {}
    variants = [("fused_warm", "on", scan), ("old_warm", "off", scan),
                ("fused_cold", "on", cold_scan), ("old_cold", "off", cold_scan),
                ("upload_only", "on", upload)]
    for _ in range(warmup):
        for _, switch, fn in variants:
            os.environ["SAIL_IO_GPU_DELTA_FUSED"] = switch
            _host_ms(fn)
    times = {k: [] for k, _, _ in variants}
    for _ in range(runs):
        for k, switch, fn in variants:
            os.environ["SAIL_IO_GPU_DELTA_FUSED"] = switch
            times[k].append(_host_ms(fn))
    os.environ.pop("SAIL_IO_GPU_DELTA_FUSED", None)
    for k in times:
        out[k] = _stats(times[k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("delta_scan_bench needs a GPU: timings taken "
                         "anywhere else say nothing about the scan path")
    from sail_amd.datagen.tpch import TpchGenerator, write_tpch_parquet
    from sail_amd.ops import kernels

    ext = kernels.require()
    out_dir = args.dir or tempfile.mkdtemp(prefix="sail_delta_bench_")
    t0 = time.time()
    tables = TpchGenerator(sf=args.sf, device=DEV).generate_all()
    path = write_tpch_parquet({"lineitem": tables["lineitem"]}, out_dir)["lineitem"]
    del tables
    torch.cuda.empty_cache()
    with open(path, "rb") as f:          # warm the page cache
        while f.read(64 << 20):
            pass
    idx = G.file_index(path)
    print(f"# sf {args.sf:g}: {idx.num_rows} rows, "
          f"{os.path.getsize(path) / 1e9:.2f} GB, setup {time.time() - t0:.1f}s",
          flush=True)

    res = {}
    for name in COLUMNS:
        row = _kernel_ab(ext, idx, name, args.warmup, args.runs)
        row["scan_ms"] = _scans(idx, path, name, args.warmup, args.runs)
        res[name] = row
        o, n = row["old"], row["new"]
        print(f"{name:16s} {row['pages']} pages, {row['packed_bytes'] / 1e6:.0f} MB "
              f"packed\n  kernels old {o['median_ms']:8.3f} ms "
              f"({o['min_ms']:.3f}-{o['max_ms']:.3f}) {o['gb_s']:7.1f} GB/s | "
              f"new {n['median_ms']:8.3f} ms ({n['min_ms']:.3f}-{n['max_ms']:.3f}) "
              f"{n['gb_s']:7.1f} GB/s = {n['share_of_6.3_tb_s']:.2f} of 6.3 TB/s | "
              f"{row['speedup']:.2f}x", flush=True)
        for k, v in row["scan_ms"].items():
            print(f"  scan {k:12s} {v['median_ms']:8.2f} ms "
                  f"({v['min_ms']:.2f}-{v['max_ms']:.2f})", flush=True)
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "delta_scan_bench", "sf": args.sf,
                      "rows": idx.num_rows, "runs": args.runs,
                      "warmup": args.warmup, "columns": res}))


if __name__ == "__main__":
    main()
