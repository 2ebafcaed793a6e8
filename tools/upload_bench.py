"""Measurement: how a column's chunk bytes get from the file into device
memory. The Python reader of datasource/gpu_parquet.py (a thread pool that
fills one column-sized pinned buffer, then one copy) against the
extension's pipelined reader (pq_read_ranges: pread into a ring of pinned
slices, each copied as it completes), with the two floors either of them
has: the threaded read alone and the copy alone.

Generates TPC-H at --sf (default 10: 60M lineitem rows), writes the
lineitem shard as bench.py does, warms the page cache, and for l_orderkey,
l_extendedprice and l_shipdate times, --warmup rounds and then the median
and min-max of --runs:

  read8, read16   the thread-pool read of the column's ranges into an
                  already allocated pinned buffer, 8 and 16 threads (host
                  clock);
  copy            one H2D copy of that filled pinned buffer (device events);
  python          _upload_ranges with SAIL_IO_NATIVE_READER=off (host clock
                  around a device synchronise);
  native          _upload_ranges with the switch on, same clock;
  native16        the same with 16 reader threads;
  nread, nread16  the extension reader's file read alone, bytes dropped
                  (pq_reader_read_only), 8 and 16 threads.

python and native alternate within a round. Before anything is timed the
two device buffers are compared byte for byte, the 16-byte zero tail
included. floor = max(read8, copy) is what a reader that hides the shorter
half entirely would take with 8 threads of the Python read.

--sweep threads:slice_mib:slots,... times the native upload of each column
under other ring configurations (median of --runs each).

Usage: python tools/upload_bench.py [--sf 10] [--runs 7] [--warmup 2]
           [--sweep 8:4:16,16:8:8]
Prints one JSON line last.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from sail_amd.datasource import gpu_parquet as G  # noqa: E402

DEV = "cuda:0"
COLUMNS = ("l_orderkey", "l_extendedprice", "l_shipdate")


def _stats(ts):
    return {"median_ms": round(statistics.median(ts), 3),
            "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    del out
    return dt


def _threaded_read(path, ranges, view, nthreads):
    """The read half of the Python reader, as _upload_ranges does it."""
    jobs, pos = [], 0
    for s, e in ranges:
        jobs.append((s, e, pos))
        pos += e - s

    def one(job):
        s, e, at = job
        with open(path, "rb") as f:
            f.seek(s)
            got = f.readinto(memoryview(view)[at:at + (e - s)])
        if got != e - s:
            raise IOError(f"short read in {path}")

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(nthreads, len(jobs))) as pool:
        list(pool.map(one, jobs))
    return (time.perf_counter() - t0) * 1e3


def _copy_ms(stage, total, dst):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    dst.copy_(stage[:total], non_blocking=True)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _upload(path, ranges, switch):
    os.environ["SAIL_IO_NATIVE_READER"] = switch
    return G._upload_ranges(path, ranges, DEV)[0]


def measure(ext, idx, path, name, warmup, runs, sweep=()):
    dec = G._ColumnDecoder(idx, name, DEV)
    ranges = [(ch.start, ch.end) for ch in dec.chunks]
    total = sum(e - s for s, e in ranges)

    a, b = _upload(path, ranges, "off"), _upload(path, ranges, "on")
    torch.cuda.synchronize()
    if a.numel() != total + 16 or not torch.equal(a, b) or bool(b[total:].any()):
        raise SystemExit(f"{name}: the native reader's bytes differ")
    del a, b

    stage = torch.empty(total + 16, dtype=torch.uint8, pin_memory=True)
    view = stage.numpy()
    dst = torch.empty(total, dtype=torch.uint8, device=DEV)
    variants = [
        ("read8", lambda: _threaded_read(path, ranges, view, 8)),
        ("read16", lambda: _threaded_read(path, ranges, view, 16)),
        ("copy", lambda: _copy_ms(stage, total, dst)),
        ("python", lambda: _host_ms(lambda: _upload(path, ranges, "off"))),
        ("native", lambda: _host_ms(lambda: _upload(path, ranges, "on"))),
        ("nread", lambda: _host_ms(lambda: ext.pq_reader_read_only(path, ranges))),
    ]
    times = {k: [] for k, _ in variants}
    for i in range(warmup + runs):
        for k, fn in variants:
            t = fn()
            if i >= warmup:
                times[k].append(t)
    # 16 reader threads: the ring is rebuilt, so in rounds of its own
    torch.cuda.synchronize()
    ext.pq_reader_configure(threads=16)
    times["native16"], times["nread16"] = [], []
    for i in range(warmup + runs):
        t = _host_ms(lambda: _upload(path, ranges, "on"))
        r = _host_ms(lambda: ext.pq_reader_read_only(path, ranges))
        if i >= warmup:
            times["native16"].append(t)
            times["nread16"].append(r)
    swept = {}
    for cfg in sweep:
        th, mib, slots = (int(x) for x in cfg.split(":"))
        torch.cuda.synchronize()
        ext.pq_reader_configure(threads=th, slice_bytes=mib << 20, slots=slots)
        ts = [_host_ms(lambda: _upload(path, ranges, "on"))
              for _ in range(warmup + runs)][warmup:]
        swept[cfg] = _stats(ts)
    torch.cuda.synchronize()
    ext.pq_reader_configure()
    os.environ.pop("SAIL_IO_NATIVE_READER", None)

    row = {"ranges": len(ranges), "bytes": total}
    for k, ts in times.items():
        row[k] = _stats(ts)
        row[k]["gb_s"] = round(total / (row[k]["median_ms"] * 1e-3) / 1e9, 1)
    if swept:
        row["sweep"] = swept
    row["floor_ms"] = max(row["read8"]["median_ms"], row["copy"]["median_ms"])
    row["native_over_floor"] = round(row["native"]["median_ms"] / row["floor_ms"], 2)
    row["speedup"] = round(row["python"]["median_ms"] / row["native"]["median_ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--sweep", default="",
                    help="threads:slice_mib:slots,... extra ring configurations")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("upload_bench needs a GPU: timings taken anywhere "
                         "else say nothing about the upload path")
    from sail_amd.datagen.tpch import TpchGenerator, write_tpch_parquet
    from sail_amd.ops import kernels

    ext = kernels.require()
    if not hasattr(ext, "pq_read_ranges"):
        raise SystemExit("the extension has no pq_read_ranges: rebuild it")
    out_dir = args.dir or tempfile.mkdtemp(prefix="sail_upload_bench_")
    t0 = time.time()
    tables = TpchGenerator(sf=args.sf, device=DEV).generate_all()
    path = write_tpch_parquet({"lineitem": tables["lineitem"]}, out_dir)["lineitem"]
    del tables
    torch.cuda.empty_cache()
    with open(path, "rb") as f:          # warm the page cache
        while f.read(64 << 20):
            pass
    idx = G.file_index(path)
    info = ext.pq_reader_info()
    print(f"# sf {args.sf:g}: {idx.num_rows} rows, "
          f"{os.path.getsize(path) / 1e9:.2f} GB, setup {time.time() - t0:.1f}s; "
          f"reader: {info[0]} threads, {info[1] >> 20} MiB slices, {info[2]} slots",
          flush=True)

    res = {}
    for name in COLUMNS:
        row = measure(ext, idx, path, name, args.warmup, args.runs,
                      [c for c in args.sweep.split(",") if c])
        res[name] = row
        print(f"{name:16s} {row['ranges']} ranges, {row['bytes'] / 1e6:.1f} MB", flush=True)
        for k in ("read8", "read16", "copy", "python", "native", "native16",
                  "nread", "nread16"):
            v = row[k]
            print(f"  {k:9s} {v['median_ms']:8.3f} ms ({v['min_ms']:.3f}-{v['max_ms']:.3f}) "
                  f"{v['gb_s']:6.1f} GB/s", flush=True)
        for cfg, v in row.get("sweep", {}).items():
            print(f"  native {cfg:9s} {v['median_ms']:8.3f} ms "
                  f"({v['min_ms']:.3f}-{v['max_ms']:.3f})", flush=True)
        print(f"  floor max(read8, copy) {row['floor_ms']:.3f} ms; native is "
              f"{row['native_over_floor']:.2f}x the floor, {row['speedup']:.2f}x "
              f"faster than python", flush=True)
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "upload_bench", "sf": args.sf, "rows": idx.num_rows,
                      "runs": args.runs, "warmup": args.warmup,
                      "reader": {"threads": info[0], "slice_bytes": info[1],
                                 "slots": info[2]},
                      "columns": res}))


if __name__ == "__main__":
    main()
