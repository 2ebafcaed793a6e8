"""Measurement: DELTA_BYTE_ARRAY string columns, device decode against the
host path, and pq_dba_expand alone.

Writes --rows rows with pq.write_table(compression="NONE",
use_dictionary=False, column_encoding=DELTA_BYTE_ARRAY). Columns:

  url   sorted, 69 bytes, long shared prefixes (section and item numbers
        under one site)
  text  unsorted word text of 10-43 bytes: prefixes of a byte or two
  key   sorted 10-byte keys

1. Scans: per column, gpuDecode=force against gpuDecode=off (pyarrow on the
   host, then upload), alternating in one process: --warmup scans each, then
   the median and range of --runs, device synchronised before the clock
   starts and stops. Before timing the two paths' columns are compared
   exactly (validity, lengths, bytes).
2. Kernels, device events, on each column's uploaded buffer: pq_dba_lengths
   and pq_dba_expand. GB/s is value bytes (the sum of the lengths) over time.
3. `switch_default`: "on" when on every column the device median beats the
   host median by more than the host's own min-max spread, else "off" with
   the losing columns.

There is no CPU arm: without a GPU the tool stops.

Usage: python tools/dba_scan_bench.py [--rows 4000000] [--runs 7]
Prints one JSON line last.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from string_scan_bench import (  # noqa: E402
    DEV, _canonical, _corpus, _event_pair, _ms, _strings, _timed_pair)

from sail_amd.datasource import gpu_parquet as G  # noqa: E402
from sail_amd.datasource import parquet_io  # noqa: E402

COLUMNS = ("url", "text", "key")


def _fixed(parts, n):
    """pa.string() array of n fixed-width values: `parts` are byte strings
    and (int64 array, digits) pairs, laid side by side."""
    width = sum(len(p) if isinstance(p, bytes) else p[1] for p in parts)
    out = np.empty((n, width), dtype=np.uint8)
    at = 0
    for p in parts:
        if isinstance(p, bytes):
            out[:, at:at + len(p)] = np.frombuffer(p, dtype=np.uint8)
            at += len(p)
        else:
            vals, digits = p
            for d in range(digits):
                out[:, at + d] = 48 + (vals // 10 ** (digits - 1 - d)) % 10
            at += digits
    return _strings(out.reshape(-1), np.full(n, width, dtype=np.int32))


def _table(nrows, seed=31, piece=500_000):
    rng = np.random.default_rng(seed)
    corpus = _corpus(rng, 1 << 20)
    item = np.sort(rng.integers(0, 10**12, nrows))     # (section, item), sorted
    key = np.sort(rng.integers(0, 10**9, nrows))
    urls, texts, keys = [], [], []
    for lo in range(0, nrows, piece):
        n = min(piece, nrows - lo)
        it = item[lo:lo + n]
        urls.append(_fixed([b"https://www.example.com/catalog/section-",
                            (it // 10**9, 3), b"/item-", (it % 10**9, 9),
                            b"/index.html"], n))
        ln = rng.integers(10, 44, n).astype(np.int32)
        start = rng.integers(0, len(corpus) - 64, n).astype(np.int32)
        offs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(ln, out=offs[1:])
        idx = np.repeat(start - offs[:-1], ln) + np.arange(offs[-1], dtype=np.int32)
        texts.append(_strings(corpus[idx], ln))
        keys.append(_fixed([b"k", (key[lo:lo + n], 9)], n))
    return pa.table({"url": pa.chunked_array(urls),
                     "text": pa.chunked_array(texts),
                     "key": pa.chunked_array(keys)})


def _scan(path, name, typ, mode):
    return parquet_io.read([path], [(name, typ)], DEV, {"gpuDecode": mode})


def _kernels(path, column, warmup, runs, ext):
    dec = G._ColumnDecoder(G.file_index(path), column, DEV, snappy=False)
    dec.upload()
    _, dense_counts = dec.decode_validity()
    n = sum(dense_counts)
    table = G._page_table(dec._value_rows(dense_counts), DEV)
    buf = dec.buf
    prefix, suffix, lengths, sstart, status = ext.pq_dba_lengths(buf, table, n)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(lengths, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    blob = torch.empty(total, dtype=torch.uint8, device=DEV)
    t = _event_pair({
        "pq_dba_lengths": lambda: ext.pq_dba_lengths(buf, table, n),
        "pq_dba_expand": lambda: ext.pq_dba_expand(
            buf, table, prefix, suffix, sstart, offsets, lengths, status, blob),
    }, warmup, runs)
    if int(status.abs().sum().item()):
        raise SystemExit(f"{column}: a page was rejected")
    out = {"pages": int(table.shape[0]), "values": n, "value_bytes": total}
    for k, v in t.items():
        out[k] = dict(_ms(v, 1.0), gb_per_s=round(total / v[0] / 1e6, 2))
        print(f"  {column:5s} {k:15s} {v[0]:9.3f} ms ({v[1]:.3f}-{v[2]:.3f})  "
              f"{out[k]['gb_per_s']:8.2f} GB/s of value bytes", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dba_scan_bench needs a GPU: timings taken anywhere "
                         "else say nothing about the scan path")
    from sail_amd.ops import kernels

    ext = kernels.require()
    path = os.path.join(args.dir or tempfile.mkdtemp(prefix="sail_dba_bench_"),
                        "dba-none.parquet")
    pq.write_table(_table(args.rows), path, compression="NONE",
                   use_dictionary=False,
                   column_encoding={c: "DELTA_BYTE_ARRAY" for c in COLUMNS})
    with open(path, "rb") as f:          # warm the page cache
        while f.read(64 << 20):
            pass
    schema = dict(parquet_io.infer_schema([path]))
    res = {"tool": "dba_scan_bench", "rows": args.rows, "runs": args.runs,
           "warmup": args.warmup, "file_mb": round(os.path.getsize(path) / 1e6, 1),
           "scan_ms": {}, "kernels": {}}
    losing = []
    for name in COLUMNS:
        a = _canonical(_scan(path, name, schema[name], "force").columns[name], ext)
        b = _canonical(_scan(path, name, schema[name], "off").columns[name], ext)
        if not all(torch.equal(x, y) for x, y in zip(a, b)):
            raise SystemExit(f"column {name}: device decode differs from the "
                             "host path")
        del a, b
        torch.cuda.empty_cache()
        t = _timed_pair(
            {"force": lambda: _scan(path, name, schema[name], "force"),
             "off": lambda: _scan(path, name, schema[name], "off")},
            args.warmup, args.runs)
        row = {k: _ms(v) for k, v in t.items()}
        row["host_over_device"] = round(t["off"][0] / t["force"][0], 2)
        res["scan_ms"][name] = row
        if not t["off"][0] - t["force"][0] > t["off"][2] - t["off"][1]:
            losing.append(name)
        print(f"  {name:5s} device {row['force']['median_ms']:9.2f} ms "
              f"({row['force']['min_ms']:.2f}-{row['force']['max_ms']:.2f})  "
              f"host {row['off']['median_ms']:9.2f} ms "
              f"({row['off']['min_ms']:.2f}-{row['off']['max_ms']:.2f})  "
              f"host/device {row['host_over_device']:.2f}x", flush=True)
    print("kernels on each column's upload:", flush=True)
    for name in COLUMNS:
        res["kernels"][name] = _kernels(path, name, args.warmup, args.runs, ext)
    res["switch_default"] = "off" if losing else "on"
    res["device_loses"] = losing
    print(json.dumps(res))


if __name__ == "__main__":
    main()
