"""Measurement: string columns of stock parquet files, device decode against
the host path, and the PLAIN byte-array kernels old against new.

Writes 4,000,000 rows twice with pq.write_table and nothing else but the
compression: once as written by default (Snappy, read with gpuSnappy=on) and
once with compression="NONE". Columns:

  comment  word text of 10-43 bytes; overflows its dictionary, so each chunk
           is RLE_DICTIONARY pages followed by PLAIN pages
  url      60-120 bytes, all distinct; the same layout, almost all PLAIN
  mode     7 distinct values; stays RLE_DICTIONARY

1. Scans: per file, for the whole table and for each column alone,
   gpuDecode=force against gpuDecode=off (pyarrow on the host, then upload;
   what these files got before the mixed layout was decoded), the two
   alternating in one process: --warmup scans each, then the median and
   range of --runs, device synchronised before the clock starts and stops.
   Before timing, the two paths' tables are compared exactly (validity,
   lengths and bytes of every row).
2. Kernels, device events, on the uploaded buffer of the uncompressed file:
   pq_bytearray_walk against pq_bytearray_index over the PLAIN pages of
   `comment` and of `url`, and pq_gather_strings against pq_gather_bytes on
   their result, old and new alternating; outputs compared first. GB/s is
   value bytes (the sum of the lengths) over the time.

There is no CPU arm: without a GPU the tool stops.

Usage: python tools/string_scan_bench.py [--rows 4000000] [--runs 7]
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

DEV = "cuda:0"
WORDS = ("the quick final pending requests sleep furiously carefully along "
         "blithely ironic deposits accounts packages regular express bold "
         "foxes nag slyly above even theodolites wake across instructions "
         "platelets haggle unusual pinto beans boost silent dolphins cajole "
         "daring asymptotes integrate special dependencies").split()


def _corpus(rng, nbytes):
    words = np.array(WORDS)
    text = " ".join(words[rng.integers(0, len(words), nbytes // 5)])
    return np.frombuffer(text.encode()[:nbytes], dtype=np.uint8)


def _strings(data, lengths):
    """pa.string() array of len(lengths) values laid back to back in data."""
    offsets = np.zeros(len(lengths) + 1, dtype=np.int32)
    np.cumsum(lengths, out=offsets[1:])
    return pa.StringArray.from_buffers(
        len(lengths), pa.py_buffer(offsets), pa.py_buffer(data))


def _table(nrows, seed=29, piece=500_000):
    rng = np.random.default_rng(seed)
    corpus = _corpus(rng, 1 << 20)
    modes = np.array(["AIR", "FOB", "MAIL", "RAIL", "SHIP", "TRUCK", "REG AIR"])
    head = np.frombuffer(b"http://example.com/", dtype=np.uint8)
    comments, urls = [], []
    for lo in range(0, nrows, piece):
        n = min(piece, nrows - lo)
        # comment: a slice of the word text, 10-43 bytes
        ln = rng.integers(10, 44, n).astype(np.int32)
        start = rng.integers(0, len(corpus) - 64, n).astype(np.int32)
        offs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(ln, out=offs[1:])
        idx = np.repeat(start - offs[:-1], ln) + np.arange(offs[-1], dtype=np.int32)
        comments.append(_strings(corpus[idx], ln))
        # url: fixed head, the row number in 9 digits (distinct), '/', then
        # 31-91 bytes of the text with blanks turned into '/': 60-120 bytes
        fill = rng.integers(31, 92, n).astype(np.int32)
        ln = fill + 29
        offs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(ln, out=offs[1:])
        data = np.empty(offs[-1], dtype=np.uint8)
        rows = np.arange(lo, lo + n, dtype=np.int64)
        fixed = np.empty((n, 29), dtype=np.uint8)
        fixed[:, :19] = head
        for d in range(9):
            fixed[:, 19 + d] = 48 + (rows // 10 ** (8 - d)) % 10
        fixed[:, 28] = ord("/")
        data[(offs[:-1, None] + np.arange(29, dtype=np.int32)).reshape(-1)] = \
            fixed.reshape(-1)
        start = rng.integers(0, len(corpus) - 128, n).astype(np.int32)
        foffs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(fill, out=foffs[1:])
        src = np.repeat(start - foffs[:-1], fill) + \
            np.arange(foffs[-1], dtype=np.int32)
        dst = np.repeat(offs[:-1] + 29 - foffs[:-1], fill) + \
            np.arange(foffs[-1], dtype=np.int32)
        body = corpus[src]
        data[dst] = np.where(body == 32, 47, body)
        urls.append(_strings(data, ln))
    return pa.table({
        "comment": pa.chunked_array(comments),
        "url": pa.chunked_array(urls),
        "mode": pa.array(modes[rng.integers(0, len(modes), nrows)]),
    })


def _layout(path, snappy):
    """Per column: pages by encoding and row groups (from the page index)."""
    idx = G.file_index(path)
    out = {}
    for ci in range(len(idx.schema)):
        pages = [p for ch in idx.chunks(ci, snappy) for p in ch.pages]
        out[idx.schema.column(ci).name] = {
            "row_groups": idx.meta.num_row_groups,
            "dict_pages": sum(p.enc == G.RLE_DICTIONARY for p in pages),
            "plain_pages": sum(p.enc == G.PLAIN for p in pages)}
    return out


def _canonical(col, ext):
    """(validity, lengths, bytes) of a string column in plain form, null
    rows empty; a coded column is expanded through its dictionary."""
    n = len(col)
    valid = (torch.ones(n, dtype=torch.bool, device=col.offsets.device)
             if col.validity is None else col.validity.to(torch.bool))
    lens = col.offsets[1:] - col.offsets[:-1]
    src = col.offsets[:-1]
    if col.codes is not None:
        valid = valid & (col.codes >= 0)
        code = col.codes.to(torch.int64).clamp(min=0)
        lens, src = lens.index_select(0, code), src.index_select(0, code)
    lens = torch.where(valid, lens, torch.zeros_like(lens)).contiguous()
    offs = torch.zeros(n + 1, dtype=torch.int64, device=lens.device)
    torch.cumsum(lens, 0, out=offs[1:])
    pad = torch.cat([col.bytes_, col.bytes_.new_zeros(16)])
    blob = ext.pq_gather_strings(pad, src.contiguous(), lens, offs[:-1],
                                 int(offs[-1].item()))
    return valid, lens, blob


def _timed_pair(fns, warmup, runs):
    """{label: (median, min, max)} of the callables, alternating."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def _event_pair(fns, warmup, runs):
    """The same with device events around each call, in milliseconds."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def _ms(t, scale=1e3):
    return {"median_ms": round(t[0] * scale, 3), "min_ms": round(t[1] * scale, 3),
            "max_ms": round(t[2] * scale, 3)}


def _scans(path, snappy, warmup, runs, ext):
    schema_all = parquet_io.infer_schema([path])
    opts = {"gpuSnappy": "on" if snappy else "off"}

    def scan(schema, mode):
        return parquet_io.read([path], schema, DEV,
                               dict(opts, gpuDecode=mode))

    dev_t, host_t = scan(schema_all, "force"), scan(schema_all, "off")
    for name, _ in schema_all:
        a = _canonical(dev_t.columns[name], ext)
        b = _canonical(host_t.columns[name], ext)
        if not all(torch.equal(x, y) for x, y in zip(a, b)):
            raise SystemExit(f"{path}: column {name}: device decode differs "
                             "from the host path")
    del dev_t, host_t, a, b
    torch.cuda.empty_cache()
    res = {}
    for label, schema in [("all", schema_all)] + [
            (n, [(n, t)]) for n, t in schema_all]:
        t = _timed_pair({"force": lambda: scan(schema, "force"),
                         "off": lambda: scan(schema, "off")}, warmup, runs)
        row = {k: _ms(v) for k, v in t.items()}
        row["host_over_device"] = round(t["off"][0] / t["force"][0], 2)
        res[label] = row
        print(f"  {label:8s} device {row['force']['median_ms']:9.2f} ms "
              f"({row['force']['min_ms']:.2f}-{row['force']['max_ms']:.2f})  "
              f"host {row['off']['median_ms']:9.2f} ms "
              f"({row['off']['min_ms']:.2f}-{row['off']['max_ms']:.2f})  "
              f"host/device {row['host_over_device']:.2f}x", flush=True)
    return res


def _kernels(path, column, warmup, runs, ext):
    """Old and new kernel pair over the PLAIN pages of one column of the
    uncompressed file, on one uploaded buffer."""
    dec = G._ColumnDecoder(G.file_index(path), column, DEV, snappy=False)
    dec.upload()
    _, dense_counts = dec.decode_validity()
    rows, base, pi = [], 0, 0
    for ch in dec.chunks:
        for p in ch.pages:
            if p.enc == G.PLAIN:
                rows.append((dec._val_off(ch, p), p.val_len, dense_counts[pi],
                             base, 0, 0))
                base += dense_counts[pi]
            pi += 1
    table = G._page_table(rows, DEV)
    buf = dec.buf
    old_len, old_pos = ext.pq_bytearray_walk(buf, table, base)
    new_len, new_pos, status = ext.pq_bytearray_index(buf, table, base)
    if int(status.abs().sum().item()) or not (
            torch.equal(old_len, new_len) and torch.equal(old_pos, new_pos)):
        raise SystemExit(f"{column}: pq_bytearray_index differs from "
                         "pq_bytearray_walk")
    offs = torch.zeros(base + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(new_len, 0, out=offs[1:])
    total = int(offs[-1].item())
    starts = offs[:-1]
    if not torch.equal(ext.pq_gather_strings(buf, new_pos, new_len, starts, total),
                       ext.pq_gather_bytes(buf, new_pos, new_len, starts, total)):
        raise SystemExit(f"{column}: pq_gather_bytes differs from "
                         "pq_gather_strings")
    t = _event_pair({
        "pq_bytearray_walk": lambda: ext.pq_bytearray_walk(buf, table, base),
        "pq_bytearray_index": lambda: ext.pq_bytearray_index(buf, table, base),
    }, warmup, runs)
    t.update(_event_pair({
        "pq_gather_strings": lambda: ext.pq_gather_strings(
            buf, new_pos, new_len, starts, total),
        "pq_gather_bytes": lambda: ext.pq_gather_bytes(
            buf, new_pos, new_len, starts, total),
    }, warmup, runs))
    out = {"pages": len(rows), "values": base, "value_bytes": total}
    for k, v in t.items():
        out[k] = dict(_ms(v, 1.0), gb_per_s=round(total / v[0] / 1e6, 2))
        print(f"  {column:8s} {k:20s} {v[0]:9.3f} ms ({v[1]:.3f}-{v[2]:.3f})  "
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
        raise SystemExit("string_scan_bench needs a GPU: timings taken "
                         "anywhere else say nothing about the scan path")
    from sail_amd.ops import kernels

    ext = kernels.require()
    out_dir = args.dir or tempfile.mkdtemp(prefix="sail_string_bench_")
    t = _table(args.rows)
    files = {"snappy": (os.path.join(out_dir, "strings-snappy.parquet"), True),
             "none": (os.path.join(out_dir, "strings-none.parquet"), False)}
    pq.write_table(t, files["snappy"][0])
    pq.write_table(t, files["none"][0], compression="NONE")
    del t
    res = {"tool": "string_scan_bench", "rows": args.rows, "runs": args.runs,
           "warmup": args.warmup, "files": {}}
    for label, (path, snappy) in files.items():
        with open(path, "rb") as f:          # warm the page cache
            while f.read(64 << 20):
                pass
        layout = _layout(path, snappy)
        mb = round(os.path.getsize(path) / 1e6, 1)
        print(f"{label}: {mb} MB; layout {layout}", flush=True)
        res["files"][label] = {
            "file_mb": mb, "layout": layout,
            "scan_ms": _scans(path, snappy, args.warmup, args.runs, ext)}
    print("kernels on the uncompressed file's upload:", flush=True)
    res["kernels"] = {c: _kernels(files["none"][0], c, args.warmup, args.runs,
                                  ext) for c in ("comment", "url")}
    res["device_loses"] = [f"{f}:{c}" for f, v in res["files"].items()
                           for c, r in v["scan_ms"].items()
                           if r["host_over_device"] < 1.0]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
