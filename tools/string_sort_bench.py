"""Ordering raw string columns: the host code against ops/csrc/string_sort.hip.

    python tools/string_sort_bench.py [--rows N] [--rounds R] [--host-rounds R] [--out FILE]

Three raw columns of N rows (default 4M) from datagen/strings_gen.py:

  comment  comment-like text, 2-10 words of a 300-word vocabulary
  url      URLs under a few long shared prefixes, drawn from N/8 distinct
           values, so most rows have duplicates
  key      short fixed-width keys, already sorted

Per column, with sail.exec.string_sort on and off, alternating in one process
after one warm-up call per side:

  ranks    executor.string_ranks (on) / the host branch of _sortable (off),
           device events around the call, which ends in a synchronise
  topk     SELECT c FROM t ORDER BY c LIMIT 10, wall time
  min      SELECT k, MIN(c) FROM t GROUP BY k (1000 groups), wall time
  cmp      SELECT COUNT(*) FROM t WHERE c >= literal, wall time

`off` runs the host code as it was before the kernels existed. Each line gives
the median, min and max in ms, the host side's spread ((max - min) / median),
the speed-up, and whether both sides returned the same result. A run without a
GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import sail_amd
from sail_amd.datagen import strings_gen as G
from sail_amd.engine import executor as X
from sail_amd.engine import types as T
from sail_amd.engine.column import Column, StringColumn, Table
from sail_amd.ops import kernels as K

WORDS = ["w%03d%s" % (i, "abcdefghij"[: 1 + i % 10]) for i in range(300)]
HOSTS = ["https://www.example-shop.com/catalogue/products/category",
         "https://www.example-shop.com/catalogue/products/search",
         "http://news.example.org/articles/2024/international/europe",
         "http://news.example.org/articles/2024/international/asia"]


def make_columns(n, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    vocab = G.pack_vocab(WORDS, dev)
    ids = torch.randint(0, len(WORDS), (n, 10), generator=g, device=dev)
    nw = torch.randint(2, 11, (n,), generator=g, device=dev)
    comment = G.assemble_words(ids, nw, vocab)
    d = max(n // 8, 1)
    uvocab = G.pack_vocab(HOSTS + WORDS, dev)
    uids = torch.randint(len(HOSTS), len(HOSTS) + len(WORDS), (d, 4), generator=g, device=dev)
    uids[:, 0] = torch.randint(0, len(HOSTS), (d,), generator=g, device=dev)
    distinct = G.assemble_words(uids, torch.randint(2, 5, (d,), generator=g, device=dev),
                                uvocab, sep=ord("/"))
    url = distinct.gather(torch.randint(0, d, (n,), generator=g, device=dev))
    key = G.keyed_names("K", torch.arange(n, device=dev))
    return {"comment": comment, "url": url, "key": key}


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3,
                    help="repeats of the host side (seconds per call)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("string_sort_bench needs a GPU")
    assert K.string_sort_ext() is not None, "extension without the string sort kernels"
    dev, n = "cuda", args.rows
    cols = make_columns(n, dev)
    kcol = Column(T.I64, torch.arange(n, device=dev) % 1000)
    rows = []
    for name, c in cols.items():
        sess = sail_amd.SessionContext(device=dev)
        sess.catalog.register_table("t", Table({"k": kcol, "c": c}))
        lit = StringColumn(c.offsets[n // 2: n // 2 + 2].clone(), c.bytes_).to_pylist()[0]
        lit = lit.replace("'", "")
        measures = {
            "ranks": (device_ms, lambda: X._sortable(c)),
            "topk": (wall_ms, lambda: sess.sql("SELECT c FROM t ORDER BY c LIMIT 10").collect()),
            "min": (wall_ms, lambda: sorted(
                sess.sql("SELECT k, MIN(c) FROM t GROUP BY k").collect())),
            "cmp": (wall_ms, lambda: sess.sql(
                f"SELECT COUNT(*) FROM t WHERE c >= '{lit}'").collect()),
        }
        for what, (clock, fn) in measures.items():
            ms, outs = {"on": [], "off": []}, {}
            for side in ("on", "off"):                      # warm-up, and the results
                os.environ["SAIL_EXEC_STRING_SORT"] = side
                outs[side] = fn()
                torch.cuda.synchronize()
                print(f"# {name} {what}: {side} warm", file=sys.stderr, flush=True)
            same = (torch.equal(outs["on"], outs["off"]) if torch.is_tensor(outs["on"])
                    else outs["on"] == outs["off"])
            del outs
            for r in range(args.rounds):
                for side in ("on", "off"):
                    if side == "on" or r < args.host_rounds:
                        os.environ["SAIL_EXEC_STRING_SORT"] = side
                        ms[side].append(clock(fn)[0])
                print(f"# {name} {what}: round {r}", file=sys.stderr, flush=True)
            row = {"column": name, "rows": n, "what": what, "results_equal": same}
            for side, v in ms.items():
                row[side] = {"ms": round(statistics.median(v), 3), "min": round(min(v), 3),
                             "max": round(max(v), 3)}
            row["host_spread"] = round((max(ms["off"]) - min(ms["off"]))
                                       / statistics.median(ms["off"]), 4)
            row["speedup"] = round(row["off"]["ms"] / row["on"]["ms"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.environ.pop("SAIL_EXEC_STRING_SORT", None)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
