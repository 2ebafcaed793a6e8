"""MIN / MAX over window frames on the device: window_frame_minmax against the torch sparse table.

    python tools/window_frame_bench.py [--n ROWS] [--rounds R] [--dtypes ...] [--frames ...]
                                       [--parts ...] [--ops ...] [--out FILE]

Per cell (dtype x frame x partitioning), `_bounded_rows_agg` / `_bounded_range_agg`
of engine/window.py on rows already in window order, two ways, alternating in
one process after a warm-up of each and timed with device events around the
call and the synchronise that ends it: median of the rounds with min - max.
`hip` is window_frame_minmax (ops/csrc/window_frames.hip), `torch` the switch
off. A call computes the frame bounds and the count of valid rows per frame
(the same torch ops on both sides) and then the minimum or maximum, so the
difference of the two columns is the difference of the two paths. Both results
are compared for equality, data and validity, before timing.

Frames: `p6` 6 PRECEDING to CURRENT ROW, `c500` 500 PRECEDING to 500
FOLLOWING, `u2` UNBOUNDED PRECEDING to 2 FOLLOWING, `range` RANGE BETWEEN 1000
PRECEDING AND 1000 FOLLOWING over a key that grows by 2 - 3 per row (about
800 rows). Partitionings: `one` partition, `p10000` uniform partitions, `hot`
half of the rows in one partition and the rest in 9999. A tenth of the rows is
NULL. A run without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

from sail_amd.engine import types as T
from sail_amd.engine import window as W
from sail_amd.engine.column import Column

FRAMES = {"p6": ("rows", ("preceding", 6), ("current", None)),
          "c500": ("rows", ("preceding", 500), ("following", 500)),
          "u2": ("rows", ("unbounded_preceding", None), ("following", 2)),
          "range": ("range", ("preceding", 1000), ("following", 1000))}
PARTS = ["one", "p10000", "hot"]
DTYPES = {"int64": T.I64, "float64": T.F64}


def make_parts(kind, n, dev):
    """(part_id, pos_in_part, part_start_pos) of rows sorted by partition."""
    i = torch.arange(n, device=dev)
    if kind == "one":
        part_id = torch.zeros_like(i)
    elif kind == "p10000":
        part_id = i * 10000 // n
    else:
        half = n // 2
        part_id = torch.where(i < half, torch.zeros_like(i), 1 + (i - half) * 9999 // (n - half))
    change = torch.ones(n, dtype=torch.bool, device=dev)
    change[1:] = part_id[1:] != part_id[:-1]
    start = torch.nonzero(change, as_tuple=False).squeeze(1)
    return part_id, i - start[part_id], start


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(t):
    return {"ms": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtypes", nargs="*", default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument("--frames", nargs="*", default=list(FRAMES), choices=list(FRAMES))
    ap.add_argument("--parts", nargs="*", default=PARTS, choices=PARTS)
    ap.add_argument("--ops", nargs="*", default=["max"], choices=["min", "max"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_frame_bench needs a GPU")
    dev, n, rows = "cuda", args.n, []
    for dt in args.dtypes:
        g = torch.Generator(device=dev).manual_seed(n % 9973 + len(dt))
        if dt == "int64":
            x = torch.randint(-10 ** 9, 10 ** 9, (n,), device=dev, generator=g)
        else:
            x = torch.rand(n, device=dev, dtype=torch.float64, generator=g) * 1e6 - 5e5
        col = Column(DTYPES[dt], x, (torch.rand(n, device=dev, generator=g) >= 0.1).to(torch.uint8))
        for part in args.parts:
            part_id, pos, start = make_parts(part, n, dev)
            key = pos * 2 + torch.randint(0, 2, (n,), device=dev, generator=g)   # rises inside a partition
            for fr in args.frames:
                for op in args.ops:
                    f = types.SimpleNamespace(name=op, dtype=None)

                    def side(name):
                        os.environ["SAIL_EXEC_WINDOW_FRAMES"] = "on" if name == "hip" else "off"
                        if FRAMES[fr][0] == "rows":
                            out = W._bounded_rows_agg(f, [col], part_id, pos, start, FRAMES[fr], n, dev)
                        else:
                            out = W._bounded_range_agg(f, [col], part_id, start, FRAMES[fr], key, n, dev)
                        assert W.LAST_WINDOW_PATH == name, (W.LAST_WINDOW_PATH, name)
                        return out

                    a, b = side("hip"), side("torch")            # warm-up, and the results
                    same = torch.equal(a.data, b.data) and torch.equal(a.valid_mask(), b.valid_mask())
                    assert same, (dt, part, fr, op)
                    del a, b
                    ms = {"hip": [], "torch": []}
                    for _ in range(args.rounds):
                        for s in ms:
                            ms[s].append(timed(lambda: side(s))[0])
                    row = {"dtype": dt, "parts": part, "frame": fr, "op": op, "n": n,
                           "results_equal": same, "hip": stats(ms["hip"]), "torch": stats(ms["torch"])}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    torch.cuda.empty_cache()
            del part_id, pos, start, key
        del x, col
    os.environ.pop("SAIL_EXEC_WINDOW_FRAMES", None)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
