"""COUNT / SUM (DISTINCT x) on the device: sail.exec.distinct_hash off against on.

    python tools/distinct_bench.py [--n ROWS] [--agg count|sum] [--rounds R] [--cases ...] [--out FILE]

Per case, `agg_eval(..., distinct=True)` with the switch off (two argsorts,
gathers, index_add_) and on (distinct_acc, ops/csrc/distinct_agg.hip),
alternating in one process after a warm-up of each and timed with device
events: median of the rounds with min - max. The two results are compared
for equality before timing. Then distinct_acc alone with each template flag
against its absence (variant bit 0: wave filter off, bit 1: LDS cache on;
variant 0 is what ships), which is what decides the flags that ship.

Cases: `one_1e3`, `one_1.7e7`, `one_1e8` no GROUP BY with that many distinct
values; `g1e4`, `g1e7` that many groups over random 64-bit values from a pool
of 1.7e7 (the UserID shape); `sorted` is g1e4 ordered by (group, value);
`hot_group` is g1e4 with half of the rows in one group; `sorted8` is g1e4 with
about 8 copies of each pair, ordered (the wave filter's case); `hot_pairs` is
g1e4 with half of the rows spread over 1000 pairs (the LDS cache's case).

Bytes are what the answer needs at the least: keys (8 B), gid (8 B, grouped
cases) and mask (1 B) read once; the rate stands next to the card's 6.3 TB/s.
A run without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

from sail_amd.engine import aggregates as A
from sail_amd.engine import types as T
from sail_amd.engine.column import Column
from sail_amd.ops import kernels as K

HBM_BYTES_PER_S = 6.3e12
CASES = ["one_1e3", "one_1.7e7", "one_1e8", "g1e4", "g1e7", "sorted", "hot_group", "sorted8",
         "hot_pairs"]
POOL = 17_000_000


def make_case(case, n, dev):
    """(gid int64, ng, keys int64)"""
    g = torch.Generator(device=dev).manual_seed(len(case) * 131 + n % 9973)

    def rand(hi):
        return torch.randint(0, hi, (n,), device=dev, dtype=torch.int64, generator=g)

    if case.startswith("one_"):
        keys = rand(int(float(case[4:]))) * 7919
        return torch.zeros(n, dtype=torch.int64, device=dev), 1, keys
    ng = 10_000_000 if case == "g1e7" else 10_000
    # odd multiplier: a bijection on 64 bits
    keys = rand(max(n // 80_000, 1) if case == "sorted8" else POOL) * -7046029254386353131
    gid = rand(ng)
    if case == "hot_group":
        gid = torch.where(rand(2) == 0, torch.zeros_like(gid), gid)
    if case == "hot_pairs":
        hot = rand(2) == 0
        gid, keys = torch.where(hot, gid % 1000, gid), torch.where(hot, gid % 1000 * 7919, keys)
    if case.startswith("sorted"):
        o = torch.argsort(keys)
        o = o[torch.argsort(gid[o], stable=True)]
        gid, keys = gid[o], keys[o]
    return gid, ng, keys


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(t, need):
    med = statistics.median(t)
    return {"ms": round(med, 3), "min": round(min(t), 3), "max": round(max(t), 3),
            "GBps": round(need / med / 1e6, 1),
            "hbm_share": round(need / (med * 1e-3) / HBM_BYTES_PER_S, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--agg", default="count", choices=["count", "sum"])
    ap.add_argument("--cases", nargs="*", default=CASES)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distinct_bench needs a GPU")
    ext = K.require()
    rows = []
    for case in args.cases:
        gid, ng, keys = make_case(case, args.n, "cuda")
        col = Column(T.I64, keys, None)
        mask = torch.ones(args.n, dtype=torch.bool, device="cuda")

        def side(v):
            os.environ["SAIL_EXEC_DISTINCT_HASH"] = v
            out = A.agg_eval(args.agg, [col], gid, ng, distinct=True)
            return out.data, A.LAST_DISTINCT_PATH

        def kernel(variant):
            return ext.distinct_acc(None if ng == 1 else gid, keys, mask, ng,
                                    args.agg == "sum", variant=variant)

        (off, p_off), (on, p_on) = side("off"), side("on")     # warm-up, and the results
        same = torch.equal(off, on) and all(torch.equal(kernel(v)[0 if args.agg == "count" else 1],
                                                        on) for v in range(4))
        distinct = int(kernel(0)[0].sum().item())
        del off, on
        need = args.n * (8 + 1 + (8 if ng > 1 else 0))
        ms = {"off": [], "on": [], "v0_wave": [], "v1_neither": [], "v2_wave_cache": [],
              "v3_cache": []}
        for r in range(args.rounds):
            for v in ("off", "on"):
                ms[v].append(timed(lambda: side(v))[0])
            for variant, name in enumerate(list(ms)[2:]):
                ms[name].append(timed(lambda: kernel(variant))[0])
            print(f"# {case}: round {r}", file=sys.stderr, flush=True)
        row = {"case": case, "n": args.n, "ng": ng, "agg": args.agg, "distinct_pairs": distinct,
               "path_off": p_off, "path_on": p_on, "results_equal": same, "need_bytes": need}
        for name, t in ms.items():
            row[name] = stats(t, need)
        row["speedup"] = round(row["off"]["ms"] / row["on"]["ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del gid, keys, col, mask
        torch.cuda.empty_cache()
    os.environ.pop("SAIL_EXEC_DISTINCT_HASH", None)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
