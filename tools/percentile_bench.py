"""median / percentile on the device: grouped_select against the sorts and the host loop.

    python tools/percentile_bench.py [--n ROWS] [--sides select sort host] [--q Q]
                                     [--rounds R] [--cases ...] [--out FILE]

Per case, `agg_eval("percentile", ...)` three ways, alternating in one process
after a warm-up of each and timed with device events: median of the rounds
with min - max. `select` is grouped_select (ops/csrc/grouped_select.hip),
`sort` the two device sorts that serve above the histogram budget (forced by
setting the budget to 0), `host` the switch off. The results are compared for
equality before timing. The host loop builds one Python object per row, so it
is meant for `--n 4000000`; the default sides leave it out.

Cases: `one` no GROUP BY; `g<ng>_uniform`, `g<ng>_sorted`, `g<ng>_hot` that many
groups with uniform ids, sorted ids, and half of the rows in group 0, over
uniform random doubles; `top6` 1e4 groups over values that share their top 6
bytes (six passes in which every row takes part); `equal` 1e4 groups over one
value (eight such passes).

Bytes are what select reads: 9 walks of vals (8 B), mask (1 B) and gid (8 B,
grouped cases); the rate stands next to the card's 6.3 TB/s, and ms / 9 is the
mean cost of a walk. A run without a GPU fails.
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

HBM_BYTES_PER_S = 6.3e12
GROUPS = [32, 33, 10_000, 262_144]
CASES = ["one"] + [f"g{ng}_{d}" for ng in GROUPS for d in ("uniform", "sorted", "hot")] + \
        ["top6", "equal"]
BUDGET = A.PERCENTILE_HIST_BUDGET


def make_case(case, n, dev):
    """(gid int64, ng, vals float64)"""
    g = torch.Generator(device=dev).manual_seed(len(case) * 131 + n % 9973)
    vals = torch.rand(n, device=dev, dtype=torch.float64, generator=g) * 1e6
    if case == "one":
        return torch.zeros(n, dtype=torch.int64, device=dev), 1, vals
    if case == "equal":
        vals = torch.full_like(vals, 7.5)
    if case == "top6":
        low = torch.randint(0, 1 << 16, (n,), device=dev, dtype=torch.int64, generator=g)
        vals = (low + (0x4059 << 48)).view(torch.float64)   # 100.0 and the 65535 doubles above
    ng, _, dist = case[1:].partition("_") if case[0] == "g" else ("10000", "", "uniform")
    ng = int(ng)
    gid = torch.randint(0, ng, (n,), device=dev, dtype=torch.int64, generator=g)
    if dist == "sorted":
        gid = gid.sort().values
    if dist == "hot":
        gid = torch.where(torch.rand(n, device=dev, generator=g) < 0.5, torch.zeros_like(gid), gid)
    return gid, ng, vals


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
    ap.add_argument("--sides", nargs="*", default=["select", "sort"],
                    choices=["select", "sort", "host"])
    ap.add_argument("--q", type=float, default=0.5)
    ap.add_argument("--cases", nargs="*", default=CASES)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("percentile_bench needs a GPU")
    qcol = Column.from_values([args.q], T.F64, device="cuda")
    rows = []
    for case in args.cases:
        gid, ng, vals = make_case(case, args.n, "cuda")
        col = Column(T.F64, vals, None)

        def side(name):
            os.environ["SAIL_EXEC_PERCENTILE_SELECT"] = "off" if name == "host" else "on"
            A.PERCENTILE_HIST_BUDGET = 0 if name == "sort" else BUDGET
            out = A.agg_eval("percentile", [col, qcol], gid, ng)
            assert A.LAST_PERCENTILE_PATH == name, (A.LAST_PERCENTILE_PATH, name)
            return out.data

        first = {s: side(s) for s in args.sides}     # warm-up, and the results
        ref = first[args.sides[0]]
        same = all(torch.equal(ref, r) for r in first.values())
        del first, ref
        ms = {s: [] for s in args.sides}
        for r in range(args.rounds):
            for s in args.sides:
                ms[s].append(timed(lambda: side(s))[0])
            print(f"# {case}: round {r}", file=sys.stderr, flush=True)
        need = 9 * args.n * (8 + 1 + (8 if ng > 1 else 0))
        row = {"case": case, "n": args.n, "ng": ng, "q": args.q, "results_equal": same,
               "select_bytes": need}
        for s, t in ms.items():
            row[s] = stats(t)
        if "select" in ms:
            med = row["select"]["ms"]
            row["select"]["GBps"] = round(need / med / 1e6, 1)
            row["select"]["hbm_share"] = round(need / (med * 1e-3) / HBM_BYTES_PER_S, 4)
            row["select"]["ms_per_walk"] = round(med / 9, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del gid, vals, col
        torch.cuda.empty_cache()
    os.environ.pop("SAIL_EXEC_PERCENTILE_SELECT", None)
    A.PERCENTILE_HIST_BUDGET = BUDGET
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
