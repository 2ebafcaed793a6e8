"""GROUP BY above 4096 groups: the torch path against grouped_acc_global.

    python tools/agg_global_bench.py [--n ROWS] [--rounds R] [--torch-rounds R] [--out FILE]

Four aggregates (sum i64, sum f64, count, max i64) over n rows for G in
{5e3, 1e5, 1e7} x {uniform, sorted, skewed with one group near 50 %}.
Per cell, alternating in one process and timed with device events:

  torch    the agg_eval loop a query takes when fused_agg_batch returns None
  fused    fused_agg_batch with sail.exec.agg_global on
  kernel   grouped_acc_global alone, as shipped / run combining off / cache off

The pass is bound by memory bandwidth: it must read n x (8 B gid + 3 x 8 B
values), and GB/s and the share of the card's 6.3 TB/s are computed from
those bytes. `--parent-aggregates FILE` times a second copy of
engine/aggregates.py (the parent commit's) as the torch side of one cell.
A run without a GPU fails.
"""
import argparse
import importlib.util
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
from sail_amd.plan import spec as S

HBM_BYTES_PER_S = 6.3e12
OPS = [0, 1, 2, 4]
AGGS = [S.AggFunc("sum"), S.AggFunc("sum"), S.AggFunc("count"), S.AggFunc("max")]


def make_gid(dist, n, G, dev):
    g = torch.randint(0, G, (n,), dtype=torch.int64, device=dev)
    if dist == "sorted":
        return torch.sort(g).values
    if dist == "skewed":  # one group on every second row or so, scattered
        hot = torch.rand(n, device=dev) < 0.5
        return torch.where(hot, torch.full_like(g, G // 3), g)
    return g


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def load_parent(path):
    spec = importlib.util.spec_from_file_location("sail_amd.engine.parent_aggregates", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-rounds", type=int, default=3,
                    help="repeats of the torch side (seconds per call on clustered ids)")
    ap.add_argument("--groups", type=int, nargs="*", default=[5_000, 100_000, 10_000_000])
    ap.add_argument("--dists", nargs="*", default=["uniform", "sorted", "skewed"])
    ap.add_argument("--no-torch", nargs="*", default=[], metavar="DIST",
                    help="distributions whose torch side is left out: on skewed ids one "
                         "torch call over 100M rows did not finish in 7 minutes")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-aggregates", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("agg_global_bench needs a GPU")
    ext = K.require()
    dev, n = "cuda", args.n
    vi = torch.randint(-(1 << 30), 1 << 30, (n,), dtype=torch.int64, device=dev)
    vf = torch.randint(-(1 << 20), 1 << 20, (n,), device=dev).to(torch.float64)
    vm = torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=dev)
    cols = [Column(T.I64, vi), Column(T.F64, vf), None, Column(T.I64, vm)]
    args_list = [[c] if c is not None else [] for c in cols]
    fmasks = [None] * 4
    vals = [vi, vf, None, vm]
    need = n * (8 + 3 * 8)
    parent = load_parent(args.parent_aggregates) if args.parent_aggregates else None
    os.environ["SAIL_EXEC_AGG_GLOBAL"] = "on"
    rows = []
    for G in args.groups:
        for dist in args.dists:
            gid = make_gid(dist, n, G, dev)

            def torch_side(mod=A):
                return [mod.agg_eval(a.name, ar, gid, G, False, None, a.dtype)
                        for a, ar in zip(AGGS, args_list)]

            sides = {
                "torch": torch_side,
                "fused": lambda: A.fused_agg_batch(AGGS, args_list, fmasks, gid, G),
                "kernel": lambda: ext.grouped_acc_global(gid, None, vals, OPS, G, 0),
                "kernel_no_runs": lambda: ext.grouped_acc_global(gid, None, vals, OPS, G, 1),
                "kernel_no_cache": lambda: ext.grouped_acc_global(gid, None, vals, OPS, G, 2),
            }
            if dist in args.no_torch:
                del sides["torch"]
            elif parent is not None and G == args.groups[0] and dist == "uniform":
                sides["torch_parent"] = lambda: torch_side(parent)
            outs = {}
            for k, f in sides.items():                      # warm-up, and the results
                outs[k] = f()
                torch.cuda.synchronize()
                print(f"# G={G} {dist}: {k} warm", file=sys.stderr, flush=True)
            same = all(torch.equal(outs[k], outs["kernel"])
                       for k in ("kernel_no_runs", "kernel_no_cache"))
            if "torch" in sides:
                same = same and all(torch.equal(w.data, g.data)
                                    for w, g in zip(outs["torch"], outs["fused"]))
            else:  # the fused columns against the kernel's rows (f64 sums bit-cast)
                same = same and all(torch.equal(g.data.view(torch.int64), k)
                                    for g, k in zip(outs["fused"], outs["kernel"]))
            del outs
            ms = {k: [] for k in sides}
            for r in range(args.rounds):
                for k, f in sides.items():
                    if r < args.torch_rounds or not k.startswith("torch"):
                        ms[k].append(timed(f)[0])
                print(f"# G={G} {dist}: round {r}", file=sys.stderr, flush=True)
            row = {"G": G, "dist": dist, "n": n, "results_equal": same}
            for k, v in ms.items():
                med = statistics.median(v)
                row[k] = {"ms": round(med, 3), "min": round(min(v), 3), "max": round(max(v), 3),
                          "GBps": round(need / med / 1e6, 1),
                          "hbm_share": round(need / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
            if "torch" in sides:
                row["torch_spread"] = round((max(ms["torch"]) - min(ms["torch"]))
                                            / statistics.median(ms["torch"]), 4)
                row["speedup"] = round(row["torch"]["ms"] / row["fused"]["ms"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del gid
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
