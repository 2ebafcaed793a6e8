"""Device equi-join matching: sail.exec.join_fused off against on.

    python tools/join_probe_bench.py [--sizes NB:NP ...] [--rounds R] [--out FILE]

Per build/probe size and per case, `_expand_matches_gpu` with the switch off
(hj_build_chain + hj_probe_count + cast + scan + hj_probe_fill) and on
(hj_build_flag + hj_probe_heads, plus hj_fill_heads when keys repeat),
alternating in one process after a warm-up of each and timed with device
events: median of the rounds with min - max. Results are compared exactly
before timing (counts equal, probe_idx equal, pairs equal as sorted pairs).

Cases: `unique_all` distinct build keys, every probe row matches;
`unique_half` distinct build keys, about half of the probe rows match;
`four_per_key` every build key four times, every probe row matches;
`exists_half` is `unique_half` asked for counts only.

Bytes are what the result needs at the least, from shapes: the build keys
and the probe keys read once and the pairs written once (8 B each; counts
only: one 8 B count per probe row in place of the pairs); the rate stands
next to the card's 6.3 TB/s. The table's random reads are what separates the
two. A run without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

from sail_amd.engine import joins as J
from sail_amd.ops import kernels as K

HBM_BYTES_PER_S = 6.3e12
CASES = ["unique_all", "unique_half", "four_per_key", "exists_half"]


def make_keys(case, nb, np_, dev):
    g = torch.Generator(device=dev).manual_seed(nb * 31 + np_)
    if case == "four_per_key":
        nk = max(nb // 4, 1)
        build = torch.arange(nb, device=dev, dtype=torch.int64) % nk
        build = build[torch.randperm(nb, device=dev, generator=g)]
        probe = torch.randint(0, nk, (np_,), device=dev, dtype=torch.int64, generator=g)
        return build * 7919, probe * 7919
    build = torch.randperm(nb, device=dev, generator=g) * 7919
    span = nb if case == "unique_all" else 2 * nb
    probe = torch.randint(0, span, (np_,), device=dev, dtype=torch.int64, generator=g) * 7919
    return build, probe


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def same_result(off, on, counts_only):
    if counts_only:
        return torch.equal(off[2].clamp_max(1), on[2]) and on[0] is None
    if not (torch.equal(off[2], on[2]) and torch.equal(off[0], on[0])):
        return False
    if torch.equal(off[1], on[1]):
        return True
    # within one probe row two builds may link a chain in different orders:
    # compare the rows' build indices as sorted (probe, build) pairs, in
    # blocks of probe rows (torch.sort takes fewer than 2^31 elements)
    n_build = int(max(off[1].max().item(), on[1].max().item())) + 1
    ends = torch.cumsum(on[2], 0)
    n, total = ends.numel(), off[0].numel()
    step = max(n // (total // (1 << 28) + 1), 1)
    s = 0
    for r in range(step, n + step, step):
        e = int(ends[min(r, n) - 1].item())
        a = torch.sort(off[0][s:e] * n_build + off[1][s:e]).values
        b = torch.sort(on[0][s:e] * n_build + on[1][s:e]).values
        if not torch.equal(a, b):
            return False
        s = e
    return s == total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["15000000:150000000", "15000000:600000000",
                                                   "150000000:600000000"],
                    help="build:probe rows")
    ap.add_argument("--cases", nargs="*", default=CASES)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("join_probe_bench needs a GPU")
    ext = K.require()
    rows = []
    for size in args.sizes:
        nb, np_ = (int(x) for x in size.split(":"))
        for case in args.cases:
            counts_only = case == "exists_half"
            build, probe = make_keys("unique_half" if counts_only else case, nb, np_, "cuda")

            def side(v):
                os.environ["SAIL_EXEC_JOIN_FUSED"] = v
                out = J._expand_matches_gpu(build, probe, ext, counts_only)
                return out, J.LAST_JOIN_PATH

            (off, p_off), (on, p_on) = side("off"), side("on")     # warm-up, and the results
            torch.cuda.synchronize()
            same = same_result(off, on, counts_only)
            pairs = int(off[0].numel())
            need = 8 * (nb + np_) + (8 * np_ if counts_only else 16 * pairs)
            del off, on
            ms = {"off": [], "on": []}
            for r in range(args.rounds):
                for v in ("off", "on"):
                    ms[v].append(timed(lambda: side(v))[0])
                print(f"# {size} {case}: round {r}", file=sys.stderr, flush=True)
            row = {"build": nb, "probe": np_, "case": case, "pairs": pairs,
                   "path_off": p_off, "path_on": p_on, "results_equal": same,
                   "need_bytes": need}
            for v, t in ms.items():
                med = statistics.median(t)
                row[v] = {"ms": round(med, 3), "min": round(min(t), 3), "max": round(max(t), 3),
                          "GBps": round(need / med / 1e6, 1),
                          "hbm_share": round(need / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
            row["speedup"] = round(row["off"]["ms"] / row["on"]["ms"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del build, probe
            torch.cuda.empty_cache()
    os.environ.pop("SAIL_EXEC_JOIN_FUSED", None)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
