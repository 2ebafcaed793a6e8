"""The one-lookup device join (`sail.exec.join_fused`, hash_join.hip:
hj_build_flag, hj_probe_heads, hj_probe_exists, hj_fill_heads).

Expected pairs and counts come from plain Python dicts. Every device case
runs with the switch on and asserts which way the join went (`unique`,
`chained`, `exists`; `legacy` with the switch off) from the record that
`engine/joins.py` keeps, so that a silent fall-back cannot pass.

The unmarked tests pin the path selection with a stub extension and the SQL
results of semi/anti joins on the host matcher; they run without a GPU.
"""
import collections
import random

import pytest
import torch

import sail_amd
from sail_amd.engine import joins as J
from sail_amd.engine import types as T
from sail_amd.engine.column import Table

gpu = pytest.mark.gpu

M64 = (1 << 64) - 1
I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
EMPTY_MARKER = I64_MIN + 1          # kEmpty of hash_join.hip; the build-side null sentinel
PROBE_NULL = I64_MIN + 2
EXTREME_KEYS = [I64_MIN, I64_MIN + 1, I64_MIN + 2, -1, 0, I64_MAX]

PROBE_SIZES = (0, 1, 255, 256, 257, 2049, 5000)     # a workgroup covers 2048 rows
BUILD_SIZES = (0, 1, 2, 33, 2000)


@pytest.fixture(scope="module")
def ext():
    from sail_amd.ops import kernels

    return kernels.require()


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    monkeypatch.delenv("SAIL_EXEC_JOIN_FUSED", raising=False)
    J.LAST_JOIN_PATH = None


def _mix64(k: int) -> int:
    k &= M64
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k


def _table_size(n: int) -> int:
    sz = 64
    while sz < 2 * n:
        sz <<= 1
    return sz


def _same_home_keys(count, nbuild, home, start=1):
    """`count` keys whose home slot is `home` in the table of an nbuild-row
    build side."""
    mask = _table_size(nbuild) - 1
    out = []
    k = start
    while len(out) < count:
        if _mix64(k) & mask == home:
            out.append(k)
        k += 1
    return out


def _reference(build, probe):
    rows_of = collections.defaultdict(list)
    for j, k in enumerate(build):
        rows_of[k].append(j)
    counts = [len(rows_of.get(k, ())) for k in probe]
    pairs = sorted((i, j) for i, k in enumerate(probe) for j in rows_of.get(k, ()))
    return counts, pairs


def _run(ext, build, probe, **kw):
    before = dict(J.JOIN_PATHS)
    out = J._expand_matches_gpu(torch.tensor(build, dtype=torch.int64).cuda(),
                                torch.tensor(probe, dtype=torch.int64).cuda(), ext, **kw)
    took = [k for k in J.JOIN_PATHS if J.JOIN_PATHS[k] != before[k]]
    assert took == [J.LAST_JOIN_PATH]           # one path, recorded once
    assert J.JOIN_PATHS[took[0]] == before[took[0]] + 1
    return out


def _check_pairs(ext, build, probe, path):
    want_counts, want_pairs = _reference(build, probe)
    p_idx, b_idx, counts = _run(ext, build, probe)
    assert J.LAST_JOIN_PATH == path
    assert counts.dtype == torch.int64 and p_idx.dtype == torch.int64
    assert counts.cpu().tolist() == want_counts
    p, b = p_idx.cpu().tolist(), b_idx.cpu().tolist()
    assert p == sorted(p)                       # probe_idx is non-decreasing
    pairs = sorted(zip(p, b))
    assert pairs == want_pairs                  # the exact multiset
    assert len(set(pairs)) == len(pairs)
    return p


# ---------------------------------------------------------------------------
# unique path
# ---------------------------------------------------------------------------

def _distinct(n, seed):
    return random.Random(seed).sample(range(-10 ** 12, 10 ** 12), n)


@gpu
@pytest.mark.parametrize("nb", BUILD_SIZES)
@pytest.mark.parametrize("np_", PROBE_SIZES)
@pytest.mark.parametrize("mode", ["all", "none", "mix"])
def test_unique_build_sizes(ext, nb, np_, mode):
    rng = random.Random(1000 * nb + np_)
    keys = _distinct(nb + np_ + 1, 70)
    build, absent = keys[:nb], keys[nb:]
    if mode == "all" and nb:
        probe = [rng.choice(build) for _ in range(np_)]
    elif mode == "mix" and nb:
        probe = [rng.choice(build) if rng.random() < 0.5 else rng.choice(absent)
                 for _ in range(np_)]
    else:
        probe = [rng.choice(absent) for _ in range(np_)]
    p = _check_pairs(ext, build, probe, "unique")
    if mode == "all" and nb:
        assert p == list(range(np_))            # identity probe_idx


@gpu
def test_unique_extreme_keys(ext):
    rng = random.Random(71)
    build = EXTREME_KEYS + [5, 6]
    rng.shuffle(build)
    probe = EXTREME_KEYS * 2 + [rng.randrange(-3, 9) for _ in range(300)]
    _check_pairs(ext, build, probe, "unique")
    _check_pairs(ext, build, EXTREME_KEYS, "unique")        # every row matches
    # each extreme key alone, probed by all of them: no key stands for a neighbour
    for k in EXTREME_KEYS:
        _check_pairs(ext, [k], EXTREME_KEYS, "unique")


@gpu
@pytest.mark.parametrize("nbuild,home,start", [(64, 120, 1), (33, 127, 10 ** 15)])
def test_unique_one_home_slot_wraps(ext, nbuild, home, start):
    """Keys that share one home slot near the end of the table: the probe
    sequence wraps; absent keys with that home end at the first empty slot."""
    same = _same_home_keys(nbuild + 32, nbuild, home, start)
    build, absent = same[:nbuild], same[nbuild:]
    _check_pairs(ext, build, same + build[:10], "unique")
    _check_pairs(ext, build, absent, "unique")
    _check_pairs(ext, build, build, "unique")


# ---------------------------------------------------------------------------
# repeat detection
# ---------------------------------------------------------------------------

def _repeat_builds():
    base = _distinct(2000, 72)
    rng = random.Random(73)
    out = {}
    out["last_repeats_first"] = (base + [base[0]], base)
    body = base[:33]
    out["empty_marker"] = (body + [EMPTY_MARKER, EMPTY_MARKER], body + [EMPTY_MARKER])
    out["build_null_sentinel"] = ([EMPTY_MARKER] + body + [EMPTY_MARKER], [EMPTY_MARKER] + body)
    out["probe_null_sentinel"] = ([PROBE_NULL] + body + [PROBE_NULL], [PROBE_NULL] + body)
    out["two_rows"] = ([4, 4], [4, 5])
    probes = {k: v[1] + [rng.choice(v[1]) for _ in range(300)] + _distinct(50, 74)
              for k, v in out.items()}
    return out, probes


REPEAT_BUILDS, REPEAT_PROBES = _repeat_builds()


@gpu
@pytest.mark.parametrize("case", sorted(REPEAT_BUILDS))
def test_single_repeat_takes_chained_path(ext, case):
    with_repeat, without = REPEAT_BUILDS[case]
    _check_pairs(ext, with_repeat, REPEAT_PROBES[case], "chained")
    _check_pairs(ext, without, REPEAT_PROBES[case], "unique")


# ---------------------------------------------------------------------------
# chained path
# ---------------------------------------------------------------------------

def _chained_cases():
    rng = random.Random(75)
    cases = {
        "all_equal_33": ([7] * 33, [7, 8, 7, 6] * 70),
        "all_equal_300": ([-5] * 300, [-5] * 17 + [5] * 3),
        "extremes": (EXTREME_KEYS * 3, EXTREME_KEYS * 2 + [1, 2, 3]),
    }
    keys = _distinct(600, 76)
    four = keys[:500] * 4
    rng.shuffle(four)
    for np_ in PROBE_SIZES:
        cases[f"four_per_key_probe{np_}"] = (four, [rng.choice(keys) for _ in range(np_)])
    for nb in (2, 33, 2000):
        b = [rng.randrange(0, max(nb // 4, 1)) for _ in range(nb - 1)]
        b.append(b[0])                          # at least one repeat
        cases[f"build{nb}"] = (b, [rng.randrange(-2, nb // 4 + 3) for _ in range(300)])
    same = _same_home_keys(40, 33, 127, start=10 ** 15)
    cases["last_slot_home"] = (same[:33] + same[:5], same + same)
    return cases


CHAINED_CASES = _chained_cases()


@gpu
@pytest.mark.parametrize("case", sorted(CHAINED_CASES))
def test_chained_path(ext, case):
    build, probe = CHAINED_CASES[case]
    _check_pairs(ext, build, probe, "chained")


@gpu
def test_chained_pairs_in_two_pass_order(ext, monkeypatch):
    """The chain of a key is walked head first on both sides of the switch:
    for one build table the pairs come out in one order. (Two builds may
    link a chain differently, so the comparison is per probe row as a set
    and, within the fused side, against the chain itself.)"""
    build = [3] * 5 + [9] * 2 + [4]
    bids = torch.tensor(build).cuda()
    pids = torch.tensor([9, 3, 1, 3, 4]).cuda()
    tkeys, theads, nxt, dup = ext.hj_build_flag(bids, False)
    assert dup.item() == 1
    heads, counts, stat = ext.hj_probe_heads(tkeys, theads, nxt, dup, pids)
    assert stat.tolist() == [1, 4]
    assert counts.tolist() == [2, 5, 0, 5, 1]
    ends = torch.cumsum(counts, 0)
    p_idx, b_idx = ext.hj_fill_heads(heads, ends, nxt, int(ends[-1]))
    offsets = ends - counts
    p_old, b_old = ext.hj_probe_fill(tkeys, theads, nxt, pids, offsets, int(ends[-1]))
    assert torch.equal(p_idx, p_old) and torch.equal(b_idx, b_old)


# ---------------------------------------------------------------------------
# existence only
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("nb", [1, 2, 33, 2000])
@pytest.mark.parametrize("np_", PROBE_SIZES)
def test_exists_kernel_counts(ext, nb, np_):
    rng = random.Random(77 + nb + np_)
    build = [rng.randrange(-nb, nb) for _ in range(nb)] + EXTREME_KEYS[:nb % 7]
    probe = [rng.randrange(-2 * nb, 2 * nb) for _ in range(np_)] + EXTREME_KEYS[:np_ % 7]
    present = set(build)
    p_idx, b_idx, counts = _run(ext, build, probe, counts_only=True)
    assert J.LAST_JOIN_PATH == "exists"
    assert p_idx is None and b_idx is None      # no pair tensors
    assert counts.dtype == torch.int64
    assert counts.cpu().tolist() == [1 if k in present else 0 for k in probe]


_L_SCHEMA = {"k": T.I64, "v": T.I64}
_SEMI_SQL = {
    "semi": "SELECT l.k, l.v FROM l LEFT SEMI JOIN r ON l.k = r.k",
    "anti": "SELECT l.k, l.v FROM l LEFT ANTI JOIN r ON l.k = r.k",
    "semi_residual": "SELECT l.k, l.v FROM l LEFT SEMI JOIN r ON l.k = r.k AND l.v < r.v",
    "anti_residual": "SELECT l.k, l.v FROM l LEFT ANTI JOIN r ON l.k = r.k AND l.v < r.v",
    "intersect": "SELECT k FROM l INTERSECT SELECT k FROM r",
    "except": "SELECT k FROM l EXCEPT SELECT k FROM r",
}


def _semi_data(nulls):
    """5000 probe rows against 2000 build rows with repeats; `nulls` puts
    NULL keys on both sides."""
    rng = random.Random(78)
    lk = [rng.randrange(0, 900) for _ in range(5000)]
    rk = [rng.randrange(300, 1200) for _ in range(2000)]
    if nulls:
        lk = [None if rng.random() < 0.1 else k for k in lk]
        rk = [None if rng.random() < 0.1 else k for k in rk]
    left = {"k": lk, "v": [rng.randrange(0, 100) for _ in lk]}
    right = {"k": rk, "v": [rng.randrange(0, 100) for _ in rk]}
    return left, right


def _semi_reference(kind, left, right):
    """Plain Python: NULL keys match nothing."""
    rows_of = collections.defaultdict(list)
    for k, v in zip(right["k"], right["v"]):
        if k is not None:
            rows_of[k].append(v)
    residual = kind.endswith("residual")
    out = []
    for k, v in zip(left["k"], left["v"]):
        vs = rows_of.get(k, ()) if k is not None else ()
        hit = any(v < rv for rv in vs) if residual else bool(vs)
        if hit == kind.startswith("semi"):
            out.append((k, v))
    return sorted(out, key=repr)


def _session(device, nulls):
    left, right = _semi_data(nulls)
    s = sail_amd.SessionContext(device=device)
    s.catalog.register_table("l", Table.from_pydict(left, _L_SCHEMA, device="cpu").to(device))
    s.catalog.register_table("r", Table.from_pydict(right, _L_SCHEMA, device="cpu").to(device))
    return s


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("kind", ["semi", "anti", "semi_residual", "anti_residual"])
def test_semi_anti_sql_on_host(kind, nulls):
    """The host matcher gives the dict reference's rows, with the flag that
    asks for counts only in place; no device path is recorded."""
    before = dict(J.JOIN_PATHS)
    got = _session("cpu", nulls).sql(_SEMI_SQL[kind]).collect()
    assert sorted(map(tuple, got), key=repr) == _semi_reference(kind, *_semi_data(nulls))
    assert J.JOIN_PATHS == before


@gpu
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("kind", sorted(_SEMI_SQL))
def test_semi_anti_sql_on_device(ext, monkeypatch, kind, nulls):
    dev = _session("cuda", nulls)
    before = dict(J.JOIN_PATHS)
    got = sorted(map(tuple, dev.sql(_SEMI_SQL[kind]).collect()), key=repr)
    took = {k for k in J.JOIN_PATHS if J.JOIN_PATHS[k] != before[k]}
    if kind.endswith("residual"):
        assert took == {"chained"}              # pairs, for the residual to filter
    else:
        assert took == {"exists"}               # and so no pair tensors
    if kind in ("intersect", "except"):
        want = sorted(map(tuple, _session("cpu", nulls).sql(_SEMI_SQL[kind]).collect()), key=repr)
    else:
        want = _semi_reference(kind, *_semi_data(nulls))
    assert got == want
    monkeypatch.setenv("SAIL_EXEC_JOIN_FUSED", "off")
    before = dict(J.JOIN_PATHS)
    off = sorted(map(tuple, dev.sql(_SEMI_SQL[kind]).collect()), key=repr)
    assert {k for k in J.JOIN_PATHS if J.JOIN_PATHS[k] != before[k]} == {"legacy"}
    assert off == got


@gpu
@pytest.mark.parametrize("counts_only", [False, True])
def test_null_keys_match_nothing(ext, counts_only):
    """Null keys on either side, through the masks of _expand_matches: the
    unique, chained and exists paths all leave them unmatched."""
    rng = random.Random(79)
    for repeats in (False, True):
        build = list(range(-20, 180)) + ([5, 6] if repeats else [])
        probe = [rng.randrange(-30, 200) for _ in range(300)]
        bv = [rng.random() < 0.8 for _ in build]
        pv = [rng.random() < 0.8 for _ in probe]
        if not repeats:
            # one null on the build side: several would repeat the sentinel
            bv = [True] * len(build)
            bv[7] = False
        rows_of = collections.defaultdict(list)
        for j, k in enumerate(build):
            if bv[j]:
                rows_of[k].append(j)
        want_counts = [len(rows_of.get(k, ())) if pv[i] else 0 for i, k in enumerate(probe)]
        p_idx, b_idx, counts = J._expand_matches(
            torch.tensor(build).cuda(), torch.tensor(probe).cuda(),
            torch.tensor(bv).cuda(), torch.tensor(pv).cuda(), counts_only)
        if counts_only:
            assert J.LAST_JOIN_PATH == "exists" and p_idx is None and b_idx is None
            assert counts.cpu().tolist() == [min(c, 1) for c in want_counts]
            continue
        assert J.LAST_JOIN_PATH == ("chained" if repeats else "unique")
        assert counts.cpu().tolist() == want_counts
        want = sorted((i, j) for i, k in enumerate(probe) if pv[i] for j in rows_of.get(k, ()))
        assert sorted(zip(p_idx.cpu().tolist(), b_idx.cpu().tolist())) == want


# ---------------------------------------------------------------------------
# switch off
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("case", ["unique", "chained", "exists"])
def test_switch_off_takes_two_pass_entry_points(ext, monkeypatch, case):
    keys = _distinct(2100, 80)
    build = keys[:2000] + (keys[:40] if case == "chained" else [])
    probe = keys[1000:] + keys[:50]
    kw = {"counts_only": True} if case == "exists" else {}
    on = _run(ext, build, probe, **kw)
    assert J.LAST_JOIN_PATH == case
    calls = []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(ext, name)

    monkeypatch.setenv("SAIL_EXEC_JOIN_FUSED", "off")
    off = _run(Spy(), build, probe, **kw)
    assert J.LAST_JOIN_PATH == "legacy"
    assert calls == ["hj_build_chain", "hj_probe_count", "hj_probe_fill"]
    want_counts, want_pairs = _reference(build, probe)
    assert off[2].cpu().tolist() == want_counts
    assert sorted(zip(off[0].cpu().tolist(), off[1].cpu().tolist())) == want_pairs
    if case == "exists":
        assert on[2].cpu().tolist() == [min(c, 1) for c in want_counts]
    else:
        assert torch.equal(on[2], off[2])
        assert sorted(zip(on[0].cpu().tolist(), on[1].cpu().tolist())) == want_pairs


# ---------------------------------------------------------------------------
# path selection without a GPU
# ---------------------------------------------------------------------------

class _StubExt:
    """Stands for the extension on the host: dict tables, same returns."""

    def __init__(self):
        self.calls = []

    def hj_build_flag(self, keys, keys_only):
        self.calls.append("hj_build_flag:keys" if keys_only else "hj_build_flag")
        rows = collections.defaultdict(list)
        for j, k in enumerate(keys.tolist()):
            rows[k].insert(0, j)
        if keys_only:
            return [rows]
        dup = torch.tensor([int(any(len(v) > 1 for v in rows.values()))], dtype=torch.int32)
        return [rows, rows, rows, dup]

    def hj_probe_heads(self, tkeys, theads, nxt, dup, keys):
        self.calls.append("hj_probe_heads")
        ks = keys.tolist()
        heads = torch.tensor([tkeys[k][0] if k in tkeys else -1 for k in ks], dtype=torch.int64)
        counts = torch.tensor([len(tkeys.get(k, ())) for k in ks], dtype=torch.int64)
        stat = torch.tensor([int(dup), int((heads >= 0).sum())])
        return [heads, counts, stat]

    def hj_probe_exists(self, tkeys, keys):
        self.calls.append("hj_probe_exists")
        return torch.tensor([int(k in tkeys) for k in keys.tolist()], dtype=torch.int64)

    def hj_fill_heads(self, heads, ends, nxt, total):
        self.calls.append("hj_fill_heads")
        by_head = {v[0]: v for v in nxt.values()}
        p, b = [], []
        for i, h in enumerate(heads.tolist()):
            for r in by_head.get(h, ()):
                p.append(i)
                b.append(r)
        assert len(p) == total == (int(ends[-1]) if len(ends) else 0)
        return [torch.tensor(p, dtype=torch.int64), torch.tensor(b, dtype=torch.int64)]


@pytest.mark.parametrize("case,build,probe,path,calls", [
    ("all_match", [5, 7, 9], [9, 5, 5, 7], "unique", ["hj_build_flag", "hj_probe_heads"]),
    ("some_match", [5, 7, 9], [9, 1, 5, 2], "unique", ["hj_build_flag", "hj_probe_heads"]),
    ("no_probe_rows", [5, 7, 9], [], "unique", ["hj_build_flag", "hj_probe_heads"]),
    ("repeats", [5, 7, 5], [9, 5, 7, 5], "chained",
     ["hj_build_flag", "hj_probe_heads", "hj_fill_heads"]),
])
def test_path_selection_with_stub(case, build, probe, path, calls):
    stub = _StubExt()
    p_idx, b_idx, counts = J._expand_matches_gpu(
        torch.tensor(build, dtype=torch.int64), torch.tensor(probe, dtype=torch.int64), stub)
    assert J.LAST_JOIN_PATH == path and stub.calls == calls
    want_counts, want_pairs = _reference(build, probe)
    assert counts.tolist() == want_counts
    assert p_idx.tolist() == sorted(p_idx.tolist())
    assert sorted(zip(p_idx.tolist(), b_idx.tolist())) == want_pairs
    if case == "all_match":
        assert p_idx.tolist() == list(range(len(probe)))


def test_counts_only_with_stub_builds_no_pairs():
    stub = _StubExt()
    p_idx, b_idx, counts = J._expand_matches_gpu(
        torch.tensor([5, 7, 5]), torch.tensor([9, 5, 7]), stub, counts_only=True)
    assert J.LAST_JOIN_PATH == "exists"
    assert stub.calls == ["hj_build_flag:keys", "hj_probe_exists"]
    assert p_idx is None and b_idx is None and counts.tolist() == [0, 1, 1]


def test_switch_is_read_from_config_and_environment(monkeypatch):
    from sail_amd.config import DEFAULTS

    assert DEFAULTS["sail.exec.join_fused"] == "on" and J.join_fused_enabled()
    for v in ("off", "0", "false", "OFF"):
        monkeypatch.setenv("SAIL_EXEC_JOIN_FUSED", v)
        assert not J.join_fused_enabled()
    monkeypatch.setenv("SAIL_EXEC_JOIN_FUSED", "on")
    assert J.join_fused_enabled()
