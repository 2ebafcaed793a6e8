"""Device ordering of raw string columns (ops/csrc/string_sort.hip):
str_sort_perm, str_dense_rank and str_compare3 against plain Python on
`bytes` objects, then the engine paths that use them against the CPU session."""
import random

import pytest
import torch

from sail_amd.engine import executor
from sail_amd.engine import types as T
from sail_amd.engine.column import Column, StringColumn, Table

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 2047, 2048, 2049, 2 * 2048 + 1, 5 * 2048 + 3, 40_000]


def _short(r, m):
    return [bytes(r.choice(b"ab") for _ in range(r.randrange(4))) for _ in range(m)]


def _key_edge(r, m):
    return [b"q" * (n - 1) + bytes([r.choice(b"abc")]) for n in (r.choice((7, 8, 9)) for _ in range(m))]


def _long_prefix(r, m):
    return [b"p" * 70 + bytes(r.choice(b"xyz") for _ in range(r.randrange(1, 4))) for _ in range(m)]


def _zero_chains(r, m):
    return [r.choice((b"x", b"y")) + b"\0" * r.randrange(12) for _ in range(m)]


def _high_bytes(r, m):
    return [bytes(r.choice((0x80 + r.randrange(128), 97 + r.randrange(3)))
                  for _ in range(r.randrange(20))) for _ in range(m)]


def _all_equal(r, m):
    return [b"the same value"] * m


def _ascending(r, m):
    return [b"key%09d" % i for i in range(m)]


def _descending(r, m):
    return _ascending(r, m)[::-1]


CONTENTS = [_short, _key_edge, _long_prefix, _zero_chains, _high_bytes, _all_equal,
            _ascending, _descending]


def _pack(vals, lead=0):
    """(offsets, bytes) on the device; `lead` unused bytes come first, so the
    values start unaligned and the last one ends exactly at bytes.numel()."""
    offs = [lead]
    for v in vals:
        offs.append(offs[-1] + len(v))
    data = b"\x55" * lead + b"".join(vals)
    return (torch.tensor(offs, dtype=torch.int64, device="cuda"),
            torch.tensor(list(data), dtype=torch.uint8, device="cuda"))


def _ext():
    from sail_amd.ops import kernels

    return kernels.require()


def _check_sort_and_rank(vals, lead=0, rows=None):
    offs, byts = _pack(vals, lead)
    rows_t = None if rows is None else torch.tensor(rows, dtype=torch.int64, device="cuda")
    perm = _ext().str_sort_perm(offs, byts, rows_t)
    rows = list(range(len(vals))) if rows is None else rows
    assert perm.tolist() == sorted(rows, key=lambda i: (vals[i], i))
    rank_sorted, nd = _ext().str_dense_rank(offs, byts, perm)
    distinct = sorted(set(vals[i] for i in rows))
    assert int(nd) == len(distinct)
    rank_of = {v: k for k, v in enumerate(distinct)}
    assert rank_sorted.tolist() == [rank_of[vals[i]] for i in perm.tolist()]


@pytest.mark.parametrize("make", CONTENTS, ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("m", SIZES)
def test_sort_perm_and_dense_rank(m, make):
    _check_sort_and_rank(make(random.Random(m), m))


@pytest.mark.parametrize("make", CONTENTS, ids=lambda f: f.__name__.strip("_"))
def test_compare3(make):
    r = random.Random(5)
    a, b = make(r, 3001), make(r, 3001)
    b[::7] = a[::7]
    oa, ba = _pack(a, 1)
    ob, bb = _pack(b, 2)
    got = _ext().str_compare3(oa, ba, ob, bb)
    assert got.tolist() == [(x > y) - (x < y) for x, y in zip(a, b)]
    lit = a[17]
    ol, bl = _pack([lit], 3)
    got = _ext().str_compare3(oa, ba, ol, bl)
    assert got.tolist() == [(x > lit) - (x < lit) for x in a]


@pytest.mark.parametrize("end", [0, 1, 2, 3])
def test_last_string_ends_at_buffer_end(end):
    # 2049 values of 9-12 bytes, the last one sized so that bytes.numel() % 4
    # == end: its tail lies in the buffer's last dword, whole or with 1, 2 or 3
    # valid bytes. 'c' is the largest letter, so its successor in the order
    # (row 0 at the latest) extends it, and that compare reads up to its end
    r = random.Random(end)
    vals = [b"w" * 8 + bytes(r.choice(b"abc") for _ in range(r.randrange(1, 5)))
            for _ in range(2048)]
    vals[0] = b"w" * 8 + b"cccca"
    lead = 1
    tail = 1 + (end - lead - sum(map(len, vals)) - 9) % 4
    vals.append(b"w" * 8 + b"c" * tail)
    assert (lead + sum(map(len, vals))) % 4 == end
    _check_sort_and_rank(vals, lead)


def _column(vals, nulls):
    return StringColumn.from_pylist(
        [None if i in nulls else v.decode() for i, v in enumerate(vals)],
        device="cuda", dict_encode=False)


def test_rows_subset_and_string_ranks_with_nulls():
    r = random.Random(11)
    vals = _short(r, 5000)
    nulls = set(r.sample(range(5000), 700))
    valid = [i for i in range(5000) if i not in nulls]
    _check_sort_and_rank(vals, rows=valid)
    rank_of = {v: k for k, v in enumerate(sorted(set(vals[i] for i in valid)))}
    want = [len(rank_of) if i in nulls else rank_of[vals[i]] for i in range(5000)]
    assert executor.string_ranks(_column(vals, nulls)).tolist() == want


N_ENGINE = 3000
STATEMENTS = [
    "SELECT i, s FROM t ORDER BY s",
    "SELECT i, s FROM t ORDER BY s DESC NULLS FIRST, i",
    "SELECT i, s FROM t ORDER BY s LIMIT 5",
    "SELECT k, MIN(s), MAX(s) FROM t GROUP BY k ORDER BY k",
    "SELECT i FROM t WHERE s < u ORDER BY i",
    "SELECT i FROM t WHERE s >= 'pppq' ORDER BY i",
]


def _register(sess, device):
    r = random.Random(3)
    words = ["p" * r.randrange(1, 12) + r.choice("qrs") * r.randrange(3) for _ in range(400)]

    def col():
        return StringColumn.from_pylist(
            [None if r.random() < 0.1 else r.choice(words) for _ in range(N_ENGINE)],
            device=device, dict_encode=False)

    ints = {"i": list(range(N_ENGINE)), "k": [i % 13 for i in range(N_ENGINE)]}
    cols = {n: Column.from_values(v, T.I64, device=device) for n, v in ints.items()}
    cols["s"], cols["u"] = col(), col()
    sess.catalog.register_table("t", Table(cols))


@pytest.fixture()
def both(session, gpu_session, monkeypatch):
    monkeypatch.setattr(executor, "TOPK_MIN_ROWS", 1000)
    _register(session, "cpu")
    _register(gpu_session, "cuda")
    return session, gpu_session


@pytest.mark.parametrize("switch", ["on", "off"])
@pytest.mark.parametrize("sql", STATEMENTS)
def test_engine_matches_cpu(both, monkeypatch, sql, switch):
    monkeypatch.setenv("SAIL_EXEC_STRING_SORT", switch)
    cpu, gpu = both
    assert gpu.sql(sql).collect() == cpu.sql(sql).collect()


def test_device_path_makes_no_python_strings(monkeypatch):
    from sail_amd.engine import eval as ev

    col = _column(_short(random.Random(1), 3000), {5, 6})
    rev = col.gather(torch.arange(2999, -1, -1, device="cuda"))
    with monkeypatch.context() as mp:
        mp.setattr(StringColumn, "to_pylist", lambda self: pytest.fail("host path taken"))
        ranks = executor._sortable(col)
        less = ev._string_cmp(col, rev, "<")
    vals = col.to_pylist()
    rank_of = {v: k for k, v in enumerate(sorted(set(v for v in vals if v is not None)))}
    assert ranks.tolist() == [rank_of.get(v, len(rank_of)) for v in vals]
    assert less.tolist() == [x is not None and y is not None and x < y
                             for x, y in zip(vals, vals[::-1])]
