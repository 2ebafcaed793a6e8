"""Edge tests for the kernels that run the queries after the scan.

`hash_agg.hip` (grouped_acc), `hash_join.hip` (hj_build_chain, hj_probe_count,
hj_probe_fill, hg_group) and `strings.hip` (like_mask, string_hash64,
string_hash64_seeded, str_pairs_equal, substr_fixed).

Every kernel test compares the extension entry point with a reference written
here in plain Python (integers, bytes, dicts, math.fsum): neither the engine
nor torch's GPU ops take part in the expected values. Inputs are the smallest
that still reach the edge in question; seeds are fixed.

The unmarked tests at the top pin the host path (like_to_regex and the CPU
string_like) to the same reference and run without a GPU.
"""
import collections
import datetime
import itertools
import math
import random

import pytest
import torch

import sail_amd
from sail_amd.engine import types as T
from sail_amd.engine.column import Column, StringColumn, Table

gpu = pytest.mark.gpu

M64 = (1 << 64) - 1
I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1


def _signed(v: int) -> int:
    v &= M64
    return v - (1 << 64) if v >> 63 else v


@pytest.fixture(scope="module")
def ext():
    from sail_amd.ops import kernels

    return kernels.require()


def _pack(vals):
    """Arrow layout (offsets int64[n+1], bytes uint8[total]) on the host."""
    offs = [0]
    for v in vals:
        offs.append(offs[-1] + len(v))
    blob = b"".join(vals)
    return (torch.tensor(offs, dtype=torch.int64),
            torch.tensor(list(blob), dtype=torch.uint8))


def _pack_cuda(vals):
    o, b = _pack(vals)
    return o.cuda(), b.cuda()


# ---------------------------------------------------------------------------
# LIKE reference: dynamic programming over (string position, pattern
# position). A row of the table is kept as a bit set over pattern positions;
# rows reached while scanning are memoised per pattern, which keeps some
# millions of (string, pattern) pairs within a few seconds of plain Python.
# ---------------------------------------------------------------------------

_LIT, _ONE, _RUN = 0, 1, 2


class LikeRef:
    def __init__(self, pat: bytes):
        toks = []
        i = 0
        while i < len(pat):
            c = pat[i]
            if c == 0x5C and i + 1 < len(pat):  # \x: the literal byte x
                toks.append((_LIT, pat[i + 1]))
                i += 2
                continue
            if c == 0x25:
                toks.append((_RUN, 0))
            elif c == 0x5F:
                toks.append((_ONE, 0))
            else:
                toks.append((_LIT, c))  # a trailing lone backslash included
            i += 1
        self.toks = toks
        self.accept = 1 << len(toks)
        self.memo = {}
        self.start = self._close(1)

    def _close(self, row):
        # '%' may match the empty run: position j reaches j + 1 for free
        # (ascending j, so adjacent '%' close in one pass)
        for j, (kind, _) in enumerate(self.toks):
            if kind == _RUN and (row >> j) & 1:
                row |= 1 << (j + 1)
        return row

    def _step(self, row, c):
        nxt = 0
        for j, (kind, b) in enumerate(self.toks):
            if (row >> j) & 1:
                if kind == _RUN:
                    nxt |= 1 << j
                elif kind == _ONE or b == c:
                    nxt |= 1 << (j + 1)
        return self._close(nxt)

    def match(self, s: bytes) -> bool:
        row = self.start
        memo = self.memo
        for c in s:
            key = (row << 8) | c
            nxt = memo.get(key)
            if nxt is None:
                nxt = memo[key] = self._step(row, c)
            row = nxt
            if not row:
                return False
        return bool(row & self.accept)


def _like(pat: bytes, s: bytes) -> bool:
    return LikeRef(pat).match(s)


# -- corpora ----------------------------------------------------------------

ALPHA_A = b"a`bc%_\\"
ALPHA_B = b"rspqed"
EDGE_LENS = (0, 1, 7, 8, 9, 15, 16, 17)

# needles of length 1, 2, 8 and 9; the two-byte ones are the pairs on which
# the 8-byte scan of the first byte used to report a match that is not there
# (first byte, then that byte with bit 0 flipped)
NEEDLES = [b"a", b"s", b"sp", b"ab", b"rs", b"de", b"pq", b"a`", b"bc",
           b"abcabcab", b"rspqedrs", b"abcabcabc", b"rspqedrsp"]


def _near_miss(nd: bytes) -> bytes:
    # the needle with the byte after its first replaced by first^1: the shape
    # that fooled the scan ("srp" for "sp", "a`b" for "ab")
    return nd[:1] + bytes([nd[0] ^ 1]) + nd[1:]


def _crafted():
    out = [b"srpxxxxx", b"a`bxxxxx", b"%ax", b"a%bc", b"a%xb", b"axb", b"a_b",
           b"a%b", b"a\\b", b"100%", b"100x", b"100", b"%", b"_", b"\\", b"%%",
           b"", b"a", b"b", b"ab", b"ba", b"aab", b"abab", b"x" * 40]
    for nd in NEEDLES:
        miss = _near_miss(nd)
        for lead in (0, 1, 6, 7, 8, 9, 15):      # straddles each 8-byte step
            for tail in (0, 3, 8):
                out.append(b"x" * lead + nd + b"y" * tail)
                out.append(b"x" * lead + miss + b"y" * tail)
        out.append(b"x" * 7 + nd[:-1])            # needle cut off by the end
        out.append(nd[:1] * 12)
    return out


def _corpus(alpha: bytes, seed: int, n: int = 4000):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = EDGE_LENS[i % len(EDGE_LENS)] if i % 3 == 0 else rng.randint(0, 40)
        out.append(bytes(rng.choice(alpha) for _ in range(ln)))
    out.extend(_crafted())
    out.append(b"")  # the last row is empty
    return out


CORPORA = {"A": _corpus(ALPHA_A, 11), "B": _corpus(ALPHA_B, 12)}

# -- patterns ---------------------------------------------------------------

ENUM_PATTERNS = [bytes(p) for k in range(5)
                 for p in itertools.product(b"ab%_", repeat=k)]

EXTRA_PATTERNS = (
    # pure containment
    [b"%" + nd + b"%" for nd in NEEDLES]
    # chains of two and three segments, adjacent '%', needle longer than any row
    + [b"%a%b%", b"%s%p%", b"%sp%qe%", b"%a%%b%", b"%%ab%%", b"%ab%c%a%",
       b"%r%s%p%", b"%rs%rs%", b"%de%de%de%", b"%a`%b%", b"%b%b%b%",
       b"%" + b"a" * 45 + b"%b%", b"%b%" + b"rs" * 25 + b"%", b"%%%"]
    # prefix, suffix, exact, inner wildcard
    + [b"ab%", b"%ab", b"ab", b"sp%", b"%sp", b"rs", b"a%b", b"s%p", b"_b%",
       b"%b_", b"a_c", b"r__s%", b"%_%_%", b"________", b"_________",
       b"%xxxxxxx_", b"100%", b"abcabcab", b"%abcabcabc", b"rspqedrs%"]
    # escapes: \% and \_ are literals, \\ is a backslash, \a is a, and a
    # trailing lone backslash stands for itself
    + [b"\\%", b"\\_", b"%\\%%", b"%\\_%", b"100\\%", b"a\\_b", b"a\\%b",
       b"a\\%%", b"%a\\_", b"\\\\", b"%\\\\%", b"%\\%\\_%", b"\\a\\b", b"a\\\\b",
       b"ab\\", b"%\\", b"\\%%", b"%\\%", b"_\\%_", b"%a\\%b%", b"%\\%a%\\_%"]
)


def _route(pat: bytes) -> str:
    """Which kernel like_mask picks for a pattern (mirrors strings.hip)."""
    plain = b"_" not in pat and b"\\" not in pat
    if plain and len(pat) >= 2 and pat[:1] == b"%" and pat[-1:] == b"%":
        return "contains" if pat.find(b"%", 1) == len(pat) - 1 else "chain"
    return "generic"


def _patterns_for(name):
    return ENUM_PATTERNS + EXTRA_PATTERNS if name == "A" else EXTRA_PATTERNS


_EXPECT = {}


def _expected(name: str, pat: bytes) -> bytes:
    """One byte (0/1) per row of the corpus; computed once per session."""
    key = (name, pat)
    if key not in _EXPECT:
        ref = LikeRef(pat)
        _EXPECT[key] = bytes(ref.match(s) for s in CORPORA[name])
    return _EXPECT[key]


def _mask_bytes(t: torch.Tensor) -> bytes:
    return t.to(torch.uint8).cpu().numpy().tobytes()


def _first_diffs(name, pat, got: bytes, want: bytes, limit=3):
    rows = [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:limit]
    return [(pat, CORPORA[name][i], bool(got[i]), bool(want[i])) for i in rows]


# ---------------------------------------------------------------------------
# host path (no GPU needed)
# ---------------------------------------------------------------------------

def test_like_reference_on_known_cases():
    """The reference itself, on answers that can be checked by eye."""
    truth = [
        (b"%sp%", b"srpxxxxx", False), (b"%ab%", b"a`bxxxxx", False),
        (b"%sp%", b"xxxxxxxsp", True), (b"%x", b"%ax", True),
        (b"a%c", b"a%bc", True), (b"%a%b", b"a%xb", True),
        (b"100\\%", b"100%", True), (b"100\\%", b"100x", False),
        (b"100\\%", b"100", False), (b"a\\_b", b"axb", False),
        (b"a\\_b", b"a_b", True), (b"a_b", b"axb", True), (b"", b"", True),
        (b"", b"a", False), (b"%", b"", True), (b"_", b"", False),
        (b"%%", b"abc", True), (b"\\\\", b"\\", True), (b"ab\\", b"ab\\", True),
        (b"\\a", b"a", True), (b"%a%%b%", b"ab", True), (b"%a%%b%", b"ba", False),
        (b"_%_", b"a", False), (b"_%_", b"ab", True), (b"%ab", b"abab", True),
        (b"a%a", b"a", False),
    ]
    for pat, s, want in truth:
        assert _like(pat, s) is want, (pat, s)
    routes = collections.Counter(_route(p) for p in ENUM_PATTERNS + EXTRA_PATTERNS)
    assert min(routes["contains"], routes["chain"], routes["generic"]) >= 10


def test_host_like_paths_match_reference():
    """like_to_regex on every (string, pattern) pair of the corpora, and the
    CPU string_like (raw and dictionary columns) on the named patterns."""
    from sail_amd.engine.eval import like_to_regex, string_like

    bad = []
    for name, rows in CORPORA.items():
        strs = [s.decode("ascii") for s in rows]
        for pat in _patterns_for(name):
            rx = like_to_regex(pat.decode("ascii"))
            got = bytes(rx.match(v) is not None for v in strs)
            want = _expected(name, pat)
            if got != want:
                bad += _first_diffs(name, pat, got, want)
        raw = StringColumn.from_pylist(strs, device="cpu", dict_encode=False)
        dic = StringColumn.from_pylist(strs, device="cpu", dict_encode=True)
        for pat in EXTRA_PATTERNS + ENUM_PATTERNS[::16]:
            want = _expected(name, pat)
            for col in (raw, dic):
                got = _mask_bytes(string_like(col, pat.decode("ascii")))
                if got != want:
                    bad += _first_diffs(name, pat, got, want)
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------
# strings.hip: like_mask
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_like_mask_matches_reference(ext, name):
    """All three routes inside like_mask (containment scan, segment chain,
    generic matcher) on the whole corpus."""
    offs, byts = _pack_cuda(CORPORA[name])
    bad = []
    seen = collections.Counter()
    for pat in _patterns_for(name):
        seen[_route(pat)] += 1
        got = _mask_bytes(ext.like_mask(offs, byts, pat))
        want = _expected(name, pat)
        if got != want:
            bad += _first_diffs(name, pat, got, want)
    assert seen["contains"] and seen["chain"] and seen["generic"]
    assert not bad, bad[:10]


@gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_like_mask_row_counts(ext, n):
    """Columns that end inside, at and just past one workgroup; the last row
    of each is empty."""
    rows = CORPORA["A"][:max(n - 1, 0)] + ([b""] if n else [])
    assert len(rows) == n
    offs, byts = _pack_cuda(rows)
    for pat in (b"%ab%", b"%a%b%", b"a_%", b"%", b"", b"%\\%%"):
        got = _mask_bytes(ext.like_mask(offs, byts, pat))
        assert got == bytes(_like(pat, s) for s in rows), pat


@gpu
def test_like_mask_all_rows_empty(ext):
    offs, byts = _pack_cuda([b""] * 300)
    for pat, want in ((b"%", 1), (b"", 1), (b"%%", 1), (b"%a%", 0), (b"_", 0),
                      (b"%a%b%", 0)):
        assert _mask_bytes(ext.like_mask(offs, byts, pat)) == bytes([want]) * 300


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_engine_string_like_on_device(ext, name):
    """string_like on raw and dictionary device columns, null rows included."""
    from sail_amd.engine.eval import string_like

    rows = CORPORA[name]
    strs = [None if i % 97 == 5 else s.decode("ascii") for i, s in enumerate(rows)]
    raw = StringColumn.from_pylist(strs, device="cpu", dict_encode=False).to("cuda")
    dic = StringColumn.from_pylist(strs, device="cpu", dict_encode=True).to("cuda")
    assert not raw.is_dict and dic.is_dict
    bad = []
    for pat in EXTRA_PATTERNS + ENUM_PATTERNS[::16]:
        want = _expected(name, pat)
        for kind, col in (("raw", raw), ("dict", dic)):
            m = string_like(col, pat.decode("ascii"))
            if col.validity is not None:
                m = m & col.valid_mask()
            got = _mask_bytes(m)
            exp = bytes(0 if strs[i] is None else w for i, w in enumerate(want))
            if got != exp:
                bad += [(kind,) + d for d in _first_diffs(name, pat, got, exp)]
    assert not bad, bad[:10]


def _sql_lit(s: str) -> str:
    return "'" + s.replace("\\", "\\\\").replace("'", "''") + "'"


@gpu
def test_string_predicates_with_wildcard_bytes_in_needle():
    """startswith / endswith / contains take their needle literally: '%', '_'
    and '\\' in it are ordinary bytes, on raw and on dictionary columns."""
    rows = [s.decode("ascii") for s in CORPORA["A"][:600] + _crafted()]
    vals = [None if i % 53 == 7 else v for i, v in enumerate(rows)]
    s = sail_amd.SessionContext(device="cuda")
    ids = Column(T.I64, torch.arange(len(vals), dtype=torch.int64).cuda())
    raw = StringColumn.from_pylist(vals, device="cpu", dict_encode=False).to("cuda")
    dic = StringColumn.from_pylist(vals, device="cpu", dict_encode=True).to("cuda")
    assert not raw.is_dict and dic.is_dict
    s.catalog.register_table("sp", Table({"i": ids, "r": raw, "d": dic}))
    fns = {"startswith": str.startswith, "endswith": str.endswith,
           "contains": lambda v, p: p in v}
    needles = ["a_b", "a%b", "a\\b", "_", "%", "\\", "a_", "%a", "ab", "a`",
               "\\%", "_%", "100%", "b\\"]
    for needle in needles:
        for fn, ref in fns.items():
            want = [(i,) for i, v in enumerate(vals) if v is not None and ref(v, needle)]
            for colname in ("r", "d"):
                got = s.sql(f"SELECT i FROM sp WHERE {fn}({colname}, {_sql_lit(needle)}) "
                            "ORDER BY i").collect()
                assert got == want, (fn, colname, needle)


@gpu
def test_sql_like_with_escapes_on_device():
    """LIKE through SQL on a raw device column, escaped wildcards included."""
    rows = [s.decode("ascii") for s in _crafted()]
    s = sail_amd.SessionContext(device="cuda")
    ids = Column(T.I64, torch.arange(len(rows), dtype=torch.int64).cuda())
    raw = StringColumn.from_pylist(rows, device="cpu", dict_encode=False).to("cuda")
    s.catalog.register_table("lk", Table({"i": ids, "r": raw}))
    for pat in ("100\\%", "a\\_b", "%\\%%", "%sp%", "%a%b", "a%c", "%x", "%a%b%"):
        ref = LikeRef(pat.encode())
        want = [(i,) for i, v in enumerate(rows) if ref.match(v.encode())]
        got = s.sql(f"SELECT i FROM lk WHERE r LIKE {_sql_lit(pat)} ORDER BY i").collect()
        assert got == want, pat


# ---------------------------------------------------------------------------
# strings.hip: hashes, pair equality, substring
# ---------------------------------------------------------------------------

def _hash_rows():
    """Lengths 0..33, all 256 byte values (>= 0x80 included), and every
    alignment of a row's first byte modulo 8."""
    rng = random.Random(21)
    rows = []
    for ln in range(34):
        rows.append(bytes((ln * 37 + k * 11) % 256 for k in range(ln)))
        rows.append(bytes(rng.randrange(256) for _ in range(ln)))
        rows.append(bytes(rng.randrange(0x80, 0x100) for _ in range(ln)))
    rows.append(bytes(range(256)))
    for pad in range(1, 9):  # a short row shifts the 16- and 24-byte rows after it
        rows.append(b"\xff" * pad)
        rows.append(bytes(rng.randrange(256) for _ in range(16)))
        rows.append(bytes(rng.randrange(256) for _ in range(24)))
    rows += [b"", b"\x00", b"\x00" * 8, b"\x80", b"\xff" * 9, b""]
    return rows


def _seeded_hash_py(s: bytes, seed: int, mult: int) -> int:
    h = seed
    for b in s:
        h = ((h ^ b) * mult) & M64
    h ^= (len(s) * 0x2545F4914F6CDD1D) & M64
    return _signed(h)


@gpu
def test_string_hash64_matches_python_fnv(ext):
    from sail_amd.engine.joins import fnv1a_hash_py

    rows = _hash_rows()
    offs, byts = _pack_cuda(rows)
    starts = {o % 8 for o in offs.tolist()[:-1]}
    assert starts == set(range(8)), starts
    got = ext.string_hash64(offs, byts).cpu().tolist()
    assert got == [fnv1a_hash_py(s) for s in rows]
    assert min(got) >= 0
    assert ext.string_hash64(*_pack_cuda([])).numel() == 0


@gpu
def test_string_hash64_seeded_matches_python(ext):
    from sail_amd.engine import joins

    rows = _hash_rows()
    offs, byts = _pack_cuda(rows)
    for seed, mult in ((joins._H2_SEED, joins._H2_MULT), (0, 1099511628211),
                       (M64, 0xFF51AFD7ED558CCD)):
        got = ext.string_hash64_seeded(offs, byts, _signed(seed), _signed(mult))
        assert got.cpu().tolist() == [_seeded_hash_py(s, seed, mult) for s in rows]
    # the engine's entry point passes the same constants
    col = StringColumn(offs, byts, None, None)
    assert joins.hash2_tensor(col).cpu().tolist() == [
        _seeded_hash_py(s, joins._H2_SEED, joins._H2_MULT) for s in rows]


@gpu
def test_str_pairs_equal_matches_python(ext):
    rng = random.Random(22)
    a_rows, b_rows, ia, ib = [], [], [], []

    def pair(x: bytes, y: bytes):
        a_rows.append(x)
        b_rows.append(y)

    def flip(x: bytes, k: int) -> bytes:
        return x[:k] + bytes([x[k] ^ 0x40]) + x[k + 1:]

    for rep in range(6):
        for ln in (0, 1, 7, 8, 9, 15, 16, 17, 33):
            x = bytes(rng.randrange(256) for _ in range(ln))
            pair(x, x)                                    # equal
            pair(x, x + b"\x00")                          # a is a prefix of b
            if ln:
                pair(x, flip(x, ln - 1))                  # last byte differs
                pair(x, flip(x, 0))                       # first byte differs
                pair(x, x[:-1])                           # b is a prefix of a
                pair(x, bytes(b ^ 0xFF for b in x))       # same length, all differ
            if ln > 8:
                pair(x, flip(x, 8))                       # only byte 8 differs
                pair(x, flip(x, 7))
    n = len(a_rows)
    assert n > 256
    # b is stored in another order than a, so the two index vectors differ
    perm = list(range(n))
    rng.shuffle(perm)
    b_store = [None] * n
    for i, p in enumerate(perm):
        b_store[p] = b_rows[i]
    ia = list(range(n)) + [rng.randrange(n) for _ in range(300)]
    ib = perm + [rng.randrange(n) for _ in range(300)]
    want = [int(a_rows[x] == b_store[y]) for x, y in zip(ia, ib)]
    assert 0 < sum(want) < len(want)
    oa, ba = _pack_cuda(a_rows)
    ob, bb = _pack_cuda(b_store)
    got = ext.str_pairs_equal(oa, ba, torch.tensor(ia).cuda(), ob, bb,
                              torch.tensor(ib).cuda())
    assert got.cpu().tolist() == want
    # a column against itself
    got = ext.str_pairs_equal(oa, ba, torch.tensor(ia).cuda(), oa, ba,
                              torch.tensor(ib).cuda())
    assert got.cpu().tolist() == [int(a_rows[x] == a_rows[y]) for x, y in zip(ia, ib)]


SUBSTR_ROWS = [b"", b"a", b"ab", b"abc", b"abcdef", b"uvwxyz", b"abcdefg",
               bytes(range(48, 48 + 64)), bytes(range(40, 40 + 70)), b"xyz", b""]


@gpu
@pytest.mark.parametrize("ln", [0, 1, 3, 64])
def test_substr_fixed_matches_slicing(ext, ln):
    """1-based start in {1, 2, len, len+1} for the six-byte rows (len = 6),
    with shorter, empty, exact-length (3 and 64) and longer rows around."""
    rows = SUBSTR_ROWS * 30  # more than one workgroup
    offs, byts = _pack_cuda(rows)
    for start in (1, 2, 6, 7):
        buf, lens = ext.substr_fixed(offs, byts, start - 1, ln)
        buf = buf.cpu().numpy().tobytes()
        want = [r[start - 1:start - 1 + ln] for r in rows]
        assert lens.cpu().tolist() == [len(w) for w in want], start
        assert len(buf) == len(rows) * ln
        for i, w in enumerate(want):  # fixed pitch, zero padded
            assert buf[i * ln:(i + 1) * ln] == w + b"\x00" * (ln - len(w)), (start, i)


@gpu
@pytest.mark.parametrize("text", ["ascii", "utf8"])
def test_sql_substring_on_raw_device_column(text):
    """substring counts characters, on a column of non-ASCII text as well."""
    if text == "ascii":
        rows = [r.decode("ascii") for r in SUBSTR_ROWS] * 3
    else:
        rows = ["", "é", "日本語テキスト", "naïve café", "abc", "ÄÖÜäöüß", "a€b€c€d",
                "x" * 70, "ab", "𝄞𝄞𝄞𝄞", "ascii only"] * 3
    rows[5] = None
    s = sail_amd.SessionContext(device="cuda")
    ids = Column(T.I64, torch.arange(len(rows), dtype=torch.int64).cuda())
    raw = StringColumn.from_pylist(rows, device="cpu", dict_encode=False).to("cuda")
    assert not raw.is_dict
    s.catalog.register_table("sb", Table({"i": ids, "r": raw}))
    for start in (1, 2, 6, 7):
        for ln in (1, 3, 64, 0):
            got = s.sql(f"SELECT substring(r, {start}, {ln}) FROM sb ORDER BY i").collect()
            want = [(None if v is None else v[start - 1:start - 1 + ln],) for v in rows]
            assert got == want, (start, ln)


# ---------------------------------------------------------------------------
# hash_agg.hip: grouped_acc
# ---------------------------------------------------------------------------

OP_SUM, OP_FSUM, OP_COUNT, OP_MIN, OP_MAX = 0, 1, 2, 3, 4

# value ranges: negative where the type has a sign, so a missing sign
# extension shows; float columns hold integers small enough for every sum of
# 50k of them to be exact in a double, which makes op 1 comparable bit for bit
_DTYPES = {
    "i64": (torch.int64, lambda r: r.randint(-(1 << 30), 1 << 30)),
    "i32": (torch.int32, lambda r: r.randint(-(1 << 31), (1 << 31) - 1)),
    "i16": (torch.int16, lambda r: r.randint(-(1 << 15), (1 << 15) - 1)),
    "i8": (torch.int8, lambda r: r.randint(-128, 127)),
    "u8": (torch.uint8, lambda r: r.randint(0, 255)),
    "bool": (torch.bool, lambda r: r.random() < 0.4),
    "f64": (torch.float64, lambda r: float(r.randint(-(1 << 30), 1 << 30))),
    "f32": (torch.float32, lambda r: float(r.randint(-(1 << 20), 1 << 20))),
}
_INT_TYPES = ["i64", "i32", "i16", "i8", "u8", "bool"]
_ALL_TYPES = _INT_TYPES + ["f64", "f32"]

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2049, 50_000]


def _make_gid(rng, n, G, kind):
    if kind == "one":            # every row in one group, the others stay empty
        g = [G - 1] * n
    elif kind == "sparse":       # only every third group receives rows
        live = list(range(0, G, 3))
        g = [rng.choice(live) for _ in range(n)]
    else:
        g = [rng.randrange(G) for _ in range(n)]
    if kind == "ascending":
        g.sort()
    return g


def _make_mask(rng, n, kind):
    if kind == "none":
        return None, None
    if kind.startswith("true"):
        m = [True] * n
    elif kind.startswith("false"):
        m = [False] * n
    else:
        m = [rng.random() < 0.6 for _ in range(n)]
    dt = torch.uint8 if kind.endswith("u8") else torch.bool
    return m, torch.tensor(m, dtype=dt).cuda()


def _reference(gid, mask, cols, ops, G):
    """Python integers: sums and counts modulo 2^64, min/max with the int64
    sentinels for a group without rows, float sums as the exact integer."""
    members = [[] for _ in range(G)]
    for i, g in enumerate(gid):
        if mask is None or mask[i]:
            members[g].append(i)
    out = []
    for vals, op in zip(cols, ops):
        row = []
        for g in range(G):
            idx = members[g]
            if op == OP_COUNT:
                row.append(len(idx))
            elif op == OP_SUM:
                row.append(_signed(sum(int(vals[i]) for i in idx)))
            elif op == OP_FSUM:
                row.append(sum(int(vals[i]) for i in idx))
            elif op == OP_MIN:
                row.append(min((int(vals[i]) for i in idx), default=I64_MAX))
            else:
                row.append(max((int(vals[i]) for i in idx), default=I64_MIN))
        out.append(row)
    return out, members


def _run_case(ext, n, G, specs, gid_kind="random", mask_kind="none", seed=0):
    """specs: [(op, dtype name or None)]. Builds the inputs, runs grouped_acc
    and compares every cell exactly."""
    rng = random.Random(seed * 1000003 + n * 31 + G)
    gid = _make_gid(rng, n, G, gid_kind)
    mask, mask_t = _make_mask(rng, n, mask_kind)
    cols, tens, ops = [], [], []
    for op, dt in specs:
        ops.append(op)
        if dt is None:
            cols.append(None)
            tens.append(None)
            continue
        tdt, gen = _DTYPES[dt]
        vals = [gen(rng) for _ in range(n)]
        cols.append(vals)
        tens.append(torch.tensor(vals, dtype=tdt).cuda())
    want, members = _reference(gid, mask, cols, ops, G)
    gid_t = torch.tensor(gid, dtype=torch.int32).cuda()
    out = ext.grouped_acc(gid_t, mask_t, tens, ops, G)
    assert tuple(out.shape) == (len(specs), G) and out.dtype == torch.int64
    raw = out.cpu()
    for c, (op, dt) in enumerate(specs):
        ctx = (n, G, c, op, dt, gid_kind, mask_kind)
        if op == OP_FSUM:
            got = raw[c].view(torch.float64).tolist()
            assert got == [float(v) for v in want[c]], ctx
            # a group without rows keeps the all-zero bit pattern
            assert all(raw[c][g].item() == 0 for g in range(G) if not members[g]), ctx
        else:
            assert raw[c].tolist() == want[c], ctx
    return out


def _cycle_specs(ncols, shift, ops_cycle, with_count=True):
    specs = []
    for c in range(ncols):
        op = ops_cycle[(c + shift) % len(ops_cycle)]
        if op == OP_COUNT:
            specs.append((op, None))
        elif op == OP_FSUM:
            specs.append((op, _ALL_TYPES[(c * 3 + shift) % len(_ALL_TYPES)]))
        else:
            specs.append((op, _INT_TYPES[(c + shift) % len(_INT_TYPES)]))
    return specs


@gpu
@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 8])
def test_grouped_acc_register_variant_every_instance(ext, G):
    """G x ncols = 1..10: every template instance of the register kernel,
    with n walking through the block-edge sizes."""
    k = [1, 2, 3, 4, 5, 8].index(G)
    for ncols in range(1, 11):
        n = SIZES[(ncols + 3 * k) % len(SIZES)]
        kinds = ("random", "ascending", "sparse", "one")
        masks = ("none", "mixed-bool", "mixed-u8", "true-bool")
        _run_case(ext, n, G, _cycle_specs(ncols, k, (OP_SUM, OP_FSUM, OP_COUNT)),
                  gid_kind=kinds[(ncols + k) % 4], mask_kind=masks[ncols % 4],
                  seed=ncols)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_grouped_acc_sizes_both_variants(ext, n):
    """Every size on the register kernel (G = 4) and the LDS kernel (G = 9,
    and G = 4 with min/max columns)."""
    sums = [(OP_SUM, "i32"), (OP_FSUM, "f64"), (OP_COUNT, None)]
    _run_case(ext, n, 4, sums, mask_kind="mixed-u8", seed=1)
    _run_case(ext, n, 9, sums + [(OP_MIN, "i16"), (OP_MAX, "i8")],
              mask_kind="mixed-bool", seed=2)
    _run_case(ext, n, 4, sums + [(OP_MIN, "i64"), (OP_MAX, "i32")], seed=3)


@gpu
@pytest.mark.parametrize("G,ncols", [(1, 5), (8, 5), (9, 6), (257, 7), (4096, 4),
                                     (2048, 10)])
def test_grouped_acc_lds_variant(ext, G, ncols):
    """The LDS kernel, up to its largest legal shapes: 4096 groups x 4 columns
    (128 KB of LDS, the engine's own upper corner) and 2048 x 10 (160 KB)."""
    ops_cycle = (OP_MIN, OP_SUM, OP_MAX, OP_FSUM, OP_COUNT)
    for j, (n, gid_kind, mask_kind) in enumerate([
            (50_000, "random", "mixed-bool"), (2049, "sparse", "none"),
            (257, "ascending", "mixed-u8"), (65, "one", "true-u8")]):
        _run_case(ext, n, G, _cycle_specs(ncols, j, ops_cycle), gid_kind=gid_kind,
                  mask_kind=mask_kind, seed=10 + j)


@gpu
def test_grouped_acc_every_op_dtype_pair(ext):
    """Each (op, dtype) the kernel can compute, on both variants; each pair it
    cannot compute raises instead of returning zeros."""
    n = 2049
    for G in (3, 300):
        for dt in _INT_TYPES:
            _run_case(ext, n, G, [(OP_SUM, dt), (OP_MIN, dt), (OP_MAX, dt)], seed=5)
            _run_case(ext, n, G, [(OP_SUM, dt), (OP_COUNT, None)], seed=6)
        for dt in _ALL_TYPES:
            _run_case(ext, n, G, [(OP_FSUM, dt)], mask_kind="mixed-bool", seed=7)
            _run_case(ext, n, G, [(OP_FSUM, dt), (OP_MAX, "i64")], seed=8)
    gid = torch.zeros(64, dtype=torch.int32).cuda()
    for op in (OP_SUM, OP_MIN, OP_MAX):
        for tdt in (torch.float64, torch.float32):
            with pytest.raises(RuntimeError):
                ext.grouped_acc(gid, None, [torch.ones(64, dtype=tdt).cuda()], [op], 2)
    for op in (OP_SUM, OP_FSUM, OP_MIN, OP_MAX):
        for tdt in (torch.float16, torch.bfloat16, torch.complex64):
            with pytest.raises(RuntimeError):
                ext.grouped_acc(gid, None, [torch.ones(64, dtype=tdt).cuda()], [op], 2)


@gpu
def test_grouped_acc_masks_and_empty_groups(ext):
    specs = [(OP_SUM, "i64"), (OP_FSUM, "f32"), (OP_COUNT, None), (OP_SUM, "bool")]
    lds = specs + [(OP_MIN, "i32"), (OP_MAX, "u8")]
    for mask_kind in ("none", "true-bool", "true-u8", "false-bool", "false-u8",
                      "mixed-bool", "mixed-u8"):
        for gid_kind in ("random", "ascending", "sparse", "one"):
            _run_case(ext, 2049, 8, specs, gid_kind, mask_kind, seed=20)
            _run_case(ext, 2049, 8, lds, gid_kind, mask_kind, seed=21)
            _run_case(ext, 2049, 700, lds, gid_kind, mask_kind, seed=22)


@gpu
def test_grouped_acc_int64_sums_wrap(ext):
    """Values near +-2^62: the sum leaves int64 and must come back modulo 2^64."""
    rng = random.Random(30)
    n = 4097
    big = [rng.choice((1, -1)) * ((1 << 62) - rng.randrange(1000)) for _ in range(n)]
    for G, extra in ((2, []), (8, []), (8, [OP_MAX]), (600, [])):
        gid = [rng.randrange(G) for _ in range(n)]
        ops = [OP_SUM, OP_COUNT] + extra
        cols = [big, None] + [big for _ in extra]
        tens = [None if c is None else torch.tensor(c, dtype=torch.int64).cuda()
                for c in cols]
        want, members = _reference(gid, None, cols, ops, G)
        exact = [sum(big[i] for i in m) for m in members]
        assert any(not I64_MIN <= v <= I64_MAX for v in exact)  # it does wrap
        out = ext.grouped_acc(torch.tensor(gid, dtype=torch.int32).cuda(), None,
                              tens, ops, G).cpu()
        for c in range(len(ops)):
            assert out[c].tolist() == want[c], (G, c)


@gpu
@pytest.mark.parametrize("G", [4, 8, 9, 1000])
def test_grouped_acc_float_sum_error_bound(ext, G):
    """Random doubles of mixed sign and magnitude. Summation of n numbers in
    any order (and any tree: per-thread, per-wave, per-block partial sums) has
    error at most n * 2^-53 * sum|x_i| against the correctly rounded sum, with
    n the number of rows that reach the group. No further margin."""
    rng = random.Random(40 + G)
    n = 50_000
    vals = [rng.uniform(-1.0, 1.0) * 10.0 ** rng.randint(-6, 6) for _ in range(n)]
    gid = [rng.randrange(G) for _ in range(n)]
    mask = [rng.random() < 0.8 for _ in range(n)]
    v32 = torch.tensor(vals, dtype=torch.float32)
    specs = [(vals, torch.tensor(vals, dtype=torch.float64)),
             (v32.to(torch.float64).tolist(), v32)]
    ops = [OP_FSUM, OP_FSUM] + ([OP_MAX] if G == 8 else [])
    tens = [t.cuda() for _, t in specs]
    if G == 8:  # the LDS kernel at a group count the register kernel also takes
        tens.append(torch.zeros(n, dtype=torch.int64).cuda())
    out = ext.grouped_acc(torch.tensor(gid, dtype=torch.int32).cuda(),
                          torch.tensor(mask).cuda(), tens, ops, G).cpu()
    members = [[] for _ in range(G)]
    for i in range(n):
        if mask[i]:
            members[gid[i]].append(i)
    for c, (ref_vals, _) in enumerate(specs):
        got = out[c].view(torch.float64).tolist()
        for g in range(G):
            xs = [ref_vals[i] for i in members[g]]
            bound = len(xs) * 2.0 ** -53 * math.fsum(abs(x) for x in xs)
            err = abs(got[g] - math.fsum(xs))
            assert err <= bound, (G, c, g, err, bound)


@gpu
def test_grouped_acc_refuses_oversize_shapes(ext):
    """Refused by the host checks, before any launch."""
    n = 64
    gid = torch.zeros(n, dtype=torch.int32).cuda()
    v = torch.ones(n, dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError):
        ext.grouped_acc(gid, None, [v], [OP_SUM], 4097)
    with pytest.raises(RuntimeError):
        ext.grouped_acc(gid, None, [v] * 5, [OP_SUM] * 5, 4096)
    with pytest.raises(RuntimeError):
        ext.grouped_acc(gid, None, [v] * 11, [OP_SUM] * 11, 4)
    with pytest.raises(RuntimeError):
        ext.grouped_acc(gid, None, [], [], 4)


_AGG_N = 12_000


def _agg_table_data():
    rng = random.Random(50)
    n = _AGG_N
    day0 = datetime.date(1995, 1, 1)
    return {
        "id": list(range(n)),
        "si": [rng.randint(-30000, 30000) for _ in range(n)],
        "i": [rng.randint(-(1 << 31), (1 << 31) - 1) for _ in range(n)],
        "b": [rng.randint(-(1 << 40), 1 << 40) for _ in range(n)],
        "dt": [day0 + datetime.timedelta(days=rng.randint(-4000, 4000)) for _ in range(n)],
        "dec": [rng.randint(-10 ** 6, 10 ** 6) / 100.0 for _ in range(n)],
        # quarters: every sum is exact, so both devices agree to the last bit
        "d": [rng.randint(-(1 << 20), 1 << 20) / 4.0 for _ in range(n)],
        "bo": [rng.random() < 0.5 for _ in range(n)],
        "nl": [None if rng.random() < 0.3 else rng.randint(-1000, 1000) for _ in range(n)],
    }


_AGG_SCHEMA = {"id": T.I64, "si": T.I16, "i": T.I32, "b": T.I64, "dt": T.DATE,
               "dec": T.DecimalType(12, 2), "d": T.F64, "bo": T.BOOL, "nl": T.I64}

_AGG_SQL = """
SELECT k, sum(si), sum(i), sum(b), sum(dec), sum(d), sum(nl),
       avg(si), avg(i), avg(dec), avg(d), avg(nl),
       count(*), count(nl), count_if(bo), count_if(i > 0),
       min(si), max(si), min(i), max(i), min(b), max(b), min(dt), max(dt),
       min(dec), max(dec), count_if(NOT bo), count_if(bo AND nl > 0),
       sum(i) FILTER (WHERE bo), count(*) FILTER (WHERE si > 0),
       avg(d) FILTER (WHERE nl IS NOT NULL), max(b) FILTER (WHERE bo)
FROM (SELECT id % {ng} AS k, * FROM agg) t GROUP BY k ORDER BY k
"""


@pytest.fixture(scope="module")
def agg_sessions():
    data = _agg_table_data()
    cpu = sail_amd.SessionContext(device="cpu")
    dev = sail_amd.SessionContext(device="cuda")
    tbl = Table.from_pydict(data, _AGG_SCHEMA, device="cpu")
    cpu.catalog.register_table("agg", tbl)
    dev.catalog.register_table("agg", tbl.to("cuda"))
    return cpu, dev


def test_agg_parity_query_runs_on_host():
    """The query of the parity test below is valid SQL for the engine (so a
    failure there is about the device path)."""
    cpu = sail_amd.SessionContext(device="cpu")
    cpu.catalog.register_table("agg", Table.from_pydict(_agg_table_data(), _AGG_SCHEMA,
                                                        device="cpu"))
    rows = cpu.sql(_AGG_SQL.format(ng=9)).collect()
    assert len(rows) == 9 and sum(r[12] for r in rows) == _AGG_N


@gpu
@pytest.mark.parametrize("ng", [8, 9, 4096, 4097])
def test_sql_aggregates_cpu_gpu_parity(ext, agg_sessions, monkeypatch, ng):
    """ng = 8 takes the register kernel (and the LDS kernel for min/max),
    9 and 4096 the LDS kernel, 4097 leaves the kernel path."""
    cpu, dev = agg_sessions
    calls = []
    real = ext.grouped_acc

    def spy(gid, mask, vals, ops, G):
        calls.append((int(G), len(ops)))
        return real(gid, mask, vals, ops, G)

    monkeypatch.setattr(ext, "grouped_acc", spy)
    got = dev.sql(_AGG_SQL.format(ng=ng)).collect()
    monkeypatch.undo()
    want = cpu.sql(_AGG_SQL.format(ng=ng)).collect()
    assert len(want) == ng
    assert got == want
    if ng <= 4096:
        assert calls and all(g == ng and c <= 4 for g, c in calls), calls
    else:
        assert not calls, calls


# ---------------------------------------------------------------------------
# hash_join.hip
# ---------------------------------------------------------------------------

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


EXTREME_KEYS = [I64_MIN, I64_MIN + 1, I64_MIN + 2, -1, 0, I64_MAX]


def _join_cases():
    rng = random.Random(60)
    cases = {}

    def rnd(n, span):
        return [rng.randrange(-span, span) for _ in range(n)]

    for nb in (0, 1, 2, 32, 33):
        cases[f"build{nb}"] = (rnd(nb, 20), rnd(300, 20))
    cases["probe0"] = (rnd(33, 20), [])
    cases["both0"] = ([], [])
    for np_ in (255, 256, 257, 2049, 5000):     # 2048 probe rows per workgroup
        cases[f"probe{np_}"] = (rnd(500, 400), rnd(np_, 400))
    cases["all_equal_33"] = ([7] * 33, [7, 8, 7, 6] * 70)
    cases["all_equal_300"] = ([-5] * 300, [-5] * 17 + [5] * 3)
    distinct = rng.sample(range(-10 ** 12, 10 ** 12), 3000)
    cases["all_distinct"] = (distinct[:2000], distinct[1000:])
    cases["none_present"] = (list(range(0, 2000, 2)), list(range(1, 2001, 2)))
    cases["extremes"] = (EXTREME_KEYS * 3 + rnd(30, 5), EXTREME_KEYS * 2 + rnd(300, 5))
    cases["extremes_apart"] = ([I64_MIN + 1, I64_MIN + 1, 3], [I64_MIN + 2, I64_MIN, 3])
    # 64 keys with one home slot near the end of the 128-slot table: the
    # probe sequence wraps past the end; absent keys with that home as well
    same = _same_home_keys(96, 64, 120)
    cases["one_home_wraps"] = (same[:64], same + same[:10] + rnd(100, 50))
    same = _same_home_keys(40, 33, 127, start=10 ** 15)
    cases["last_slot_home"] = (same[:33] + same[:5], same + same)
    return cases


JOIN_CASES = _join_cases()


@gpu
@pytest.mark.parametrize("case", sorted(JOIN_CASES))
def test_hash_join_matches_dict_reference(ext, case):
    from sail_amd.engine.joins import _expand_matches_gpu

    build, probe = JOIN_CASES[case]
    rows_of = collections.defaultdict(list)
    for j, k in enumerate(build):
        rows_of[k].append(j)
    want_counts = [len(rows_of.get(k, ())) for k in probe]
    want_pairs = sorted((i, j) for i, k in enumerate(probe) for j in rows_of.get(k, ()))
    p_idx, b_idx, counts = _expand_matches_gpu(
        torch.tensor(build, dtype=torch.int64).cuda(),
        torch.tensor(probe, dtype=torch.int64).cuda(), ext)
    assert counts.cpu().tolist() == want_counts
    p, b = p_idx.cpu().tolist(), b_idx.cpu().tolist()
    assert p == sorted(p)                       # probe_idx is non-decreasing
    pairs = sorted(zip(p, b))
    assert pairs == want_pairs                  # as a multiset: no pair twice
    assert len(set(pairs)) == len(pairs)


@gpu
def test_join_null_keys_never_match(ext):
    """The engine marks null keys with two sentinels at the bottom of the
    int64 range, one per side: a null matches nothing, not even a null, and
    real keys next to the sentinels keep their own matches."""
    from sail_amd.engine.joins import _expand_matches

    rng = random.Random(61)
    # (the two sentinel values themselves are reserved by the engine)
    near = [I64_MIN, I64_MIN + 3, -1, 0, I64_MAX]
    build = [rng.randrange(-3, 4) for _ in range(200)] + near
    probe = [rng.randrange(-3, 4) for _ in range(300)] + near
    bv = [rng.random() < 0.8 for _ in build]
    pv = [rng.random() < 0.8 for _ in probe]
    for k in range(len(near)):                  # these keys are not null
        bv[-1 - k] = pv[-1 - k] = True
    rows_of = collections.defaultdict(list)
    for j, k in enumerate(build):
        if bv[j]:
            rows_of[k].append(j)
    want = sorted((i, j) for i, k in enumerate(probe) if pv[i] for j in rows_of.get(k, ()))
    p_idx, b_idx, counts = _expand_matches(
        torch.tensor(build).cuda(), torch.tensor(probe).cuda(),
        torch.tensor(bv).cuda(), torch.tensor(pv).cuda())
    assert sorted(zip(p_idx.cpu().tolist(), b_idx.cpu().tolist())) == want
    assert counts.cpu().tolist() == [
        len(rows_of.get(k, ())) if pv[i] else 0 for i, k in enumerate(probe)]


@gpu
@pytest.mark.parametrize("case", sorted(JOIN_CASES))
def test_hg_group_matches_dict_reference(ext, case):
    build, probe = JOIN_CASES[case]
    for keys in (build, probe):
        gid, rep, counter = ext.hg_group(torch.tensor(keys, dtype=torch.int64).cuda())
        groups = collections.defaultdict(list)
        for i, k in enumerate(keys):
            groups[k].append(i)
        ng = int(counter.item())
        assert ng == len(groups)
        g = gid.cpu().tolist()
        assert len(g) == len(keys)
        if not keys:
            continue
        assert min(g) >= 0 and max(g) < ng
        by_gid = collections.defaultdict(list)
        for i, x in enumerate(g):
            by_gid[x].append(i)
        assert sorted(by_gid.values()) == sorted(groups.values())
        r = rep.cpu().tolist()
        for x in range(ng):
            assert g[r[x]] == x                 # rep[g] is a row of group g
