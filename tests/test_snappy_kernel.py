"""pq_snappy_decompress (ops/csrc/snappy.hip) on synthetic Snappy pages: one
case table, two backends.

Every case is (name, builder); a builder returns a list of pages
(stream, uncompressed_len, expected bytes or None, expected status). The
expectation is always the bytes the builder chose (tests/snappy_encode.py
expands its own element plan), never the output of a decoder.

* CPU half: every valid stream is accepted by pa.Codec("snappy") and
  decodes to the expectation, every malformed one is rejected by it, and
  the Python reference decoder agrees on both, status code included.
* GPU half (`gpu` mark): the pages of a case go through the HIP kernel in
  one launch. `out` is prefilled with 0xEE, pages are 4 KiB or more apart
  in both buffers, and everything outside the valid pages' output ranges
  must still be 0xEE afterwards, except inside a malformed page's own
  output range, whose contents are unspecified.

A malformed page sits between two valid neighbours, which must decode
correctly. Every malformed length or offset exceeds its bound by at most
64 bytes, so even a decoder that misses the check stays inside the 4 KiB
guards and fails here by assertion."""
import functools

import numpy as np
import pyarrow as pa
import pytest
import torch

import snappy_encode as S

GUARD = 4096
FILL_SRC = 0xFF
FILL_OUT = 0xEE


def _rng(seed):
    return np.random.default_rng(seed)


def _bytes(rng, n, lo=0, hi=256):
    return bytes(rng.integers(lo, hi, n, dtype=np.uint8))


class Page:
    def __init__(self, stream, ulen, expected, status):
        self.stream = bytes(stream)
        self.ulen = ulen
        self.expected = None if expected is None else bytes(expected)
        self.status = status


def _valid(s: S.Stream):
    return Page(s.finish(), len(s.out), s.out, S.OK)


# ---------------------------------------------------------------------------
# valid single-page cases
# ---------------------------------------------------------------------------

def _b_empty():
    return [Page(b"\x00", 0, b"", S.OK)]


def _b_lit(n, form=None):
    def build():
        return [_valid(S.Stream().lit(_bytes(_rng(n), n), form))]
    return build


def _b_copy1(length, offset):
    def build():
        data = _bytes(_rng(100 + offset), offset)
        return [_valid(S.Stream().lit(data).copy(1, length, offset))]
    return build


def _b_copy2(length, where):
    def build():
        rng = _rng(200 + length)
        if where == "off1":
            produced, offset = 5, 1
        elif where == "off_eq_len":
            produced, offset = length + 3, length
        elif where == "off_all_produced":
            produced = offset = 2 * length + 5
        else:
            produced, offset = 65535 + 2, 65535
        s = S.Stream().lit(_bytes(rng, produced)).copy(2, length, offset)
        return [_valid(s.lit(b"end"))]
    return build


def _b_copy4_near():
    s = S.Stream().lit(_bytes(_rng(31), 10)).copy(4, 7, 3).copy(4, 64, 17)
    return [_valid(s)]


def _b_copy4_far():
    s = S.Stream().lit(_bytes(_rng(32), 70000)).copy(4, 64, 69001)
    assert 69001 > 65535
    return [_valid(s.copy(4, 33, 70000 + 64))]      # reaches byte 0


def _b_lit_then_copy():
    """Each copy reads the bytes of the literal just before it."""
    s = S.Stream()
    rng = _rng(33)
    for n in (8, 1, 5, 64, 3):
        s.lit(_bytes(rng, n)).copy(2, min(n + 2, 64), n)
    return [_valid(s)]


def _b_copy_then_copy():
    """Each copy reads the bytes the copy before it wrote: fully, partly,
    and overlapping itself."""
    s = S.Stream().lit(_bytes(_rng(34), 6))
    s.copy(1, 4, 6).copy(1, 8, 4).copy(2, 3, 2).copy(2, 64, 3)
    s.copy(2, 64, 64).copy(1, 11, 10).copy(4, 20, 1)
    return [_valid(s)]


def _b_gt_literal_table():
    """1,300 literal/copy pairs: the literal table (512) fills, and the
    first element of each new batch is a copy of the literal that ended
    the batch before."""
    rng = _rng(35)
    s = S.Stream()
    for _ in range(1300):
        s.lit(_bytes(rng, 3)).copy(1, 4, 3)
    return [_valid(s)]


def _b_gt_copy_table():
    """2,100 copies in a chain, each reading the four bytes the one before
    wrote: the copy table (1024) fills twice, and the first copy of a new
    batch reads the last bytes of the batch before."""
    s = S.Stream().lit(_bytes(_rng(36), 4))
    for i in range(2100):
        s.copy(1, 4 + i % 3, 4)
    return [_valid(s)]


def _b_copy_chain_through_literals():
    """What a PLAIN column of small int64 compresses to: per value a short
    literal and a copy of the previous value's zero bytes, which the
    previous value's copy wrote. The kernel points such a copy at its
    predecessor's own source; the chain is 700 values long."""
    rng = _rng(37)
    s = S.Stream().lit(_bytes(rng, 3) + bytes(5))
    for _ in range(700):
        s.lit(_bytes(rng, 3, 1)).copy(1, 5, 8)
    return [_valid(s)]


def _b_copy_of_copy_shapes():
    """A copy reading its predecessor copy A: inside A and itself
    overlapping; straddling A's start and A's end; inside an A that
    overlaps itself; inside A across a literal in between."""
    rng = _rng(38)
    s = S.Stream().lit(_bytes(rng, 40))
    s.copy(2, 20, 30)          # A: linear, bytes 40..59
    s.copy(2, 30, 7)           # inside A (53..59), period 7 < length
    s.copy(2, 12, 12)          # inside the copy before it, linear
    s.copy(2, 10, 15)          # straddles the start of the copy before it
    s.lit(_bytes(rng, 2))
    s.copy(2, 6, 8)            # the copy before it, across the literal
    s.copy(2, 9, 3)            # overlapping A ...
    s.copy(2, 5, 6)            # ... and a copy inside that A
    s.copy(2, 8, 4).copy(1, 8, 8).copy(1, 4, 8).copy(1, 4, 2)
    return [_valid(s)]


def _mixed_near(seed, n_elems):
    """Random elements with offsets of at most 40: most copies read bytes
    that one of the last few copies wrote."""
    rng = _rng(seed)
    s = S.Stream().lit(_bytes(rng, 9))
    for _ in range(n_elems):
        have = len(s.out)
        if rng.integers(0, 3) == 0:
            s.lit(_bytes(rng, int(rng.integers(1, 6))))
        else:
            s.copy(2, int(rng.integers(1, 30)),
                   int(rng.integers(1, min(have, 40) + 1)))
    return s


def _b_near_offsets():
    return [_valid(_mixed_near(43, 3000)), _valid(_mixed_near(44, 500))]


def _mixed(seed, n_elems):
    rng = _rng(seed)
    s = S.Stream().lit(_bytes(rng, 9))
    for _ in range(n_elems):
        r = int(rng.integers(0, 4))
        have = len(s.out)
        if r == 0:
            s.lit(_bytes(rng, int(rng.integers(1, 80))))
        elif r == 1:
            s.copy(1, int(rng.integers(4, 12)),
                   int(rng.integers(1, min(have, 2047) + 1)))
        elif r == 2:
            s.copy(2, int(rng.integers(1, 65)),
                   int(rng.integers(1, min(have, 65535) + 1)))
        else:
            s.copy(4, int(rng.integers(1, 65)), int(rng.integers(1, have + 1)))
    return s


def _b_many_pages():
    """Nine pages of three distinct sizes, empty pages between full ones;
    the layout gives them odd source and output skews."""
    empty = Page(b"\x00", 0, b"", S.OK)
    a, b, c = (_valid(_mixed(40, 60)), _valid(_mixed(41, 400)),
               _valid(S.Stream().lit(_bytes(_rng(42), 61))))
    return [a, empty, b, c, a, empty, empty, b, c]


def _b_8200_pages():
    """More pages than the 8192-block grid cap: the grid-stride loop."""
    pages = []
    for p in range(8200):
        s = S.Stream().lit(p.to_bytes(3, "little")).copy(1, 4 + p % 8, 3)
        pages.append(_valid(s))
    return pages


def _b_real(kind):
    def build():
        rng = _rng(50)
        if kind == "low_entropy":
            data = _bytes(rng, 100_000, 0, 4)
        elif kind == "random":
            data = _bytes(rng, 100_000)
        else:
            words = [b"the ", b"quick ", b"brown ", b"fox ", b"jumps ",
                     b"over ", b"lazy ", b"dog. ", b"pack my box with ",
                     b"five dozen liquor jugs\n"]
            idx = rng.integers(0, len(words), 40_000)
            data = b"".join(words[i] for i in idx)
            assert len(data) > 4 * 65536
        stream = pa.Codec("snappy").compress(data, asbytes=True)
        if kind != "random":
            assert len(stream) < len(data) // 2
        return [Page(stream, len(data), data, S.OK)]
    return build


# ---------------------------------------------------------------------------
# malformed cases: [valid neighbour, malformed page, valid neighbour]
# ---------------------------------------------------------------------------

def _between(bad):
    return [_valid(_mixed(60, 50)), bad, _valid(_mixed(61, 70))]


def _base():
    return S.Stream().lit(b"abcdefgh").copy(2, 4, 8)     # 12 bytes


def _b_bad_preamble(delta):
    def build():
        s = _base()
        return _between(Page(s.finish(12 + delta), 12, None, S.PREAMBLE))
    return build


def _b_bad_literal_truncated():
    s = S.Stream().lit(b"abcdefgh")
    s.raw(S.literal_header(40) + b"x" * 30)               # 10 bytes short
    return _between(Page(s.finish(48), 48, None, S.TRUNCATED))


def _b_bad_offset0():
    s = S.Stream().lit(b"abcdefgh").raw(S.copy2(4, 0))
    return _between(Page(s.finish(12), 12, None, S.BAD_OFFSET))


def _b_bad_offset_past():
    s = S.Stream().lit(b"abcdefgh").raw(S.copy2(4, 9))    # 8 produced
    return _between(Page(s.finish(12), 12, None, S.BAD_OFFSET))


def _b_bad_copy_overrun():
    s = S.Stream().lit(b"abcdefgh").raw(S.copy2(20, 4))   # 10 bytes over
    return _between(Page(s.finish(18), 18, None, S.OVERRUN))


def _b_bad_literal_overrun():
    s = S.Stream().lit(b"abcdefgh").raw(S.literal_header(9) + b"y" * 9)
    return _between(Page(s.finish(16), 16, None, S.OVERRUN))


def _b_bad_input_ends_early():
    s = _base()                                           # 12 of 20 bytes
    return _between(Page(s.finish(20), 20, None, S.TRUNCATED))


def _b_bad_tag_cut():
    stream = _base().finish()[:-1]                        # offset byte gone
    return _between(Page(stream, 12, None, S.TRUNCATED))


def _b_bad_trailing():
    return _between(Page(_base().finish() + b"\x00", 12, None, S.TRAILING))


CASES = [
    ("empty_page", _b_empty),
] + [(f"literal_{n}", _b_lit(n)) for n in (1, 60, 61, 256, 257, 65537)] + [
    (f"literal_5_forced_{f}_length_bytes", _b_lit(5, f)) for f in (1, 2, 3, 4)
] + [
    (f"copy1_len{ln}_off{off}", _b_copy1(ln, off))
    for ln in (4, 11) for off in (1, 2047)
] + [
    (f"copy2_len{ln}_{w}", _b_copy2(ln, w))
    for ln in (1, 64)
    for w in ("off1", "off_eq_len", "off_all_produced", "off65535")
] + [
    ("copy4_near", _b_copy4_near),
    ("copy4_off_gt_65535", _b_copy4_far),
    ("literal_then_copy_of_it", _b_lit_then_copy),
    ("copy_then_copy_of_it", _b_copy_then_copy),
    ("copy_chain_through_literals_700_values", _b_copy_chain_through_literals),
    ("copy_of_copy_inside_straddling_overlapping", _b_copy_of_copy_shapes),
    ("random_near_offsets_3000_elements", _b_near_offsets),
    ("literal_table_refill_first_copy_reads_last_literal",
     _b_gt_literal_table),
    ("copy_table_refill_first_copy_reads_last_copy", _b_gt_copy_table),
    ("nine_pages_three_sizes_skews_empty_between", _b_many_pages),
    ("8200_pages_grid_stride", _b_8200_pages),
    ("real_low_entropy_100k", _b_real("low_entropy")),
    ("real_random_100k", _b_real("random")),
    ("real_text_300k_several_blocks", _b_real("text")),
    ("bad_preamble_plus_1", _b_bad_preamble(+1)),
    ("bad_preamble_minus_1", _b_bad_preamble(-1)),
    ("bad_literal_truncated_by_end_of_input", _b_bad_literal_truncated),
    ("bad_copy_offset_0", _b_bad_offset0),
    ("bad_copy_offset_one_past_produced", _b_bad_offset_past),
    ("bad_copy_overruns_uncompressed_len", _b_bad_copy_overrun),
    ("bad_literal_overruns_uncompressed_len", _b_bad_literal_overrun),
    ("bad_input_ends_early", _b_bad_input_ends_early),
    ("bad_input_ends_inside_copy_tag", _b_bad_tag_cut),
    ("bad_one_trailing_byte", _b_bad_trailing),
]

_BUILDERS = dict(CASES)
NAMES = [n for n, _ in CASES]
assert len(_BUILDERS) == len(CASES)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _BUILDERS[name]()


def _layout(pages):
    """(buf, table, out_len, [out_off]): every page has GUARD or more
    filler bytes on both sides in both buffers; offsets cycle through all
    residues mod 4, source and output out of step."""
    total_src = sum(len(p.stream) for p in pages) + (len(pages) + 1) * (GUARD + 4)
    buf = np.full(total_src + 16, FILL_SRC, dtype=np.uint8)
    rows, out_offs = [], []
    at_s, at_o = 0, 0
    for i, p in enumerate(pages):
        at_s += GUARD
        while at_s % 4 != (2 * i + 1) % 4:
            at_s += 1
        at_o += GUARD
        while at_o % 4 != (i + 3) % 4:
            at_o += 1
        buf[at_s:at_s + len(p.stream)] = np.frombuffer(p.stream, dtype=np.uint8)
        rows.append((at_s, len(p.stream), p.ulen, at_o, 0, 0))
        out_offs.append(at_o)
        at_s += len(p.stream)
        at_o += p.ulen
    assert at_s + GUARD <= buf.size
    table = torch.from_numpy(np.asarray(rows, dtype=np.int64).reshape(-1, 6))
    return torch.from_numpy(buf), table, at_o + GUARD, out_offs


def _check(pages, out_offs, out, status, name):
    out = out.cpu().numpy()
    status = status.cpu()
    assert status.dtype == torch.int32 and status.shape == (len(pages),)
    assert status.tolist() == [p.status for p in pages], name
    want = np.full(out.size, FILL_OUT, dtype=np.uint8)
    for p, off in zip(pages, out_offs):
        if p.expected is not None:
            want[off:off + p.ulen] = np.frombuffer(p.expected, dtype=np.uint8)
        else:               # malformed: its own output range is unspecified
            want[off:off + p.ulen] = out[off:off + p.ulen]
    if not np.array_equal(out, want):
        bad = np.nonzero(out != want)[0]
        raise AssertionError(
            f"{name}: {bad.size} wrong bytes, first at {bad[:8].tolist()}: "
            f"got {out[bad[:8]].tolist()} want {want[bad[:8]].tolist()}")


def _run(name, ext, dev):
    pages = _case(name)
    buf, table, out_len, out_offs = _layout(pages)
    out = torch.full((out_len,), FILL_OUT, dtype=torch.uint8, device=dev)
    status = ext.pq_snappy_decompress(buf.to(dev), table.to(dev), out)
    _check(pages, out_offs, out, status, name)


@pytest.mark.parametrize("name", NAMES)
def test_cpu_case(name):
    """pyarrow's decoder and the Python reference decoder on every page."""
    codec = pa.Codec("snappy")
    for p in _case(name):
        got, st = S.decompress(p.stream, p.ulen)
        assert st == p.status, name
        if p.status == S.OK:
            assert p.expected is not None and len(p.expected) == p.ulen
            theirs = codec.decompress(p.stream, decompressed_size=p.ulen,
                                      asbytes=True)
            assert theirs == p.expected, name
            assert got == p.expected, name
        else:
            with pytest.raises((OSError, pa.ArrowInvalid)):
                codec.decompress(p.stream, decompressed_size=p.ulen)


@pytest.mark.parametrize("name", NAMES)
def test_sim_case(name):
    """The laid-out table through the simulator entry point that the CPU
    orchestration tests use: same guards, same checks as on the GPU."""
    _run(name, S.SIM, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_case(name):
    from sail_amd.ops import kernels

    _run(name, kernels.require(), "cuda:0")


@pytest.mark.gpu
def test_gpu_wrapper_rejects_bad_tables():
    """The host wrapper refuses, before any launch, a table that is not
    int64 [n,6], a length of 2^31 or more, and a range outside its
    tensor."""
    from sail_amd.ops import kernels

    ext = kernels.require()
    dev = "cuda:0"
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)

    def table(rows, dtype=torch.int64):
        return torch.tensor(rows, dtype=dtype, device=dev)

    for bad in (table([[0, 1, 0, 0, 0, 0]], torch.int32),
                table([[0, 1, 0, 0, 0]]),
                table([[0, 1, 1 << 31, 0, 0, 0]]),
                table([[0, 1, -1, 0, 0, 0]]),
                table([[60, 5, 0, 0, 0, 0]]),
                table([[0, 1, 8, 60, 0, 0]]),
                table([[-1, 1, 0, 0, 0, 0]])):
        with pytest.raises(RuntimeError):
            ext.pq_snappy_decompress(buf, bad, out)


def test_entry_point_is_registered():
    """module.cpp registers the entry point this file's cases drive."""
    import os
    import re

    from sail_amd.ops import kernels

    src = os.path.join(os.path.dirname(kernels.__file__), "csrc", "module.cpp")
    with open(src) as f:
        assert re.search(r'm\.def\(\s*"pq_snappy_decompress"', f.read())
