"""pq_bytearray_index and pq_gather_bytes (ops/csrc/parquet_bytearray.hip):
the PLAIN BYTE_ARRAY length chain and the byte gather.

One case table per entry point, two backends, the shape of
tests/test_pq_delta_fused.py. A builder lays out pages of strings of its own
choosing with tests/pq_encode.py (plain_byte_array, Layout, page_table); the
expectation is those strings and the positions the builder put them at,
never the output of a simulator or of a kernel. Every comparison is exact.
Every index case runs with the first page at output row 0 and at row 3.

* CPU half: each case through tests/pq_bytearray_sim.py.
* GPU half (`gpu` mark): the same cases through the HIP extension, and for
  well-formed cases bit for bit against pq_bytearray_walk +
  pq_gather_strings of the same extension on the same buffer.

Sizes: the index kernel stages a page through LDS in windows of W = 2048
bytes that start on 16-byte boundaries of the address space, keeps two of
them, and writes its results in batches of 64 values; one wave owns a page,
four pages share a workgroup and the grid is capped at 8,192 workgroups
(32,768 pages in flight; a page beyond that is a wave's second page). The
gather kernel takes chunks of 32 to 512 values per workgroup, 16 output
bytes per lane and step, reads each value's part of those 16 bytes as whole
aligned dwords of the buffer, and is capped at 8,192 workgroups too: its
grid strides from 8,192 * 512 = 4,194,304 values on.

The rejection cases hand the kernel pages that break the format. They check
bounds the kernel enforces by construction (every length is compared with
the page region before it is used), in the manner of
tests/test_snappy_kernel.py, and pass in the simulator first."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from sail_amd.datasource import gpu_parquet as G

import pq_bytearray_sim as S
import pq_encode as E

W = 2048          # kWin
BATCH = 64        # kBatch
FIRST_ROWS = (0, 3)


def _rng(seed):
    return np.random.default_rng(seed)


def _rand_strings(rng, n, lo, hi):
    return [rng.bytes(int(k)) for k in rng.integers(lo, hi + 1, n)]


def _next_off(lay, skew, gap=1):
    """The offset Layout.add(payload, skew, gap) is about to return."""
    off = len(lay._buf) + gap
    while off % 4 != skew:
        off += 1
    return off


class Page:
    """One page of a case. `strings` may be a function of the page's offset
    in the buffer. src_len defaults to the payload's length and n to the
    number of strings; `status` and `resolved` state what a malformed page
    must give (resolved: how many leading values are still described);
    `tail` is raw bytes behind the values, inside the page."""

    def __init__(self, strings, skew=0, gap=1, src_len=None, n=None,
                 status=0, resolved=None, tail=b""):
        self.strings, self.skew, self.gap, self.tail = strings, skew, gap, tail
        self.src_len, self.n = src_len, n
        self.status, self.resolved = status, resolved


class Case:
    def __init__(self, first_row, pages):
        lay = E.Layout()
        rows, self.lengths, self.src_pos, self.status = [], [], [], []
        self.blob = b""
        base = first_row
        for pg in pages:
            off0 = _next_off(lay, pg.skew, pg.gap)
            strings = pg.strings(off0) if callable(pg.strings) else pg.strings
            payload = E.plain_byte_array(strings) + pg.tail
            off = lay.add(payload, pg.skew, pg.gap)
            assert off == off0
            src_len = len(payload) if pg.src_len is None else pg.src_len
            n = len(strings) if pg.n is None else pg.n
            good = len(strings) if pg.resolved is None else pg.resolved
            assert (pg.status == 0) == (good == n)
            rows.append((off, src_len, n, base, 0, 0))
            at = off
            for s in strings[:good]:
                self.lengths.append(len(s))
                self.src_pos.append(at + 4)
                self.blob += s
                at += 4 + len(s)
            self.lengths += [0] * (n - good)
            self.src_pos += [off] * (n - good)
            self.status.append(pg.status)
            base += n
        self.buf = lay.finish()
        self.rows = rows
        self.pages = E.page_table(rows)
        self.first, self.total = first_row, base
        self.well_formed = not any(self.status)


# -- index builders -----------------------------------------------------------

def _b_page_sizes(first_row):
    rng = _rng(1)
    return Case(first_row, [Page(_rand_strings(rng, n, 0, 20), k % 4)
                            for k, n in enumerate((1, 2, 63, 64, 65, 257, 0,
                                                   128, 129))])


def _b_all_empty(first_row):
    return Case(first_row, [Page([b""] * 200, 1), Page([b""], 2),
                            Page([b""] * 600, 3)])   # 2,400 bytes: 2 windows


def _b_random_lengths(first_row):
    rng = _rng(3)
    pages = [Page(_rand_strings(rng, 70, 0, 300), k) for k in range(4)]
    assert all(4 * W < len(E.plain_byte_array(p.strings)) < 7 * W
               for p in pages)
    return Case(first_row, pages)


def _b_long_value(first_row):
    """One value of 3 W + 1 bytes between short ones: the walk skips windows;
    then 5 W, and one that ends exactly where a window does."""
    rng = _rng(4)
    short = lambda: _rand_strings(rng, 3, 1, 9)      # noqa: E731
    p1 = short() + [rng.bytes(3 * W + 1)] + short()
    p2 = [rng.bytes(5 * W)] + short() + [rng.bytes(2 * W + 7)]

    def p3(off):
        head = [b"ab", b""]
        used = 4 + 2 + 4 + 4            # two values and the next prefix
        fill = 3 * W - off % 16 - used  # value ends at the end of window 2
        return head + [rng.bytes(fill)] + short()

    return Case(first_row, [Page(p1, 1), Page(p2, 2), Page(p3, 3)])


def _b_prefix_straddle(first_row):
    """The second value's prefix starts j bytes before the end of window 0
    and the third's j bytes before the end of window 1, j = 0..4 (0 and 4:
    the prefix touches the boundary from either side)."""
    rng = _rng(5)
    pages = []
    for j in range(5):
        for skew in (0, 3):
            def strings(off, j=j):
                first = W - off % 16 - j - 4
                return [rng.bytes(first), rng.bytes(W - 4), b"xyz", b"",
                        rng.bytes(40)]
            pages.append(Page(strings, skew))
    case = Case(first_row, pages)
    for k, (off, _len, _n, row, _a, _b) in enumerate(case.rows):
        second, third = (case.src_pos[row - first_row + i] - 4 - off
                         for i in (1, 2))
        assert (second + off % 16) == W - k // 2, k
        assert (third + off % 16) == 2 * W - k // 2, k
    return case


def _b_source_alignment(first_row):
    """Pages at every offset mod 16 (so skew 0-3 and every start within a
    16-byte load), 70 values each."""
    rng = _rng(6)
    lay_probe, pages = 4, []
    for r in range(16):
        pages.append((r, _rand_strings(rng, 70, 0, 40)))
    out = []
    pos = lay_probe
    for r, strings in pages:
        gap = 1
        while True:
            off = pos + gap
            while off % 4 != r % 4:
                off += 1
            if off % 16 == r:
                break
            gap += 1
        out.append(Page(strings, r % 4, gap))
        pos = off + len(E.plain_byte_array(strings))
    case = Case(first_row, out)
    assert sorted(row[0] % 16 for row in case.rows) == list(range(16))
    return case


def _b_empty_between(first_row):
    """A page with n_values == 0 (its region holds a real value) between two
    full ones whose rows it must not touch; one more at the very end with
    out_row == total."""
    a = [bytes([0xA0 + i % 16]) * (1 + i % 7) for i in range(65)]
    b = [bytes([0xB0 + i % 16]) * (1 + i % 5) for i in range(130)]
    ghost = [b"\xEE" * 9]
    case = Case(first_row, [Page(a, 1), Page(ghost, 2, n=0, resolved=0),
                            Page(b, 3), Page(ghost, 0, n=0, resolved=0)])
    assert case.rows[1][3] == case.rows[2][3] and case.rows[3][3] == case.total
    return case


def _b_many_pages(first_row):
    rng = _rng(8)
    counts = rng.integers(1, 4, 8200)
    return Case(first_row, [Page(_rand_strings(rng, int(n), 0, 6), p % 4)
                            for p, n in enumerate(counts)])


def _b_grid_strides(first_row):
    """33,000 pages: with four pages to a workgroup and 8,192 workgroups,
    pages from 32,768 on are the second page of waves 0-231. Most pages hold
    one value. Pages 0-7 and 32,768-32,775, the first and second page of the
    same eight waves, span five or six windows with a prefix across a window
    boundary and a value longer than the ring, so a second page meets a ring
    and a walk state that its wave has used."""
    rng = _rng(13)

    def wide(off):
        return [rng.bytes(W - off % 16 - 6), rng.bytes(3 * W + 1), b"x", b"",
                rng.bytes(int(rng.integers(200, 2 * W)))]

    pages = []
    for p in range(33_000):
        if p < 8 or 32_768 <= p < 32_776:
            pages.append(Page(wide, p % 4))
        else:
            pages.append(Page([rng.bytes(int(rng.integers(0, 7)))], p % 4))
    case = Case(first_row, pages)
    assert len(case.rows) > 8192 * 4 + 8
    return case


def _good(rng, n=66):
    return _rand_strings(rng, n, 0, 30)


def _b_length_past_page(first_row):
    """The third value's length ends one byte past src_len; the bytes behind
    the page are the value's own last byte and real filler."""
    rng = _rng(9)
    bad = [b"one", b"three", rng.bytes(50), b"never"]
    cut = len(E.plain_byte_array(bad[:3])) - 1
    return Case(first_row, [Page(_good(rng), 1),
                            Page(bad, 2, src_len=cut, status=1, resolved=2),
                            Page(_good(rng), 3)])


def _b_length_far_past_page(first_row):
    """A length of 0xFFFFFFF0, and one that would end past the whole buffer,
    behind 70 good values (more than one batch)."""
    rng = _rng(10)
    pages = [Page(_good(rng), 0)]
    for k, ln in enumerate((0xFFFFFFF0, 1 << 20)):
        head = _rand_strings(rng, 70, 0, 25)
        pages.append(Page(head, 1 + k, tail=ln.to_bytes(4, "little") + b"tail",
                          n=71, status=1, resolved=70))
        pages.append(Page(_good(rng), 2))
    return Case(first_row, pages)


def _b_page_ends_in_prefix(first_row):
    """src_len ends 1, 2 and 3 bytes into the fourth value's prefix, and
    exactly in front of it (a page that is merely out of values)."""
    rng = _rng(11)
    pages = [Page(_good(rng), 3)]
    for inside in (1, 2, 3, 0):
        vals = [b"a", b"", rng.bytes(33), b"lost", b"lost too"]
        cut = len(E.plain_byte_array(vals[:3])) + inside
        pages.append(Page(vals, inside, src_len=cut, status=2, resolved=3))
        pages.append(Page(_good(rng), (inside + 1) % 4))
    return Case(first_row, pages)


def _b_more_values_than_page(first_row):
    """n_values is 5 (and 200) more than the page holds."""
    rng = _rng(12)
    a, b = _rand_strings(rng, 10, 0, 12), _rand_strings(rng, 130, 0, 12)
    return Case(first_row, [Page(_good(rng), 0),
                            Page(a, 1, n=15, status=2, resolved=10),
                            Page(_good(rng), 2),
                            Page(b, 3, n=330, status=2, resolved=130),
                            Page(_good(rng), 1)])


INDEX_CASES = [
    ("pages_of_1_2_63_64_65_257_0_128_129_values", _b_page_sizes),
    ("all_empty_strings", _b_all_empty),
    ("random_lengths_0_to_300_over_five_windows", _b_random_lengths),
    ("one_value_of_3w_plus_1_between_short_ones", _b_long_value),
    ("prefix_straddles_a_window_boundary_at_each_byte", _b_prefix_straddle),
    ("source_offsets_every_residue_mod_16", _b_source_alignment),
    ("empty_page_between_two_full_ones", _b_empty_between),
    ("many_pages_8200_of_1_to_3_values", _b_many_pages),
    ("grid_strides_33000_pages_second_pages_span_windows", _b_grid_strides),
    ("reject_length_one_byte_past_the_page", _b_length_past_page),
    ("reject_length_far_past_the_page_and_the_buffer", _b_length_far_past_page),
    ("reject_page_ends_inside_a_prefix", _b_page_ends_in_prefix),
    ("reject_n_values_larger_than_the_page_holds", _b_more_values_than_page),
]
_INDEX = dict(INDEX_CASES)
assert len(_INDEX) == len(INDEX_CASES)
INDEX_PARAMS = [(n, f) for n, _ in INDEX_CASES for f in FIRST_ROWS]


@functools.lru_cache(maxsize=None)
def _index_case(name, first_row):
    return _INDEX[name](first_row)


def _check_index(case, out, gather, what):
    lengths, src_pos, status = (t.cpu() for t in out)
    assert lengths.dtype == src_pos.dtype == torch.int64, what
    assert status.dtype == torch.int32, what
    assert lengths.numel() == src_pos.numel() == case.total, what
    assert status.tolist() == case.status, what
    # rows in front of the first page belong to nobody: zero
    assert not lengths[:case.first].any() and not src_pos[:case.first].any()
    got_len = lengths[case.first:].tolist()
    got_pos = src_pos[case.first:].tolist()
    if got_len != case.lengths or got_pos != case.src_pos:
        bad = [i for i in range(len(got_len))
               if (got_len[i], got_pos[i]) != (case.lengths[i],
                                               case.src_pos[i])][:6]
        raise AssertionError(
            f"{what}: rows {bad}: got "
            f"{[(got_len[i], got_pos[i]) for i in bad]} want "
            f"{[(case.lengths[i], case.src_pos[i]) for i in bad]}")
    # a gather over the result returns the described values' bytes
    offs = torch.zeros(case.total + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offs[1:])
    dev = out[0].device
    blob = gather(case.buf.to(dev), out[1], out[0], offs[:-1].to(dev),
                  int(offs[-1]))
    assert blob.cpu().numpy().tobytes() == case.blob, what


@pytest.mark.parametrize("name,first_row", INDEX_PARAMS)
def test_sim_index_case(name, first_row):
    case = _index_case(name, first_row)
    out = S.pq_bytearray_index(case.buf, case.pages, case.total)
    _check_index(case, out, S.pq_gather_bytes, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,first_row", INDEX_PARAMS)
def test_gpu_index_case(name, first_row):
    from sail_amd.ops import kernels

    ext = kernels.require()
    case = _index_case(name, first_row)
    buf, pages = case.buf.to("cuda:0"), case.pages.to("cuda:0")
    out = ext.pq_bytearray_index(buf, pages, case.total)
    _check_index(case, out, ext.pq_gather_bytes, name)
    if case.well_formed:
        old_len, old_pos = ext.pq_bytearray_walk(buf, pages, case.total)
        assert torch.equal(out[0], old_len) and torch.equal(out[1], old_pos)


# -- gather cases -------------------------------------------------------------

LENGTHS = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 4097, 70000)


class GatherCase:
    def __init__(self, buf, values):
        """values: (src_pos, length) in output order, back to back."""
        self.buf = torch.from_numpy(buf)
        self.src_pos = torch.tensor([v[0] for v in values], dtype=torch.int64)
        self.lengths = torch.tensor([v[1] for v in values], dtype=torch.int64)
        self.offsets = torch.zeros(len(values) + 1, dtype=torch.int64)
        torch.cumsum(self.lengths, 0, out=self.offsets[1:])
        self.total = int(self.offsets[-1])
        self.expected = np.concatenate(
            [np.zeros(0, np.uint8)] + [buf[s:s + n] for s, n in values])


def _source(rng, n):
    return np.frombuffer(rng.bytes(n), dtype=np.uint8).copy()


def _g_alignments(length):
    """`length` at every source and destination alignment mod 16: each
    tested value follows a filler that moves the output to the wanted
    residue."""
    def build():
        rng = _rng(100 + length)
        buf = _source(rng, length + 64 + E.TAIL_PAD)
        values, at = [], 0
        for s in range(16):
            for d in range(16):
                fill = (d - at) % 16
                values.append((int(rng.integers(0, 40)), fill))
                at += fill
                assert at % 16 == d
                values.append((16 + s, length))
                at += length
        return GatherCase(buf, values)
    return build


def _g_repeated_source():
    rng = _rng(200)
    return GatherCase(_source(rng, 64), [(13, 5)] * 10_000)


def _g_overlapping_sources():
    rng = _rng(201)
    buf = _source(rng, 4000)
    return GatherCase(buf, [(3 * i % 3900, 1 + (7 * i) % 90)
                            for i in range(3000)])


def _g_mixed_lengths_many_values():
    """2,100 values (more than one chunk at every chunk size), lengths 0-9
    with a 70,000-byte value in the middle."""
    rng = _rng(202)
    buf = _source(rng, 80_000)
    values = [(int(rng.integers(0, 9000)), int(k))
              for k in rng.integers(0, 10, 2100)]
    values[1000] = (7, 70_000)
    return GatherCase(buf, values)


def _g_source_ends_with_buffer(numel):
    """A buffer whose size is no multiple of 4 and has no padding behind it;
    every source ends at its last byte, so the last dword read is the
    buffer's partial one. Fillers move the output over all alignments."""
    def build():
        rng = _rng(300 + numel)
        buf = _source(rng, numel)
        values = []
        for ln in (1, 2, 3, 4, 5, 15, 16, 17, 33, numel - 1, numel):
            values += [(numel - ln, ln), (int(rng.integers(0, 8)),
                                          int(rng.integers(0, 6)))]
        return GatherCase(buf, values)
    return build


def _g_no_values():
    return GatherCase(_source(_rng(203), 32), [])


def _g_no_bytes():
    return GatherCase(_source(_rng(204), 32), [(i % 30, 0) for i in range(50)])


GATHER_CASES = [(f"length_{n}_every_alignment_mod_16", _g_alignments(n))
                for n in LENGTHS] + [
    ("one_5_byte_source_gathered_10000_times", _g_repeated_source),
    ("overlapping_sources", _g_overlapping_sources),
    ("2100_short_values_around_one_of_70000_bytes", _g_mixed_lengths_many_values),
    ("source_ends_with_a_buffer_of_61_bytes", _g_source_ends_with_buffer(61)),
    ("source_ends_with_a_buffer_of_62_bytes", _g_source_ends_with_buffer(62)),
    ("source_ends_with_a_buffer_of_63_bytes", _g_source_ends_with_buffer(63)),
    ("no_values", _g_no_values),
    ("values_but_no_bytes", _g_no_bytes),
]
_GATHER = dict(GATHER_CASES)
assert len(_GATHER) == len(GATHER_CASES)
GATHER_NAMES = [n for n, _ in GATHER_CASES]


@functools.lru_cache(maxsize=None)
def _gather_case(name):
    return _GATHER[name]()


def _check_gather(case, got, what):
    assert got.dtype == torch.uint8 and got.numel() == case.total, what
    g = got.cpu().numpy()
    if not np.array_equal(g, case.expected):
        bad = np.nonzero(g != case.expected)[0][:8]
        raise AssertionError(f"{what}: bytes {bad.tolist()}: got "
                             f"{g[bad].tolist()} want "
                             f"{case.expected[bad].tolist()}")


@pytest.mark.parametrize("name", GATHER_NAMES)
def test_sim_gather_case(name):
    c = _gather_case(name)
    _check_gather(c, S.pq_gather_bytes(c.buf, c.src_pos, c.lengths,
                                       c.offsets[:-1], c.total), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GATHER_NAMES)
def test_gpu_gather_case(name):
    from sail_amd.ops import kernels

    ext = kernels.require()
    c = _gather_case(name)
    args = [t.to("cuda:0") for t in (c.buf, c.src_pos, c.lengths,
                                     c.offsets[:-1])]
    got = ext.pq_gather_bytes(*args, c.total)
    _check_gather(c, got, name)
    assert torch.equal(got, ext.pq_gather_strings(*args, c.total)), name


@pytest.mark.gpu
def test_gpu_gather_grid_strides():
    """8,192 * 512 + 777 values of 0-3 bytes: with chunks of 512 values and
    8,192 workgroups, the first 777 / 512 workgroups take a second chunk and
    load their LDS tables again. No CPU half: a simulator has no grid."""
    from sail_amd.ops import kernels

    ext = kernels.require()
    rng = _rng(400)
    n = 8192 * 512 + 777
    buf = _source(rng, 4096)
    lens = rng.integers(0, 4, n)
    src = rng.integers(0, 4096 - 3, n)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    total = int(offs[-1])
    expected = buf[np.repeat(src - offs[:-1], lens) + np.arange(total)]
    args = [torch.from_numpy(a).to("cuda:0")
            for a in (buf, src, lens, offs[:-1].copy())]
    got = ext.pq_gather_bytes(*args, total)
    assert np.array_equal(got.cpu().numpy(), expected)
    assert torch.equal(got, ext.pq_gather_strings(*args, total))


# -- wrappers and registration ------------------------------------------------

def _wrapper_checks(index, gather, dev):
    case = _index_case("all_empty_strings", 0)
    buf, pages = case.buf.to(dev), case.pages.to(dev)
    with pytest.raises(RuntimeError, match="contiguous uint8"):
        index(buf.to(torch.int32), pages, case.total)
    with pytest.raises(RuntimeError, match=r"int64 \[n,6\]"):
        index(buf, pages[:, :5].contiguous(), case.total)
    with pytest.raises(RuntimeError, match="negative"):
        index(buf, pages, -1)
    lengths, src_pos, status = index(buf, pages[:0], 5)
    assert lengths.tolist() == [0] * 5 and src_pos.tolist() == [0] * 5
    assert status.numel() == 0
    # descriptors that do not fit the buffer or the outputs: status 3
    bad = E.page_table([(0, buf.numel() + 1, 1, 0, 0, 0),
                        (-4, 8, 1, 0, 0, 0),
                        (4, 8, 1, case.total, 0, 0),
                        (4, 8, 1, -1, 0, 0)]).to(dev)
    lengths, src_pos, status = index(buf, bad, case.total)
    assert status.tolist() == [3, 3, 3, 3]
    assert not lengths.any() and not src_pos.any()
    i64 = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="one length"):
        gather(buf, i64, i64[:3], i64, 0)
    with pytest.raises(RuntimeError, match="one length"):
        gather(buf, i64, i64.to(torch.int32), i64, 0)
    with pytest.raises(RuntimeError, match="negative"):
        gather(buf, i64, i64, i64, -1)
    # sources outside the buffer read as 0; nothing lands outside the output
    n = buf.numel()
    src = torch.tensor([n - 2, -3, 1 << 40], dtype=torch.int64, device=dev)
    lens = torch.tensor([4, 5, 6], dtype=torch.int64, device=dev)
    offs = torch.tensor([0, 4, 9], dtype=torch.int64, device=dev)
    got = gather(buf, src, lens, offs, 15).cpu().tolist()
    tail = case.buf[n - 2:].tolist()
    assert got == tail + [0, 0] + [0, 0, 0] + case.buf[:2].tolist() + [0] * 6


def test_sim_wrappers_check_their_arguments():
    _wrapper_checks(S.pq_bytearray_index, S.pq_gather_bytes, "cpu")


@pytest.mark.gpu
def test_gpu_wrappers_check_their_arguments():
    from sail_amd.ops import kernels

    ext = kernels.require()
    _wrapper_checks(ext.pq_bytearray_index, ext.pq_gather_bytes, "cuda:0")
    with pytest.raises(RuntimeError, match="device tensor"):
        ext.pq_bytearray_index(torch.zeros(32, dtype=torch.uint8),
                               E.page_table([]).to("cuda:0"), 0)


def test_entry_points_are_registered_with_their_own_table():
    """Both are registered in the split form that tests/test_pq_kernels.py
    leaves to other case tables, and the simulator object has them."""
    src = os.path.join(os.path.dirname(G.__file__), "..", "ops", "csrc",
                       "module.cpp")
    with open(src) as f:
        registered = set(re.findall(r'm\.def\(\s*\n\s*"(pq_\w+)"', f.read()))
    assert {"pq_bytearray_index", "pq_gather_bytes"} <= registered
    assert callable(S.SIM.pq_bytearray_index)
    assert callable(S.SIM.pq_gather_bytes)
    assert callable(S.SIM.pq_bytearray_walk) and callable(S.SIM.pq_delta_values)
