"""BOOLEAN / INT96 / BYTE_STREAM_SPLIT page kernels
(ops/csrc/parquet_types.hip) on synthetic pages: one case table, two
backends, the shape of tests/test_pq_kernels.py.

Every case is (name, builder). A builder encodes values of its own choosing
with tests/pq_types_sim.py's encoders; the expectation is always those
values (for INT96, microseconds computed in Python integers), never the
output of the simulator or of a kernel, and every comparison is exact.
Floats are compared as bytes, so NaN payloads, -0.0 and infinities count.

* CPU half: each case through the numpy twins (tests/pq_types_sim.py).
* GPU half (`gpu` mark): the same cases through the HIP extension, compared
  with the expectation and with the simulator's output for the same buffer.

Sizes: the kernels run 256 threads per block, one value per thread, and
split a page over blockIdx.y once the mean page passes 2048 values; 5000
values in one page is the smallest case that takes three slices, 8200 pages
the one that makes blockIdx.x stride."""
import datetime
import functools
import os
import re

import numpy as np
import pytest
import torch

from sail_amd.datasource import gpu_parquet as G

import pq_encode as E
import pq_types_sim as S

NEW_ENTRY_POINTS = {"pq_bool_unpack", "pq_int96_micros", "pq_bss_decode"}


class Case:
    def __init__(self, kind, buf, rows, expected, total, width=0):
        self.kind = kind
        self.buf = buf
        self.pages = E.page_table(rows)
        self.expected = expected
        self.total = total
        self.width = width


def _rng(seed):
    return np.random.default_rng(seed)


def _u8(data: bytes):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())


def run_case(case, ext, dev):
    buf = case.buf.to(dev)
    pages = case.pages.to(dev)
    if case.kind == "bool":
        return {"values": ext.pq_bool_unpack(buf, pages, case.total)}
    if case.kind == "int96":
        return {"values": ext.pq_int96_micros(buf, pages, case.total)}
    if case.kind == "bss":
        return {"bytes": ext.pq_bss_decode(buf, pages, case.total, case.width)}
    raise ValueError(case.kind)


REACHED = {"bool": {"pq_bool_unpack"}, "int96": {"pq_int96_micros"},
           "bss": {"pq_bss_decode"}}


# ---------------------------------------------------------------------------
# pq_bool_unpack
# ---------------------------------------------------------------------------

def _bool_case(value_lists, skews, pad_ones=True):
    """One page per list, packed back to back in the output. Padding bits
    of each page's last byte are 1 and the gap bytes around it 0xFF, so a
    bit read past n_values shows wherever the expectation has a 0."""
    lay = E.Layout()
    rows, exp, base = [], [], 0
    for vals, skew in zip(value_lists, skews):
        payload = S.bool_bits(vals, pad_ones=pad_ones)
        assert len(payload) == (len(vals) + 7) // 8
        rows.append((lay.add(payload, skew), len(payload), len(vals), base,
                     0, 0))
        exp += [int(v) for v in vals]
        base += len(vals)
    return Case("bool", lay.finish(), rows,
                {"values": torch.tensor(exp, dtype=torch.uint8)}, base)


def _b_bool_counts():
    rng = _rng(1)
    counts = [1, 0, 7, 9, 8, 63, 65, 64, 257, 1000]   # odd ones first
    lists = [rng.integers(0, 2, n).tolist() for n in counts]
    skews = [1, 3, 1, 2, 3, 1, 0, 3, 1, 3]
    case = _bool_case(lists, skews)
    rows = case.pages.tolist()
    assert sum(r[3] % 8 != 0 for r in rows) >= 5     # out_row off the byte
    assert sum(r[0] % 2 == 1 for r in rows) >= 7     # odd src_off
    return case


def _b_bool_empty_middle():
    """A, an empty page with a real all-ones payload whose out_row is B's,
    then B: B's first slot must hold B's value (0), A's last its own."""
    a = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 1]
    b = [0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1]
    lay = E.Layout()
    pa_, pe, pb = S.bool_bits(a, True), b"\xff\xff", S.bool_bits(b, True)
    rows = [(lay.add(pa_, 1), len(pa_), len(a), 0, 0, 0),
            (lay.add(pe, 3), len(pe), 0, len(a), 0, 0),
            (lay.add(pb, 3), len(pb), len(b), len(a), 0, 0)]
    return Case("bool", lay.finish(), rows,
                {"values": torch.tensor(a + b, dtype=torch.uint8)},
                len(a) + len(b))


def _b_bool_ones_zeros():
    """All-ones with zero padding, all-zeros with one padding, 77 each."""
    lay = E.Layout()
    p1 = S.bool_bits([1] * 77, pad_ones=False)
    p0 = S.bool_bits([0] * 77, pad_ones=True)
    rows = [(lay.add(p1, 3), len(p1), 77, 0, 0, 0),
            (lay.add(p0, 1), len(p0), 77, 77, 0, 0)]
    return Case("bool", lay.finish(), rows,
                {"values": torch.tensor([1] * 77 + [0] * 77,
                                        dtype=torch.uint8)}, 154)


def _b_bool_5000():
    return _bool_case([_rng(2).integers(0, 2, 5000).tolist()], [3])


def _b_bool_8200_pages():
    v = _rng(3).integers(0, 2, (8200, 3)).tolist()
    return _bool_case(v, [p % 4 for p in range(8200)])


# ---------------------------------------------------------------------------
# pq_int96_micros
# ---------------------------------------------------------------------------

def _int96_case(triple_lists, skews, expect=None):
    """triple_lists: per page, (nanos, julian_day) pairs. `expect`
    overrides the per-value expectation (boundary cases state theirs)."""
    lay = E.Layout()
    rows, exp, base = [], [], 0
    for vals, skew in zip(triple_lists, skews):
        payload = S.int96_page(vals)
        off = lay.add(payload, skew)
        assert off % 4 == skew
        rows.append((off, len(payload), len(vals), base, 0, 0))
        exp += [S.int96_micros(n, d) for n, d in vals]
        base += len(vals)
    if expect is not None:
        assert exp == expect           # the helper agrees with the literals
    return Case("int96", lay.finish(), rows,
                {"values": torch.tensor(exp, dtype=torch.int64)}, base)


def _b_int96_boundaries():
    day_us = 86_400_000_000
    epoch_ord = datetime.date(1970, 1, 1).toordinal()

    def jd(date):
        return 2440588 + date.toordinal() - epoch_ord

    y1, y9999 = datetime.date(1, 1, 1), datetime.date(9999, 12, 31)
    vals = [(0, 2440588),                      # the epoch
            (1000, 2440588),                   # +1 us
            (86_399_999_999_000, 2440587),     # -1 us
            (0, 2440589),                      # +1 day
            (0, 2440587),                      # -1 day
            (999, 2440588),                    # below one microsecond
            (86_399_999_999_999, 2440588),     # last nanosecond of the day
            (0, jd(y1)), (0, jd(y9999)),
            (86_399_999_999_999, jd(y9999))]
    expect = [0, 1, -1, day_us, -day_us, 0, 86_399_999_999,
              (y1.toordinal() - epoch_ord) * day_us,
              (y9999.toordinal() - epoch_ord) * day_us,
              (y9999.toordinal() - epoch_ord) * day_us + 86_399_999_999]
    assert jd(y1) == 1721426 and jd(y9999) == 5373484
    return _int96_case([vals], [1], expect)


def _b_int96_truncate_wrap():
    """Negative nanoseconds divide towards zero; extreme Julian days wrap
    in 64 bits."""
    vals = [(-1, 2440588), (-999, 2440588), (-1000, 2440588),
            (-1001, 2440588), (-(1 << 63), 2440588), ((1 << 63) - 1, 2440588),
            (0, -(1 << 31)), (0, (1 << 31) - 1), (-1, -(1 << 31))]
    expect = [0, 0, -1, -1, -9223372036854775, 9223372036854775,
              E.wrap64((-(1 << 31) - 2440588) * 86_400_000_000),
              E.wrap64(((1 << 31) - 1 - 2440588) * 86_400_000_000),
              E.wrap64((-(1 << 31) - 2440588) * 86_400_000_000)]
    return _int96_case([vals], [3], expect)


def _random_int96(rng, n):
    nanos = rng.integers(0, 86_400_000_000_000, n).tolist()
    days = rng.integers(2_300_000, 2_600_000, n).tolist()
    return list(zip(nanos, days))


def _b_int96_layout():
    rng = _rng(10)
    lists, skews = [], []
    for skew in range(4):
        for n in (0, 1, 64, 65, 257):
            lists.append(_random_int96(rng, n))
            skews.append(skew)
    return _int96_case(lists, skews)


def _b_int96_5000():
    return _int96_case([_random_int96(_rng(11), 5000)], [1])


# ---------------------------------------------------------------------------
# pq_bss_decode
# ---------------------------------------------------------------------------

def _bss_case(plain_pages, skews, width):
    lay = E.Layout()
    rows, exp, base = [], b"", 0
    for plain, skew in zip(plain_pages, skews):
        n = len(plain) // width
        payload = S.byte_stream_split(plain, width)
        rows.append((lay.add(payload, skew), len(payload), n, base, 0, 0))
        exp += plain
        base += n
    return Case("bss", lay.finish(), rows, {"bytes": _u8(exp)}, base, width)


def _positional(n, width, salt):
    """n values whose byte j differs from every other byte of the value and
    from byte j of the neighbours: a wrong stride or byte order shows."""
    i = np.arange(n, dtype=np.int64)[:, None]
    j = np.arange(width, dtype=np.int64)[None, :]
    b = ((i * 11 + j * 53 + salt) % 251).astype(np.uint8)
    assert n == 0 or all(len(set(row)) == width for row in b.tolist())
    return b.tobytes()


def _b_bss_counts(width):
    def build():
        counts = [0, 1, 2, 63, 64, 65, 257]
        skews = [1, 3, 1, 2, 3, 0, 1]
        return _bss_case([_positional(n, width, 7 + k)
                          for k, n in enumerate(counts)], skews, width)
    return build


def _b_bss_specials(width):
    def build():
        if width == 4:
            bits = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000,
                    0x7F800000, 0xFF800000, 0x00000001, 0x7F7FFFFF, 0x3F800000]
            plain = np.array(bits, dtype="<u4").tobytes()
            assert np.isnan(np.frombuffer(plain, "<f4")[:3]).all()
        else:
            bits = [0x7FF8000000000001, 0xFFF8123456789ABC, 0x7FF0000000000001,
                    0x8000000000000000, 0, 0x7FF0000000000000,
                    0xFFF0000000000000, 1, 0x7FEFFFFFFFFFFFFF,
                    0x3FF0000000000000]
            plain = np.array(bits, dtype="<u8").tobytes()
            assert np.isnan(np.frombuffer(plain, "<f8")[:3]).all()
        return _bss_case([plain, plain[width:], plain[:3 * width]],
                         [3, 1, 2], width)
    return build


def _b_bss_5000(width):
    def build():
        return _bss_case([_positional(5000, width, 3)], [1], width)
    return build


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------

CASES = [
    ("bool_n0_1_7_8_9_63_64_65_257_1000_unaligned", _b_bool_counts),
    ("bool_empty_page_shares_out_row_with_next", _b_bool_empty_middle),
    ("bool_all_ones_and_all_zeros_pages", _b_bool_ones_zeros),
    ("bool_5000_values_three_slices", _b_bool_5000),
    ("bool_8200_pages_grid_stride", _b_bool_8200_pages),
    ("int96_epoch_day_microsecond_year_boundaries", _b_int96_boundaries),
    ("int96_negative_nanos_truncate_and_wrap", _b_int96_truncate_wrap),
    ("int96_skew_0_to_3_x_n0_1_64_65_257", _b_int96_layout),
    ("int96_5000_values_three_slices", _b_int96_5000),
    ("bss_w4_n0_1_2_63_64_65_257_unaligned", _b_bss_counts(4)),
    ("bss_w8_n0_1_2_63_64_65_257_unaligned", _b_bss_counts(8)),
    ("bss_w4_float_specials_three_pages", _b_bss_specials(4)),
    ("bss_w8_double_specials_three_pages", _b_bss_specials(8)),
    ("bss_w4_5000_values_three_slices", _b_bss_5000(4)),
    ("bss_w8_5000_values_three_slices", _b_bss_5000(8)),
]

_BUILDERS = dict(CASES)
NAMES = [n for n, _ in CASES]
assert len(_BUILDERS) == len(CASES)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def _sim_out(name):
    """Simulator output of a case: computed once, shared by both halves."""
    return run_case(_case(name), S.SIM, "cpu")


def _check_expected(got, case, name):
    for key, want in case.expected.items():
        g = got[key].cpu()
        assert g.dtype == want.dtype and g.shape == want.shape, (name, key)
        if not torch.equal(g, want):
            bad = torch.nonzero(g != want).flatten()[:8].tolist()
            raise AssertionError(
                f"{name}/{key}: mismatches, first at {bad}: "
                f"got {g[bad].tolist()} want {want[bad].tolist()}")


@pytest.mark.parametrize("name", NAMES)
def test_sim_case(name):
    _check_expected(_sim_out(name), _case(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_case(name):
    from sail_amd.ops import kernels

    case = _case(name)
    got = run_case(case, kernels.require(), "cuda:0")
    _check_expected(got, case, name)
    sim = _sim_out(name)
    assert set(got) == set(sim)
    for key in sim:
        assert torch.equal(got[key].cpu(), sim[key]), (name, key)


def _bss_width_3(ext, dev):
    case = _case("bss_w4_n0_1_2_63_64_65_257_unaligned")
    with pytest.raises(RuntimeError, match="width must be 4 or 8"):
        ext.pq_bss_decode(case.buf.to(dev), case.pages.to(dev), case.total, 3)


def test_sim_bss_width_3_raises():
    _bss_width_3(S.SIM, "cpu")


@pytest.mark.gpu
def test_gpu_bss_width_3_raises():
    from sail_amd.ops import kernels

    _bss_width_3(kernels.require(), "cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NEW_ENTRY_POINTS))
def test_gpu_wrappers_check_their_arguments(name):
    """Device, dtype and table shape are checked before any launch."""
    from sail_amd.ops import kernels

    fn = getattr(kernels.require(), name)
    extra = (4,) if name == "pq_bss_decode" else ()
    case = _case("bool_all_ones_and_all_zeros_pages")
    buf, pages = case.buf.to("cuda:0"), case.pages.to("cuda:0")
    with pytest.raises(RuntimeError, match="device tensor"):
        fn(case.buf, pages, 0, *extra)
    with pytest.raises(RuntimeError, match="contiguous uint8"):
        fn(buf.to(torch.int32), pages, 0, *extra)
    with pytest.raises(RuntimeError, match=r"int64 \[n,6\]"):
        fn(buf, pages.to(torch.int32), 0, *extra)
    with pytest.raises(RuntimeError, match=r"int64 \[n,6\]"):
        fn(buf, pages[:, :5].contiguous(), 0, *extra)
    with pytest.raises(RuntimeError, match=r"int64 \[n,6\]"):
        fn(buf, pages.t(), 0, *extra)
    assert fn(buf, pages[:0], 0, *extra).numel() == 0


def test_every_new_entry_point_has_a_case():
    """The three entry points are registered (name on the line after
    `m.def(`, the form tests/test_pq_kernels.py leaves to other tables),
    and each is reached by a case of this table."""
    src = os.path.join(os.path.dirname(G.__file__), "..", "ops", "csrc",
                       "module.cpp")
    with open(src) as f:
        registered = set(re.findall(r'm\.def\(\s*\n\s*"(pq_\w+)"', f.read()))
    assert NEW_ENTRY_POINTS <= registered, NEW_ENTRY_POINTS - registered
    kinds = {_case(n).kind for n in NAMES}
    covered = set().union(*(REACHED[k] for k in kinds))
    assert covered == NEW_ENTRY_POINTS
    for name in NEW_ENTRY_POINTS:
        assert callable(getattr(S.SIM, name))
