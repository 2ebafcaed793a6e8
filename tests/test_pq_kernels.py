"""Parquet page-decode kernels (ops/csrc/parquet_decode.hip) on synthetic
pages: one case table, two backends.

Every case is (name, builder). A builder encodes values of its own choosing
with tests/pq_encode.py; the expectation is always those values, never the
output of the simulator or of a kernel, and every comparison is exact.

* CPU half: each case through the numpy simulator (tests/pq_sim.py), which
  validates encoder and simulator against each other without a GPU.
* GPU half (`gpu` mark): the same cases through the HIP extension, compared
  with the expectation and, separately, with the simulator's output for the
  same buffer (all outputs, including data_end and src_pos), so contract
  drift in either direction shows.

Case names say which kernel and which branch they reach."""
import functools

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from sail_amd.datasource import gpu_parquet as G

import pq_encode as E
import pq_sim

I64 = np.int64


class Case:
    def __init__(self, kind, buf, pages, expected, **kw):
        self.kind = kind
        self.buf = buf
        self.pages = pages if torch.is_tensor(pages) else E.page_table(pages)
        self.expected = expected      # name -> CPU tensor
        self.__dict__.update(kw)


def _i64(vals):
    return torch.from_numpy(np.array([int(v) for v in vals], dtype=I64)
                            .reshape(-1))


def _i32_bits(vals):
    """Unsigned 32-bit values -> int32 tensor with the same bit pattern."""
    return torch.from_numpy(np.array([int(v) for v in vals], dtype=np.uint32)
                            .reshape(-1).view(np.int32).copy())


def _u8(data: bytes):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())


def _rng(seed):
    return np.random.default_rng(seed)


# ---------------------------------------------------------------------------
# running a case against a backend (`ext` is the HIP extension or pq_sim)
# ---------------------------------------------------------------------------

def run_case(case, ext, dev):
    buf = case.buf.to(dev)
    pages = case.pages.to(dev)
    k = case.kind
    if k == "rle":
        return {"values": ext.pq_rle_decode(buf, pages, case.total)}
    if k == "delta":
        out, data_end = ext.pq_delta_decode(buf, pages, case.total)
        ext.pq_segscan(out, pages)
        return {"values": out, "data_end": data_end}
    if k == "segscan":
        data = case.data.clone().to(dev)
        ext.pq_segscan(data, pages)
        return {"values": data}
    if k == "plain":
        return {"bytes": ext.pq_plain_copy(buf, pages, case.total, case.width)}
    if k == "copy":
        out = torch.full((case.out_len,), 0xEE, dtype=torch.uint8, device=dev)
        ext.pq_copy_bytes(buf, pages, out)
        return {"bytes": out}
    if k == "flba":
        return {"values": ext.pq_flba_i64(buf, pages, case.total, case.width)}
    if k == "walk":
        lengths, src_pos = ext.pq_bytearray_walk(buf, pages, case.total)
        offs = torch.cumsum(lengths, 0) - lengths
        blob = ext.pq_gather_strings(buf, src_pos, lengths, offs,
                                     int(lengths.sum().item()))
        return {"lengths": lengths, "src_pos": src_pos, "blob": blob}
    if k == "dlba":
        # the DELTA_LENGTH_BYTE_ARRAY chain of the host: length deltas,
        # payload copy from data_end on, per-page scan to lengths
        deltas, data_end = ext.pq_delta_decode(buf, pages, case.total)
        rows, at = [], 0
        for r, de in zip(case.pages.tolist(), data_end.cpu().tolist()):
            rows.append((r[0] + de, r[1] - de, 0, 0, at, 0))
            at += r[1] - de
        blob = torch.full((at,), 0xEE, dtype=torch.uint8, device=dev)
        ext.pq_copy_bytes(buf, E.page_table(rows).to(dev), blob)
        ext.pq_segscan(deltas, pages)
        return {"lengths": deltas, "blob": blob, "data_end": data_end}
    if k == "dictcodes":
        # host entry point: strips the leading bit-width byte of each page
        dec = object.__new__(G._ColumnDecoder)
        dec.buf = buf
        dec.device = dev
        saved = G._ext
        G._ext = lambda: ext
        try:
            codes = dec._decode_dict_codes(ext, case.pages.tolist())
        finally:
            G._ext = saved
        return {"codes": codes}
    raise ValueError(k)


# ---------------------------------------------------------------------------
# pq_rle_decode
# ---------------------------------------------------------------------------

def _mixed_plan(rng, bw, tail=67):
    """~200 values: RLE runs and bit-packed groups; the last entry is a
    bit-packed run of `tail` values (padded by the encoder to 72)."""
    top = (1 << bw) - 1

    def rv(n=None):
        v = rng.integers(0, top + 1, n, dtype=np.uint64)
        return int(v) if n is None else [int(x) for x in v]

    return [("rle", 17, rv()), ("packed", rv(40)), ("rle", 1, top),
            ("packed", rv(8)), ("rle", 60, rv()), ("rle", 2, 0),
            ("packed", rv(tail))]


def _rle_single(plan, bw, skew, pad_varint=0, drop_pad=True):
    payload, vals = E.rle_hybrid(plan, bw, pad_varint)
    if drop_pad and plan[-1][0] == "packed":
        vals = vals[:len(vals) - (-len(plan[-1][1]) % 8)]
    lay = E.Layout()
    off = lay.add(payload, skew)
    rows = [(off, len(payload), len(vals), 0, 0, bw)]
    return Case("rle", lay.finish(), rows, {"values": _i32_bits(vals)},
                total=len(vals))


def _b_rle_bw(bw):
    def build():
        return _rle_single(_mixed_plan(_rng(100 + bw), bw), bw, skew=bw % 4)
    return build


def _b_rle_topbit():
    rng = _rng(7)
    hi = [int(x) | 0x80000000 for x in rng.integers(0, 1 << 31, 21)]
    plan = [("rle", 10, 0xFFFFFFFF), ("packed", hi), ("rle", 3, 0x80000001),
            ("packed", [0x80000000] * 8)]
    return _rle_single(plan, 32, skew=1, drop_pad=False)


def _b_rle_zero_len_run():
    plan = [("rle", 5, 3), ("rle", 0, 7), ("packed", [1, 2, 3, 4, 5, 6, 7, 0]),
            ("rle", 0, 6), ("rle", 4, 1), ("rle", 0, 2)]
    return _rle_single(plan, 3, skew=3)


def _b_rle_clamp():
    """n_values smaller than the runs cover, RLE and bit-packed; the page
    after each would be overwritten by an unclamped run."""
    lay = E.Layout()
    p0, _ = E.rle_hybrid([("rle", 100, 5)], 4)
    p1, v1 = E.rle_hybrid([("rle", 2, 9), ("packed", list(range(24)))], 5)
    p2, v2 = E.rle_hybrid([("rle", 6, 2)], 2)
    rows = [(lay.add(p0, 0), len(p0), 37, 0, 0, 4),
            (lay.add(p1, 1), len(p1), 13, 37, 0, 5),
            (lay.add(p2, 2), len(p2), 6, 50, 0, 2)]
    exp = [5] * 37 + v1[:13] + v2
    return Case("rle", lay.finish(), rows, {"values": _i32_bits(exp)},
                total=56)


def _b_rle_gt_kruns():
    """1,100 runs in one page: the 512-entry LDS run table is refilled
    three times."""
    rng = _rng(11)
    bw = 9
    plan = []
    for _ in range(550):
        plan.append(("rle", 3, int(rng.integers(0, 1 << bw))))
        plan.append(("packed", [int(x) for x in rng.integers(0, 1 << bw, 8)]))
    assert len(plan) > 2 * 512
    return _rle_single(plan, bw, skew=2)


def _b_rle_padded_varint():
    return _rle_single(_mixed_plan(_rng(12), 6), 6, skew=1, pad_varint=1)


def _b_rle_empty_page_between():
    lay = E.Layout()
    pa_, va = E.rle_hybrid([("rle", 9, 1), ("packed", [0, 1] * 4)], 1)
    pe, _ = E.rle_hybrid([("rle", 4, 1)], 1)
    pb, vb = E.rle_hybrid([("packed", [1, 0, 0, 1, 1, 1, 0, 1]), ("rle", 3, 0)], 1)
    rows = [(lay.add(pa_, 0), len(pa_), len(va), 0, 0, 1),
            (0, 0, 0, len(va), 0, 1),                      # as the host writes
            (lay.add(pe, 3), len(pe), 0, len(va), 0, 1),   # real payload, n=0
            (lay.add(pb, 1), len(pb), len(vb), len(va), 0, 1)]
    return Case("rle", lay.finish(), rows, {"values": _i32_bits(va + vb)},
                total=len(va) + len(vb))


def _b_rle_8200_pages():
    """More pages than the 8192-block grid cap: the grid-stride loop."""
    rng = _rng(13)
    lay = E.Layout()
    rows, exp = [], []
    for p in range(8200):
        a, b = int(rng.integers(0, 8)), [int(x) for x in rng.integers(0, 8, 3)]
        payload, vals = E.rle_hybrid([("rle", 2, a), ("packed", b)], 3)
        rows.append((lay.add(payload, p % 4), len(payload), 5, 5 * p, 0, 3))
        exp += vals[:5]
    return Case("rle", lay.finish(), rows, {"values": _i32_bits(exp)},
                total=5 * 8200)


# ---------------------------------------------------------------------------
# pq_delta_decode + pq_segscan
# ---------------------------------------------------------------------------

def _delta_case(value_lists, skews=None, forced_bw=None, want_widths=None,
                extra_rows=(), extra_end=(), block=E.BLOCK,
                mbpb=E.MINIBLOCKS):
    """One page per value list, packed back to back in the output."""
    lay = E.Layout()
    rows, exp, ends, base = [], [], [], 0
    for i, vals in enumerate(value_lists):
        payload, used = E.delta_binary_packed(vals, forced_bw, block, mbpb)
        if want_widths is not None:
            assert set(used) == set(want_widths), (used, want_widths)
        skew = (skews[i] if skews else i) % 4
        rows.append((lay.add(payload, skew), len(payload), len(vals), base,
                     0, 0))
        ends.append(len(payload))
        exp += list(vals)
        base += len(vals)
    for payload, out_row in extra_rows:       # hand-written empty pages
        rows.append((lay.add(payload, 1), len(payload), 0, out_row, 0, 0))
    ends += list(extra_end)
    return Case("delta", lay.finish(), rows,
                {"values": _i64(exp), "data_end": _i64(ends)}, total=base)


def _values_for_width(rng, bw, n):
    """n values whose every miniblock needs exactly `bw` bits."""
    nd = n - 1
    if bw == 64:
        deltas = [int(x) for x in rng.integers(E.INT64_MIN, E.INT64_MAX, nd,
                                               endpoint=True)]
        for i in range(0, nd, 32):
            deltas[i] = E.INT64_MIN
            if i + 1 < nd:
                deltas[i + 1] = E.INT64_MAX
    else:
        min_delta = -5
        top = (1 << bw) - 1
        adj = [int(x) for x in rng.integers(0, top + 1, nd, dtype=np.uint64)]
        for i in range(0, nd, 32):
            adj[i] = 0
            if i + 1 < nd:
                adj[i + 1] = top
        deltas = [min_delta + a for a in adj]
    vals = [int(rng.integers(-1000, 1000))]
    for d in deltas:
        vals.append(E.wrap64(vals[-1] + d))
    return vals


def _b_delta_bw(bw):
    def build():
        vals = _values_for_width(_rng(200 + bw), bw, 300)
        return _delta_case([vals], skews=[bw], forced_bw=bw,
                           want_widths=[bw])
    return build


def _b_delta_partial_blocks():
    rng = _rng(21)
    lists = [[int(x) for x in rng.integers(-10**15, 10**15, n)]
             for n in (1, 2, 32, 33, 128, 129, 130, 257)]
    return _delta_case(lists)


def _b_delta_extremes():
    vals = [E.INT64_MIN if i % 2 == 0 else E.INT64_MAX for i in range(131)]
    return _delta_case([vals], skews=[3])


def _b_delta_negative_min_delta():
    rng = _rng(22)
    falling = np.cumsum(-rng.integers(1, 10**9, 200)).tolist()
    wild = [0, E.INT64_MIN, -1, E.INT64_MAX, 0, 17] * 30
    deltas = [E.wrap64(wild[i + 1] - wild[i]) for i in range(len(wild) - 1)]
    assert min(deltas) == E.INT64_MIN
    return _delta_case([falling, wild], skews=[2, 1])


def _b_delta_40000():
    """16,384 deltas fit one LDS batch (128 blocks): three batches."""
    rng = _rng(23)
    vals = np.cumsum(rng.integers(-2**40, 2**40, 40000)).tolist()
    return _delta_case([vals], skews=[1])


def _b_delta_skews():
    rng = _rng(24)
    lists = [[int(x) for x in rng.integers(-2**62, 2**62, 70)]
             for _ in range(4)]
    return _delta_case(lists, skews=[0, 1, 2, 3])


def _b_delta_empty_middle():
    """Pages A, B, then 32 empty pages whose out_row is B's. See
    test_sim_case for what the unfixed decoder does here."""
    rng = _rng(25)
    a = [int(x) for x in rng.integers(10**6, 10**9, 50)]
    b = [int(x) for x in rng.integers(10**6, 10**9, 60)]
    hdr = E.delta_header(0, 12345)
    return _delta_case([a, b], extra_rows=[(hdr, 50)] * 32,
                       extra_end=[len(hdr)] * 32)


def _b_delta_empty_trailing():
    """Last page empty, out_row == total; total * 8 = 296 bytes is no
    multiple of 512."""
    rng = _rng(26)
    a = [int(x) for x in rng.integers(-10**9, 10**9, 37)]
    hdr = E.delta_header(0, -777)
    return _delta_case([a], extra_rows=[(hdr, 37)], extra_end=[len(hdr)])


def _b_delta_block256():
    """The geometry recent pyarrow writes for int64: 64-value miniblocks."""
    rng = _rng(29)
    lists = [[int(x) for x in rng.integers(-10**17, 10**17, n)]
             for n in (700, 65, 258)]
    return _delta_case(lists, skews=[1, 2, 3], block=256, mbpb=4)


def _b_delta_8200_pages():
    rng = _rng(27)
    v = rng.integers(-2**50, 2**50, (8200, 3)).tolist()
    return _delta_case(v)


def _b_dlba():
    """DELTA_LENGTH_BYTE_ARRAY: delta-coded lengths, data_end, payload copy
    to unaligned destinations, per-page scan."""
    rng = _rng(28)
    lay = E.Layout()
    rows, ends, lens, blob, base = [], [], [], b"", 0
    for p, n in enumerate((1, 40, 131, 7)):
        strs = [bytes(rng.integers(1, 256, int(k), dtype=np.uint8))
                for k in rng.integers(0, 30, n)]
        if p == 1:
            strs[0] = strs[-1] = b""
        page, head = E.delta_length_byte_array(strs)
        rows.append((lay.add(page, (p + 1) % 4), len(page), n, base, 0, 0))
        ends.append(head)
        lens += [len(s) for s in strs]
        blob += b"".join(strs)
        base += n
    return Case("dlba", lay.finish(), rows,
                {"lengths": _i64(lens), "blob": _u8(blob),
                 "data_end": _i64(ends)}, total=base)


# ---------------------------------------------------------------------------
# pq_segscan alone
# ---------------------------------------------------------------------------

def _b_segscan_tiles():
    """Segment lengths around the 2048-element tile; sentinel slots between
    segments must survive; full-range inputs make the sums wrap."""
    rng = _rng(31)
    lens = [0, 1, 2047, 2048, 2049, 4097]
    aux = [7, -3, 0, 1 << 40, -(1 << 62), E.INT64_MAX]
    gap = 3
    total = sum(lens) + gap * (len(lens) + 1)
    data = rng.integers(E.INT64_MIN, E.INT64_MAX, total, endpoint=True)
    exp = data.copy()
    rows, at = [], gap
    with np.errstate(over="ignore"):
        for n, a in zip(lens, aux):
            rows.append((0, 0, n, at, a, 0))
            exp[at:at + n] = np.cumsum(data[at:at + n], dtype=I64) + I64(a)
            at += n + gap
    true_sum = sum(int(x) for x in data[rows[5][3]:rows[5][3] + 4097])
    assert not E.INT64_MIN <= true_sum <= E.INT64_MAX  # the sums do wrap
    return Case("segscan", torch.zeros(16, dtype=torch.uint8), rows,
                {"values": torch.from_numpy(exp)},
                data=torch.from_numpy(data))


# ---------------------------------------------------------------------------
# pq_plain_copy / pq_copy_bytes / pq_flba_i64
# ---------------------------------------------------------------------------

def _b_plain(width):
    def build():
        rng = _rng(40 + width)
        lay = E.Layout()
        rows, exp, base = [], b"", 0
        for skew in range(4):
            for n in (0, 1, 2, 3, 257):
                dt = np.int32 if width == 4 else np.int64
                info = np.iinfo(dt)
                vals = rng.integers(info.min, info.max, n, dtype=dt,
                                    endpoint=True)
                payload = E.plain_fixed(vals)
                assert len(payload) == n * width
                rows.append((lay.add(payload, skew), len(payload), n, base,
                             0, width))
                exp += payload
                base += n
        return Case("plain", lay.finish(), rows, {"bytes": _u8(exp)},
                    total=base, width=width)
    return build


def _b_copy_bytes():
    """src skew x dst alignment x length; untouched output stays 0xEE."""
    rng = _rng(50)
    lay = E.Layout()
    rows, chunks, at = [], [], 0
    for skew in range(4):
        for dskew in range(4):
            for n in (0, 1, 3, 4, 5, 9, 1027):
                payload = bytes(rng.integers(0, 256, n, dtype=np.uint8))
                at += 2                       # 0xEE guard between ranges
                while at % 4 != dskew:
                    at += 1
                rows.append((lay.add(payload, skew), n, 0, 0, at, 0))
                chunks.append((at, payload))
                at += n
    out_len = at + 5
    exp = np.full(out_len, 0xEE, dtype=np.uint8)
    for a, payload in chunks:
        exp[a:a + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    return Case("copy", lay.finish(), rows, {"bytes": torch.from_numpy(exp)},
                out_len=out_len)


def _b_flba(width):
    def build():
        rng = _rng(60 + width)
        lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
        lay = E.Layout()
        rows, exp, base = [], [], 0
        for skew in range(4):
            vals = [0, -1, lo, hi, 1, lo + 1, hi - 1] + [
                int(x) for x in rng.integers(lo, hi, 13, endpoint=True)]
            vals = vals[skew:]
            payload = E.flba_be(vals, width)
            rows.append((lay.add(payload, skew), len(payload), len(vals),
                         base, 0, width))
            exp += vals
            base += len(vals)
            if skew == 1:                     # a page with no values
                rows.append((lay.add(b"", 2), 0, 0, base, 0, width))
        return Case("flba", lay.finish(), rows, {"values": _i64(exp)},
                    total=base, width=width)
    return build


# ---------------------------------------------------------------------------
# pq_bytearray_walk + pq_gather_strings
# ---------------------------------------------------------------------------

def _b_walk():
    rng = _rng(70)
    big = bytes(rng.integers(0, 256, 5000, dtype=np.uint8))
    p0 = [b"", b"", b"abc", b"", b"", big, b"tail", b""]
    p2 = [b"aa", b"bbb", b"c"]           # + a length prefix cut in half
    p3 = [b"", b"after-the-truncated-page", b""]
    lay = E.Layout()
    rows, lens, spos, blob, base = [], [], [], b"", 0

    def add(strs, skew, nvals=None, extra=b""):
        nonlocal base, blob
        payload = E.plain_byte_array(strs) + extra
        off = lay.add(payload, skew)
        n = len(strs) if nvals is None else nvals
        rows.append((off, len(payload), n, base, 0, 0))
        pos = 0
        for s in strs[:n]:
            lens.append(len(s))
            spos.append(off + pos + 4)
            pos += 4 + len(s)
            blob += s
        lens.extend([0] * (n - len(strs)))   # slots after the cut stay 0
        spos.extend([0] * (n - len(strs)))
        base += n

    add(p0, 1)
    add([b"unused"], 2, nvals=0)              # zero-n_values page
    add(p2, 3, nvals=5, extra=b"\x09\x00")    # src_len ends inside a prefix
    add(p3, 0)
    return Case("walk", lay.finish(), rows,
                {"lengths": _i64(lens), "src_pos": _i64(spos),
                 "blob": _u8(blob)}, total=base)


# ---------------------------------------------------------------------------
# _decode_dict_codes (host)
# ---------------------------------------------------------------------------

def _b_dict_bw0():
    """Index width 0 (one-entry dictionary, parquet-mr / arrow-rs): an RLE
    run of 5 with no value byte, 0xFF behind it; then a width-3 page that
    only decodes if the stream stayed in sync."""
    lay = E.Layout()
    p0 = b"\x00" + E.varint(5 << 1)
    body, v1 = E.rle_hybrid([("rle", 4, 5), ("packed", [7, 0, 1, 2, 3, 4, 5, 6]),
                             ("rle", 2, 6)], 3)
    p1 = b"\x03" + body
    rows = [(lay.add(p0, 1, gap=8), len(p0), 5, 0, 0, 0),
            (lay.add(p1, 2, gap=8), len(p1), len(v1), 5, 0, 3)]
    return Case("dictcodes", lay.finish(), rows,
                {"codes": _i32_bits([0] * 5 + v1)})


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------

DELTA_WIDTHS = [0, 1, 7, 8, 31, 32, 33, 56, 57, 59, 61, 62, 63, 64]

CASES = (
    [(f"rle_bw{bw}", _b_rle_bw(bw)) for bw in range(33)] + [
        ("rle_bw32_top_bit_set", _b_rle_topbit),
        ("rle_zero_length_run_middle_and_end", _b_rle_zero_len_run),
        ("rle_nvals_clamps_rle_and_packed_runs", _b_rle_clamp),
        ("rle_1100_runs_three_lds_batches", _b_rle_gt_kruns),
        ("rle_padded_varint_header", _b_rle_padded_varint),
        ("rle_empty_page_between_pages", _b_rle_empty_page_between),
        ("rle_8200_pages_grid_stride", _b_rle_8200_pages),
    ] + [
        # widths 59, 61, 62 and 63 put a value across nine bytes
        (f"delta_forced_bw{bw}", _b_delta_bw(bw)) for bw in DELTA_WIDTHS
    ] + [
        ("delta_n1_2_32_33_128_129_130_257_partial_blocks",
         _b_delta_partial_blocks),
        ("delta_int64_min_max_alternating_wrap", _b_delta_extremes),
        ("delta_negative_and_int64_min_min_delta", _b_delta_negative_min_delta),
        ("delta_40000_values_three_lds_batches", _b_delta_40000),
        ("delta_page_skew_0_to_3", _b_delta_skews),
        ("delta_empty_pages_share_out_row_middle", _b_delta_empty_middle),
        ("delta_empty_page_trailing_out_row_eq_total", _b_delta_empty_trailing),
        ("delta_8200_pages_grid_stride", _b_delta_8200_pages),
        ("delta_block_256_miniblock_64", _b_delta_block256),
        ("dlba_lengths_data_end_payload_copy", _b_dlba),
        ("segscan_len_0_1_2047_2048_2049_4097_aux_wrap", _b_segscan_tiles),
        ("plain_copy_w4_skew_x_nvals", _b_plain(4)),
        ("plain_copy_w8_skew_x_nvals", _b_plain(8)),
        ("copy_bytes_src_skew_x_dst_align_x_len", _b_copy_bytes),
    ] + [(f"flba_w{w}_skew_0_to_3", _b_flba(w)) for w in range(1, 9)] + [
        ("bytearray_walk_gather_empty_long_truncated", _b_walk),
        ("dict_codes_bit_width_0_then_3", _b_dict_bw0),
    ])

_BUILDERS = dict(CASES)
NAMES = [n for n, _ in CASES]
assert len(_BUILDERS) == len(CASES)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def _sim_out(name):
    """Simulator output of a case: computed once, shared by both halves."""
    return run_case(_case(name), pq_sim, "cpu")


def _check_expected(got, case, name):
    for key, want in case.expected.items():
        g = got[key].cpu()
        assert g.dtype == want.dtype and g.shape == want.shape, (name, key)
        if not torch.equal(g, want):
            bad = torch.nonzero(g != want).flatten()[:8].tolist()
            raise AssertionError(
                f"{name}/{key}: {len(bad)}+ mismatches, first at {bad}: "
                f"got {g[bad].tolist()} want {want[bad].tolist()}")


@pytest.mark.parametrize("name", NAMES)
def test_sim_case(name):
    """Every case through the numpy simulator, against the values the
    encoder was given.

    Before the empty-page fix (`dst[0] = first` stored unconditionally, in
    the kernel and in pq_sim alike) the simulator fails
    delta_empty_pages_share_out_row_middle with a wrong value in B's first
    slot (an empty page's header value, 12345) and
    delta_empty_page_trailing_out_row_eq_total with IndexError. On the
    device the trailing store lands past a tensor the wrapper allocates
    and cannot be observed from Python; the middle case is the one that
    shows the write. Before the bit-width fix (host clamp of width 0 to 1)
    dict_codes_bit_width_0_then_3 raises IndexError in the simulator."""
    _check_expected(_sim_out(name), _case(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_case(name):
    """The same cases through the HIP kernels: equal to the encoder's
    values, and equal to the simulator on every output."""
    from sail_amd.ops import kernels

    case = _case(name)
    got = run_case(case, kernels.require(), "cuda:0")
    _check_expected(got, case, name)
    sim = _sim_out(name)
    assert set(got) == set(sim)
    for key in sim:
        assert torch.equal(got[key].cpu(), sim[key]), (name, key)


def test_every_pq_entry_point_has_a_case():
    import os
    import re

    src = os.path.join(os.path.dirname(G.__file__), "..", "ops", "csrc",
                       "module.cpp")
    with open(src) as f:
        entry = set(re.findall(r'm\.def\("(pq_\w+)"', f.read()))
    reached = {"rle": {"pq_rle_decode"},
               "delta": {"pq_delta_decode", "pq_segscan"},
               "segscan": {"pq_segscan"},
               "plain": {"pq_plain_copy"},
               "copy": {"pq_copy_bytes"},
               "flba": {"pq_flba_i64"},
               "walk": {"pq_bytearray_walk", "pq_gather_strings"},
               "dlba": {"pq_delta_decode", "pq_copy_bytes", "pq_segscan"},
               "dictcodes": {"pq_rle_decode"}}
    kinds = {_case(n).kind for n in NAMES}
    covered = set().union(*(reached[k] for k in kinds))
    assert entry and entry <= covered, entry - covered


# ---------------------------------------------------------------------------
# the encoder against pyarrow's own pages
# ---------------------------------------------------------------------------

def _file_pages(path, column):
    idx = G.file_index(path)
    chunks = idx.chunks(idx.column_index(column))
    with open(path, "rb") as f:
        raw = f.read()
    return raw, [p for ch in chunks for p in ch.pages]


def _raw_buf(raw):
    return _u8(raw + bytes([E.FILL] * E.TAIL_PAD))


def test_encoder_matches_pyarrow_delta_int64(tmp_path):
    rng = _rng(80)
    vals = rng.integers(-10**14, 10**14, 700).tolist()
    p = str(tmp_path / "x.parquet")
    pq.write_table(pa.table({"k": pa.array(vals, pa.int64())}), p,
                   compression="NONE", use_dictionary=False,
                   column_encoding={"k": "DELTA_BINARY_PACKED"},
                   data_page_version="1.0")
    raw, pages = _file_pages(p, "k")
    assert len(pages) == 1 and pages[0].enc == G.DELTA_BINARY_PACKED
    pg = pages[0]
    theirs = E.page_table([(pg.val_off, pg.val_len, pg.nvals, 0, 0, 0)])
    a, a_end = pq_sim.pq_delta_decode(_raw_buf(raw), theirs, len(vals))
    pq_sim.pq_segscan(a, theirs)

    # pyarrow's block geometry is in its header (128/4 or 256/4 by version)
    theirs_bytes = raw[pg.val_off:pg.val_off + pg.val_len]
    block, pos = pq_sim._read_varint(theirs_bytes, 0)
    mbpb, pos = pq_sim._read_varint(theirs_bytes, pos)
    mine = _delta_case([vals], skews=[1], block=block, mbpb=mbpb)
    b = run_case(mine, pq_sim, "cpu")
    assert torch.equal(a, b["values"])
    assert a.tolist() == vals
    assert int(a_end[0]) == int(b["data_end"][0]) == pg.val_len
    # and the same stream byte for byte: minimal widths, last miniblock
    # padded fully, unused miniblocks of width 0 without data
    assert theirs_bytes == E.delta_binary_packed(vals, None, block, mbpb)[0]
    # the default geometry decodes to the same values
    c = run_case(_delta_case([vals], skews=[2]), pq_sim, "cpu")
    assert torch.equal(a, c["values"])


def test_encoder_matches_pyarrow_dictionary(tmp_path):
    rng = _rng(81)
    words = ["AIR", "FOB", "MAIL", "RAIL", "SHIP", "TRUCK", "REG AIR"]
    vals = [words[i] for i in rng.integers(0, len(words), 900)]
    vals[100:400] = ["MAIL"] * 300             # long RLE run
    p = str(tmp_path / "d.parquet")
    pq.write_table(pa.table({"s": pa.array(vals)}), p, compression="NONE",
                   use_dictionary=["s"], data_page_version="1.0")
    raw, pages = _file_pages(p, "s")
    assert len(pages) == 1 and pages[0].enc == G.RLE_DICTIONARY
    pg = pages[0]
    bw = pg.bw0
    theirs = E.page_table([(pg.val_off + 1, pg.val_len - 1, pg.nvals, 0, 0, bw)])
    a = pq_sim.pq_rle_decode(_raw_buf(raw), theirs, len(vals))

    first_seen = {}
    for v in vals:                              # first-occurrence codes
        first_seen.setdefault(v, len(first_seen))
    codes = [first_seen[v] for v in vals]
    assert bw == (len(first_seen) - 1).bit_length()
    # bit-packed runs hold multiples of 8, so the RLE run starts at 104
    plan = [("packed", codes[:104]), ("rle", 296, codes[104]),
            ("packed", codes[400:])]
    payload, _ = E.rle_hybrid(plan, bw)
    lay = E.Layout()
    off = lay.add(payload, 3)
    b = pq_sim.pq_rle_decode(
        lay.finish(), E.page_table([(off, len(payload), len(vals), 0, 0, bw)]),
        len(vals))
    assert torch.equal(a, b)
    assert a.tolist() == codes


# ---------------------------------------------------------------------------
# whole files through G.read_gpu: pages with no non-null value
# ---------------------------------------------------------------------------

def _null_file(path, kind, null_rows, row_group_size):
    n = 4000
    mask = np.zeros(n, dtype=bool)
    mask[null_rows] = True
    if kind == "str":
        arr = pa.array([f"v{i}" for i in range(n)], pa.string(), mask=mask)
        enc = "DELTA_LENGTH_BYTE_ARRAY"
    else:
        # random, so the delta stream is wide enough to split into pages
        arr = pa.array(_rng(90).integers(-10**14, 10**14, n), pa.int64(),
                       mask=mask)
        enc = "DELTA_BINARY_PACKED"
    tbl = pa.table({"c": arr})
    pq.write_table(tbl, path, column_encoding={"c": enc},
                   use_dictionary=False, data_page_size=512,
                   data_page_version="1.0", compression="NONE",
                   row_group_size=row_group_size)
    return tbl


def _empty_page_count(path):
    """Pages whose non-null count is 0, from the page index and the
    definition levels the writer stored."""
    raw, pages = _file_pages(path, "c")
    empty = 0
    for pg in pages:
        if pg.all_valid:
            continue
        lv = pq_sim.pq_rle_decode(
            _raw_buf(raw),
            E.page_table([(pg.def_off, pg.def_len, pg.nvals, 0, 0, 1)]),
            pg.nvals)
        empty += int(lv.sum().item()) == 0
    return empty


# name -> (null rows, row group size). pyarrow cuts a page only after a batch
# that added value bytes, so within one row group a null run ends up in the
# page of the values before it; the row-group variant is the one that puts
# pages without values in the middle of the page table (row groups of 1000
# rows: the second and third hold nulls only).
NULL_FILES = {"trailing": (slice(2000, 4000), None),
              "middle": (slice(1000, 3000), None),
              "middle_row_groups": (slice(1000, 3000), 1000),
              "all": (slice(0, 4000), None),
              "all_row_groups": (slice(0, 4000), 1000)}


def _null_file_roundtrip(tmp_path, kind, where, device):
    p = str(tmp_path / f"{kind}_{where}.parquet")
    tbl = _null_file(p, kind, *NULL_FILES[where])
    if _empty_page_count(p) == 0:
        pytest.skip("this pyarrow build wrote no page without non-null "
                    "values; the file does not reach the empty-page path")
    out = G.read_gpu([p], [("c", None)], device)
    assert out.columns["c"].to_pylist() == tbl.column("c").to_pylist()


def test_segmented_cumsum_pages_without_values():
    """Host scan over nullable DELTA_LENGTH pages: zero counts in the
    middle, at the end, and (the case that used to raise IndexError from
    the base gather) no values in any of several pages."""
    d = torch.tensor([5, 1, 1, 7, 2], dtype=torch.int64)
    got = G._segmented_cumsum(d, [3, 0, 2, 0])
    assert got.tolist() == [5, 6, 7, 7, 9]
    empty = torch.zeros(0, dtype=torch.int64)
    assert G._segmented_cumsum(empty, [0, 0, 0]).tolist() == []


@pytest.fixture()
def sim(monkeypatch):
    monkeypatch.setattr(G, "_ext", lambda: pq_sim)
    monkeypatch.setattr(G, "_ALLOW_CPU", True)
    yield


@pytest.mark.parametrize("where", list(NULL_FILES))
@pytest.mark.parametrize("kind", ["str", "int"])
def test_sim_file_with_empty_pages(tmp_path, sim, kind, where):
    """DELTA_LENGTH_BYTE_ARRAY strings / DELTA_BINARY_PACKED int64 whose
    null runs leave whole pages without a value. Before the empty-page fix
    the simulator raises IndexError on these files."""
    _null_file_roundtrip(tmp_path, kind, where, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("where", list(NULL_FILES))
@pytest.mark.parametrize("kind", ["str", "int"])
def test_gpu_file_with_empty_pages(tmp_path, kind, where):
    _null_file_roundtrip(tmp_path, kind, where, "cuda:0")


def _bit_width_0_file_roundtrip(tmp_path, device):
    """A one-entry dictionary column as parquet-mr / arrow-rs write it:
    pyarrow's page body [0x01][varint(n<<1)][0x00] (width 1, one RLE run of
    code 0) is patched in place, at equal length, to
    [0x00][varint(n<<1) padded by one continuation byte] (width 0, the run
    carries no value byte)."""
    n = 50
    vals = ["only"] * n
    src = str(tmp_path / "w1.parquet")
    pq.write_table(pa.table({"s": pa.array(vals)}), src, compression="NONE",
                   use_dictionary=["s"], data_page_version="1.0")
    raw, pages = _file_pages(src, "s")
    pg = pages[0] if len(pages) == 1 else None
    want = bytes([0x01]) + E.varint(n << 1) + bytes([0x00])
    if pg is None or raw[pg.val_off:pg.val_off + pg.val_len] != want:
        pytest.skip("this pyarrow build lays the one-entry dictionary page "
                    "out differently; nothing to patch")
    patched = bytearray(raw)
    patched[pg.val_off:pg.val_off + pg.val_len] = \
        bytes([0x00]) + E.varint(n << 1, pad=1)
    assert len(patched) == len(raw)
    dst = str(tmp_path / "w0.parquet")
    with open(dst, "wb") as f:
        f.write(patched)
    out = G.read_gpu([dst], [("s", None)], device)
    assert out.columns["s"].to_pylist() == vals


def test_sim_file_dictionary_bit_width_0(tmp_path, sim):
    _bit_width_0_file_roundtrip(tmp_path, "cpu")


@pytest.mark.gpu
def test_gpu_file_dictionary_bit_width_0(tmp_path):
    _bit_width_0_file_roundtrip(tmp_path, "cuda:0")
