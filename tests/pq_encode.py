"""Test-side parquet page encoders (pure Python/numpy).

Produces page payloads and page-descriptor tables for the kernel contract
of ops/csrc/parquet_decode.hip, int64 [n,6] =
{src_off, src_len, n_values, out_row, aux, bw}, from values the test chose.
Nothing here imports the code under test: the expectation of every case in
tests/test_pq_kernels.py is the values handed to these encoders, never the
output of the simulator (tests/pq_sim.py) or of a kernel.

Unlike a real parquet writer these encoders take explicit plans (run
layout, forced bit widths, padded varints), so the corners of the format
that pyarrow never emits can be reached on purpose."""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

MASK64 = (1 << 64) - 1
INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1

FILL = 0xFF       # gap / filler byte: never zero, so stray reads show
TAIL_PAD = 16     # the staging upload is total + 16 bytes


# -- primitives --------------------------------------------------------------

def wrap64(v: int) -> int:
    """Two's-complement wrap of a Python int to int64."""
    v &= MASK64
    return v - (1 << 64) if v >> 63 else v


def varint(v: int, pad: int = 0) -> bytes:
    """ULEB128. `pad` appends that many redundant continuation bytes
    (non-canonical but legal: 0x85 0x00 still decodes to 5)."""
    assert v >= 0
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            break
    for _ in range(pad):
        out[-1] |= 0x80
        out.append(0x00)
    return bytes(out)


def zigzag64(v: int) -> int:
    """Signed int64 -> unsigned zigzag (INT64_MIN -> 2**64 - 1)."""
    assert INT64_MIN <= v <= INT64_MAX
    return ((v << 1) ^ (v >> 63)) & MASK64


def pack_bits(values: Sequence[int], bw: int) -> bytes:
    """Little-endian bit packing of unsigned `values` at `bw` bits each;
    the result is padded with zero bits to a whole byte."""
    if bw == 0 or len(values) == 0:
        return b""
    assert all(0 <= int(v) < (1 << bw) for v in values)
    arr = np.array([int(v) for v in values], dtype=np.uint64)
    shifts = np.arange(bw, dtype=np.uint64)
    bits = ((arr[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.reshape(-1), bitorder="little").tobytes()


# -- RLE / bit-packed hybrid -------------------------------------------------

def rle_hybrid(plan, bw: int, pad_varint: int = 0) -> Tuple[bytes, List[int]]:
    """Encode an explicit run plan.

    plan entries: ("rle", count, value) or ("packed", [values...]).
    A bit-packed entry is padded to a multiple of 8 values with the all-ones
    value of the width (non-zero where the width allows, so a decoder that
    runs into padding is noticed). Returns (payload, values the stream
    encodes, padding included). A count of 0 is allowed for an RLE run."""
    assert 0 <= bw <= 32
    top = (1 << bw) - 1
    nbytes = (bw + 7) // 8
    out = bytearray()
    decoded: List[int] = []
    for entry in plan:
        if entry[0] == "rle":
            _, count, value = entry
            assert 0 <= value <= top and count >= 0
            out += varint(count << 1, pad_varint)
            out += int(value).to_bytes(nbytes, "little")
            decoded += [int(value)] * count
        elif entry[0] == "packed":
            vals = [int(v) for v in entry[1]]
            vals += [top] * (-len(vals) % 8)
            assert vals, "empty bit-packed entry"
            out += varint(((len(vals) // 8) << 1) | 1, pad_varint)
            out += pack_bits(vals, bw)
            decoded += vals
        else:
            raise ValueError(entry[0])
    return bytes(out), decoded


# -- DELTA_BINARY_PACKED -----------------------------------------------------

BLOCK = 128
MINIBLOCKS = 4


def delta_header(total: int, first: int, block: int = BLOCK,
                 mbpb: int = MINIBLOCKS) -> bytes:
    return (varint(block) + varint(mbpb) + varint(total)
            + varint(zigzag64(first)))


def delta_binary_packed(values: Iterable[int],
                        forced_bw: Optional[int] = None,
                        block: int = BLOCK, mbpb: int = MINIBLOCKS
                        ) -> Tuple[bytes, List[int]]:
    """DELTA_BINARY_PACKED in wrapping 64-bit arithmetic; block size 128
    with 4 miniblocks unless told otherwise (pyarrow writes other sizes).
    Each miniblock gets its minimal width, or `forced_bw` (which must be
    at least the minimal one). The last miniblock is padded
    fully; unused trailing miniblocks get width 0 and no data. Returns
    (payload, widths of the miniblocks that hold values)."""
    vals = [int(v) for v in values]
    assert all(INT64_MIN <= v <= INT64_MAX for v in vals)
    n = len(vals)
    assert block % mbpb == 0 and (block // mbpb) % 8 == 0
    out = bytearray(delta_header(n, vals[0] if n else 0, block, mbpb))
    deltas = [wrap64(vals[i + 1] - vals[i]) for i in range(n - 1)]
    vpm = block // mbpb
    used: List[int] = []
    for b in range(0, len(deltas), block):
        blk = deltas[b:b + block]
        min_delta = min(blk)
        out += varint(zigzag64(min_delta))
        adj = [d - min_delta for d in blk]        # in [0, 2**64)
        mbs = [adj[k * vpm:(k + 1) * vpm] for k in range(mbpb)]
        widths = []
        for mb in mbs:
            if not mb:
                widths.append(0)
                continue
            need = max(x.bit_length() for x in mb)
            w = need if forced_bw is None else forced_bw
            assert need <= w <= 64, (need, w)
            widths.append(w)
            used.append(w)
        out += bytes(widths)
        for mb, w in zip(mbs, widths):
            if mb:
                out += pack_bits(mb + [0] * (vpm - len(mb)), w)
    return bytes(out), used


# -- raw fixed-width / byte arrays -------------------------------------------

def plain_fixed(values: np.ndarray) -> bytes:
    """PLAIN fixed width: little-endian values back to back."""
    a = np.ascontiguousarray(values)
    return a.astype(a.dtype.newbyteorder("<")).tobytes()


def flba_be(values: Iterable[int], width: int) -> bytes:
    """FIXED_LEN_BYTE_ARRAY: big-endian two's complement, `width` bytes."""
    assert 1 <= width <= 8
    return b"".join(int(v).to_bytes(width, "big", signed=True) for v in values)


def plain_byte_array(strings: Iterable[bytes]) -> bytes:
    """PLAIN byte_array: <u32 little-endian length><bytes> per value."""
    return b"".join(len(s).to_bytes(4, "little") + s for s in strings)


def delta_length_byte_array(strings: Sequence[bytes]) -> Tuple[bytes, int]:
    """DELTA_LENGTH_BYTE_ARRAY: delta stream of the lengths, then the
    concatenated payload. Returns (page, length of the delta stream)."""
    head, _ = delta_binary_packed([len(s) for s in strings])
    return head + b"".join(strings), len(head)


# -- layout ------------------------------------------------------------------

class Layout:
    """Concatenates page payloads into one source buffer.

    Every page starts at an offset with the requested `offset % 4` (skew
    0-3), so all four source alignments of the dword-copy kernels occur;
    gaps are filled with 0xFF and the buffer ends with 16 pad bytes of 0xFF
    (the real staging buffer uploads total + 16 bytes)."""

    def __init__(self, lead: int = 4):
        self._buf = bytearray([FILL] * lead)

    def add(self, payload: bytes, skew: int = 0, gap: int = 1) -> int:
        """Append a page after at least `gap` filler bytes; returns its
        offset, which is congruent to `skew` mod 4."""
        assert 0 <= skew <= 3
        self._buf += bytes([FILL] * gap)
        while len(self._buf) % 4 != skew:
            self._buf.append(FILL)
        off = len(self._buf)
        self._buf += payload
        return off

    def finish(self) -> torch.Tensor:
        data = bytes(self._buf) + bytes([FILL] * TAIL_PAD)
        return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())


def page_table(rows) -> torch.Tensor:
    """rows of (src_off, src_len, n_values, out_row, aux, bw) -> int64 [n,6]."""
    arr = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    return torch.from_numpy(arr)
