"""Test side of ops/csrc/parquet_types.hip: small page encoders, numpy
twins of the three entry points, and a simulator object.

Encoders (bit-packed booleans, INT96 triples, byte-stream transposition)
take the values a test chose; the expectation of every case in
tests/test_pq_types_kernels.py is those values. The twins implement the
kernel contracts (page table int64 [n,6] = {src_off, src_len, n_values,
out_row, 0, 0}; a page with n_values == 0 writes nothing) in plain
Python/numpy and import nothing from the code under test. SIM layers them
over snappy_encode.SIM, so it stands in for the whole HIP extension in
datasource/gpu_parquet.py."""
from __future__ import annotations

from typing import Iterable, Sequence

import numpy as np
import torch

import snappy_encode

JULIAN_UNIX_EPOCH = 2440588
MICROS_PER_DAY = 86_400_000_000


# -- encoders ----------------------------------------------------------------

def bool_bits(values: Sequence[int], pad_ones: bool = False) -> bytes:
    """PLAIN BOOLEAN: value i is bit i & 7 of byte i >> 3. The unused bits
    of the last byte are 0, or 1 with `pad_ones`."""
    vals = [int(bool(v)) for v in values]
    pad = -len(vals) % 8
    bits = np.array(vals + [int(pad_ones)] * pad, dtype=np.uint8)
    return np.packbits(bits, bitorder="little").tobytes()


def int96(nanos: int, julian_day: int) -> bytes:
    """One INT96 timestamp: nanoseconds of day (LE int64), Julian day (LE
    int32)."""
    return (int(nanos).to_bytes(8, "little", signed=True)
            + int(julian_day).to_bytes(4, "little", signed=True))


def int96_page(values: Iterable[tuple]) -> bytes:
    return b"".join(int96(n, d) for n, d in values)


def byte_stream_split(plain: bytes, width: int) -> bytes:
    """BYTE_STREAM_SPLIT of PLAIN little-endian values: all byte 0s, then
    all byte 1s, ..."""
    assert len(plain) % width == 0
    a = np.frombuffer(plain, dtype=np.uint8).reshape(-1, width)
    return np.ascontiguousarray(a.T).tobytes()


def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def int96_micros(nanos: int, julian_day: int) -> int:
    """Expectation in Python integers: truncating division, int64 wrap."""
    q = abs(nanos) // 1000
    if nanos < 0:
        q = -q
    return _wrap64((julian_day - JULIAN_UNIX_EPOCH) * MICROS_PER_DAY + q)


# -- numpy twins of the entry points ------------------------------------------

def _rows(pages_t):
    return pages_t.cpu().numpy().reshape(-1, 6)


def pq_bool_unpack(buf_t, pages_t, total):
    buf = buf_t.cpu().numpy()
    out = np.zeros(total, dtype=np.uint8)
    for src_off, _len, n, out_row, _a, _b in _rows(pages_t):
        if n == 0:
            continue
        src = buf[src_off:src_off + (n + 7) // 8]
        out[out_row:out_row + n] = np.unpackbits(src, bitorder="little")[:n]
    return torch.from_numpy(out)


def pq_int96_micros(buf_t, pages_t, total):
    buf = buf_t.cpu().numpy()
    out = np.zeros(total, dtype=np.int64)
    for src_off, _len, n, out_row, _a, _b in _rows(pages_t):
        for i in range(n):
            raw = bytes(buf[src_off + 12 * i:src_off + 12 * i + 12])
            out[out_row + i] = int96_micros(
                int.from_bytes(raw[:8], "little", signed=True),
                int.from_bytes(raw[8:], "little", signed=True))
    return torch.from_numpy(out)


def pq_bss_decode(buf_t, pages_t, total, width):
    if width not in (4, 8):
        raise RuntimeError(f"byte_stream_split width must be 4 or 8, got {width}")
    buf = buf_t.cpu().numpy()
    out = np.zeros(total * width, dtype=np.uint8)
    for src_off, _len, n, out_row, _a, _b in _rows(pages_t):
        if n == 0:
            continue
        streams = buf[src_off:src_off + width * n].reshape(width, n)
        out[out_row * width:(out_row + n) * width] = streams.T.reshape(-1)
    return torch.from_numpy(out)


class TypesSimExt(snappy_encode.SimExt):
    """snappy_encode.SIM (tests/pq_sim.py + pq_snappy_decompress) plus the
    three entry points of parquet_types.hip."""

    pq_bool_unpack = staticmethod(pq_bool_unpack)
    pq_int96_micros = staticmethod(pq_int96_micros)
    pq_bss_decode = staticmethod(pq_bss_decode)


SIM = TypesSimExt()
