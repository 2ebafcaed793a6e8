"""Test-side Snappy element emitter, reference decoder and simulator object.

The emitter writes raw Snappy streams (the per-page format parquet stores)
from explicit element plans, so every tag form can be reached on purpose,
malformed ones included. The decoder mirrors the (out, status) contract of
ops/csrc/snappy.hip in plain Python. Nothing here imports the code under
test: the expectation of every case in tests/test_snappy_kernel.py is the
bytes the builder chose."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

import pq_sim

# status codes of pq_snappy_decompress (ops/csrc/snappy.hip header)
OK = 0
PREAMBLE = 1
TRUNCATED = 2
OVERRUN = 3
BAD_OFFSET = 4
TRAILING = 5


def varint(v: int) -> bytes:
    assert v >= 0
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def literal_header(n: int, form: Optional[int] = None) -> bytes:
    """Tag (+ length bytes) of an n-byte literal. form 0 is the in-tag
    length (n <= 60); forms 1..4 put n-1 into that many length bytes
    (tags 60..63). Default: the shortest form that holds n."""
    assert n >= 1
    m = n - 1
    if form is None:
        form = 0 if m < 60 else (m.bit_length() + 7) // 8
    if form == 0:
        assert m < 60
        return bytes([m << 2])
    assert 1 <= form <= 4 and m < (1 << (8 * form))
    return bytes([(59 + form) << 2]) + m.to_bytes(form, "little")


def copy1(length: int, offset: int) -> bytes:
    assert 4 <= length <= 11 and 0 <= offset < 2048
    return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5),
                  offset & 0xFF])


def copy2(length: int, offset: int) -> bytes:
    assert 1 <= length <= 64 and 0 <= offset < (1 << 16)
    return bytes([2 | ((length - 1) << 2)]) + offset.to_bytes(2, "little")


def copy4(length: int, offset: int) -> bytes:
    assert 1 <= length <= 64 and 0 <= offset < (1 << 32)
    return bytes([3 | ((length - 1) << 2)]) + offset.to_bytes(4, "little")


class Stream:
    """Builds one Snappy stream and, alongside, the bytes it decodes to.

    The preamble is written by finish(); `preamble` overrides its value
    (malformed cases). Offsets are validated against the bytes produced so
    far unless `check=False`."""

    def __init__(self):
        self.body = bytearray()
        self.out = bytearray()

    def lit(self, data: bytes, form: Optional[int] = None) -> "Stream":
        self.body += literal_header(len(data), form) + data
        self.out += data
        return self

    def _expand(self, length: int, offset: int):
        for _ in range(length):
            self.out.append(self.out[-offset])

    def copy(self, kind: int, length: int, offset: int) -> "Stream":
        assert 1 <= offset <= len(self.out), (offset, len(self.out))
        self.body += {1: copy1, 2: copy2, 4: copy4}[kind](length, offset)
        self._expand(length, offset)
        return self

    def raw(self, data: bytes) -> "Stream":
        """Append bytes to the stream without touching the expectation."""
        self.body += data
        return self

    def finish(self, preamble: Optional[int] = None) -> bytes:
        n = len(self.out) if preamble is None else preamble
        return varint(n) + bytes(self.body)


def decompress(src: bytes, ulen: int):
    """Reference decoder with the kernel's contract: (out, status). `out`
    has ulen bytes; on a non-zero status its contents are unspecified."""
    out = bytearray(ulen)
    n = len(src)
    pos = 0
    v = 0
    shift = 0
    closed = False
    while pos < n and shift <= 28:
        b = src[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if not (b & 0x80):
            closed = True
            break
        shift += 7
    if not closed:
        return bytes(out), (TRUNCATED if pos >= n and shift <= 28
                            else PREAMBLE)
    if v != ulen:
        return bytes(out), PREAMBLE
    prod = 0
    while pos < n:
        if prod == ulen:
            return bytes(out), TRAILING
        tag = src[pos]
        pos += 1
        kind = tag & 3
        if kind == 0:
            m = tag >> 2
            if m >= 60:
                nb = m - 59
                if n - pos < nb:
                    return bytes(out), TRUNCATED
                m = int.from_bytes(src[pos:pos + nb], "little")
                pos += nb
            ln = m + 1
            if ln > ulen - prod:
                return bytes(out), OVERRUN
            if ln > n - pos:
                return bytes(out), TRUNCATED
            out[prod:prod + ln] = src[pos:pos + ln]
            pos += ln
            prod += ln
            continue
        nb = {1: 1, 2: 2, 3: 4}[kind]
        if n - pos < nb:
            return bytes(out), TRUNCATED
        if kind == 1:
            ln = 4 + ((tag >> 2) & 7)
            off = ((tag >> 5) << 8) | src[pos]
        else:
            ln = 1 + (tag >> 2)
            off = int.from_bytes(src[pos:pos + nb], "little")
        pos += nb
        if off == 0 or off > prod:
            return bytes(out), BAD_OFFSET
        if ln > ulen - prod:
            return bytes(out), OVERRUN
        if off >= ln:
            out[prod:prod + ln] = out[prod - off:prod - off + ln]
        else:
            for i in range(ln):
                out[prod + i] = out[prod - off + i % off]
        prod += ln
    if prod != ulen:
        return bytes(out), TRUNCATED
    return bytes(out), OK


def pq_snappy_decompress(buf_t, pages_t, out_t):
    """Simulator twin of the HIP entry point: decompresses each page of the
    table into `out_t` in place, returns the int32 status tensor."""
    buf = buf_t.cpu().numpy()
    out = out_t.numpy()
    pages = pages_t.cpu().numpy().reshape(-1, 6)
    status = np.zeros(len(pages), dtype=np.int32)
    for p, (src_off, src_len, ulen, out_off, _a, _b) in enumerate(pages):
        assert 0 <= src_off and src_off + src_len <= buf.size
        assert 0 <= out_off and out_off + ulen <= out.size
        data, st = decompress(bytes(buf[src_off:src_off + src_len]), int(ulen))
        status[p] = st
        if st == OK:
            out[out_off:out_off + ulen] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(status)


class SimExt:
    """The numpy kernel simulator (tests/pq_sim.py) plus
    pq_snappy_decompress: stands in for the HIP extension in the host
    orchestration of datasource/gpu_parquet.py."""

    pq_snappy_decompress = staticmethod(pq_snappy_decompress)

    def __getattr__(self, name):
        return getattr(pq_sim, name)


SIM = SimExt()
