"""CPU twins of pq_bytearray_index and pq_gather_bytes
(ops/csrc/parquet_bytearray.hip), written from the parquet format and the
entry points' contract, not from the kernels.

PLAIN BYTE_ARRAY is `<u32 little-endian length><bytes>` per value. The page
table is int64 [n,6] = {src_off, src_len, n_values, out_row, aux, bw}.

pq_bytearray_index(buf, pages, total) -> [lengths, src_pos, status]
    Row out_row + v of `lengths` / `src_pos` describes value v of a page:
    its length and the offset of its first byte in `buf`. status[p] is 0
    for a well-formed page, else
      1  a length ends past src_off + src_len,
      2  the page ends inside a length prefix or before n_values values,
      3  the descriptor does not fit `buf` or the outputs (nothing written);
    the rows of a rejected page that were not resolved before the break hold
    length 0 and src_pos = src_off. Rows that no page owns are 0. A page
    with n_values == 0 writes nothing.

pq_gather_bytes(buf, src_pos, lengths, out_offsets, total_bytes) -> uint8
    out[out_offsets[i] : + lengths[i]] = buf[src_pos[i] : + lengths[i]].
    Sources may repeat and overlap; a length of 0 copies nothing; a source
    byte outside `buf` reads as 0 and nothing is written outside `out`.
    Bytes of `out` that no value covers are unspecified (0 here).

SIM adds the two entry points to pq_delta_sim.SIM, which stands in for the
whole extension in datasource/gpu_parquet.py."""
from __future__ import annotations

import numpy as np
import torch

import pq_delta_sim


def pq_bytearray_index(buf_t, pages_t, total):
    if buf_t.dtype != torch.uint8 or not buf_t.is_contiguous():
        raise RuntimeError("buf must be contiguous uint8")
    if (pages_t.dtype != torch.int64 or pages_t.dim() != 2
            or pages_t.size(1) != 6 or not pages_t.is_contiguous()):
        raise RuntimeError("pages must be contiguous int64 [n,6]")
    if total < 0:
        raise RuntimeError("total must not be negative")
    raw = buf_t.cpu().numpy().tobytes()
    rows = pages_t.cpu().numpy().reshape(-1, 6).tolist()
    lengths = np.zeros(total, dtype=np.int64)
    src_pos = np.zeros(total, dtype=np.int64)
    status = np.zeros(len(rows), dtype=np.int32)
    for p, (src_off, src_len, n, out_row, _aux, _bw) in enumerate(rows):
        if (out_row < 0 or n < 0 or out_row + n > total or src_off < 0
                or src_len < 0 or src_off + src_len > len(raw)):
            status[p] = 3
            continue
        end = src_off + src_len
        at = src_off
        for v in range(n):
            if at + 4 > end:
                status[p] = 2
            else:
                ln = int.from_bytes(raw[at:at + 4], "little")
                if at + 4 + ln > end:
                    status[p] = 1
            if status[p]:
                lengths[out_row + v:out_row + n] = 0
                src_pos[out_row + v:out_row + n] = src_off
                break
            lengths[out_row + v] = ln
            src_pos[out_row + v] = at + 4
            at += 4 + ln
    return [torch.from_numpy(lengths), torch.from_numpy(src_pos),
            torch.from_numpy(status)]


def pq_gather_bytes(buf_t, src_pos_t, lengths_t, out_offsets_t, total_bytes):
    if buf_t.dtype != torch.uint8 or not buf_t.is_contiguous():
        raise RuntimeError("buf must be contiguous uint8")
    n = src_pos_t.numel()
    for t in (src_pos_t, lengths_t, out_offsets_t):
        if (t.dtype != torch.int64 or t.dim() != 1 or t.numel() != n
                or not t.is_contiguous()):
            raise RuntimeError("src_pos, lengths and out_offsets must be "
                               "contiguous int64 of one length")
    if total_bytes < 0:
        raise RuntimeError("total_bytes must not be negative")
    buf = buf_t.cpu().numpy()
    out = np.zeros(total_bytes, dtype=np.uint8)
    for sp, ln, oo in zip(src_pos_t.tolist(), lengths_t.tolist(),
                          out_offsets_t.tolist()):
        if ln <= 0:
            continue
        if 0 <= sp and sp + ln <= len(buf) and 0 <= oo and \
                oo + ln <= total_bytes:
            out[oo:oo + ln] = buf[sp:sp + ln]
            continue
        for k in range(ln):                    # the clipped, slow way
            if 0 <= oo + k < total_bytes:
                out[oo + k] = buf[sp + k] if 0 <= sp + k < len(buf) else 0
    return torch.from_numpy(out)


class ByteArraySimExt(pq_delta_sim.DeltaSimExt):
    """pq_delta_sim.SIM (which extends pq_types_sim.SIM) plus the two entry
    points of parquet_bytearray.hip."""

    pq_bytearray_index = staticmethod(pq_bytearray_index)
    pq_gather_bytes = staticmethod(pq_gather_bytes)


SIM = ByteArraySimExt()
