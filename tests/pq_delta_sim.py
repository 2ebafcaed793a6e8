"""CPU twin of pq_delta_values (ops/csrc/parquet_delta.hip).

The fused kernel must give, bit for bit, what the two older entry points and
the caller's cast gave: pq_delta_decode, pq_segscan, then .to(int32) for an
INT32 column. This twin is exactly that composition over the numpy
simulator (tests/pq_sim.py), so tests/test_pq_delta_fused.py can check its
case table, and the host orchestration that calls the new entry, without a
GPU. SIM stands in for the whole extension, new entry included."""
from __future__ import annotations

import torch

import pq_sim
import pq_types_sim


def pq_delta_values(buf_t, pages_t, total, as_int32):
    if buf_t.dtype != torch.uint8 or not buf_t.is_contiguous():
        raise RuntimeError("buf must be contiguous uint8")
    if (pages_t.dtype != torch.int64 or pages_t.dim() != 2
            or pages_t.size(1) != 6 or not pages_t.is_contiguous()):
        raise RuntimeError("pages must be contiguous int64 [n,6]")
    if total < 0:
        raise RuntimeError("total must not be negative")
    vals, _ = pq_sim.pq_delta_decode(buf_t, pages_t, total)
    pq_sim.pq_segscan(vals, pages_t)
    return vals.to(torch.int32) if as_int32 else vals


class DeltaSimExt(pq_types_sim.TypesSimExt):
    """pq_types_sim.SIM plus pq_delta_values."""

    pq_delta_values = staticmethod(pq_delta_values)


SIM = DeltaSimExt()
