"""Column-chunk bytes of a parquet file -> one device buffer, for the GPU
parquet scan (gpu_parquet.py).

The chunk bytes of a column reach the device through the extension's
pipelined reader (ops/csrc/scan_reader.h, scan_reader.hip, pq_read_ranges):
a persistent pool of workers preads 16 MiB slices into a ring of 8 pinned
slots and each slice is copied on the copy stream as soon as it is complete,
so the file read and the copy of one column overlap and the pinned footprint
stays at the ring. SAIL_IO_NATIVE_READER=off, and every CPU run, takes the
Python reader instead: a thread pool fills one column-sized pinned buffer,
then one copy.
"""
from __future__ import annotations

import os
from typing import List, Tuple

import torch

from .pq_index import native_reader_enabled


class _StagingPool:
    """Two pinned host buffers in rotation. The async H2D copy out of a
    buffer must complete before the NEXT column's file read overwrites it;
    the recorded event enforces that while still letting the CPU read
    column i+1 during column i's device decode."""

    def __init__(self):
        self.bufs = [None, None]
        self.events = [None, None]
        self.i = 0

    def acquire(self, nbytes: int):
        i = self.i
        self.i ^= 1
        ev = self.events[i]
        if ev is not None:
            ev.synchronize()
            self.events[i] = None
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            cap = max(nbytes, 64 << 20)
            pin = torch.cuda.is_available()
            self.bufs[i] = torch.empty(cap, dtype=torch.uint8, pin_memory=pin)
        return i, self.bufs[i]

    def mark_uploaded(self, i: int):
        if torch.cuda.is_available():
            ev = torch.cuda.Event()
            ev.record()
            self.events[i] = ev


_STAGING = _StagingPool()
_COPY_STREAM = None


def _copy_stream(device):
    global _COPY_STREAM
    if _COPY_STREAM is None:
        _COPY_STREAM = torch.cuda.Stream(device=device)
    return _COPY_STREAM


def _coalesce(ranges: List[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """Neighbours in the list that are neighbours in the file as one range,
    empty ranges dropped: the same bytes in fewer reads."""
    out: List[Tuple[int, int]] = []
    for s, e in ranges:
        if e == s:
            continue
        if out and out[-1][1] == s:
            out[-1] = (out[-1][0], e)
        else:
            out.append((s, e))
    return out


def _native_reader(device):
    """The extension, when uploads to `device` go through its pipelined
    reader: a GPU device, the switch on, the extension loaded and holding
    the entry point. None selects the Python reader below."""
    if not (native_reader_enabled() and str(device).startswith("cuda")
            and torch.cuda.is_available()):
        return None
    from ..ops import kernels

    ext = kernels._load()
    return ext if hasattr(ext, "pq_read_ranges") else None


def _upload_ranges(path: str, ranges: List[Tuple[int, int]], device):
    """File byte ranges -> one device u8 tensor of their concatenation plus
    16 zero bytes; returns (tensor, [offset per range]). On a GPU the
    extension's reader streams the bytes through a ring of pinned slices
    (pq_read_ranges: reads and copies overlap within the column). Otherwise:
    read into pinned staging, one H2D copy."""
    offs, total = [], 0
    for s, e in ranges:
        offs.append(total)
        total += e - s
    ext = _native_reader(device)
    if ext is not None:
        # allocated under the copy stream and handed to the compute stream,
        # as the staged copy below: a block the allocator recycles is never
        # written while an earlier kernel still reads it
        cs = _copy_stream(device)
        cur = torch.cuda.current_stream()
        with torch.cuda.stream(cs):
            dev = torch.empty(total + 16, dtype=torch.uint8, device=device)
            ext.pq_read_ranges(os.path.abspath(path), _coalesce(ranges), dev,
                               cs.cuda_stream)
        cur.wait_stream(cs)
        dev.record_stream(cur)
        return dev, offs
    slot, stage = _STAGING.acquire(total + 16)  # +16: aligned-word kernels
    view = stage.numpy()                        # may read past the last page
    jobs = [(s, e, at) for (s, e), at in zip(ranges, offs)]
    # parallel pread into pinned staging: readinto releases the GIL, so
    # page-cache-warm scans move at memory bandwidth instead of one core
    from concurrent.futures import ThreadPoolExecutor

    def _one(job):
        s, e, at = job
        with open(path, "rb") as f:
            f.seek(s)
            got = f.readinto(memoryview(view)[at:at + (e - s)])
        if got != e - s:
            raise IOError(f"short read in {path}")

    nthreads = int(os.environ.get("SAIL_IO_READ_THREADS", "8"))
    if len(jobs) > 1 and total > (64 << 20) and nthreads > 1:
        with ThreadPoolExecutor(max_workers=min(nthreads, len(jobs))) as pool:
            list(pool.map(_one, jobs))
    else:
        for j in jobs:
            _one(j)
    view[total:total + 16] = 0
    if torch.cuda.is_available() and str(device).startswith("cuda"):
        # H2D on a dedicated copy stream so the NEXT column's upload
        # overlaps the CURRENT column's decode kernels; the compute stream
        # waits on the copy event before its kernels touch the buffer
        cs = _copy_stream(device)
        cur = torch.cuda.current_stream()
        with torch.cuda.stream(cs):
            dev = stage[:total + 16].to(device, non_blocking=True)
        cur.wait_stream(cs)
        dev.record_stream(cur)
    else:
        dev = stage[:total + 16].to(device, non_blocking=True)
    _STAGING.mark_uploaded(slot)
    return dev, offs
