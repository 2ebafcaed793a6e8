"""Write one parquet file from many threads.

pyarrow's ParquetWriter encodes a file on a single core, which makes
persisting the SF100 benchmark shards (25 GB) take longer than everything
else the benchmark does. Row groups are independent, though: here worker
threads encode runs of row groups into in-memory parquet files (pyarrow
releases the GIL while it encodes), the calling thread assigns every part
its place in the output in order, copier threads put the row-group bytes
there, and one merged footer is written whose offsets are shifted to where
the bytes landed. The result is byte-for-byte the file a single
ParquetWriter fed the same row groups would have written.
"""
from __future__ import annotations

import functools
import os
from collections import deque
from concurrent.futures import Future, ThreadPoolExecutor
from typing import Callable, Iterable, List, Tuple

from ..utils import thrift_compact as tc

MAGIC = b"PAR1"

# parquet.thrift field ids
_FMD_NUM_ROWS, _FMD_ROW_GROUPS = 3, 4
_RG_COLUMNS, _RG_FILE_OFFSET, _RG_ORDINAL = 1, 5, 7
_CC_FILE_OFFSET, _CC_META = 2, 3
_CC_PAGE_INDEX_FIELDS = (4, 5, 6, 7)   # offset/column index locations
_CMD_OFFSETS = (9, 10, 11)             # data / index / dictionary page offset
_CMD_BLOOM = (14, 15)


def default_threads() -> int:
    n = int(os.environ.get("SAIL_IO_WRITE_THREADS", "0"))
    return n if n > 0 else max(1, min(16, os.cpu_count() or 1))


def _field(tree, fid):
    for f in tree:
        if f[0] == fid:
            return f
    return None


def _split(part) -> Tuple[memoryview, list]:
    """(row-group bytes, footer tree) of one complete in-memory parquet file."""
    mv = memoryview(part).cast("B")
    if bytes(mv[:4]) != MAGIC or bytes(mv[-4:]) != MAGIC:
        raise ValueError("not a parquet file")
    flen = int.from_bytes(mv[-8:-4], "little")
    fstart = len(mv) - 8 - flen
    tree, _ = tc.read_tree(mv, fstart)
    return mv[4:fstart], tree


def _shift_row_group(rg, shift: int, ordinal: int) -> None:
    for f in rg:
        if f[0] == _RG_FILE_OFFSET:
            f[2] += shift
        elif f[0] == _RG_ORDINAL:
            f[2] = ordinal
    for cc in _field(rg, _RG_COLUMNS)[2][1]:
        for f in cc:
            if f[0] == _CC_FILE_OFFSET and f[2]:
                f[2] += shift
            elif f[0] in _CC_PAGE_INDEX_FIELDS:
                raise ValueError("page indexes are not supported")
        for f in _field(cc, _CC_META)[2]:
            if f[0] in _CMD_OFFSETS:
                f[2] += shift
            elif f[0] in _CMD_BLOOM:
                raise ValueError("bloom filters are not supported")


class _Stitcher:
    """Lays parts (complete parquet files holding consecutive row groups of
    one table) out in a single file. add() only reserves the byte range and
    shifts the metadata; the copy itself is a positional write that the
    caller may run on any thread."""

    def __init__(self, path: str):
        self.fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        self.pos = 4
        self.head = None       # footer tree of the first part
        self.row_groups: List[list] = []
        self.num_rows = 0
        self.writes: List[Future] = []

    def add(self, part) -> Callable[[], None]:
        body, tree = _split(part)
        at = self.pos
        for rg in _field(tree, _FMD_ROW_GROUPS)[2][1]:
            _shift_row_group(rg, at - 4, len(self.row_groups))
            self.row_groups.append(rg)
        self.num_rows += _field(tree, _FMD_NUM_ROWS)[2]
        if self.head is None:
            self.head = tree
        self.pos += len(body)
        return functools.partial(_pwrite_all, self.fd, body, at)

    def close(self) -> None:
        try:
            for w in self.writes:
                w.result()
            if self.head is None:
                raise ValueError("no parts written")
            _field(self.head, _FMD_NUM_ROWS)[2] = self.num_rows
            _field(self.head, _FMD_ROW_GROUPS)[2] = (tc.CT_STRUCT, self.row_groups)
            footer = tc.write_tree(self.head)
            _pwrite_all(self.fd, MAGIC, 0)
            _pwrite_all(self.fd, bytes(footer) + len(footer).to_bytes(4, "little") + MAGIC,
                        self.pos)
        finally:
            os.close(self.fd)


def _pwrite_all(fd: int, data, at: int) -> None:
    mv = memoryview(data)
    while len(mv):
        n = os.pwrite(fd, mv, at)
        mv = mv[n:]
        at += n


def write_files(jobs: Iterable[Tuple[str, List[Callable[[], object]]]],
                threads: int = 0) -> None:
    """jobs: (output path, [part makers]) per file; each maker returns a
    complete parquet file (bytes-like) holding the next run of row groups.
    Makers run on `threads` workers and a few more threads copy finished
    parts into place; at most 2*threads parts are held in memory, and the
    parts of every file are laid out strictly in order."""
    threads = threads or default_threads()
    flat = [(path, i, len(makers), mk)
            for path, makers in jobs for i, mk in enumerate(makers)]
    pending = deque()      # parts being encoded
    copying = deque()      # parts being copied into their file
    nxt = 0
    out = None
    with ThreadPoolExecutor(max_workers=threads) as pool, \
            ThreadPoolExecutor(max_workers=min(4, threads)) as copiers:
        try:
            while nxt < len(flat) or pending:
                while copying and (copying[0].done() or len(copying) >= threads):
                    copying.popleft().result()
                while nxt < len(flat) and len(pending) + len(copying) < 2 * threads:
                    pending.append((flat[nxt], pool.submit(flat[nxt][3])))
                    nxt += 1
                (path, i, n, _), fut = pending.popleft()
                part = fut.result()
                if i == 0:
                    out = _Stitcher(path)
                w = copiers.submit(out.add(part))
                del part
                out.writes.append(w)
                copying.append(w)
                if i == n - 1:
                    out.close()
                    out = None
        finally:
            for _, fut in pending:
                fut.cancel()
            if out is not None:  # failed mid-file: let its copies land first
                for w in out.writes:
                    w.exception()
                os.close(out.fd)
