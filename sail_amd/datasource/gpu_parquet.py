"""GPU Parquet -> Arrow-in-HBM decode path (BASELINE config #2).

The reference scans parquet with arrow-rs on the CPU
(ref: crates/sail-data-source/src/formats/parquet/mod.rs, tuning surface
crates/sail-common/src/config/application.yaml:424-521). Here the decode
itself runs on the MI355X: the host reads raw column-chunk bytes into HBM
(pq_upload.py), parses page headers once per file (pq_index.py,
utils/thrift_compact), and this module launches batched page-table kernels
(ops/csrc/parquet_decode.hip, ops/csrc/parquet_types.hip).
Decoded columns are born as device tensors — no pyarrow on the hot path.

Supported: uncompressed v1 and v2 data pages (mixed freely within a
column), PLAIN fixed-width, PLAIN byte_array, RLE_DICTIONARY (+PLAIN
dictionary pages), string columns that fall back from RLE_DICTIONARY to
PLAIN pages, DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY,
DELTA_BYTE_ARRAY, BYTE_STREAM_SPLIT on INT32/INT64/FLOAT/DOUBLE, BOOLEAN (PLAIN and RLE),
INT96 timestamps (PLAIN and dictionary; decoded to int64 microseconds),
FLBA/INT32/INT64 decimals, definition levels (nulls). Anything else raises
Unsupported and the caller falls back to the host pyarrow path
(parquet_io.read): v2 pages in a compressed chunk, codecs other than
opt-in Snappy, DELTA_BYTE_ARRAY on FIXED_LEN_BYTE_ARRAY or mixed with another
encoding in one column, BYTE_STREAM_SPLIT on FIXED_LEN_BYTE_ARRAY,
dictionary-encoded BOOLEAN, nested columns.

DELTA_BYTE_ARRAY (front-coded) string pages decode in two launches
(ops/csrc/parquet_delta_bytearray.hip): pq_dba_lengths reads both length
streams of every page and checks all the format asks of them, their running
sum gives the output offsets, and pq_dba_expand rebuilds the values, one
wave per page, in an LDS buffer it edits in place. A page either kernel
rejects raises Unsupported. SAIL_IO_GPU_DELTA_BYTEARRAY=off refuses the
encoding. A chunk that mixes it with dictionary pages (parquet-java's v2
dictionary fallback) is still refused.

DELTA_BINARY_PACKED integer pages decode with one launch of pq_delta_values
(ops/csrc/parquet_delta.hip), which writes final values of the column's own
width; SAIL_IO_GPU_DELTA_FUSED=off selects the older pq_delta_decode +
pq_segscan + cast. The finished page tables of a fixed-width column depend
only on the file, the column and the row-group window, so they are built
once, kept on the FileIndex with their device copies (_Tables, at most
TABLE_CACHE_CAP bytes per process) and reused by every later scan.

Opt-in (config sail.io.gpu_snappy / env SAIL_IO_GPU_SNAPPY / read option
gpuSnappy, default off): SNAPPY column chunks with v1 data pages. The
compressed chunk bytes are uploaded as they are, one launch of
pq_snappy_decompress (ops/csrc/snappy.hip) expands every page of the
window, dictionary pages included, into a packed device buffer, and the
page decoders above run on that buffer. In a compressed page the
definition levels and the dictionary bit-width byte are inside the
compressed body, so they are resolved after the first decompress of a
column from two small device->host gathers and cached on the page index.
A page the kernel rejects (non-zero status) raises Unsupported.

PLAIN byte arrays (plain string pages and every string dictionary page)
are indexed by pq_bytearray_index and copied by pq_gather_bytes
(ops/csrc/parquet_bytearray.hip); SAIL_IO_GPU_BYTEARRAY_FAST=off selects
the older pq_bytearray_walk + pq_gather_strings. pq_bytearray_index checks
every length against its page and reports a status per page; a page it
rejects raises Unsupported.

A string column whose dictionary outgrew the writer's limit holds
RLE_DICTIONARY pages followed by PLAIN pages, within one chunk or across
the row groups of a window (stock pyarrow, parquet-java and arrow-rs all
write this for comment, URL, name and address columns). It decodes to the
plain form StringColumn(offsets, bytes, validity, None): every dense value
is described as (length, position in the upload), from the length chain
for PLAIN pages and from the chunk's indexed dictionary page through the
decoded codes for dictionary pages, and one gather assembles the bytes.
Such a column carries no dictionary codes, so a later GROUP BY or join on
it goes through exact string codes; a single-encoding column keeps its
coded form. A mix that involves DELTA_LENGTH_BYTE_ARRAY is still refused.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ..engine import types as T
from ..engine.column import Column, StringColumn, Table
# re-exported: callers and tests reach the index, the switches and the
# upload through this module
from .pq_index import (  # noqa: F401
    BYTE_STREAM_SPLIT, DELTA_BINARY_PACKED, DELTA_BYTE_ARRAY,
    DELTA_LENGTH_BYTE_ARRAY, PLAIN, PLAIN_DICTIONARY, RLE, RLE_DICTIONARY,
    TABLE_CACHE_CAP, _INDEX_CACHE, FileIndex, Unsupported, _check_all_valid,
    bytearray_fast_enabled, cached_table_bytes, delta_bytearray_enabled,
    delta_fused_enabled, file_index, forget_files, native_reader_enabled,
    snappy_enabled)
from .pq_upload import _coalesce, _native_reader, _upload_ranges  # noqa: F401

_JULIAN_UNIX_EPOCH = 2440588          # Julian day number of 1970-01-01
_MICROS_PER_DAY = 86_400_000_000


def _check_dict_codes(codes: torch.Tensor, limits: torch.Tensor, name: str):
    """Raise Unsupported unless 0 <= codes[i] < limits[i] for every i.
    `limits` holds, per code, the entry count of the dictionary the code
    indexes. Runs on the device and reads one flag back; callers index
    with `codes` only after it returns."""
    if codes.numel() == 0:
        return
    c = codes.to(torch.int64)
    bad = (c < 0) | (c >= limits)
    if bool(bad.any().item()):
        i = int(torch.nonzero(bad).flatten()[0].item())
        raise Unsupported(f"{name}: dictionary code {int(c[i].item())} at "
                          f"dense value {i} outside a dictionary of "
                          f"{int(limits[i].item())} entries")


class PageRow(NamedTuple):
    """One row of a kernel page table (ops/csrc/parquet_decode.hip): a
    source region of the upload, the values it holds, the output row they
    start at, and two per-kernel extras."""
    src_off: int
    src_len: int
    n_values: int
    out_row: int
    aux: int = 0
    bw: int = 0


# the same fields as columns of an int64 [n,6] table
SRC_OFF, SRC_LEN, N_VALUES, OUT_ROW, AUX, BW = range(6)


def _rows_array(rows) -> np.ndarray:
    """Page rows (PageRows, any 6-sequences, or an array of them) as an
    int64 [n,6] array. A list goes through one flat iterator: np.asarray
    takes twice as long over tuple subclasses as over plain tuples."""
    if isinstance(rows, np.ndarray):
        return rows.astype(np.int64, copy=False).reshape(-1, 6)
    flat = itertools.chain.from_iterable(rows)
    return np.fromiter(flat, np.int64, 6 * len(rows)).reshape(-1, 6)


class _Tables:
    """The finished page tables of one fixed-width column window: per row
    class the int64 [n,6] array and its device copy, and what decode() needs
    beside them. A pure function of file, column, row-group window and
    Snappy switch while every chunk is uncompressed: the upload-relative
    offsets are cumulative chunk lengths."""

    __slots__ = ("n_pages", "n_dense", "all_valid", "rows", "dev",
                 "delta_total", "dict_chunks", "nbytes")

    def __init__(self, n_pages, n_dense, all_valid, classes, dict_chunks,
                 device):
        self.n_pages = n_pages
        self.n_dense = n_dense
        self.all_valid = all_valid
        self.rows: Dict[str, np.ndarray] = {}
        self.dev: Dict[str, torch.Tensor] = {}
        for name, rows in classes.items():
            arr = self.rows[name] = _rows_array(rows)
            if len(arr):
                self.dev[name] = torch.from_numpy(arr).to(device)
        d = self.rows["delta"]
        self.delta_total = int((d[:, OUT_ROW] + d[:, N_VALUES]).max()) \
            if len(d) else 0
        self.dict_chunks = dict_chunks
        self.nbytes = 2 * sum(a.nbytes for a in self.rows.values())


def _lex_perm(offsets: torch.Tensor, blob: torch.Tensor) -> torch.Tensor:
    """Permutation that lex-sorts the strings of a (offsets, blob) pair.

    Parquet dictionary pages are in writer first-occurrence order, but the
    engine's dict-code invariant is code order == byte order (StringColumn
    min/max, comparisons and ORDER BY all compare codes). LSD-stable
    argsorts over big-endian 8-byte words restore it on device; 0x00
    padding past each string's end makes prefixes sort first."""
    n = offsets.numel() - 1
    dev = offsets.device
    if n <= 1:
        return torch.arange(n, device=dev)
    lens = offsets[1:] - offsets[:-1]
    maxw = (int(lens.max().item()) + 7) // 8
    perm = torch.arange(n, device=dev)
    if maxw == 0:
        return perm
    starts = offsets[:-1]
    ends = offsets[1:]
    pad_blob = torch.cat([blob, blob.new_zeros(8)])
    sentinel = blob.numel()
    byte_off = torch.arange(8, device=dev)
    for w in range(maxw - 1, -1, -1):
        idx = starts.unsqueeze(1) + w * 8 + byte_off
        idx = torch.where(idx < ends.unsqueeze(1), idx,
                          torch.full_like(idx, sentinel))
        b = pad_blob.index_select(0, idx.reshape(-1)) \
            .reshape(n, 8).to(torch.int64)
        key = ((b[:, 0] << 56) | (b[:, 1] << 48) | (b[:, 2] << 40) |
               (b[:, 3] << 32) | (b[:, 4] << 24) | (b[:, 5] << 16) |
               (b[:, 6] << 8) | b[:, 7])
        key = key ^ (-(1 << 63))  # top bit flip: unsigned byte order
        perm = perm.index_select(
            0, torch.argsort(key.index_select(0, perm), stable=True))
    return perm


def _lex_sort_dict(d_offs: torch.Tensor, d_bytes: torch.Tensor):
    """Sort a device dictionary lexicographically.
    Returns (sorted_offsets, sorted_bytes, old_code -> new_code map)."""
    perm = _lex_perm(d_offs, d_bytes)
    n = perm.numel()
    old_to_new = torch.empty(n, dtype=torch.int64, device=perm.device)
    old_to_new.scatter_(0, perm, torch.arange(n, device=perm.device))
    col = StringColumn(d_offs, d_bytes, None, None).gather(perm)
    return col.offsets, col.bytes_, old_to_new


# -- decode ------------------------------------------------------------------

_ALLOW_CPU = False  # tests: run the orchestration against a kernel simulator


def _ext():
    from ..ops import kernels

    return kernels.require()


def _page_table(rows, device):
    return torch.from_numpy(_rows_array(rows)).to(device)


def _segmented_cumsum(deltas: torch.Tensor, counts: List[int]) -> torch.Tensor:
    """Per-page cumulative sum: deltas holds [first, d1, ...] per segment."""
    cs = torch.cumsum(deltas, 0)
    # no values at all (every page null): the base gather below would index
    # an empty tensor
    if len(counts) <= 1 or deltas.numel() == 0:
        return cs
    bounds = np.cumsum([0] + counts[:-1])
    starts = torch.from_numpy(bounds).to(deltas.device)
    base = torch.where(starts > 0, cs.index_select(0, (starts - 1).clamp(min=0)),
                       torch.zeros_like(starts))
    rep = torch.repeat_interleave(
        base, torch.from_numpy(np.asarray(counts)).to(deltas.device))
    return cs - rep


def _decode_dict_host(raw: bytes, physical: str, nvals: int, flba_w: int):
    """Decode a PLAIN fixed-width dictionary page on the host (dict pages
    are small; string dictionaries are decoded on the device)."""
    if physical == "INT64":
        return np.frombuffer(raw, dtype="<i8", count=nvals).copy()
    if physical == "INT32":
        return np.frombuffer(raw, dtype="<i4", count=nvals).copy()
    if physical == "DOUBLE":
        return np.frombuffer(raw, dtype="<f8", count=nvals).copy()
    if physical == "FLOAT":
        return np.frombuffer(raw, dtype="<f4", count=nvals).copy()
    if physical == "INT96":
        # same arithmetic as pq_int96_micros: truncating division (fmod
        # keeps the dividend's sign), wrapping int64
        if len(raw) < 12 * nvals:
            raise Unsupported("INT96 dict page shorter than its values")
        b = np.frombuffer(raw, dtype=np.uint8,
                          count=nvals * 12).reshape(nvals, 12)
        nanos = np.ascontiguousarray(b[:, :8]).view("<i8").reshape(nvals)
        days = np.ascontiguousarray(b[:, 8:]).view("<i4").reshape(nvals) \
            .astype(np.int64) - _JULIAN_UNIX_EPOCH
        with np.errstate(over="ignore"):
            return days * np.int64(_MICROS_PER_DAY) + \
                (nanos - np.fmod(nanos, 1000)) // 1000
    if physical == "FIXED_LEN_BYTE_ARRAY":
        b = np.frombuffer(raw, dtype=np.uint8,
                          count=nvals * flba_w).reshape(nvals, flba_w)
        out = np.zeros(nvals, dtype=np.int64)
        for i in range(flba_w):
            out = (out << 8) | b[:, i]
        sign = 1 << (8 * flba_w - 1)
        return np.where(out & sign, out - (1 << (8 * flba_w)), out)
    raise Unsupported(f"dict page physical type {physical}")


_PHYS_WIDTH = {"INT32": 4, "INT64": 8, "FLOAT": 4, "DOUBLE": 8}
_PHYS_TORCH = {"INT32": torch.int32, "INT64": torch.int64,
               "FLOAT": torch.float32, "DOUBLE": torch.float64}


class _ColumnDecoder:
    """Decodes one column of one file into device buffers. `rg_window`
    restricts to row groups [lo, hi) — the out-of-core scan streams
    batches of row groups instead of whole files."""

    def __init__(self, idx: FileIndex, name: str, device, rg_window=None,
                 snappy: Optional[bool] = None):
        self.idx = idx
        self.device = device
        self.ci = idx.column_index(name)
        self.sc = idx.schema.column(self.ci)
        self.physical = self.sc.physical_type
        self.flba_w = self.sc.length or 0
        snappy = snappy_enabled() if snappy is None else bool(snappy)
        window = None if rg_window is None else tuple(rg_window)
        win = idx.window(self.ci, window, snappy)
        self.chunks, self.pages = win.chunks, win.pages
        self.nrows, self.compressed, encs = win.nrows, win.compressed, win.encs
        # what this column's caches on the index are keyed by
        self._dict_key = (self.ci, window)
        self._win_key = (self.ci, window, snappy, str(device))
        if self.physical == "BOOLEAN":
            ok = {PLAIN, RLE}
        elif self.physical == "INT96":
            ok = {PLAIN, RLE_DICTIONARY}
        else:
            ok = {PLAIN, RLE_DICTIONARY, DELTA_BINARY_PACKED,
                  DELTA_LENGTH_BYTE_ARRAY}
            if self.physical in _PHYS_WIDTH:
                ok.add(BYTE_STREAM_SPLIT)
            # front-coded strings: with the switch on, and only from an
            # extension that has the decoder (the kernel simulators of the
            # tests do not), as for pq_bytearray_index below
            if self.physical == "BYTE_ARRAY" and DELTA_BYTE_ARRAY in encs \
                    and delta_bytearray_enabled() \
                    and hasattr(_ext(), "pq_dba_expand"):
                ok.add(DELTA_BYTE_ARRAY)
        bad = encs - ok
        if bad:
            raise Unsupported(f"{self.sc.name}: encodings {bad}")
        # strings: one encoding, or the dictionary-fallback layout
        if self.physical == "BYTE_ARRAY" and len(encs) > 1 and \
                encs != {PLAIN, RLE_DICTIONARY}:
            raise Unsupported(f"{self.sc.name}: mixed string encodings {encs}")
        if self.physical not in ("INT32", "INT64", "FLOAT", "DOUBLE",
                                 "BYTE_ARRAY", "FIXED_LEN_BYTE_ARRAY",
                                 "BOOLEAN", "INT96"):
            raise Unsupported(f"{self.sc.name}: physical {self.physical}")

    # -- staging ----------------------------------------------------------
    def upload(self):
        ranges = [(ch.start, ch.end) for ch in self.chunks]
        self.buf, offs = _upload_ranges(self.idx.path, ranges, self.device)
        # Where things sit in self.buf, the one place that knows whether the
        # column is compressed. _page_at[page ordinal]: what the page's
        # def_off/val_off count from (uncompressed: file offset -> upload
        # offset; compressed: the page's start in the packed buffer).
        # _dict_at[chunk ordinal]: (offset, length) of its dictionary page.
        if self.compressed:
            self._decompress(offs)
            return
        rel = [off - ch.start for ch, off in zip(self.chunks, offs)]
        # an array, repeated per chunk: a column whose tables are cached
        # must not pay per page here
        self._page_at = np.repeat(np.asarray(rel, dtype=np.int64),
                                  [len(ch.pages) for ch in self.chunks])
        self._dict_at = [None if ch.dict_off is None
                         else (ch.dict_off + r, ch.dict_len)
                         for ch, r in zip(self.chunks, rel)]

    def _walk(self, counts):
        """Every page of the window in page order: (page, chunk ordinal,
        page ordinal, offset of its value region in self.buf,
        counts[ordinal], sum of the counts before it). With the per-page
        dense counts the last two are a row's n_values and out_row."""
        pi = base = 0
        page_at = self._page_at.tolist()
        for k, ch in enumerate(self.chunks):
            for p in ch.pages:
                yield p, k, pi, page_at[pi] + p.val_off, counts[pi], base
                base += counts[pi]
                pi += 1

    def _value_rows(self, dense_counts) -> np.ndarray:
        """The walk's common case as an [n,6] table: one row per page over
        its whole value region, bw the page's bit-width byte (0 unless
        dictionary-coded). A string column rebuilds this on every scan, so
        it is filled column-wise: a named tuple per page costs a third
        more host time per scan than the tuples it replaced."""
        n = len(self.pages)
        counts = np.asarray(dense_counts, dtype=np.int64)
        rows = np.zeros((n, 6), dtype=np.int64)
        for col, field in ((SRC_OFF, "val_off"), (SRC_LEN, "val_len"),
                           (BW, "bw0")):
            rows[:, col] = np.fromiter(
                (getattr(p, field) for p in self.pages), np.int64, n)
        rows[:, SRC_OFF] += self._page_at
        rows[:, N_VALUES] = counts
        rows[:, OUT_ROW] = np.cumsum(counts) - counts
        return rows

    def _decompress(self, offs):
        """SNAPPY chunks, uploaded at `offs`: expand every page of the
        window (dictionary pages too) with one launch into a packed buffer,
        make that buffer self.buf, and resolve the page-internal layout of
        pages seen for the first time."""
        if not all(ch.compressed for ch in self.chunks):
            raise Unsupported(f"{self.sc.name}: compressed and uncompressed "
                              "row groups in one column")
        rows = []
        at = 0
        page_at, self._dict_at = [], []
        for ch, off in zip(self.chunks, offs):
            rel = off - ch.start
            self._dict_at.append(None)
            if ch.dict_off is not None:
                rows.append(PageRow(ch.dict_off + rel, ch.dict_len,
                                    ch.dict_ulen, at))
                self._dict_at[-1] = (at, ch.dict_ulen)
                at += ch.dict_ulen
            for p in ch.pages:
                rows.append(PageRow(p.comp_off + rel, p.comp_len, p.ulen, at))
                page_at.append(at)
                at += p.ulen
        self._page_at = np.asarray(page_at, dtype=np.int64)
        # +16 zeroed tail: the buffer contract of the page decoders
        packed = torch.empty(at + 16, dtype=torch.uint8, device=self.device)
        packed[at:] = 0
        status = _ext().pq_snappy_decompress(
            self.buf, _page_table(rows, self.device), packed)
        bad = torch.nonzero(status).flatten()
        if bad.numel():
            i = int(bad[0].item())
            raise Unsupported(f"{self.sc.name}: snappy page {i} of "
                              f"{len(rows)} rejected, status "
                              f"{int(status[i].item())}")
        # the compressed upload is released here; its record_stream() keeps
        # the allocator from reusing it before the decompress has run
        self.buf = packed
        self._resolve_pages()

    def _resolve_pages(self):
        """Fill def_len/all_valid/val_off/val_len/bw0 of compressed pages
        not seen before: one gather of each page's first 16 bytes, and for
        dictionary-encoded pages behind definition levels one more of the
        bit-width byte at 4 + def_len."""
        pending = [(p, base) for p, base in
                   zip(self.pages, self._page_at.tolist()) if not p.resolved]
        if not pending:
            return
        todo, at = zip(*pending)
        max_def = self.sc.max_definition_level
        bases = torch.tensor(at, dtype=torch.int64, device=self.device)
        # the packed buffer's 16-byte tail keeps base + 15 inside it
        idx = bases.unsqueeze(1) + torch.arange(16, device=self.device)
        heads = self.buf[idx.reshape(-1)].reshape(-1, 16).cpu().numpy()
        layout = []
        for p, head in zip(todo, heads):
            raw = head.tobytes()
            if max_def > 0:
                dl = int.from_bytes(raw[:4], "little")
                if p.ulen < 4 or dl > p.ulen - 4:
                    raise Unsupported(f"{self.sc.name}: def-level length "
                                      f"{dl} outside its page")
                av = _check_all_valid(raw, 4, dl, p.nvals)
                layout.append((4, dl, av, 4 + dl))
            else:
                layout.append((0, 0, True, 0))
        bw = [0] * len(todo)
        want = [k for k, p in enumerate(todo) if p.enc == RLE_DICTIONARY
                and layout[k][3] < p.ulen]
        if want:
            bw_at = torch.tensor([at[k] + layout[k][3] for k in want],
                                 dtype=torch.int64, device=self.device)
            for k, b in zip(want, self.buf[bw_at].cpu().tolist()):
                bw[k] = int(b)
        for p, (doff, dl, av, voff), b in zip(todo, layout, bw):
            p.def_off, p.def_len, p.all_valid = doff, dl, av
            p.val_off, p.val_len, p.bw0 = voff, p.ulen - voff, b
            p.resolved = True

    # -- validity ---------------------------------------------------------
    def decode_validity(self):
        """(validity u8 tensor or None, per-page dense (non-null) counts)."""
        nvals = [p.nvals for p in self.pages]
        if all(p.all_valid for p in self.pages):
            return None, nvals
        # a page without levels to decode gets an empty row: filled below.
        # off - p.val_off is what the page's def_off counts from as well
        rows = [PageRow(0, 0, 0, base, 0, 1)
                if p.all_valid or p.def_len == 0 else
                PageRow(off - p.val_off + p.def_off, p.def_len, n, base, 0, 1)
                for p, _, _, off, n, base in self._walk(nvals)]
        ext = _ext()
        levels = ext.pq_rle_decode(self.buf, _page_table(rows, self.device),
                                   self.nrows)
        # pages skipped above are all-valid: fill their ranges with 1
        base = 0
        for p in self.pages:
            if p.all_valid or p.def_len == 0:
                levels[base:base + p.nvals] = 1
            base += p.nvals
        valid = levels.to(torch.bool)
        counts = []
        base = 0
        for p in self.pages:
            if p.all_valid:
                counts.append(p.nvals)
            elif p.ndense is not None:
                counts.append(p.ndense)   # v2 header: no device round trip
            else:
                counts.append(int(valid[base:base + p.nvals].sum().item()))
            base += p.nvals
        return valid.to(torch.uint8), counts

    # -- value decode ------------------------------------------------------
    def _fixed_width(self):
        if self.physical == "FIXED_LEN_BYTE_ARRAY":
            return self.flba_w, torch.int64
        if self.physical == "BOOLEAN":
            return 0, torch.uint8           # bit-packed; one byte per value
        if self.physical == "INT96":
            return 12, torch.int64          # decoded to epoch microseconds
        return _PHYS_WIDTH[self.physical], _PHYS_TORCH[self.physical]

    def _build_tables(self, dense_counts, all_valid) -> Tuple[_Tables, bool]:
        """Page tables of a fixed-width column, one per row class, from the
        per-page dense counts. Second value: whether the row loop met a
        class whose regions it checks against n_values (those tables are
        rebuilt, and so rechecked, on every scan)."""
        width, _ = self._fixed_width()
        classes = {"plain": [], "dict": [], "delta": [], "bss": [], "rle": []}
        plain_rows, dict_rows, delta_rows, bss_rows, rle_rows = (
            classes[k] for k in ("plain", "dict", "delta", "bss", "rle"))
        dict_chunks = []  # (chunk ordinal, dense row range) needing dict values
        checked = self.physical in ("BOOLEAN", "INT96")

        def _short(what):   # `pi`: the page the walk below has reached
            return Unsupported(f"{self.sc.name}: page {pi}: {what}")

        # the value kernels trust n_values: every region is checked against
        # it here, while the table is still on the host
        for p, k, pi, off, c, b in self._walk(dense_counts):
            if p.enc == PLAIN:
                if self.physical == "BOOLEAN" and p.val_len * 8 < c:
                    raise _short(f"{p.val_len} bytes for {c} booleans")
                if self.physical == "INT96" and p.val_len < 12 * c:
                    raise _short(f"{p.val_len} bytes for {c} INT96 values")
                plain_rows.append(PageRow(off, p.val_len, c, b, 0, width))
            elif p.enc == RLE_DICTIONARY:
                dict_rows.append(PageRow(off, p.val_len, c, b, 0, p.bw0))
                dict_chunks.append((k, b, c))
            elif p.enc == DELTA_BINARY_PACKED:
                delta_rows.append(PageRow(off, p.val_len, c, b))
            elif p.enc == BYTE_STREAM_SPLIT:
                checked = True
                if p.val_len != width * c:
                    raise _short(f"{p.val_len} bytes for {c} "
                                 f"byte-stream-split values of {width}")
                bss_rows.append(PageRow(off, p.val_len, c, b))
            elif p.enc == RLE:
                checked = True
                # RLE booleans: 4-byte length prefix, then hybrid runs
                # of width 1. A page of nulls only has no value bytes.
                if c == 0:
                    rle_rows.append(PageRow(0, 0, 0, b, 0, 1))
                elif p.val_len < 4:
                    raise _short(f"{p.val_len} bytes for {c} RLE booleans")
                else:
                    rle_rows.append(PageRow(off + 4, p.val_len - 4, c, b, 0, 1))
        return _Tables(len(self.pages), sum(dense_counts), all_valid, classes,
                       dict_chunks, self.device), checked

    def _tables(self):
        """(page tables, validity) of this scan. The tables come from the
        FileIndex when they were built before; the bypasses are columns
        with compressed chunks (their bases come from the decompress step),
        columns whose dense counts need a device round trip (v1 pages with
        nulls and no count in the header) and columns with a length-checked
        class."""
        tabs = None if self.compressed else self.idx.tables(self._win_key)
        if tabs is not None:
            validity = None if tabs.all_valid else self.decode_validity()[0]
            return tabs, validity
        validity, dense_counts = self.decode_validity()
        tabs, checked = self._build_tables(dense_counts, validity is None)
        if not (self.compressed or checked) and all(
                p.all_valid or p.ndense is not None for p in self.pages):
            self.idx.remember_tables(self._win_key, tabs)
        return tabs, validity

    def decode(self):
        self.upload()
        ext = _ext()
        dev = self.device

        if self.physical == "BYTE_ARRAY":
            validity, dense_counts = self.decode_validity()
            return self._decode_strings(ext, validity, dense_counts), validity

        # fixed-width physical types; the pages of a column may mix the
        # row classes plain, dict, delta, byte-stream-split and RLE booleans
        width, dt = self._fixed_width()
        tabs, validity = self._tables()
        n_dense, pi = tabs.n_dense, tabs.n_pages
        plain_rows, dict_rows, delta_rows, bss_rows, rle_rows = (
            tabs.rows[k] for k in ("plain", "dict", "delta", "bss", "rle"))
        dense: Optional[torch.Tensor] = None

        def _out():
            nonlocal dense
            if dense is None:
                dense = torch.empty(n_dense, dtype=dt, device=dev)
            return dense

        def _place(rows, vals):
            """Rows of one class decoded into `vals` (n_dense long, written
            at each page's out_row): the column itself when every page is of
            that class, else copied page by page into the common output."""
            nonlocal dense
            if len(rows) == pi:
                dense = vals if vals.dtype == dt else vals.to(dt)
            else:
                o = _out()
                for r in rows:
                    lo, hi = r[OUT_ROW], r[OUT_ROW] + r[N_VALUES]
                    o[lo:hi] = vals[lo:hi]

        if len(plain_rows):
            # kernels write at out_row (dense row base); the output tensor
            # covers all n_dense rows even when other pages use another enc
            table = tabs.dev["plain"]
            if self.physical == "FIXED_LEN_BYTE_ARRAY":
                _place(plain_rows,
                       ext.pq_flba_i64(self.buf, table, n_dense, width))
            elif self.physical == "BOOLEAN":
                _place(plain_rows,
                       ext.pq_bool_unpack(self.buf, table, n_dense))
            elif self.physical == "INT96":
                _place(plain_rows,
                       ext.pq_int96_micros(self.buf, table, n_dense))
            else:
                raw = ext.pq_plain_copy(self.buf, table, n_dense, width)
                _place(plain_rows, raw.view(dt))

        if len(bss_rows):
            raw = ext.pq_bss_decode(self.buf, tabs.dev["bss"], n_dense, width)
            _place(bss_rows, raw.view(dt))

        if len(rle_rows):
            bits = ext.pq_rle_decode(self.buf, tabs.dev["rle"], n_dense)
            _place(rle_rows, bits)

        if len(delta_rows):
            if self.physical not in ("INT32", "INT64"):
                raise Unsupported(f"{self.sc.name}: DELTA on {self.physical}")
            table = tabs.dev["delta"]
            if delta_fused_enabled() and hasattr(ext, "pq_delta_values"):
                # one pass: packed bytes in, final values of the column's
                # own width out
                vals = ext.pq_delta_values(self.buf, table, tabs.delta_total,
                                           dt == torch.int32)
            else:
                vals, _ = ext.pq_delta_decode(self.buf, table,
                                              tabs.delta_total)
                # finish [first, d1, ...] -> values with the on-device
                # per-page scan (replaces torch.cumsum + cat + correction
                # gathers)
                ext.pq_segscan(vals, table)
            _place(delta_rows, vals)

        if len(dict_rows):
            codes = self._decode_dict_codes(ext, dict_rows)
            o = _out()
            at = 0
            for (k, b, c) in tabs.dict_chunks:
                o[b:b + c] = self._dict_values(k).index_select(
                    0, codes[at:at + c].to(torch.int64))
                at += c

        return self._fixed_to_column(_out(), validity), validity

    def _decode_dict_codes(self, ext, dict_rows):
        """RLE_DICTIONARY pages: first byte = bitwidth (captured at index
        time), then hybrid runs. Decodes codes densely in dict_rows order.
        Width 0 is legal (one-entry dictionary under parquet-mr/arrow-rs):
        RLE runs then carry no value bytes, so it must not be clamped."""
        pages = _rows_array(dict_rows)
        n = pages[:, N_VALUES]
        rows = pages.copy()
        rows[:, SRC_OFF] += 1
        rows[:, SRC_LEN] -= 1
        rows[:, OUT_ROW] = np.cumsum(n) - n
        rows[:, AUX] = 0
        return ext.pq_rle_decode(self.buf, _page_table(rows, self.device),
                                 int(n.sum()))

    def _remap_codes(self, codes_dense, dense_counts, entry_codes,
                     entry_bases):
        """Map per-chunk dictionary codes to merged-dictionary codes in
        place."""
        at = 0
        pi = 0
        for ci, ch in enumerate(self.chunks):
            ch_n = sum(dense_counts[pi + k] for k in range(len(ch.pages)))
            base = entry_bases[ci]
            seg = codes_dense[at:at + ch_n]
            codes_dense[at:at + ch_n] = entry_codes.index_select(
                0, seg.to(torch.int64) + base).to(torch.int32)
            at += ch_n
            pi += len(ch.pages)

    def _decode_dict_strings(self, ext, k: int):
        """Decode the PLAIN string dictionary page of chunk `k` on the
        device: (offsets int64[n+1], bytes u8) tensors."""
        ch = self.chunks[k]
        if ch.dict_off is None:
            raise Unsupported(f"{self.sc.name}: dict-encoded page, no dict")
        rows = [PageRow(*self._dict_at[k], ch.dict_nvals, 0)]
        lengths, src_pos, status = self._index_bytearrays(
            ext, rows, ch.dict_nvals)
        return self._gather_bytearrays(ext, lengths, src_pos, status,
                                       lambda i: "dictionary page")

    def _dict_values(self, k: int) -> torch.Tensor:
        """The fixed-width dictionary of chunk `k` on the device; its
        host-decoded values are kept on the index."""
        ch = self.chunks[k]
        key = (self.ci, ch.start)
        vals = self.idx._dict_host.get(key)
        if vals is None:
            if ch.dict_off is None:
                raise Unsupported(f"{self.sc.name}: dict-encoded page, no dict")
            if ch.compressed:
                # the decompressed dictionary page is in the packed buffer
                d_off, d_len = self._dict_at[k]
                raw = self.buf[d_off:d_off + d_len].cpu().numpy().tobytes()
            else:
                with open(self.idx.path, "rb") as f:
                    f.seek(ch.dict_off)
                    raw = f.read(ch.dict_len)
            vals = self.idx._dict_host[key] = _decode_dict_host(
                raw, self.physical, ch.dict_nvals, self.flba_w)
        return torch.from_numpy(np.ascontiguousarray(vals)).to(self.device)

    # -- strings -----------------------------------------------------------
    def _merged_dictionary(self, ext):
        """(offsets, bytes, entry_codes, entry_bases): the window's
        lex-sorted string dictionary, and the map into it from chunk k's
        dictionary code c, entry_codes[entry_bases[k] + c]."""
        dev = self.device
        # decode every chunk's dictionary PAGE on the device (a
        # ClickBench URL dictionary is ~1M entries per row group —
        # host loops took minutes; device walk+gather takes ms)
        dict_cols = [self._decode_dict_strings(ext, k)
                     for k in range(len(self.chunks))]
        if len(dict_cols) == 1:
            # parquet dictionary pages are first-occurrence ordered;
            # re-sort to the engine's code-order == byte-order invariant
            d_offs, d_bytes, old_to_new = _lex_sort_dict(*dict_cols[0])
            return d_offs, d_bytes, old_to_new, [0]
        # merge: exact codes over the concatenated dictionaries,
        # then remap each chunk's codes through its entry codes
        from ..engine.joins import exact_string_codes

        lens = torch.cat([o[1:] - o[:-1] for o, _ in dict_cols])
        offs = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offs[1:])
        blob = torch.cat([b for _, b in dict_cols])
        comb = StringColumn(offs, blob, None, None)
        entry_codes = exact_string_codes([comb])[0]
        n_merged = int(entry_codes.max().item()) + 1 \
            if entry_codes.numel() else 0
        rep = torch.zeros(n_merged, dtype=torch.int64, device=dev)
        rep.scatter_(0, entry_codes,
                     torch.arange(entry_codes.numel(), device=dev))
        merged_col = comb.gather(rep)
        # merged codes are hash-ordered: lex-sort the merged
        # dictionary and compose the remap (invariant above)
        d_offs, d_bytes, old_to_new = _lex_sort_dict(
            merged_col.offsets, merged_col.bytes_)
        sizes = [o.numel() - 1 for o, _ in dict_cols]
        return (d_offs, d_bytes, old_to_new.index_select(0, entry_codes),
                np.cumsum([0] + sizes[:-1]).tolist())

    def _decode_strings(self, ext, validity, dense_counts):
        enc = self.pages[0].enc if self.pages else PLAIN
        dev = self.device
        n_dense = sum(dense_counts)
        if any(p.enc != enc for p in self.pages):
            return self._decode_mixed_strings(ext, validity, dense_counts)
        rows = self._value_rows(dense_counts)
        if enc == RLE_DICTIONARY:
            codes_dense = self._decode_dict_codes(ext, rows)
            # merged dictionary + per-chunk entry remaps are a pure
            # function of the FILE (like the page index): kept on it, on
            # device — the per-row codes (the bulk) are still re-read and
            # re-decoded on every scan
            merged = self.idx._dicts.get(self._dict_key)
            if merged is None:
                merged = self.idx._dicts[self._dict_key] = \
                    self._merged_dictionary(ext)
            d_offs, d_bytes, entry_codes, entry_bases = merged
            self._remap_codes(codes_dense, dense_counts, entry_codes,
                              entry_bases)
            codes = self._scatter_codes(codes_dense, validity)
            return StringColumn(d_offs, d_bytes, validity, codes)

        if enc == DELTA_LENGTH_BYTE_ARRAY:
            pages = _rows_array(rows)
            deltas, data_end = ext.pq_delta_decode(
                self.buf, _page_table(pages, dev), n_dense)
            # per page: its string bytes follow the delta stream; copied
            # back to back (aux: the page's byte base in the blob)
            ends = data_end.cpu().numpy().astype(np.int64)
            nbytes = pages[:, SRC_LEN] - ends
            total_bytes = int(nbytes.sum())
            copy_rows, scan_rows = np.zeros_like(pages), np.zeros_like(pages)
            copy_rows[:, SRC_OFF] = pages[:, SRC_OFF] + ends
            copy_rows[:, SRC_LEN] = nbytes
            copy_rows[:, AUX] = scan_rows[:, AUX] = np.cumsum(nbytes) - nbytes
            scan_rows[:, N_VALUES] = pages[:, N_VALUES]
            scan_rows[:, OUT_ROW] = pages[:, OUT_ROW]
            blob = torch.empty(total_bytes, dtype=torch.uint8, device=dev)
            ext.pq_copy_bytes(self.buf, _page_table(copy_rows, dev), blob)
            if validity is None:
                # scan 1: delta stream -> length values (per page);
                # scan 2: lengths -> offsets, page byte base folded in via
                # aux (base == sum of earlier pages' lengths, so offsets
                # are globally continuous)
                len_rows = scan_rows.copy()
                len_rows[:, AUX] = 0
                ext.pq_segscan(deltas, _page_table(len_rows, dev))
                ext.pq_segscan(deltas, _page_table(scan_rows, dev))
                offsets = torch.zeros(n_dense + 1, dtype=torch.int64,
                                      device=dev)
                offsets[1:] = deltas
                return StringColumn(offsets, blob, None, None)
            lengths = _segmented_cumsum(deltas, dense_counts)
            offsets = torch.zeros(n_dense + 1, dtype=torch.int64, device=dev)
            torch.cumsum(lengths, 0, out=offsets[1:])
            return self._assemble_strings(offsets, blob, lengths, validity)

        if enc == DELTA_BYTE_ARRAY:
            # front-coded values: both length streams -> lengths; their
            # running sum -> output offsets; then one wave per page rebuilds
            # the values in LDS and writes them (parquet_delta_bytearray.hip)
            table = _page_table(rows, dev)
            prefix, suffix, lengths, suffix_start, status = \
                ext.pq_dba_lengths(self.buf, table, n_dense)
            offsets = torch.zeros(n_dense + 1, dtype=torch.int64, device=dev)
            torch.cumsum(lengths, 0, out=offsets[1:])
            # the one device->host read: the byte total and the rejections
            total, nbad = torch.stack(
                [offsets[-1], (status != 0).sum()]).tolist()
            if nbad:
                i = int(torch.nonzero(status).flatten()[0].item())
                raise Unsupported(
                    f"{self.sc.name}: DELTA_BYTE_ARRAY page {i} of "
                    f"{len(rows)} rejected, status {int(status[i].item())}")
            # every rule of the format is settled by now: pq_dba_expand
            # repeats the checks only to stay in bounds whatever it is handed
            blob = torch.empty(total, dtype=torch.uint8, device=dev)
            ext.pq_dba_expand(self.buf, table, prefix, suffix, suffix_start,
                              offsets, lengths, status, blob)
            return self._assemble_strings(offsets, blob, lengths, validity)

        # PLAIN byte arrays: sequential walk + parallel gather
        lengths, src_pos, status = self._index_bytearrays(ext, rows, n_dense)
        offsets, blob = self._gather_bytearrays(
            ext, lengths, src_pos, status, lambda i: f"page {i} of {len(rows)}")
        return self._assemble_strings(offsets, blob, lengths, validity)

    def _index_bytearrays(self, ext, rows, total):
        """PLAIN byte-array regions of self.buf -> (lengths, src_pos,
        per-region status or None): pq_bytearray_index, or
        pq_bytearray_walk (which checks nothing and has no status) when the
        switch is off or the extension lacks the new entry point."""
        table = _page_table(rows, self.device)
        if bytearray_fast_enabled() and hasattr(ext, "pq_bytearray_index"):
            return ext.pq_bytearray_index(self.buf, table, total)
        lengths, src_pos = ext.pq_bytearray_walk(self.buf, table, total)
        return lengths, src_pos, None

    def _gather_bytearrays(self, ext, lengths, src_pos, status, what):
        """(offsets int64[n+1], bytes u8) of values described by length
        and position in self.buf: one cumsum, one device->host read (the
        byte total and, with a status, the count of rejected regions), one
        gather. A rejected region raises Unsupported; what(i) names region
        i of the status."""
        n = lengths.numel()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(lengths, 0, out=offsets[1:])
        if status is not None and status.numel():
            total, nbad = torch.stack(
                [offsets[-1], (status != 0).sum()]).tolist()
            if nbad:
                i = int(torch.nonzero(status).flatten()[0].item())
                raise Unsupported(
                    f"{self.sc.name}: {what(i)} rejected, status "
                    f"{int(status[i].item())}")
        else:
            total = int(offsets[-1].item())
        if bytearray_fast_enabled() and hasattr(ext, "pq_gather_bytes"):
            blob = ext.pq_gather_bytes(self.buf, src_pos, lengths,
                                       offsets[:-1], total)
        else:
            blob = ext.pq_gather_strings(self.buf, src_pos, lengths,
                                         offsets[:-1], total)
        return offsets, blob

    def _decode_mixed_strings(self, ext, validity, dense_counts):
        """RLE_DICTIONARY and PLAIN pages in one column (the writer's
        dictionary overflowed): every dense value becomes (length, position
        in self.buf), then one gather. The result is a plain StringColumn,
        without codes."""
        dev = self.device
        n_dense = sum(dense_counts)
        plain_rows, dict_rows = [], []
        page_chunk = []     # per dictionary-encoded page: index of its chunk
        for p, ci, _, off, c, b in self._walk(dense_counts):
            if p.enc == PLAIN:
                plain_rows.append(PageRow(off, p.val_len, c, b))
            else:
                dict_rows.append(PageRow(off, p.val_len, c, b, 0, p.bw0))
                page_chunk.append(ci)
        # PLAIN pages write their dense rows; the rest stay (0, 0)
        lengths, src_pos, status = self._index_bytearrays(
            ext, plain_rows, n_dense)
        n_plain = len(plain_rows)
        used = sorted(set(page_chunk))   # chunks with dictionary-coded pages

        def what(i):
            if i < n_plain:
                return f"plain page {i} of {n_plain}"
            return f"dictionary page of row group {used[i - n_plain]}"

        n_codes = sum(r.n_values for r in dict_rows)
        if n_codes:
            codes = self._decode_dict_codes(ext, dict_rows)
            # one index launch over the dictionary pages of the chunks that
            # use them; chunk ci's entries start at ent_base[ci]
            ent_base, ent_rows, at = {}, [], 0
            for ci in used:
                ch = self.chunks[ci]
                if ch.dict_off is None:
                    raise Unsupported(
                        f"{self.sc.name}: dict-encoded page, no dict")
                ent_rows.append(PageRow(*self._dict_at[ci], ch.dict_nvals, at))
                ent_base[ci] = at
                at += ch.dict_nvals
            ent_len, ent_src, ent_status = self._index_bytearrays(
                ext, ent_rows, at)
            # per code: its dictionary's size and base, and its dense row
            per_page = torch.tensor(
                [[self.chunks[ci].dict_nvals for ci in page_chunk],
                 [ent_base[ci] for ci in page_chunk],
                 [r.out_row for r in dict_rows],
                 np.cumsum([0] + [r.n_values for r in dict_rows[:-1]]).tolist()],
                dtype=torch.int64, device=dev)
            counts = torch.tensor([r.n_values for r in dict_rows],
                                  dtype=torch.int64, device=dev)
            page_of = torch.repeat_interleave(
                torch.arange(len(dict_rows), device=dev), counts,
                output_size=n_codes)
            limit, base, row0, code0 = per_page.index_select(1, page_of)
            _check_dict_codes(codes, limit, self.sc.name)
            entry = codes.to(torch.int64) + base
            dest = row0 + (torch.arange(n_codes, device=dev) - code0)
            lengths[dest] = ent_len.index_select(0, entry)
            src_pos[dest] = ent_src.index_select(0, entry)
            if ent_status is not None:
                status = torch.cat([status, ent_status])
        offsets, blob = self._gather_bytearrays(ext, lengths, src_pos, status,
                                                what)
        return self._assemble_strings(offsets, blob, lengths, validity)

    def _scatter_codes(self, codes_dense, validity):
        if validity is None:
            return codes_dense
        full = torch.full((self.nrows,), -1, dtype=torch.int32,
                          device=self.device)
        vidx = torch.nonzero(validity, as_tuple=False).flatten()
        full[vidx] = codes_dense
        return full

    def _assemble_strings(self, offsets, blob, lengths, validity):
        if validity is None:
            return StringColumn(offsets, blob, None, None)
        full_len = torch.zeros(self.nrows, dtype=torch.int64,
                               device=self.device)
        vidx = torch.nonzero(validity, as_tuple=False).flatten()
        full_len[vidx] = lengths
        full_off = torch.zeros(self.nrows + 1, dtype=torch.int64,
                               device=self.device)
        torch.cumsum(full_len, 0, out=full_off[1:])
        return StringColumn(full_off, blob, validity, None)

    # -- type finishing ----------------------------------------------------
    def _fixed_to_column(self, dense: torch.Tensor, validity):
        at = self.idx.arrow_schema.field(self.sc.name).type
        import pyarrow as pa

        full = dense
        if validity is not None:
            full = torch.zeros(self.nrows, dtype=dense.dtype,
                               device=self.device)
            vidx = torch.nonzero(validity, as_tuple=False).flatten()
            full[vidx] = dense
        if pa.types.is_decimal(at):
            dt = T.DecimalType(at.precision, at.scale)
            return Column(dt, full.to(torch.int64), validity)
        if pa.types.is_date32(at):
            return Column(T.DATE, full.to(torch.int32), validity)
        if self.physical == "BOOLEAN":
            if not pa.types.is_boolean(at):
                raise Unsupported(f"{self.sc.name}: arrow type {at}")
            return Column(T.BOOL, full.to(torch.bool), validity)
        if self.physical == "INT96":
            # the file's arrow type says timestamp[ns]; the INT96 decoders
            # already produced the engine's epoch microseconds
            return Column(T.TIMESTAMP, full, validity)
        if pa.types.is_timestamp(at):
            unit = at.unit
            v = full.to(torch.int64)
            if unit == "ms":
                v = v * 1000
            elif unit == "ns":
                v = v // 1000
            elif unit == "s":
                v = v * 1_000_000
            return Column(T.TIMESTAMP, v, validity)
        m = {"int32": T.I32, "int64": T.I64, "float": T.F32, "double": T.F64,
             "int16": T.I16, "int8": T.I8}
        s = str(at)
        if s in m:
            want = m[s].storage
            return Column(m[s], full.to(want) if full.dtype != want else full,
                          validity)
        raise Unsupported(f"{self.sc.name}: arrow type {at}")


def read_gpu(files: List[str], schema, device, rg_window=None,
             snappy: Optional[bool] = None) -> Table:
    """Decode `schema`'s columns of the given parquet files on the GPU.
    Raises Unsupported when any file/column needs the host fallback.
    `snappy` turns device Snappy decompression on or off (None: the
    SAIL_IO_GPU_SNAPPY environment switch, default off)."""
    if not str(device).startswith("cuda") and not _ALLOW_CPU:
        raise Unsupported("gpu decode needs a cuda device")
    from ..engine.executor import concat_columns

    per_file: List[Dict[str, Column]] = []
    for path in files:
        idx = file_index(path)
        cols: Dict[str, Column] = {}
        names = [n for n, _ in schema] if schema else [
            idx.schema.column(i).name for i in range(len(idx.schema))]
        for n in names:
            dec = _ColumnDecoder(idx, n, device, rg_window=rg_window,
                                 snappy=snappy)
            col, _ = dec.decode()
            cols[n] = col
        per_file.append(cols)
    if len(per_file) == 1:
        return Table(per_file[0])
    return Table({n: concat_columns([pf[n] for pf in per_file])
                  for n in per_file[0]})
