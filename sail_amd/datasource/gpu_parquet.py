"""GPU Parquet -> Arrow-in-HBM decode path (BASELINE config #2).

The reference scans parquet with arrow-rs on the CPU
(ref: crates/sail-data-source/src/formats/parquet/mod.rs, tuning surface
crates/sail-common/src/config/application.yaml:424-521). Here the decode
itself runs on the MI355X: the host reads raw column-chunk bytes (pinned
staging -> HBM), parses page headers once per file (utils/thrift_compact),
and launches batched page-table kernels (ops/csrc/parquet_decode.hip,
ops/csrc/parquet_types.hip).
Decoded columns are born as device tensors — no pyarrow on the hot path.

The chunk bytes of a column reach the device through the extension's
pipelined reader (ops/csrc/scan_reader.h, scan_reader.hip, pq_read_ranges):
a persistent pool of workers preads 16 MiB slices into a ring of 8 pinned
slots and each slice is copied on the copy stream as soon as it is complete,
so the file read and the copy of one column overlap and the pinned footprint
stays at the ring. SAIL_IO_NATIVE_READER=off, and every CPU run, takes the
Python reader instead: a thread pool fills one column-sized pinned buffer,
then one copy.

Supported: uncompressed v1 and v2 data pages (mixed freely within a
column), PLAIN fixed-width, PLAIN byte_array, RLE_DICTIONARY (+PLAIN
dictionary pages), string columns that fall back from RLE_DICTIONARY to
PLAIN pages, DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY,
BYTE_STREAM_SPLIT on INT32/INT64/FLOAT/DOUBLE, BOOLEAN (PLAIN and RLE),
INT96 timestamps (PLAIN and dictionary; decoded to int64 microseconds),
FLBA/INT32/INT64 decimals, definition levels (nulls). Anything else raises
Unsupported and the caller falls back to the host pyarrow path
(parquet_io.read): v2 pages in a compressed chunk, codecs other than
opt-in Snappy, DELTA_BYTE_ARRAY, BYTE_STREAM_SPLIT on FIXED_LEN_BYTE_ARRAY,
dictionary-encoded BOOLEAN, nested columns.

A v2 page keeps its levels outside the value region and says in its header
how long they are and how many values are null, so its layout and dense
(non-null) count are known at index time: no length prefix to read, and no
per-page count to fetch from the device.

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
A page the kernel rejects (non-zero status) raises Unsupported. Other
codecs, v2 data pages in a compressed chunk and pages of 2^31 bytes or
more stay on the host path.

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

import collections
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..engine import types as T
from ..engine.column import Column, StringColumn, Table
from ..utils import thrift_compact as tc

# parquet encoding ids
PLAIN = 0
PLAIN_DICTIONARY = 2
RLE = 3
DELTA_BINARY_PACKED = 5
DELTA_LENGTH_BYTE_ARRAY = 6
RLE_DICTIONARY = 8
BYTE_STREAM_SPLIT = 9

_JULIAN_UNIX_EPOCH = 2440588          # Julian day number of 1970-01-01
_MICROS_PER_DAY = 86_400_000_000

_MAX_PAGE = 1 << 31   # pq_snappy_decompress takes lengths below 2^31


class Unsupported(Exception):
    """Feature outside the GPU decoder; caller falls back to host decode."""


def snappy_enabled(options=None) -> bool:
    """The opt-in switch for device Snappy decompression: read option
    `gpuSnappy`, else env SAIL_IO_GPU_SNAPPY (config sail.io.gpu_snappy);
    default off."""
    if options and options.get("gpuSnappy") is not None:
        v = options["gpuSnappy"]
    else:
        v = os.environ.get("SAIL_IO_GPU_SNAPPY", "off")
    return str(v).lower() in ("on", "true", "1")


def delta_fused_enabled() -> bool:
    """SAIL_IO_GPU_DELTA_FUSED (config sail.io.gpu_delta_fused), default on:
    DELTA_BINARY_PACKED integer pages decode with one pq_delta_values launch.
    `off`, `0` or `false` selects pq_delta_decode + pq_segscan + cast. Read
    on every decode, so one process can alternate the two paths."""
    v = os.environ.get("SAIL_IO_GPU_DELTA_FUSED", "on")
    return str(v).lower() not in ("off", "false", "0")


def bytearray_fast_enabled() -> bool:
    """SAIL_IO_GPU_BYTEARRAY_FAST (config sail.io.gpu_bytearray_fast),
    default on: PLAIN byte arrays go through pq_bytearray_index +
    pq_gather_bytes. `off`, `0` or `false` selects pq_bytearray_walk +
    pq_gather_strings. Read on every decode, so one process can alternate
    the two pairs."""
    v = os.environ.get("SAIL_IO_GPU_BYTEARRAY_FAST", "on")
    return str(v).lower() not in ("off", "false", "0")


def native_reader_enabled() -> bool:
    """SAIL_IO_NATIVE_READER (config sail.io.native_reader), default on: on
    a GPU the bytes of a column's chunks go through the extension's
    pipelined reader (pq_read_ranges). `off`, `0` or `false` selects the
    Python reader with its column-sized pinned buffers. Read on every
    upload, so one process can alternate the two."""
    v = os.environ.get("SAIL_IO_NATIVE_READER", "on")
    return str(v).lower() not in ("off", "false", "0")


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


#: Cap on the bytes of cached page tables (host array plus device copy) held
#: by one process; least recently used entries go first. A 600M-row column
#: of 30,000 pages is 1.4 MB on each side.
TABLE_CACHE_CAP = 256 << 20
_TABLE_LRU: "collections.OrderedDict[tuple, tuple]" = collections.OrderedDict()
_table_bytes = 0


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
            arr = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
            self.rows[name] = arr
            if len(arr):
                self.dev[name] = torch.from_numpy(arr).to(device)
        d = self.rows["delta"]
        self.delta_total = int((d[:, 3] + d[:, 2]).max()) if len(d) else 0
        self.dict_chunks = dict_chunks
        self.nbytes = 2 * sum(a.nbytes for a in self.rows.values())


def _remember_tables(idx: "FileIndex", key, entry: _Tables):
    """Keep `entry` on its FileIndex, dropping the least recently used
    entries of the process while over TABLE_CACHE_CAP."""
    global _table_bytes
    if entry.nbytes > TABLE_CACHE_CAP:
        return
    idx._tables[key] = entry
    _TABLE_LRU[(id(idx), key)] = (idx, entry.nbytes)
    _table_bytes += entry.nbytes
    while _table_bytes > TABLE_CACHE_CAP:
        (_, old_key), (old_idx, n) = _TABLE_LRU.popitem(last=False)
        old_idx._tables.pop(old_key, None)
        _table_bytes -= n


class _Page:
    """One data page. Uncompressed: def_off/val_off are absolute file
    offsets, known at index time. Compressed: comp_off/comp_len is the
    compressed body in the file, ulen its uncompressed length, and
    def_off/val_off are relative to the start of the decompressed body;
    they, def_len, val_len, all_valid and bw0 are filled in on the first
    decode (`resolved`). `ndense` is the non-null count where the page
    header states it (v2 pages: num_values - num_nulls), else None and the
    count comes from the decoded definition levels."""

    __slots__ = ("nvals", "enc", "def_off", "def_len", "val_off", "val_len",
                 "all_valid", "bw0", "comp_off", "comp_len", "ulen",
                 "resolved", "ndense")

    def __init__(self, nvals, enc, def_off, def_len, val_off, val_len,
                 all_valid, bw0=0, comp_off=None, comp_len=0, ulen=0,
                 ndense=None):
        self.nvals = nvals
        self.ndense = ndense
        self.enc = enc
        self.def_off = def_off    # absolute file offset of RLE def runs
        self.def_len = def_len
        self.val_off = val_off    # absolute file offset of the value region
        self.val_len = val_len
        self.all_valid = all_valid
        self.bw0 = bw0            # RLE_DICTIONARY: leading bit-width byte
        self.comp_off = comp_off  # compressed page: absolute file offset
        self.comp_len = comp_len
        self.ulen = ulen
        self.resolved = comp_off is None


class _Chunk:
    __slots__ = ("start", "end", "pages", "dict_off", "dict_len", "dict_nvals",
                 "compressed", "dict_ulen")

    def __init__(self):
        self.start = 0
        self.end = 0
        self.pages: List[_Page] = []
        self.dict_off = None
        self.dict_len = 0
        self.dict_nvals = 0
        self.compressed = False   # SNAPPY: dict_off/dict_len are compressed
        self.dict_ulen = 0        # ... and this is the dictionary's length


def _check_all_valid(raw: bytes, pos: int, length: int, nvals: int) -> bool:
    """True iff the def-level region is one RLE run of value 1 covering all
    values (the common no-nulls case — skips the decode kernel)."""
    end = pos + length
    try:
        h = 0
        shift = 0
        while True:
            b = raw[pos]
            pos += 1
            h |= (b & 0x7F) << shift
            if not (b & 0x80):
                break
            shift += 7
        if h & 1:
            return False
        if (h >> 1) < nvals:
            return False
        return pos < end and raw[pos] == 1
    except IndexError:
        return False


class FileIndex:
    """Cached per-file page tables (one-time header parse — the analogue of
    the reference's parquet metadata cache, application.yaml parquet.*)."""

    def __init__(self, path: str):
        import pyarrow.parquet as pq

        self.path = path
        pf = pq.ParquetFile(path)
        self.meta = pf.metadata
        self.schema = pf.schema
        self.arrow_schema = pf.schema_arrow
        self.num_rows = self.meta.num_rows
        self._cols: Dict[str, int] = {
            self.schema.column(i).name: i for i in range(len(self.schema))}
        # keyed by (column, snappy switch): an index built with the switch
        # off must not answer for one built with it on
        self._chunks: Dict[Tuple[int, bool], List[_Chunk]] = {}
        # per (column, row-group window, snappy switch): the flat page list
        # with its totals, and the finished page tables (_Tables)
        self._windows: Dict[tuple, tuple] = {}
        self._tables: Dict[tuple, _Tables] = {}

    def column_index(self, name: str) -> int:
        if name not in self._cols:
            raise Unsupported(f"column {name} not in {self.path}")
        return self._cols[name]

    @staticmethod
    def _v2_page(name, dph, raw, start, dpos, csz, max_def) -> _Page:
        """Index one uncompressed DATA_PAGE_V2 whose body is raw[dpos:
        dpos + csz]: repetition levels, definition levels (bare RLE-hybrid
        runs, no length prefix), values; lengths and null count are in the
        header."""
        nvals = dph.get(tc.DPH2_NUM_VALUES, 0)
        nnull = dph.get(tc.DPH2_NUM_NULLS, 0)
        enc = dph.get(tc.DPH2_ENCODING, PLAIN)
        if enc == PLAIN_DICTIONARY:
            enc = RLE_DICTIONARY
        dl = dph.get(tc.DPH2_DEF_LEVELS_BYTE_LENGTH, 0)
        rl = dph.get(tc.DPH2_REP_LEVELS_BYTE_LENGTH, 0)
        if rl != 0:
            raise Unsupported(f"{name}: repetition levels in a v2 page")
        if not (0 <= nnull <= nvals and 0 <= dl <= csz):
            raise Unsupported(f"{name}: v2 page header out of range")
        if nnull and (max_def == 0 or dl == 0):
            raise Unsupported(f"{name}: v2 page with nulls but no "
                              "definition levels")
        body = dpos + dl
        val_len = csz - dl
        bw0 = raw[body] if enc == RLE_DICTIONARY and val_len > 0 else 0
        if max_def > 0:
            def_off, def_len = start + dpos, dl
        else:
            def_off, def_len = 0, 0
        return _Page(nvals, enc, def_off, def_len, start + body, val_len,
                     nnull == 0, bw0, ndense=nvals - nnull)

    def chunks(self, ci: int, snappy: Optional[bool] = None) -> List[_Chunk]:
        """Page tables of column `ci`. `snappy` accepts SNAPPY chunks
        (None: the SAIL_IO_GPU_SNAPPY environment switch)."""
        snappy = snappy_enabled() if snappy is None else bool(snappy)
        if (ci, snappy) in self._chunks:
            return self._chunks[(ci, snappy)]
        sc = self.schema.column(ci)
        if sc.max_repetition_level > 0:
            raise Unsupported(f"nested column {sc.name}")
        max_def = sc.max_definition_level
        out = []
        import mmap

        # mapped, not read: only the pages holding headers and def levels
        # are touched, not the gigabytes of values between them
        with open(self.path, "rb") as f, \
                mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm, \
                memoryview(mm) as whole:
            for rg in range(self.meta.num_row_groups):
                cmd = self.meta.row_group(rg).column(ci)
                comp = cmd.compression != "UNCOMPRESSED"
                if comp and not (snappy and cmd.compression == "SNAPPY"):
                    raise Unsupported(f"{sc.name}: compression {cmd.compression}")
                ch = _Chunk()
                ch.compressed = comp
                ch.start = (cmd.dictionary_page_offset
                            if cmd.dictionary_page_offset is not None
                            else cmd.data_page_offset)
                ch.end = ch.start + cmd.total_compressed_size
                with whole[ch.start:ch.end] as raw:
                    pos = 0
                    while pos < len(raw):
                        hdr, dpos = tc.parse_page_header(raw, pos)
                        ptype = hdr[tc.PAGE_TYPE]
                        csz = hdr[tc.COMPRESSED_SIZE]
                        usz = hdr.get(tc.UNCOMPRESSED_SIZE, csz)
                        if comp and not (0 <= csz < _MAX_PAGE
                                         and 0 <= usz < _MAX_PAGE):
                            raise Unsupported(f"{sc.name}: page of 2^31 bytes "
                                              "or more")
                        if ptype == 2:  # dictionary page
                            dph = hdr.get(tc.DICT_PAGE_HEADER, {})
                            if dph.get(tc.DICT_ENCODING, PLAIN) not in (
                                    PLAIN, PLAIN_DICTIONARY):
                                raise Unsupported(f"{sc.name}: dict page encoding")
                            ch.dict_off = ch.start + dpos
                            ch.dict_len = csz
                            ch.dict_ulen = usz
                            ch.dict_nvals = dph.get(tc.DICT_NUM_VALUES, 0)
                        elif ptype == 0:  # data page v1
                            dph = hdr.get(tc.DATA_PAGE_HEADER, {})
                            nvals = dph.get(tc.DPH_NUM_VALUES, 0)
                            enc = dph.get(tc.DPH_ENCODING, PLAIN)
                            if enc == PLAIN_DICTIONARY:
                                enc = RLE_DICTIONARY
                            body = dpos
                            if max_def > 0 and \
                                    dph.get(tc.DPH_DEF_ENCODING, RLE) != RLE:
                                raise Unsupported(f"{sc.name}: def-level encoding")
                            if comp:
                                # levels and bit width are inside the
                                # compressed body: resolved at first decode
                                ch.pages.append(
                                    _Page(nvals, enc, None, 0, None, 0, False,
                                          comp_off=ch.start + dpos,
                                          comp_len=csz, ulen=usz))
                                pos = dpos + csz
                                continue
                            if max_def > 0:
                                dl = int.from_bytes(raw[body:body + 4], "little")
                                def_off = ch.start + body + 4
                                def_len = dl
                                av = _check_all_valid(raw, body + 4, dl, nvals)
                                body += 4 + dl
                            else:
                                def_off, def_len, av = 0, 0, True
                            val_off = ch.start + body
                            val_len = csz - (body - dpos)
                            bw0 = raw[body] if (enc == RLE_DICTIONARY
                                                and body < len(raw)) else 0
                            ch.pages.append(
                                _Page(nvals, enc, def_off, def_len, val_off,
                                      val_len, av, bw0))
                        elif ptype == 3 and not comp:  # data page v2
                            ch.pages.append(self._v2_page(
                                sc.name, hdr.get(tc.DATA_PAGE_HEADER_V2, {}),
                                raw, ch.start, dpos, csz, max_def))
                        else:
                            raise Unsupported(f"{sc.name}: page type {ptype}")
                        pos = dpos + csz
                out.append(ch)
        self._chunks[(ci, snappy)] = out
        if not any(ch.compressed for ch in out):
            self._chunks[(ci, not snappy)] = out  # the switch changed nothing
        return out


_INDEX_CACHE: Dict[Tuple[str, float, int], FileIndex] = {}
#: merged device dictionaries per (file index id, column, row-group window)
#: — dictionary pages are file metadata-scale (MBs vs the GBs of codes
#: re-decoded per scan); cached like the page index
_DICT_CACHE: Dict[tuple, tuple] = {}


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
    from ..engine.column import StringColumn

    perm = _lex_perm(d_offs, d_bytes)
    n = perm.numel()
    old_to_new = torch.empty(n, dtype=torch.int64, device=perm.device)
    old_to_new.scatter_(0, perm, torch.arange(n, device=perm.device))
    col = StringColumn(d_offs, d_bytes, None, None).gather(perm)
    return col.offsets, col.bytes_, old_to_new


def file_index(path: str) -> FileIndex:
    st = os.stat(path)
    key = (os.path.abspath(path), st.st_mtime, st.st_size)
    idx = _INDEX_CACHE.get(key)
    if idx is None:
        idx = FileIndex(path)
        _INDEX_CACHE[key] = idx
        # a new or changed file: the native reader must not keep reading
        # through a descriptor of the file this path used to name
        from ..ops import kernels

        ext = kernels._ext  # only if already loaded: indexing needs no GPU
        if ext is not None and hasattr(ext, "pq_reader_invalidate"):
            ext.pq_reader_invalidate(key[0])
    return idx


# -- pinned staging ----------------------------------------------------------


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
    total = sum(e - s for s, e in ranges)
    ext = _native_reader(device)
    if ext is not None:
        offs = []
        pos = 0
        for s, e in ranges:
            offs.append(pos)
            pos += e - s
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
    offs = []
    pos = 0
    jobs = []
    for s, e in ranges:
        jobs.append((s, e, pos))
        offs.append(pos)
        pos += e - s
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


# -- decode ------------------------------------------------------------------

_ALLOW_CPU = False  # tests: run the orchestration against a kernel simulator


def _ext():
    from ..ops import kernels

    return kernels.require()


def _page_table(rows, device):
    arr = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    return torch.from_numpy(arr).to(device)


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
    """Decode a PLAIN dictionary page on the host (dict pages are small)."""
    if physical == "BYTE_ARRAY":
        vals = []
        pos = 0
        for _ in range(nvals):
            ln = int.from_bytes(raw[pos:pos + 4], "little")
            vals.append(raw[pos + 4:pos + 4 + ln])
            pos += 4 + ln
        return vals
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
        self.chunks = idx.chunks(self.ci, snappy)
        window = None if rg_window is None else tuple(rg_window)
        if rg_window is not None:
            self.chunks = self.chunks[rg_window[0]:rg_window[1]]
        # merged dictionaries belong to the row groups they were built from:
        # a window must not pick up another window's (or the whole file's)
        self._dict_key = (id(idx), self.ci, window)
        # the page list of a window never changes: flattened once per index
        self._win_key = (self.ci, window, snappy, str(device))
        meta = idx._windows.get(self._win_key)
        if meta is None:
            pages = [p for ch in self.chunks for p in ch.pages]
            meta = (pages, sum(p.nvals for p in pages), {p.enc for p in pages},
                    any(ch.compressed for ch in self.chunks))
            idx._windows[self._win_key] = meta
        self.pages, self.nrows, encs, self.compressed = meta
        if self.physical == "BOOLEAN":
            ok = {PLAIN, RLE}
        elif self.physical == "INT96":
            ok = {PLAIN, RLE_DICTIONARY}
        else:
            ok = {PLAIN, RLE_DICTIONARY, DELTA_BINARY_PACKED,
                  DELTA_LENGTH_BYTE_ARRAY}
            if self.physical in _PHYS_WIDTH:
                ok.add(BYTE_STREAM_SPLIT)
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
        # absolute file offset -> offset within self.buf
        self.rel = {id(ch): offs[i] - ch.start
                    for i, ch in enumerate(self.chunks)}
        if any(ch.compressed for ch in self.chunks):
            self._decompress()

    def _off(self, ch: _Chunk, abs_off: int) -> int:
        return abs_off + self.rel[id(ch)]

    # offsets of a page's regions within self.buf. Uncompressed: the file
    # offset moved into the upload. Compressed: the page's base in the
    # packed buffer plus the region's offset within the page.
    def _def_off(self, ch: _Chunk, p: _Page) -> int:
        if ch.compressed:
            return self.pbase[id(p)] + p.def_off
        return self._off(ch, p.def_off)

    def _val_off(self, ch: _Chunk, p: _Page) -> int:
        if ch.compressed:
            return self.pbase[id(p)] + p.val_off
        return self._off(ch, p.val_off)

    def _dict_region(self, ch: _Chunk) -> Tuple[int, int]:
        if ch.compressed:
            return self.dbase[id(ch)], ch.dict_ulen
        return self._off(ch, ch.dict_off), ch.dict_len

    def _decompress(self):
        """SNAPPY chunks: expand every page of the window (dictionary
        pages too) with one launch into a packed buffer, make that buffer
        self.buf, and resolve the page-internal layout of pages seen for
        the first time."""
        if not all(ch.compressed for ch in self.chunks):
            raise Unsupported(f"{self.sc.name}: compressed and uncompressed "
                              "row groups in one column")
        rows = []
        at = 0
        self.pbase: Dict[int, int] = {}
        self.dbase: Dict[int, int] = {}
        for ch in self.chunks:
            if ch.dict_off is not None:
                rows.append((self._off(ch, ch.dict_off), ch.dict_len,
                             ch.dict_ulen, at, 0, 0))
                self.dbase[id(ch)] = at
                at += ch.dict_ulen
            for p in ch.pages:
                rows.append((self._off(ch, p.comp_off), p.comp_len, p.ulen,
                             at, 0, 0))
                self.pbase[id(p)] = at
                at += p.ulen
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
        todo = [p for p in self.pages if not p.resolved]
        if not todo:
            return
        max_def = self.sc.max_definition_level
        bases = torch.tensor([self.pbase[id(p)] for p in todo],
                             dtype=torch.int64, device=self.device)
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
            at = torch.tensor(
                [self.pbase[id(todo[k])] + layout[k][3] for k in want],
                dtype=torch.int64, device=self.device)
            for k, b in zip(want, self.buf[at].cpu().tolist()):
                bw[k] = int(b)
        for p, (doff, dl, av, voff), b in zip(todo, layout, bw):
            p.def_off, p.def_len, p.all_valid = doff, dl, av
            p.val_off, p.val_len, p.bw0 = voff, p.ulen - voff, b
            p.resolved = True

    # -- validity ---------------------------------------------------------
    def decode_validity(self):
        """(validity u8 tensor or None, per-page dense (non-null) counts)."""
        if all(p.all_valid for p in self.pages):
            return None, [p.nvals for p in self.pages]
        rows = []
        base = 0
        for ch in self.chunks:
            for p in ch.pages:
                if p.all_valid or p.def_len == 0:
                    rows.append((0, 0, 0, base, 0, 1))  # filled below
                else:
                    rows.append((self._def_off(ch, p), p.def_len,
                                 p.nvals, base, 0, 1))
                base += p.nvals
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
        dense_base = np.cumsum([0] + dense_counts[:-1])
        classes = {"plain": [], "dict": [], "delta": [], "bss": [], "rle": []}
        plain_rows, dict_rows, delta_rows, bss_rows, rle_rows = (
            classes[k] for k in ("plain", "dict", "delta", "bss", "rle"))
        dict_chunks = []  # (chunk, page row ranges) needing dict values
        checked = self.physical in ("BOOLEAN", "INT96")
        pi = 0

        def _short(what):
            return Unsupported(f"{self.sc.name}: page {pi}: {what}")

        # the value kernels trust n_values: every region is checked against
        # it here, while the table is still on the host
        for ch in self.chunks:
            for p in ch.pages:
                b = int(dense_base[pi])
                c = dense_counts[pi]
                if p.enc == PLAIN:
                    if self.physical == "BOOLEAN" and p.val_len * 8 < c:
                        raise _short(f"{p.val_len} bytes for {c} booleans")
                    if self.physical == "INT96" and p.val_len < 12 * c:
                        raise _short(f"{p.val_len} bytes for {c} INT96 values")
                    plain_rows.append((self._val_off(ch, p), p.val_len,
                                       c, b, 0, width))
                elif p.enc == RLE_DICTIONARY:
                    bw_off = self._val_off(ch, p)
                    dict_rows.append((bw_off, p.val_len, c, b, 0, p.bw0))
                    dict_chunks.append((ch, b, c))
                elif p.enc == DELTA_BINARY_PACKED:
                    delta_rows.append((self._val_off(ch, p), p.val_len,
                                       c, b, 0, 0))
                elif p.enc == BYTE_STREAM_SPLIT:
                    checked = True
                    if p.val_len != width * c:
                        raise _short(f"{p.val_len} bytes for {c} "
                                     f"byte-stream-split values of {width}")
                    bss_rows.append((self._val_off(ch, p), p.val_len,
                                     c, b, 0, 0))
                elif p.enc == RLE:
                    checked = True
                    # RLE booleans: 4-byte length prefix, then hybrid runs
                    # of width 1. A page of nulls only has no value bytes.
                    if c == 0:
                        rle_rows.append((0, 0, 0, b, 0, 1))
                    elif p.val_len < 4:
                        raise _short(f"{p.val_len} bytes for {c} RLE booleans")
                    else:
                        rle_rows.append((self._val_off(ch, p) + 4,
                                         p.val_len - 4, c, b, 0, 1))
                pi += 1
        return _Tables(pi, sum(dense_counts), all_valid, classes, dict_chunks,
                       self.device), checked

    def _tables(self):
        """(page tables, validity) of this scan. The tables come from the
        FileIndex when they were built before; the bypasses are columns
        with compressed chunks (their bases come from the decompress step),
        columns whose dense counts need a device round trip (v1 pages with
        nulls and no count in the header) and columns with a length-checked
        class."""
        tabs = None if self.compressed else \
            self.idx._tables.get(self._win_key)
        if tabs is not None:
            _TABLE_LRU.move_to_end((id(self.idx), self._win_key))
            validity = None if tabs.all_valid else self.decode_validity()[0]
            return tabs, validity
        validity, dense_counts = self.decode_validity()
        tabs, checked = self._build_tables(dense_counts, validity is None)
        if not (self.compressed or checked) and all(
                p.all_valid or p.ndense is not None for p in self.pages):
            _remember_tables(self.idx, self._win_key, tabs)
        return tabs, validity

    def decode(self):
        self.upload()
        ext = _ext()
        dev = self.device

        if self.physical == "BYTE_ARRAY":
            validity, dense_counts = self.decode_validity()
            # per-page dense row base
            dense_base = np.cumsum([0] + dense_counts[:-1])
            col = self._decode_strings(ext, validity, dense_counts, dense_base)
            return col, validity

        # fixed-width physical types; the pages of a column may mix the
        # row classes plain, dict, delta, byte-stream-split and RLE booleans
        width, dt = self._fixed_width()
        tabs, validity = self._tables()
        n_dense, pi = tabs.n_dense, tabs.n_pages
        plain_rows, dict_rows, delta_rows, bss_rows, rle_rows = (
            tabs.rows[k] for k in ("plain", "dict", "delta", "bss", "rle"))
        dict_chunks = tabs.dict_chunks
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
                    o[r[3]:r[3] + r[2]] = vals[r[3]:r[3] + r[2]]

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
            o = _out() if dense is None or len(dict_rows) < pi else dense
            if dense is None:
                dense = o
            at = 0
            for (ch, b, c) in dict_chunks:
                dvals = self._dict_values_tensor(ch)
                o[b:b + c] = dvals.index_select(
                    0, codes[at:at + c].to(torch.int64))
                at += c

        if dense is None:
            dense = _out()
        col = self._fixed_to_column(dense, validity)
        return col, validity

    def _decode_dict_codes(self, ext, dict_rows):
        """RLE_DICTIONARY pages: first byte = bitwidth (captured at index
        time), then hybrid runs. Decodes codes densely in dict_rows order.
        Width 0 is legal (one-entry dictionary under parquet-mr/arrow-rs):
        RLE runs then carry no value bytes, so it must not be clamped."""
        rows = []
        at = 0
        for r in dict_rows:
            rows.append((r[0] + 1, r[1] - 1, r[2], at, 0, int(r[5])))
            at += r[2]
        return _ext().pq_rle_decode(self.buf, _page_table(rows, self.device), at)

    def _remap_codes(self, codes_dense, dense_counts, entry_codes,
                     entry_bases):
        """Map per-chunk dictionary codes to merged-dictionary codes in
        place (no-op for single-dictionary files)."""
        if entry_codes is None:
            return
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

    def _decode_dict_strings(self, ext, ch: _Chunk):
        """Decode a PLAIN string dictionary page on the device:
        (offsets int64[n+1], bytes u8) tensors."""
        if ch.dict_off is None:
            raise Unsupported(f"{self.sc.name}: dict-encoded page, no dict")
        d_off, d_len = self._dict_region(ch)
        rows = [(d_off, d_len, ch.dict_nvals, 0, 0, 0)]
        lengths, src_pos, status = self._index_bytearrays(
            ext, rows, ch.dict_nvals)
        return self._gather_bytearrays(ext, lengths, src_pos, status,
                                       lambda i: "dictionary page")

    def _dict_values_tensor(self, ch: _Chunk) -> torch.Tensor:
        vals = self._dict_values_host(ch)
        if isinstance(vals, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(vals))
            return t.to(self.device)
        raise Unsupported("string dict used as tensor")

    _dict_host_cache: Dict[int, object] = {}

    def _dict_values_host(self, ch: _Chunk):
        key = (id(self.idx), self.ci, ch.start)
        cache = _ColumnDecoder._dict_host_cache
        if key in cache:
            return cache[key]
        if ch.dict_off is None:
            raise Unsupported(f"{self.sc.name}: dict-encoded page, no dict")
        if ch.compressed:
            # the decompressed dictionary page is in the packed buffer
            d_off, d_len = self._dict_region(ch)
            raw = self.buf[d_off:d_off + d_len].cpu().numpy().tobytes()
        else:
            with open(self.idx.path, "rb") as f:
                f.seek(ch.dict_off)
                raw = f.read(ch.dict_len)
        vals = _decode_dict_host(raw, self.physical, ch.dict_nvals, self.flba_w)
        cache[key] = vals
        return vals

    # -- strings -----------------------------------------------------------
    def _decode_strings(self, ext, validity, dense_counts, dense_base):
        enc = self.pages[0].enc if self.pages else PLAIN
        dev = self.device
        n_dense = sum(dense_counts)
        if any(p.enc != enc for p in self.pages):
            return self._decode_mixed_strings(ext, validity, dense_counts,
                                              dense_base)
        if enc == RLE_DICTIONARY:
            dict_rows = []
            pi = 0
            for ch in self.chunks:
                for p in ch.pages:
                    dict_rows.append((self._val_off(ch, p), p.val_len,
                                      dense_counts[pi], int(dense_base[pi]),
                                      0, p.bw0))
                    pi += 1
            codes_dense = self._decode_dict_codes(ext, dict_rows)
            cached = _DICT_CACHE.get(self._dict_key)
            if cached is not None:
                # merged dictionary + per-chunk entry remaps are a pure
                # function of the FILE (like the page index): cache them
                # on device — the per-row codes (the bulk) are still
                # re-read and re-decoded on every scan
                d_offs, d_bytes, entry_codes, entry_bases = cached
                self._remap_codes(codes_dense, dense_counts, entry_codes,
                                  entry_bases)
                codes = self._scatter_codes(codes_dense, validity,
                                            dense_counts)
                return StringColumn(d_offs, d_bytes, validity, codes)
            # decode every chunk's dictionary PAGE on the device (a
            # ClickBench URL dictionary is ~1M entries per row group —
            # host loops took minutes; device walk+gather takes ms)
            dict_cols = [self._decode_dict_strings(ext, ch)
                         for ch in self.chunks]
            if len(dict_cols) == 1:
                # parquet dictionary pages are first-occurrence ordered;
                # re-sort to the engine's code-order == byte-order invariant
                o0, b0 = dict_cols[0]
                d_offs, d_bytes, old_to_new = _lex_sort_dict(o0, b0)
                entry_codes, entry_bases = old_to_new, [0]
                _DICT_CACHE[self._dict_key] = (
                    d_offs, d_bytes, entry_codes, entry_bases)
                self._remap_codes(codes_dense, dense_counts, entry_codes,
                                  entry_bases)
            else:
                # merge: exact codes over the concatenated dictionaries,
                # then remap each chunk's codes through its entry codes
                from ..engine.joins import exact_string_codes

                lens = torch.cat([o[1:] - o[:-1] for o, _ in dict_cols])
                offs = torch.zeros(lens.numel() + 1, dtype=torch.int64,
                                   device=dev)
                torch.cumsum(lens, 0, out=offs[1:])
                blob = torch.cat([b for _, b in dict_cols])
                comb = StringColumn(offs, blob, None, None)
                entry_codes = exact_string_codes([comb])[0]
                n_merged = int(entry_codes.max().item()) + 1                     if entry_codes.numel() else 0
                rep = torch.zeros(n_merged, dtype=torch.int64, device=dev)
                rep.scatter_(0, entry_codes,
                             torch.arange(entry_codes.numel(), device=dev))
                merged_col = comb.gather(rep)
                # merged codes are hash-ordered: lex-sort the merged
                # dictionary and compose the remap (invariant above)
                d_offs, d_bytes, old_to_new = _lex_sort_dict(
                    merged_col.offsets, merged_col.bytes_)
                entry_codes = old_to_new.index_select(0, entry_codes)
                entry_bases = []
                eb = 0
                for o, _b2 in dict_cols:
                    entry_bases.append(eb)
                    eb += o.numel() - 1
                _DICT_CACHE[self._dict_key] = (
                    d_offs, d_bytes, entry_codes, entry_bases)
                self._remap_codes(codes_dense, dense_counts, entry_codes,
                                  entry_bases)
            codes = self._scatter_codes(codes_dense, validity, dense_counts)
            return StringColumn(d_offs, d_bytes, validity, codes)

        if enc == DELTA_LENGTH_BYTE_ARRAY:
            rows = []
            pi = 0
            for ch in self.chunks:
                for p in ch.pages:
                    rows.append((self._val_off(ch, p), p.val_len,
                                 dense_counts[pi], int(dense_base[pi]), 0, 0))
                    pi += 1
            deltas, data_end = ext.pq_delta_decode(
                self.buf, _page_table(rows, dev), n_dense)
            total_bytes = 0
            copy_rows = []
            scan_rows = []
            ends = data_end.cpu().tolist()
            for r, de in zip(rows, ends):
                nbytes = r[1] - de
                copy_rows.append((r[0] + de, nbytes, 0, 0, total_bytes, 0))
                scan_rows.append((0, 0, r[2], r[3], total_bytes, 0))
                total_bytes += nbytes
            blob = torch.empty(total_bytes, dtype=torch.uint8, device=dev)
            ext.pq_copy_bytes(self.buf, _page_table(copy_rows, dev), blob)
            if validity is None:
                # scan 1: delta stream -> length values (per page);
                # scan 2: lengths -> offsets, page byte base folded in via
                # aux (base == sum of earlier pages' lengths, so offsets
                # are globally continuous)
                len_rows = [(0, 0, r[2], r[3], 0, 0) for r in scan_rows]
                ext.pq_segscan(deltas, _page_table(len_rows, dev))
                ext.pq_segscan(deltas, _page_table(scan_rows, dev))
                offsets = torch.zeros(n_dense + 1, dtype=torch.int64,
                                      device=dev)
                offsets[1:] = deltas
                return StringColumn(offsets, blob, None, None)
            lengths = _segmented_cumsum(deltas, dense_counts)
            offsets = torch.zeros(n_dense + 1, dtype=torch.int64, device=dev)
            torch.cumsum(lengths, 0, out=offsets[1:])
            return self._assemble_strings(offsets, blob, lengths, validity,
                                          dense_counts)

        # PLAIN byte arrays: sequential walk + parallel gather
        rows = []
        pi = 0
        for ch in self.chunks:
            for p in ch.pages:
                rows.append((self._val_off(ch, p), p.val_len,
                             dense_counts[pi], int(dense_base[pi]), 0, 0))
                pi += 1
        lengths, src_pos, status = self._index_bytearrays(ext, rows, n_dense)
        offsets, blob = self._gather_bytearrays(
            ext, lengths, src_pos, status, lambda i: f"page {i} of {len(rows)}")
        return self._assemble_strings(offsets, blob, lengths, validity,
                                      dense_counts)

    def _index_bytearrays(self, ext, rows, total):
        """PLAIN byte-array regions of self.buf -> (lengths, src_pos,
        per-region status or None): pq_bytearray_index, or
        pq_bytearray_walk (which checks nothing and has no status) when the
        switch is off or the extension lacks the new entry point."""
        table = _page_table(rows, self.device)
        if bytearray_fast_enabled() and hasattr(ext, "pq_bytearray_index"):
            lengths, src_pos, status = ext.pq_bytearray_index(
                self.buf, table, total)
            return lengths, src_pos, status
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

    def _decode_mixed_strings(self, ext, validity, dense_counts, dense_base):
        """RLE_DICTIONARY and PLAIN pages in one column (the writer's
        dictionary overflowed): every dense value becomes (length, position
        in self.buf), then one gather. The result is a plain StringColumn,
        without codes."""
        dev = self.device
        n_dense = sum(dense_counts)
        plain_rows, dict_rows = [], []
        page_chunk = []     # per dictionary-encoded page: index of its chunk
        pi = 0
        for ci, ch in enumerate(self.chunks):
            for p in ch.pages:
                row = (self._val_off(ch, p), p.val_len, dense_counts[pi],
                       int(dense_base[pi]), 0, 0)
                if p.enc == PLAIN:
                    plain_rows.append(row)
                else:
                    dict_rows.append(row[:5] + (p.bw0,))
                    page_chunk.append(ci)
                pi += 1
        # PLAIN pages write their dense rows; the rest stay (0, 0)
        lengths, src_pos, status = self._index_bytearrays(
            ext, plain_rows, n_dense)
        n_plain = len(plain_rows)
        used = sorted(set(page_chunk))   # chunks with dictionary-coded pages

        def what(i):
            if i < n_plain:
                return f"plain page {i} of {n_plain}"
            return f"dictionary page of row group {used[i - n_plain]}"

        n_codes = sum(r[2] for r in dict_rows)
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
                d_off, d_len = self._dict_region(ch)
                ent_rows.append((d_off, d_len, ch.dict_nvals, at, 0, 0))
                ent_base[ci] = at
                at += ch.dict_nvals
            ent_len, ent_src, ent_status = self._index_bytearrays(
                ext, ent_rows, at)
            # per code: its dictionary's size and base, and its dense row
            per_page = torch.tensor(
                [[self.chunks[ci].dict_nvals for ci in page_chunk],
                 [ent_base[ci] for ci in page_chunk],
                 [r[3] for r in dict_rows],
                 np.cumsum([0] + [r[2] for r in dict_rows[:-1]]).tolist()],
                dtype=torch.int64, device=dev)
            counts = torch.tensor([r[2] for r in dict_rows],
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
        return self._assemble_strings(offsets, blob, lengths, validity,
                                      dense_counts)

    def _scatter_codes(self, codes_dense, validity, dense_counts):
        if validity is None:
            return codes_dense
        full = torch.full((self.nrows,), -1, dtype=torch.int32,
                          device=self.device)
        vidx = torch.nonzero(validity, as_tuple=False).flatten()
        full[vidx] = codes_dense
        return full

    def _assemble_strings(self, offsets, blob, lengths, validity, dense_counts):
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
    out = {}
    for n in per_file[0]:
        out[n] = concat_columns([pf[n] for pf in per_file])
    return Table(out)
