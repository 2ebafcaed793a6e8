"""Host side of the GPU parquet scan (gpu_parquet.py): the page index of a
file, and the owner of everything cached about that file. Needs pyarrow for
the footer and utils/thrift_compact for the page headers, but no device.

_INDEX_CACHE holds one FileIndex per path. A path whose (mtime, size)
changed gets a new index, and the old one is forgotten with all it owns:
page lists, page tables, dictionaries (see FileIndex.__init__). The page
tables of all indexes together stay under TABLE_CACHE_CAP bytes, least
recently used first; that book-keeping refers to an index weakly, and no
key anywhere is the id() of an object. forget_files() drops every index
(REFRESH TABLE).

A v2 page keeps its levels outside the value region and says in its header
how long they are and how many values are null, so its layout and dense
(non-null) count are known at index time: no length prefix to read, and no
per-page count to fetch from the device. In a SNAPPY chunk the levels are
inside the compressed body: the decoder resolves them after its first
decompress and stores them on the _Page. Other codecs, v2 data pages in a
compressed chunk and pages of 2^31 bytes or more stay on the host path.
"""
from __future__ import annotations

import collections
import os
import weakref
from typing import Dict, List, NamedTuple, Optional, Tuple

from ..utils import thrift_compact as tc

# parquet encoding ids
PLAIN = 0
PLAIN_DICTIONARY = 2
RLE = 3
DELTA_BINARY_PACKED = 5
DELTA_LENGTH_BYTE_ARRAY = 6
DELTA_BYTE_ARRAY = 7
RLE_DICTIONARY = 8
BYTE_STREAM_SPLIT = 9

_MAX_PAGE = 1 << 31   # pq_snappy_decompress takes lengths below 2^31


class Unsupported(Exception):
    """Feature outside the GPU decoder; caller falls back to host decode."""


def _switch(env: str, default: bool, value=None) -> bool:
    """An on/off switch: `value` when given, else the environment variable,
    else the default. Only a spelling of the other side flips a default."""
    v = os.environ.get(env) if value is None else value
    if v is None:
        return default
    v = str(v).lower()
    return v not in ("off", "false", "0") if default else \
        v in ("on", "true", "1")


def snappy_enabled(options=None) -> bool:
    """The opt-in switch for device Snappy decompression: read option
    `gpuSnappy`, else env SAIL_IO_GPU_SNAPPY (config sail.io.gpu_snappy);
    default off."""
    return _switch("SAIL_IO_GPU_SNAPPY", False,
                   options.get("gpuSnappy") if options else None)


def delta_fused_enabled() -> bool:
    """SAIL_IO_GPU_DELTA_FUSED (config sail.io.gpu_delta_fused), default on:
    DELTA_BINARY_PACKED integer pages decode with one pq_delta_values launch.
    `off`, `0` or `false` selects pq_delta_decode + pq_segscan + cast. Read
    on every decode, so one process can alternate the two paths."""
    return _switch("SAIL_IO_GPU_DELTA_FUSED", True)


def bytearray_fast_enabled() -> bool:
    """SAIL_IO_GPU_BYTEARRAY_FAST (config sail.io.gpu_bytearray_fast),
    default on: PLAIN byte arrays go through pq_bytearray_index +
    pq_gather_bytes. `off`, `0` or `false` selects pq_bytearray_walk +
    pq_gather_strings. Read on every decode, so one process can alternate
    the two pairs."""
    return _switch("SAIL_IO_GPU_BYTEARRAY_FAST", True)


def delta_bytearray_enabled() -> bool:
    """SAIL_IO_GPU_DELTA_BYTEARRAY (config sail.io.gpu_delta_bytearray),
    default on: DELTA_BYTE_ARRAY string columns decode on the device with
    pq_dba_lengths + pq_dba_expand. `off`, `0` or `false` refuses the
    encoding, so such a column goes to the host path. Read on every decode,
    so one process can alternate the two."""
    return _switch("SAIL_IO_GPU_DELTA_BYTEARRAY", True)


def native_reader_enabled() -> bool:
    """SAIL_IO_NATIVE_READER (config sail.io.native_reader), default on: on
    a GPU the bytes of a column's chunks go through the extension's
    pipelined reader (pq_read_ranges). `off`, `0` or `false` selects the
    Python reader with its column-sized pinned buffers. Read on every
    upload, so one process can alternate the two."""
    return _switch("SAIL_IO_NATIVE_READER", True)


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


class _Window(NamedTuple):
    """The chunks of one column inside a row-group window, their pages
    flattened in page order, and what the decoder asks of all of them."""
    chunks: List[_Chunk]
    pages: List[_Page]
    nrows: int
    encs: set
    compressed: bool


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


#: Cap on the bytes of cached page tables (host array plus device copy) held
#: by one process; least recently used entries go first. A 600M-row column
#: of 30,000 pages is 1.4 MB on each side.
TABLE_CACHE_CAP = 256 << 20
# every remembered table of the process, least recently used first, with a
# weak reference to the index that holds it and its key there
_TABLE_LRU: "collections.OrderedDict[object, tuple]" = \
    collections.OrderedDict()
_table_bytes = 0


def cached_table_bytes() -> int:
    """Bytes of page tables the process remembers at the moment."""
    return _table_bytes


class FileIndex:
    """Cached per-file page tables (one-time header parse — the analogue of
    the reference's parquet metadata cache, application.yaml parquet.*),
    and the owner of everything else cached about the file."""

    def __init__(self, path: str, stamp=None):
        import pyarrow.parquet as pq

        self.path = path
        self.stamp = stamp        # (mtime, size) of the generation indexed
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
        # with its totals; with the device added, the finished page tables
        # (entries with .nbytes, see remember_tables)
        self._windows: Dict[tuple, _Window] = {}
        self._tables: Dict[tuple, object] = {}
        # per (column, row-group window): the merged device dictionary of a
        # string column. It belongs to the row groups it was built from: a
        # window must not pick up another window's (or the whole file's)
        self._dicts: Dict[tuple, tuple] = {}
        # per (column, chunk start): host values of a fixed-width dictionary
        self._dict_host: Dict[Tuple[int, int], object] = {}

    def column_index(self, name: str) -> int:
        if name not in self._cols:
            raise Unsupported(f"column {name} not in {self.path}")
        return self._cols[name]

    def window(self, ci: int, rg_window, snappy: bool) -> _Window:
        """Column `ci` restricted to row groups [lo, hi) (None: all). The
        page list of a window never changes: flattened once per index."""
        key = (ci, rg_window, snappy)
        win = self._windows.get(key)
        if win is None:
            chunks = self.chunks(ci, snappy)
            if rg_window is not None:
                chunks = chunks[rg_window[0]:rg_window[1]]
            pages = [p for ch in chunks for p in ch.pages]
            win = self._windows[key] = _Window(
                chunks, pages, sum(p.nvals for p in pages),
                {p.enc for p in pages},
                any(ch.compressed for ch in chunks))
        return win

    def tables(self, key):
        """The page tables remembered under `key`, now the most recently
        used of the process; None when there are none."""
        entry = self._tables.get(key)
        if entry is not None:
            _TABLE_LRU.move_to_end(entry)
        return entry

    def remember_tables(self, key, entry):
        """Keep `entry` (anything with .nbytes) under `key`, dropping the
        least recently used entries of the process while over
        TABLE_CACHE_CAP."""
        global _table_bytes
        if entry.nbytes > TABLE_CACHE_CAP:
            return
        self._tables[key] = entry
        _TABLE_LRU[entry] = (weakref.ref(self), key)
        _table_bytes += entry.nbytes
        while _table_bytes > TABLE_CACHE_CAP:
            old, (owner, old_key) = _TABLE_LRU.popitem(last=False)
            _table_bytes -= old.nbytes
            idx = owner()
            if idx is not None:
                del idx._tables[old_key]

    def forget(self):
        """Drop everything remembered from decoding this file, and its share
        of the cached-table bytes; the parsed page headers stay."""
        global _table_bytes
        for entry in self._tables.values():
            del _TABLE_LRU[entry]
            _table_bytes -= entry.nbytes
        for cache in (self._tables, self._windows, self._dicts,
                      self._dict_host):
            cache.clear()

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


# one index per absolute path, of the file generation `stamp` names
_INDEX_CACHE: Dict[str, FileIndex] = {}


def file_index(path: str) -> FileIndex:
    st = os.stat(path)
    key = os.path.abspath(path)
    stamp = (st.st_mtime, st.st_size)
    idx = _INDEX_CACHE.get(key)
    if idx is None or idx.stamp != stamp:
        if idx is not None:
            idx.forget()
        idx = _INDEX_CACHE[key] = FileIndex(path, stamp)
        # a new or changed file: the native reader must not keep reading
        # through a descriptor of the file this path used to name
        from ..ops import kernels

        ext = kernels._ext  # only if already loaded: indexing needs no GPU
        if ext is not None and hasattr(ext, "pq_reader_invalidate"):
            ext.pq_reader_invalidate(key)
    return idx


def forget_files():
    """Drop every file index with all it owns, and the table book-keeping:
    the next scan of any file parses and builds everything anew."""
    global _table_bytes
    for idx in _INDEX_CACHE.values():
        idx.forget()
    _INDEX_CACHE.clear()
    _TABLE_LRU.clear()
    _table_bytes = 0
