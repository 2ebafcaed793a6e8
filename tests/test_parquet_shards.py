"""The threaded shard writer must produce exactly the file a single
sequential pyarrow ParquetWriter produces from the same row groups."""
import os

import pyarrow.parquet as pq
import pytest

from sail_amd.datagen.tpch import TpchGenerator, write_tpch_parquet
from sail_amd.datasource.arrow_io import chunk_to_arrow
from sail_amd.engine import types as T
from sail_amd.engine.chunk import Chunk
from sail_amd.engine.column import StringColumn
from sail_amd.utils import thrift_compact as tc

RG = 1000  # not a divisor of any table's row count -> ragged last row group
PAGE = 1 << 12


@pytest.fixture(scope="module")
def tables():
    return TpchGenerator(sf=0.002, device="cpu", full=True).generate_all()


def _sequential(tbl, path):
    """The single-writer loop the shard writer replaces."""
    schema = [(n, c.dtype) for n, c in tbl.columns.items()]
    use_dict, col_enc = [], {}
    for n, c in tbl.columns.items():
        if isinstance(c, StringColumn):
            if c.is_dict:
                use_dict.append(n)
            else:
                col_enc[n] = "DELTA_LENGTH_BYTE_ARRAY"
        elif c.dtype.is_integer or isinstance(
                c.dtype, (T.DateType, T.TimestampType, T.DecimalType)):
            col_enc[n] = "DELTA_BINARY_PACKED"
    n = tbl.num_rows
    writer = None
    for lo in range(0, max(n, 1), RG):
        ln = min(RG, n - lo)
        sub = Chunk([c.slice(lo, ln) for c in tbl.columns.values()], list(tbl.columns))
        at = chunk_to_arrow(sub, schema)
        if writer is None:
            writer = pq.ParquetWriter(
                path, at.schema, compression="NONE",
                use_dictionary=use_dict or False,
                column_encoding=col_enc or None, data_page_size=PAGE,
                store_decimal_as_integer=True,
                dictionary_pagesize_limit=64 << 20, data_page_version="1.0")
        writer.write_table(at, row_group_size=RG)
    writer.close()


@pytest.mark.parametrize("threads", ["1", "5"])
def test_shards_byte_identical_to_sequential_writer(tables, tmp_path, monkeypatch, threads):
    monkeypatch.setenv("SAIL_IO_WRITE_THREADS", threads)
    paths = write_tpch_parquet(dict(tables), str(tmp_path / "par"),
                               row_group_rows=RG, page_size=PAGE)
    assert set(paths) == set(tables)
    for name, tbl in tables.items():
        ref = str(tmp_path / f"{name}.seq.parquet")
        _sequential(tbl, ref)
        with open(ref, "rb") as f, open(paths[name], "rb") as g:
            assert f.read() == g.read(), name
        md = pq.ParquetFile(paths[name]).metadata
        assert md.num_rows == tbl.num_rows
        assert md.num_row_groups == max(1, -(-tbl.num_rows // RG))
        with open(paths[name] + ".ok") as f:
            assert f.read().strip() == str(tbl.num_rows)


def test_shards_are_reused(tables, tmp_path):
    small = {"nation": tables["nation"]}
    paths = write_tpch_parquet(dict(small), str(tmp_path), row_group_rows=RG)
    before = os.stat(paths["nation"]).st_mtime_ns
    write_tpch_parquet(dict(small), str(tmp_path), row_group_rows=RG)
    assert os.stat(paths["nation"]).st_mtime_ns == before


def test_thrift_tree_roundtrip_is_lossless(tables, tmp_path):
    paths = write_tpch_parquet({"orders": tables["orders"]}, str(tmp_path),
                               row_group_rows=RG, page_size=PAGE)
    with open(paths["orders"], "rb") as f:
        raw = f.read()
    flen = int.from_bytes(raw[-8:-4], "little")
    footer = raw[-8 - flen:-8]
    tree, end = tc.read_tree(footer, 0)
    assert end == len(footer)
    assert bytes(tc.write_tree(tree)) == footer
