"""Persist generated tables as parquet shards and swap the catalog entries
to scan VIEWS — the shared machinery behind the scan-inclusive benchmarks
(BASELINE configs #2/#3: every timed query re-reads + GPU-decodes from
disk). Planner statistics are computed while the data is still resident
and survive the swap (the analogue of the reference's statistics cache)."""
from __future__ import annotations

import os
from typing import Dict, Optional

from ..engine.column import Table
from ..plan import spec as S


def persist_and_swap(session, tables: Dict[str, Table], *,
                     data_dir: Optional[str], default_dir: str,
                     rank: int, world: int,
                     write_fn) -> dict:
    """write_fn(tables, data_dir, rank) -> {name: path}. Tables must
    already be registered (with replication + global_rows set) so stats
    pre-warm correctly."""
    cat = session.catalog
    for name, tbl in tables.items():
        for cn in tbl.columns:
            cat.column_stats(name, cn)  # pre-warm: cached past the swap
    if world > 1 and getattr(session, "dist", None) is not None:
        from ..exec.distributed import sync_table_stats

        sync_table_stats(session)
    if data_dir is None:
        from ..utils.tmpdir import user_tmp

        data_dir = os.environ.get("SAIL_BENCH_DATA_DIR", user_tmp(default_dir))
    paths = write_fn(tables, data_dir, rank)
    total_bytes = sum(os.path.getsize(p) for p in paths.values())
    for name, tbl in tables.items():
        schema = [(n, c.dtype) for n, c in tbl.columns.items()]
        sharded = not cat.is_replicated(name)
        node = S.DataSourceRead(
            format="parquet", paths=[paths[name]],
            options={"partitioning": "sharded" if sharded else "replicated"})
        node.schema = schema
        node.__dict__["_table_name"] = name  # planner statistics key
        with cat._lock:
            k = cat._key(name)
            cat._tables.pop(k, None)
            cat._views[k] = node
    tables.clear()
    import torch as _t

    if _t.cuda.is_available():
        _t.cuda.empty_cache()
    return {"data_dir": data_dir, "bytes": total_bytes, "paths": paths}
