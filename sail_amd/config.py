"""Application configuration.

Single source of defaults + SAIL_-prefixed environment overrides — the
analogue of the reference's figment-loaded application.yaml
(ref: crates/sail-common/src/config/application.yaml, loader.rs).
"""
from __future__ import annotations

import os
from typing import Dict

DEFAULTS: Dict[str, str] = {
    # execution
    "sail.mode": "local",                       # local | spmd
    "sail.execution.device": "auto",            # auto | cpu | cuda[:N]
    "sail.execution.result_batch_rows": "65536",
    # optimizer (ref: application.yaml optimizer.*)
    "sail.optimizer.enable_join_reorder": "true",
    "sail.optimizer.join_reorder_max_relations": "12",
    "sail.optimizer.agg_mask_min_selectivity": "0.2",
    "sail.execution.checkpoint_path": "",       # df.checkpoint() root (temp dir when empty)
    "sail.execution.max_recursion": "100",      # WITH RECURSIVE iteration cap
    # distributed exchanges (SPMD over RCCL)
    "sail.exec.broadcast_threshold_bytes": str(2 << 30),  # gathered build side above this -> hash shuffle
    "sail.exec.agg_shuffle_threshold_groups": "4000000",  # est. groups above this -> shuffled aggregation
    # GROUP BY above 4096 groups and direct-address aggregation through
    # grouped_acc_global (ops/csrc/hash_agg.hip); off = torch index_add_ /
    # scatter_reduce_, one call per aggregate (env SAIL_EXEC_AGG_GLOBAL, read
    # on every aggregate)
    "sail.exec.agg_global": "on",
    # COUNT / SUM / AVG (DISTINCT x) on the device through distinct_acc
    # (ops/csrc/distinct_agg.hip): one pass over a hash set of (group, value)
    # pairs, also inside a fused aggregate list; off = two argsorts and one
    # index_add_ per output (env SAIL_EXEC_DISTINCT_HASH, read at each use)
    "sail.exec.distinct_hash": "on",
    # median / percentile / percentile_disc over a device column stay on the
    # device: radix select per group (grouped_select,
    # ops/csrc/grouped_select.hip), device sorts above its histogram budget;
    # off = the host loop (env SAIL_EXEC_PERCENTILE_SELECT, read at each use)
    "sail.exec.percentile_select": "on",
    # MIN / MAX over a ROWS or RANGE window frame of a device column by
    # window_frame_minmax (ops/csrc/window_frames.hip): wave scans per 64-row
    # block and a sparse table over blocks; off = a sparse table over rows in
    # torch (env SAIL_EXEC_WINDOW_FRAMES, read at each use)
    "sail.exec.window_frames": "on",
    # device equi-joins look each probe row up once (hj_probe_heads /
    # hj_probe_exists, ops/csrc/hash_join.hip): unique builds and
    # existence-only joins skip the count/scan/fill passes; off = chain build
    # + hj_probe_count + hj_probe_fill (env SAIL_EXEC_JOIN_FUSED, read on
    # every join)
    "sail.exec.join_fused": "on",
    # raw string columns on the device are sorted, ranked (ORDER BY, top-k,
    # MIN/MAX) and compared (<, <=, >, >=) by ops/csrc/string_sort.hip; off =
    # the host code, one Python object per row (env SAIL_EXEC_STRING_SORT,
    # read at each use)
    "sail.exec.string_sort": "on",
    # scan path: GPU parquet page decode (datasource/gpu_parquet.py)
    # auto = GPU decode when supported, host pyarrow otherwise;
    # force = raise instead of falling back (tests); off = host only
    "sail.io.gpu_parquet": "auto",
    # opt-in: decompress SNAPPY parquet pages on the GPU (ops/csrc/snappy.hip)
    # instead of sending the file to the host path; on | off
    # (env SAIL_IO_GPU_SNAPPY, read option gpuSnappy)
    "sail.io.gpu_snappy": "off",
    # PLAIN byte arrays (plain string pages, string dictionary pages) through
    # pq_bytearray_index + pq_gather_bytes (ops/csrc/parquet_bytearray.hip);
    # off = pq_bytearray_walk + pq_gather_strings (env
    # SAIL_IO_GPU_BYTEARRAY_FAST, read on every decode)
    "sail.io.gpu_bytearray_fast": "on",
    # DELTA_BYTE_ARRAY (front-coded) string columns decode on the device with
    # pq_dba_lengths + pq_dba_expand (ops/csrc/parquet_delta_bytearray.hip);
    # off = the encoding is refused and the file goes to the host path (env
    # SAIL_IO_GPU_DELTA_BYTEARRAY, read on every decode)
    "sail.io.gpu_delta_bytearray": "on",
    # column chunks reach the device through the extension's pipelined reader
    # (ops/csrc/scan_reader.h, scan_reader.hip): pread into a small ring of
    # pinned slices, each copied as it completes; off = the Python reader
    # with one column-sized pinned buffer and one copy (env
    # SAIL_IO_NATIVE_READER, read on every upload)
    "sail.io.native_reader": "on",
    # kernels
    "sail.kernels.require_on_gpu": "true",
    "sail.kernels.grouped_agg_max_lds_groups": "4096",
    # debugging (the compute-sanitizer analogue)
    "sail.debug.sync_kernels": "false",         # device sync + error check after every operator
    # tracing (ref: sail-telemetry)
    "sail.trace": "false",
    # spark-compatible session confs
    "spark.sql.session.timeZone": "UTC",
    "spark.sql.ansi.enabled": "false",
    "spark.sql.caseSensitive": "false",
    "spark.sql.shuffle.partitions": "1",
}


def load_config() -> Dict[str, str]:
    """Defaults overridden by SAIL_FOO_BAR env vars (SAIL_ prefix, _ -> .)."""
    conf = dict(DEFAULTS)
    for k, v in os.environ.items():
        if k.startswith("SAIL_") and k not in ("SAIL_TRACE",):
            key = "sail." + k[len("SAIL_"):].lower().replace("_", ".")
            conf[key] = v
    if os.environ.get("SAIL_TRACE") == "1":
        conf["sail.trace"] = "true"
    return conf
