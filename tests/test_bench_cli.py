"""bench.py command line: result line, --full, --dump-outputs (CPU, tiny scale)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, *extra):
    env = dict(os.environ, SAIL_BENCH_DATA_DIR=str(tmp_path / "shards"))
    p = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu",
         "--sf", "0.01", "--gpus", "1", "--warmup", "0", "--queries", "1,6,16", *extra],
        cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr


def test_plain_and_full_result_line_and_dump(tmp_path):
    out, err = _bench(tmp_path, "--steps", "2", "--dump-outputs", str(tmp_path / "a"))
    assert out["steps"] == 2 and out["metric"] == "tpch_sf0.01_total_s"
    assert out["unit"] == "s" and out["higher_is_better"] is False
    assert abs(out["ms_per_step"] - out["value"] * 1000) < 0.1
    assert "per_query_ms" not in out and "# q1:" not in err

    full, err = _bench(tmp_path, "--steps", "1", "--full",
                       "--dump-outputs", str(tmp_path / "b"))
    assert full["steps"] == 1
    assert sorted(full["per_query_ms"]) == ["1", "16", "6"] and "# q1:" in err
    assert {k: v for k, v in full.items() if k in ("metric", "unit", "dtype")} == \
        {k: v for k, v in out.items() if k in ("metric", "unit", "dtype")}

    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert "q01_c02_sum_qty.npy" in names and "q06_c00_revenue.npy" in names
    assert any(n.startswith("q16_c00") for n in names)      # a string column
    assert np.load(tmp_path / "a" / "q01_rows.npy").tolist() == [4.0]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and a.ndim == 1 and len(a) > 0
        assert np.array_equal(a, b, equal_nan=True), n     # same inputs, same outputs
        total += a.nbytes
    assert total < 64 << 20


def test_dump_samples_large_outputs_deterministically(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    from sail_amd.engine.chunk import Chunk
    from sail_amd.engine.column import Column
    from sail_amd.engine import types as T

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 2 * 100)  # 100 rows x 2 columns
    vals = list(range(1000))
    chunk = Chunk([Column.from_values(vals, T.I64), Column.from_values(vals, T.I64)],
                  ["k", "v"])
    bench.dump_outputs({3: chunk}, str(tmp_path / "d1"))
    bench.dump_outputs({3: chunk}, str(tmp_path / "d2"))
    k1 = np.load(tmp_path / "d1" / "q03_c00_k.npy")
    assert len(k1) == 100 and np.all(np.diff(k1) > 0)        # sampled, original order
    assert np.array_equal(k1, np.load(tmp_path / "d1" / "q03_c01_v.npy"))  # same rows
    assert np.array_equal(k1, np.load(tmp_path / "d2" / "q03_c00_k.npy"))  # fixed sample
    assert np.load(tmp_path / "d1" / "q03_rows.npy").tolist() == [1000.0]  # true count

    # a query without rows leaves its count and no empty arrays
    empty = Chunk([Column.from_values([], T.I64)], ["k"])
    bench.dump_outputs({3: chunk, 11: empty}, str(tmp_path / "d3"))
    names = sorted(os.listdir(tmp_path / "d3"))
    assert [n for n in names if n.startswith("q11")] == ["q11_rows.npy"]
    assert np.load(tmp_path / "d3" / "q11_rows.npy").tolist() == [0.0]
    assert all(np.load(tmp_path / "d3" / n).size > 0 for n in names)
