"""bench.py --dump-outputs: the arrays of the last timed step as float32 / float64 .npy files,
capped at 64 MB by a seeded sample of the query rows, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_dtypes_cap_and_seeded_sample(tmp_path):
    import bench
    rng = np.random.default_rng(0)
    n = 1000
    arrays = {"p_ids": rng.integers(-1, 1 << 40, size=(n, 10)),
              "p_scores": np.where(rng.random((n, 10)) < 0.1, -np.inf, rng.standard_normal((n, 10))),
              "p_rerank": rng.standard_normal((n, 10)).astype(np.float32),
              "p_counts": rng.integers(0, 11, size=n).astype(np.int32)}
    # under the cap: every row of every array
    info = bench.dump_outputs(str(tmp_path / "whole"), arrays)
    got = _load(tmp_path / "whole")
    assert sorted(got) == sorted(arrays) == info["arrays"] and info["query_rows"] == info["of"] == n
    for k, a in arrays.items():
        assert got[k].dtype == (np.float32 if a.dtype == np.float32 else np.float64)
        assert np.array_equal(got[k], a)          # (ids below 2**53 and counts are exact in float64)
    # over the cap: the same rows of every array, the same ones in every run, within the cap
    cap = 60_000
    info = bench.dump_outputs(str(tmp_path / "a"), arrays, max_bytes=cap)
    bench.dump_outputs(str(tmp_path / "b"), arrays, max_bytes=cap)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(arrays) + ["sample_rows"]
    rows = a["sample_rows"].astype(np.int64)
    assert 0 < len(rows) == info["query_rows"] < n and np.all(np.diff(rows) > 0)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k])
        if k != "sample_rows":
            assert np.array_equal(a[k], arrays[k][rows])
    on_disk = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert cap // 2 < on_disk <= cap


@pytest.mark.gpu
def test_bench_dump_outputs_same_arrays_in_two_runs(tmp_path):
    """Two runs of bench.py with the same arguments write the same arrays: what every timed
    pipeline returned in its last timed step (seeded inputs, exact results)."""
    dirs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        out = subprocess.run(
            [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
             "--docs", "40000", "--queries", "192", "--token-docs", "20000", "--config", "all",
             "--no-extras", "--no-cpu-baseline", "--dump-outputs", d],
            cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        rec = json.loads(lines[0])
        assert rec["steps"] == 3 and rec["dumped_outputs"]["query_rows"] == 192
        dirs.append(d)
    a, b = _load(dirs[0]), _load(dirs[1])
    assert sorted(a) == sorted(b) == rec["dumped_outputs"]["arrays"]
    for cfg, channels in (("dense", ["semantic"]), ("dense_bm25", ["semantic", "lexical"]),
                          ("triple", ["semantic", "lexical", "graph"]),
                          ("triple_rerank", ["semantic", "lexical", "graph"])):
        assert a[f"{cfg}_ids"].shape == a[f"{cfg}_scores"].shape == (192, 10)
        assert a[f"{cfg}_counts"].shape == (192,) and a[f"{cfg}_counts"].max() == 10
        for ch in channels:
            assert a[f"{cfg}_{ch}_ids"].shape == a[f"{cfg}_{ch}_scores"].shape
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], b[k]), k
    # the dense channel does not depend on the pipeline around it
    assert np.array_equal(a["dense_semantic_ids"], a["triple_semantic_ids"])
    assert np.array_equal(a["dense_semantic_scores"], a["triple_semantic_scores"])
