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


EXTRA_SECTIONS = ("configs", "stages_alone", "other_shortlists", "latency", "parity_check")


def test_plain_run_times_the_headline_alone():
    """Without --full a run times one pipeline, the headline's (dense unless --config names
    another), at every N; all four follow only where their arrays are asked for."""
    import bench
    plain = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert plain.full is False
    assert bench.which_config(plain, 1) == bench.which_config(plain, 8) == "dense"
    full = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert full.full is True
    assert bench.which_config(full, 1) == "all" and bench.which_config(full, 8) == "dense"
    dump = bench.parse(["--dump-outputs", "d"])
    assert bench.which_config(dump, 1) == "all" and bench.which_config(dump, 8) == "dense"
    assert bench.which_config(bench.parse(["--dump-outputs", "d", "--no-extras"]), 1) == "dense"
    assert bench.which_config(bench.parse(["--full", "--no-extras"]), 1) == "dense"
    for cfg in bench.CONFIGS + ("all",):
        for more in ([], ["--full"], ["--dump-outputs", "d"]):
            assert bench.which_config(bench.parse(["--config", cfg] + more), 1) == cfg
    assert bench.which_config(bench.parse(["--preset", "configs3", "--gpus", "8"]), 8) == "triple"
    # a measurement of its own is asked for with --full, not dropped in silence
    with pytest.raises(SystemExit):
        bench.parse(["--shard-proxy", "8"])
    assert bench.parse(["--full", "--shard-proxy", "8"]).shard_proxy == 8


def _bench(args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args,
                         cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_line_is_the_headline_and_full_adds_the_rest(tmp_path):
    """A plain run prints the headline line without any section that takes runs of its own;
    --full prints the same line with all of them; both dump the same arrays of all four pipelines."""
    # (200 000 rows: below 2**17 the scan probe of the f16-inline flavour plans a larger workspace
    # than the search reserved and the library refuses it, so a --full run wants a corpus above that)
    size = ["--steps", "3", "--warmup", "1", "--docs", "200000", "--queries", "192"]
    bare = _bench(size)
    plain = _bench(size + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(size + ["--full", "--dump-outputs", str(tmp_path / "full")])
    for rec in (bare, plain, full):
        assert rec["metric"] == "queries/sec (fused top-10)" and rec["unit"] == "queries/s"
        assert rec["higher_is_better"] is True and rec["dtype"].startswith("f16 MFMA shortlist scan")
        assert rec["n_gpus"] == 1 and rec["steps"] == 3 and rec["warmup"] == 1
        assert rec["value"] > 0 and rec["ms_per_step"] > 0
        assert rec["value"] == pytest.approx(192 / (rec["ms_per_step"] * 1e-3), rel=1e-2)
        assert rec["config"]["pipeline"] == "dense" and rec["config"]["rescued_queries"] == 0
        assert rec["full"] is (rec is full)
    for rec in (bare, plain):
        assert rec["roofline"] is None and rec["cpu_baseline"] is None
        assert rec["config"]["shard_floor_proxy"] is None
    assert not set(EXTRA_SECTIONS + ("dumped_outputs",)) & set(bare)
    assert set(EXTRA_SECTIONS) & set(plain) == {"configs"}      # timed for their arrays: their rates
    assert set(plain["configs"]) == set(full["configs"]) == {"dense_bm25", "triple", "triple_rerank"}
    assert all(c["value"] > 0 and "parity_sample" not in c for c in plain["configs"].values())
    assert set(EXTRA_SECTIONS) <= set(full)
    assert full["roofline"]["launch_ms"] > 0 and full["cpu_baseline"]["value"] > 0
    assert full["parity_check"] == {"fused_top10_identical": "192/192", "recall_at_10": 1.0}
    assert all(c["parity_sample"].split()[0] in ("32/32", "8/8") for c in full["configs"].values())
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert sorted(a) == sorted(b) == plain["dumped_outputs"]["arrays"] == full["dumped_outputs"]["arrays"]
    assert {k.rsplit("_", 1)[0] for k in a} >= {"dense", "dense_bm25", "triple", "triple_rerank"}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
