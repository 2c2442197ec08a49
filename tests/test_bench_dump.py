"""`bench.py --dump-outputs DIR`: what the last timed step computed, as float32 / float64 .npy files within a 64 MB budget, the same
from run to run under the same arguments (so that two builds compare output for output); `--steps` sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env)
    return out


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_sample_is_fixed_and_within_budget(tmp_path):
    import bench
    assert np.array_equal(bench.sample_rows(100, 8, 10_000, 1), np.arange(100))              # fits: every row
    a, b = bench.sample_rows(10_000, 72_008, 256 * 72_008, 7), bench.sample_rows(10_000, 72_008, 256 * 72_008, 7)
    assert len(a) == 256 and np.array_equal(a, b) and np.all(np.diff(a) > 0) and a[-1] < 10_000
    assert not np.array_equal(a, bench.sample_rows(10_000, 72_008, 256 * 72_008, 8))
    m = bench.dump_outputs(str(tmp_path), {"x": np.arange(6, dtype=np.float32).reshape(2, 3), "y": np.ones(4)})
    assert m["bytes"] == 24 + 32 and m["arrays"]["x"] == {"shape": [2, 3], "dtype": "float32"}
    z = _load(str(tmp_path))
    assert z["x"].dtype == np.float32 and np.array_equal(z["x"], np.arange(6, dtype=np.float32).reshape(2, 3)) and z["y"].dtype == np.float64
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), {"ids": np.ones(4, np.int64)})                   # float32 / float64 only
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), {"big": np.zeros(bench.DUMP_BUDGET // 8 + 1)})   # 64 MB in all


def test_bench_refuses_zero_steps_and_untimed_dumps():
    assert _bench(["--steps", "0"], timeout=120).returncode == 2
    assert _bench(["--workload", "c5dist", "--dump-outputs", "x"], timeout=120).returncode == 2


SMALL_REQUEST = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--db-genomes", "20000", "--genome-len", "1000000", "--queries", "2048",
                 "--queries-per-step", "1024", "--no-extra-legs", "--no-cpu-baseline"]


@pytest.mark.gpu
def test_bench_request_dump_is_the_last_step_and_repeatable(tmp_path):
    runs = []
    for rep in range(2):
        d = str(tmp_path / ("run%d" % rep))
        out = _bench(SMALL_REQUEST + ["--dump-outputs", d])
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout[-3000:]
        r = json.loads(lines[0])
        assert r["steps"] == 3 and len(r["step_ms"]) == 3 and r["ms_per_step"] > 0
        assert r["dumped_outputs"]["dir"] == d and r["dumped_outputs"]["bytes"] <= 64 << 20
        runs.append(_load(d))
    a, b = runs
    assert sorted(a) == ["answer_rows", "counts", "dist_evals", "distances", "ids", "query_signatures", "query_signatures_rows"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)              # same arguments, same outputs
    assert a["ids"].shape == (1024, 50) and a["distances"].shape == (1024, 50) and np.array_equal(a["answer_rows"], np.arange(1024))
    assert a["query_signatures"].shape == (256, 18000) and len(np.unique(a["query_signatures_rows"])) == 256
    cnt = a["counts"].astype(int)
    assert np.all((cnt >= 1) & (cnt <= 50)) and np.all(a["dist_evals"] >= cnt)
    for i in range(0, 1024, 97):
        c = cnt[i]
        assert np.all(np.diff(a["distances"][i, :c]) >= 0) and np.all(a["ids"][i, :c] < 20000)


@pytest.mark.gpu
def test_bench_sketch_dump_holds_the_signatures(tmp_path):
    d = str(tmp_path / "sk")
    out = _bench(["--gpus", "1", "--workload", "sketch", "--steps", "2", "--warmup", "1", "--genomes", "64", "--genome-len", "1000000",
                  "--full", "--no-cpu-baseline", "--dump-outputs", d])
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["parity_checked"]["bit_exact_vs_oracle"]
    z = _load(d)
    assert z["signatures"].dtype == np.float32 and z["signatures"].shape == (64, 18000) and np.array_equal(z["signatures_rows"], np.arange(64))
    assert np.all(np.isfinite(z["signatures"]))


@pytest.mark.gpu
def test_bench_plain_run_leaves_the_checks_to_full(tmp_path):
    """a plain run times the steps and dumps them, nothing else: the oracle parity sample, the CPU baseline, the gather-mode roofline and the
    side legs run with --full only, after the same timed steps (same dumped outputs)"""
    small = [a for a in SMALL_REQUEST if a not in ("--no-extra-legs", "--no-cpu-baseline")]
    res = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-extra-legs"])):
        d = str(tmp_path / mode)
        out = _bench(small + extra + ["--dump-outputs", d])
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout[-3000:]
        res[mode] = (json.loads(lines[0]), _load(d))
    (p, pz), (f, fz) = res["plain"], res["full"]
    for r in (p, f):
        assert r["metric"] == "query genomes/sec" and r["unit"] == "genomes/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
        assert r["steps"] == 3 and len(r["step_ms"]) == 3 and r["ms_per_step"] > 0 and r["value"] > 0 and r["kernels"]
    assert p["cpu_baseline"] is None
    assert not any(k in p for k in ("parity_checked", "roofline_gather_mode", "request_redundant", "extra_legs", "request_skewed"))
    assert f["cpu_baseline"]["value"] > 0 and f["roofline_gather_mode"]["same_answers_as_dense"]
    pc = f["parity_checked"]
    assert pc["sketch_bit_exact_vs_oracle"] and pc["neighbour_ids_and_distances_equal_oracle"] and pc["dist_evaluation_counts_equal_oracle"]
    assert sorted(pz) == sorted(fz) and all(np.array_equal(pz[k], fz[k]) for k in pz)
