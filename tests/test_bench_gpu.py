"""bench.py --gpus 1 as a fresh process: a plain run prints the headline line and nothing else, spending little time outside
its steps; --full adds the roofline object."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_KEYS = {"roofline", "configs", "end_to_end", "end_to_end_arrow", "record_shapes", "cpu_baseline", "reader_sharded"}


def _bench(args, timeout):
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True,
                         timeout=timeout)
    wall = time.perf_counter() - t0
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), wall


def test_plain_run_is_the_headline_alone(gpu, tmp_path):
    """the flagship command with few steps: the headline fields, the verified output, the dumped arrays, no side leg, and at
    most 30 s of wall clock besides the warm-up and timed steps"""
    steps, warmup = 2, 1
    j, wall = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)], 300)
    assert j["metric"] == "FASTQ records/sec into DataChunks" and j["unit"] == "records/s" and j["higher_is_better"] is True
    assert j["dtype"] == "u8" and j["steps"] == steps and j["warmup"] == warmup and j["verified"] is True
    records = j["config"]["file_bytes"] // 332
    assert abs(j["value"] - records * j["config"]["launches_per_step"] / (j["ms_per_step"] / 1e3)) < 1e-6 * j["value"]
    assert not EXTRA_KEYS & set(j), sorted(EXTRA_KEYS & set(j))
    assert sorted(os.listdir(tmp_path)) == sorted(f"{n}.npy" for n in ("rows", "result", "name", "description", "sequence",
                                                                        "quality_scores", "description_validity"))
    outside = wall - (steps + warmup) * j["ms_per_step"] / 1e3
    assert outside < 30.0, f"{outside:.1f} s outside the steps"


def test_full_adds_the_roofline(gpu):
    """--full with the file-level legs, the CPU baseline and the counter passes left out: the per-launch HIP-event times and the
    read-only stream rate of the same buffer come back in `roofline`"""
    j, _ = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--gb", "1", "--full", "--no-configs", "--no-cpu-baseline",
                   "--no-traffic"], 300)
    assert j["verified"] is True and not (EXTRA_KEYS - {"roofline"}) & set(j)
    r = j["roofline"]
    assert r["avg_launch_ms"] > 0 and r["min_launch_ms"] <= r["avg_launch_ms"] and r["read_only_stream_GBps"] > 0
    assert r["algorithmic_bytes_per_launch"] == j["config"]["bytes_per_gpu"]
