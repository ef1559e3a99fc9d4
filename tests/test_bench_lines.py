"""bench.py --gpus 1: a plain run measures only what its headline figure needs; --full adds the one-at-a-time passes and the
per-stage breakdown (and, unless switched off, -s, the other workloads, the CLI end to end and the CPU baseline)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--workload", "hprc-wg", "--scale", "0.002", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest():
    plain = _bench()
    full = _bench("--full", "--no-secondary", "--no-cpu-baseline")
    for line in (plain, full):
        assert line["metric"] == "edges/sec decomposed (flubble+PVST)" and line["unit"] == "edges/s"
        assert line["higher_is_better"] is True and line["dtype"] == "u32"
        assert line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1
        assert line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(line["config"]["links"] * 1e3 / line["ms_per_step"])
        assert line["roofline"]["ms_per_launch"] > 0 and line["roofline"]["pass_latency_ms"] > 0
        for k in ("secondary", "subflubbles", "end_to_end", "cpu_baseline"):
            assert k not in line, k
    assert plain["config"] == full["config"]
    for k in ("stage_ms", "ms_per_step_one_pass_at_a_time"):
        assert k not in plain and k in full, k
    for k in ("dominant_stage", "ms_per_launch_one_pass_at_a_time"):
        assert k not in plain["roofline"] and k in full["roofline"], k
    assert full["stage_ms"]["total"] > 0 and len(full["stage_ms"]) > 1
    assert full["roofline"]["dominant_stage"]["name"] in full["stage_ms"]
    assert full["ms_per_step_one_pass_at_a_time"] > 0
