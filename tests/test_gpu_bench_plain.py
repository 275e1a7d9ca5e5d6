"""A plain run of bench.py (no --full) on the GPU: the headline line and nothing else, within the time a caller who only wants that line
should wait."""
import json
import os
import subprocess
import sys
import time

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTSIDE_STEPS_S = 30.0        # whole process, start to exit, less (steps + warmup) x ms_per_step: imports, set-up, first-step work, exit


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_spends_little_outside_its_steps(tmp_path):
    steps, warmup = 5, 2
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "multi-image prefill images/sec (Leopard-LLaVA, 6x1344x896 per sample)" and d["unit"] == "images/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f16" and (d["steps"], d["warmup"], d["n_gpus"]) == (steps, warmup, 1)
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(6 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert d["full"] is False
    for extra in ("parity", "roofline", "fast_schedule", "cpu_baseline", "other_configs", "tp", "ms_per_step_excl_tiler", "ms_per_step_from_host_pixels"):
        assert extra not in d, extra
    assert sorted(os.listdir(out_dir)) == ["kv_k.npy", "kv_v.npy", "logits_last.npy"]
    outside = wall - (steps + warmup) * d["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.1f} s in all, {d['ms_per_step']:.1f} ms per step, {outside:.1f} s outside its {steps + warmup} steps")
    assert outside <= OUTSIDE_STEPS_S, (wall, d["ms_per_step"])
