"""bench.py's command line: a plain run prints the headline line and nothing that takes runs of its own; --full adds
the self-check and the roofline block.  The GPU cases run the benchmark itself (that is what they test) on the
smallest batch that takes a fused pipeline: 2 frames, one warm-up step, one timed step."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config", "argv")
FULL_ONLY = ("roofline", "checked", "check", "cpu_baseline", "cpu_baseline_all_cores", "whole_mex", "whole_mex_radial_directions",
             "whole_mex_random_directions", "host_call_ms")


def _bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def test_help_names_full_and_needs_no_device():
    out = _bench("--help")
    assert "--full" in out and "--dump-outputs" in out


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_only(gpu_lib):
    lines = [l for l in _bench("--gpus", "1", "--steps", "1", "--warmup", "1", "--frames-per-gpu", "2").splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert all(k in d for k in HEADLINE), sorted(d)
    assert not any(k in d for k in FULL_ONLY), sorted(d)
    assert d["full"] is False and d["unit"] == "voxel-paths/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["steps"] == 1 and d["warmup"] == 1 and d["config"]["frames_per_gpu"] == 2
    assert d["ms_per_step"] > 0
    # value is the step's voxel-paths over its time: 2 frames x 1242 x 375 x 128 x 8 paths
    assert d["value"] == pytest.approx(2 * 1242 * 375 * 128 * 8 / (d["ms_per_step"] * 1e-3), rel=1e-9)


@pytest.mark.gpu
def test_full_run_adds_the_self_check_and_the_roofline(gpu_lib):
    d = json.loads([l for l in _bench("--gpus", "1", "--steps", "1", "--warmup", "1", "--frames-per-gpu", "2", "--full",
                                      "--no-extras", "--no-cpu-baseline").splitlines() if l.startswith("{")][-1])
    assert all(k in d for k in HEADLINE), sorted(d)
    assert d["full"] is True and d["checked"] is True
    assert d["roofline"]["stage_ms"] > 0 and d["roofline"]["copy_GBps_measured"] > 0
    assert d["unit"] == "voxel-paths/s" and d["dtype"] == "u8" and d["config"]["frames_per_gpu"] == 2
    # --no-extras and --no-cpu-baseline still take their legs out of a full run
    assert not any(k in d for k in ("cpu_baseline", "cpu_baseline_all_cores", "whole_mex", "host_call_ms"))
