"""The gateways' own host arithmetic under AddressSanitizer + UndefinedBehaviorSanitizer, in a stand-alone program (CPU only, no
device, no Python under a sanitizer): tests/mexstub/refusals_main.cpp drives calc_pyd_cost_sgm and calc_pyd_cost_sgm_ng with
argument lists they must refuse -- among them the window half sizes whose candidate count, printed before the library sees the
values, does not fit an int."""
import os
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "mexstub")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gateway_refusals_are_asan_ubsan_clean(tmp_path):
    exe = tmp_path / "refusals_main"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", STUB, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "fsgm_amd", "mex"),
                           "-o", str(exe), os.path.join(STUB, "refusals_main.cpp"), "-x", "c", os.path.join(STUB, "mexstub.c")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "gateway refusals finished" in out.stdout and "runtime error" not in out.stderr
