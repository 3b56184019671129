"""fsgm_epi_cost_kernels (fsgm_amd.epi.cost_kernels): which kernels the cost stage launches, as far as no device is needed.
The function prints the selector the launchers themselves switch on (select_cost_kernels, epi_cost.hip); this file holds the
table it must follow, written down independently:

    dMax = 16, 32, 64, 128, 256, width < 2^22, height < 2^24, FSGM_COST_FUSED not 0   "costbox" ("stereo-costbox" rectified)
    otherwise  raw:  rectified "stereo";  dMax % 8 == 0, width < 2^22, height < 2^24 "px";  dMax % 4 == 0 "vec4";  else "scalar"
               box:  dMax % 16 == 0 and FSGM_BOX16 not 0 "box16";  dMax % 4 == 0 "box4";  else "box1"

tests/test_gpu_cost_two_kernel.py asserts these names next to every volume it compares."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from fsgm_amd import _lib
from fsgm_amd.epi import cost_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_D = (16, 32, 64, 128, 256)
SAMPLINGS = (_lib.SAMPLING_VZ, _lib.SAMPLING_LINEAR, _lib.SAMPLING_RECTIFIED)


def expected(W, H, D, sampling=_lib.SAMPLING_VZ, fused=True, box16=True):
    rect = sampling == _lib.SAMPLING_RECTIFIED
    narrow = W < (1 << 22) and H < (1 << 24)
    if fused and D in FUSED_D and narrow:
        return "stereo-costbox" if rect else "costbox"
    raw = "stereo" if rect else "px" if D % 8 == 0 and narrow else "vec4" if D % 4 == 0 else "scalar"
    box = "box16" if D % 16 == 0 and box16 else "box4" if D % 4 == 0 else "box1"
    return raw + "+" + box


@pytest.fixture
def fused_env():
    """sets FSGM_COST_FUSED for the length of a test (read at every call) and puts the caller's value back"""
    old = os.environ.get("FSGM_COST_FUSED")

    def set_(v):
        if v is None:
            os.environ.pop("FSGM_COST_FUSED", None)
        else:
            os.environ["FSGM_COST_FUSED"] = v
    yield set_
    set_(old)


def test_every_range_follows_the_divisibility_rule(fused_env):
    fused_env(None)
    names = set()
    for s in SAMPLINGS:
        for D in range(1, 1025):
            got = cost_kernels(37, 21, D, s)
            assert got == expected(37, 21, D, s), (D, s)
            names.add(got)
    assert names == {"costbox", "stereo-costbox", "px+box16", "px+box4", "vec4+box4", "scalar+box1", "stereo+box16", "stereo+box4",
                     "stereo+box1"}
    # the ranges tests/test_gpu_cost_two_kernel.py runs, spelled out
    assert [cost_kernels(7, 33, D) for D in (48, 24, 20, 7, 1024, 1020, 516, 1016)] == \
        ["px+box16", "px+box4", "vec4+box4", "scalar+box1", "px+box16", "vec4+box4", "vec4+box4", "px+box4"]
    assert [cost_kernels(7, 33, D, _lib.SAMPLING_RECTIFIED) for D in (48, 20, 7, 64)] == \
        ["stereo+box16", "stereo+box4", "stereo+box1", "stereo-costbox"]


@pytest.mark.parametrize("value,fused", [("0", False), ("0x", False), ("1", True), ("", True), ("no", True)])
def test_cost_fused_switch_is_read_at_every_call(fused_env, value, fused):
    """only a value that starts with 0 switches the fused kernel off, and the next call sees a change"""
    fused_env(value)
    for s in SAMPLINGS:
        for D in list(FUSED_D) + [8, 48, 20, 7, 512, 1024]:
            assert cost_kernels(131, 77, D, s) == expected(131, 77, D, s, fused=fused), (D, s)
    fused_env(None)
    assert cost_kernels(131, 77, 128) == "costbox"


def test_width_and_height_limits_of_the_fused_and_px_kernels(fused_env):
    """costbox_ok and the px kernel share W < 2^22 and H < 2^24 (24-bit multiplies): at the limit a fused range falls to vec4, not
    to px.  Shapes a plan accepts: fewer than 2^31 voxels."""
    fused_env(None)
    W22, H24 = 1 << 22, 1 << 24
    for D in (16, 32, 64, 128, 256):
        Hfit = (1 << 31) // (W22 * D) - 1 or 1                # rows that keep W22 x H x D below 2^31
        assert cost_kernels(W22 - 1, 1, D) == "costbox"
        assert cost_kernels(W22, 1, D) == "vec4+box16"
        assert cost_kernels(W22 - 1, Hfit, D) == "costbox"
        assert cost_kernels(W22 - 1, 1, D, _lib.SAMPLING_RECTIFIED) == "stereo-costbox"
        assert cost_kernels(W22, 1, D, _lib.SAMPLING_RECTIFIED) == "stereo+box16"
    for D in (16, 32, 64):                                    # 2^24 rows x D < 2^31 only up to 64
        assert cost_kernels(1, H24 - 1, D) == "costbox"
        assert cost_kernels(1, H24, D) == "vec4+box16"
        assert cost_kernels(1, H24, D, _lib.SAMPLING_RECTIFIED) == "stereo+box16"
    for D, box in ((8, "box4"), (24, "box4"), (48, "box16")):
        assert cost_kernels(W22 - 1, 1, D) == "px+" + box
        assert cost_kernels(W22, 1, D) == "vec4+" + box
        assert cost_kernels(1, H24 - 1, D) == "px+" + box
        assert cost_kernels(1, H24, D) == "vec4+" + box
    assert cost_kernels(W22, 1, 20) == "vec4+box4" and cost_kernels(1, H24, 7) == "scalar+box1"


def test_refused_arguments():
    """what plan creation refuses, with its status, and a buffer that cannot hold the name; buf is "" after a refusal"""
    lib = _lib.load()
    buf = C.create_string_buffer(b"untouched", 32)

    def call(W, H, D, s, b=buf, n=32):
        return lib.fsgm_epi_cost_kernels(W, H, D, s, b, n)
    for args in ((0, 5, 16, 0), (5, 0, 16, 0), (-3, 5, 16, 0), (5, 5, 0, 0), (5, 5, -16, 0), (5, 5, 16, 3), (5, 5, 16, -1)):
        buf.value = b"untouched"
        assert call(*args) == 1, args                         # FSGM_ERR_INVALID
        assert buf.value == b""
        assert lib.fsgm_last_error()
    for args in ((5, 5, 1025, 0), (5, 5, 1 << 20, 2), (1 << 16, 1 << 15, 1, 0), (1 << 11, 1 << 10, 1024, 1)):
        buf.value = b"untouched"
        assert call(*args) == 4, args                         # FSGM_ERR_UNSUPPORTED: dMax above 1024, 2^31 voxels
        assert buf.value == b""
    assert call((1 << 16) - 1, 1 << 15, 1, 0) == 0 and buf.value == b"scalar+box1"       # one column short of 2^31 voxels
    assert call(5, 5, 16, 0, None, 32) == 1
    assert call(5, 5, 16, 0, buf, 0) == 1
    small = C.create_string_buffer(b"xxxxxxxxxxxxxxx", 16)
    assert call(5, 5, 20, 0, small, len("vec4+box4")) == 1 and small.value == b""         # no room for the terminator
    assert small.raw[1:] == b"xxxxxxxxxxxxxx\x00"                                          # and nothing past the first byte written
    assert call(5, 5, 20, 0, small, len("vec4+box4") + 1) == 0 and small.value == b"vec4+box4"
    with pytest.raises(_lib.FsgmError) as e:
        cost_kernels(5, 5, 1025)
    assert e.value.status == 4


_CHILD = """
import sys
sys.path.insert(0, {root!r})
from fsgm_amd.epi import cost_kernels
print(",".join(cost_kernels(37, 21, D, s) for s in (0, 2) for D in (16, 48, 1024, 24, 20, 7)))
"""


@pytest.mark.parametrize("box16,fused", [("0", "1"), ("0", "0"), ("1", "0"), (None, None)])
def test_box16_switch_in_a_fresh_process(box16, fused):
    """FSGM_BOX16 is read once per process: its off state needs a process that starts with it"""
    env = {k: v for k, v in os.environ.items() if k not in ("FSGM_BOX16", "FSGM_COST_FUSED")}
    if box16 is not None:
        env["FSGM_BOX16"] = box16
    if fused is not None:
        env["FSGM_COST_FUSED"] = fused
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = [expected(37, 21, D, s, fused=fused != "0", box16=box16 != "0") for s in (0, 2) for D in (16, 48, 1024, 24, 20, 7)]
    assert out.stdout.strip().split(",") == want
    if box16 == "0":
        assert "px+box4" in want[:3] and "stereo+box4" in want[6:9] and not any(n.endswith("box16") for n in want)
