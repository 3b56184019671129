"""Generates tests/golden/ref_mex_calc_cost_sgm_linear.npz from the REFERENCE's own calc_cost_sgm.cpp compiled WITHOUT its line 4
(`#define USE_VZIND`): the plain 1-D matcher that fsgm_calc_cost_sgm_linear_* and fsgm_stereo_sgm_* restate.  Run where the reference
tree is present (REF in the environment; default: oracle/Makefile's), after the build (oracle/_ref/librefmex.so must exist):
    python tests/golden/make_ref_linear_golden.py
The source is read where it lies, its line 4 is dropped on the way into a temporary directory outside the repository, and that
copy is compiled with oracle/Makefile's REF_FLAGS together with the reference's common.cpp against the stand-in MEX runtime
(oracle/refmex/, linked as oracle/_ref/librefmex.so).  Nothing of it is kept: the fixture holds data only -- per case i the
inputs (c<i>_I1, c<i>_I2, c<i>_pd0, c<i>_nd, c<i>_off, the scalars dMax, vMax, P1, P2 as c<i>_args), the case's name (c<i>_id,
bytes) and the four outputs the MEX wrote (c<i>_out0..3: bestD, minC, and conf / bestD2, which stay zero because the
forward-backward check is commented out in the reference, :589-590).  `n` is the number of cases.  Every case runs twice and
must repeat itself byte for byte."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fsgm_amd import synth          # noqa: E402
from oracle import pyref            # noqa: E402
from tests import ref_cases         # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "calc_cost_sgm_linear"


def _make_var(name, op):
    """a variable of oracle/Makefile, read from it"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        return re.search(rf"^{name}\s*{re.escape(op)}\s*(.+)$", f.read(), re.M).group(1).strip()


REF = os.environ.get("REF") or _make_var("REF", "?=")          # where the reference tree lies: oracle/Makefile's default
ref_flags = lambda: _make_var("REF_FLAGS", ":=").split()       # noqa: E731


def build(tmp):
    with open(os.path.join(REF, "calc_cost_sgm.cpp")) as f:
        lines = f.readlines()
    assert lines[3].strip() == "#define USE_VZIND", f"line 4 of calc_cost_sgm.cpp is {lines[3]!r}"
    src = os.path.join(tmp, "calc_cost_sgm_no_vzind.cpp")
    with open(src, "w") as f:
        f.writelines(lines[:3] + lines[4:])
    refdir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(tmp, f"ref_{NAME}.so")
    cmd = ["g++"] + ref_flags() + ["-I" + os.path.join(ROOT, "oracle", "refmex"), "-I" + REF, src, os.path.join(REF, "common.cpp"),
                                   "-o", so, "-Wl,-Bsymbolic", "-L" + refdir, "-lrefmex", "-Wl,-rpath," + refdir]
    print(" ".join(cmd))
    subprocess.check_call(cmd)
    return so


def rect(W, H, direction):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (np.ascontiguousarray(np.stack([xx + 1.0, yy + 1.0])),
            np.ascontiguousarray(np.stack([np.full((H, W), float(direction)), np.zeros((H, W))])))


def slanted(W, H, seed):
    """fractional start positions, unit directions between -35 and +35 degrees off the x axis, either way along it"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    pd0 = np.stack([xx + 1.0, yy + 1.0]) + (synth.uniform_f64(seed, (2, H, W)) - 0.5)
    pd0[0, ::3, ::4] = np.round(pd0[0, ::3, ::4]) + 0.5                     # exact halves for round()
    ang = 0.6 * np.sin(xx / 7.0 + yy / 5.0) + np.pi * (synth.uniform_f64(seed + 1, (H, W)) < 0.3)
    return np.ascontiguousarray(pd0), np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)]))


def shifted_pair(W, H, shift, seed):
    """I2[y][x] = I1[y][x + shift]: with direction -1 the match of x lies at x - shift"""
    big = synth.uniform_u8(seed, (H, W + shift))
    I1, I2 = np.ascontiguousarray(big[:, :W]), np.ascontiguousarray(big[:, shift:])
    # the last three rows unshifted: when the LAST pixel's winner is dMax - 1 the reference's parabola reads one word past its
    # sums (calc_cost_sgm.cpp:293-296), an uninitialised value, and does not repeat itself
    I2[-3:] = I1[-3:]
    return I1, I2


def cases():
    def pair(W, H, D, seed):
        return synth.image_pair(W, H, D, seed=seed)
    c = []
    c.append(("rect-24x16x16-left", (*pair(24, 16, 16, 1), 16, *rect(24, 16, -1), 6, 64)))
    c.append(("rect-21x13x32-right", (*pair(21, 13, 32, 2), 32, *rect(21, 13, +1), 6, 32)))
    c.append(("slanted-20x14x16", (*pair(20, 14, 16, 3), 16, *slanted(20, 14, 5), 6, 64)))
    c.append(("slanted-17x11x64", (*pair(17, 11, 64, 4), 64, *slanted(17, 11, 6), 6, 64)))
    c.append(("rect-5x7x16-narrow", (*pair(5, 7, 16, 5), 16, *rect(5, 7, -1), 6, 64)))          # W < dMax: every far sample clamps
    I1, I2 = shifted_pair(40, 9, 15, 6)
    c.append(("rect-40x9x16-last-d", (I1, I2, 16, *rect(40, 9, -1), 6, 64)))                     # the winner is dMax - 1
    pd0, nd, _ = synth.epi_maps(16, 10, "general", seed=10)
    c.append(("general-16x10x20-wrap", (*pair(16, 10, 20, 7), 20, pd0, nd, 100, 200)))           # penalties that wrap mod 256
    I1, I2 = shifted_pair(150, 4, 100, 8)
    c.append(("rect-150x4x128-far-d", (I1, I2, 128, *rect(150, 4, -1), 6, 64)))                  # D = 128 with winners around 100
    c.append(("rect-1x9x16", (*pair(1, 9, 16, 9), 16, *rect(1, 9, +1), 6, 64)))
    c.append(("slanted-9x1x16", (*pair(9, 1, 16, 10), 16, *slanted(9, 1, 7), 255, 0)))
    pd0, nd, off = synth.epi_maps(20, 12, "general", seed=9)
    ref_cases.out_of_range(pd0, nd, off)                                                        # inf / NaN start positions
    pd0[0, 2, 3], pd0[1, 4, 5], pd0[0, 6, 7] = 1e12, -1e12, 2147483648.5
    c.append(("general-20x12x16-out-of-range", (*pair(20, 12, 16, 11), 16, pd0, nd, 6, 64)))
    return c


def call(so, I1, I2, D, pd0, nd, P1, P2, vMax, off):
    if NAME not in pyref._mex:                                   # pyref's caller, on the binary built here
        pyref._runtime()
        pyref._mex[NAME] = C.CDLL(so, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        pyref._mex[NAME].mexFunction.restype = None
    H, W = I1.shape
    return pyref._call(NAME, [I1, I2, D, vMax, np.ascontiguousarray(pd0), np.ascontiguousarray(nd), off, P1, P2],
                       [((H, W), np.uint32), ((H, W), np.uint32), ((H, W), np.uint8), ((H, W), np.uint32)])


def main():
    assert pyref.available("calc_cost_sgm"), "build first: oracle/_ref/librefmex.so is missing"
    arrays = {}
    with tempfile.TemporaryDirectory(prefix="fsgm_ref_linear_") as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        so = build(tmp)
        cs = cases()
        for i, (cid, (I1, I2, D, pd0, nd, P1, P2)) in enumerate(cs):
            H, W = I1.shape
            vMax = 0.3
            off = np.full((H, W), 200.0) if i % 2 else 40.0 + 400.0 * synth.uniform_f64(90 + i, (H, W))   # read, never used
            (outs, printed), (outs2, printed2) = (call(so, I1, I2, D, pd0, nd, P1, P2, vMax, off) for _ in range(2))
            assert printed == printed2
            for x, y in zip(outs, outs2):
                assert x.tobytes() == y.tobytes(), f"{cid}: the reference does not repeat itself"
            if "last-d" in cid:
                assert ((outs[0] >> 8) == D - 1).any(), f"{cid}: no pixel's winner is dMax - 1"
            if "far-d" in cid:
                assert ((outs[0] >> 8) >= 99).sum() > outs[0].size // 20 and (outs[0] & 255).any(), f"{cid}: argmin / parabola not exercised"
            ins = dict(I1=I1, I2=I2, pd0=pd0, nd=nd, off=off, args=np.array([D, vMax, P1, P2], np.float64),
                       id=np.frombuffer(cid.encode(), np.uint8))
            arrays.update({f"c{i}_{k}": np.ascontiguousarray(v) for k, v in ins.items()})
            arrays.update({f"c{i}_out{k}": v for k, v in enumerate(outs)})
        arrays["n"] = np.array(len(cs), np.int64)
    path = os.path.join(HERE, f"ref_mex_{NAME}.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote ref_mex_{NAME}.npz: {len(cs)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
