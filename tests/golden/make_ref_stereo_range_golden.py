"""Generates tests/golden/ref_mex_stereo_range.npz from the REFERENCE's own calc_cost_sgm.cpp compiled without its line 4
(`#define USE_VZIND`) on the maps of a rectified pair whose search range starts at d_min:
    Pd0 = (x + 1 + direction * d_min, y + 1),  normDir = (direction, 0)
so that its index d samples clamp(x + direction * (d_min + d), 0, W - 1) (:368-375) -- what fsgm_stereo_sgm_*_range and
fsgm_epi_plan_set_d_min restate.  Run where the reference tree is present (REF in the environment; default: oracle/Makefile's),
after the build (oracle/_ref/librefmex.so must exist), never on the GPU machine:
    python tests/golden/make_ref_stereo_range_golden.py
Written like make_ref_adaptive_golden.py: the source is read where it lies, the lines are asserted to read as expected and changed
on the way into a temporary directory outside the repository -- line 4 dropped, line 104 (`enableDiagnalPath`) set for 8 paths,
the comment marks of the call of forward_backward_check (:589-590) removed for the builds with the check -- and each copy is
compiled with oracle/Makefile's REF_FLAGS together with the reference's common.cpp against the stand-in MEX runtime.  Nothing of
it is kept: the fixture holds data only -- per frame j the images (f<j>_I1, f<j>_I2) and its name (f<j>_id, bytes); per case i
c<i>_args = [frame, dMax, direction, d_min, P1, P2, paths, fb] and the four outputs the MEX wrote (c<i>_out0..3: bestD, minC,
conf, bestD2 -- candidate indices * 256, 512 << 8 for an invalid bestD2; conf / bestD2 stay zero in the builds without the
check).  The maps are not stored: tests/stereo_range_restatement.shifted_maps rebuilds them.  `n` cases, `nf` frames.  Every
case runs twice and must repeat itself byte for byte."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fsgm_amd import synth                           # noqa: E402
from oracle import pyref                             # noqa: E402
from tests import stereo_range_restatement as SR     # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ref_linear_golden as lin                 # noqa: E402  (REF, REF_FLAGS)

NAME = "stereo_range"
VARIANTS = ((4, 0), (8, 0), (4, 1), (8, 1))          # (paths, fb)


def build(tmp, variant):
    paths, fb = variant
    with open(os.path.join(lin.REF, "calc_cost_sgm.cpp")) as f:
        lines = f.readlines()
    assert lines[3].strip() == "#define USE_VZIND", f"line 4 of calc_cost_sgm.cpp is {lines[3]!r}"
    assert lines[103].strip() == "const bool enableDiagnalPath = false;", f"line 104 of calc_cost_sgm.cpp is {lines[103]!r}"
    assert lines[588].strip() == "//forward_backward_check(conf, bestD2, bestD, width, height,", f"line 589 of calc_cost_sgm.cpp is {lines[588]!r}"
    assert lines[589].strip() == "//    pixelPosD0, normlizeDirection, offsetFromPosD0, vMax, dMax + 1);", f"line 590 of calc_cost_sgm.cpp is {lines[589]!r}"
    if paths == 8:
        lines[103] = lines[103].replace("false", "true")
    if fb:
        lines[588] = lines[588].replace("//", "", 1)
        lines[589] = lines[589].replace("//", "", 1)
    del lines[3]
    tag = f"lin{paths}{'fb' if fb else ''}"
    src = os.path.join(tmp, f"calc_cost_sgm_{tag}.cpp")
    with open(src, "w") as f:
        f.writelines(lines)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    so = os.path.join(tmp, f"ref_{NAME}_{tag}.so")
    cmd = ["g++"] + lin.ref_flags() + ["-I" + os.path.join(ROOT, "oracle", "refmex"), "-I" + lin.REF, src, os.path.join(lin.REF, "common.cpp"),
                                       "-o", so, "-Wl,-Bsymbolic", "-L" + refdir, "-lrefmex", "-Wl,-rpath," + refdir]
    print(" ".join(cmd))
    subprocess.check_call(cmd)
    return tag, so


def frames():
    """(name, I1, I2, cases), a case (dMax, direction, d_min, paths, fb).  One texture with a smooth disparity field in [0, 8)
    and two pairs with one true disparity that only a shifted range reaches: -20 (direction -1) and +45 (direction +1)."""
    f = []
    f.append(("smooth-37x11", *synth.image_pair(37, 11, 16, seed=3),
              ((16, -1, -70, 4, 0), (16, +1, -1, 8, 1), (48, -1, 1, 4, 1), (64, +1, 7, 8, 0), (48, +1, 40, 4, 0), (64, -1, -1, 8, 1),
               (16, +1, -70, 4, 1), (16, -1, 1, 8, 0))))
    f.append(("shift-20-61x9", *SR.shifted_pair(61, 9, -20, -1, 21),
              ((64, -1, -70, 4, 1), (64, -1, -70, 8, 0), (48, -1, -1, 4, 0), (16, -1, 7, 8, 1))))
    f.append(("shift+45-64x8", *SR.shifted_pair(64, 8, 45, +1, 22),
              ((16, +1, 40, 4, 1), (48, +1, 40, 8, 1), (64, +1, 7, 4, 0), (64, +1, 40, 8, 0), (16, +1, 1, 4, 0))))
    return f


def call(tag, so, I1, I2, D, pd0, nd, P1, P2):
    key = f"{NAME}_{tag}"
    if key not in pyref._mex:                                    # pyref's caller, on the binaries built here
        pyref._runtime()
        pyref._mex[key] = C.CDLL(so, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        pyref._mex[key].mexFunction.restype = None
    H, W = I1.shape
    off = np.full((H, W), 200.0)                                 # read, never used
    return pyref._call(key, [I1, I2, D, 0.3, np.ascontiguousarray(pd0), np.ascontiguousarray(nd), off, P1, P2],
                       [((H, W), np.uint32), ((H, W), np.uint32), ((H, W), np.uint8), ((H, W), np.uint32)])


def main():
    assert pyref.available("calc_cost_sgm"), "build first: oracle/_ref/librefmex.so is missing"
    arrays, n, P1, P2 = {}, 0, 6, 64
    seen, fb_seen = set(), set()
    with tempfile.TemporaryDirectory(prefix="fsgm_ref_stereo_range_") as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        sos = {v: build(tmp, v) for v in VARIANTS}
        fs = frames()
        for j, (fid, I1, I2, cases) in enumerate(fs):
            H, W = I1.shape
            arrays[f"f{j}_I1"], arrays[f"f{j}_I2"] = np.ascontiguousarray(I1), np.ascontiguousarray(I2)
            arrays[f"f{j}_id"] = np.frombuffer(fid.encode(), np.uint8)
            for D, direction, d_min, paths, fb in cases:
                pd0, nd = SR.shifted_maps(W, H, direction, d_min)
                (outs, printed), (outs2, printed2) = (call(*sos[(paths, fb)], I1, I2, D, pd0, nd, P1, P2) for _ in range(2))
                assert printed == printed2
                for x, y in zip(outs, outs2):
                    assert x.tobytes() == y.tobytes(), f"{fid} {(D, direction, d_min, paths, fb)}: the reference does not repeat itself"
                # (a last pixel whose winner is dMax - 1 makes the reference's parabola read one word past its sums, :293-296)
                assert (int(outs[0][-1, -1]) >> 8) != D - 1, f"{fid} {(D, direction, d_min, paths, fb)}: the last pixel's winner is dMax - 1"
                if fb:
                    fb_seen |= {("conf", int(v)) for v in np.unique(outs[2])} | {("invalid", bool(v)) for v in np.unique(outs[3] == 512 << 8)}
                else:
                    assert not outs[2].any() and not outs[3].any()
                arrays[f"c{n}_args"] = np.array([j, D, direction, d_min, P1, P2, paths, fb], np.int64)
                arrays.update({f"c{n}_out{k}": o for k, o in enumerate(outs)})
                seen.add((direction, d_min, D, paths, fb))
                n += 1
        arrays["n"], arrays["nf"] = np.array(n, np.int64), np.array(len(fs), np.int64)
    assert fb_seen == {("conf", 0), ("conf", 1), ("invalid", False), ("invalid", True)}, f"the check is not exercised: {fb_seen}"
    for k, want in enumerate(({-1, 1}, {-70, -1, 1, 7, 40}, {16, 48, 64}, {4, 8}, {0, 1})):
        assert {s[k] for s in seen} == want, (k, want)
    path = os.path.join(HERE, f"ref_mex_{NAME}.npz")
    np.savez_compressed(path, **arrays)
    size, cap = os.path.getsize(path), max(os.path.getsize(os.path.join(HERE, p)) for p in os.listdir(HERE) if p.startswith("ref_mex_") and NAME not in p)
    print(f"wrote ref_mex_{NAME}.npz: {n} cases on {len(fs)} frames, {size} bytes")
    assert size <= cap, f"the fixture ({size} bytes) is larger than the largest ref_mex_ fixture beside it ({cap})"


if __name__ == "__main__":
    main()
