"""Rectified stereo with a search range that starts at d_min: the yardsticks of tests/test_stereo_range_cpu.py and
tests/test_gpu_stereo_range*.py.  Nothing here is new semantics: the feature IS the reference's linear build (calc_cost_sgm.cpp
without USE_VZIND) on the maps Pd0 = (x + 1 + direction * d_min, y + 1), normDir = (direction, 0), whose index d then samples
clamp(x + direction * (d_min + d), 0, W - 1) (:368-375) and whose forward-backward check (:429-536) works on those same maps.

  oracle(...)        tests/stereo_restatement.py's restated linear cost on the shifted MAPS (fp64 positions, C round, clamp), the
                     unchanged oracle's aggregation and WTA, the restated check on the shifted maps
  closed_form(...)   the plain integer statement clamp(x + direction * (d_min + d)) + box + SGM
  true_disp / true_disp2   what the _range entry points return: int32 256 * d_min + value, INT32_MIN for the invalid marker

tests/golden/ref_mex_stereo_range.npz (make_ref_stereo_range_golden.py) pins all of it to the reference's own compiled code."""
import os

import numpy as np

from oracle import pyoracle
from tests import stereo_restatement as R

INT32_MIN = -(1 << 31)
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mex_stereo_range.npz")
_golden = None


def shifted_maps(W, H, direction, d_min):
    """(pixelPosD0, normlizeDirection) of the shifted range: R.rectified_maps with the start column moved by direction * d_min"""
    pd0, nd = R.rectified_maps(W, H, direction)
    pd0[0] += float(int(direction) * int(d_min))
    return pd0, nd


def range_raw_cost(I1, I2, D, direction, d_min):
    """Hamming distance of census(I1)[y][x] and census(I2)[y][clamp(x + direction * (d_min + d))], (H, W, D) uint8"""
    cen1, cen2 = pyoracle.census(I1), pyoracle.census(I2)
    H, W = cen1.shape
    xs = np.clip(np.arange(W)[:, None] + int(direction) * (int(d_min) + np.arange(D)[None, :]), 0, W - 1)       # (W, D)
    x = cen1[:, :, None] ^ cen2[:, xs]
    bits = np.zeros(x.shape, np.uint8)
    for b in range(32):
        bits += ((x >> np.uint32(b)) & np.uint32(1)).astype(np.uint8)
    return bits


def true_disp(v, d_min):
    """candidate index * 256 (+ parabola) -> int32 true disparity * 256"""
    return (np.asarray(v, np.uint32).astype(np.int64) + 256 * int(d_min)).astype(np.int32)


def true_disp2(v, d_min):
    """the same for the second view: the invalid marker 512 << 8 -> INT32_MIN"""
    v = np.asarray(v, np.uint32)
    return np.where(v == R.INVALID_DISPARITY, INT32_MIN, v.astype(np.int64) + 256 * int(d_min)).astype(np.int32)


def _finish(Cv, I1, P1, P2, paths, subpixel, adaptive, fb_check, pd0, nd):
    H, W, D = Cv.shape
    if adaptive:
        from tests import adaptive_p2_restatement as A
        S = A.aggregate(Cv, I1, P1, P2, paths, 1)
    else:
        S = pyoracle.epi_aggregate(Cv, P1, P2, paths)
    bestD, minC = pyoracle.epi_wta(S, W, H, D, subpixel)
    out = dict(C=Cv, S=np.asarray(S)[:-1].reshape(H, W, D), bestD=bestD, minC=minC)
    if fb_check:
        out["conf"], out["bestD2"] = R.linear_fb_check(bestD, pd0, nd)
    return out


def oracle(I1, I2, D, direction, d_min, P1=6, P2=64, paths=4, subpixel=1, adaptive=0, fb_check=0):
    """dict(C, S, bestD, minC[, conf, bestD2]) -- bestD / bestD2 still candidate indices * 256 -- through the MAPS"""
    H, W = I1.shape
    pd0, nd = shifted_maps(W, H, direction, d_min)
    return _finish(R.linear_cost(I1, I2, D, pd0, nd), I1, P1, P2, paths, subpixel, adaptive, fb_check, pd0, nd)


def closed_form(I1, I2, D, direction, d_min, P1=6, P2=64, paths=4, subpixel=1):
    H, W = I1.shape
    return _finish(R.box_mean(range_raw_cost(I1, I2, D, direction, d_min)), I1, P1, P2, paths, subpixel, 0, 0, None, None)


def shifted_pair(W, H, s, direction, seed):
    """A textured pair whose true disparity is s everywhere (s may be negative): the match of I1[y][x] lies at
    I2[y][x + direction * s].  Columns of I2 that no column of I1 maps to carry independent texture."""
    from fsgm_amd import synth
    k = int(direction) * int(s)
    big = synth.uniform_u8(seed, (H, W + abs(k)))
    if k >= 0:                                                   # I2[x'] = I1[x' - k]
        I1, I2 = big[:, abs(k):], big[:, :W]
    else:                                                        # I2[x'] = I1[x' + |k|]
        I1, I2 = big[:, :W], big[:, abs(k):]
    return np.ascontiguousarray(I1), np.ascontiguousarray(I2)


def shift_matters(I1, I2, D, direction, d_min, s, paths=4):
    """(share of the interior pixels whose winner is within one index of s - d_min, share of those pixels whose disp differs
    at d_min = 0): the conditions a pair is adopted on.  Interior: more than |s| + 2 columns from either side edge."""
    H, W = I1.shape
    m = abs(int(s)) + 2
    inner = np.zeros((H, W), bool)
    inner[:, m + 1:W - m - 1] = True
    assert inner.any(), "no interior"
    a = oracle(I1, I2, D, direction, d_min, paths=paths)
    b = oracle(I1, I2, D, direction, 0, paths=paths)
    near = np.abs((a["bestD"].astype(np.int64) >> 8) - (int(s) - int(d_min))) <= 1
    differs = true_disp(a["bestD"], d_min) != true_disp(b["bestD"], 0)
    return float(near[inner].mean()), float(differs[inner].mean())


# ---------------------------------------------------------------------------------------------- the fixture
def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN_PATH, allow_pickle=False) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_count():
    return int(golden()["n"])


def golden_case(i):
    """(inputs, [bestD, minC, conf, bestD2]) of fixture case i.  inputs: I1, I2, D, direction, d_min, P1, P2, paths, fb, id;
    the images are rebuilt from the frame the case ran on.  Without fb conf / bestD2 are the zeros the reference leaves."""
    g = golden()
    j, D, direction, d_min, P1, P2, paths, fb = (int(v) for v in g[f"c{i}_args"])
    ins = dict(I1=g[f"f{j}_I1"], I2=g[f"f{j}_I2"], D=D, direction=direction, d_min=d_min, P1=P1, P2=P2, paths=paths, fb=fb,
               id=bytes(g[f"f{j}_id"]).decode() + f"/D{D}/dir{direction:+d}/dmin{d_min}/p{paths}/fb{fb}")
    return ins, [g[f"c{i}_out{k}"] for k in range(4)]


# Pairs whose one true disparity s lies outside [0, dMax) and inside [d_min, d_min + dMax): (W, H, dMax, direction, d_min, s,
# seed).  Adopted on shift_matters() -- tests/test_stereo_range_cpu.py asserts both conditions on the oracle alone.
SHIFT_CASES = [(61, 7, 64, -1, -40, -20, 31), (130, 7, 16, +1, 40, 50, 32), (61, 9, 32, +1, -17, -5, 33)]
