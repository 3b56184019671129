"""numpy restatement of what calc_cost_sgm.cpp does differently when it is built without its line 4 (#define USE_VZIND): the
yardstick of tests/test_stereo_cpu.py and tests/test_gpu_stereo.py.  Only the lines that differ are restated here --
linear_raw_cost (:368-378) on pyoracle.census, the box mean (:387-407) and linear_fb_check (:429-536, the #else branches);
aggregation and WTA are the unchanged oracle's (pyoracle.epi_aggregate, pyoracle.epi_wta).  tests/golden/
ref_mex_calc_cost_sgm_linear.npz pins all of it to the reference's own compiled code.

Conventions are pyoracle's: images (H, W) uint8, maps (2, H, W) float64 with 1-based start positions, bestD = index * 256."""
import os

import numpy as np

from oracle import pyoracle

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mex_calc_cost_sgm_linear.npz")
_golden = None


def golden():
    """the fixture tests/golden/make_ref_linear_golden.py wrote, loaded once"""
    global _golden
    if _golden is None:
        with np.load(GOLDEN_PATH, allow_pickle=False) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_count():
    return int(golden()["n"])


def golden_case(i):
    """(inputs, [bestD, minC, conf, bestD2]) of fixture case i"""
    g = golden()
    D, vMax, P1, P2 = g[f"c{i}_args"]
    ins = dict(I1=g[f"c{i}_I1"], I2=g[f"c{i}_I2"], D=int(D), vMax=float(vMax), pd0=g[f"c{i}_pd0"], nd=g[f"c{i}_nd"], off=g[f"c{i}_off"],
               P1=int(P1), P2=int(P2), id=bytes(g[f"c{i}_id"]).decode())
    return ins, [g[f"c{i}_out{k}"] for k in range(4)]


INVALID_DISPARITY = 512 << 8                                   # calc_cost_sgm.cpp:5
INT_MIN = -(1 << 31)


def c_round(v):
    """C round(): to nearest, halves away from zero (exact: no v + 0.5)."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(v)
        return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def to_int(v):
    """double -> int as x86-64 converts it (cvttsd2si): truncation, INT_MIN for NaN and everything outside int's range."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(v)
        ok = np.isfinite(t) & (t >= -2147483648.0) & (t <= 2147483647.0)
    return np.where(ok, np.where(ok, t, 0.0).astype(np.int64), INT_MIN)


def sample_positions(D, pd0, nd):
    """(x2, y2), each (H, W, D) int64: :368-375 -- d converted to double, one multiply and one add per axis, C round, clamp."""
    _, H, W = pd0.shape
    d = np.arange(D, dtype=np.float64)[None, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        vx = (pd0[0] - 1.0)[:, :, None] + d * nd[0][:, :, None]
        vy = (pd0[1] - 1.0)[:, :, None] + d * nd[1][:, :, None]
    x2 = np.clip(to_int(c_round(vx)), 0, W - 1)
    y2 = np.clip(to_int(c_round(vy)), 0, H - 1)
    return x2, y2


def linear_raw_cost(I1, I2, D, pd0, nd):
    """:343-381 without USE_VZIND: Hamming distance of the census codes, (H, W, D) uint8."""
    cen1, cen2 = pyoracle.census(I1), pyoracle.census(I2)
    x2, y2 = sample_positions(D, np.asarray(pd0, np.float64), np.asarray(nd, np.float64))
    x = cen1[:, :, None] ^ cen2[y2, x2]
    bits = np.zeros(x.shape, np.uint8)
    for b in range(32):
        bits += ((x >> np.uint32(b)) & np.uint32(1)).astype(np.uint8)
    return bits


def rectified_raw_cost(I1, I2, D, direction):
    """The closed form of linear_raw_cost on rectified maps: cen2[y][clamp(x + direction * d)]."""
    cen1, cen2 = pyoracle.census(I1), pyoracle.census(I2)
    H, W = cen1.shape
    xs = np.clip(np.arange(W)[:, None] + int(direction) * np.arange(D)[None, :], 0, W - 1)       # (W, D)
    x = cen1[:, :, None] ^ cen2[:, xs]
    bits = np.zeros(x.shape, np.uint8)
    for b in range(32):
        bits += ((x >> np.uint32(b)) & np.uint32(1)).astype(np.uint8)
    return bits


def box_mean(raw):
    """:387-407: 5x5 mean with replicate border, (u8)(1.0 * sum / 25 + 0.5) == (2 sum + 25) // 50."""
    H, W, D = raw.shape
    pad = np.pad(raw.astype(np.uint32), ((2, 2), (2, 2), (0, 0)), mode="edge")
    s = np.zeros((H, W, D), np.uint32)
    for dy in range(5):
        for dx in range(5):
            s += pad[dy:dy + H, dx:dx + W]
    return ((2 * s + 25) // 50).astype(np.uint8)


def rectified_maps(W, H, direction):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (np.ascontiguousarray(np.stack([xx + 1.0, yy + 1.0])),
            np.ascontiguousarray(np.stack([np.full((H, W), float(direction)), np.zeros((H, W))])))


def linear_cost(I1, I2, D, pd0, nd):
    return box_mean(linear_raw_cost(I1, I2, D, pd0, nd))


def calc_cost_sgm_linear(I1, I2, D, pd0, nd, P1, P2, paths=4, subpixel=1, want_cost=False):
    """(bestD, minC) of the linear build: the restated cost volume through the oracle's aggregation and WTA."""
    H, W = I1.shape
    Cv = linear_cost(I1, I2, D, pd0, nd)
    bestD, minC = pyoracle.epi_wta(pyoracle.epi_aggregate(Cv, P1, P2, paths), W, H, D, subpixel)
    return (bestD, minC, Cv) if want_cost else (bestD, minC)


def linear_fb_check(D1, pd0, nd, thr=2):
    """(conf, D2) of forward_backward_check / calc_disp_from_first, :429-536, the #else branches: d = D1 / 256.0."""
    D1 = np.asarray(D1, np.uint32)
    H, W = D1.shape
    d = D1.astype(np.float64) / 256.0                                                   # :453, :508
    with np.errstate(invalid="ignore", over="ignore"):
        vx = (pd0[0] - 1.0) + d * nd[0]
        vy = (pd0[1] - 1.0) + d * nd[1]
    sx, sy = to_int(vx), to_int(vy)                                                     # :462-463 truncating
    cx, cy = to_int(c_round(vx)), to_int(c_round(vy))                                   # :516-517
    D2 = np.full((H, W), INVALID_DISPARITY, np.uint32)                                  # :440-442
    for y in range(H):
        for x in range(W):
            for dy in (0, 1):
                for dx in (0, 1):
                    tx, ty = dx + int(sx[y, x]), dy + int(sy[y, x])                     # (int arithmetic: INT_MIN + 1 stays outside)
                    if 0 <= tx < W and 0 <= ty < H and (D2[ty, tx] == INVALID_DISPARITY or D2[ty, tx] < D1[y, x]):
                        D2[ty, tx] = D1[y, x]                                           # :471-474
    conf = np.ones((H, W), np.uint8)                                                    # :485
    for y in range(H):
        for x in range(W):
            px, py = int(cx[y, x]), int(cy[y, x])
            if px < 0 or px > W - 1 or py < 0 or py > H - 1:                            # :519-522
                conf[y, x] = 0
            elif D2[py, px] == INVALID_DISPARITY:                                       # :524-527
                conf[y, x] = 0
            elif abs(int(np.int32(D1[y, x])) - int(np.int32(D2[py, px]))) > thr:        # :529
                conf[y, x] = 0
    return conf, D2
