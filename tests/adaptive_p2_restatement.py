"""numpy restatement of calc_cost_sgm.cpp:33-72 (sgm_step, adaptive_P2) and :86-257 (sgm) with the two switches the reference
compiles in as constants -- `adpativeP2` (:102) and `enableDiagnalPath` (:104) -- as arguments: the yardstick of
tests/test_adaptive_p2_cpu.py and tests/test_gpu_adaptive_p2*.py.  Only the aggregation is restated; cost volume, WTA, parabola,
vz -> disparity and the forward-backward check are the unchanged oracle's (pyoracle.epi_cost, epi_wta, epi_vz_to_disp,
epi_fb_check) and, for the linear build, tests/stereo_restatement.py's.  tests/golden/ref_mex_calc_cost_sgm_adaptive.npz pins
it to the reference's own compiled code with the two constants flipped.

PathCost, PixelType and CostType are unsigned char (common.h:4-6): every place the reference narrows to one of them is an
`& 0xFF` here.  A path's steps are vectorised over d and over the lines that advance together (the rows for the along-x path,
the columns for the other three); pass 1 (:115-123) is pass 0 on the point-mirrored frame.

Conventions are pyoracle's: images (H, W) uint8, volumes (H, W, D) uint8, maps (2, H, W) float64, bestD = index * 256."""
import os

import numpy as np

from oracle import pyoracle
from tests import stereo_restatement as SR

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mex_calc_cost_sgm_adaptive.npz")
THRESHOLD = 25                                                 # :69
_golden = None


def c_div(a, b):
    """C's int division: truncation towards zero"""
    q = abs(int(a)) // abs(int(b))
    return q if (a >= 0) == (b > 0) else -q


def adaptive_P2(P2, pixCur, pixPre):
    """:68-72, elementwise on int arrays"""
    return np.where(np.abs(pixCur - pixPre) > THRESHOLD, c_div(P2, 8), int(P2))


def sgm_step(Lpre, mpre, C, P1, P2):
    """:33-66 on n pixels at once: Lpre, C (n, D) and the stored minimum mpre (n,) as int64 holding u8 values, P2 (n,) int64.
    Returns (L, min over d of L)."""
    jump = ((mpre + P2) & 0xFF)[:, None]                       # :46, :51 PathCost min2 = min3 = LpreMin + P2
    best = np.minimum(jump, Lpre)                              # :43, :55
    nb = (Lpre + P1) & 0xFF                                    # :47-48 std::min<PathCost>(.., Lpre[d +- 1] + P1)
    best[:, 1:] = np.minimum(best[:, 1:], nb[:, :-1])          # d > 0
    best[:, :-1] = np.minimum(best[:, :-1], nb[:, 1:])         # d < dMax - 1
    L = (C + best - mpre[:, None]) & 0xFF                      # :60
    return L, np.minimum(L.min(axis=1), 255)                   # :39, :61, :65


def _pass0(C, I, P1, P2, paths, adaptive):
    """sum over the pass-0 paths of their costs, (H, W, D) int64: along x (:182-190), along y (:193-202) and, with 8 paths, from
    the upper left (:205-213) and the upper right (:215-225)"""
    H, W, D = C.shape
    p2 = (lambda cur, pre: adaptive_P2(P2, cur, pre)) if adaptive else (lambda cur, pre: np.full(cur.shape, int(P2), np.int64))
    S = np.zeros((H, W, D), np.int64)
    # L1: a path per row, started at x == xstart (:152-155: L = C, stored minimum 0)
    L, m = C[:, 0].copy(), np.zeros(H, np.int64)
    S[:, 0] += L
    for x in range(1, W):
        L, m = sgm_step(L, m, C[:, x], P1, p2(I[:, x], I[:, x - 1]))
        S[:, x] += L
    # L3: a path per column, started at y == ystart (:162-164)
    L, m = C[0].copy(), np.zeros(W, np.int64)
    S[0] += L
    for y in range(1, H):
        L, m = sgm_step(L, m, C[y], P1, p2(I[y], I[y - 1]))
        S[y] += L
    if paths == 8:
        # L2: predecessor (x - 1, y - 1); a start in the first row and the first column (:156-159, :166-168)
        L, m = C[0].copy(), np.zeros(W, np.int64)
        S[0] += L
        for y in range(1, H):
            Ln, mn = C[y].copy(), np.zeros(W, np.int64)
            if W > 1:
                Ln[1:], mn[1:] = sgm_step(L[:-1], m[:-1], C[y, 1:], P1, p2(I[y, 1:], I[y - 1, :-1]))
            L, m = Ln, mn
            S[y] += L
        # L4: predecessor (x + 1, y - 1); a start in the first row and the last column (:170-171, :175-179)
        L, m = C[0].copy(), np.zeros(W, np.int64)
        S[0] += L
        for y in range(1, H):
            Ln, mn = C[y].copy(), np.zeros(W, np.int64)
            if W > 1:
                Ln[:-1], mn[:-1] = sgm_step(L[1:], m[1:], C[y, :-1], P1, p2(I[y, :-1], I[y - 1, 1:]))
            L, m = Ln, mn
            S[y] += L
    return S


def aggregate(Cv, I1, P1, P2, paths=4, adaptive=0):
    """Sp of :86-257 as pyoracle.epi_aggregate returns it: flat uint32 of H * W * D + 1 words (the last one 0: what the parabola
    of the last pixel may read, :293-296)."""
    assert paths in (4, 8)
    C = np.ascontiguousarray(Cv, np.uint8).astype(np.int64)
    I = np.ascontiguousarray(I1, np.uint8).astype(np.int64)
    S = _pass0(C, I, int(P1), int(P2), paths, adaptive)
    S += _pass0(C[::-1, ::-1], I[::-1, ::-1], int(P1), int(P2), paths, adaptive)[::-1, ::-1]     # pass 1: the point mirror
    out = np.zeros(C.size + 1, np.uint32)
    out[:-1] = S.reshape(-1)
    return out


def calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, paths=4, adaptive=0, subpixel=1, vz_to_disp=1, fb_check=0):
    """(bestD, minC[, conf, bestD2]) of the shipped (USE_VZIND) build with the two switches"""
    H, W = I1.shape
    Cv = pyoracle.epi_cost(I1, I2, D, vMax, pd0, nd, off)
    bestD, minC = pyoracle.epi_wta(aggregate(Cv, I1, P1, P2, paths, adaptive), W, H, D, subpixel)
    fb = pyoracle.epi_fb_check(bestD, pd0, nd, off, vMax, D + 1) if fb_check else ()
    if vz_to_disp:
        bestD = pyoracle.epi_vz_to_disp(bestD, off, vMax, D + 1)
    return (bestD, minC) + tuple(fb)


def calc_cost_sgm_linear(I1, I2, D, pd0, nd, P1, P2, paths=4, adaptive=0, subpixel=1, fb_check=0):
    """the same for the build without USE_VZIND (tests/stereo_restatement.py)"""
    H, W = I1.shape
    Cv = SR.linear_cost(I1, I2, D, pd0, nd)
    bestD, minC = pyoracle.epi_wta(aggregate(Cv, I1, P1, P2, paths, adaptive), W, H, D, subpixel)
    fb = SR.linear_fb_check(bestD, pd0, nd) if fb_check else ()
    return (bestD, minC) + tuple(fb)


def golden():
    """the fixture tests/golden/make_ref_adaptive_golden.py wrote, loaded once"""
    global _golden
    if _golden is None:
        with np.load(GOLDEN_PATH, allow_pickle=False) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_count():
    return int(golden()["n"])


def golden_case(i):
    """(inputs, [bestD, minC, conf, bestD2]) of fixture case i; inputs carry the variant: linear, paths, adaptive"""
    g = golden()
    j, linear, paths, adaptive = (int(v) for v in g[f"c{i}_variant"])
    D, vMax, P1, P2 = g[f"f{j}_args"]
    ins = dict(I1=g[f"f{j}_I1"], I2=g[f"f{j}_I2"], D=int(D), vMax=float(vMax), pd0=g[f"f{j}_pd0"], nd=g[f"f{j}_nd"], off=g[f"f{j}_off"],
               P1=int(P1), P2=int(P2), linear=linear, paths=paths, adaptive=adaptive, frame=j,
               id=f"{bytes(g[f'f{j}_id']).decode()}/{'lin' if linear else 'vz'}{paths}{'a' if adaptive else ''}")
    return ins, [g[f"c{i}_out{k}"] for k in range(4)]


def restate(c, **kw):
    """the restatement on a fixture case's inputs (its own variant unless overridden)"""
    a = dict(paths=c["paths"], adaptive=c["adaptive"])
    a.update(kw)
    if c["linear"]:
        return calc_cost_sgm_linear(c["I1"], c["I2"], c["D"], c["pd0"], c["nd"], c["P1"], c["P2"], **a)
    return calc_cost_sgm(c["I1"], c["I2"], c["D"], c["vMax"], c["pd0"], c["nd"], c["off"], c["P1"], c["P2"], **a)
