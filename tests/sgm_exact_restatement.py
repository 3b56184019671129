"""numpy restatement (int64) of sgm(C) with EXACT path arithmetic (include/fsgm.h, fsgm_sgm_batch_host_exact): the yardstick of
tests/test_sgm_exact_cpu.py and tests/test_gpu_sgm_exact*.py.  It is calc_cost_sgm.cpp:86-257 with every narrowing to unsigned
char taken out:

  path start (:152-180)   L[d] = C[d], stored minimum m = 0;
  step (:33-66)           L[d] = C[d] + min(Lp[d], Lp[d-1] + P1 (d > 0), Lp[d+1] + P1 (d < D-1), m_p + P2) - m_p,
                          m = min over d of L[d] -- the true minimum, the 255 of :39 is no clamp here;
  adaptive P2 (:68-72)    P2 / 8 (C's division) in place of P2 where |I1[cur] - I1[pre]| > 25;
  passes and paths        along x (:182-190), along y (:193-202), from the upper left (:205-213) and the upper right (:215-225),
                          a diagonal that leaves the frame re-entering at the opposite border as a new path; pass 1 (:115-123) is
                          pass 0 on the point-mirrored frame; S = the sum of the 4 or 8 path costs.

Nothing here calls the library, and nothing is taken from the oracle but its winner-take-all (pyoracle.epi_wta, u32 sums in,
first minimum, the bestIdx > 1 && bestIdx < dMax rule and the parabola out), which the exact call shares with the plain one.
Each path is written per line, a step at a time over d only: slower than tests/adaptive_p2_restatement.py's vectorised form
and independent of it; tests/test_sgm_exact_cpu.py ties the two (and the C++ oracle) together inside the no-wrap budget.

Conventions are pyoracle's: volumes (H, W, D) uint8, images (H, W) uint8, bestD = index * 256 (+ sub-pixel)."""
import numpy as np

from oracle import pyoracle

THRESHOLD = 25                                                 # :69


def step(Lp, mp, C, P1, P2):
    """one pixel: Lp, C (D,) int64, mp the previous pixel's stored minimum.  Returns (L, min L)."""
    best = np.minimum(Lp, mp + P2)
    best[1:] = np.minimum(best[1:], Lp[:-1] + P1)              # d > 0
    best[:-1] = np.minimum(best[:-1], Lp[1:] + P1)             # d < D - 1
    L = C + best - mp
    return L, int(L.min())


def _p2(P2, I, cur, pre, adaptive):
    if not adaptive:
        return P2
    return P2 // 8 if abs(int(I[cur]) - int(I[pre])) > THRESHOLD else P2      # (P2 >= 0: floor = C's truncation)


def _pass0(C, I, P1, P2, paths, adaptive):
    H, W, D = C.shape
    S = np.zeros((H, W, D), np.int64)
    dirs = [(1, 0), (0, 1)] + ([(1, 1), (-1, 1)] if paths == 8 else [])
    for dx, dy in dirs:
        # the path through every pixel in raster order: its predecessor is (x - dx, y - dy), a pixel without one starts a path
        L = np.zeros((H, W, D), np.int64)
        m = np.zeros((H, W), np.int64)
        for y in range(H):
            for x in range(W):                                 # (a predecessor lies to the left or in the row above: already done)
                px, py = x - dx, y - dy
                if px < 0 or px >= W or py < 0:
                    L[y, x], m[y, x] = C[y, x], 0                                      # :152-180
                else:
                    L[y, x], m[y, x] = step(L[py, px], int(m[py, px]), C[y, x], P1, _p2(P2, I, (y, x), (py, px), adaptive))
        S += L
    return S


def aggregate(Cv, P1, P2, paths=4, guide=None):
    """S (H, W, D) int64 of the exact recurrence; guide (H, W) uint8: adaptive P2 read from it"""
    assert paths in (4, 8) and 0 <= int(P1) <= 255 and 0 <= int(P2) <= 255
    C = np.ascontiguousarray(Cv, np.uint8).astype(np.int64)
    adaptive = guide is not None
    I = np.ascontiguousarray(guide, np.uint8).astype(np.int64) if adaptive else np.zeros(C.shape[:2], np.int64)
    S = _pass0(C, I, int(P1), int(P2), paths, adaptive)
    S += _pass0(C[::-1, ::-1], I[::-1, ::-1], int(P1), int(P2), paths, adaptive)[::-1, ::-1]          # pass 1: the point mirror
    assert S.min() >= 0 and S.max() <= paths * (255 + int(P2))
    return S


def sgm(Cv, P1, P2, paths=4, guide=None, subpixel=1):
    """(bestD, minC, S) of one volume: uint32 (H, W), (H, W), (H, W, D)"""
    H, W, D = Cv.shape
    S = aggregate(Cv, P1, P2, paths, guide)
    flat = np.zeros(S.size + 1, np.uint32)                     # (one word past the end, 0: what the last pixel's parabola may read)
    flat[:-1] = S.reshape(-1)
    bestD, minC = pyoracle.epi_wta(flat, W, H, D, subpixel)
    return bestD, minC, S.astype(np.uint32)


def sgm_batch(Cvs, P1, P2, paths=4, guides=None, subpixel=1):
    """the same on (N, H, W, D): stacked outputs"""
    outs = [sgm(Cvs[f], P1, P2, paths, None if guides is None else guides[f], subpixel) for f in range(len(Cvs))]
    return tuple(np.stack([o[k] for o in outs]) for k in range(3))
