"""numpy restatement (int64) of the 2-D matcher with EXACT path arithmetic (include/fsgm.h, fsgm_sgm2d_batch_host_exact,
fsgm_pyd_plan_set_exact): the yardstick of tests/test_sgm2d_exact_cpu.py and tests/test_gpu_sgm2d_exact*.py.  It is
calc_pyd_cost_sgm.cpp:34-89 (sgm_step) and :114-296 (sgm2d's path loops) with every narrowing to unsigned char taken out:

  path start (:180-208)   L[c] = C[c], stored minimum m = 0 (memcpy of the costs, L[dMax] = 0);
  step (:34-89)           xpre = (int)(sx + dx + 0.5), ypre = (int)(sy + dy + 0.5) (:46-47, C truncation);
                          min1 = Lp[xpre, ypre] where that cell lies in the window, else m_p + P2 (:50, :56-59);
                          min2 = min(m_p + P2, Lp[tx, ty] + P1 over the 5x5 around (xpre, ypre) without its centre, cells
                          outside the window skipped) (:61-76);
                          L[c] = C[c] + min(m_p + P2, min1, min2) - m_p (:78-83); m = min over c of L[c] (:84, :88) -- the true
                          minimum: MAX_PATH_COST is no clamp here;
  adaptive P2 (:91-95)    P2 / 8 (C's division) in place of P2 where |I1[cur] - I1[pre]| > 50;
  paths (:162-277)        L1 along x, L3 along y, L2 from (x - xstep, y - ystep), L4 from (x + xstep, y - ystep); L1 and L2 start
                          at x == xstart, L3, L2 and L4 at y == ystart, L4 at x == xend - xstep; hint and intensity deltas are
                          those of the pixel and its predecessor (:213-257);
  passes (:142-151)       pass 0 runs x and y upwards, every later pass downwards (xstep = ystep = -1);
  S (:266-271)            += L1 + L3 (+ L2 + L4 with the diagonal paths), per pass.

Nothing here calls the library, and nothing is taken from tests/py_restatement.py's aggregation or from the oracle but its
winner-take-all and parabolas (pyoracle.pyd_wta), which the exact call shares with the plain one.  The loops are the
reference's own, pixel by pixel; one step is vectorised over the window.  The runner-up cost is computed here from S by the rule
of include/fsgm.h.

Conventions are pyoracle's: volumes (H, W, D) uint8 with candidate index sx * Sy + sy, hints (2, mvH, mvW) float64 with plane 0 = x,
images (H, W) uint8."""
import numpy as np

from oracle import pyoracle

THRESHOLD = 50                                                 # :92
ABSENT = np.int64(1) << 40                                     # a cell outside the window: above every sum that can occur
R = 2                                                          # :61
NO_RUNNER_UP = 0xFFFFFFFF


def _pre(n, delta):
    """(int)(s + delta + 0.5) for s = 0..n-1 (:46-47), limited to where the 5x5 around it can still touch the window"""
    v = np.trunc(np.clip((np.arange(n, dtype=np.float64) + delta) + 0.5, -1.0e6, 1.0e6)).astype(np.int64)
    return np.clip(v, -(R + 1), n + R)                         # (farther out every cell of the 5x5 is outside the window as well)


def step(Lp, mp, C, dx, dy, P1, P2):
    """one pixel: Lp, C (Sx, Sy) int64, mp the previous pixel's stored minimum.  Returns (L, min L)."""
    Sx, Sy = C.shape
    pad = 2 * R + 1
    G = np.full((Sx + 2 * pad, Sy + 2 * pad), ABSENT, np.int64)
    G[pad:pad + Sx, pad:pad + Sy] = Lp
    xpre, ypre = _pre(Sx, dx)[:, None] + pad, _pre(Sy, dy)[None, :] + pad
    jump = mp + P2                                             # :50-53
    min1 = np.minimum(G[xpre, ypre], jump)                     # :56-59 (an absent centre leaves min1 = jump)
    min2 = np.full((Sx, Sy), jump, np.int64)
    for k in range(-R, R + 1):
        for m in range(-R, R + 1):
            if m == 0 and k == 0:                              # :64
                continue
            min2 = np.minimum(min2, G[xpre + m, ypre + k] + P1)                # :67-74 (absent + P1 never wins)
    L = C + np.minimum(min1, min2) - mp                        # :78-83
    return L, int(L.min())


def _p2(P2, I, cur, pre, adaptive):
    if not adaptive:
        return P2
    return P2 // 8 if abs(int(I[cur]) - int(I[pre])) > THRESHOLD else P2      # (P2 >= 0: floor = C's truncation)


def aggregate(Cv, preMv, Sx, Sy, P1, P2, diagonal=1, totalPass=2, guide=None, paths_out=None):
    """S (H, W, D) int64 of the exact recurrence.  guide (H, W) uint8: adaptive P2 read from it.  paths_out (a list): gets one
    (pass, name, L (H, W, D) int64, start (H, W) bool) per pass and path."""
    P1, P2 = int(P1), int(P2)
    assert 0 <= P1 <= 255 and 0 <= P2 <= 255 and totalPass >= 1
    H, W, D = Cv.shape
    assert D == Sx * Sy
    C = np.ascontiguousarray(Cv, np.uint8).astype(np.int64).reshape(H, W, Sx, Sy)
    adaptive = guide is not None
    I = np.ascontiguousarray(guide, np.uint8).astype(np.int64) if adaptive else np.zeros((H, W), np.int64)
    mvx, mvy = np.asarray(preMv[0], np.float64), np.asarray(preMv[1], np.float64)
    S = np.zeros((H, W, Sx, Sy), np.int64)
    names = ("L1", "L3") + (("L2", "L4") if diagonal else ())
    for p in range(totalPass):
        ystart, yend, ystep = (0, H, 1) if p == 0 else (H - 1, -1, -1)       # :134-151
        xstart, xend, xstep = (0, W, 1) if p == 0 else (W - 1, -1, -1)
        vol = {n: np.zeros((H, W, Sx, Sy), np.int64) for n in names}
        mins = {n: np.zeros((H, W), np.int64) for n in names}
        started = {n: np.zeros((H, W), bool) for n in names}

        def run(name, y, x, py, px):
            """the path `name` at (y, x) from its predecessor (py, px), or its start when (py, px) is None"""
            if py is None:
                vol[name][y, x], mins[name][y, x], started[name][y, x] = C[y, x], 0, True
                return
            dx, dy = mvx[y, x] - mvx[py, px], mvy[y, x] - mvy[py, px]           # :213-214 and its siblings
            vol[name][y, x], mins[name][y, x] = step(vol[name][py, px], int(mins[name][py, px]), C[y, x], dx, dy, P1,
                                                     _p2(P2, I, (y, x), (py, px), adaptive))

        for y in range(ystart, yend, ystep):
            for x in range(xstart, xend, xstep):
                first_x, first_y, last_x = x == xstart, y == ystart, x == xend - xstep
                run("L1", y, x, *((None, None) if first_x else (y, x - xstep)))                   # :180-182, :210-222
                run("L3", y, x, *((None, None) if first_y else (y - ystep, x)))                   # :190-192, :225-236
                if diagonal:
                    run("L2", y, x, *((None, None) if first_x or first_y else (y - ystep, x - xstep)))    # :184-196, :239-250
                    run("L4", y, x, *((None, None) if last_x or first_y else (y - ystep, x + xstep)))     # :198-207, :252-264
        for n in names:                                                          # :266-271
            S += vol[n]
            if paths_out is not None:
                paths_out.append((p, n, vol[n].reshape(H, W, D), started[n]))
    assert S.min() >= 0 and S.max() <= len(names) * totalPass * (255 + P2)
    return S.reshape(H, W, D)


def runner_up(S, bestD, Sx, Sy):
    """minC2 (H, W) uint32 of include/fsgm.h: the smallest S at a Chebyshev distance >= 2 from the winner, NO_RUNNER_UP where none"""
    H, W, D = S.shape
    sx, sy = np.arange(D) // Sy, np.arange(D) % Sy
    bx, by = (bestD // Sy).astype(np.int64), (bestD % Sy).astype(np.int64)
    far = np.maximum(np.abs(sx[None, None, :] - bx[:, :, None]), np.abs(sy[None, None, :] - by[:, :, None])) >= 2
    return np.where(far, S.astype(np.int64), NO_RUNNER_UP).min(axis=2).astype(np.uint32)


def sgm2d(Cv, rX, rY, P1, P2, hints=None, guide=None, diagonal=1, totalPass=2, subpixel=1):
    """(bestD, minC, mvSub, flow, S, minC2) of one volume: bestD, minC, minC2 uint32 (H, W); mvSub, flow float64 (2, H, W) with
    flow = hint + window offset + mvSub (pyramidal_sgm.m:57-64); S uint32 (H, W, D).  guide: adaptive P2."""
    H, W, D = Cv.shape
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    mv = np.zeros((2, H, W)) if hints is None else np.asarray(hints, np.float64)
    S = aggregate(Cv, mv, Sx, Sy, P1, P2, diagonal, totalPass, guide).astype(np.uint32)
    bestD, minC, mvSub = pyoracle.pyd_wta(S, Sx, Sy, subpixel)
    off = np.stack([bestD // Sy, bestD % Sy]).astype(np.float64) - np.array([rX, rY], np.float64)[:, None, None]
    flow = mv[:, :H, :W] + off + mvSub
    return bestD, minC, mvSub, flow, S, runner_up(S, bestD, Sx, Sy)


def sgm2d_batch(Cvs, rX, rY, P1, P2, hints=None, guides=None, **kw):
    """the same on (N, H, W, D): stacked outputs"""
    outs = [sgm2d(Cvs[f], rX, rY, P1, P2, None if hints is None else hints[f], None if guides is None else guides[f], **kw)
            for f in range(len(Cvs))]
    return tuple(np.stack([o[k] for o in outs]) for k in range(6))
