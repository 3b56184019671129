"""The yardstick of the rectified-stereo post-processing chain (tests/test_stereo_pp_cpu.py, tests/test_gpu_stereo_pp.py).

calc_disp_from_first.m and forward_backward_check.m restated ONCE, in the reference's own raster order, with the disparity
function as a parameter:

  disp_from_first(D1, Pd0, nd, disp_of)        calc_disp_from_first.m:4-48
  fb_check(D1, D2, Pd0, nd, disp_of, thr)      forward_backward_check.m:4-37

With disp_of = vz_disp(O, vMax, n) (vzInd2Disp.m) they are fsgm_oracle_calc_disp_from_first / _forward_backward_check bit for
bit (pinned in tests/test_stereo_pp_cpu.py).  The stereo form is the same two functions on the rectified maps
Pd0 = (x + 1, y + 1), direction (direction, 0), with disp_of = w -> d_min + w: no second, row-only statement exists here.
Speckle filter and in-fill are the oracle's own scalar functions, the matcher is tests/stereo_range_restatement.py's."""
import numpy as np

from oracle import pyoracle
from tests import stereo_range_restatement as SR
from tests import stereo_restatement as R


def vz_disp(O, vMax, n):
    """vzInd2Disp.m:1-5 as a disparity function"""
    def f(w):
        with np.errstate(all="ignore"):
            r = w / n * vMax
            return O * (r / (1 - r))
    return f


def linear_disp(d_min):
    """the rectified case: disp = d_min + w"""
    return lambda w: float(d_min) + w


def round_half_away(a):
    """MATLAB's round: half away from zero (exact: a - trunc(a) is)"""
    with np.errstate(all="ignore"):
        t = np.trunc(a)
        return np.where(np.abs(a - t) >= 0.5, t + np.sign(a), t)


def _targets(D1, Pd0, nd, disp_of):
    with np.errstate(all="ignore"):
        disp = disp_of(D1)                                       # :11 / :15
        return Pd0[0] + disp * nd[0], Pd0[1] + disp * nd[1]      # :13-14 / :17-18


def disp_from_first(D1, Pd0, nd, disp_of):
    D1 = np.asarray(D1, np.float64)
    H, W = D1.shape
    p2x, p2y = _targets(D1, Pd0, nd, disp_of)
    sx0, sy0 = np.floor(p2x).tolist(), np.floor(p2y).tolist()    # :16
    v1 = D1.tolist()
    D2 = [[-1.0] * W for _ in range(H)]                          # :6
    for j in range(H):                                           # :8-9
        for i in range(W):
            v, x0, y0 = v1[j][i], sx0[j][i], sy0[j][i]
            for sx, sy in ((x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)):       # :24-46
                if sx >= 1 and sx <= W and sy >= 1 and sy <= H:
                    row = D2[int(sy) - 1]
                    t = row[int(sx) - 1]
                    if t == 0 or t < v:                          # :25
                        row[int(sx) - 1] = v
    return np.array(D2, np.float64).reshape(H, W)


def fb_check(D1, D2, Pd0, nd, disp_of, thr=2.0):
    D1 = np.asarray(D1, np.float64)
    H, W = D1.shape
    p2x, p2y = _targets(D1, Pd0, nd, disp_of)
    p2x, p2y = round_half_away(p2x), round_half_away(p2y)        # :20
    out = D1.copy()
    with np.errstate(all="ignore"):
        valid = ~np.isnan(D1)                                    # :12
        inside = (p2x >= 1) & (p2x <= W) & (p2y >= 1) & (p2y <= H)   # :22 (a NaN target: outside, as the oracle)
        out[valid & ~inside] = np.nan
        m = valid & inside
        d2 = np.asarray(D2, np.float64)[p2y[m].astype(np.int64) - 1, p2x[m].astype(np.int64) - 1]
        bad = (d2 == -1) | (np.abs(D1[m] - d2) > thr)            # :27, :32
    sel = np.zeros((H, W), bool)
    sel[m] = bad
    out[sel] = np.nan
    return out


# ---------------------------------------------------------------------------------------------- the stereo form
def stereo_disp_from_first(w, d_min, direction):
    w = np.asarray(w, np.float64)
    pd0, nd = R.rectified_maps(w.shape[1], w.shape[0], direction)
    return disp_from_first(w, pd0, nd, linear_disp(d_min))


def stereo_fb_check(w, D2, d_min, direction, thr=2.0):
    w = np.asarray(w, np.float64)
    pd0, nd = R.rectified_maps(w.shape[1], w.shape[0], direction)
    return fb_check(w, D2, pd0, nd, linear_disp(d_min), thr)


def chain(w, dMax, d_min, direction, speckle_max_diff=2.0, speckle_max_size=100.0, fb_threshold=2.0, island_fraction=0.1, in_fill=1):
    """test.m:45-50 on the candidate-index map w: dict(w1, D2, c0 (after the check), c (after island removal), filled (:49), g (what
    disp_pp is made of: filled, or c with in_fill=0))"""
    H, W = w.shape
    w1 = pyoracle.speckle_filter(w, speckle_max_diff, speckle_max_size)[0]                   # :45
    D2 = stereo_disp_from_first(w1, d_min, direction)                                        # :46
    c0 = stereo_fb_check(w1, D2, d_min, direction, fb_threshold)                             # :47
    c = pyoracle.speckle_filter(c0, float(dMax), float(H * W) * island_fraction)[0]         # :48
    filled = pyoracle.scanline_in_fill(c)                                                    # :49
    return dict(w1=w1, D2=D2, c0=c0, c=c, filled=filled, g=filled if in_fill else c.copy())


def index_map(bestD):
    """w = bestD / 256, exact (with subpixel=0 the matcher's bestD is the reference's unscaled index, calc_cost_sgm.cpp:273: the
    chain takes bestD / 256 all the same)"""
    return np.asarray(bestD, np.uint32).astype(np.float64) / 256.0


def outputs(I1, I2, dMax, d_min, direction, P1=6, P2=64, paths=4, subpixel=1, adaptive=0, **chain_kw):
    """what stereo_sgm_pp returns for one pair, and the chain's intermediates: dict(disp_pp, disp_checked, disp, minC, disp2, ch)"""
    o = SR.oracle(I1, I2, dMax, direction, d_min, P1, P2, paths, subpixel, adaptive)
    ch = chain(index_map(o["bestD"]), dMax, d_min, direction, **chain_kw)
    return dict(disp_pp=float(d_min) + ch["g"], disp_checked=float(d_min) + ch["c"], disp=SR.true_disp(o["bestD"], d_min), minC=o["minC"],
                disp2=np.where(ch["D2"] == -1.0, -1.0, float(d_min) + ch["D2"]), ch=ch)


def shares(ch):
    """the non-vacuity figures of one frame: (share of the pixels the check removes, share kept after island removal, pixels
    the in-fill fills)"""
    n = ch["w1"].size
    lost = int((~np.isnan(ch["w1"]) & np.isnan(ch["c0"])).sum())
    kept = int((~np.isnan(ch["c"])).sum())
    filled = int((np.isnan(ch["c"]) & ~np.isnan(ch["filled"])).sum())
    return lost / n, kept / n, filled


# ---------------------------------------------------------------------------------------------- inputs of the tests
def occluding_pair(W, H, D, seed, rect, bg, delta, direction=-1):
    """A pair with an occlusion band by construction, over synth.image_pair's texture: the background of I1 lies `bg` columns
    further left in I2 (direction -1: its disparity is bg, which may be negative), and the rectangle rect = (y0, y1, x0, x1)
    of I1 is pasted into I2 bg + delta columns to the left, delta > 0: the delta columns of background left of the rectangle
    are hidden behind it in I2.  direction +1: both images mirrored, so that the matches lie at x + d."""
    from fsgm_amd import synth
    m = 64
    wide = synth.image_pair(W + 2 * m, H, D, seed=seed)[0]
    I1 = wide[:, m:m + W].copy()
    I2 = wide[:, m + bg:m + bg + W].copy()
    y0, y1, x0, x1 = rect
    fg = bg + delta
    assert 0 <= x0 - fg and x1 - fg <= W and abs(bg) < m
    I2[y0:y1, x0 - fg:x1 - fg] = I1[y0:y1, x0:x1]
    if direction == +1:
        I1, I2 = I1[:, ::-1], I2[:, ::-1]
    return np.ascontiguousarray(I1), np.ascontiguousarray(I2)


# The whole-call frames per shape: (W, H, D, seed, rect, delta); the background's disparity is d_min + BG_OFFSET[key], inside
# every search range.  Adopted on the conditions tests/test_stereo_pp_cpu.py asserts.
FRAMES = {
    "96x40": [(96, 40, 32, 41, (8, 32, 50, 80), 8), (96, 40, 32, 42, (4, 30, 44, 76), 9), (96, 40, 32, 43, (10, 36, 48, 84), 7)],
    "61x37": [(61, 37, 16, 51, (6, 30, 28, 50), 6), (61, 37, 16, 52, (8, 33, 26, 50), 5), (61, 37, 16, 53, (4, 28, 30, 54), 6)],
}
BG_OFFSET = {"96x40": 6, "61x37": 3}


def frames(key, n, d_min=0, direction=-1):
    ps = [occluding_pair(W, H, D, seed, rect, d_min + BG_OFFSET[key], delta, direction) for W, H, D, seed, rect, delta in FRAMES[key][:n]]
    return np.stack([p[0] for p in ps]), np.stack([p[1] for p in ps])


# The whole calls of the GPU tests: (shape key, frames, paths, subpixel, adaptive P2, d_min, direction, in_fill, chain overrides)
CALLS = [
    ("96x40", 1, 4, 1, 0, 0, -1, 1, {}),
    ("96x40", 3, 8, 1, 1, -5, -1, 1, {}),
    ("96x40", 1, 8, 0, 0, 12, +1, 0, {}),
    ("96x40", 3, 4, 1, 0, 12, -1, 1, dict(speckle_max_size=40.0, island_fraction=0.05)),
    ("61x37", 3, 4, 0, 1, -5, +1, 1, {}),
    ("61x37", 1, 8, 1, 0, 0, -1, 1, dict(speckle_max_size=30.0, island_fraction=0.2)),
    ("61x37", 1, 4, 1, 0, 12, +1, 0, {}),
]


def call_id(c):
    key, n, paths, sub, ad, d_min, direction, fill, kw = c
    return f"{key}-n{n}-p{paths}-s{sub}-a{ad}-dmin{d_min}-dir{direction:+d}-fill{fill}" + ("-chain" if kw else "")


_call_cache = {}


def call_reference(c):
    """(left, right, [outputs(...) per frame]) of one entry of CALLS, computed once"""
    cid = call_id(c)
    if cid not in _call_cache:
        key, n, paths, sub, ad, d_min, direction, fill, kw = c
        L, Rt = frames(key, n, d_min, direction)
        D = FRAMES[key][0][2]
        _call_cache[cid] = (L, Rt, D, [outputs(L[f], Rt[f], D, d_min, direction, 6, 64, paths, sub, ad, in_fill=fill, **kw) for f in range(n)])
    return _call_cache[cid]


def two_plane_map(W, H):
    """a rectangle of index 12 on a background of 4 (direction -1: the rectangle hides a band of the background)"""
    w = np.full((H, W), 4.0)
    w[H // 4:H - H // 4 if H >= 4 else H, W // 3:W - W // 4] = 12.0
    return w


def stage_maps(W, H, dMax=24, seed=5):
    """the input maps of the row kernel's tests, by name"""
    from fsgm_amd import synth
    u = synth.uniform_f64(seed + W * 7 + H, (2, H, W))
    rnd = np.floor(u[0] * dMax * 256.0) / 256.0
    rnd[u[1] < 0.1] = np.nan
    yy, xx = np.mgrid[0:H, 0:W]
    half = ((xx * 3 + yy) % 9).astype(np.float64) + 0.5          # k + 0.5: round meets ties, also across the image edges
    nanrow = rnd.copy()
    nanrow[H // 2] = np.nan
    return {"random": rnd, "half": half, "constant": np.full((H, W), 3.0), "two_plane": two_plane_map(W, H), "nan_row": nanrow,
            "all_nan": np.full((H, W), np.nan)}
