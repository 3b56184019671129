"""numpy restatement of the median between pyramid levels (test yardstick, no GPU code): pyramidal_sgm.m:66-72 with the
commented-out lines :70-71 live and a window size s,

    mvPyd{l} = mv                                                     (:66, the unfiltered flow)
    mv(:,:,c) = medfilt2(mv(:,:,c), [s s])                            (:70-71)
    mvPre = 2 * imresize(mv, 2, 'nearest')                            (:72, the hints of level l - 1)

medfilt2 by the rule the project picked for vmf: zero padding outside the map, the (s*s+1)/2-th smallest
value of the window, NaN above every number (np.sort puts it last), +-Inf as numbers.  The level loops are composed from the
oracle's impyramid_reduce, rgb2gray and single-level matchers; with s = 0 they are oracle.pyramidal_sgm and
tests.edge_inputs.oracle_pyramidal_ng.
"""
import numpy as np


def medfilt2(plane, s):
    """medfilt2(plane, [s s]) of one (H, W) plane, s odd"""
    plane = np.asarray(plane, np.float64)
    H, W = plane.shape
    r = s // 2
    pad = np.zeros((H + 2 * r, W + 2 * r))
    pad[r:r + H, r:r + W] = plane
    windows = np.lib.stride_tricks.sliding_window_view(pad, (s, s)).reshape(H, W, s * s)   # window (y, x) = pad[y:y+s, x:x+s]
    return np.ascontiguousarray(np.sort(windows, axis=-1)[..., (s * s) // 2])


def upsample2(flow):
    """2 * imresize(flow, 2, 'nearest') of a (2, H, W) flow"""
    return np.ascontiguousarray(2.0 * np.repeat(np.repeat(np.asarray(flow, np.float64), 2, axis=1), 2, axis=2))


def level_hints(flow, s):
    """the next finer level's hint map (2, 2H, 2W) from a level's flow (2, H, W); s = 0: no median"""
    flow = np.asarray(flow, np.float64)
    return upsample2(flow if s == 0 else np.stack([medfilt2(c, s) for c in flow]))


def _gray_levels(oracle, I0, I1, numPyd):
    rgb = I0.ndim == 3
    lv = [(np.ascontiguousarray(I0), np.ascontiguousarray(I1))]
    red = (lambda im: np.stack([oracle.impyramid_reduce(c) for c in im])) if rgb else oracle.impyramid_reduce
    for _ in range(1, numPyd):
        a, b = lv[-1]
        lv.append((red(a), red(b)))                              # :28-31
    return [(oracle.rgb2gray(a), oracle.rgb2gray(b)) if rgb else (a, b) for a, b in lv]      # :44-45


def pyramidal_sgm_lm(oracle, I0, I1, numPyd, s, P1=6, P2=32, agg=2, ver=5, hor=5, diagonal=1, totalPass=2, adaptiveP2=0):
    """The level loop around calc_pyd_cost_sgm.  Returns (mv of level 1, minC of level 1, [flow per level, finest first],
    the hint map level 1 ran with) -- the shapes of oracle.pyramidal_sgm plus the hints."""
    gray = _gray_levels(oracle, I0, I1, numPyd)
    mvPre = np.zeros((2,) + gray[-1][0].shape)                   # :34
    flows, Sy = [None] * numPyd, 2 * ver + 1
    for l in range(numPyd - 1, -1, -1):                          # :37
        g0, g1 = gray[l]
        h, w = g0.shape
        hints = mvPre
        bestD, minC, mvSub = oracle.calc_pyd_cost_sgm(g0, g1, mvPre, hor, ver, agg, int(l == 0), P1, P2, diagonal, totalPass, adaptiveP2)   # :50
        sx, sy = (bestD // Sy).astype(np.int64), (bestD % Sy).astype(np.int64)                # :57
        cur = np.stack([((sx - hor).astype(np.float64) + mvPre[0, :h, :w]) + mvSub[0],        # :59-64
                        ((sy - ver).astype(np.float64) + mvPre[1, :h, :w]) + mvSub[1]])
        flows[l] = cur                                           # :66
        if l > 0:
            mvPre = level_hints(cur, s)                          # :70-72
    return flows[0], minC, flows, hints


def pyramidal_ng_lm(oracle, I0, I1, numPyd, s, half=1, agg=2, sub=0, P1=6, P2=32):
    """The level loop around calc_pyd_cost_sgm_ng (tests.edge_inputs.oracle_pyramidal_ng with the median).  Returns ([flow per
    level, coarsest first], minC of level 1, the hint map level 1 ran with)."""
    gray = _gray_levels(oracle, I0, I1, numPyd)
    mvPre = np.zeros((2,) + gray[-1][0].shape)
    flows = []
    for l in range(numPyd, 0, -1):
        hints = mvPre
        mc, fl = oracle.calc_pyd_cost_sgm_ng(gray[l - 1][0], gray[l - 1][1], mvPre, half, agg, sub, P1, P2)
        flows.append(fl)
        if l > 1:
            mvPre = level_hints(fl, s)
    return flows, mc, hints
