"""Plain-numpy restatement of the filtered-flow chain for the pyramidal matchers (test yardstick, no GPU code).

Written from the reference's MATLAB files -- speckle_filter.m, forward_backward_check.m, scanline_in_fill.m, test.m:45-49 --
with the rules that extend them from a scalar map to a two-channel flow (include/fsgm.h, "Consistency-checked, filtered
flow").  Flows are (2, H, W) float64, plane 0 = u (x); a pixel is valid when neither channel is NaN.  The speckle filter is
the reference's flood fill (a FIFO queue from each raster-order seed), not the library's union-find.
"""
from collections import deque

import numpy as np


def matlab_round(x):
    """MATLAB's round: half away from zero (numpy's rounds half to even).  x - trunc(x) is exact in fp64."""
    x = np.asarray(x, np.float64)
    t = np.trunc(x)
    with np.errstate(invalid="ignore"):
        return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def valid(flow):
    return ~np.isnan(flow[0]) & ~np.isnan(flow[1])


def flow_speckle_filter(flow, maxDiff=2.0, maxSpeckleSize=100.0):
    """speckle_filter.m:22-99 with the neighbour test of :55 on vectors: |du| < maxDiff and |dv| < maxDiff.
    Returns (filtered flow, mask of the pixels it dropped)."""
    flow = np.asarray(flow, np.float64)
    _, H, W = flow.shape
    ok = valid(flow)
    u, v = flow
    with np.errstate(invalid="ignore"):
        # the test of :54-55 / :74-75 for every pixel and its right / bottom neighbour (the left / top tests are these seen
        # from the other side: the relation is symmetric)
        right = np.zeros((H, W), bool)
        right[:, :-1] = ok[:, :-1] & ok[:, 1:] & (np.abs(u[:, :-1] - u[:, 1:]) < maxDiff) & (np.abs(v[:, :-1] - v[:, 1:]) < maxDiff)
        down = np.zeros((H, W), bool)
        down[:-1] = ok[:-1] & ok[1:] & (np.abs(u[:-1] - u[1:]) < maxDiff) & (np.abs(v[:-1] - v[1:]) < maxDiff)
    right, down, okf = right.ravel().tolist(), down.ravel().tolist(), ok.ravel().tolist()
    labelled = [False] * (H * W)
    dropped = np.zeros(H * W, bool)
    for seed in range(H * W):                                   # :23-24, raster order
        if not okf[seed] or labelled[seed]:
            continue
        labelled[seed] = True
        queue, region = deque([seed]), []                       # :33-36
        while queue:                                            # :44
            i = queue.popleft()
            region.append(i)                                    # :48 regionPixelNum
            x = i % W
            if x + 1 < W and right[i] and not labelled[i + 1]:          # :52-60
                labelled[i + 1] = True
                queue.append(i + 1)
            if x > 0 and right[i - 1] and not labelled[i - 1]:          # :63-70
                labelled[i - 1] = True
                queue.append(i - 1)
            if i + W < H * W and down[i] and not labelled[i + W]:       # :73-80
                labelled[i + W] = True
                queue.append(i + W)
            if i >= W and down[i - W] and not labelled[i - W]:          # :83-90
                labelled[i - W] = True
                queue.append(i - W)
        if float(len(region)) < maxSpeckleSize:                 # :94
            dropped[region] = True
    dropped = dropped.reshape(H, W)
    out = flow.copy()
    out[:, dropped] = np.nan
    return out, dropped


def flow_fb_check(f, b, thr=2.0):
    """forward_backward_check.m:8-37 with p2 = round(p + f(p)) for :15-20 (p 1-based).  Returns (checked f, dict of the masks
    of the pixels rejected as 'outside' (:22), 'partner' (:27) and 'mismatch' (:32))."""
    f, b = np.asarray(f, np.float64), np.asarray(b, np.float64)
    _, H, W = f.shape
    jj, ii = np.mgrid[1:H + 1, 1:W + 1].astype(np.float64)     # MATLAB's j (row), i (column)
    ok = valid(f)                                               # :12
    with np.errstate(invalid="ignore"):
        p2x, p2y = matlab_round(ii + f[0]), matlab_round(jj + f[1])            # :20
        outside = ok & ((p2x < 1) | (p2x > W) | (p2y < 1) | (p2y > H))         # :22
        walk = ok & ~outside
        tx, ty = np.where(walk, p2x, 1).astype(np.int64) - 1, np.where(walk, p2y, 1).astype(np.int64) - 1
        bu, bv = b[0, ty, tx], b[1, ty, tx]
        partner = walk & (np.isnan(bu) | np.isnan(bv))                         # :27
        mismatch = walk & ~partner & ((np.abs(f[0] + bu) > thr) | (np.abs(f[1] + bv) > thr))   # :32
    why = {"outside": outside, "partner": partner, "mismatch": mismatch}
    out = f.copy()
    out[:, outside | partner | mismatch] = np.nan
    return out, why


def flow_in_fill(flow):
    """scanline_in_fill.m:2-70 with lines 16 and 19 restored; isnan(input(v, u)) of a 3-D array tests its first plane."""
    a = np.array(flow, np.float64)
    _, H, W = a.shape
    for v in range(H):                                          # :6
        count = 0
        for u in range(W):
            if not np.isnan(a[0, v, u]):
                if count >= 1:
                    u1, u2 = u - count, u - 1                   # 0-based first / last column of the gap
                    if u1 > 0 and u2 < W - 1:                   # :14
                        a[0, v, u1:u2 + 1] = np.fmin(a[0, v, u1 - 1], a[0, v, u2 + 1])     # :15, :18 (min skips a NaN)
                        a[1, v, u1:u2 + 1] = np.fmin(a[1, v, u1 - 1], a[1, v, u2 + 1])     # :16, :19
                count = 0
            else:
                count += 1
        for u in range(W):                                      # :30-37
            if not np.isnan(a[0, v, u]):
                a[:, v, :u] = a[:, v, u:u + 1]
                break
        for u in range(W - 1, -1, -1):                          # :39-46
            if not np.isnan(a[0, v, u]):
                a[:, v, u + 1:] = a[:, v, u:u + 1]
                break
    for u in range(W):                                          # :50
        for v in range(H):                                      # :52-59
            if not np.isnan(a[0, v, u]):
                a[:, :v, u] = a[:, v:v + 1, u]
                break
        for v in range(H - 1, -1, -1):                          # :61-68
            if not np.isnan(a[0, v, u]):
                a[:, v + 1:, u] = a[:, v:v + 1, u]
                break
    return a


def island_threshold(H, W, island_fraction):
    return float(H * W) * island_fraction                       # test.m:48 rows*cols/10, never rounded


def chain(f, b, speckle_max_diff=2.0, speckle_max_size=100.0, fb_thr=2.0, island_fraction=0.1):
    """test.m:45-49 on the forward flow f with the backward flow b.  Returns (flow_pp (3, H, W), checked flow (2, H, W),
    dict of reject masks: 'speckle' (either speckle pass, on f) and flow_fb_check's three)."""
    _, H, W = f.shape
    fs, d1 = flow_speckle_filter(f, speckle_max_diff, speckle_max_size)       # :45
    bs, _ = flow_speckle_filter(b, speckle_max_diff, speckle_max_size)
    c, why = flow_fb_check(fs, bs, fb_thr)                                     # :47
    c, d2 = flow_speckle_filter(c, np.inf, island_threshold(H, W, island_fraction))   # :48
    why["speckle"] = d1 | d2
    g = flow_in_fill(c)                                                        # :49
    return np.concatenate([g, valid(c)[None].astype(np.float64)]), c, why     # :53
