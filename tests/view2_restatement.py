"""The second view's rule (include/fsgm.h, "Second view") restated in vectorised numpy on a given S, and the left-right check.
Not a test module: tests import it.  S is (..., H, W, D) uint32 as fsgm_epi_plan_download_sum returns it."""
import numpy as np

NO_VIEW2 = np.uint32(0xFFFFFFFF)
INT32_MIN = np.int32(-2 ** 31)


def view2(S, direction, d_min=0, subpixel=1):
    """(disp2, minC_v2), uint32 (..., H, W): disp2 in index units * 256, NO_VIEW2 where no candidate lies in the image."""
    S = np.asarray(S, np.uint32)
    W, D = S.shape[-2], S.shape[-1]
    s = int(direction)
    x2 = np.arange(W)[:, None]
    i = np.arange(D)[None, :]
    x = x2 - s * (int(d_min) + i)                                # (W, D): the first-view column of candidate i of x2
    ok = (x >= 0) & (x < W)
    diag = S[..., np.clip(x, 0, W - 1), i].astype(np.int64)      # (..., H, W, D): S[y][x2 - s*delta(i)][i]
    BIG = np.int64(1) << 40
    diag = np.where(ok, diag, BIG)
    best = np.argmin(diag, axis=-1)                              # the first minimum
    c = np.take_along_axis(diag, best[..., None], -1)[..., 0]
    none = c >= BIG
    disp2 = (best * 256).astype(np.int64)
    if subpixel:
        lo, hi = np.clip(best - 1, 0, D - 1), np.clip(best + 1, 0, D - 1)
        okb = np.broadcast_to(ok, diag.shape)
        sub_ok = (best >= 1) & (best + 1 < D) & ~none
        sub_ok &= np.take_along_axis(okb, lo[..., None], -1)[..., 0] & np.take_along_axis(okb, hi[..., None], -1)[..., 0]
        c_1 = np.take_along_axis(diag, lo[..., None], -1)[..., 0].astype(np.float64)
        c1 = np.take_along_axis(diag, hi[..., None], -1)[..., 0].astype(np.float64)
        cf = c.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            off = np.where(c1 < c_1, ((c1 - c_1) / (cf - c_1)) / 2.0, ((c1 - c_1) / (cf - c1)) / 2.0)
            val = (best.astype(np.float64) + off) * 256.0
        disp2 = np.where(sub_ok, np.trunc(np.where(sub_ok, val, 0.0)).astype(np.int64), disp2)
    disp2 = np.where(none, np.int64(NO_VIEW2), disp2).astype(np.uint32)
    minc = np.where(none, np.int64(NO_VIEW2), c).astype(np.uint32)
    return disp2, minc


def to_true(disp2, d_min):
    """The stereo forms' int32 true disparities * 256 of a disp2 in index units (INT32_MIN where invalid)."""
    v = disp2.astype(np.int64) + 256 * int(d_min)
    return np.where(disp2 == NO_VIEW2, np.int64(INT32_MIN), v).astype(np.int32)


def check(d1, d2, valid2, direction, max_diff=256):
    """conf uint8 (..., H, W) of true disparities * 256 d1, d2 (integers, any width) and the validity mask of d2."""
    d1 = np.asarray(d1).astype(np.int64)
    d2 = np.asarray(d2).astype(np.int64)
    W = d1.shape[-1]
    x2 = np.arange(W) + int(direction) * ((d1 + 128) >> 8)
    inside = (x2 >= 0) & (x2 < W)
    xc = np.clip(x2, 0, W - 1)
    d2x = np.take_along_axis(d2, xc, -1)
    v2x = np.take_along_axis(np.asarray(valid2, bool), xc, -1)
    return (inside & v2x & (np.abs(d1 - d2x) <= int(max_diff))).astype(np.uint8)


def check_sgm(bestD, disp2, direction, d_min=0, max_diff=256, subpixel=1):
    """The sgm(C) forms' check: bestD and disp2 uint32 in index units (a call without sub-pixel returns bestD as the whole index)."""
    add = 256 * int(d_min)
    d1 = bestD.astype(np.int64) * (1 if subpixel else 256)
    return check(d1 + add, disp2.astype(np.int64) + add, disp2 != NO_VIEW2, direction, max_diff)


def check_true(disp, disp2, direction, max_diff=256):
    """The stereo forms' and the stand-alone check: int32 true disparities, disp2's marker INT32_MIN."""
    return check(disp, disp2, np.asarray(disp2) != INT32_MIN, direction, max_diff)


def brute(S, direction, d_min=0, subpixel=1):
    """The rule as a triple loop on one frame S (H, W, D), Python integers and floats."""
    H, W, D = S.shape
    disp2 = np.empty((H, W), np.uint32)
    minc = np.empty((H, W), np.uint32)
    for y in range(H):
        for x2 in range(W):
            cand = [i for i in range(D) if 0 <= x2 - direction * (d_min + i) < W]
            if not cand:
                disp2[y, x2] = minc[y, x2] = NO_VIEW2
                continue
            val = {i: int(S[y, x2 - direction * (d_min + i), i]) for i in cand}
            b = min(cand, key=lambda i: (val[i], i))
            v = b * 256
            if subpixel and (b - 1) in val and (b + 1) in val:
                c_1, c, c1 = float(val[b - 1]), float(val[b]), float(val[b + 1])
                off = ((c1 - c_1) / (c - c_1)) / 2.0 if c1 < c_1 else ((c1 - c_1) / (c - c1)) / 2.0
                v = int((b + off) * 256.0)
            disp2[y, x2], minc[y, x2] = v, val[b]
    return disp2, minc
