"""Synthetic forward / backward flow pairs for the filtered-flow tests: a smooth field that is consistent over most of the
image, with every way of being rejected planted in it (seeded, no GPU code)."""
import numpy as np

from fsgm_amd import synth


def flow_pair(W, H, kind="general", seed=5):
    """(f, b), each (2, H, W) float64.  f: a smooth quarter-step field; isolated outliers drawn from synth.hint_map(kind)
    (speckles); NaN holes; strips along all four edges that point out of the image; exact halves in p + f.  b: minus f at
    f's target pixel, so that most pixels are consistent; a block left unreached and a block of NaN (invalid partners);
    a 12x12 block off by exactly thr = 2 (kept: the test is >) and one off by 2.25 (mismatch), each large enough to survive
    the speckle filter as a region of its own."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.stack([np.round((2.5 * np.sin(xx / 37.0) * np.cos(yy / 29.0) + 1.0) * 4) / 4,
                  np.round((1.5 * np.cos(xx / 41.0) + 0.5 * np.sin(yy / 23.0)) * 4) / 4])
    f[0, 1::7, 2::9] += 0.5 - np.mod(f[0, 1::7, 2::9], 1.0)                   # x + f_u = k + 0.5
    out = synth.hint_map(W, H, kind, seed=seed, amp=9.0)
    speck = synth.uniform_f64(seed + 1, (H, W)) < 0.03
    f[:, speck] = f[:, speck] + out[:, speck] + 4.0
    if H > 8 and W > 8:
        f[0, :, :2] = -3.0                                                     # out of the left edge
        f[0, :, -2:] = 3.5                                                     # the right
        f[1, :2, :] = -2.5                                                     # the top (-(k + 0.5) for row 2)
        f[1, -2:, :] = 4.0                                                     # the bottom
    hole = synth.uniform_f64(seed + 2, (H, W)) < 0.04
    if H > 8 and W > 8:
        hole[H // 3, W // 4: W // 2] = True
    f[:, hole] = np.nan
    f[1, synth.uniform_f64(seed + 3, (H, W)) < 0.002] = np.nan                # only one channel missing

    b = np.full((2, H, W), np.nan)
    r = lambda a: np.trunc(a) + np.where(np.abs(a - np.trunc(a)) >= 0.5, np.sign(a), 0.0)   # noqa: E731
    ok = ~np.isnan(f[0]) & ~np.isnan(f[1])
    tx = np.where(ok, r(xx + 1 + np.nan_to_num(f[0])), 0).astype(np.int64) - 1
    ty = np.where(ok, r(yy + 1 + np.nan_to_num(f[1])), 0).astype(np.int64) - 1
    inside = ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    for c in range(2):
        b[c, ty[inside], tx[inside]] = -f[c][inside]
    b[:, np.isnan(b[0])] = 0.0 if kind == "zero" else np.nan                   # unreached targets
    if H > 8 and W > 8:
        b[:, H // 2: H // 2 + 3, W // 2: W // 2 + 5] = np.nan                  # invalid partners
        b[0, H // 4: H // 4 + 12, W // 3: W // 3 + 12] += 2.0                   # |sum| = thr exactly where it was 0
        b[1, 3 * H // 4 - 12: 3 * H // 4, W // 5: W // 5 + 12] -= 2.25         # mismatch in v only
    return np.ascontiguousarray(f), np.ascontiguousarray(b)
