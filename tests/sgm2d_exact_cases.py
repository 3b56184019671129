"""The inputs of tests/test_gpu_sgm2d_exact.py, shared with tests/test_sgm2d_exact_cpu.py, which proves on the CPU that each of
them lies where the exact recurrence and the mod-256 one differ.  Everything is generated from seeds; the yardstick
(tests/sgm2d_exact_restatement.py) is computed once per case and left unchanged."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import sgm2d_exact_restatement as X

LAYOUTS = ("hwd", "dhw", "dhw_yx")
# (halfX, halfY): 1x1, 3x3, 9x9 (rows layout), 5x11 (rows layout with row padding: RS 12, Sy 11), 13x13 (compact, NCMAX 4),
# 17x17 (compact, NCMAX 16)
WINDOWS = [(0, 0), (1, 1), (4, 4), (2, 5), (6, 6), (8, 8)]
PENALTIES = [(7, 100), (20, 200), (255, 255), (0, 0)]
IMAGES = [(21, 13), (7, 5), (1, 9), (9, 1)]                      # (W, H)
HINTS = (None, "general", "beyond")

Case = namedtuple("Case", "W H rX rY n P1 P2 layout hints adaptive diagonal passes subpixel volume")


def _cases():
    out = []
    k = 0
    for i, (rX, rY) in enumerate(WINDOWS):                       # every window at every penalty pair on the largest image
        for j, (P1, P2) in enumerate(PENALTIES):
            out.append(Case(21, 13, rX, rY, 3 if (i + j) % 2 else 1, P1, P2, LAYOUTS[k % 3], HINTS[(k // 3) % 3], int(k % 4 == 1),
                            int(k % 5 != 2), 1 if k % 7 == 3 else 2, int(k % 6 != 4), "random"))
            k += 1
    for W, H in IMAGES[1:]:                                      # every window on the small and the degenerate images
        for i, (rX, rY) in enumerate(WINDOWS):
            P1, P2 = PENALTIES[k % 3]
            out.append(Case(W, H, rX, rY, 3 if k % 2 else 1, P1, P2, LAYOUTS[k % 3], HINTS[(k // 2) % 3], int(k % 4 == 2), int(k % 5 != 0),
                            1 if k % 7 == 5 else 2, int(k % 6 != 1), "random"))
            k += 1
    for rX, rY in ((4, 4), (6, 6)):                              # the all-255 volume: L = 510 at each path's second pixel with P2 = 255
        for P1, P2 in ((255, 255), (7, 100)):
            out.append(Case(21, 13, rX, rY, 1, P1, P2, "dhw", None, 0, 1, 2, 1, "all255"))
    # one-switch variants of one rows-layout and one compact case: diagonal off, one pass, no sub-pixel, adaptive with hints beyond
    for rX, rY in ((4, 4), (6, 6)):
        out.append(Case(21, 13, rX, rY, 1, 7, 100, "dhw_yx", "general", 0, 0, 2, 1, "random"))
        out.append(Case(21, 13, rX, rY, 1, 7, 100, "hwd", "general", 0, 1, 1, 1, "random"))
        out.append(Case(21, 13, rX, rY, 3, 20, 200, "dhw", "general", 0, 1, 2, 0, "random"))
        out.append(Case(21, 13, rX, rY, 3, 20, 200, "dhw", "beyond", 1, 1, 2, 1, "random"))
    return out


CASES = _cases()


def case_id(c):
    return (f"{c.W}x{c.H}-{2 * c.rX + 1}x{2 * c.rY + 1}-n{c.n}-P{c.P1}_{c.P2}-{c.layout}-{c.hints or 'nohints'}"
            f"-a{c.adaptive}d{c.diagonal}p{c.passes}s{c.subpixel}-{c.volume}")


def outside_budget(c):
    """the no-wrap budget of the plain kernels, with the costs up to 255 every case holds"""
    return 255 + c.P2 + max(c.P1, c.P2) > 255


def volumes(W, H, D, n, seed, kind="random"):
    """(n, H, W, D) uint8 in reference order: uniform bytes 0..255, or all 255.  The first frame's first pixel holds 255 and its
    right and lower neighbours at least 200: they follow a path start (stored minimum 0), so L = C + min(Lp, P2, ..) >= 300 there
    at every P2 >= 100 whatever the draw -- on a 9x1 image with a 1x1 window no other pixel can leave a byte."""
    if kind == "all255":
        return np.full((n, H, W, D), 255, np.uint8)
    v = np.random.default_rng(seed).integers(0, 256, (n, H, W, D), dtype=np.uint8)
    v[0, 0, 0] = 255
    v[0, 0, min(1, W - 1)] = np.maximum(v[0, 0, min(1, W - 1)], 200)
    v[0, min(1, H - 1), 0] = np.maximum(v[0, min(1, H - 1), 0], 200)
    return v


def hints(kind, W, H, rX, rY, n, seed):
    """(n, 2, mvH, mvW) float64, larger than the image.  "general": steps of up to +-3 between neighbours, fractions included;
    "beyond": some steps that shift the centre farther than the window and its 5x5 reach, on top of them"""
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    mv = rng.uniform(-1.5, 1.5, (n, 2, H + 2, W + 3))
    mv[:, :, ::2, ::3] += 0.5                                    # exact halves: the truncation of :46-47 at a tie
    if kind == "beyond":
        far = rng.random((n, 2, H + 2, W + 3)) < 0.15
        mv = np.where(far, mv + np.array([2 * rX + 6.0, -(2 * rY + 6.0)])[None, :, None, None], mv)
    return np.ascontiguousarray(mv)


def guides(W, H, n, seed):
    """(n, H, W) uint8 with a 120-step edge down the middle and small steps elsewhere: |dI| of 120 (> 50) and of <= 20"""
    g = np.random.default_rng(seed).integers(0, 21, (n, H, W)).astype(np.uint8) + 40
    g[:, :, W // 2:] += 120
    g[:, H // 2:, :] += 60                                       # (a second edge, across the vertical and diagonal paths: 60 > 50)
    return g


def as_layout(layout, vols, Sx, Sy):
    """the same volumes as the caller of that layout holds them"""
    n, H, W, D = vols.shape
    if layout == "hwd":
        return vols
    if layout == "dhw":
        return np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
    return np.ascontiguousarray(vols.reshape(n, H, W, Sx, Sy).transpose(0, 4, 3, 1, 2).reshape(n, D, H, W))


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(vols, hints, guides) of a case; arrays that every user leaves unchanged"""
    Sx, Sy = 2 * c.rX + 1, 2 * c.rY + 1
    seed = zlib.crc32(repr(tuple(c)).encode()) % 100000
    v = volumes(c.W, c.H, Sx * Sy, c.n, seed, c.volume)
    h = hints(c.hints, c.W, c.H, c.rX, c.rY, c.n, 1000 + seed)
    g = guides(c.W, c.H, c.n, 2000 + seed) if c.adaptive else None
    for a in (v, h, g):
        if a is not None:
            a.setflags(write=False)
    return v, h, g


@functools.lru_cache(maxsize=None)
def want(c, bound=255):
    """(bestD, minC, mvSub, flow, S, minC2) of the restatement for every frame of the case, the costs saturated at `bound`"""
    v, h, g = inputs(c)
    out = X.sgm2d_batch(np.minimum(v, bound), c.rX, c.rY, c.P1, c.P2, h, g, diagonal=c.diagonal, totalPass=c.passes, subpixel=c.subpixel)
    for a in out:
        a.setflags(write=False)
    return out
