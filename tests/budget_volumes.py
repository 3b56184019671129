"""Penalty sets and cost volumes at the edges of the fused pipelines' byte budgets (choose_pipeline, fsgm_amd/csrc/capi_epi.hip),
shared by tests/test_gpu_fused_budgets.py (the kernels against the oracle) and tests/test_oracle_epi.py (the oracle against the
second restatement).

The block sweeps (8 paths) keep y + P1 per path and sum three of them into a byte: 3 * (P1 + P2) <= 255.  The pair kernels
(4 paths) sum two: 2 * (P1 + P2) <= 255.  Both need 0 <= P1 <= P2 and no wrap: cm + P2 + max(P1, P2) <= 255."""
import numpy as np

from fsgm_amd import synth

# 8 paths: sweep16 / sweep16par / sweep16mid
SWEEP_PENALTIES = [
    (21, 64),     # 3 * (P1 + P2) = 255 at the headline P2
    (42, 43),     # 255 with P1 ~ P2
    (0, 85),      # 255 with P1 = 0
    (28, 57),     # 255 with neither penalty small
    (1, 1),
    (0, 0),       # cmax = 255: S reaches 8 * 255 = 2040, the WTA keys' documented limit
    (6, 32),      # the shipped pyramidal set at a correlation layer's costs
]
# 4 paths: pairs16
PAIR_PENALTIES = [
    (63, 64),     # P1 + P2 = 127
    (0, 127),     # P1 + P2 = 127 with P1 = 0
    (40, 40),     # P1 = P2
    (6, 64),
    (21, 64),
    (0, 0),
]
KINDS = ("uniform", "columns", "minimum", "constant", "zeros")


def nowrap_cmax(P1, P2):
    """The largest cost choose_pipeline accepts as no-wrap: cm + P2 + max(P1, P2) <= 255."""
    return 255 - P2 - max(P1, P2)


def volume(kind, W, H, D, cmax, seed):
    """(H, W, D) uint8 with maximum cmax (all zeros: 0):
    uniform   synth.cost_volume, uniform in [0, cmax];
    columns   the same with every fifth column zeroed: paths carry information far;
    minimum   cmax everywhere, 0 at d0 = 7 * pixel mod D: y = 0 far from the minimum and P2 at it;
    constant  cmax everywhere: from the third pixel of a path on y = P2 at every d, the largest sum bytes, and every d ties;
    zeros     all zeros."""
    if kind == "uniform" or kind == "columns":
        v = synth.cost_volume(W, H, D, seed=seed, cmax=cmax)
        if kind == "columns":
            v[:, ::5, :] = 0
    elif kind == "minimum":
        v = np.full((H, W, D), cmax, np.uint8)
        d0 = (np.arange(W * H).reshape(H, W) * 7) % D
        np.put_along_axis(v, d0[..., None], 0, axis=2)
    elif kind == "constant":
        v = np.full((H, W, D), cmax, np.uint8)
    elif kind == "zeros":
        v = np.zeros((H, W, D), np.uint8)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(v)


def volumes(W, H, D, cmax, seed, n=len(KINDS)):
    """n frames: the five kinds in turn, every frame with a seed of its own."""
    return [volume(KINDS[f % len(KINDS)], W, H, D, cmax, seed + f) for f in range(n)]


def sweep_shape(D):
    """The smallest frame that crosses one column-strip and one row-block boundary of the block sweeps (epi_sweep.hip: a wave owns
    PXW = 1024 / D columns, a workgroup's strip is 4 * PXW columns, a launch's block 2 * PXW rows)."""
    pxw = 1024 // D
    return 4 * pxw + 3, 2 * pxw + 5
