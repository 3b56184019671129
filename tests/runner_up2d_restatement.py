"""numpy restatement of the 2-D matcher's runner-up cost, straight from its definition (include/fsgm.h):

    S[sx*Sy + sy]  the u32 sums the WTA minimises, candidate order x-slow
    best = bx*Sy + by, the first strict minimum in candidate order;  minC = S[best]
    minC2 = min { S[sx*Sy + sy] : max(|sx - bx|, |sy - by|) >= 2 },  NO_RUNNER_UP where that set is empty

The uniqueness test on (minC, minC2) is runner_up_restatement.uniqueness_reject; on a flow both planes of a rejected pixel go.
"""
import numpy as np

from tests.runner_up_restatement import NO_RUNNER_UP, uniqueness_reject


def runner_up2d(S, Sx, Sy):
    """(best, minC, minC2) of S[..., Sx*Sy]: int64 index, uint32 costs"""
    S = np.asarray(S)
    assert S.shape[-1] == Sx * Sy
    best = np.argmin(S, axis=-1)                                 # (numpy's argmin: the first minimum)
    minC = np.take_along_axis(S, best[..., None], axis=-1)[..., 0]
    d = np.arange(Sx * Sy)
    far = np.maximum(np.abs(d // Sy - (best // Sy)[..., None]), np.abs(d % Sy - (best % Sy)[..., None])) >= 2
    masked = np.where(far, S.astype(np.uint64), np.uint64(NO_RUNNER_UP))
    return best.astype(np.int64), minC.astype(np.uint32), masked.min(axis=-1).astype(np.uint32)


def uniqueness_filter_flow(flow, minC, minC2, ratio):
    """flow (..., 2, H, W) with NaN in both planes where (minC, minC2) (..., H, W) fail the test"""
    out = np.array(flow, np.float64, copy=True)
    rej = uniqueness_reject(minC, minC2, ratio)
    np.moveaxis(out, -3, 0)[:, rej] = np.nan
    return out
