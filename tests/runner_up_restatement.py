"""numpy restatement of the runner-up cost and the uniqueness test, straight from their definition (include/fsgm.h):

    best  = the first strict minimum of S[0 .. D-1]          (the WTA's index)
    minC  = S[best]
    minC2 = min { S[d] : |d - best| >= 2 },  NO_RUNNER_UP where that set is empty
    reject  <=>  minC2 != NO_RUNNER_UP  and  minC2 * (100 - ratio) < minC * 100        (exact integers)
"""
import numpy as np

NO_RUNNER_UP = 0xFFFFFFFF


def runner_up(S):
    """(best, minC, minC2) of S[..., D]: int64 index, uint32 costs"""
    S = np.asarray(S)
    D = S.shape[-1]
    best = np.argmin(S, axis=-1)                                 # (numpy's argmin: the first minimum)
    minC = np.take_along_axis(S, best[..., None], axis=-1)[..., 0]
    far = np.abs(np.arange(D) - best[..., None]) >= 2
    masked = np.where(far, S.astype(np.uint64), np.uint64(NO_RUNNER_UP))
    minC2 = masked.min(axis=-1) if D else np.full(S.shape[:-1], NO_RUNNER_UP, np.uint64)
    return best.astype(np.int64), minC.astype(np.uint32), minC2.astype(np.uint32)


def uniqueness_reject(minC, minC2, ratio):
    """boolean mask of the rejected pixels; Python integers, so no product can overflow"""
    minC, minC2 = np.asarray(minC), np.asarray(minC2)
    c = minC.astype(object).ravel()
    c2 = minC2.astype(object).ravel()
    out = [int(b) != NO_RUNNER_UP and int(b) * (100 - int(ratio)) < int(a) * 100 for a, b in zip(c, c2)]
    return np.array(out, bool).reshape(minC.shape)


def uniqueness_filter(map_, minC, minC2, ratio):
    out = np.array(map_, np.float64, copy=True)
    out[uniqueness_reject(minC, minC2, ratio)] = np.nan
    return out
