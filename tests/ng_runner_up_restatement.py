"""numpy restatement of the neighbour-guided matcher's runner-up cost, straight from its definition (include/fsgm.h), on the
oracle's volumes calc_pyd_cost_sgm_ng(..., want_volumes=True) -> (minC, flow, Cc, S):

    S[d], (mvx_d, mvy_d)   the u32 sum and the integer motion vector of candidate d of a pixel, d = 0 .. D-1
    best = the first minimum of S over d;  (bx, by) its vector;  minC = S[best]
    minC2 = min { S[d] : max(|mvx_d - bx|, |mvy_d - by|) >= 2 },  NO_RUNNER_UP where that set is empty

The distance is between motion vectors (taken in Python-sized integers: |mv| goes up to 2^31), never between list indices.
The pipeline restatement applies the uniqueness test of runner_up_restatement to the forward and to the backward flow, each
with its own costs, and hands both to flow_pp_restatement.chain.
"""
import numpy as np

from tests import flow_pp_restatement
from tests.runner_up_restatement import NO_RUNNER_UP, uniqueness_reject
from tests.runner_up2d_restatement import uniqueness_filter_flow


def ng_runner_up(mvx, mvy, S):
    """(best, minC, minC2) of S[..., D] with the candidates' vectors mvx, mvy [..., D]: int64 index, uint32 costs"""
    S = np.asarray(S)
    mvx, mvy = np.asarray(mvx).astype(np.int64), np.asarray(mvy).astype(np.int64)
    best = np.argmin(S, axis=-1)                                 # (numpy's argmin: the first minimum)
    pick = lambda a: np.take_along_axis(a, best[..., None], axis=-1)          # noqa: E731
    far = np.maximum(np.abs(mvx - pick(mvx)), np.abs(mvy - pick(mvy))) >= 2   # (|a - b| < 2^32: exact in int64)
    masked = np.where(far, S.astype(np.uint64), np.uint64(NO_RUNNER_UP))
    return best.astype(np.int64), pick(S)[..., 0].astype(np.uint32), masked.min(axis=-1).astype(np.uint32)


def ng_runner_up_of_volumes(Cc, S):
    """the same from the oracle's candidate volume (fields mvx, mvy, cost) and sums"""
    return ng_runner_up(Cc["mvx"], Cc["mvy"], S)


def flow_pp_u(fwd, bwd, cf, c2f, cb, c2b, ratio, **chain):
    """(flow_pp, flow_checked, reject masks) of the pipeline with a uniqueness ratio: both directions are blanked by their own
    (minC, minC2) ahead of the chain's first speckle filter; ratio 0 rejects nothing"""
    f = uniqueness_filter_flow(fwd, cf, c2f, ratio)
    b = uniqueness_filter_flow(bwd, cb, c2b, ratio)
    return flow_pp_restatement.chain(f, b, **chain)


__all__ = ["NO_RUNNER_UP", "uniqueness_reject", "ng_runner_up", "ng_runner_up_of_volumes", "flow_pp_u"]
