"""GPU parity tests of the band sweeps' DP step (fsgm_amd/csrc/epi_band.hip, step_x): the costs' bias folded into the
subtraction (n' = (YB ^ 0x7F) + C), the final pass's S rebuilt from its own paths' n' and the first pass's sums, and the
from-above-left states / load rings walked two steps an iteration.  Against the CPU oracle: S of every voxel (debug tap),
bestD and minC of every pixel, for

  * the edges of the first pass's sums: sum(y) = 0 (far from a strong minimum), 255 / 256 (4 * P2 = 256: every path starts
    at the frame's first pixel and y = P2 there, at every d of every lane), and sums across the whole 9-bit range;
  * P1 = 0, P1 = P2, P1 + P2 = 127, at the largest cost band_ok accepts;
  * frame widths whose walks end the two-step loop on an odd and on an even step;
  * 8 and 4 paths, the sequential (mode 4) and the chained (mode 5) form."""
import numpy as np
import pytest

from fsgm_amd import synth, EpiPlan
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA

pytestmark = pytest.mark.gpu


def _cmax(paths, P1, P2):
    # the largest C the band sweeps accept: no wrap (C + P2 + max(P1, P2) <= 255, the plan's choice) and band_ok's
    # 16 * paths * (C + P2 + P1) + 15 < 0x7C00
    return min(255 - P2 - max(P1, P2), (0x7C00 - 16) // (16 * paths) - (P1 + P2))


def _volumes(W, H, D, B, cmax, seed):
    vols = []
    for f in range(B):
        v = synth.cost_volume(W, H, D, seed=seed + f, cmax=cmax)
        if f % 2 == 0:
            v[:, ::5, :] = 0                                 # strong structure: paths carry information far
        else:                                                # one strong minimum a pixel: y = 0 far from it, P2 at it
            v[...] = cmax
            d0 = (np.arange(W * H).reshape(H, W) * 7) % D
            np.put_along_axis(v, d0[..., None], 0, axis=2)
        vols.append(np.ascontiguousarray(v))
    return vols


def _run_and_check(oracle, W, H, D, B, paths, P1, P2, cmax, mode, seed=11):
    vols = _volumes(W, H, D, B, cmax, seed)
    _, _, off = synth.epi_maps(W, H, "general", seed=5)
    with EpiPlan(W, H, D, B, paths=paths) as plan:
        plan.set_penalties(P1, P2, 0.3)
        for f in range(B):
            plan.upload_cost(f, vols[f])
            plan.upload_offset(f, off)
        plan.set_agg_mode(mode)
        assert plan.kernel_name == ("band16/nowrap" if mode == 4 else "band16chain/nowrap")
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        for f in range(B):
            S = oracle.epi_aggregate(vols[f], P1, P2, paths)
            bd, mc = oracle.epi_wta(S, W, H, D, 1)
            np.testing.assert_array_equal(plan.download_sum(f), S[:-1].reshape(H, W, D), err_msg=f"frame {f} S")
            gbd, gmc = plan.download(f)
            np.testing.assert_array_equal(gmc, mc, err_msg=f"frame {f} minC")
            np.testing.assert_array_equal(gbd, oracle.epi_vz_to_disp(bd, off, 0.3, D + 1), err_msg=f"frame {f} bestD")
        plan.sync()


PENALTIES = [
    (6, 64),      # the headline: 4 * P2 = 256, the first pass's sums reach their 9th bit
    (0, 64),      # P1 = 0
    (0, 127),     # P1 + P2 = 127, sums up to 508
    (63, 64),     # P1 + P2 = 127
    (40, 40),     # P1 = P2
    (0, 0),
    (5, 63),      # 4 * P2 = 252: the sums stay below 256
]


@pytest.mark.parametrize("mode", [4, 5])
@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("P1,P2", PENALTIES)
def test_band_step_penalties_at_the_largest_cost(gpu_lib, oracle, P1, P2, paths, mode):
    _run_and_check(oracle, 53, 70, 128, 2, paths, P1, P2, _cmax(paths, P1, P2), mode)


@pytest.mark.parametrize("mode", [4, 5])
@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("W", [40, 41, 1, 2, 3])
def test_band_step_walk_lengths(gpu_lib, oracle, W, paths, mode):
    """The walk has W + SKEW * (rows - 1) steps: odd and even counts end the two-step loop on either step."""
    for H in (30, 31, 64, 65):
        _run_and_check(oracle, W, H, 128, 1, paths, 6, 64, 24, mode, seed=W + H)
