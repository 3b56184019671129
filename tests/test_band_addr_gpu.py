"""GPU parity tests of the band sweeps' carried addresses (fsgm_amd/csrc/epi_band.hip): the prefetch offset advanced by
+-D a step and clamped against the row's two ends, the first pass's store offset and both passes' bit-plane offset taken
from that register.  Every case runs the band sweeps (mode 4, or 5 for the chained form) and the per-direction line
kernels (mode 1) on the same volumes and compares bestD and minC of every pixel of every frame exactly; frame 0 also
against the CPU oracle.  Shapes: one-, two- and three-pixel-wide frames (every step an edge step, the prefetch past the
row end from step one), a plain interior longer than the unrolled loop plus a tail (W = 130), heights up to, at and
across the band boundaries (the offsets restart per band), with the 9th-bit plane (P2 = 64) and without it (P2 = 32),
every D with its own rows per band, 8 and 4 paths, three frames with distinct volumes."""
import numpy as np
import pytest

from fsgm_amd import synth, EpiPlan
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA

pytestmark = pytest.mark.gpu

BAND_NAME = {4: "band16/nowrap", 5: "band16chain/nowrap"}


def _band_rows(D):
    return 8 * 64 // (D // 16)                               # band_rows(D): 8 waves of 64 / LPP rows, LPP = D / 16


def _cmax(paths, P1, P2):
    # the largest C the band sweeps accept: no wrap (C + P2 + max(P1, P2) <= 255, the plan's choice) and band_ok's
    # 16 * paths * (C + P2 + P1) + 15 < 0x7C00
    return min(255 - P2 - max(P1, P2), (0x7C00 - 16) // (16 * paths) - (P1 + P2))


def _plan(W, H, D, vols, off, paths, P1, P2, mode):
    plan = EpiPlan(W, H, D, len(vols), paths=paths)
    plan.set_penalties(P1, P2, 0.3)
    for f, v in enumerate(vols):
        plan.upload_cost(f, v)
        plan.upload_offset(f, off)
    plan.set_agg_mode(mode)
    return plan


def _compare(oracle, W, H, D, B, paths, P1, P2, cmax=24, mode=4, tap=False):
    vols = [synth.cost_volume(W, H, D, seed=7 * W + 3 * H + D + f, cmax=cmax) for f in range(B)]
    _, _, off = synth.epi_maps(W, H, "general", seed=3)
    with _plan(W, H, D, vols, off, paths, P1, P2, mode) as plan, _plan(W, H, D, vols, off, paths, P1, P2, 1) as ref:
        assert plan.kernel_name == BAND_NAME[mode] and ref.kernel_name == "packed16/nowrap"
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        ref.run(STAGE_AGGREGATE | STAGE_WTA)
        plan.sync()
        for f in range(B):
            (gbd, gmc), (rbd, rmc) = plan.download(f), ref.download(f)
            assert np.array_equal(gmc, rmc), f"frame {f}: minC differs from the line kernels"
            assert np.array_equal(gbd, rbd), f"frame {f}: bestD differs from the line kernels"
        S = oracle.epi_aggregate(vols[0], P1, P2, paths)
        bd, mc = oracle.epi_wta(S, W, H, D, 1)
        gbd, gmc = plan.download(0)
        assert np.array_equal(gmc, mc), "minC differs from the oracle"
        assert np.array_equal(gbd, oracle.epi_vz_to_disp(bd, off, 0.3, D + 1)), "bestD differs from the oracle"
        if tap:                                              # S of every voxel in natural d order (the kernel's debug tap)
            for f in (0, B - 1):
                assert np.array_equal(plan.download_sum(f), ref.download_sum(f)), f"frame {f}: S differs from the line kernels"
            assert np.array_equal(plan.download_sum(0), S[:-1].reshape(H, W, D)), "S differs from the oracle"


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("P2", [64, 32])                     # 4 * (P1 + P2) > 255: bit plane on / off (8 paths)
@pytest.mark.parametrize("H", [1, 2, 9, 63, 64, 65, 129])
@pytest.mark.parametrize("W", [1, 2, 3, 5, 17, 130])
def test_band_boundaries_and_row_ends(gpu_lib, oracle, W, H, P2, paths):
    _compare(oracle, W, H, 128, 3, paths, 6, P2)


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("P2", [64, 32])
@pytest.mark.parametrize("D", [16, 32, 64])
def test_other_depths_across_their_band_boundary(gpu_lib, oracle, D, P2, paths):
    _compare(oracle, 17, _band_rows(D) + 1, D, 3, paths, 6, P2)


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("P2", [64, 32])
def test_chained_form(gpu_lib, oracle, P2, paths):
    _compare(oracle, 17, 129, 128, 3, paths, 6, P2, mode=5)


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("P2", [64, 32])
def test_largest_admitted_costs(gpu_lib, oracle, P2, paths):
    _compare(oracle, 17, 65, 128, 3, paths, 6, P2, cmax=_cmax(paths, 6, P2))


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("P2", [64, 32])
def test_debug_tap(gpu_lib, oracle, P2, paths):
    _compare(oracle, 17, 65, 128, 3, paths, 6, P2, tap=True)
