"""GPU parity tests of the band sweeps' first pass (fsgm_amd/csrc/epi_band.hip, MODE 0, 8 paths): its ring of cost words
-- a slot is unpacked, then reloaded with the words of two steps on -- and its step with P2 + m in one half.  Every case
forces the band sweeps (mode 4) and compares bestD and minC of every pixel of both frames with the per-direction line
kernels (mode 1) on the same volumes, exactly.  P1 = 6, P2 = 64 (the 9th-bit plane on), costs up to 24.  Shapes where the
ring and the tail steps can go wrong: frames of 1, 2, 3 and 5 columns (fewer steps than a loop iteration in the first
rows' waves, odd tails), two and three bands with a last band of one row, every D with its own rows per band and steps
per band, and one case without the bit plane (P2 = 57: 4 * (P1 + P2) <= 255).  Two frames each, distinct volumes: the
frame strides."""
import numpy as np
import pytest

from fsgm_amd import synth, EpiPlan
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA

pytestmark = pytest.mark.gpu

PATHS, P1, CMAX, FRAMES = 8, 6, 24, 2


def _plan(W, H, D, vols, off, P2, mode):
    plan = EpiPlan(W, H, D, len(vols), paths=PATHS)
    plan.set_penalties(P1, P2, 0.3)
    for f, v in enumerate(vols):
        plan.upload_cost(f, v)
        plan.upload_offset(f, off)
    plan.set_agg_mode(mode)
    return plan


def _compare(W, H, D, P2=64):
    vols = [synth.cost_volume(W, H, D, seed=11 * W + 5 * H + D + P2 + f, cmax=CMAX) for f in range(FRAMES)]
    _, _, off = synth.epi_maps(W, H, "general", seed=3)
    with _plan(W, H, D, vols, off, P2, 4) as plan, _plan(W, H, D, vols, off, P2, 1) as ref:
        assert plan.kernel_name == "band16/nowrap" and ref.kernel_name == "packed16/nowrap"
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        ref.run(STAGE_AGGREGATE | STAGE_WTA)
        plan.sync()
        for f in range(FRAMES):
            (gbd, gmc), (rbd, rmc) = plan.download(f), ref.download(f)
            assert np.array_equal(gmc, rmc), f"frame {f}: minC differs from the line kernels"
            assert np.array_equal(gbd, rbd), f"frame {f}: bestD differs from the line kernels"


@pytest.mark.parametrize("W", [1, 2, 3, 5])
def test_narrow_frames(gpu_lib, W):
    _compare(W, 9, 128)


@pytest.mark.parametrize("H", [65, 129])
def test_last_band_of_one_row(gpu_lib, H):
    _compare(17, H, 128)


@pytest.mark.parametrize("D", [16, 32, 64, 128, 256])
def test_depths(gpu_lib, D):
    _compare(40, 70, D)


def test_without_bit_plane(gpu_lib):
    _compare(17, 65, 128, P2=57)
