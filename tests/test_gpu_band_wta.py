"""GPU parity tests of the band sweeps' WTA (the final pass of fsgm_amd/csrc/epi_band.hip, band_wta_record): the record
{best, minC, S[best-1], S[best+1]} + S[0] of every pixel, where the neighbours come from a per-workgroup offset table and a
mask zeroes the absent one.  Agg mode 4 forced, everything against the CPU oracle (bestD, minC; the S tap on one frame):
minima placed at d = 0, 1, 2, D-2, D-1; exact ties of S inside one lane and across the lanes of a pixel (the first minimum
wins); S near its largest value; the band boundaries with and without the 9th-bit plane."""
import numpy as np
import pytest

from fsgm_amd import synth, EpiPlan
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA

pytestmark = pytest.mark.gpu


def _run(oracle, vols, P1, P2, paths, W, H, D, taps=(0,)):
    """Runs the band pipeline on `vols` and checks every frame against the oracle; returns the oracle's S of frame 0."""
    _, _, off = synth.epi_maps(W, H, "general", seed=5)
    with EpiPlan(W, H, D, len(vols), paths=paths) as plan:
        plan.set_penalties(P1, P2, 0.3)
        for f, v in enumerate(vols):
            plan.upload_cost(f, v)
            plan.upload_offset(f, off)
        plan.set_agg_mode(4)
        assert plan.kernel_name == "band16/nowrap"
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        S0 = None
        for f, v in enumerate(vols):
            S = oracle.epi_aggregate(v, P1, P2, paths)
            bd, mc = oracle.epi_wta(S, W, H, D, 1)
            gbd, gmc = plan.download(f)
            np.testing.assert_array_equal(gmc, mc, err_msg=f"frame {f} minC")
            np.testing.assert_array_equal(gbd, oracle.epi_vz_to_disp(bd, off, 0.3, D + 1), err_msg=f"frame {f} bestD")
            if f in taps:
                np.testing.assert_array_equal(plan.download_sum(f), S[:-1].reshape(H, W, D), err_msg=f"frame {f} S")
            if f == 0:
                S0 = np.asarray(S[:-1]).reshape(H, W, D)
        return S0


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("D", [128, 64, 256])
@pytest.mark.parametrize("P1,P2", [(6, 64), (6, 32)])
def test_band_wta_best_at_the_ends_of_the_range(gpu_lib, oracle, D, P1, P2, paths):
    """Deep cost minima at d = 0, 1, 2, D-2, D-1 in blocks of pixels: best lands on every one of them (c_1 = 0 at best = 0,
    c1 = 0 at best = D-1, in-range neighbours next to them)."""
    W, H = 47, 70
    targets = np.array([0, 1, 2, D - 2, D - 1])
    ys, xs = np.mgrid[0:H, 0:W]
    dstar = targets[(ys // 5 + xs // 6) % len(targets)]
    vols = []
    for f in range(2):
        v = synth.cost_volume(W, H, D, seed=40 + f, cmax=24)
        v = np.where(np.arange(D)[None, None, :] == dstar[:, :, None], 0, np.maximum(v, 12)).astype(np.uint8)
        vols.append(np.ascontiguousarray(v))
    S = _run(oracle, vols, P1, P2, paths, W, H, D)
    best = np.argmin(S, axis=2)
    for d in targets:
        assert (best == d).any(), f"no pixel with best = {d}"


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("P1,P2", [(6, 64), (6, 32)])
def test_band_wta_exact_ties_take_the_first_minimum(gpu_lib, oracle, P1, P2, paths):
    """Uniform frames whose costs have equal minima at two d: in one lane (same register / other half / other register)
    and in different lanes of a pixel; and a frame of one constant cost (every d ties: best = 0)."""
    W, H, D = 40, 66, 128
    pairs = [(17, 25), (16, 18), (20, 29), (5, 21), (3, 100), (40, 120), (64, 65 + 8)]
    vols = []
    for a, b in pairs:
        v = np.full((H, W, D), 20, np.uint8)
        v[:, :, a] = 0
        v[:, :, b] = 0
        vols.append(v)
    vols.append(np.full((H, W, D), 7, np.uint8))
    S = _run(oracle, vols[:1], P1, P2, paths, W, H, D)
    a, b = pairs[0]
    assert (S[:, :, a] == S[:, :, b]).all() and (S[:, :, a] == S.min(axis=2)).all(), "the first frame must tie exactly"
    _run(oracle, vols, P1, P2, paths, W, H, D, taps=(0, len(vols) - 1))


@pytest.mark.parametrize("paths,P1,P2,cmax", [(8, 6, 64, 24), (8, 63, 64, 120), (8, 6, 100, 55), (4, 63, 64, 127), (4, 6, 64, 24)])
def test_band_wta_large_sums(gpu_lib, oracle, paths, P1, P2, cmax):
    """S near its largest value: cmax = 24 with P2 = 64, and the largest cmax + P1 + P2 that the band sweeps take (no wrap,
    cmax + P2 + max(P1, P2) <= 255; the packed keys S * 16 + index below 0x7C00)."""
    assert 16 * paths * (cmax + P1 + P2) + 15 < 0x7C00
    W, H, D = 53, 67, 128
    vols = []
    for f in range(2):
        v = synth.cost_volume(W, H, D, seed=70 + f, cmax=cmax)
        v[:, ::3, :] = cmax                                   # whole columns of the largest cost
        v[::4, :, :] = np.maximum(v[::4, :, :], cmax - 2)
        vols.append(np.ascontiguousarray(v))
    _run(oracle, vols, P1, P2, paths, W, H, D)


BOUNDARY_SHAPES = [
    # W, H, D: one row short of / at / one row past a band boundary (R = 8 waves * 64 / (D / 16) rows)
    (23, 63, 128), (23, 64, 128), (23, 65, 128), (19, 128, 128), (19, 129, 128), (17, 193, 128),
    (21, 127, 64), (21, 128, 64), (21, 129, 64),
    (25, 31, 256), (25, 32, 256), (25, 33, 256), (13, 65, 256),
    (11, 255, 32), (11, 257, 32), (7, 511, 16), (7, 513, 16),
]


@pytest.mark.parametrize("paths", [8, 4])
@pytest.mark.parametrize("P1,P2", [(6, 64), (10, 40)])
@pytest.mark.parametrize("W,H,D", BOUNDARY_SHAPES)
def test_band_wta_band_boundaries(gpu_lib, oracle, W, H, D, P1, P2, paths):
    """Every band boundary, with (4 * (P1 + P2) > 255) and without the first pass's 9th-bit plane."""
    vols = [synth.cost_volume(W, H, D, seed=W + H + D + f, cmax=24) for f in range(2)]
    for v in vols:
        v[:, ::7, :] = 0
    _run(oracle, vols, P1, P2, paths, W, H, D)
