"""GPU tests of the linear build of calc_cost_sgm and of rectified stereo.  Every compared output is an integer array and is
compared for equality: against the reference's own code compiled without USE_VZIND (tests/golden/
ref_mex_calc_cost_sgm_linear.npz), against the numpy restatement (tests/stereo_restatement.py) and between the rectified cost
kernel and the general linear path on the maps it implies.  The torch ops: tests/test_gpu_stereo_torch.py."""
import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import EpiPlan, _lib, synth
from fsgm_amd._lib import FsgmError, STAGE_ALL
from tests import mexharness as mh
from tests import ref_golden
from tests import stereo_restatement as R
from tests.stereo_restatement import golden_case

N_CASES = R.golden_count()

pytestmark = pytest.mark.gpu
FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


# ---------------------------------------------------------------------------------------------- the reference's own code
@pytest.mark.parametrize("i", range(N_CASES))
def test_linear_c_abi_matches_the_reference_built_without_vzind(gpu_lib, i):
    c, (bestD, minC, _, _) = golden_case(i)
    bd, mc = fsgm_amd.calc_cost_sgm_linear(c["I1"], c["I2"], c["D"], c["pd0"], c["nd"], c["P1"], c["P2"])
    _eq(mc, minC, c["id"] + " minC")
    _eq(bd, bestD, c["id"] + " bestD")
    if c["id"].startswith("rect-"):                              # the same case through the rectified kernel
        direction = int(c["nd"][0, 0, 0])
        sd, sm = fsgm_amd.stereo_sgm(c["I1"], c["I2"], c["D"], c["P1"], c["P2"], direction=direction)
        _eq(sm, minC, c["id"] + " stereo minC")
        _eq(sd, bestD, c["id"] + " stereo disp")


@pytest.mark.parametrize("i", range(N_CASES))
def test_linear_gateway_matches_the_reference_built_without_vzind(gpu_lib, i):
    c, (bestD, minC, conf, bestD2) = golden_case(i)
    outs, _ = mh.call("calc_cost_sgm_linear", 4, c["I1"], c["I2"], c["D"], c["vMax"], c["pd0"], c["nd"], c["off"], c["P1"], c["P2"])
    for got, want, name in zip(outs, (bestD, minC, conf, bestD2), ("bestD", "minC", "conf", "bestD2")):
        assert got.dtype == want.dtype and got.shape == want.shape
        _eq(got, want, f"{c['id']} {name}")
    if i == 0:
        (only,), _ = mh.call("calc_cost_sgm_linear", 0, c["I1"], c["I2"], c["D"], c["vMax"], c["pd0"], c["nd"], c["off"], c["P1"], c["P2"])
        _eq(only, bestD, "nlhs = 0")


# ---------------------------------------------------------------------------------------------- the rectified kernel
# W: the strip edges (60 output columns a workgroup); H: 1, 4, 5 (fewer raw rows than the ring holds) and 15 / 16 / 17 -- the
# launcher cuts a frame into segments of >= 8 rows while the launch fits the chip in one round (at most 18 workgroups here, any
# device with 18 compute units or more): 15 rows are one segment, 16 two of 8, 17 are 9 + 8; D: the fused kernel's
# 16, 32, 128 and 24 for the raw-cost kernel in front of the box kernels; 5x7x16: W < D, every far sample clamps
STEREO_SHAPES = [
    (1, 1, 16, -1, 4, 1, 1), (4, 4, 16, +1, 8, 0, 1), (59, 5, 32, -1, 4, 1, 3), (60, 15, 16, +1, 4, 1, 1), (61, 16, 32, -1, 8, 1, 1),
    (121, 17, 16, +1, 4, 0, 3), (121, 70, 128, -1, 4, 1, 1), (61, 5, 128, +1, 8, 1, 1), (5, 7, 16, -1, 4, 1, 1), (5, 7, 16, +1, 8, 1, 1),
    (37, 9, 24, -1, 4, 1, 3), (60, 4, 24, +1, 8, 0, 1), (121, 16, 32, +1, 4, 1, 1), (4, 1, 128, -1, 4, 1, 1), (60, 17, 128, +1, 4, 1, 3),
]


@pytest.mark.parametrize("W,H,D,direction,paths,subpixel,batch", STEREO_SHAPES)
def test_stereo_sgm_matches_the_restatement_and_the_linear_path(gpu_lib, oracle, W, H, D, direction, paths, subpixel, batch):
    pairs = [synth.image_pair(W, H, D, seed=W + 3 * H + f) for f in range(batch)]
    pd0, nd = R.rectified_maps(W, H, direction)
    # the plan level: the cost volume tapped from a rectified plan
    with EpiPlan(W, H, D, batch, paths=paths, subpixel=subpixel, sampling=_lib.SAMPLING_RECTIFIED, direction=direction) as plan:
        plan.set_penalties(6, 64)
        for f, (I1, I2) in enumerate(pairs):
            plan.upload_images(f, I1, I2)
        plan.run(STAGE_ALL)
        got = [(plan.download_cost(f),) + plan.download(f) for f in range(batch)]
        with pytest.raises(FsgmError):                           # a rectified plan has no maps to take
            plan.upload(0, *pairs[0], pd0, nd, np.ones((H, W)))
    L = np.stack([p[0] for p in pairs])
    Rt = np.stack([p[1] for p in pairs])
    disp, minC = fsgm_amd.stereo_sgm(L if batch > 1 else L[0], Rt if batch > 1 else Rt[0], D, 6, 64, paths=paths, subpixel=subpixel,
                                     direction=direction)
    assert disp.dtype == np.uint32 and disp.shape == ((batch, H, W) if batch > 1 else (H, W))
    disp, minC = disp.reshape(batch, H, W), minC.reshape(batch, H, W)
    lin = fsgm_amd.calc_cost_sgm_linear_batch([(I1, I2, pd0, nd) for I1, I2 in pairs], D, 6, 64, paths=paths, subpixel=subpixel,
                                              return_volumes=True)
    for f, (I1, I2) in enumerate(pairs):
        Cv = R.box_mean(R.rectified_raw_cost(I1, I2, D, direction))
        wbd, wmc = oracle.epi_wta(oracle.epi_aggregate(Cv, 6, 64, paths), W, H, D, subpixel)
        _eq(got[f][0], Cv, f"C of frame {f} vs the restatement")
        _eq(got[f][2], wmc, f"minC of frame {f} vs the restatement")
        _eq(got[f][1], wbd, f"bestD of frame {f} vs the restatement")
        _eq(minC[f], wmc, f"stereo_sgm minC of frame {f}")
        _eq(disp[f], wbd, f"stereo_sgm disp of frame {f}")
        _eq(lin[f][2], Cv, f"C of frame {f}, linear path on the implied maps")
        _eq(lin[f][1], wmc, f"minC of frame {f}, linear path")
        _eq(lin[f][0], wbd, f"bestD of frame {f}, linear path")


@pytest.mark.parametrize("direction", [-1, 1])
def test_rectified_cost_two_kernel_form_matches_the_fused_kernel(gpu_lib, monkeypatch, direction):
    W, H, D = 61, 9, 32
    I1, I2 = synth.image_pair(W, H, D, seed=4)
    vols = []
    for fused in ("1", "0"):
        monkeypatch.setenv("FSGM_COST_FUSED", fused)
        with EpiPlan(W, H, D, 1, sampling=_lib.SAMPLING_RECTIFIED, direction=direction) as plan:
            plan.upload_images(0, I1, I2)
            plan.run(_lib.STAGE_COST)
            vols.append(plan.download_cost(0))
    _eq(vols[1], vols[0], "raw-cost + box kernels vs the fused kernel")
    _eq(vols[0], R.box_mean(R.rectified_raw_cost(I1, I2, D, direction)), "fused kernel vs the restatement")


def test_linear_matches_the_restatement_on_a_slanted_field(gpu_lib, oracle):
    W, H, D = 83, 21, 32
    I1, I2 = synth.image_pair(W, H, D, seed=12)
    pd0, nd, _ = synth.epi_maps(W, H, "general", seed=3)
    for paths, sub in ((4, 1), (8, 0)):
        bd, mc, Cv, _ = fsgm_amd.calc_cost_sgm_linear(I1, I2, D, pd0, nd, 6, 64, paths=paths, subpixel=sub, return_volumes=True)
        wbd, wmc, wC = R.calc_cost_sgm_linear(I1, I2, D, pd0, nd, 6, 64, paths=paths, subpixel=sub, want_cost=True)
        _eq(Cv, wC, "C")
        _eq(mc, wmc, "minC")
        _eq(bd, wbd, "bestD")


# ---------------------------------------------------------------------------------------------- forward-backward check
@pytest.mark.parametrize("W,H,D,direction", [(61, 9, 16, -1), (37, 12, 32, +1), (5, 7, 16, -1), (45, 8, 24, +1)])
def test_stereo_fb_check_matches_the_restatement(gpu_lib, W, H, D, direction):
    I1, I2 = synth.image_pair(W, H, D, seed=W)
    if direction > 0:
        I1, I2 = I2, I1
    disp, minC, conf, disp2 = fsgm_amd.stereo_sgm(I1, I2, D, direction=direction, fb_check=1)
    d0, m0 = fsgm_amd.stereo_sgm(I1, I2, D, direction=direction)
    _eq(disp, d0, "disp with and without the check")
    _eq(minC, m0, "minC with and without the check")
    wconf, wd2 = R.linear_fb_check(disp, *R.rectified_maps(W, H, direction))
    assert conf.dtype == np.uint8 and disp2.dtype == np.uint32
    _eq(disp2, wd2, "disp2")
    _eq(conf, wconf, "conf")


def test_linear_fb_check_on_a_slanted_field_matches_the_restatement(gpu_lib, monkeypatch):
    W, H, D = 48, 14, 16
    I1, I2 = synth.image_pair(W, H, D, seed=2)
    pd0, nd, _ = synth.epi_maps(W, H, "general", seed=5)
    bd, mc, conf, d2 = fsgm_amd.calc_cost_sgm_linear(I1, I2, D, pd0, nd, 6, 64, fb_check=1)
    b0, _ = fsgm_amd.calc_cost_sgm_linear(I1, I2, D, pd0, nd, 6, 64)
    _eq(bd, b0, "bestD with and without the check")
    wconf, wd2 = R.linear_fb_check(bd, pd0, nd)
    _eq(d2, wd2, "bestD2")
    _eq(conf, wconf, "conf")
    monkeypatch.setenv("FSGM_EPI_FB_CHECK", "1")
    outs, _ = mh.call("calc_cost_sgm_linear", 4, I1, I2, D, 0.3, pd0, nd, np.ones((H, W)), 6, 64)
    _eq(outs[2], wconf, "gateway conf")
    _eq(outs[3], wd2, "gateway bestD2")


def test_fb_check_rejects_dmax_512(gpu_lib):
    I1, I2 = synth.image_pair(9, 4, 16)
    pd0, nd = R.rectified_maps(9, 4, -1)
    with pytest.raises(FsgmError) as e:
        fsgm_amd.stereo_sgm(I1, I2, 512, fb_check=1)
    assert e.value.status == FSGM_ERR_UNSUPPORTED
    with pytest.raises(FsgmError) as e:
        fsgm_amd.calc_cost_sgm_linear(I1, I2, 512, pd0, nd, 6, 64, fb_check=1)
    assert e.value.status == FSGM_ERR_UNSUPPORTED
    d, _, conf, _ = fsgm_amd.stereo_sgm(I1, I2, 511, fb_check=1)     # the largest dMax the check takes
    assert d.shape == (4, 9) and conf.shape == (4, 9)


# ---------------------------------------------------------------------------------------------- existing behaviour
def test_calc_cost_sgm_is_unchanged_after_a_stereo_call_of_the_same_shape(gpu_lib):
    c = ref_golden.case("calc_cost_sgm", 0)
    D, vMax, P1, P2 = c["args"]
    H, W = c["I1"].shape
    s1 = fsgm_amd.stereo_sgm(c["I1"], c["I2"], int(D), int(P1), int(P2))
    l1 = fsgm_amd.calc_cost_sgm_linear(c["I1"], c["I2"], int(D), c["pd0"], c["nd"], int(P1), int(P2))
    bd, mc = fsgm_amd.calc_cost_sgm(c["I1"], c["I2"], int(D), float(vMax), c["pd0"], c["nd"], c["off"], int(P1), int(P2))
    _eq(bd, c["outs"][0], "bestD against the reference's compiled MEX code")
    _eq(mc, c["outs"][1], "minC against the reference's compiled MEX code")
    s2 = fsgm_amd.stereo_sgm(c["I1"], c["I2"], int(D), int(P1), int(P2))
    l2 = fsgm_amd.calc_cost_sgm_linear(c["I1"], c["I2"], int(D), c["pd0"], c["nd"], int(P1), int(P2))
    for a, b in zip(s1 + l1, s2 + l2):
        _eq(a, b, "the stereo / linear result after a vz-index call of the same shape")
