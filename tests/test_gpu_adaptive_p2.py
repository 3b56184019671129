"""GPU tests of adaptive P2 (fsgm_epi_options.adaptive_p2): the library against the reference's own compiled code
(tests/golden/ref_mex_calc_cost_sgm_adaptive.npz) bit for bit through the plan API, the one-shot host calls, both MEX gateways and
fsgm_stereo_sgm_host; against the numpy restatement (tests/adaptive_p2_restatement.py) where the fixture has no case; the
refusals; the plan cache.  Fixtures only: the reference tree is never read."""
import ctypes as C

import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import EpiPlan, _lib, synth
from fsgm_amd._lib import FsgmError, STAGE_AGGREGATE, STAGE_ALL, STAGE_WTA
from tests import adaptive_p2_restatement as A
from tests import mexharness as mh

pytestmark = pytest.mark.gpu

CASES = [A.golden_case(i) for i in range(A.golden_count())]
IDS = [c["id"] for c, _ in CASES]
LINES = ("packed16/nowrap", "packed16/wrap", "generic")


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: minC differs on {(got[1] != want[1]).sum()} pixels"
    assert np.array_equal(got[0], want[0]), f"{what}: bestD differs on {(got[0] != want[0]).sum()} pixels"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_plan_matches_the_reference_built_with_the_flags(gpu_lib, i):
    c, want = CASES[i]
    H, W = c["I1"].shape
    with EpiPlan(W, H, c["D"], 1, paths=c["paths"], sampling=_lib.SAMPLING_LINEAR if c["linear"] else _lib.SAMPLING_VZ,
                 adaptive_p2=c["adaptive"]) as plan:
        plan.set_penalties(c["P1"], c["P2"], c["vMax"])
        plan.upload(0, c["I1"], c["I2"], c["pd0"], c["nd"], None if c["linear"] else c["off"])
        plan.run(STAGE_ALL)
        assert plan.kernel_name in LINES
        _same(plan.download(0), want, c["id"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_host_calls_match_the_reference_built_with_the_flags(gpu_lib, i):
    c, want = CASES[i]
    if c["linear"]:
        got = fsgm_amd.calc_cost_sgm_linear(c["I1"], c["I2"], c["D"], c["pd0"], c["nd"], c["P1"], c["P2"], paths=c["paths"],
                                            adaptive_p2=c["adaptive"])
    else:
        got = fsgm_amd.calc_cost_sgm(c["I1"], c["I2"], c["D"], c["vMax"], c["pd0"], c["nd"], c["off"], c["P1"], c["P2"],
                                     paths=c["paths"], adaptive_p2=c["adaptive"])
    _same(got, want, c["id"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_gateways_match_the_reference_built_with_the_flags(gpu_lib, monkeypatch, i):
    c, want = CASES[i]
    monkeypatch.setenv("FSGM_EPI_PATHS", str(c["paths"]))
    monkeypatch.setenv("FSGM_EPI_ADAPTIVE_P2", str(c["adaptive"]))
    outs, _ = mh.call("calc_cost_sgm_linear" if c["linear"] else "calc_cost_sgm", 4, c["I1"], c["I2"], c["D"], c["vMax"], c["pd0"], c["nd"],
                      c["off"], c["P1"], c["P2"])
    _same(outs, want, c["id"])
    assert not outs[2].any() and not outs[3].any()


@pytest.mark.parametrize("i", [i for i, (c, _) in enumerate(CASES) if c["linear"] and c["id"].startswith("rect")], ids=lambda i: IDS[i])
def test_stereo_sgm_matches_the_reference_on_the_rectified_cases(gpu_lib, i):
    c, want = CASES[i]
    _same(fsgm_amd.stereo_sgm(c["I1"], c["I2"], c["D"], c["P1"], c["P2"], paths=c["paths"], direction=-1, adaptive_p2=c["adaptive"]), want, c["id"])


def _frame(W, H, D, seed):
    I1, I2 = synth.image_pair(W, H, D, seed=seed)
    return (I1, I2, D, 0.3, *synth.epi_maps(W, H, "general", seed=seed))


# along-x and along-y lines across several prefetch rounds (16 steps along x, 4 elsewhere), D = 256, the generic kernel past
# one round of its 64 lanes, and wrapping penalties at a packed D
@pytest.mark.parametrize("W,H,D,P1,P2", [(70, 40, 128, 6, 64), (40, 70, 32, 6, 64), (19, 11, 256, 6, 64), (23, 9, 72, 6, 64),
                                         (21, 13, 64, 100, 200)])
def test_eight_paths_whole_disparities_and_fb_check_match_the_restatement(gpu_lib, W, H, D, P1, P2):
    I1, I2, _, vMax, pd0, nd, off = _frame(W, H, D, W + H)
    want = A.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, paths=8, adaptive=1, subpixel=0, fb_check=1)
    got = fsgm_amd.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, paths=8, subpixel=0, fb_check=1, adaptive_p2=1)
    _same(got, want, "vz")
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    off_ = fsgm_amd.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, P1, P2, paths=8, subpixel=0, fb_check=1)
    assert (off_[1] != got[1]).any()                             # the switch does something on this frame


def test_batch_of_distinct_frames_through_a_plan(gpu_lib):
    """three frames with images of their own: a wrong frame stride of the pixel loads shows"""
    W, H, D = 37, 21, 32
    fr = [_frame(W, H, D, s) for s in (3, 4, 5)]
    with EpiPlan(W, H, D, 3, paths=8, adaptive_p2=1) as plan:
        plan.set_penalties(6, 64, 0.3)
        for f, (I1, I2, _, _, pd0, nd, off) in enumerate(fr):
            plan.upload(f, I1, I2, pd0, nd, off)
        plan.run(STAGE_ALL)
        for f, (I1, I2, _, vMax, pd0, nd, off) in enumerate(fr):
            _same(plan.download(f), A.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, 6, 64, paths=8, adaptive=1), f"frame {f}")


def test_aggregation_only_plan_takes_its_image_from_upload_images(gpu_lib, oracle):
    W, H, D = 33, 9, 32
    Cv = synth.cost_volume(W, H, D, seed=2, cmax=24)
    I1, I2 = synth.image_pair(W, H, D, seed=6)
    _, _, off = synth.epi_maps(W, H, "general")
    with EpiPlan(W, H, D, 2, paths=8, vz_to_disp=0, adaptive_p2=1) as plan:
        plan.set_penalties(6, 64, 0.3)
        for f in range(2):
            plan.upload_cost(f, Cv)
        plan.upload_images(0, I1, I2)
        with pytest.raises(FsgmError) as e:                      # slot 1 has no image: refused, nothing read
            plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert e.value.status == 1 and "frame 1" in str(e.value)
        plan.upload_images(1, I1[::-1].copy(), I2)
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        for f, img in enumerate((I1, I1[::-1].copy())):
            _same(plan.download(f), oracle.epi_wta(A.aggregate(Cv, img, 6, 64, 8, 1), W, H, D, 1), f"frame {f}")
        plan.set_adaptive_p2(0)                                  # and back: the non-adaptive answer
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        _same(plan.download(1), oracle.epi_wta(oracle.epi_aggregate(Cv, 6, 64, 8), W, H, D, 1), "adaptive off")


def test_fused_modes_are_refused_on_an_adaptive_plan(gpu_lib):
    with EpiPlan(64, 32, 64, 40, paths=8) as plan:
        lines = plan.kernel_name
        plan.set_adaptive_p2(1)
        assert plan.kernel_name == "packed16/nowrap"             # 40 frames, still the line kernels
        for mode in (2, 3, 4, 5, 6):
            with pytest.raises(FsgmError) as e:
                plan.set_agg_mode(mode)
            assert e.value.status == 4
        plan.set_agg_mode(1)
        plan.set_agg_mode(0)
        plan.set_adaptive_p2(0)
        assert plan.kernel_name == lines                         # the selection of a non-adaptive plan is what it was
        plan.set_agg_mode(4)
        with pytest.raises(FsgmError) as e:
            plan.set_adaptive_p2(1)
        assert e.value.status == 4 and plan.kernel_name == "band16/nowrap"
    assert fsgm_amd.epi.auto_pipeline(1242, 375, 128, 40, paths=8, adaptive_p2=1) == "packed16/nowrap"
    assert fsgm_amd.epi.auto_pipeline(1242, 375, 128, 40, paths=8) not in LINES


def test_alternating_calls_of_one_shape_each_get_their_own_answer(gpu_lib):
    I1, I2, D, vMax, pd0, nd, off = _frame(33, 17, 32, 8)
    want = {a: A.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, 6, 64, paths=4, adaptive=a) for a in (0, 1)}
    assert (want[0][1] != want[1][1]).any()
    for a in (1, 0, 1, 0, 0, 1):
        _same(fsgm_amd.calc_cost_sgm(I1, I2, D, vMax, pd0, nd, off, 6, 64, adaptive_p2=a), want[a], f"adaptive_p2={a}")
    pd0r, ndr = fsgm_amd.stereo_maps(33, 17)
    wl = {a: A.calc_cost_sgm_linear(I1, I2, D, pd0r, ndr, 6, 64, paths=4, adaptive=a) for a in (0, 1)}
    for a in (1, 0, 1):
        _same(fsgm_amd.stereo_sgm(I1, I2, D, adaptive_p2=a), wl[a], f"stereo adaptive_p2={a}")
        _same(fsgm_amd.calc_cost_sgm_linear(I1, I2, D, pd0r, ndr, 6, 64, adaptive_p2=a), wl[a], f"linear adaptive_p2={a}")


def test_options_off_is_byte_identical_to_the_entry_points_without_options(gpu_lib):
    lib = _lib.load()
    I1, I2, D, vMax, pd0, nd, off = _frame(40, 24, 64, 9)
    H, W = I1.shape
    e, prm = _lib.EpiIn(), lib.fsgm_epi_params_default()
    e.I1, e.I2, e.width, e.height, e.dMax, e.vMax = _lib.ptr(I1), _lib.ptr(I2), W, H, D, vMax
    e.pixelPosD0, e.normDir, e.offset, e.P1, e.P2 = _lib.ptr(pd0), _lib.ptr(nd), _lib.ptr(off), 6, 64
    prm.paths = 8

    def run(fn, *tail):
        o, bd, mc = _lib.EpiOut(), np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
        o.bestD, o.minC = _lib.ptr(bd), _lib.ptr(mc)
        _lib.check(fn(C.byref(e), C.byref(o), C.byref(prm), *tail))
        return bd, mc
    zero = _lib.options(0)
    for old, new in ((lib.fsgm_calc_cost_sgm_host, lib.fsgm_calc_cost_sgm_host_opts),
                     (lib.fsgm_calc_cost_sgm_linear_host, lib.fsgm_calc_cost_sgm_linear_host_opts)):
        a, b, c = run(old), run(new, None), run(new, C.byref(zero))
        assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()
    L, R = np.stack([I1, I1[::-1]]), np.stack([I2, I2[::-1]])
    sp = lib.fsgm_stereo_params_default()
    outs = []
    for fn, tail in ((lib.fsgm_stereo_sgm_host, ()), (lib.fsgm_stereo_sgm_host_opts, (None,)), (lib.fsgm_stereo_sgm_host_opts, (C.byref(zero),))):
        d, m = np.zeros(L.shape, np.uint32), np.zeros(L.shape, np.uint32)
        _lib.check(fn(2, _lib.ptr(L), _lib.ptr(R), W, H, D, 6, 64, C.byref(sp), *tail, _lib.ptr(d), _lib.ptr(m), None, None))
        outs.append(d.tobytes() + m.tobytes())
    assert outs[0] == outs[1] == outs[2]
