"""GPU tests of the runner-up cost (fsgm_epi_plan_set_runner_up / _download_runner_up, fsgm_stereo_sgm_host_ru) and of the
uniqueness filter: every WTA instantiation against the numpy restatement on the plan's own S, the routing rules of the switch,
the outputs a plain call keeps, the stereo one-shot call and the filter.

Expected values come from tests/runner_up_restatement.py applied to fsgm_epi_plan_download_sum; the crafted volumes and the edge
counts they must meet from tests/runner_up_volumes.py (checked on the CPU oracle's S in tests/test_runner_up_cpu.py).
With subpixel = 0 the matcher's bestD is the reference's unscaled index (calc_cost_sgm.cpp:273), so bestD itself -- not
bestD >> 8 -- is held against the restatement's best."""
import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import EpiPlan, _lib, synth
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA, STAGE_ALL, FsgmError
from fsgm_amd.epi import auto_pipeline, stereo_last_kernel
from tests import runner_up_restatement as RU
from tests import runner_up_volumes as V

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 4
LINES = ("packed16/nowrap", "packed16/wrap", "generic")


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.mark.parametrize("D", V.ALL_D)
def test_every_wta_instantiation_against_the_restatement(gpu_lib, D):
    name = "packed16/nowrap" if V.split_of(D)[0] else "generic"
    for paths in (4, 8):
        for batch in (1, 3):
            vols = V.volumes(D, batch, seed=100 * D + paths)
            total = {}
            with EpiPlan(V.W, V.H, D, batch, paths=paths, subpixel=0, vz_to_disp=0) as plan:
                plan.set_penalties(V.P1, V.P2)
                for f, Cv in enumerate(vols):
                    plan.upload_cost(f, Cv)
                plan.set_runner_up(1)
                plan.run(STAGE_AGGREGATE | STAGE_WTA)
                assert plan.kernel_name == name
                for f in range(batch):
                    what = f"D {D}, {paths} paths, frame {f} of {batch}"
                    S = plan.download_sum(f)
                    best, minC, minC2 = RU.runner_up(S)
                    bd, mc = plan.download(f)
                    _eq(bd, best.astype(np.uint32), f"{what}: bestD")
                    _eq(mc, minC, f"{what}: minC")
                    _eq(plan.download_runner_up(f), minC2, f"{what}: minC2")
                    for k, v in V.edge_counts(D, best, minC, minC2, S).items():
                        total[k] = total.get(k, 0) + v
            for k in V.required(D, batch):
                assert total[k] > 0, f"D {D}, {paths} paths, batch {batch}: no pixel with {k} ({total})"


def test_routing(gpu_lib):
    W, H, D, B = 192, 96, 128, 40
    fused = auto_pipeline(W, H, D, B, 8, 6, 64)
    assert fused not in LINES, "40 frames of this shape must take a fused pipeline in auto mode"
    Cv = synth.cost_volume(W, H, D, seed=2, cmax=24)
    with EpiPlan(W, H, D, B, paths=8, vz_to_disp=0) as plan:
        plan.set_penalties(6, 64)
        plan.upload_cost(0, Cv)
        for f in range(1, B):
            plan.copy_cost(f, 0, 7 * f)
        assert plan.kernel_name == fused
        with pytest.raises(FsgmError) as e:
            plan.download_runner_up(0)
        assert e.value.status == INVALID
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        before = [plan.download(f) for f in (0, 17, B - 1)]
        plan.set_runner_up(1)
        assert plan.kernel_name == "packed16/nowrap"
        for mode in range(2, 7):
            with pytest.raises(FsgmError) as e:
                plan.set_agg_mode(mode)
            assert e.value.status == UNSUPPORTED and plan.kernel_name == "packed16/nowrap"
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        for (bd, mc), f in zip(before, (0, 17, B - 1)):
            got = plan.download(f)
            _eq(got[0], bd, f"frame {f}: bestD with the switch on")
            _eq(got[1], mc, f"frame {f}: minC with the switch on")
            _, _, m2 = RU.runner_up(plan.download_sum(f))
            _eq(plan.download_runner_up(f), m2, f"frame {f}: minC2")
        plan.set_runner_up(0)
        assert plan.kernel_name == fused
        with pytest.raises(FsgmError) as e:
            plan.download_runner_up(0)
        assert e.value.status == INVALID
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        for (bd, mc), f in zip(before, (0, 17, B - 1)):
            got = plan.download(f)
            _eq(got[0], bd, f"frame {f}: bestD with the switch off again")
            _eq(got[1], mc, f"frame {f}: minC with the switch off again")
    with EpiPlan(V.W, V.H, 128, 2, paths=8) as plan:
        plan.set_agg_mode(4)
        with pytest.raises(FsgmError) as e:
            plan.set_runner_up(1)
        assert e.value.status == UNSUPPORTED and plan.runner_up == 0
        with pytest.raises(FsgmError) as e:
            plan.download_runner_up(0)
        assert e.value.status == INVALID
        with pytest.raises(FsgmError) as e:
            plan.set_runner_up(2)
        assert e.value.status == INVALID


@pytest.mark.parametrize("sampling", ["rectified", "vz", "linear"])
def test_plain_outputs_stay_with_the_switch_on(gpu_lib, sampling):
    """bestD, minC, conf and bestD2 of a plan with the switch on are those of the same plan without it in mode 1"""
    W, H, D, B = 61, 23, 32, 2
    kind = {"rectified": _lib.SAMPLING_RECTIFIED, "vz": _lib.SAMPLING_VZ, "linear": _lib.SAMPLING_LINEAR}[sampling]
    pd0, nd, off = synth.epi_maps(W, H, "general")
    with EpiPlan(W, H, D, B, paths=8, fb_check=1, sampling=kind, direction=-1) as plan:
        for f in range(B):
            I1, I2 = synth.image_pair(W, H, D, seed=40 + f)
            if sampling == "rectified":
                plan.upload_images(f, I1, I2)
            else:
                plan.upload(f, I1, I2, pd0, nd, None if sampling == "linear" else off)
        plan.set_agg_mode(1)
        plan.run(STAGE_ALL)
        want = [plan.download(f) + plan.download_fb(f) for f in range(B)]
        plan.set_runner_up(1)
        plan.run(STAGE_ALL)
        for f in range(B):
            got = plan.download(f) + plan.download_fb(f)
            for g, w, n in zip(got, want[f], ("bestD", "minC", "conf", "bestD2")):
                _eq(g, w, f"{sampling}, frame {f}: {n}")
            _, _, m2 = RU.runner_up(plan.download_sum(f))
            _eq(plan.download_runner_up(f), m2, f"{sampling}, frame {f}: minC2")


@pytest.mark.parametrize("D", [64, 48])
def test_stereo_one_shot(gpu_lib, monkeypatch, D):
    W, H, d_min = 64, 48, -3
    L, R = synth.image_pair(W, H, D, seed=7)
    plain = fsgm_amd.stereo_sgm(L, R, D, paths=8, d_min=d_min)
    got = fsgm_amd.stereo_sgm(L, R, D, paths=8, d_min=d_min, runner_up=True)
    assert stereo_last_kernel() == "packed16/nowrap"
    assert len(got) == 3 and got[2].dtype == np.uint32 and got[2].shape == (H, W)
    for g, w, n in zip(got, plain, ("disp", "minC")):
        assert g.dtype == w.dtype
        _eq(g, w, f"D {D}: {n}")
    with EpiPlan(W, H, D, 1, paths=8, sampling=_lib.SAMPLING_RECTIFIED, direction=-1) as plan:
        plan.set_d_min(d_min)
        plan.upload_images(0, L, R)
        plan.run(STAGE_ALL)
        best, minC, minC2 = RU.runner_up(plan.download_sum(0))
    _eq(got[1], minC, f"D {D}: minC against the restatement")
    _eq(got[2], minC2, f"D {D}: minC2 against the restatement")
    # without d_min and with the check: the dtypes and values of the call without the flag, minC2 last
    a = fsgm_amd.stereo_sgm(L, R, D, paths=8, fb_check=1)
    b = fsgm_amd.stereo_sgm(L, R, D, paths=8, fb_check=1, runner_up=True)
    assert len(b) == 5
    for g, w, n in zip(b, a, ("disp", "minC", "conf", "disp2")):
        assert g.dtype == w.dtype
        _eq(g, w, f"D {D}, fb_check: {n}")
    # a plain caller of the same shape at batch 40 keeps its pipeline: the two never share a plan.  (Frames this small stay on the
    # line kernels in auto mode -- the switch points scale with the frame --, so the override that says "fused from 4 frames"
    # is set for this call: FSGM_EPI_PAR_MIN is read when a pipeline is chosen.)
    monkeypatch.setenv("FSGM_EPI_PAR_MIN", "4")
    want = auto_pipeline(W, H, D, 40, 8, 6, 64)
    assert (want not in LINES) == (D == 64), "the fused pipelines take 16 << k candidates only"
    L40, R40 = np.stack([np.roll(L, f, axis=1) for f in range(40)]), np.stack([np.roll(R, f, axis=1) for f in range(40)])
    ru40 = fsgm_amd.stereo_sgm(L40, R40, D, paths=8, d_min=d_min, runner_up=True)
    assert stereo_last_kernel() == "packed16/nowrap"
    p40 = fsgm_amd.stereo_sgm(L40, R40, D, paths=8, d_min=d_min)
    assert stereo_last_kernel() == want
    _eq(ru40[0], p40[0], f"D {D}, 40 frames: disp")
    _eq(ru40[1], p40[1], f"D {D}, 40 frames: minC")
    _eq(ru40[0][0], plain[0], f"D {D}: frame 0 of 40")
    _eq(ru40[2][0], got[2], f"D {D}: minC2 of frame 0 of 40")


@pytest.mark.parametrize("ratio", [0, 15, 100])
def test_uniqueness_filter(gpu_lib, ratio):
    rng = np.random.default_rng(11 + ratio)
    shape = (3, 19, 37)
    m = rng.uniform(0, 64, shape)
    m[rng.random(shape) < 0.2] = np.nan
    minC = rng.integers(0, 2041, shape).astype(np.uint32)
    minC2 = (minC + rng.integers(0, 400, shape)).astype(np.uint32)
    minC2[rng.random(shape) < 0.1] = RU.NO_RUNNER_UP
    big = rng.random(shape) < 0.2                                # around 2^32 / 100: a 32-bit product would wrap
    minC2[big] = (2 ** 32 // 100 + rng.integers(-50, 50, int(big.sum()))).astype(np.uint32)
    minC[big] = (minC2[big].astype(np.int64) - rng.integers(0, 2 ** 24, int(big.sum()))).astype(np.uint32)
    near = rng.random(shape) < 0.1                               # all ones less a little: a runner-up, not the marker
    minC2[near] = (2 ** 32 - 2 - rng.integers(0, 5, int(near.sum()))).astype(np.uint32)
    minC[near] = (2 ** 32 - 9 - rng.integers(0, 2 ** 29, int(near.sum()))).astype(np.uint32)
    want = RU.uniqueness_filter(m, minC, minC2, ratio)
    keep = m.copy()
    got = fsgm_amd.uniqueness_filter(m, minC, minC2, ratio)
    assert got.dtype == np.float64 and np.array_equal(m, keep, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
    rejected = int((np.isnan(want) & ~np.isnan(m)).sum())
    assert (rejected == 0) == (ratio == 0), "the inputs must make the ratio matter"
    one = fsgm_amd.uniqueness_filter(m[1], minC[1], minC2[1], ratio)
    assert np.array_equal(one, want[1], equal_nan=True)
    # out aliased to map, at the entry point
    inplace = m.copy()
    p = _lib.ptr
    assert gpu_lib.fsgm_uniqueness_filter_host(3, p(inplace), p(minC), p(minC2), 37, 19, ratio, p(inplace), 0) == 0
    assert np.array_equal(inplace, want, equal_nan=True)
