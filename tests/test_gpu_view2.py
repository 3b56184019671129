"""The second view from the aggregated volume on the GPU (include/fsgm.h, "Second view").  The yardstick is equality, bit for bit:
disp2 and minC_v2 equal the numpy restatement applied to the S the same call returns, conf equals the restatement's check on the
call's own bestD and disp2, and bestD, minC, minC2 and S equal those of the call without the second view."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import _lib, synth, view2
from fsgm_amd.sgm import _bind as _bind_sgm, last_kernel as sgm_kernel, params as sgm_params
from fsgm_amd._lib import SAMPLING_RECTIFIED, STAGE_ALL

from tests.view2_restatement import check_sgm, check_true, to_true, view2 as restate

pytestmark = pytest.mark.gpu

# how the path volumes come about, cycled over the shapes: (name, cost ceiling, P1, P2, arith, runner_up, adaptive_p2, kernel family)
MODES = [("nowrap", 24, 6, 64, "mod256", False, 0),
         ("wrap", 255, 200, 250, "mod256", False, 0),          # packed16/wrap, generic
         ("exact", 255, 7, 255, "exact", False, 0),            # costs up to 255 at P2 = 255
         ("ru", 2, 3, 9, "mod256", True, 0),                   # low entropy: ties everywhere
         ("adaptive", 24, 6, 64, "mod256", False, 1)]
D_ALL = [16, 32, 128, 48, 224, 144, 256, 272, 1024]


def widths(D):
    T = view2.tile(D) or 64                                      # (the generic kernel has no tile: one wave a pixel)
    return sorted({1, D - 1, T, T + 1, 2 * T + 3})


def volume(n, H, W, D, ceil, seed, layout):
    rng = np.random.default_rng(seed)
    Cv = rng.integers(0, ceil + 1, (n, H, W, D), dtype=np.uint8)
    return Cv if layout == "hwd" else np.ascontiguousarray(Cv.transpose(0, 3, 1, 2))


def run_case(D, W, H, n, paths, direction, d_min, subpixel, layout, mode, seed=0, max_diff=256):
    name, ceil, P1, P2, arith, ru, adaptive = mode
    Cv = volume(n, H, W, D, ceil, seed, layout)
    guide = np.random.default_rng(seed + 1).integers(0, 256, (n, H, W), dtype=np.uint8) if adaptive else None
    kw = dict(paths=paths, layout=layout, subpixel=subpixel, return_sum=True, runner_up=ru, arith=arith, adaptive_p2=adaptive, guide=guide)
    base = fsgm_amd.sgm_batch(Cv, P1, P2, **kw)
    base_kernel = sgm_kernel()
    outs = fsgm_amd.sgm_batch(Cv, P1, P2, second_view=True, direction=direction, d_min=d_min, max_diff=max_diff, **kw)
    assert sgm_kernel() == base_kernel and base_kernel.split("/")[0] in ("packed16", "generic")
    assert len(outs) == len(base) + 3
    for a, b in zip(base, outs):                                 # bestD, minC, (minC2,) S: those of the call without the second view
        assert np.array_equal(a, b)
    S, bestD = outs[len(base) - 1], outs[0]
    disp2, minC_v2, conf = outs[-3:]
    rd2, rmc = restate(S, direction, d_min, subpixel)
    assert np.array_equal(minC_v2, rmc)
    assert np.array_equal(disp2, rd2)
    assert np.array_equal(conf, check_sgm(bestD, disp2, direction, d_min, max_diff, subpixel))
    return base_kernel, disp2


@pytest.mark.parametrize("D", D_ALL)
def test_every_d_width_and_height(D):
    """One D class (packed, split, generic <= 256 on the tiled kernel, 256, generic) at every width around the tile crossed with
    H = 1 and 3; the other parameters are cycled over those ten cases so that, for this D, every mode, both layouts, both
    directions, both path counts, every d_min, both frame counts and sub-pixel on and off occur -- asserted below"""
    hit = {k: set() for k in ("mode", "layout", "direction", "paths", "d_min", "n", "subpixel", "kernel", "WH")}
    invalid = 0
    cases = [(W, H) for W in widths(D) for H in (1, 3)]
    assert len(cases) == 10
    for k, (W, H) in enumerate(cases):
        c = dict(mode=MODES[k % 5], layout=("hwd", "dhw")[(k % 5 + k // 5) % 2], direction=(-1, 1)[(k // 2) % 2], paths=(4, 8)[(k // 3) % 2],
                 d_min=(-3, 0, 5)[k % 3], n=(1, 3)[((k + 1) // 2) % 2] if W * D < 150000 else 1, subpixel=(k // 4 + k) % 2)
        kernel, disp2 = run_case(D, W, H, c["n"], c["paths"], c["direction"], c["d_min"], c["subpixel"], c["layout"], c["mode"], seed=100 * D + k)
        for name, v in c.items():
            hit[name].add(v[0] if name == "mode" else v)
        hit["kernel"].add(kernel)
        hit["WH"].add((W, H))
        invalid += int((disp2 == view2.NO_VIEW2).sum())
    assert hit["WH"] == {(W, H) for W in widths(D) for H in (1, 3)}
    assert hit["mode"] == {m[0] for m in MODES} and hit["layout"] == {"hwd", "dhw"} and hit["direction"] == {-1, 1}
    assert hit["paths"] == {4, 8} and hit["d_min"] == {-3, 0, 5} and hit["subpixel"] == {0, 1} and 1 in hit["n"]
    assert 3 in hit["n"] or D >= 272
    packed = view2.tile(D) and D in (16, 32, 128, 48, 224, 256)
    want = {"packed16/nowrap", "packed16/wrap", "packed16/exact"} if packed else {"generic", "generic/exact"}
    assert hit["kernel"] == want
    assert invalid > 0                                           # (d_min > 0 leaves second-view pixels without a candidate)


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("d_min", [-3, 0, 5])
def test_direction_d_min_subpixel(direction, d_min):
    """both directions x every d_min x sub-pixel on and off x 4 and 8 paths, on the tiled and on the generic kernel"""
    for D, W in ((32, 41), (272, 70)):
        for subpixel, paths, mode in itertools.product((0, 1), (4, 8), (MODES[1], MODES[3])):
            _, disp2 = run_case(D, W, 3, 2, paths, direction, d_min, subpixel, "hwd", mode, seed=7)
            if d_min > 0:
                assert (disp2 == view2.NO_VIEW2).any()


def test_wrap_pipelines():
    """wrapping penalties reach generic/wrap (a generic plan names one pipeline) and packed16/wrap"""
    assert run_case(128, 70, 2, 1, 8, -1, 0, 1, "hwd", MODES[1])[0] == "packed16/wrap"
    assert run_case(144, 70, 2, 1, 8, -1, 0, 1, "hwd", MODES[1])[0] == "generic"


def test_max_diff_zero_and_planted():
    """a planted volume (0 at i = k, 20 elsewhere): disp2 = 256 k wherever the planted candidate is in range, and the check passes
    there even at max_diff = 0"""
    W, H, D, k = 40, 2, 16, 5
    Cv = np.full((1, H, W, D), 20, np.uint8)
    Cv[..., k] = 0
    # (whole disparities: the aggregated S is not flat beside the minimum near the image border, so the parabola may move there)
    bestD, minC, disp2, minC_v2, conf = fsgm_amd.sgm_batch(Cv, 3, 9, second_view=True, direction=-1, max_diff=0, subpixel=0)
    assert (bestD == k).all()                                    # (whole indices without sub-pixel; disp2 is index * 256 always)
    assert (disp2[..., :W - k] == 256 * k).all() and (conf[..., k:] == 1).all() and (conf[..., :k] == 0).all()


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("d_min", [-3, 0, 5])
def test_stereo(direction, d_min):
    """the stereo forms on a synthetic pair at 61 x 47: a rectified plan with the switch on against the restatement on its own S,
    and the one-shot form against the plan (true disparities, INT32_MIN) and against the call without the second view"""
    W, H, D = 61, 47, 24
    I1, I2 = synth.image_pair(W, H, D, seed=3)
    with fsgm_amd.EpiPlan(W, H, D, 1, paths=8, vz_to_disp=0, sampling=SAMPLING_RECTIFIED, direction=direction) as plan:
        plan.set_penalties(6, 64, 0.3)
        plan.set_d_min(d_min)
        plan.set_view2(1, direction)
        plan.upload_images(0, I1, I2)
        plan.run(STAGE_ALL)
        bestD, minC = plan.download(0)
        S = plan.download_sum(0)
        disp2, minC_v2 = plan.download_view2(0)
    rd2, rmc = restate(S, direction, d_min, 1)
    assert np.array_equal(disp2, rd2) and np.array_equal(minC_v2, rmc)
    ref = fsgm_amd.stereo_sgm(I1, I2, D, 6, 64, paths=8, direction=direction, d_min=d_min, runner_up=True)
    out = fsgm_amd.stereo_sgm(I1, I2, D, 6, 64, paths=8, direction=direction, d_min=d_min, runner_up=True, second_view=True, max_diff=300)
    for a, b in zip(ref, out):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    disp, d2, mv, conf = out[0], out[3], out[4], out[5]
    assert np.array_equal(disp, bestD.astype(np.int64) + 256 * d_min)
    assert d2.dtype == np.int32 and np.array_equal(d2, to_true(rd2, d_min)) and np.array_equal(mv, rmc)
    assert np.array_equal(conf, check_true(disp, d2, direction, 300))
    assert np.array_equal(fsgm_amd.view2_check(disp, d2, direction=direction, max_diff=300), conf)
    assert conf.any() and not conf.all()


@pytest.mark.parametrize("d_min", [0, 5])
def test_stereo_without_subpixel(d_min):
    """subpixel = 0: the first view is the whole index + 256 d_min as the _range forms return it (unchanged), disp2 is always * 256;
    the call's own check scales the first view, and view2_check agrees once the caller does the same"""
    W, H, D = 61, 47, 24
    I1, I2 = synth.image_pair(W, H, D, seed=5)
    ref = fsgm_amd.stereo_sgm(I1, I2, D, 6, 64, paths=4, d_min=d_min, subpixel=0)
    disp, minC, d2, mv, conf = fsgm_amd.stereo_sgm(I1, I2, D, 6, 64, paths=4, d_min=d_min, subpixel=0, second_view=True)
    assert np.array_equal(ref[0], disp) and np.array_equal(ref[1], minC)
    index = disp.astype(np.int64) - 256 * d_min
    assert index.min() >= 0 and index.max() < D
    valid = d2 != np.iinfo(np.int32).min
    assert ((d2[valid] - 256 * d_min) % 256 == 0).all()
    scaled = (256 * (index + d_min)).astype(np.int32)
    assert np.array_equal(conf, check_true(scaled, d2, -1, 256))
    assert np.array_equal(fsgm_amd.view2_check(scaled, d2), conf) and conf.any() and not conf.all()


def test_plan_refusals_on_device():
    """the switch on plans whose candidates share no line, and forced modes with it"""
    with fsgm_amd.EpiPlan(32, 8, 16, 1) as plan:                 # vz sampling with vz_to_disp
        with pytest.raises(fsgm_amd.FsgmError) as e:
            plan.set_view2(1, -1)
        assert e.value.status == 4
    with fsgm_amd.EpiPlan(32, 8, 16, 1, vz_to_disp=0, sampling=_lib.SAMPLING_LINEAR) as plan:
        with pytest.raises(fsgm_amd.FsgmError) as e:
            plan.set_view2(1, -1)
        assert e.value.status == 4
    with fsgm_amd.EpiPlan(32, 8, 16, 1, vz_to_disp=0) as plan:
        with pytest.raises(fsgm_amd.FsgmError) as e:
            plan.download_view2(0)
        assert e.value.status == 1
        plan.set_view2(1, 1)
        with pytest.raises(fsgm_amd.FsgmError) as e:
            plan.set_agg_mode(3)
        assert e.value.status == 4


def test_dptr_forms_on_a_side_stream():
    """the _dptr forms on a non-default stream, outputs pre-filled with a sentinel: written where they lie, equal to the host forms"""
    torch = pytest.importorskip("torch")
    lib = view2.bind(_bind_sgm(_lib.load()))
    n, H, W, D = 2, 3, 70, 48
    Cv = volume(n, H, W, D, 255, 11, "hwd")
    host = fsgm_amd.sgm_batch(Cv, 200, 250, paths=8, runner_up=True, return_sum=True, second_view=True, direction=1, d_min=5, max_diff=128)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    dC = torch.from_numpy(Cv).to(dev)
    u32 = lambda *s: torch.full(s, -0x5A5A5A5B, dtype=torch.int32, device=dev)
    bestD, minC, minC2, disp2, minC_v2 = (u32(n, H, W) for _ in range(5))
    S = u32(n, H, W, D)
    conf = torch.full((n, H, W), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    prm = sgm_params(lib, paths=8)
    v2 = view2.params(lib, 1, 5, 128)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        _lib.check(lib.fsgm_sgm_view2_dptr(n, dC.data_ptr(), W, H, D, 200, 250, C.byref(prm), C.byref(v2), None, bestD.data_ptr(),
                                           minC.data_ptr(), minC2.data_ptr(), S.data_ptr(), 0, disp2.data_ptr(), minC_v2.data_ptr(),
                                           conf.data_ptr(), stream.cuda_stream, status.data_ptr()))
        d1 = (bestD + 256 * 5)
        d2 = torch.where(disp2 == -1, torch.full_like(disp2, -2 ** 31), disp2 + 256 * 5)
        conf2 = torch.full((n, H, W), 0x5A, dtype=torch.uint8, device=dev)
        _lib.check(lib.fsgm_view2_check_dptr(n, d1.data_ptr(), d2.data_ptr(), W, H, 1, 128, conf2.data_ptr(), 0, stream.cuda_stream,
                                             status.data_ptr()))
    stream.synchronize()
    assert int(status.item()) == 0
    got = [t.cpu().numpy().view(np.uint32) for t in (bestD, minC, minC2, S, disp2, minC_v2)] + [conf.cpu().numpy()]
    for a, b in zip(host, got):
        assert np.array_equal(a, b)
    assert np.array_equal(conf2.cpu().numpy(), host[-1])


def test_stereo_dptr_on_a_side_stream():
    torch = pytest.importorskip("torch")
    lib = view2.bind(_lib.load())
    W, H, D, d_min = 61, 47, 24, -3
    I1, I2 = synth.image_pair(W, H, D, seed=4)
    host = fsgm_amd.stereo_sgm(I1, I2, D, 6, 64, paths=4, d_min=d_min, second_view=True)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    a, b = torch.from_numpy(I1).to(dev), torch.from_numpy(I2).to(dev)
    disp, minC, d2, mv = (torch.full((H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(4))
    conf = torch.full((H, W), 0x5A, dtype=torch.uint8, device=dev)
    prm = lib.fsgm_stereo_params_default()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        _lib.check(lib.fsgm_stereo_sgm_view2_dptr(1, a.data_ptr(), b.data_ptr(), W, H, D, 6, 64, C.byref(prm), None, d_min, 256,
                                                  disp.data_ptr(), minC.data_ptr(), None, d2.data_ptr(), mv.data_ptr(), conf.data_ptr(),
                                                  stream.cuda_stream, None))
    stream.synchronize()
    got = [disp.cpu().numpy(), minC.cpu().numpy().view(np.uint32), d2.cpu().numpy(), mv.cpu().numpy().view(np.uint32), conf.cpu().numpy()]
    for x, y in zip(host, got):
        assert np.array_equal(x, y)
