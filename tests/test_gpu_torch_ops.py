"""GPU tests of the device-pointer interface (fsgm_amd.torch_ops over the *_device entry points of include/fsgm.h): bit-exact
parity with the host entry points and the oracle, stream order, no host wait after warm-up, two caller streams on one
cached plan, untouched inputs, odd storage offsets, and the refusals (pinned host memory, graph capture)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth, _lib  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError, STAGE_ALL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _frames(W, H, D, n, seed=1, kind="general"):
    out = []
    for f in range(n):
        I1, I2 = synth.image_pair(W, H, D, seed=seed + f)
        pd0, nd, off = synth.epi_maps(W, H, kind, seed=7 + f)
        out.append((I1, I2, pd0, nd, off))
    return out


def _stack(frames):
    return [_t(np.stack([fr[k] for fr in frames])) for k in range(5)]


def _rgb(W, H, seed):
    I0, I1 = synth.image_pair(W, H, 12, seed=seed)
    n0 = synth.uniform_u8(seed + 50, (3, H, W), hi=40).astype(np.int32)
    rgb = lambda I: np.clip(np.stack([I, I // 2 + 60, 255 - I]).astype(np.int32) + n0 - 20, 0, 255).astype(np.uint8)  # noqa: E731
    return rgb(I0), rgb(I1)


def _status_ok(status):
    torch.cuda.synchronize()
    assert int(status.item()) == 0


# ---------------------------------------------------------------------------------------------- calc_cost_sgm parity
@pytest.mark.parametrize("W,H", [(83, 47), (160, 96)])
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("n", [1, 8, 12])
def test_calc_cost_sgm_parity(gpu_lib, W, H, paths, fb, n):
    D = 64
    frames = _frames(W, H, D, n, seed=W + n)
    want = fsgm_amd.calc_cost_sgm_batch(frames, D, 0.3, 6, 64, paths=paths, fb_check=fb)
    args = _stack(frames)
    if n == 1:
        args = [a[0] for a in args]
    got = torch_ops.calc_cost_sgm(args[0], args[1], D, 0.3, args[2], args[3], args[4], 6, 64, paths=paths, fb_check=fb,
                                  return_status=True)
    _status_ok(got[-1])
    got = [_n(g) for g in got[:-1]]
    if n == 1:
        got = [g[None] for g in got]
    for f in range(n):
        for k, name in enumerate(("bestD", "minC", "conf", "bestD2")[:len(want[f])]):
            np.testing.assert_array_equal(got[k][f], want[f][k], err_msg=f"{name} frame {f}")


def test_calc_cost_sgm_full_size_and_oracle(gpu_lib, oracle):
    W, H, D = 1242, 375, 64
    (fr,) = _frames(W, H, D, 1, seed=3, kind="general")
    bd, mc = torch_ops.calc_cost_sgm(*[_t(a) for a in fr[:2]], D, 0.3, *[_t(a) for a in fr[2:]], 6, 64, check=True)
    wbd, wmc = fsgm_amd.calc_cost_sgm(fr[0], fr[1], D, 0.3, fr[2], fr[3], fr[4], 6, 64)
    np.testing.assert_array_equal(_n(bd), wbd)
    np.testing.assert_array_equal(_n(mc), wmc)
    W, H = 83, 47
    (fr,) = _frames(W, H, D, 1, seed=5)
    for paths in (4, 8):
        bd, mc = torch_ops.calc_cost_sgm(*[_t(a) for a in fr[:2]], D, 0.3, *[_t(a) for a in fr[2:]], 6, 64, paths=paths, check=True)
        rbd, rmc = oracle.calc_cost_sgm(fr[0], fr[1], D, 0.3, fr[2], fr[3], fr[4], 6, 64, paths)
        np.testing.assert_array_equal(_n(bd), rbd)
        np.testing.assert_array_equal(_n(mc), rmc)


@pytest.mark.parametrize("paths,modes", [(8, (1, 2, 3, 4, 5, 6)), (4, (1, 2, 4, 5))])
def test_plan_entry_every_aggregation_mode(gpu_lib, paths, modes):
    """Each aggregation pipeline's final kernels write through the caller's pointers: the plan-level device entry against the
    host plan forced into the same mode."""
    W, H, D, n = 83, 47, 64, 3
    frames = _frames(W, H, D, n, seed=40)
    args = _stack(frames)
    for mode in modes:
        with fsgm_amd.EpiPlan(W, H, D, n, paths=paths) as ref, fsgm_amd.EpiPlan(W, H, D, n, paths=paths) as plan:
            for p in (ref, plan):
                p.set_penalties(6, 64, 0.3)
                p.set_agg_mode(mode)
            for f, fr in enumerate(frames):
                ref.upload(f, *fr)
            ref.run(STAGE_ALL)
            want = [ref.download(f) for f in range(n)]
            name = ref.kernel_name
            bd, mc, st = plan.run_tensors(*args, check=True, return_status=True)
            assert plan.kernel_name == name
            assert int(st.item()) == 0
            for f in range(n):
                np.testing.assert_array_equal(_n(bd[f]), want[f][0], err_msg=f"mode {mode} ({name}) bestD frame {f}")
                np.testing.assert_array_equal(_n(mc[f]), want[f][1], err_msg=f"mode {mode} ({name}) minC frame {f}")


# ---------------------------------------------------------------------------------------------- epipolar_sgm_of parity
@pytest.mark.parametrize("rgb", [False, True])
def test_epipolar_sgm_of_parity(gpu_lib, oracle, rgb):
    W, H, D, n = 160, 96, 64, 4
    pairs = [(_rgb(W, H, 60 + f) if rgb else synth.image_pair(W, H, 12, seed=60 + f)) for f in range(n)]
    geos = [synth.epi_geometry(W, H, "forward" if f % 2 == 0 else "contract") for f in range(n)]
    want = [fsgm_amd.epipolar_sgm_of(a, b, *g, D, 0.3) for (a, b), g in zip(pairs, geos)]
    # one frame, and against the oracle
    flow, minC = torch_ops.epipolar_sgm_of(_t(pairs[0][0]), _t(pairs[0][1]), *geos[0], D, 0.3, check=True)
    np.testing.assert_array_equal(_n(flow), want[0][0])
    np.testing.assert_array_equal(_n(minC), want[0][1])
    rflow, rminC = oracle.epipolar_sgm_of(pairs[0][0], pairs[0][1], *geos[0], D, 0.3)
    np.testing.assert_array_equal(_n(flow), rflow)
    np.testing.assert_array_equal(_n(minC), rminC)
    # a batch of different pairs with alternating geometries
    I0 = _t(np.stack([p[0] for p in pairs]))
    I1 = _t(np.stack([p[1] for p in pairs]))
    F, Hm, e, d = (list(x) for x in zip(*geos))
    flow, minC, st = torch_ops.epipolar_sgm_of(I0, I1, F, Hm, e, d, D, 0.3, return_status=True)
    _status_ok(st)
    for f in range(n):
        np.testing.assert_array_equal(_n(flow[f]), want[f][0], err_msg=f"flow frame {f}")
        np.testing.assert_array_equal(_n(minC[f]), want[f][1], err_msg=f"minC frame {f}")


# ---------------------------------------------------------------------------------------------- pyramids parity
@pytest.mark.parametrize("ng", [False, True])
def test_pyramids_parity(gpu_lib, oracle, ng):
    host = fsgm_amd.pyramidal_sgm_ng if ng else fsgm_amd.pyramidal_sgm
    dev = torch_ops.pyramidal_sgm_ng if ng else torch_ops.pyramidal_sgm
    I0, I1 = _rgb(1242, 375, 90)
    wmv, _, wmc = host(I0, I1, 3)
    mv, mc, st = dev(_t(I0), _t(I1), 3, return_status=True)
    _status_ok(st)
    np.testing.assert_array_equal(_n(mv), wmv)
    np.testing.assert_array_equal(_n(mc), wmc)
    pairs = [_rgb(320, 240, 95 + f) for f in range(4)]
    mv, mc, st = dev(_t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs])), 3, return_status=True)
    _status_ok(st)
    for f, (a, b) in enumerate(pairs):
        wmv, _, wmc = host(a, b, 3)
        np.testing.assert_array_equal(_n(mv[f]), wmv, err_msg=f"flow pair {f}")
        np.testing.assert_array_equal(_n(mc[f]), wmc, err_msg=f"minC pair {f}")
    if not ng:
        rmv, rmc, _ = oracle.pyramidal_sgm(*pairs[0], 3)
        np.testing.assert_array_equal(_n(mv[0]), rmv)
        np.testing.assert_array_equal(_n(mc[0]), rmc)


def test_pyramid_gray_batch(gpu_lib):
    pairs = [synth.image_pair(97, 61, 12, seed=30 + f) for f in range(3)]
    mv, mc = torch_ops.pyramidal_sgm(_t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs])), 3,
                                    batch=True, check=True)   # (3, H, W) alone would read as one RGB pair
    for f, (a, b) in enumerate(pairs):
        wmv, _, wmc = fsgm_amd.pyramidal_sgm(a, b, 3)
        np.testing.assert_array_equal(_n(mv[f]), wmv)
        np.testing.assert_array_equal(_n(mc[f]), wmc)


# ---------------------------------------------------------------------------------------------- streams
def test_stream_order_on_a_side_stream(gpu_lib):
    """Inputs made by torch ops on a side stream, the op, and torch ops consuming the outputs, with no synchronisation between."""
    W, H, D = 160, 96, 64
    (fr,) = _frames(W, H, D, 1, seed=11)
    want = fsgm_amd.calc_cost_sgm(fr[0], fr[1], D, 0.3, fr[2], fr[3], fr[4], 6, 64, paths=8)
    host = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in fr]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = [h.to(DEV, non_blocking=True) for h in host]
        I1 = (dev[0].to(torch.int16) + 0).to(torch.uint8)           # produced by kernels on s
        pd0 = dev[2] * 1.0
        bd, mc = torch_ops.calc_cost_sgm(I1, dev[1], D, 0.3, pd0, dev[3], dev[4], 6, 64, paths=8)
        bd2 = bd.clone()
        total = mc.view(torch.int32).to(torch.int64).sum()
    s.synchronize()
    np.testing.assert_array_equal(_n(bd2), want[0])
    np.testing.assert_array_equal(_n(mc), want[1])
    assert int(total) == int(want[1].astype(np.int64).sum())


def test_no_host_wait_after_warm_up(gpu_lib):
    W, H, D = 160, 96, 64
    (fr,) = _frames(W, H, D, 1, seed=12)
    args = [_t(a) for a in fr]
    want = fsgm_amd.calc_cost_sgm(*fr[:2], D, 0.3, *fr[2:], 6, 64, paths=8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch_ops.calc_cost_sgm(args[0], args[1], D, 0.3, args[2], args[3], args[4], 6, 64, paths=8)   # warm-up
        s.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        torch.cuda._sleep(1_000_000)
        t1.record()
        t1.synchronize()
        cycles = int(1_000_000 * 50.0 / max(t0.elapsed_time(t1), 1e-3))   # ~50 ms of sleep
        torch.cuda._sleep(cycles)
        bd, mc = torch_ops.calc_cost_sgm(args[0], args[1], D, 0.3, args[2], args[3], args[4], 6, 64, paths=8)
        busy = not s.query()
    s.synchronize()
    assert busy, "the call waited for the device"
    np.testing.assert_array_equal(_n(bd), want[0])
    np.testing.assert_array_equal(_n(mc), want[1])


def test_two_caller_streams_share_one_plan(gpu_lib):
    W, H, D, n = 160, 96, 64, 2
    sets = [_frames(W, H, D, n, seed=100 + 10 * k) for k in range(2)]
    want = [fsgm_amd.calc_cost_sgm_batch(fr, D, 0.3, 6, 64, paths=8) for fr in sets]
    args = [_stack(fr) for fr in sets]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for rep in range(3):
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                a = args[k]
                outs.append((k, torch_ops.calc_cost_sgm(a[0], a[1], D, 0.3, a[2], a[3], a[4], 6, 64, paths=8)))
    torch.cuda.synchronize()
    for k, (bd, mc) in outs:
        for f in range(n):
            np.testing.assert_array_equal(_n(bd[f]), want[k][f][0])
            np.testing.assert_array_equal(_n(mc[f]), want[k][f][1])


# ---------------------------------------------------------------------------------------------- inputs, alignment, opcheck
def test_inputs_untouched_and_opcheck(gpu_lib):
    W, H, D = 83, 47, 64
    (fr,) = _frames(W, H, D, 1, seed=21)
    args = [_t(a)[None] for a in fr]
    before = [a.clone() for a in args]
    torch_ops.calc_cost_sgm(args[0][0], args[1][0], D, 0.3, args[2][0], args[3][0], args[4][0], 6, 64, check=True)
    I0, I1 = _rgb(W, H, 22)
    g = synth.epi_geometry(W, H, "forward")
    pair = [_t(I0)[None], _t(I1)[None]]
    pair_before = [a.clone() for a in pair]
    torch_ops.epipolar_sgm_of(pair[0][0], pair[1][0], *g, D, 0.3, check=True)
    torch_ops.pyramidal_sgm(pair[0][0], pair[1][0], 3, check=True)
    torch_ops.pyramidal_sgm_ng(pair[0][0], pair[1][0], 3, check=True)
    torch.cuda.synchronize()
    for a, b in zip(args + pair, before + pair_before):
        assert torch.equal(a, b)
    geometry = [float(x) for x in np.asarray(g[0]).reshape(-1)] + [float(x) for x in np.asarray(g[1]).reshape(-1)] + [g[2][0], g[2][1], float(g[3])]
    checks = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.fsgm.calc_cost_sgm.default, (*args, D, 0.3, 6, 64, 4, 1, 1, 0), test_utils=checks)
    torch.library.opcheck(torch.ops.fsgm.epipolar_sgm_of.default, (*pair, geometry, D, 0.3, 4), test_utils=checks)
    torch.library.opcheck(torch.ops.fsgm.pyramidal_sgm.default, (*pair, 3, [6, 32, 2, 5, 5, 1, 2, 0]), test_utils=checks)
    torch.library.opcheck(torch.ops.fsgm.pyramidal_sgm_ng.default, (*pair, 3, [6, 32, 1, 2, 0]), test_utils=checks)


def test_odd_storage_offsets(gpu_lib):
    W, H, D = 83, 47, 64
    (fr,) = _frames(W, H, D, 1, seed=23)
    want = fsgm_amd.calc_cost_sgm(*fr[:2], D, 0.3, *fr[2:], 6, 64, paths=8)

    def shifted(a):                                 # a view one element into a larger buffer: 1 byte (u8), 8 bytes (f64)
        t = _t(a)
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)
    args = [shifted(a) for a in fr]
    assert args[0].data_ptr() % 2 == 1
    bd, mc = torch_ops.calc_cost_sgm(args[0], args[1], D, 0.3, args[2], args[3], args[4], 6, 64, paths=8, check=True)
    np.testing.assert_array_equal(_n(bd), want[0])
    np.testing.assert_array_equal(_n(mc), want[1])
    I0, I1 = _rgb(W, H, 24)
    g = synth.epi_geometry(W, H, "contract")
    wf, wm = fsgm_amd.epipolar_sgm_of(I0, I1, *g, D, 0.3)
    flow, minC = torch_ops.epipolar_sgm_of(shifted(I0), shifted(I1), *g, D, 0.3, check=True)
    np.testing.assert_array_equal(_n(flow), wf)
    np.testing.assert_array_equal(_n(minC), wm)
    # non-contiguous views are copied first
    big = _t(np.stack([I0, I0]))
    wmv, _, wmc = fsgm_amd.pyramidal_sgm(I0, I1, 3)
    mv, mc = torch_ops.pyramidal_sgm(big[:, :, :, :].transpose(0, 1)[:, 0], shifted(I1), 3, check=True)
    np.testing.assert_array_equal(_n(mv), wmv)
    np.testing.assert_array_equal(_n(mc), wmc)


# ---------------------------------------------------------------------------------------------- refusals
def test_pinned_host_memory_is_refused(gpu_lib):
    W, H, D = 32, 24, 16
    (fr,) = _frames(W, H, D, 1, seed=31)
    args = [_t(a) for a in fr]
    pinned = torch.from_numpy(fr[0]).pin_memory()
    bd, mc = torch.empty((H, W), dtype=torch.uint32, device=DEV), torch.empty((H, W), dtype=torch.uint32, device=DEV)
    e, o = _lib.EpiIn(), _lib.EpiOut()
    e.I1, e.I2 = C.c_void_p(pinned.data_ptr()), C.c_void_p(args[1].data_ptr())
    e.pixelPosD0, e.normDir, e.offset = (C.c_void_p(a.data_ptr()) for a in args[2:])
    e.width, e.height, e.dMax, e.vMax, e.P1, e.P2 = W, H, D, 0.3, 6, 64
    o.bestD, o.minC = C.c_void_p(bd.data_ptr()), C.c_void_p(mc.data_ptr())
    lib = _lib.load()
    st = lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), None, None, None)
    assert st == 1, lib.fsgm_last_error()
    assert b"not device memory" in lib.fsgm_last_error()


def _nan_equal(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0))


def _refusal_case(family):
    """(refused(lib) -> status with the first input in pinned host memory, got() -> torch_ops outputs, want() -> host outputs)
    of one family of device entry points, at a shape no other test runs that family at: its plan does not exist yet."""
    W, H, D = 33, 17, 16
    if family == "fsgm_calc_cost_sgm_device":
        D = 24                                       # (the epipolar driver's plan at D = 16 has this family's cache key)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()  # noqa: E731
    if family == "fsgm_epi_postprocess_device":
        maps = (synth.vz_index_map(W, H, D, seed=41)[None],) + tuple(m[None] for m in synth.epi_maps(W, H, "general", seed=42))
        maps = maps[:3] + (maps[3] / 8,)
        dev = [_t(a) for a in maps]
        out = torch.empty((1, H, W), dtype=torch.float64, device=DEV)
        pinned = pin(maps[0])
        return (lambda lib: lib.fsgm_epi_postprocess_device(1, p(pinned), W, H, p(dev[1]), p(dev[2]), p(dev[3]), 0.3, D + 1.0, float(D),
                                                            p(out), None, None, 0, None, None),
                lambda: torch_ops.epi_postprocess(*dev, 0.3, D + 1, D, check=True),
                lambda: fsgm_amd.epi_postprocess_batch(*maps, 0.3, D + 1, D))
    if family == "fsgm_calc_cost_sgm_device":
        (fr,) = _frames(W, H, D, 1, seed=43)
        dev = [_t(a) for a in fr]
        bd, mc = (torch.empty((H, W), dtype=torch.uint32, device=DEV) for _ in range(2))
        pinned = pin(fr[0])
        e, o = _lib.EpiIn(), _lib.EpiOut()
        e.I1, e.I2, e.pixelPosD0, e.normDir, e.offset = p(pinned), p(dev[1]), p(dev[2]), p(dev[3]), p(dev[4])
        e.width, e.height, e.dMax, e.vMax, e.P1, e.P2 = W, H, D, 0.3, 6, 64
        o.bestD, o.minC = p(bd), p(mc)
        return (lambda lib: lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), None, None, None),
                lambda: torch_ops.calc_cost_sgm(dev[0], dev[1], D, 0.3, dev[2], dev[3], dev[4], 6, 64, check=True),
                lambda: fsgm_amd.calc_cost_sgm(fr[0], fr[1], D, 0.3, fr[2], fr[3], fr[4], 6, 64))
    I0, I1 = synth.image_pair(W, H, 12, seed=44)
    d0, d1, pinned = _t(I0), _t(I1), pin(I0[None])
    minC = torch.empty((1, H, W), dtype=torch.uint32, device=DEV)
    if family == "fsgm_pyramidal_sgm_device":
        lib = _lib.load()
        prm = lib.fsgm_pyramid_params_default()
        prm.numPyd = 2
        flow = torch.empty((1, 2, H, W), dtype=torch.float64, device=DEV)
        return (lambda lib: lib.fsgm_pyramidal_sgm_device(1, p(pinned), p(d1), W, H, 1, C.byref(prm), p(flow), p(minC), None, None),
                lambda: torch_ops.pyramidal_sgm(d0, d1, 2, check=True),
                lambda: fsgm_amd.pyramidal_sgm(I0, I1, 2)[::2])         # (mv, minC) of (mv, mvPyd, minC)
    assert family == "fsgm_epipolar_sgm_of_device"
    g = synth.epi_geometry(W, H, "forward")
    geo = torch_ops._geometries([float(x) for x in np.asarray(g[0]).reshape(-1)] + [float(x) for x in np.asarray(g[1]).reshape(-1)]
                                + [g[2][0], g[2][1], float(g[3])], 1)
    flow = torch.empty((1, 3, H, W), dtype=torch.float64, device=DEV)
    return (lambda lib: lib.fsgm_epipolar_sgm_of_device(1, p(pinned), p(d1), W, H, 1, geo, D, 0.3, None, p(flow), p(minC), None, None),
            lambda: torch_ops.epipolar_sgm_of(d0, d1, *g, D, 0.3, check=True),
            lambda: fsgm_amd.epipolar_sgm_of(I0, I1, *g, D, 0.3))


@pytest.mark.parametrize("family", ["fsgm_epi_postprocess_device", "fsgm_pyramidal_sgm_device", "fsgm_epipolar_sgm_of_device",
                                    "fsgm_calc_cost_sgm_device"])
def test_a_refused_first_call_does_not_disturb_the_next(gpu_lib, family):
    """The entry points check the stream and every pointer before they look up or build a plan (capi_device.h,
    device_check_args): a shape's first call, refused for one input in host memory, and then the valid call at that shape
    against the host-pointer form, bit for bit.  (That the refused call built no plan is the order of the code; the ABI has
    no plan count to assert it by.)"""
    refused, got, want = _refusal_case(family)
    lib = _lib.load()
    assert refused(lib) == 1, lib.fsgm_last_error()
    assert b"not device memory" in lib.fsgm_last_error()
    for k, (g, w) in enumerate(zip(got(), want(), strict=True)):
        assert _nan_equal(_n(g).reshape(w.shape), w), f"{family}: output {k}"


def test_graph_capture_is_refused(gpu_lib):
    W, H, D = 32, 24, 16
    (fr,) = _frames(W, H, D, 1, seed=32)
    args = [_t(a) for a in fr]
    torch_ops.calc_cost_sgm(args[0], args[1], D, 0.3, args[2], args[3], args[4], 6, 64, check=True)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(FsgmError) as ei:
        with torch.cuda.graph(g):
            torch_ops.calc_cost_sgm(args[0], args[1], D, 0.3, args[2], args[3], args[4], 6, 64)
    assert ei.value.status == 4 and "captured" in str(ei.value)
    torch.cuda.synchronize()
