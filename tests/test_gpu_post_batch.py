"""GPU tests of the post-processing chain on batches of maps (fsgm_epi_postprocess_batch_host / _device, fsgm_vmf_device) and of
test.m's frame body on the device (fsgm_epipolar_flow_pp_*), against the CPU oracle frame by frame.  Values are copies / minima /
IEEE expressions of the inputs: compared exactly, NaN positions included."""
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError  # noqa: E402
from tests import flow_pp_inputs  # noqa: E402
from tests import flow_pp_restatement as R  # noqa: E402
from tests.edge_inputs import oracle_flow_pp_frame  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VMAX, D = 0.3, 64
FSGM_ERR_INVALID = 1


def _same(a, b, msg=""):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg)
    np.testing.assert_array_equal(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0), err_msg=msg)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _batch(W, H, N, seed=0):
    """N maps made like the real thing (vz indices with holes and speckles), different seeds, invalid shares and geometry
    kinds; with N >= 3 the middle frame is all NaN."""
    D1, pd0, nd, off = [], [], [], []
    for f in range(N):
        D1.append(synth.vz_index_map(W, H, D, seed=seed + f, invalid=(0.05, 0.2, 0.5)[f % 3]))
        p, n, o = synth.epi_maps(W, H, ("general", "radial", "axis")[f % 3], seed=seed + 10 + f)
        pd0.append(p), nd.append(n), off.append(o / 8)
    D1 = np.stack(D1)
    if N >= 3:
        D1[N // 2] = np.nan
    return D1, np.stack(pd0), np.stack(nd), np.stack(off)


def _check_frames(got, D1, pd0, nd, off, oracle, what):
    for f in range(D1.shape[0]):
        want = oracle.postprocess(D1[f], pd0[f], nd[f], off[f], VMAX, D + 1, D)
        for g, w, name in zip(got, want, ("filterD1", "filterD2", "filterdisparites")):
            _same(g[f], w, f"{what}: {name} frame {f}")


# ---------------------------------------------------------------------------------------------- batched chain parity
@pytest.mark.parametrize("W,H,N", [(37, 23, 1), (37, 23, 3), (37, 23, 8), (257, 65, 1), (257, 65, 3), (257, 65, 8), (1242, 375, 2)])
def test_batched_chain_matches_single_frames(gpu_lib, oracle, W, H, N):
    maps = _batch(W, H, N, seed=W + N)
    got = fsgm_amd.epi_postprocess_batch(*maps, VMAX, D + 1, D)
    _check_frames(got, *maps, oracle, "host batch")
    if N == 1:                                                   # the single-map entry point on the same map
        for g, w in zip(got, fsgm_amd.epi_postprocess(maps[0][0], maps[1][0], maps[2][0], maps[3][0], VMAX, D + 1, D)):
            _same(g[0], w)


def _isolation_batch():
    """Four frames built so that treating the batch as one tall image would change every stage's answer:
    - frame 0's last two rows and frame 1's first two rows hold 10.0 in columns 0..39: 80 pixels each (dropped by the first
      speckle pass), 160 together (kept);
    - frame 0's last rows hold 35.0 in columns 60..127, frame 1's first rows 31.0: identity Pd0 with O = 0 sends every pixel's
      offers to the rows below it, so frame 0's last row would raise frame 1's D2 row 0 to 35 and fail its check;
    - frame 2 is NaN except its last three rows: the column pass fills the rows above from them, unless frame 1's valid rows
      came first in the same column;
    - frame 3 has valid rows at its top only."""
    W, H, N = 128, 24, 4
    D1 = np.full((N, H, W), np.nan)
    D1[0, :H - 3] = 30.0
    D1[0, H - 2:, :40] = 10.0
    D1[0, H - 2:, 60:] = 35.0
    D1[1, :2, :40] = 10.0
    D1[1, :2, 60:] = 31.0
    D1[1, 3:H - 1] = 40.0
    D1[2, H - 3:] = 20.0
    D1[3, :4] = 50.0
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    pd0 = np.broadcast_to(np.stack([xx + 1.0, yy + 1.0]), (N, 2, H, W)).copy()
    nd = np.ones((N, 2, H, W))
    off = np.zeros((N, H, W))
    return D1, pd0, nd, off


def test_frames_stay_isolated(gpu_lib, oracle):
    maps = _isolation_batch()
    N, H, W = maps[0].shape
    yy, xx = np.mgrid[0:N * H, 0:W].astype(np.float64)            # the same batch as one tall image, identity geometry
    tall = oracle.postprocess(maps[0].reshape(N * H, W), np.stack([xx + 1.0, yy + 1.0]), np.ones((2, N * H, W)),
                              np.zeros((N * H, W)), VMAX, D + 1, D)
    per = [oracle.postprocess(maps[0][f], maps[1][f], maps[2][f], maps[3][f], VMAX, D + 1, D) for f in range(N)]
    for k in range(2):                                           # the test means something: filterD1 and filterD2 differ
        t, p = np.nan_to_num(tall[k], nan=-7.0), np.nan_to_num(np.concatenate([q[k] for q in per]), nan=-7.0)
        assert not np.array_equal(t, p)
    got = fsgm_amd.epi_postprocess_batch(*maps, VMAX, D + 1, D)
    _check_frames(got, *maps, oracle, "host batch")
    got = torch_ops.epi_postprocess(*[_t(a) for a in maps], VMAX, D + 1, D, check=True)
    _check_frames([_n(g) for g in got], *maps, oracle, "device batch")


# ---------------------------------------------------------------------------------------------- the plan caches
CACHE_SHAPES = [(W, 7) for W in range(5, 11)] + [(5, 7)]         # six shapes, two more than a cache holds; then the first again


def _flows(W, H, N, seed):
    kinds = ("general", "int", "even", "zero")
    return np.stack([flow_pp_inputs.flow_pair(W, H, kinds[(k + W) % 4], seed=seed + k)[0] for k in range(N)])


def test_post_plan_cache_evicts_and_rebuilds(gpu_lib, oracle):
    for W, H in CACHE_SHAPES:
        maps = _batch(W, H, 2, seed=W)
        _check_frames(fsgm_amd.epi_postprocess_batch(*maps, VMAX, D + 1, D), *maps, oracle, f"host batch {W}x{H}")


def test_flow_plan_cache_evicts_and_rebuilds(gpu_lib):
    """maxSpeckleSize 4: maps of 35 to 70 pixels keep some regions and lose others."""
    for W, H in CACHE_SHAPES:
        f = _flows(W, H, 2, seed=W)
        _same(fsgm_amd.flow_speckle_filter(f, 2, 4), np.stack([R.flow_speckle_filter(a, 2, 4)[0] for a in f]), f"speckle {W}x{H}")
        _same(fsgm_amd.flow_in_fill(f), np.stack([R.flow_in_fill(a) for a in f]), f"fill {W}x{H}")


def test_two_host_threads_on_one_device(gpu_lib):
    """The map chain and the flow stages from two host threads at once (ctypes calls run without the GIL): each keeps its
    own plans under the device's lock, and every call gives what it gave alone."""
    maps = _batch(37, 23, 3, seed=3)
    flows = _flows(61, 47, 2, seed=5)
    want_pp = fsgm_amd.epi_postprocess_batch(*maps, VMAX, D + 1, D)
    want_sp = fsgm_amd.flow_speckle_filter(flows, 2, 100)
    want_fill = fsgm_amd.flow_in_fill(want_sp)
    assert not np.isnan(want_pp[0][0]).all() and np.isnan(want_sp).any() and not np.isnan(want_sp).all()
    failures = []

    def post(i):
        for g, w, name in zip(fsgm_amd.epi_postprocess_batch(*maps, VMAX, D + 1, D), want_pp, ("filterD1", "filterD2", "disp")):
            _same(g, w, f"{name}, iteration {i}")

    def flow(i):
        sp = fsgm_amd.flow_speckle_filter(flows, 2, 100)
        _same(sp, want_sp, f"flow speckle filter, iteration {i}")
        _same(fsgm_amd.flow_in_fill(sp), want_fill, f"flow fill, iteration {i}")

    def loop(body):
        try:
            for i in range(20):
                body(i)
        except BaseException as e:  # noqa: BLE001  (reported by the main thread)
            failures.append(e)

    threads = [threading.Thread(target=loop, args=(body,), daemon=True) for body in (post, flow)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60.0)
        assert not t.is_alive(), "a thread is still inside the library after 60 s"
    assert not failures, failures


# ---------------------------------------------------------------------------------------------- device = host
def test_device_chain_equals_host_on_a_side_stream(gpu_lib):
    maps = _batch(83, 47, 3, seed=5)
    want = fsgm_amd.epi_postprocess_batch(*maps, VMAX, D + 1, D)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        args = [_t(a) * 1.0 for a in maps]                       # produced by kernels on s
        f1, f2, disp, st = torch_ops.epi_postprocess(*args, VMAX, D + 1, D, return_status=True)
        f1c = f1.clone()
    s.synchronize()
    assert int(st.item()) == 0
    for g, w, name in zip((f1c, f2, disp), want, ("filterD1", "filterD2", "disp")):
        for f in range(3):
            _same(_n(g)[f], w[f], f"{name} frame {f}")
    # one frame at a time through the op without a batch dimension
    g1 = torch_ops.epi_postprocess(*[_t(a[1]) for a in maps], VMAX, D + 1, D, check=True)
    for g, w in zip(g1, want):
        _same(_n(g), w[1])


def test_negative_map_sets_the_status(gpu_lib):
    D1, pd0, nd, off = _batch(40, 30, 2, seed=9)
    D1[1, 7, 3] = -1.0
    args = [_t(a) for a in (D1, pd0, nd, off)]
    *_, st = torch_ops.epi_postprocess(*args, VMAX, D + 1, D, return_status=True)
    torch.cuda.synchronize()
    assert int(st.item()) == FSGM_ERR_INVALID
    with pytest.raises(FsgmError) as ei:
        torch_ops.epi_postprocess(*args, VMAX, D + 1, D, check=True)
    assert ei.value.status == FSGM_ERR_INVALID
    D1[1, 7, 3] = 2.0                                            # the flag does not stick
    *_, st = torch_ops.epi_postprocess(_t(D1), *args[1:], VMAX, D + 1, D, return_status=True)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    with pytest.raises(FsgmError):                               # the host entry point refuses such maps outright
        D1[0, 0, 0] = -3.0
        fsgm_amd.epi_postprocess_batch(D1, pd0, nd, off, VMAX, D + 1, D)


def test_the_negative_flag_is_cleared_by_the_call_that_reports_it(gpu_lib):
    """one negative D1 value: FSGM_ERR_INVALID, and 0 from the very next call at the same shape on the same stream"""
    D1, pd0, nd, off = _batch(9, 6, 2, seed=13)
    bad = D1.copy()
    bad[1, 2, 5] = -1.0
    rest = [_t(a) for a in (pd0, nd, off)]
    status = [torch_ops.epi_postprocess(_t(m), *rest, VMAX, D + 1, D, return_status=True)[-1] for m in (bad, D1)]
    torch.cuda.synchronize()
    assert [int(s.item()) for s in status] == [FSGM_ERR_INVALID, 0]


# ---------------------------------------------------------------------------------------------- vmf
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_vmf_batch(gpu_lib, oracle, ch):
    W, H, N = 37, 23, 4
    flow = (synth.uniform_f64(ch * 10 + N, (N, ch, H, W)) - 0.5) * 40
    got = _n(torch_ops.vmf(_t(flow)))
    for f in range(N):
        np.testing.assert_array_equal(got[f], oracle.vmf(flow[f]), err_msg=f"frame {f}")
    np.testing.assert_array_equal(_n(torch_ops.vmf(_t(flow[2]))), oracle.vmf(flow[2]))


# ---------------------------------------------------------------------------------------------- test.m's frame body
def _rgb(W, H, seed):
    I0, I1 = synth.image_pair(W, H, 12, seed=seed)
    n0 = synth.uniform_u8(seed + 50, (3, H, W), hi=40).astype(np.int32)
    rgb = lambda I: np.clip(np.stack([I, I // 2 + 60, 255 - I]).astype(np.int32) + n0 - 20, 0, 255).astype(np.uint8)  # noqa: E731
    return rgb(I0), rgb(I1)


def _oracle_frame(oracle, I0, I1, geo, paths):
    """test.m:32-54 composed from the oracle's pieces (tests/edge_inputs.py) at this file's dMax and vMax."""
    return oracle_flow_pp_frame(oracle, I0, I1, geo, paths, D, VMAX)


@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("N", [1, 4])
def test_epipolar_flow_pp_end_to_end(gpu_lib, oracle, rgb, N):
    W, H, paths = 160, 96, 4
    pairs = [(_rgb(W, H, 70 + f) if rgb else synth.image_pair(W, H, 12, seed=70 + f)) for f in range(N)]
    geos = [synth.epi_geometry(W, H, "forward" if f % 2 == 0 else "contract") for f in range(N)]
    want = [_oracle_frame(oracle, a, b, g, paths) for (a, b), g in zip(pairs, geos)]
    F, Hm, e, d = (list(x) for x in zip(*geos))
    I0, I1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    host = fsgm_amd.epipolar_flow_pp(I0, I1, F, Hm, e, d, D, VMAX, paths=paths)
    dev = torch_ops.epipolar_flow_pp(_t(I0), _t(I1), F, Hm, e, d, D, VMAX, paths=paths, return_status=True)
    assert int(dev[-1].item()) == 0
    dev = [_n(t) for t in dev[:-1]]
    for f in range(N):
        for k, name in enumerate(("flow", "flow2", "D1", "minC")):
            _same(host[k][f], want[f][k], f"host {name} frame {f}")
            _same(dev[k][f], host[k][f], f"torch {name} frame {f}")
    assert any(np.isnan(w[1]).sum() == 0 and (w[1][2] == 1).all() for w in want)      # the chain filled the holes it made
    if N == 1:                                                   # one frame without the batch dimension
        one = fsgm_amd.epipolar_flow_pp(pairs[0][0], pairs[0][1], *geos[0], D, VMAX, paths=paths)
        tone = torch_ops.epipolar_flow_pp(_t(pairs[0][0]), _t(pairs[0][1]), *geos[0], D, VMAX, paths=paths, check=True)
        for k in range(4):
            _same(one[k], want[0][k])
            _same(_n(tone[k]), want[0][k])


# ---------------------------------------------------------------------------------------------- streams, inputs, opcheck
def _sleep_then(s, fn):
    """Queue ~50 ms of device sleep on s, then fn(); True when s was still busy after fn returned (fn did not wait)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(1_000_000)
    t1.record()
    t1.synchronize()
    cycles = int(1_000_000 * 50.0 / max(t0.elapsed_time(t1), 1e-3))
    torch.cuda._sleep(cycles)
    out = fn()
    return not s.query(), out


def test_no_host_wait_after_warm_up(gpu_lib):
    W, H = 160, 96
    maps = [_t(a) for a in _batch(W, H, 2, seed=31)]
    I0, I1 = (np.stack(x) for x in zip(*[synth.image_pair(W, H, 12, seed=80 + f) for f in range(2)]))
    geos = [synth.epi_geometry(W, H, k) for k in ("forward", "contract")]
    F, Hm, e, d = (list(x) for x in zip(*geos))
    imgs = (_t(I0), _t(I1))
    want_pp = fsgm_amd.epi_postprocess_batch(*[_n(m) for m in maps], VMAX, D + 1, D)
    want_fl = fsgm_amd.epipolar_flow_pp(I0, I1, F, Hm, e, d, D, VMAX)
    calls = {
        "epi_postprocess": lambda: torch_ops.epi_postprocess(*maps, VMAX, D + 1, D),
        "vmf": lambda: torch_ops.vmf(maps[1]),
        "epipolar_flow_pp": lambda: torch_ops.epipolar_flow_pp(*imgs, F, Hm, e, d, D, VMAX),
    }
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for fn in calls.values():                                # warm-up: plans made, tables uploaded
            fn()
        s.synchronize()
        for name, fn in calls.items():
            busy, out = _sleep_then(s, fn)
            assert busy, f"{name}: the call waited for the device"
            s.synchronize()
            if name == "epi_postprocess":
                for g, w in zip(out, want_pp):
                    for f in range(2):
                        _same(_n(g)[f], w[f])
            elif name == "epipolar_flow_pp":
                for g, w in zip(out, want_fl):
                    _same(_n(g), w)


def test_inputs_untouched_and_opcheck(gpu_lib):
    W, H = 83, 47
    maps = [_t(a) for a in _batch(W, H, 2, seed=41)]
    I0, I1 = _rgb(W, H, 42)
    g = synth.epi_geometry(W, H, "forward")
    pair = [_t(I0)[None], _t(I1)[None]]
    flow = _t((synth.uniform_f64(43, (2, 3, H, W)) - 0.5) * 40)
    before = [a.clone() for a in maps + pair + [flow]]
    torch_ops.epi_postprocess(*maps, VMAX, D + 1, D, check=True)
    torch_ops.vmf(flow)
    torch_ops.epipolar_flow_pp(pair[0][0], pair[1][0], *g, D, VMAX, check=True)
    torch.cuda.synchronize()
    for a, b in zip(maps + pair + [flow], before):
        assert torch.equal(a.nan_to_num(-7.0) if a.is_floating_point() else a, b.nan_to_num(-7.0) if b.is_floating_point() else b)
    geometry = [float(x) for x in np.asarray(g[0]).reshape(-1)] + [float(x) for x in np.asarray(g[1]).reshape(-1)] + [g[2][0], g[2][1], float(g[3])]
    checks = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.fsgm.epi_postprocess.default, (*maps, VMAX, float(D + 1), float(D)), test_utils=checks)
    torch.library.opcheck(torch.ops.fsgm.vmf.default, (flow,), test_utils=checks)
    torch.library.opcheck(torch.ops.fsgm.epipolar_flow_pp.default, (*pair, geometry, D, VMAX, 4), test_utils=checks)
