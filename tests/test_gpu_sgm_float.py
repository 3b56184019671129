"""GPU tests of the float cost-volume entries (include/fsgm.h, "Float cost volumes").  The yardstick is equality throughout:
1. the quantising ingest kernels alone -- a float plan ingest, then the plan's cost volume read back, equals the numpy restatement
   (tests/cost_quant_restatement.py) byte for byte, and the status word equals its flag;
2. the door -- torch_ops.sgm_float / sgm2d_float equal torch_ops.sgm / sgm2d on the restatement's bytes with the same cost_bound,
   in every output, and ran the same pipeline;
3. the host forms against the same bytes, and a flagged volume refused with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402  (torch first, then the library)
from fsgm_amd import torch_ops, synth, EpiPlan, PydPlan, _lib  # noqa: E402
from fsgm_amd.sgm import _bind as _bind_sgm, cost_format, last_kernel as sgm_kernel, params as sgm_params  # noqa: E402
from fsgm_amd.sgm2d import _bind as _bind_sgm2d, last_kernel as sgm2d_kernel, params as sgm2d_params  # noqa: E402
from tests import cost_quant_restatement as Q  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FSGM_ERR_INVALID = 1
DTYPES = ["float32", "float16", "bfloat16"]
# (scale, offset, bound): the identity, where the planted ties are exact; a negative scale that is no power of two, so that the
# product rounds, with a bound below 255
FORMATS = ((1.0, 0.0, 255), (-1.7, 130.3, 200))


def _planted(rng, shape, scale, offset, bound, clean=False):
    """fp32 voxels whose rule value u = x * scale + offset covers -6 .. bound + 6, with ties k + 0.5 for even and odd k, values
    around bound +- 0.5 and around -0.5, -0.0, NaN and both infinities planted (scale 1, offset 0: exactly those; otherwise
    close to them).  clean: every voxel quantises inside 0..bound, the ties included, and nothing is flagged."""
    lo, hi = (0.0, bound - 0.5) if clean else (-6.0, bound + 6.0)
    u = rng.uniform(lo, hi, shape)
    flat = u.reshape(-1)
    k = rng.integers(0, bound - 1, flat.size // 7)
    flat[rng.choice(flat.size, k.size, replace=False)] = k + 0.5
    x = ((u - offset) / scale).astype(np.float32)
    if not clean:
        special = [bound + 0.5, np.nextafter(np.float32(bound + 0.5), np.float32(1e9)), np.nextafter(np.float32(bound + 0.5), np.float32(0)),
                   bound - 0.5, bound + 1.0, -0.5, np.nextafter(np.float32(-0.5), np.float32(-1)), -0.0, -1.0, np.nan, np.inf, -np.inf]
        xf = x.reshape(-1)
        at = rng.choice(xf.size, 4 * len(special), replace=False)
        xf[at] = np.tile(((np.array(special, np.float64) - offset) / scale).astype(np.float32), 4)
        xf[0], xf[-1] = np.float32((bound + 2 - offset) / scale), np.float32((-2 - offset) / scale)      # the first and the last voxel
    return x


def _cast(x, dtype):
    """(the volume as a torch tensor of `dtype` on the host, the same values widened back to fp32: what the rule sees)"""
    t = torch.from_numpy(x).to(getattr(torch, dtype))
    return t, t.float().numpy()


def _dev(t, sliced=False):
    """t on the device; sliced: as a view that starts one element into its allocation"""
    t = t.contiguous()
    if not sliced:
        return t.to(DEV)
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    big[1:] = t.reshape(-1).to(DEV)
    view = big[1:].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + t.element_size()
    return view


def _as2d(layout, t, Sx, Sy):
    """(n, H, W, D) in reference order (candidate sx*Sy + sy) -> the layout's tensor"""
    n, H, W, D = t.shape
    if layout == "hwd":
        return t
    if layout == "dhw":
        return t.permute(0, 3, 1, 2)
    return t.reshape(n, H, W, Sx, Sy).permute(0, 4, 3, 1, 2).reshape(n, D, H, W)


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
@pytest.mark.parametrize("layout", ["hwd", "dhw"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ingest_1d_equals_the_restatement(gpu_lib, dtype, layout):
    """(W, H, D): a partial x tile; the second d tile; a D that is no multiple of 4"""
    rng = np.random.default_rng(11)
    first = True
    for W, H, D in ((33, 5, 16), (67, 4, 80), (130, 3, 21)):
        for n in (1, 3):
            with EpiPlan(W, H, D, n, vz_to_disp=0) as plan:
                for scale, offset, bound in FORMATS:
                    for clean in (False, True):
                        t, wide = _cast(_planted(rng, (n, H, W, D), scale, offset, bound, clean), dtype)
                        q, flagged = Q.quantise(wide, scale, offset, bound)
                        assert flagged.any() != clean
                        src = _dev(t if layout == "hwd" else t.permute(0, 3, 1, 2), sliced=first)
                        first = False
                        st = torch_ops.ingest_cost_float(plan, src, scale, offset, layout=layout, cost_bound=bound, return_status=True)
                        what = f"{dtype} {layout} {W}x{H}x{D} n={n} scale {scale} clean {clean}"
                        for f in range(n):
                            np.testing.assert_array_equal(plan.download_cost(f), q[f], err_msg=f"{what} frame {f}")
                        assert int(st.item()) == (0 if clean else FSGM_ERR_INVALID), what


@pytest.mark.parametrize("layout", ["hwd", "dhw", "dhw_yx"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ingest_2d_equals_the_restatement(gpu_lib, dtype, layout):
    """windows 3x5 (padded candidate rows) and 9x9, a partial x tile and a second one"""
    rng = np.random.default_rng(12)
    first = True
    for rX, rY in ((1, 2), (4, 4)):
        Sx, Sy = 2 * rX + 1, 2 * rY + 1
        for W, H in ((33, 5), (67, 4)):
            for n in (1, 3):
                with PydPlan(W, H, W, H, rX, rY, 0, batch=n) as plan:
                    for scale, offset, bound in FORMATS:
                        for clean in (False, True):
                            t, wide = _cast(_planted(rng, (n, H, W, Sx * Sy), scale, offset, bound, clean), dtype)
                            q, flagged = Q.quantise(wide, scale, offset, bound)
                            assert flagged.any() != clean
                            src = _dev(_as2d(layout, t, Sx, Sy), sliced=first)
                            first = False
                            st = torch_ops.ingest_cost2d_float(plan, src, scale, offset, layout=layout, cost_bound=bound, return_status=True)
                            what = f"{dtype} {layout} {W}x{H} {Sx}x{Sy} n={n} scale {scale} clean {clean}"
                            for f in range(n):
                                np.testing.assert_array_equal(plan.download_cost(f), q[f], err_msg=f"{what} frame {f}")
                            assert int(st.item()) == (0 if clean else FSGM_ERR_INVALID), what


# ---------------------------------------------------------------------------------------------- 2. the door
def _same(got, want, names, what):
    assert len(got) == len(want) == len(names), (len(got), len(want), names)
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name}"
        assert torch.equal(g.contiguous().reshape(-1).view(torch.uint8), w.contiguous().reshape(-1).view(torch.uint8)), f"{what}: {name} differs"


def _guide(n, H, W):
    g = np.stack([synth.image_pair(W, H, 16, seed=3 + f)[0] // 2 for f in range(n)])
    g[:, :, W // 2:] += 120
    return torch.from_numpy(g).to(DEV)


SGM_CASES = {
    # name: (W, H, D, n, P1, P2, format, keywords)
    "plain": (37, 9, 16, 1, 7, 100, FORMATS[0], dict(paths=8)),
    "runner_up": (37, 9, 48, 3, 7, 100, FORMATS[1], dict(runner_up=True)),
    "exact": (37, 9, 21, 3, 7, 100, FORMATS[0], dict(arith="exact", paths=8)),
    "adaptive": (37, 9, 16, 3, 6, 64, FORMATS[1], dict(adaptive_p2=1)),
    "fused": (37, 11, 16, 3, 6, 32, (0.1, 0.0, 24), dict(paths=8, agg_mode=2)),
}


@pytest.mark.parametrize("clean", [True, False], ids=["clean", "flagged"])
@pytest.mark.parametrize("layout", ["hwd", "dhw"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(SGM_CASES))
def test_sgm_float_equals_sgm_on_the_quantised_bytes(gpu_lib, case, dtype, layout, clean):
    W, H, D, n, P1, P2, (scale, offset, bound), kw = SGM_CASES[case]
    rng = np.random.default_rng(21)
    t, wide = _cast(_planted(rng, (n, H, W, D), scale, offset, bound, clean), dtype)
    q, flagged = Q.quantise(wide, scale, offset, bound)
    assert flagged.any() != clean
    if layout == "dhw":
        t, q = t.permute(0, 3, 1, 2), q.transpose(0, 3, 1, 2)
    kw = dict(kw, layout=layout, cost_bound=bound, return_sum=True, return_status=True)
    if kw.get("adaptive_p2"):
        kw["guide"] = _guide(n, H, W)
    want = torch_ops.sgm(torch.from_numpy(np.ascontiguousarray(q)).to(DEV), P1, P2, **kw)
    kernel = sgm_kernel()
    got = torch_ops.sgm_float(_dev(t), scale, offset, P1, P2, **kw)
    assert sgm_kernel() == kernel
    if case == "fused":
        assert kernel == "sweep16/nowrap"
    names = ("bestD", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("S", "status")
    _same(got[:-1], want[:-1], names[:-1], f"{case} {dtype} {layout}")
    assert int(want[-1].item()) == 0 and int(got[-1].item()) == (0 if clean else FSGM_ERR_INVALID)


SGM2D_CASES = {
    # name: (W, H, rX, rY, n, P1, P2, format, hints, keywords)
    "plain": (33, 7, 1, 2, 1, 6, 32, FORMATS[0], False, dict()),
    "hints": (40, 9, 4, 4, 3, 6, 32, FORMATS[1], True, dict(runner_up=True)),
    "exact": (33, 7, 1, 2, 3, 7, 100, FORMATS[0], True, dict(arith="exact", runner_up=True)),
    "adaptive": (33, 7, 2, 1, 3, 6, 32, FORMATS[1], False, dict(adaptive_p2=1, arith="exact")),
    "small_bound": (40, 9, 4, 4, 3, 6, 32, (0.1, 0.0, 24), True, dict()),
}


@pytest.mark.parametrize("clean", [True, False], ids=["clean", "flagged"])
@pytest.mark.parametrize("layout", ["hwd", "dhw", "dhw_yx"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(SGM2D_CASES))
def test_sgm2d_float_equals_sgm2d_on_the_quantised_bytes(gpu_lib, case, dtype, layout, clean):
    W, H, rX, rY, n, P1, P2, (scale, offset, bound), hints, kw = SGM2D_CASES[case]
    Sx, Sy = 2 * rX + 1, 2 * rY + 1
    rng = np.random.default_rng(22)
    t, wide = _cast(_planted(rng, (n, H, W, Sx * Sy), scale, offset, bound, clean), dtype)
    q, flagged = Q.quantise(wide, scale, offset, bound)
    assert flagged.any() != clean
    kw = dict(kw, layout=layout, cost_bound=bound, return_flow=True, return_sum=True, return_status=True)
    if hints:
        kw["hints"] = torch.from_numpy(np.stack([synth.hint_map(W + 2, H + 1, "general", seed=40 + 5 * f, amp=3.0) for f in range(n)])).to(DEV)
    if kw.get("adaptive_p2"):
        kw["guide"] = _guide(n, H, W)
    want = torch_ops.sgm2d(_as2d(layout, torch.from_numpy(q), Sx, Sy).contiguous().to(DEV), rX, rY, P1, P2, **kw)
    kernel = sgm2d_kernel()
    got = torch_ops.sgm2d_float(_dev(_as2d(layout, t, Sx, Sy)), rX, rY, scale, offset, P1, P2, **kw)
    assert sgm2d_kernel() == kernel
    if case == "small_bound":
        assert kernel in ("rows", "generic")                     # (not the wrapping kernel: the declared bound selected)
    names = ("bestD", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("mvSub", "flow", "S", "status")
    _same(got[:-1], want[:-1], names[:-1], f"{case} {dtype} {layout}")
    assert int(want[-1].item()) == 0 and int(got[-1].item()) == (0 if clean else FSGM_ERR_INVALID)


def test_a_captured_stream_is_refused(gpu_lib):
    """with exact too, where the u8 form fsgm_sgm_device_exact accepts a warm captured call"""
    Cv = torch.zeros((1, 16, 9, 33), dtype=torch.float16, device=DEV)
    torch_ops.sgm_float(Cv, 1.0, arith="exact", check=True)      # warm: the plan and its buffers exist
    torch.cuda.synchronize()
    with pytest.raises(_lib.FsgmError) as ei:
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            torch_ops.sgm_float(Cv, 1.0, arith="exact")
    assert ei.value.status == 4 and "captured" in str(ei.value)
    torch.cuda.synchronize()
    torch_ops.sgm_float(Cv, 1.0, arith="exact", check=True)      # and the shape still serves eager calls


# ---------------------------------------------------------------------------------------------- 3. the host forms
@pytest.mark.parametrize("layout", ["hwd", "dhw"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_sgm_batch_float_equals_sgm_batch_on_the_quantised_bytes(gpu_lib, dtype, layout):
    rng = np.random.default_rng(31)
    W, H, D, n = 37, 9, 21, 3
    for (scale, offset, bound), kw in ((FORMATS[0], dict(paths=8)), (FORMATS[1], dict(runner_up=True)), (FORMATS[0], dict(arith="exact")),
                                       ((0.1, 0.0, 24), dict(paths=8))):
        x = _planted(rng, (n, H, W, D), scale, offset, bound, clean=True).astype(dtype)
        q, flagged = Q.quantise(x.astype(np.float32), scale, offset, bound)
        assert not flagged.any()
        if layout == "dhw":
            x, q = x.transpose(0, 3, 1, 2), q.transpose(0, 3, 1, 2)
        kw = dict(kw, layout=layout, cost_bound=bound, return_sum=True)
        want = fsgm_amd.sgm_batch(q, 7, 100, **kw)
        got = fsgm_amd.sgm_batch_float(x, scale, offset, 7, 100, **kw)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("layout", ["hwd", "dhw", "dhw_yx"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_sgm2d_batch_float_equals_sgm2d_batch_on_the_quantised_bytes(gpu_lib, dtype, layout):
    rng = np.random.default_rng(32)
    W, H, n = 33, 7, 3
    for rX, rY, (scale, offset, bound), kw in ((1, 2, FORMATS[0], dict()), (4, 4, FORMATS[1], dict(runner_up=True)),
                                               (1, 2, (0.1, 0.0, 24), dict(arith="exact", runner_up=True))):
        Sx, Sy = 2 * rX + 1, 2 * rY + 1
        x = _planted(rng, (n, H, W, Sx * Sy), scale, offset, bound, clean=True).astype(dtype)
        q, flagged = Q.quantise(x.astype(np.float32), scale, offset, bound)
        assert not flagged.any()
        x, q = (_as2d(layout, torch.from_numpy(a), Sx, Sy).contiguous().numpy() for a in (x, q))
        hints = np.stack([synth.hint_map(W + 2, H + 1, "general", seed=40 + 5 * f, amp=3.0) for f in range(n)])
        kw = dict(kw, layout=layout, cost_bound=bound, hints=hints, return_flow=True, return_sum=True)
        want = fsgm_amd.sgm2d_batch(q, rX, rY, 6, 32, **kw)
        got = fsgm_amd.sgm2d_batch_float(x, rX, rY, scale, offset, 6, 32, **kw)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_host_forms_refuse_a_flagged_volume_and_write_nothing(gpu_lib):
    lib = _bind_sgm2d(_bind_sgm(_lib.load()))
    ptr = _lib.ptr
    W, H, n = 33, 7, 2
    for plant in (300.0, -1.0, np.nan):
        # 1-D
        D = 16
        x = np.full((n, H, W, D), 7.25, np.float32)
        x[-1, -1, -1, -1] = plant
        outs = [np.full((n, H, W), 0xCDCDCDCD, np.uint32) for _ in range(3)] + [np.full((n, H, W, D), 0xCDCDCDCD, np.uint32)]
        fmt, prm = cost_format(x.dtype, 1.0, 0.0), sgm_params(lib)
        st = lib.fsgm_sgm_float_batch_host(n, ptr(x), C.byref(fmt), W, H, D, 7, 100, C.byref(prm), None, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                           ptr(outs[3]), 0)
        assert st == FSGM_ERR_INVALID and "quantises outside" in lib.fsgm_last_error().decode()
        assert all((o == 0xCDCDCDCD).all() for o in outs)
        with pytest.raises(_lib.FsgmError) as e:
            fsgm_amd.sgm_batch_float(x, 1.0)
        assert e.value.status == FSGM_ERR_INVALID
        # the flag was cleared: the same plan takes a clean volume afterwards
        x[-1, -1, -1, -1] = 7.25
        bd, mc = fsgm_amd.sgm_batch_float(x, 1.0)
        wbd, wmc = fsgm_amd.sgm_batch(np.full((n, H, W, D), 7, np.uint8))
        assert np.array_equal(bd, wbd) and np.array_equal(mc, wmc)
        # 2-D
        D = 15
        x = np.full((n, D, H, W), 7.25, np.float16)
        x[0, 0, 0, 0] = plant
        u32s = [np.full((n, H, W), 0xCDCDCDCD, np.uint32) for _ in range(3)] + [np.full((n, H, W, D), 0xCDCDCDCD, np.uint32)]
        f64s = [np.full((n, 2, H, W), -6.2e66, np.float64) for _ in range(2)]
        fmt, prm = cost_format(x.dtype, 1.0, 0.0), sgm2d_params(lib, layout="dhw")
        st = lib.fsgm_sgm2d_float_batch_host(n, ptr(x), C.byref(fmt), W, H, 1, 2, 6, 32, C.byref(prm), None, 0, 0, None, ptr(u32s[0]), ptr(u32s[1]),
                                             ptr(u32s[2]), ptr(f64s[0]), ptr(f64s[1]), ptr(u32s[3]), 0)
        assert st == FSGM_ERR_INVALID and "quantises outside" in lib.fsgm_last_error().decode()
        assert all((o == 0xCDCDCDCD).all() for o in u32s) and all((o == -6.2e66).all() for o in f64s)
        x[0, 0, 0, 0] = 7.25
        got = fsgm_amd.sgm2d_batch_float(x, 1, 2, 1.0)
        want = fsgm_amd.sgm2d_batch(np.full((n, D, H, W), 7, np.uint8), 1, 2)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
