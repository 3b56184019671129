"""GPU tests of the filtered flow for the pyramidal matchers: every stage and the whole pipeline against the numpy restatement
(tests/flow_pp_restatement.py), bit for bit -- every operation of the chain is a copy, a compare, one fp64 add or a round."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth, _lib  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError  # noqa: E402
from fsgm_amd import pyramid as _pyramid  # noqa: E402
from tests import flow_pp_inputs  # noqa: E402
from tests import flow_pp_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = np.nan


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(np.nan_to_num(got), np.nan_to_num(want), err_msg=what)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- stages
KINDS = ("general", "int", "even", "zero")


@pytest.mark.parametrize("W,H,N", [(1, 1, 1), (9, 1, 1), (1, 9, 3), (61, 47, 1), (61, 47, 3), (320, 240, 1), (320, 240, 3), (1242, 375, 1)])
def test_stages_against_the_restatement(gpu_lib, W, H, N):
    """Each stage alone on the restatement's input for it; frames of a batch hold different maps."""
    pairs = [flow_pp_inputs.flow_pair(W, H, KINDS[(k + W) % 4], seed=5 + k) for k in range(N)]
    f, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    thr_island = R.island_threshold(H, W, 0.1)
    fs, bs, c, k, g = [], [], [], [], []
    for n in range(N):
        pp, ck, why = R.chain(f[n], b[n])
        if W > 8 and H > 8:                                      # the inputs must exercise every rule and leave something
            for reason in ("outside", "partner", "mismatch", "speckle"):
                assert why[reason].any(), (reason, n)
            assert R.valid(ck).mean() >= 0.25
        fs.append(R.flow_speckle_filter(f[n])[0])
        bs.append(R.flow_speckle_filter(b[n])[0])
        c.append(R.flow_fb_check(fs[n], bs[n])[0])
        k.append(ck)
        g.append(pp[:2])
    fs, bs, c, k, g = (np.stack(a) for a in (fs, bs, c, k, g))
    one = (lambda a: a[0]) if N == 1 else (lambda a: a)          # N = 1 goes in without the batch dimension
    _same(fsgm_amd.flow_speckle_filter(one(f), 2, 100), one(fs), "speckle f")
    _same(fsgm_amd.flow_speckle_filter(one(b), 2, 100), one(bs), "speckle b")
    _same(fsgm_amd.flow_fb_check(one(fs), one(bs), 2.0), one(c), "fb check")
    _same(fsgm_amd.flow_speckle_filter(one(c), np.inf, thr_island), one(k), "island removal")
    _same(fsgm_amd.flow_in_fill(one(k)), one(g), "fill")
    _same(fsgm_amd.flow_in_fill(one(f)), one(np.stack([R.flow_in_fill(a) for a in f])), "fill of the raw flow")


@pytest.mark.parametrize("fill", [NAN, 1.25])
def test_all_nan_and_no_nan_maps(gpu_lib, fill):
    W, H = 70, 9
    f = np.full((2, H, W), fill)
    b = np.full((2, H, W), -fill)
    for got, want in ((fsgm_amd.flow_speckle_filter(f, 2, 100), R.flow_speckle_filter(f, 2, 100)[0]),
                      (fsgm_amd.flow_speckle_filter(f, 2, W * H + 1), R.flow_speckle_filter(f, 2, W * H + 1)[0]),
                      (fsgm_amd.flow_fb_check(f, b), R.flow_fb_check(f, b)[0]),
                      (fsgm_amd.flow_in_fill(f), R.flow_in_fill(f))):
        _same(got, want)
    if not np.isnan(fill):
        assert np.isnan(fsgm_amd.flow_speckle_filter(f, 2, W * H + 1)).all()
        assert not np.isnan(fsgm_amd.flow_speckle_filter(f, 2, W * H)).any()


def test_values_exactly_at_max_diff(gpu_lib):
    """Two halves of 60 pixels: a step of exactly maxDiff does not join them (the test is <), a step one ulp below does."""
    for ch in (0, 1):
        for step, joined in ((2.0, False), (np.nextafter(2.0, 0.0), True)):
            f = np.zeros((2, 6, 20))
            f[ch, :, 10:] = step
            got = fsgm_amd.flow_speckle_filter(f, 2.0, 100.0)
            _same(got, R.flow_speckle_filter(f, 2.0, 100.0)[0])
            assert np.isnan(got).all() != joined


def test_region_sizes_around_max_speckle_size(gpu_lib):
    f = np.full((2, 30, 40), NAN)
    f[:, 2:11, 3:14] = 1.0                                       # 9 x 11 = 99
    f[:, 15:25, 20:30] = -3.0                                    # 10 x 10 = 100
    got = fsgm_amd.flow_speckle_filter(f, 2, 100)
    _same(got, R.flow_speckle_filter(f, 2, 100)[0])
    assert np.isnan(got[:, 2:11, 3:14]).all() and not np.isnan(got[:, 15:25, 20:30]).any()


def test_sums_exactly_at_thr(gpu_lib):
    f = np.zeros((2, 4, 8))
    b = np.zeros((2, 4, 8))
    b[0, 0, :] = 2.0
    b[0, 1, :] = np.nextafter(2.0, 3.0)
    b[1, 2, :] = -2.0
    b[1, 3, :] = -np.nextafter(2.0, 3.0)
    got = fsgm_amd.flow_fb_check(f, b, 2.0)
    _same(got, R.flow_fb_check(f, b, 2.0)[0])
    np.testing.assert_array_equal(np.isnan(got[0]).all(axis=1), [False, True, False, True])
    _same(fsgm_amd.flow_fb_check(f, b, 0.0), R.flow_fb_check(f, b, 0.0)[0])


def _snake(W, H):
    """One 1-pixel-wide region that runs along every other row and turns at alternating ends: it crosses every 64 x 4 tile
    of the merge kernel's grid many times."""
    f = np.full((2, H, W), NAN)
    for y in range(0, H, 2):
        f[:, y, :] = 0.5
        if y + 1 < H:
            f[:, y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = 0.5
    return f


def test_a_region_that_snakes_across_workgroup_tiles(gpu_lib):
    W, H = 320, 240
    f = _snake(W, H)
    size = int(R.valid(f).sum())
    for limit, kept in ((size, True), (size + 1, False)):
        got = fsgm_amd.flow_speckle_filter(f, 2, limit)
        _same(got, R.flow_speckle_filter(f, 2, limit)[0])
        assert R.valid(got).any() == kept


def test_island_threshold_on_a_regions_exact_size(gpu_lib):
    """64 x 50 pixels, island_fraction 1/8: the threshold is exactly 400; a region of 400 stays (400 < 400 is false), 399 goes."""
    W, H = 64, 50
    thr = R.island_threshold(H, W, 0.125)
    assert thr == 400.0
    f = np.full((2, H, W), NAN)
    f[:, 2:22, 2:22] = 1.0                                       # 400, values far apart inside: any difference joins
    f[0, 2:22, 2:22] += 50.0 * synth.uniform_f64(3, (20, 20))
    f[:, 25:46, 30:49] = 7.0                                     # 21 x 19 = 399
    got = fsgm_amd.flow_speckle_filter(f, np.inf, thr)
    _same(got, R.flow_speckle_filter(f, np.inf, thr)[0])
    assert not np.isnan(got[:, 2:22, 2:22]).any() and np.isnan(got[:, 25:46, 30:49]).all()


# ---------------------------------------------------------------------------------------------- the pipeline
def _pair(W, H, seed):
    return synth.image_pair(W, H, 4, seed=seed)


def _check_pipeline(out, fwd, bwd, minC=None, **chain):
    pp, checked, gf, gb, gm = out
    _same(gf, fwd, "flow_fwd")
    _same(gb, bwd, "flow_bwd")
    want_pp, want_c, why = R.chain(fwd, bwd, **chain)
    _same(checked, want_c, "flow_checked")
    _same(pp, want_pp, "flow_pp")
    if minC is not None:
        np.testing.assert_array_equal(gm, minC)
    return why


@pytest.mark.parametrize("W,H", [(160, 120), (97, 75)])
def test_pipeline_pyd_against_the_oracle(gpu_lib, oracle, W, H):
    I0, I1 = _pair(W, H, 31)
    fwd, minC, _ = oracle.pyramidal_sgm(I0, I1, 3)
    bwd, _, _ = oracle.pyramidal_sgm(I1, I0, 3)
    out = fsgm_amd.pyramidal_flow_pp(I0, I1, 3, "pyd")
    _check_pipeline(out, fwd, bwd, minC)
    mv, _, mc = fsgm_amd.pyramidal_sgm(I0, I1, 3)                # the batch-2N run does not change the matcher's result
    _same(out[2], mv)
    np.testing.assert_array_equal(out[4], mc)


@pytest.mark.parametrize("W,H", [(160, 120), (1242, 375)])
def test_pipeline_ng_against_the_restatement(gpu_lib, W, H):
    I0, I1 = _pair(W, H, 32)
    fwd, _, minC = fsgm_amd.pyramidal_sgm_ng(I0, I1, 3)
    bwd, _, _ = fsgm_amd.pyramidal_sgm_ng(I1, I0, 3)
    _check_pipeline(fsgm_amd.pyramidal_flow_pp(I0, I1, 3, "ng"), fwd, bwd, minC)


def test_pipeline_parameters_and_rgb_batch(gpu_lib):
    W, H, N = 96, 64, 3
    I0 = np.stack([synth.uniform_u8(40 + k, (3, H, W)) for k in range(N)])
    I1 = np.stack([np.roll(I0[k], (1, 2), axis=(1, 2)) for k in range(N)])
    chain = dict(speckle_max_diff=1.5, speckle_max_size=20.0, fb_thr=1.0, island_fraction=0.03125)
    out = fsgm_amd.pyramidal_flow_pp(I0, I1, 2, "pyd", P2=40, **chain)
    for k in range(N):
        fwd, _, minC = fsgm_amd.pyramidal_sgm(I0[k], I1[k], 2, P2=40)
        bwd, _, _ = fsgm_amd.pyramidal_sgm(I1[k], I0[k], 2, P2=40)
        _check_pipeline([o[k] for o in out], fwd, bwd, minC, **chain)


def test_median_is_vmf_of_the_filled_flow(gpu_lib):
    I0, I1 = _pair(160, 120, 33)
    base = fsgm_amd.pyramidal_flow_pp(I0, I1, 3, "ng")
    med = fsgm_amd.pyramidal_flow_pp(I0, I1, 3, "ng", median=1)
    _same(med[0][:2], fsgm_amd.vmf(np.ascontiguousarray(base[0][:2])))
    _same(med[0][2], base[0][2])
    _same(med[1], base[1])


# ---------------------------------------------------------------------------------------------- host = device = torch
@pytest.mark.parametrize("matcher", ["pyd", "ng"])
def test_host_device_and_torch_forms_agree_on_a_side_stream(gpu_lib, matcher):
    """The torch op on a non-default stream, its inputs produced by kernels queued before it and its outputs consumed by
    kernels queued after it, with no synchronisation in between."""
    W, H, N = 160, 120, 2
    pairs = [_pair(W, H, 50 + k) for k in range(N)]
    I0, I1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = fsgm_amd.pyramidal_flow_pp(I0, I1, 3, matcher)
    torch_ops.pyramidal_flow_pp(_t(I0), _t(I1), 3, matcher, check=True)                   # warm: the plans exist
    host = [torch.from_numpy(a).pin_memory() for a in (I0, I1)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d0, d1 = (h.to(DEV, non_blocking=True) for h in host)
        d0 = (d0.to(torch.int16) + 0).to(torch.uint8)                                      # produced by kernels on s
        torch.cuda._sleep(20_000_000)
        outs = torch_ops.pyramidal_flow_pp(d0, d1, 3, matcher, return_status=True)
        busy = not s.query()
        valid_count = outs[0][:, 2].sum()
        checked2 = outs[1].clone()
    s.synchronize()
    assert busy, "the call waited for the device"
    assert int(outs[5].item()) == 0
    for got, w, name in zip(outs[:5], want, ("flow_pp", "flow_checked", "flow_fwd", "flow_bwd", "minC")):
        _same(_n(got), w, name)
    _same(_n(checked2), want[1])
    assert float(valid_count) == want[0][:, 2].sum()
    # the stages' device forms
    f, b = _t(want[2]), _t(want[3])
    _same(_n(torch_ops.flow_fb_check(f, b, 2.0)), fsgm_amd.flow_fb_check(want[2], want[3], 2.0))
    lib = _lib.load()
    out = torch.empty_like(f)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.fsgm_flow_speckle_filter_device(N, C.c_void_p(f.data_ptr()), W, H, 2.0, 100.0, C.c_void_p(out.data_ptr()), 0, C.c_void_p(st)))
    _same(_n(out), fsgm_amd.flow_speckle_filter(want[2], 2, 100))
    out2 = torch.empty_like(f)
    _lib.check(lib.fsgm_flow_in_fill_device(N, C.c_void_p(out.data_ptr()), W, H, C.c_void_p(out2.data_ptr()), 0, C.c_void_p(st)))
    _same(_n(out2), fsgm_amd.flow_in_fill(fsgm_amd.flow_speckle_filter(want[2], 2, 100)))


def test_single_pair_torch_wrapper(gpu_lib):
    I0, I1 = _pair(97, 75, 34)
    want = fsgm_amd.pyramidal_flow_pp(I0, I1, 3)
    got = torch_ops.pyramidal_flow_pp(_t(I0), _t(I1), 3, check=True)
    for g, w in zip(got, want):
        _same(_n(g), w)


def test_refusals(gpu_lib):
    W, H = 32, 24
    I0, I1 = _pair(W, H, 35)
    t0, t1 = _t(I0), _t(I1)
    torch_ops.pyramidal_flow_pp(t0, t1, 2, check=True)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(FsgmError) as ei:
        with torch.cuda.graph(g):
            torch_ops.pyramidal_flow_pp(t0, t1, 2)
    assert ei.value.status == 4 and "captured" in str(ei.value)
    f = _t(np.zeros((1, 2, H, W)))
    with pytest.raises(FsgmError) as ei:
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            torch_ops.flow_fb_check(f, f)
    assert ei.value.status == 4
    torch.cuda.synchronize()

    lib = _lib.load()
    _pyramid._bind_flow_pp(lib)
    prm = lib.fsgm_flow_pp_params_default(0)
    prm.pyd.numPyd = 2
    pp = torch.empty((1, 3, H, W), dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def refused(st, text):
        assert st == 1, (st, lib.fsgm_last_error())
        assert text in lib.fsgm_last_error().decode(), lib.fsgm_last_error()

    pinned = torch.from_numpy(I0).pin_memory()
    refused(lib.fsgm_pyramidal_flow_pp_device(1, p(pinned), p(t1), W, H, 1, C.byref(prm), p(pp), None, None, None, None, None, None),
            "not device memory")
    small = torch.empty((1, 2, H, W), dtype=torch.float64, device=DEV)
    # a shape the arrays do not have: more bytes than their allocations hold
    refused(lib.fsgm_pyramidal_flow_pp_device(1, p(t0), p(t1), 4096, 4096, 1, C.byref(prm), p(pp), None, None, None, None, None, None),
            "needs")
    refused(lib.fsgm_pyramidal_flow_pp_device(1, p(t0), p(t1), W, H, 1, C.byref(prm), C.c_void_p(pp.data_ptr() + 4), None, None, None, None, None, None),
            "aligned")
    refused(lib.fsgm_flow_fb_check_device(1, p(f), p(f), 4096, 4096, 2.0, p(small), 0, None), "needs")
    refused(lib.fsgm_flow_fb_check_device(1, p(f), p(f), W, H, -2.0, p(small), 0, None), "thr")
    for field, value in (("fb_thr", -1.0), ("island_fraction", 1.25), ("island_fraction", -0.5)):
        q = lib.fsgm_flow_pp_params_default(0)
        q.pyd.numPyd = 2
        setattr(q, field, value)
        refused(lib.fsgm_pyramidal_flow_pp_device(1, p(t0), p(t1), W, H, 1, C.byref(q), p(pp), None, None, None, None, None, None), field)
        with pytest.raises(FsgmError) as ei:
            fsgm_amd.pyramidal_flow_pp(I0, I1, 2, **{field: value})
        assert ei.value.status == 1
    with pytest.raises(FsgmError) as ei:
        fsgm_amd.flow_fb_check(np.zeros((2, H, W)), np.zeros((2, H, W)), -1.0)
    assert ei.value.status == 1 and "thr" in str(ei.value)
    # the library still works after the refusals
    _same(fsgm_amd.pyramidal_flow_pp(I0, I1, 2)[0], _n(torch_ops.pyramidal_flow_pp(t0, t1, 2)[0]))
