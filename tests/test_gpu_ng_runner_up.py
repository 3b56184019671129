"""GPU tests of the runner-up cost of the neighbour-guided matcher, of level 1 of both pyramid drivers and of the uniqueness
filter in pyramidal_flow_pp: bit-exact against the numpy restatement (tests/ng_runner_up_restatement.py) on the oracle's
volumes, and every other output against the same call without the switch."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth, ng as _ng, _lib  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError  # noqa: E402
from fsgm_amd import pyramid as _pyramid  # noqa: E402
from tests import ng_runner_up_restatement as NR  # noqa: E402
from tests import runner_up2d_restatement as RU2  # noqa: E402
from tests.ng_helpers import COMPACT_NAMES, kept  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NONE = NR.NO_RUNNER_UP
_cache = {}


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(np.nan_to_num(got), np.nan_to_num(want), err_msg=what)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- hint maps
# A pixel's nine hints are those of (x + dx, y + dy), dx, dy in {-8, 0, 8}, clamped to the map (calc_pyd_cost_sgm_ng.cpp:381-393):
# they agree where the map is constant over that 17 x 17 reach.  With one hint h and r = 1 the candidates are h + {-1, 0, 1}^2: no
# vector lies two from the winner's when the winner is h itself, and one does when the winner sits on the ring.
def random_hints(W, H, seed):
    """random integers in +-6 with one constant patch of 25 x 25 (or what of it fits the map) at (-3, 0), the true motion of
    synth.image_pair(.., 16) near the top left corner: the hint itself wins there"""
    mv = synth.hint_map(W, H, "int", seed=seed, amp=6.0)
    mv[0, 2:27, 3:28], mv[1, 2:27, 3:28] = -3.0, 0.0
    return mv


def blocky_hints(W, H, seed, block=24):
    """integers in +-6, constant in blocks of 24 x 24: a pixel sees one to four distinct hints -- short candidate lists, the
    compact matcher's ground -- with runners-up near the block borders and, where the hint itself wins, none inside a block"""
    coarse = synth.hint_map((W + block - 1) // block, (H + block - 1) // block, "int", seed=seed, amp=6.0)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, axis=1), block, axis=2)[:, :H, :W])


def far_hints(W, H, seed):
    """blocky hints with a band of columns spanning 4094 .. 4097 (the 4-byte key holds |v| <= 4095) and a patch near +-5000"""
    mv = blocky_hints(W, H, seed)
    mv[0, :24, :24], mv[1, :24, :24] = -3.0, 0.0                 # the true motion there (random_hints)
    cols = slice(W // 2, W // 2 + 12)
    mv[0, :, cols] = 4094.0 + (np.arange(H)[:, None] // 24 + np.arange(12)[None, :] // 6) % 4
    mv[:, H - 10:H - 2, 2:10] = np.array([5000.0, -5000.0])[:, None, None]
    return mv


def _want(oracle, key, I1, I2, mv, r, agg, sub):
    """the oracle's (minC, flow) and the restatement's minC2 from its volumes, once per input"""
    if key not in _cache:
        mc, fl, Cc, S = oracle.calc_pyd_cost_sgm_ng(I1, I2, mv, r, agg, sub, 6, 32, want_volumes=True)
        best, c, c2 = NR.ng_runner_up_of_volumes(Cc, S)
        np.testing.assert_array_equal(c, mc)                     # the restatement's winner is the oracle's
        k = kept(Cc)
        for a in (mc, fl, c2):
            a.setflags(write=False)
        _cache[key] = (mc, fl, c2, float(k.mean()), int(k.max()))
    return _cache[key]


def _check(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what} minC")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what} flow")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{what} minC2")


# ---------------------------------------------------------------------------------------------- single level
@pytest.mark.parametrize("W,H", [(1, 1), (24, 17), (61, 47)])
def test_single_level_against_the_restatement(gpu_lib, oracle, W, H):
    """1 x 1; 408 pixels: the last block's tail; an odd pixel count: idle quarter-waves.  At 1 x 1 all nine hints are the one
    pixel's and every candidate but the hint itself leaves the image: they tie, the first of them -- on the ring -- wins, and the
    candidate on the ring's other side is two away.  So that pixel has a runner-up by the rule; both kinds are asked for above it."""
    I1, I2 = synth.image_pair(W, H, 16, seed=W + 1)
    mv = random_hints(W, H, seed=H)
    want = _want(oracle, ("single", W, H), I1, I2, mv, 1, 2, 0)
    has = want[2] != NONE
    if (W, H) != (1, 1):                                         # a condition on the inputs: both kinds occur
        assert has.mean() >= 0.25 and (~has).any(), has.mean()
    got = fsgm_amd.calc_pyd_cost_sgm_ng(I1, I2, mv, 1, 2, 0, 6, 32, runner_up=True)
    _check(got, want, f"{W}x{H}")
    plain = fsgm_amd.calc_pyd_cost_sgm_ng(I1, I2, mv, 1, 2, 0, 6, 32)
    np.testing.assert_array_equal(got[0], plain[0])
    np.testing.assert_array_equal(got[1], plain[1])
    mc, fl, c2, S = fsgm_amd.calc_pyd_cost_sgm_ng(I1, I2, mv, 1, 2, 0, 6, 32, runner_up=True, return_sum=True)
    np.testing.assert_array_equal(c2, want[2])
    np.testing.assert_array_equal(S, fsgm_amd.calc_pyd_cost_sgm_ng(I1, I2, mv, 1, 2, 0, 6, 32, return_sum=True)[2])


@pytest.mark.parametrize("r", [0, 1])
def test_constant_hints_have_no_runner_up(gpu_lib, oracle, r):
    """All nine neighbours' hints agree and the hint is the true motion, so the hint itself wins everywhere: every candidate lies
    within distance 1 of the winner, the matcher considered one hypothesis.  (r = 0 leaves one vector whatever wins.)"""
    W, H = 37, 23
    I1 = synth.uniform_u8(9, (H, W))                             # white noise: no other shift matches as well
    mv = np.zeros((2, H, W))
    want = _want(oracle, ("const", r), I1, I1, mv, r, 2, 0)
    assert (want[1] == 0).all() and (want[2] == NONE).all()      # a condition on the inputs, from the restatement alone
    I2 = I1
    got = fsgm_amd.calc_pyd_cost_sgm_ng(I1, I2, mv, r, 2, 0, 6, 32, runner_up=True)
    _check(got, want, f"constant hints r={r}")
    assert (got[2] == NONE).all()


# ---------------------------------------------------------------------------------------------- the WTA's sources
# (ng_level_enqueue and the FSGM_NG_* switches of DESIGN.md 4.5)   name: (r, hints, environment, the matcher that must have run)
SOURCES = {
    "compact_k4": (1, blocky_hints, {"FSGM_NG_COMPACT_G": "64"}, COMPACT_NAMES),     # sums in L4, vectors from the 4-byte keys
    # a key that does not fit: the 12-byte list is written.  The rule of ng_choose then steps aside from the compact matcher
    # (kstat bit 1), so the sums come from S: the matcher's name is recorded, not asserted
    "key_overflow": (1, far_hints, {"FSGM_NG_COMPACT_G": "64"}, None),
    "no_compact": (1, blocky_hints, {"FSGM_NG_COMPACT": "0"}, ("split2", "lines", "grid", "list")),   # S through the kept table, Cand list
    "no_k4": (1, blocky_hints, {"FSGM_NG_K4": "0"}, COMPACT_NAMES),                  # 12-byte entries from the start: L4's sums, Cand list
    "generic_225": (2, random_hints, {}, ("generic",)),                              # no table: all D candidates, 15 rounds
    "nine": (0, random_hints, {}, None),                                             # D = 9: one round, 7 idle lanes a pixel
}


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("source", list(SOURCES))
def test_every_source_of_the_wta(gpu_lib, oracle, monkeypatch, source, sub, frames):
    r, hints, env, names = SOURCES[source]
    W, H = 61, 47
    ins, wants = [], []
    for i in range(frames):
        I1, I2 = synth.image_pair(W, H, 16, seed=70 + i)
        mv = hints(W, H, seed=80 + i)
        ins.append((I1, I2, mv))
        wants.append(_want(oracle, (source, sub, i), I1, I2, mv, r, 2, sub))
    c2 = np.stack([w[2] for w in wants])
    if r <= 1:                                                   # conditions on the inputs: both kinds occur
        assert (c2 != NONE).mean() >= 0.25 and (c2 == NONE).any()
    else:                                                        # r = 2 reaches two away from any hint: every pixel has one
        assert (c2 != NONE).all()
    if names == COMPACT_NAMES:                                   # what ng_choose asks of the lists before a compact kernel runs
        assert max(w[4] for w in wants) <= 64 and np.mean([w[3] for w in wants]) < 40
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if frames == 1:
        got = [fsgm_amd.calc_pyd_cost_sgm_ng(*ins[0], r, 2, sub, 6, 32, runner_up=True)]
        ran = _ng.last_decision()[0]
        plain = [fsgm_amd.calc_pyd_cost_sgm_ng(*ins[0], r, 2, sub, 6, 32)]
    else:
        got = fsgm_amd.calc_pyd_cost_sgm_ng_batch(ins, r, 2, sub, 6, 32, runner_up=True)
        ran = _ng.last_decision()[0]
        plain = fsgm_amd.calc_pyd_cost_sgm_ng_batch(ins, r, 2, sub, 6, 32)
    print(f"{source} sub={sub} frames={frames}: matcher {ran}")
    if names is not None:
        assert ran in names, ran
    for i, (g, w, p) in enumerate(zip(got, wants, plain)):
        _check(g, w, f"{source} sub={sub} frame {i}")
        np.testing.assert_array_equal(g[0], p[0])
        np.testing.assert_array_equal(g[1], p[1])
    if sub:                                                      # the flow changes with the sub-pixel step, minC2 does not
        for i in range(frames):
            np.testing.assert_array_equal(wants[i][2], _want(oracle, (source, 0, i), *ins[i], r, 2, 0)[2])


# ---------------------------------------------------------------------------------------------- pyramids
def _pair(W, H, seed):
    """shifts of up to 15 pixels: level 1's hints vary, so its candidate lists hold vectors two and more apart (with shifts below
    two pixels the hint itself wins everywhere and no pixel of the neighbour-guided level 1 has a runner-up)"""
    return synth.image_pair(W, H, 32, seed=seed)


def _ng_level1_want(oracle, plan_flow2, g0, g1, W, H):
    """the single-level restatement fed level 1's gray images and hints: 2 * imresize(flow of level 2, 2, 'nearest')"""
    hint = 2.0 * np.repeat(np.repeat(plan_flow2, 2, axis=1), 2, axis=2)
    mc, fl, Cc, S = oracle.calc_pyd_cost_sgm_ng(g0, g1, np.ascontiguousarray(hint), 1, 2, 0, 6, 32, want_volumes=True)
    return mc, fl, NR.ng_runner_up_of_volumes(Cc, S)[2]


@pytest.mark.parametrize("W,H", [(97, 75), (160, 120)])
def test_ng_pyramid_level_one(gpu_lib, oracle, W, H):
    I0, I1 = _pair(W, H, 41)
    plain = fsgm_amd.pyramidal_sgm_ng(I0, I1, 3)                 # a cached plain plan first
    with fsgm_amd.NgPyramidPlan(W, H, 1, 3) as plan:
        plan.upload(I0, I1)
        plan.run()
        with pytest.raises(FsgmError, match="switch is off"):
            plan.download_runner_up()
        plan.set_runner_up()
        plan.run()
        flow2, _ = plan.download(2)
        flow1, minC1 = plan.download(1)
        minC2 = plan.download_runner_up()
    mc, fl, want2 = _ng_level1_want(oracle, flow2, I0, I1, W, H)
    np.testing.assert_array_equal(minC1, mc)
    np.testing.assert_array_equal(flow1, fl)
    np.testing.assert_array_equal(minC2, want2)
    assert (want2 != NONE).any()
    got = fsgm_amd.pyramidal_sgm_ng(I0, I1, 3, runner_up=True)
    assert len(got) == 4
    np.testing.assert_array_equal(got[3], want2)
    again = fsgm_amd.pyramidal_sgm_ng(I0, I1, 3)                 # warm plain call after the runner-up call, and the reverse
    got2 = fsgm_amd.pyramidal_sgm_ng(I0, I1, 3, runner_up=True)
    assert len(again) == 3 and len(got2) == 4
    for a, b, c in zip(plain, again, got):
        for x, y, z in zip(*(([v] if isinstance(v, np.ndarray) else v) for v in (a, b, c))):
            np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(x, z)
    np.testing.assert_array_equal(got2[3], want2)


@pytest.mark.parametrize("W,H", [(97, 75), (160, 120)])
def test_pyd_pyramid_level_one(gpu_lib, oracle, W, H):
    I0, I1 = _pair(W, H, 42)
    plain = fsgm_amd.pyramidal_sgm(I0, I1, 3)
    with fsgm_amd.PyramidPlan(W, H, 1, 3) as plan:
        plan.upload(I0, I1)
        plan.run()
        with pytest.raises(FsgmError, match="switch is off"):
            plan.download_runner_up()
        plan.set_runner_up()
        plan.run()
        flow2, _ = plan.download(2)
        flow1, minC1 = plan.download(1)
        minC2 = plan.download_runner_up()
    hint = np.ascontiguousarray(2.0 * np.repeat(np.repeat(flow2, 2, axis=1), 2, axis=2))     # pyramidal_sgm.m:72
    bd, mc, ms, Cv, S = oracle.calc_pyd_cost_sgm(I0, I1, hint, 5, 5, 2, 1, 6, 32, 1, 2, 0, want_volumes=True)
    best, c, want2 = RU2.runner_up2d(S, 11, 11)
    np.testing.assert_array_equal(c, mc)
    np.testing.assert_array_equal(minC1, mc)
    np.testing.assert_array_equal(minC2, want2)
    assert (want2 != NONE).any()
    got = fsgm_amd.pyramidal_sgm(I0, I1, 3, runner_up=True)
    again = fsgm_amd.pyramidal_sgm(I0, I1, 3)
    got2 = fsgm_amd.pyramidal_sgm(I0, I1, 3, runner_up=True)
    assert len(got) == 4 and len(again) == 3 and len(got2) == 4
    np.testing.assert_array_equal(got[3], want2)
    np.testing.assert_array_equal(got2[3], want2)
    for a, b, c in zip(plain, again, got):
        for x, y, z in zip(*(([v] if isinstance(v, np.ndarray) else v) for v in (a, b, c))):
            np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(x, z)
    np.testing.assert_array_equal(flow1, plain[0])


# ---------------------------------------------------------------------------------------------- the pipeline
def _pick_ratio(cf, c2f):
    """on the CPU, from the restatement alone: the first ratio that rejects between 5 % and 95 % of the forward pixels"""
    for ratio in (15, 5, 10, 25, 40, 60, 80, 2, 1, 95):
        share = NR.uniqueness_reject(cf, c2f, ratio).mean()
        if 0.05 <= share <= 0.95:
            return ratio, share
    raise AssertionError("no ratio rejects between 5 % and 95 % of the forward pixels")


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("matcher", ["pyd", "ng"])
@pytest.mark.parametrize("W,H", [(97, 75), (160, 120)])
def test_pipeline_with_a_ratio(gpu_lib, W, H, matcher, N):
    run = fsgm_amd.pyramidal_sgm if matcher == "pyd" else fsgm_amd.pyramidal_sgm_ng
    pairs = [_pair(W, H, 60 + k) for k in range(N)]
    I0, I1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    arg = (lambda a: a) if N > 1 else (lambda a: a[0])
    plain = fsgm_amd.pyramidal_flow_pp(arg(I0), arg(I1), 3, matcher)
    zero = fsgm_amd.pyramidal_flow_pp(arg(I0), arg(I1), 3, matcher, uniqueness_ratio=0)
    assert len(plain) == 5 and len(zero) == 6
    for g, w, name in zip(zero, plain, ("flow_pp", "flow_checked", "flow_fwd", "flow_bwd", "minC")):
        _same(g, w, f"ratio 0 {name}")
    f = [run(a, b, 3, runner_up=True) for a, b in pairs]        # (flow, levels, minC, minC2) of each direction on its own
    b = [run(b_, a, 3, runner_up=True) for a, b_ in pairs]
    ratio, share = _pick_ratio(np.stack([x[2] for x in f]), np.stack([x[3] for x in f]))
    print(f"{matcher} {W}x{H} N={N}: ratio {ratio} rejects {share:.3f} of the forward pixels")
    host = fsgm_amd.pyramidal_flow_pp(arg(I0), arg(I1), 3, matcher, uniqueness_ratio=ratio)
    outs = [o if N > 1 else o[None] for o in host]
    for k in range(N):
        want_pp, want_c, _ = NR.flow_pp_u(f[k][0], b[k][0], f[k][2], f[k][3], b[k][2], b[k][3], ratio)
        _same(outs[0][k], want_pp, "flow_pp")
        _same(outs[1][k], want_c, "flow_checked")
        _same(outs[2][k], f[k][0], "flow_fwd stays raw")
        _same(outs[3][k], b[k][0], "flow_bwd stays raw")
        np.testing.assert_array_equal(outs[4][k], f[k][2])
        np.testing.assert_array_equal(outs[5][k], f[k][3])
    # the device form on a side stream, through the torch wrapper
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = torch_ops.pyramidal_flow_pp(_t(arg(I0)), _t(arg(I1)), 3, matcher, uniqueness_ratio=ratio, return_status=True)
    s.synchronize()
    assert int(dev[6].item()) == 0
    for g, w in zip(dev[:6], host):
        _same(_n(g), w)
    plain_again = fsgm_amd.pyramidal_flow_pp(arg(I0), arg(I1), 3, matcher)     # the plain plan is still the plain plan
    for g, w in zip(plain_again, plain):
        _same(g, w)


def test_pipeline_refusals(gpu_lib):
    I0, I1 = _pair(32, 24, 5)
    lib = _lib.load()
    prm = _pyramid.flow_pp_params(lib, "ng", 2, 0, 0, {})
    pp, c2 = np.zeros((3, 24, 32)), np.zeros((24, 32), np.uint32)
    p = _lib.ptr
    for ratio, m2, word in ((-1, p(c2), "uniqueness_ratio"), (101, p(c2), "uniqueness_ratio"), (15, None, "minC2")):
        st = lib.fsgm_pyramidal_flow_pp_host_u(1, p(I0), p(I1), 32, 24, 1, C.byref(prm), ratio, p(pp), None, None, None, None, m2)
        assert st == 1 and word in lib.fsgm_last_error().decode()
    for ratio in (-1, 101):
        with pytest.raises(ValueError, match="uniqueness_ratio"):
            fsgm_amd.pyramidal_flow_pp(I0, I1, 2, "ng", uniqueness_ratio=ratio)
    assert not pp.any()


# ---------------------------------------------------------------------------------------------- torch
@pytest.mark.parametrize("matcher", ["pyd", "ng"])
def test_torch_pyramids_on_a_side_stream(gpu_lib, matcher):
    W, H, N = 97, 75, 2
    host_fn = fsgm_amd.pyramidal_sgm if matcher == "pyd" else fsgm_amd.pyramidal_sgm_ng
    op = torch_ops.pyramidal_sgm if matcher == "pyd" else torch_ops.pyramidal_sgm_ng
    pairs = [_pair(W, H, 90 + k) for k in range(N)]
    I0, I1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = [host_fn(a, b, 3, runner_up=True) for a, b in pairs]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d0 = (_t(I0).to(torch.int16) + 0).to(torch.uint8)        # produced by kernels on s
        flow, minC, minC2, status = op(d0, _t(I1), 3, runner_up=True, return_status=True)
        plain = op(d0, _t(I1), 3)
        total = minC2.to(torch.int64).sum()                      # consumed by a kernel on s
    s.synchronize()
    assert int(status.item()) == 0 and tuple(minC2.shape) == (N, H, W)
    for k in range(N):
        np.testing.assert_array_equal(_n(flow[k]), want[k][0])
        np.testing.assert_array_equal(_n(minC[k]), want[k][2])
        np.testing.assert_array_equal(_n(minC2[k]), want[k][3])
    assert int(total) == int(sum(w[3].astype(np.int64).sum() for w in want))
    assert len(plain) == 2
    np.testing.assert_array_equal(_n(plain[0]), _n(flow))
    np.testing.assert_array_equal(_n(plain[1]), _n(minC))
    one = op(_t(I0[0]), _t(I1[0]), 3, runner_up=True, check=True)
    np.testing.assert_array_equal(_n(one[2]), want[0][3])
