"""One-shot calls on warm cached plans: every call here meets a plan that an earlier call -- of another form, with other
penalties, costs, bounds, ranges, outputs -- left behind, or one that was evicted and built again.

The seeded sequences come from tests/call_sequences.py (their draws are checked in tests/test_call_sequences_cpu.py); every
returned array is compared for equality with the oracle's or a restatement's answer for the step's own arguments, and where the
call reports the kernel that ran, with what a fresh plan would choose.  The directed cases below them run A, B, A on one key, one
per hazard read from cached_plan, epi_prepare, set_penalties (fsgm_amd/csrc/capi_epi.hip), stereo_host (capi_stereo.hip) and
sgm_run_* (capi_sgm.hip)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch  # noqa: I001 -- before the library: its HIP runtime is the one libfsgm_hip.so binds to (fsgm_amd/torch_ops.py)

import fsgm_amd  # noqa: E402
from fsgm_amd import _lib, synth, torch_ops  # noqa: E402
from fsgm_amd._lib import FsgmError  # noqa: E402
from fsgm_amd.sgm import last_kernel, sgm_batch  # noqa: E402
from tests import budget_volumes as BV  # noqa: E402
from tests import call_sequences as CS  # noqa: E402
from tests import ng_helpers as NG  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def side():
    return torch.cuda.Stream()


def _same(got, want, what):
    """equal arrays; doubles: NaNs at the same places, every other value equal (tests/test_gpu_post.py)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} for {want.dtype}{want.shape}"
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaNs moved"
        got, want = np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def _check_step(s, side, what):
    """run the step and hold everything it returns against its expectation; returns the kernel it reported ('' if none)"""
    if s.refuse is not None:
        with pytest.raises(FsgmError) as e:
            CS.run(s)
        assert e.value.status == INVALID and s.refuse in str(e.value), what
        return ""
    got, want = CS.run(s, stream=side), CS.expected(s)
    kernel = last_kernel() if CS.FAMILY[s.form] == "sgm_batch" else ""
    what = f"{what} [{kernel}]"
    if kernel:
        assert kernel == CS.pipeline(s), f"{what}: a fresh plan runs {CS.pipeline(s)}"
    assert set(got) == set(want), what
    for name in sorted(want):
        if name == "status":
            assert got[name] == want[name], f"{what}: status {got[name]} for {want[name]}"
        else:
            _same(got[name], want[name], f"{what}: {name}")
    return kernel


@pytest.mark.parametrize("seed", CS.EPI_SEEDS)
def test_epi_sequence(gpu_lib, oracle, side, seed):
    steps = CS.epi_sequence(seed)
    walk = CS.cache_walk(steps)
    kernels = []
    for i, (s, w) in enumerate(zip(steps, walk)):
        prev = w["prev"]
        state = "cold" if not w["hit"] else f"warm, last used by step {prev}: {steps[prev]} [{kernels[prev]}]"
        if w["returned"]:
            state = "built again after an eviction"
        kernels.append(_check_step(s, side, f"seed {seed} step {i} ({state}): {s}"))


# ------------------------------------------------------------------------------------------------------------ directed cases
def _base(form, W, H, D, batch, paths, **kw):
    d = dict(form=form, W=W, H=H, D=D, batch=batch, paths=paths, vz=0, adaptive=0, agg_mode=0, direction=-1, P1=6, P2=64, subpixel=1,
             vMax=0.3, d_min=None, vol_cmax=24, cost_bound=255, guide=False, want_S=False, want_C=False, seed=1, refuse=None)
    d.update(kw)
    return CS.Step(**d)


def _walk(steps, side, what):
    keys = {CS.key(s) for s in steps if s.refuse is None}
    assert len(keys) == 1, f"{what}: the steps of a directed case share one key"
    for i, s in enumerate(steps):
        _check_step(s, side, f"{what}, call {i}: {s}")


@pytest.mark.parametrize("paths", [8, 4])
def test_device_sgm_then_the_host_forms_of_one_key(gpu_lib, oracle, side, paths):
    """sgm_run_device leaves cmax = cost_bound = 24 and the no-wrap kernels selected; fsgm_sgm_host and calc_cost_sgm without the
    vz conversion get that plan with costs up to 255 (upload_cost) or census costs (prepare) and must select again.
    The handover here is between the two forms of the LINE kernels (packed16/nowrap, then packed16/wrap): auto mode keeps one
    frame of this size on them, and a forced fused mode is part of the key, so the host forms never meet a fused plan.  No test
    covers a fused-to-lines handover across families; within sgm(C) the sequences and the 17-frame case below do."""
    W, H, D = 37, 21, 32
    dev = _base("sgm_torch", W, H, D, 1, paths, vol_cmax=24, cost_bound=24, want_S=True)
    assert CS.pipeline(dev) == "packed16/nowrap" and CS.pipeline(dev._replace(cost_bound=255)) == "packed16/wrap"
    host = _base("sgm", W, H, D, 1, paths, vol_cmax=255, want_S=True)
    cost = _base("calc_cost_sgm", W, H, D, 1, paths, P1=100, P2=200, want_S=True, want_C=True)
    batch = _base("sgm_batch", W, H, D, 1, paths, vol_cmax=255, subpixel=0)
    _walk([dev, host, dev, cost, dev, batch, cost._replace(P1=6, P2=64), host, dev], side, f"{paths} paths")


def test_vmax_alone_changes_between_calls(gpu_lib, oracle, side):
    """set_penalties clears vz_valid when vMax moves: the vz table and the conversion follow"""
    a = _base("calc_cost_sgm", 13, 26, 64, 2, 4, vz=1, vMax=0.3)
    b = a._replace(vMax=0.5)
    assert not np.array_equal(CS.expected(a)["bestD"], CS.expected(b)["bestD"])
    _walk([a, b, a, a._replace(vMax=0.125), a], side, "vMax")


def test_d_min_alone_changes_between_calls(gpu_lib, oracle, side):
    a = _base("stereo_sgm", 61, 9, 16, 2, 8, direction=1, d_min=-17)
    b, c = a._replace(d_min=None), a._replace(d_min=7)
    assert not np.array_equal(CS.expected(a)["minC"], CS.expected(b)["minC"])
    _walk([a, b, a, c, b, a._replace(d_min=0)], side, "d_min")


def test_penalties_walk_a_batch_plan_across_the_budget_and_back(gpu_lib, oracle):
    """17 frames (tests/test_gpu_fused_budgets.py's large-batch forms), mode 2: the block sweeps at (21, 64), the line kernels and
    the S tap at (22, 64), the sweeps again"""
    D = 64
    W, H = BV.sweep_shape(D)
    vols = np.stack(BV.volumes(W, H, D, BV.nowrap_cmax(22, 64), seed=1000 + D, n=17))
    want = {}
    for P1 in (21, 22):
        S = [oracle.epi_aggregate(v, P1, 64, 8) for v in vols]
        bd, mc = zip(*[oracle.epi_wta(s, W, H, D, 1) for s in S])
        want[P1] = (np.stack(bd), np.stack(mc), np.stack([s[:-1].reshape(H, W, D) for s in S]))
    for i, (P1, name) in enumerate([(21, "sweep16/nowrap"), (22, "packed16/nowrap"), (21, "sweep16/nowrap")]):
        got = sgm_batch(vols, P1, 64, paths=8, agg_mode=2, cost_bound=127, return_sum=(i == 1))
        assert last_kernel() == name, f"call {i}"
        for g, w, n in zip(got, want[P1], ("bestD", "minC", "S")):
            _same(g, w, f"call {i} (P1 {P1}, {name}): {n}")


def test_a_refused_call_between_two_good_ones(gpu_lib, oracle, side):
    lib = gpu_lib
    # adaptive P2 without its guide, on the shape of a warm adaptive plan
    a = _base("sgm_batch", 19, 13, 48, 2, 8, adaptive=1, guide=True, want_S=True)
    _walk([a, a._replace(guide=False, refuse="adaptive_p2 needs the guide image"), a], side, "missing guide")
    # d_min beyond its limit, straight at the entry point (the Python wrapper would refuse it first)
    s = _base("stereo_sgm", 61, 9, 16, 1, 4, d_min=7)
    _check_step(s, side, "d_min, before")
    I1, I2 = CS.images(s.W, s.H, s.D, s.seed, 0)
    disp, minC = np.zeros((s.H, s.W), np.int32), np.zeros((s.H, s.W), np.uint32)
    prm, opt = fsgm_amd.epi._stereo_params(4, 1, -1, 0, 0), _lib.options(0)
    st = lib.fsgm_stereo_sgm_host_range(1, _lib.ptr(I1), _lib.ptr(I2), s.W, s.H, s.D, 6, 64, C.byref(prm), C.byref(opt), 1025,
                                        _lib.ptr(disp), _lib.ptr(minC), None, None)
    assert st == INVALID and b"|d_min| must be <= 1024" in lib.fsgm_last_error() and not disp.any()
    _check_step(s, side, "d_min, after")
    _check_step(s._replace(d_min=None), side, "d_min, after, no range")
    # a window beyond 1024 candidates between two calls of the pyramidal matcher on one key
    W, H = 21, 13
    I1, I2 = synth.image_pair(W, H, 16, seed=4)
    mv = synth.hint_map(W, H, "general", seed=9, amp=3.0)
    args = (2, 1, 2, 1, 6, 32, 1, 2, 0)
    want = oracle.calc_pyd_cost_sgm(I1, I2, mv, *args)
    for i in range(2):
        for g, w, n in zip(fsgm_amd.calc_pyd_cost_sgm(I1, I2, mv, *args), want, ("bestD", "minC", "mvSub")):
            _same(g, w, f"pyd call {i}: {n}")
        if i == 0:
            with pytest.raises(FsgmError) as e:
                fsgm_amd.calc_pyd_cost_sgm(I1, I2, mv, 16, 16, 2, 1, 6, 32, 1, 2, 0)
            assert e.value.status == UNSUPPORTED


def test_adaptive_and_plain_callers_of_one_shape_never_share_a_plan(gpu_lib, oracle, side):
    """adaptive is part of the key: the plain caller must not get the adaptive caller's plan, nor the other way round"""
    a = _base("calc_cost_sgm", 37, 21, 32, 2, 8, vz=1)
    c = _base("sgm_batch", 37, 21, 32, 2, 8, guide=True, want_S=True)
    for plain in (a, c):
        adaptive = plain._replace(adaptive=1)
        assert CS.key(plain) != CS.key(adaptive)
        assert not np.array_equal(CS.expected(plain)["minC"], CS.expected(adaptive)["minC"]), "the edge must matter"
        for i, s in enumerate([plain, adaptive, plain, adaptive]):
            _check_step(s, side, f"{plain.form}, call {i}: {s}")


def test_pyd_parameters_walk_one_key(gpu_lib, oracle):
    """g_pyd's key holds shape and window only: set_params must bring every other parameter along, and mvSub of a call without
    the sub-pixel refinement is zeros again"""
    W, H, rX, rY, rAgg = 29, 17, 2, 3, 2
    I1, I2 = synth.image_pair(W, H, 16, seed=6)
    mv = synth.hint_map(W, H, "general", seed=11, amp=3.0)
    # (subPixelRefine, P1, P2, diagonal, totalPass, adaptiveP2)
    calls = [(1, 6, 32, 1, 3, 1), (1, 6, 32, 1, 1, 1), (1, 6, 32, 1, 2, 1), (1, 6, 32, 0, 2, 1), (1, 6, 32, 0, 2, 0), (0, 6, 32, 0, 2, 0),
             (1, 100, 200, 1, 2, 0), (0, 6, 32, 1, 3, 1), (1, 6, 32, 1, 3, 1)]
    wants = [oracle.calc_pyd_cost_sgm(I1, I2, mv, rX, rY, rAgg, *c) for c in calls]
    assert len({w[0].tobytes() + w[2].tobytes() for w in wants[:7]}) == 7, "every change must matter"
    for i, (c, want) in enumerate(zip(calls, wants)):
        got = fsgm_amd.calc_pyd_cost_sgm(I1, I2, mv, rX, rY, rAgg, *c)
        for g, w, n in zip(got, want, ("bestD", "minC", "mvSub")):
            _same(g, w, f"call {i} {c} after {calls[i - 1] if i else None}: {n}")
        if c[0] == 0:
            assert not got[2].any(), f"call {i}: mvSub without the refinement"


def test_eviction_and_return_host_forms(gpu_lib, oracle, side):
    """cap + 1 keys, then the first again: 4 + 1 for g_epi, 6 + 1 for g_pyd"""
    steps = [_base("sgm", W, 9, 16, 1, 8, vol_cmax=255, want_S=True) for W in (61, 60, 59, 58, 57)]
    walk = CS.cache_walk(steps + steps[:1])
    assert walk[4]["evicted"] == CS.key(steps[0]) and walk[5]["returned"]
    for i, s in enumerate(steps + steps[:1]):
        _check_step(s, side, f"epi key {i}")
    I = [synth.image_pair(W, 11, 16, seed=W) for W in range(20, 27)]
    mvs = [synth.hint_map(W, 11, "general", seed=W, amp=2.0) for W in range(20, 27)]
    for i in list(range(7)) + [0]:
        want = oracle.calc_pyd_cost_sgm(*I[i], mvs[i], 1, 1, 2, 1, 6, 32, 1, 2, 0)
        for g, w, n in zip(fsgm_amd.calc_pyd_cost_sgm(*I[i], mvs[i], 1, 1, 2, 1, 6, 32, 1, 2, 0), want, ("bestD", "minC", "mvSub")):
            _same(g, w, f"pyd key {i}: {n}")


def test_eviction_with_the_evicted_plans_work_still_queued(gpu_lib, oracle, side):
    """Device form: key A's call is queued on a side stream, four more keys follow on the same stream without a wait -- the last
    of them evicts A's plan, whose work may not have run yet (fsgm_epi_plan_destroy drains it first) -- then everything is
    compared, A's outputs included."""
    steps = [_base("sgm_torch", W, 9, 16, 2, 8, cost_bound=24, want_S=True) for W in (61, 60, 59, 58, 57)]
    outs = []
    with torch.cuda.stream(side):
        for s in steps:
            Ct = torch.from_numpy(np.ascontiguousarray(CS.volumes(s).transpose(0, 3, 1, 2))).to(DEV, non_blocking=True)
            outs.append(torch_ops.sgm(Ct, s.P1, s.P2, layout="dhw", paths=8, cost_bound=24, return_sum=True, return_status=True))
    side.synchronize()
    for i, (s, got) in enumerate(zip(steps, outs)):
        want = CS.expected(s)
        assert int(got[3].item()) == 0
        for g, n in zip(got, ("bestD", "minC", "S")):
            _same(g.cpu().numpy(), want[n], f"key {i}: {n}")
    _check_step(steps[0], side, "the first key again")


def _ng_fresh_choice(want, W, H, D, frames):
    """The matcher the last level reported against what a fresh call must find: the sample size is the host rule's for this
    many pixels, the summed list lengths of the sample lie between that many of the ORACLE's shortest and longest candidate
    lists, and the name is the rule's answer for those statistics (the level samples a subset of the pixels that only the
    device knows, so the sum itself cannot be restated)."""
    ng = fsgm_amd.ng
    name, s, n, flags = ng.last_decision()
    assert name == ng.auto_matcher(W, H, D, frames, s, n, flags), (name, s, n, flags)
    if n:                                                        # (a set of one member takes no statistics)
        kept = np.concatenate([NG.kept(w[2]) for w in want])
        assert n == ng.sample_pixels(W * H * frames), (n, W, H, frames)
        assert n * int(kept.min()) <= s <= n * int(kept.max()), (s, n, int(kept.min()), int(kept.max()))
    return name


def test_ng_arena_shrinks_after_eight_small_calls_and_grows_again(gpu_lib, oracle):
    """Three 40 x 30 frames at halfSearchWinSize 2 (225 candidates) take 3 * 270000 * 24 bytes of candidate buffers, above the
    16 MiB from which the arena counts small calls (DevBufs::commit, capi_ng.hip); nine single 8 x 6 frames at halfSearchWinSize 0
    use less than a quarter of it, so the eighth gives the arena back and carves a small one; the large batch then grows it
    again.  All eleven answers against the oracle, S on the first and the last through the single-frame call."""
    assert 3 * 40 * 30 * 225 * 24 >= 1 << 24
    big, want_big = NG.ng_frames(oracle, 40, 30, 3, "general", 2.0, r=2)
    small, want_small = NG.ng_frames(oracle, 8, 6, 9, "general", 2.0, r=0)
    NG.run_and_compare(big[:1], want_big[:1], r=2, what="one large frame, S")
    NG.run_and_compare(big, want_big, r=2, what="large batch, first")
    _ng_fresh_choice(want_big, 40, 30, 225, 3)
    for i in range(9):
        gmc, gfl = fsgm_amd.calc_pyd_cost_sgm_ng(*small[i], 0, 2, 0, 6, 32)
        _same(gmc, want_small[i][0], f"small {i}: minC")
        _same(gfl, want_small[i][1], f"small {i}: flow")
        _ng_fresh_choice(want_small[i:i + 1], 8, 6, 9, 1)
    NG.run_and_compare(big, want_big, r=2, what="large batch, again")
    _ng_fresh_choice(want_big, 40, 30, 225, 3)
    NG.run_and_compare(big[:1], want_big[:1], r=2, what="one large frame, S, again")


def test_two_host_threads_across_the_cache(gpu_lib, oracle, side):
    """Each thread alternates between two keys; the four keys and a fifth that the main thread warmed exceed g_epi's cap, so the
    threads keep evicting each other's plans (tests/test_gpu_post_batch.py's pattern)."""
    _check_step(_base("sgm", 23, 9, 144, 1, 4), side, "fifth key")
    pairs = [[_base("sgm", 37, 21, 32, 1, 8, vol_cmax=255, want_S=True), _base("stereo_sgm", 61, 9, 16, 2, 4, d_min=-17)],
             [_base("calc_cost_sgm", 13, 26, 64, 1, 4, vz=1, vMax=0.5), _base("sgm_batch", 19, 13, 48, 2, 8, P1=100, P2=200)]]
    for p in pairs:
        for s in p:
            CS.expected(s)                                       # (computed once, here: the threads only compare)
    errors = []

    def loop(mine):
        try:
            for it in range(10):
                for s in mine:
                    got, want = CS.run(s), CS.expected(s)
                    for n in want:
                        _same(got[n], want[n], f"iteration {it}, {s.form}: {n}")
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=loop, args=(p,)) for p in pairs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a thread is stuck"
    assert not errors, errors


# ------------------------------------------------------------------------------------------ a smaller bound, then a cost stage
def test_a_small_bound_then_a_cost_stage_on_one_key(gpu_lib, oracle, side):
    """sgm(C) with costs up to 4 leaves cmax = 4, for which (120, 125) does not wrap (4 + 250 <= 255); calc_cost_sgm without the
    vz conversion on that plan brings census costs up to 24 (24 + 250 > 255: a path state of up to 24 + 125 plus P1 passes a
    byte): epi_prepare() must put cmax back to 24 and select the wrapping kernels.  In device and in host form."""
    W, H, D = 61, 9, 16
    P = dict(P1=120, P2=125)
    cost = _base("calc_cost_sgm", W, H, D, 1, 8, want_S=True, want_C=True, **P)
    assert int(CS.expected(cost)["C"].max()) + 125 + 120 > 255, "no cost large enough for a path state + P1 to pass a byte"
    dev = _base("sgm_torch", W, H, D, 1, 8, vol_cmax=4, cost_bound=4, want_S=True, **P)
    host = _base("sgm_batch", W, H, D, 1, 8, vol_cmax=4, cost_bound=255, **P)
    assert CS.pipeline(dev) == CS.pipeline(host) == "packed16/nowrap" and CS.pipeline(cost) == "packed16/wrap"
    _walk([dev, cost, dev, host, cost, _base("sgm", W, H, D, 1, 8, vol_cmax=4, **P), cost], side, "small bound")


# ------------------------------------------------------------------------------------------------------- sgm2d on one key
_sgm2d_want, _sgm2d_inputs = CS.sgm2d_want, CS.sgm2d_inputs


def _sgm2d_call(form, side, vols, hints, guide, rX, rY, P1, P2, **kw):
    from fsgm_amd import sgm2d_batch
    src = np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
    if form == "host":
        return sgm2d_batch(src, rX, rY, P1, P2, layout="dhw", hints=hints, guide=guide, return_flow=True, return_sum=True, **kw), 0
    with torch.cuda.stream(side):
        t = lambda a: None if a is None else torch.from_numpy(a).to(DEV, non_blocking=True)  # noqa: E731
        *got, st = torch_ops.sgm2d(t(src), rX, rY, P1, P2, layout="dhw", hints=t(hints), guide=t(guide), return_flow=True,
                                   return_sum=True, return_status=True, **kw)
    side.synchronize()
    return tuple(g.cpu().numpy() for g in got), int(st.item())


def test_sgm2d_parameters_walk_one_key(gpu_lib, oracle, side):
    """g_sgm2d keys a plan by shape, window, hint-map size, batch and whether a guide is held: the path set, the passes, adaptive
    P2, the refinement, the penalties, the bound and the hints themselves (present, absent: the plan's own map must be zeros
    again) all move on a warm plan, through the host and the device form in turn (adaptive P2 decides whether a guide is held,
    so the adaptive and the plain calls alternate between two plans of the cache).  The 13 x 9 window never takes the row-packed
    kernels, so the reported aggregation follows from the bound alone."""
    from fsgm_amd.sgm2d import last_kernel as last2d
    W, H, rX, rY, n = 23, 11, 6, 4, 2
    low, hi = _sgm2d_inputs(W, H, rX, rY, n, 3, 24), _sgm2d_inputs(W, H, rX, rY, n, 3, 255)
    # (volumes, hints, P1, P2, bound, diagonal, totalPass, adaptive, subpixel)
    calls = [(low, True, 6, 32, 24, 1, 2, 1, 1), (low, True, 6, 32, 24, 1, 1, 1, 1), (low, True, 6, 32, 24, 1, 2, 1, 1),
             (low, True, 6, 32, 24, 0, 2, 1, 1), (low, True, 6, 32, 24, 0, 2, 0, 1), (low, True, 6, 32, 24, 0, 2, 0, 0),
             (low, False, 6, 32, 24, 0, 2, 0, 0), (low, False, 6, 32, 24, 1, 2, 0, 1), (low, True, 6, 32, 24, 1, 2, 0, 1),
             (hi, True, 6, 32, 255, 1, 2, 0, 1), (low, False, 6, 32, 24, 1, 2, 1, 1), (hi, False, 100, 200, 100, 1, 2, 0, 1),
             (low, True, 6, 32, 24, 1, 2, 1, 1)]
    seen = set()
    for i, (inp, with_hints, P1, P2, bound, diag, passes, adaptive, sub) in enumerate(calls):
        vols, hints, guide = inp
        hints = hints if with_hints else None
        want = _sgm2d_want(oracle, vols, hints, guide, rX, rY, P1, P2, bound, diag, passes, adaptive, sub)
        seen.add(want[0].tobytes() + want[2].tobytes() + want[3].tobytes())
        for form in (("host", "device") if i % 2 else ("device", "host")):
            if form == "host" and int(vols.max()) > bound:
                continue                                         # (the host form refuses a volume above its bound)
            got, st = _sgm2d_call(form, side, vols, hints, guide, rX, rY, P1, P2, cost_bound=bound, diagonal=diag, total_pass=passes,
                                  adaptive_p2=adaptive, subpixel=sub)
            what = f"call {i} {form} {calls[i][1:]} after {calls[i - 1][1:] if i else None}"
            cm = min(int(vols.max()), bound) if form == "host" else bound
            assert last2d() == ("generic/wrap" if cm + P2 + max(P1, P2) > 255 else "generic"), what
            assert st == (1 if int(vols.max()) > bound else 0), what
            for g, w, name in zip(got, want, ("bestD", "minC", "mvSub", "flow", "S")):
                _same(g, w, f"{what}: {name}")
            if not sub:
                assert not got[2].any(), f"{what}: mvSub without the refinement"
    assert len(seen) == 11, "every change must matter"           # (calls 0, 2 and 12 are one configuration)


# ---------------------------------------------------------------------------- eviction and return, the other caches
def _queue_then_compare(side, keys, queue, compare):
    """Device form: every key's call queued on one side stream without a wait -- from the cap + 1st on each evicts the oldest
    plan, whose work may not have run -- then the first key again; one wait, then every answer is compared."""
    outs = []
    with torch.cuda.stream(side):
        for k in list(keys) + [keys[0]]:
            outs.append(queue(k))
    side.synchronize()
    for k, o in zip(list(keys) + [keys[0]], outs):
        compare(k, o)


def _dt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, non_blocking=True)


def test_eviction_and_return_sgm2d(gpu_lib, oracle, side):
    """g_sgm2d: 6 + 1 keys, then the first again; host form, then the device form with the evicted plans' work still queued"""
    keys = list(range(20, 27))
    inputs = {W: _sgm2d_inputs(W, 7, 1, 2, 2, W, 24) for W in keys}
    want = {W: _sgm2d_want(oracle, *inputs[W], 1, 2, 6, 32, 24, 1, 2, 0, 1) for W in keys}

    def compare(W, got):
        for g, w, name in zip(got, want[W], ("bestD", "minC", "mvSub", "flow", "S")):
            _same(g.cpu().numpy() if isinstance(g, torch.Tensor) else g, w, f"width {W}: {name}")

    for W in keys + keys[:1]:
        compare(W, _sgm2d_call("host", side, *inputs[W], 1, 2, 6, 32, cost_bound=24)[0])
    _queue_then_compare(side, keys, lambda W: torch_ops.sgm2d(
        _dt(inputs[W][0].transpose(0, 3, 1, 2)), 1, 2, 6, 32, layout="dhw", hints=_dt(inputs[W][1]), guide=_dt(inputs[W][2]),
        cost_bound=24, return_flow=True, return_sum=True), compare)


def test_eviction_and_return_post_flow_and_stereo_pp(gpu_lib, oracle, side):
    """g_post, g_flow and g_spp (cap 4 each): five shapes, then the first again, in host and in device form"""
    from tests import flow_pp_inputs, flow_pp_restatement as FR, stereo_pp_restatement as SP
    shapes = [(W, 7) for W in range(11, 16)]
    # the map chain (test.m:45-50) against the oracle
    maps = {}
    for W, H in shapes:
        D1 = np.stack([synth.vz_index_map(W, H, 64, seed=W + f, invalid=0.1) for f in range(2)])
        g = [synth.epi_maps(W, H, ("general", "radial")[f], seed=W + 10 + f) for f in range(2)]
        maps[W, H] = (D1, np.stack([x[0] for x in g]), np.stack([x[1] for x in g]), np.stack([x[2] / 8 for x in g]))
    want = {k: [oracle.postprocess(m[0][f], m[1][f], m[2][f], m[3][f], 0.3, 65, 64) for f in range(2)] for k, m in maps.items()}

    def compare_post(k, got):
        for f in range(2):
            for g, w, name in zip(got, want[k][f], ("filterD1", "filterD2", "disp")):
                _same(np.asarray(g.cpu() if isinstance(g, torch.Tensor) else g)[f], w, f"post {k} frame {f}: {name}")

    for k in shapes + shapes[:1]:
        compare_post(k, fsgm_amd.epi_postprocess_batch(*maps[k], 0.3, 65, 64))
    _queue_then_compare(side, shapes, lambda k: torch_ops.epi_postprocess(*[_dt(a) for a in maps[k]], 0.3, 65, 64), compare_post)
    # the flow stages against their restatement
    flows = {(W, H): [np.stack([flow_pp_inputs.flow_pair(W, H, ("general", "int")[f], seed=W + f)[j] for f in range(2)]) for j in range(2)]
             for W, H in shapes}
    fwant = {k: np.stack([FR.flow_fb_check(fb[0][f], fb[1][f], 2.0)[0] for f in range(2)]) for k, fb in flows.items()}
    for k in shapes + shapes[:1]:
        _same(fsgm_amd.flow_fb_check(flows[k][0], flows[k][1], 2.0), fwant[k], f"flow {k}, host")
    _queue_then_compare(side, shapes, lambda k: torch_ops.flow_fb_check(_dt(flows[k][0]), _dt(flows[k][1]), 2.0),
                        lambda k, g: _same(g.cpu().numpy(), fwant[k], f"flow {k}, device"))
    # the rectified check against its restatement
    smaps = {(W, H): np.stack([SP.stage_maps(W, H, 24, seed=5 + f)["random"] for f in range(2)]) for W, H in shapes}
    swant = {k: np.stack([SP.stereo_fb_check(w, SP.stereo_disp_from_first(w, -3, 1), -3, 1, 1.0) for w in m]) for k, m in smaps.items()}
    for k in shapes + shapes[:1]:
        _same(fsgm_amd.stereo_fb_check(smaps[k], None, -3, 1, 1.0), swant[k], f"stereo_pp {k}, host")
    _queue_then_compare(side, shapes, lambda k: torch_ops.stereo_fb_check(_dt(smaps[k]), None, -3, 1, 1.0),
                        lambda k, g: _same(g.cpu().numpy(), swant[k], f"stereo_pp {k}, device"))


def test_eviction_and_return_pyramids(gpu_lib, oracle, side):
    """both pyramid caches (cap 2): three shapes, then the first again, in host and in device form"""
    from tests.edge_inputs import oracle_pyramidal_ng
    shapes = [(41, 29), (37, 23), (33, 27)]
    pairs = {k: synth.image_pair(k[0], k[1], 8, seed=k[0]) for k in shapes}
    want = {k: oracle.pyramidal_sgm(*pairs[k], 2)[:2] for k in shapes}
    want_ng = {}
    for k in shapes:
        flows, mc = oracle_pyramidal_ng(oracle, *pairs[k], 2, 1, 2, 0, 6, 32)
        want_ng[k] = (flows[-1], mc)

    def compare(table, what):
        def cmp(k, got):
            _same(np.asarray(got[0].cpu() if isinstance(got[0], torch.Tensor) else got[0]), table[k][0], f"{what} {k}: flow")
            _same(np.asarray(got[1].cpu() if isinstance(got[1], torch.Tensor) else got[1]), table[k][1], f"{what} {k}: minC")
        return cmp

    for k in shapes + shapes[:1]:
        mv, _, mc = fsgm_amd.pyramidal_sgm(*pairs[k], 2)
        compare(want, "pyd host")(k, (mv, mc))
        fl, _, mc = fsgm_amd.pyramidal_sgm_ng(*pairs[k], 2)
        compare(want_ng, "ng host")(k, (fl, mc))
    _queue_then_compare(side, shapes, lambda k: torch_ops.pyramidal_sgm(_dt(pairs[k][0]), _dt(pairs[k][1]), 2), compare(want, "pyd device"))
    _queue_then_compare(side, shapes, lambda k: torch_ops.pyramidal_sgm_ng(_dt(pairs[k][0]), _dt(pairs[k][1]), 2), compare(want_ng, "ng device"))


# --------------------------------------------------------------------------------------- seeded sequences, the other caches
@pytest.mark.parametrize("seed", CS.OTHER_SEEDS)
@pytest.mark.parametrize("group", CS.GROUPS)
def test_other_sequence(gpu_lib, oracle, side, group, seed):
    """pyd + sgm2d, the neighbour-guided level, the two pyramids, post + flow_pp + stereo_pp: Python wrappers, MEX gateways and
    torch ops on a side stream in one drawn order, every output against the oracle or a restatement, the reported sgm2d
    aggregation and ng matcher against a fresh call's"""
    from fsgm_amd.sgm2d import last_kernel as last2d
    steps = CS.other_sequence(group, seed)
    walk = CS.other_walk(steps)
    told = []
    for i, (s, w) in enumerate(zip(steps, walk)):
        prev = w["prev"]
        state = "built again after an eviction" if w["returned"] else "cold" if not w["hit"] else f"warm, last used by step {prev}: {steps[prev]} [{told[prev]}]"
        got, want = CS.other_run(s, stream=side), CS.other_expected(s)
        told.append(last2d() if s.cache == "sgm2d" else fsgm_amd.ng.last_decision()[0] if s.cache == "ng" else "")
        what = f"{group} seed {seed} step {i} ({state}): {s} [{told[-1]}]"
        if s.cache == "sgm2d":
            assert told[-1] == CS.sgm2d_kernel(s), f"{what}: a fresh plan runs {CS.sgm2d_kernel(s)}"
        if s.cache == "ng":
            W, H, half, *_, frames, _ = s.nk
            _ng_fresh_choice(CS._ng_frames(s)[1], W, H, 9 * (2 * half + 1) ** 2, frames)
        assert len(got) == len(want), what
        for k, (g, x) in enumerate(zip(got, want)):
            _same(g, x, f"{what}: output {k}")
        if s.cache == "pyd" and s.nk[0] == 0 or s.cache == "sgm2d" and s.nk[4] == 0:
            assert not np.asarray(got[2]).any(), f"{what}: mvSub without the refinement"
