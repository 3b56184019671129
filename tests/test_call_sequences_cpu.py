"""The draws of tests/call_sequences.py, checked without a device: a sequence that meets these conditions cannot quietly test
nothing.  The cache's behaviour is computed from the key rules restated in call_sequences.key / cache_walk: the key of g_epi is
(W, H, D, batch, paths, fb_check, vz_to_disp, sampling, direction, adaptive, agg_mode), eviction is first in, first out at 4."""
import numpy as np
import pytest

from fsgm_amd import FsgmError, epi
from tests import call_sequences as CS

INVALID, NO_DEVICE = 1, 2


def _accepted(call):
    """The call got past the argument checks: it succeeds, or fails for want of a device (tests/test_pyd_limits_cpu.py)."""
    from tests.mexharness import MexError
    try:
        call()
    except FsgmError as e:
        assert e.status == NO_DEVICE and "no HIP device" in str(e), e
    except MexError as e:
        assert "no HIP device" in str(e), e


@pytest.fixture(scope="module", params=CS.EPI_SEEDS)
def seq(request):
    steps = CS.epi_sequence(request.param)
    return steps, CS.cache_walk(steps)


def test_the_draws_are_reproducible_and_stay_in_the_pools():
    for seed in CS.EPI_SEEDS:
        a, b = CS.epi_sequence(seed), CS.epi_sequence(seed)
        assert a == b and 28 <= len(a) <= 32
        for s in a:
            assert (s.W, s.H, s.D) in CS.EPI_SHAPES and s.W * s.H * s.D < 40000 and s.batch in (1, 2, 3)
            assert (s.P1, s.P2) in CS.PENALTIES and s.vMax in CS.VMAX and s.d_min in CS.D_MIN
            assert s.vol_cmax in CS.VOL_CMAX and s.cost_bound in CS.COST_BOUND and s.subpixel in (0, 1)
    assert len({tuple(CS.epi_sequence(seed)) for seed in CS.EPI_SEEDS}) == len(CS.EPI_SEEDS)


def test_every_step_passes_the_argument_checks_and_every_refusal_is_refused(seq):
    steps, _ = seq
    for i, s in enumerate(steps):
        if s.refuse is None:
            _accepted(lambda: CS.run(s, host_only=True))
        else:
            with pytest.raises(FsgmError) as e:
                CS.run(s, host_only=True)
            assert e.value.status == INVALID and s.refuse in str(e.value), (i, s)


def test_warm_hits_differ_in_what_the_key_does_not_hold(seq):
    steps, walk = seq
    warm = [i for i, w in enumerate(walk) if w["hit"] and CS.non_key(steps[i]) != CS.non_key(steps[w["prev"]])]
    assert len(warm) >= 3, warm
    # every kind of carried-over state moves on some warm plan of the eight sequences together: see the test below
    cross = [i for i, w in enumerate(walk) if w["hit"] and CS.FAMILY[steps[i].form] != CS.FAMILY[steps[w["prev"]].form]]
    assert len(cross) >= 1, "no hit whose previous user was another family"


def test_an_evicted_key_comes_back(seq):
    steps, walk = seq
    assert any(w["evicted"] is not None for w in walk)
    back = [i for i, w in enumerate(walk) if w["returned"]]
    assert back, "no return to an evicted key"
    assert all(len({CS.key(s) for s in steps[:i + 1] if s.refuse is None}) > CS.EPI_CAP for i in back)


def test_the_pipeline_moves_on_one_live_plan(seq):
    """Auto mode cannot leave the line kernels at these shapes -- its switch to the fused pipelines lies at hundreds of frames
    for volumes below 40k voxels (scaled_batch, capi_epi.hip), asserted here -- so the class changes come from the key with the
    forced mode 2 of sgm(C), and the wrap / no-wrap changes of the line kernels from every key."""
    steps, walk = seq
    for s in steps:
        name = epi.auto_pipeline(s.W, s.H, s.D, s.batch, s.paths, s.P1, s.P2, 24)
        assert CS.pipeline_class(name) == ("generic" if s.D not in CS.LINE_D else "lines"), (s, name)
    changes, by_bound, names = {}, 0, 0
    for i, w in enumerate(walk):
        if not w["hit"]:
            continue
        s, q = steps[i], steps[w["prev"]]
        a, b = CS.pipeline(q), CS.pipeline(s)
        names += a != b
        if CS.pipeline_class(a) != CS.pipeline_class(b):
            changes[CS.key(s)] = changes.get(CS.key(s), 0) + 1
            by_bound += (s.P1, s.P2) == (q.P1, q.P2) and CS.plan_cmax(s) != CS.plan_cmax(q)
    assert changes and max(changes.values()) >= 2, changes
    assert by_bound >= 1, "no change of class caused by the bound of the costs alone"
    assert names >= 3                                            # (the first four calls of a sequence alone make three)


def test_the_sequences_together_move_every_kind_of_state():
    moved = set()
    forms = set()
    for seed in CS.EPI_SEEDS:
        steps = CS.epi_sequence(seed)
        for i, w in enumerate(CS.cache_walk(steps)):
            forms.add(steps[i].form)
            if w["hit"]:
                s, q = steps[i], steps[w["prev"]]
                moved |= {f for f in ("P1", "subpixel", "vMax", "d_min", "vol_cmax", "cost_bound", "guide", "want_S", "want_C", "form")
                          if getattr(s, f) != getattr(q, f)}
    assert moved == {"P1", "subpixel", "vMax", "d_min", "vol_cmax", "cost_bound", "guide", "want_S", "want_C", "form"}, moved
    assert forms == set(CS.FAMILY)


def test_cache_walk_is_first_in_first_out():
    mk = lambda W: CS.Step("sgm", W, 5, 16, 1, 4, 0, 0, 0, -1, 6, 64, 1, 0.3, None, 24, 255, False, False, False, 0, None)  # noqa: E731
    walk = CS.cache_walk([mk(W) for W in (1, 2, 3, 4, 1, 5, 1, 2)])
    assert [w["hit"] for w in walk] == [False, False, False, False, True, False, False, False]
    assert walk[5]["evicted"] == CS.key(mk(1)) and walk[6]["returned"] and walk[6]["evicted"] == CS.key(mk(2))   # the hit on 1 did not save it
    assert walk[4]["prev"] == 0 and walk[6]["prev"] is None


def test_expectations_are_memoised_and_left_unchanged():
    s = CS.epi_sequence(0)[0]
    a, b = CS.expected(s), CS.expected(s._replace(want_S=not s.want_S))
    assert np.array_equal(a["bestD"], b["bestD"]) and not CS.volume(s.W, s.H, s.D, s.vol_cmax, s.seed, 0).flags.writeable


# ---------------------------------------------------------------------------------------------------------- the other caches
OTHER = [(g, seed) for g in CS.GROUPS for seed in CS.OTHER_SEEDS]


@pytest.fixture(scope="module", params=OTHER, ids=lambda p: f"{p[0]}-{p[1]}")
def oseq(request):
    steps = CS.other_sequence(*request.param)
    return request.param[0], steps, CS.other_walk(steps)


def test_other_draws_are_reproducible_and_small():
    for g, seed in OTHER:
        a = CS.other_sequence(g, seed)
        assert a == CS.other_sequence(g, seed) and 14 <= len(a) <= 32
        assert {s.cache for s in a} == set(CS.CACHES[g])
        for s in a:
            assert s.form in CS.FORMS[s.cache] and (s.key in CS.KEYS[s.cache])
    assert len({tuple(CS.other_sequence(g, seed)) for g, seed in OTHER}) == len(OTHER)


def test_every_other_step_passes_the_argument_checks(oseq):
    _, steps, _ = oseq
    for s in steps:
        _accepted(lambda: CS.other_run(s, host_only=True))


def test_other_sequences_hit_warm_plans_in_another_state(oseq):
    """per sequence: three hits whose other parameters or data differ from the plan's previous call, one hit through another
    form (wrapper, gateway, torch op) than the previous user's, and per cache with a cap an eviction and a return"""
    group, steps, walk = oseq
    warm = [i for i, w in enumerate(walk) if w["hit"] and (steps[i].nk, steps[i].seed) != (steps[w["prev"]].nk, steps[w["prev"]].seed)]
    assert len(warm) >= 3, warm
    assert any(w["hit"] and steps[i].form != steps[w["prev"]].form for i, w in enumerate(walk))
    for cache in CS.CACHES[group]:
        if CS.CAPS[cache] is None:
            continue
        assert any(w["evicted"] is not None and steps[i].cache == cache for i, w in enumerate(walk)), cache
        assert any(w["returned"] and steps[i].cache == cache for i, w in enumerate(walk)), cache
        assert len({s.key for s in steps if s.cache == cache}) > CS.CAPS[cache]


def test_other_sequences_together_use_every_form_and_move_every_parameter():
    forms, moved = set(), {}
    for g, seed in OTHER:
        steps = CS.other_sequence(g, seed)
        for i, w in enumerate(CS.other_walk(steps)):
            s = steps[i]
            forms.add((s.cache, s.form))
            if w["hit"] and s.nk:
                q = steps[w["prev"]]
                moved.setdefault(s.cache, set()).update(j for j in range(len(s.nk)) if s.nk[j] != q.nk[j])
    assert forms == {(c, f) for c, fs in CS.FORMS.items() for f in fs}
    for cache, n in (("pyd", 6), ("sgm2d", 7), ("ng", 9), ("post", 2), ("flow", 2), ("spp", 4)):
        assert moved[cache] == set(range(n)), (cache, moved[cache])


def test_the_arena_is_carved_for_other_sizes():
    """the neighbour-guided level's steps: the bytes asked of the arena change at least three times in a sequence, and grow again
    after a smaller call at least once"""
    for seed in CS.OTHER_SEEDS:
        need = [CS.ng_need(s) for s in CS.other_sequence("ng", seed)]
        assert sum(a != b for a, b in zip(need, need[1:])) >= 3, need
        assert any(b < a and c > b for a, b, c in zip(need, need[1:], need[2:])), need


def test_other_walk_keeps_one_cache_per_family():
    mk = lambda c, W: CS.OStep(c, "host", (W, 7, 1), (), 0)  # noqa: E731
    walk = CS.other_walk([mk("pyramid", 1), mk("ng_pyramid", 1), mk("pyramid", 2), mk("pyramid", 3), mk("pyramid", 1), mk("ng_pyramid", 1)])
    assert [w["hit"] for w in walk] == [False, False, False, False, False, True] and walk[4]["returned"] and walk[3]["evicted"] == ("pyramid", (1, 7, 1))
