"""GPU tests of sgm(C) with exact path arithmetic (fsgm_sgm_batch_host_exact through fsgm_amd.sgm_batch(arith="exact"),
EpiPlan.set_exact) against tests/sgm_exact_restatement.py, bit for bit in bestD, minC and S.  tests/test_sgm_exact_cpu.py ties
that yardstick to the pinned oracle inside the no-wrap budget and shows that outside it, on the shapes used here, the mod-256
kernels could not pass these comparisons.

Shapes: (W, H) = (37, 11) takes the along-x lines past one 16-step prefetch round, (9, 21) every other direction past 4 steps,
and the two re-enter the diagonals with W > H and with W < H.  Every dMax class of the packed kernels and two generic ones
(24, 300) meets, on each of the two shapes, all four penalty pairs and all four kinds of volume (one kind per penalty pair,
shifted with dMax; on (37, 11) one more call takes the `top` volume at P1 = P2 = 255, 8 paths); paths, batch and layout rotate over that grid so that
every value of each meets every dMax class at least once.  The edges volume meets both shapes again at every dMax."""
import functools

import numpy as np
import pytest

from fsgm_amd import _lib
from fsgm_amd._lib import FsgmError, STAGE_AGGREGATE, STAGE_WTA
from fsgm_amd.epi import EpiPlan
from fsgm_amd.sgm import last_kernel, sgm_batch
from oracle import pyoracle
from tests import sgm_exact_restatement as X

pytestmark = pytest.mark.gpu
FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4
SHAPES = ((37, 11), (9, 21))
PACKED = {16: 16, 32: 16, 64: 16, 128: 16, 256: 16, 48: 12, 96: 12, 192: 12, 80: 20, 160: 20, 112: 28, 224: 28}   # dMax: costs a lane
GENERIC = (24, 300)
DMAX = (16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 224, 256) + GENERIC
PENALTIES = ((7, 100), (0, 255), (255, 255), (200, 10))
KINDS = ("random", "full", "edges", "top")


def _name(D):
    return "packed16/exact" if D in PACKED else "generic/exact"


def _volume(kind, W, H, D, seed):
    """random: uniform bytes.  full: all 255.  edges: high costs with each pixel's minimum at d = 0, d = D-1 or on either side of
    a lane boundary (the generic kernels: of 16).  top: costs (0, 255, 255, ...) everywhere but at odd (x, y), where all are 255:
    with P1 = P2 = 255 every path reaches such a pixel with L = 510 at d >= 2 -- S = 4080 with 8 paths, the top of the range."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (H, W, D), dtype=np.uint8)
    if kind == "full":
        return np.full((H, W, D), 255, np.uint8)
    if kind == "edges":
        b = PACKED.get(D, 16)
        Cv = rng.integers(120, 256, (H, W, D), dtype=np.uint8)
        where = rng.choice(np.array([d for d in (0, D - 1, b - 1, b) if d < D]), (H, W))      # (D = 16: one lane, no boundary)
        np.put_along_axis(Cv, where[..., None], rng.integers(0, 20, (H, W, 1), dtype=np.uint8), axis=2)
        return Cv
    Cv = np.full((H, W, D), 255, np.uint8)
    Cv[..., 0] = 0
    Cv[1::2, 1::2, 0] = 255
    return Cv


@functools.lru_cache(maxsize=None)
def _case(kind, W, H, D, n, seed, P1, P2, paths, adaptive=False):
    """(volumes, guides or None, the restatement's (bestD, minC, S)): computed once, shared, never written to"""
    vols = np.stack([_volume(kind, W, H, D, seed + 101 * f) for f in range(n)])
    guides = None
    if adaptive:                                                 # steps of 10 and 20 (below the threshold of 25), of 30 and more (above)
        guides = np.random.default_rng(seed + 5).choice(np.array([10, 30, 40, 70, 200], np.uint8), (n, H, W))
    want = X.sgm_batch(vols, P1, P2, paths, guides)
    for a in (vols,) + want + (() if guides is None else (guides,)):
        a.setflags(write=False)
    return vols, guides, want


def _run(vols, P1, P2, paths, layout="hwd", guides=None, arith="exact", **kw):
    Cin = vols if layout == "hwd" else np.ascontiguousarray(vols.transpose(0, 3, 1, 2))
    return sgm_batch(Cin, P1, P2, paths=paths, layout=layout, return_sum=True, arith=arith, guide=guides,
                     adaptive_p2=int(guides is not None), **kw)


def _same(got, want, what):
    for g, w, n in zip(got, want, ("bestD", "minC", "S")):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {n} differs at {len(bad)} places, first {tuple(bad[0])}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"


@pytest.mark.parametrize("W,H", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("D", DMAX)
def test_exact_equals_the_restatement(gpu_lib, D, W, H):
    i = DMAX.index(D) + SHAPES.index((W, H))
    for k, (P1, P2) in enumerate(PENALTIES + (((255, 255),) if W > H else ())):
        r = i + k
        paths, n, layout = (4, 8)[r % 2], (1, 3)[(r // 2) % 2], ("hwd", "dhw")[(r // 4 + r) % 2]
        kind = KINDS[(DMAX.index(D) + k) % 4]                    # both shapes of a dMax see all four kinds, a penalty pair each
        if k == len(PENALTIES):                                  # one more call on (37, 11): the top of the range, S = 4080
            paths, kind = 8, "top"
        vols, _, want = _case(kind, W, H, D, n, 17 * D + W, P1, P2, paths)
        got = _run(vols, P1, P2, paths, layout)
        assert last_kernel() == _name(D)
        _same(got, want, f"D {D} {W}x{H} P ({P1}, {P2}) paths {paths} n {n} {layout} {kind}")
        if kind == "top" and paths == 8 and (P1, P2) == (255, 255):
            assert int(want[2].max()) == 4080 and int(got[2].max()) == 4080


@pytest.mark.parametrize("D", [16, 48, 128, 256, 24, 300])
def test_all_255_at_the_largest_penalties(gpu_lib, D):
    """every cost 255 at P1 = P2 = 255, 8 paths, both layouts of a batch of 3: L = 510 at the second pixel of every path (a path
    start stores the minimum 0), 255 from the third on; S reaches 3315 on these shapes -- S = 4080 is `top`'s, in the test above"""
    for (W, H), layout in zip(SHAPES, ("dhw", "hwd")):
        vols, _, want = _case("full", W, H, D, 3, 1, 255, 255, 8)
        assert int(want[2].max()) == 3315                        # 6 paths at L = 510 and 1 at 255 where a path starts
        _same(_run(vols, 255, 255, 8, layout), want, f"all 255, D {D} {W}x{H} {layout}")


@pytest.mark.parametrize("D", DMAX)
def test_minimum_at_the_edges_of_d_and_of_a_lane(gpu_lib, D):
    """every dMax at the penalty pair whose P1 exceeds P2 and at the largest one: an absent neighbour that turned into a small
    number after the add of P1 would win here"""
    for k, (P1, P2) in enumerate(((200, 10), (255, 255), (7, 100), (200, 10))):
        W, H = SHAPES[(DMAX.index(D) + k) % 2]                   # both shapes, the pair with P1 > P2 on each
        vols, _, want = _case("edges", W, H, D, 1, 3 * D, P1, P2, 8)
        _same(_run(vols, P1, P2, 8), want, f"edges, D {D} {W}x{H} P ({P1}, {P2})")


@pytest.mark.parametrize("D", [16, 32, 80, 128, 192, 224, 256, 24])
@pytest.mark.parametrize("paths", [4, 8])
def test_adaptive_p2(gpu_lib, D, paths):
    W, H = SHAPES[(DMAX.index(D) + paths // 8) % 2]
    n = 1 + 2 * (DMAX.index(D) % 2)
    vols, guides, want = _case("random", W, H, D, n, 9 * D, 7, 100, paths, True)
    _same(_run(vols, 7, 100, paths, "dhw" if n == 3 else "hwd", guides), want, f"adaptive, D {D} {W}x{H} paths {paths} n {n}")
    assert last_kernel() == _name(D)
    plain = _case("random", W, H, D, n, 9 * D, 7, 100, paths)[2]
    assert not np.array_equal(plain[2], want[2]), "the guide never lowered P2: the case tests nothing"


@pytest.mark.parametrize("D,plain_name", [(32, "packed16/nowrap"), (48, "packed16/nowrap"), (24, "generic")])
@pytest.mark.parametrize("paths", [4, 8])
def test_inside_the_budget_exact_equals_plain(gpu_lib, D, plain_name, paths):
    W, H = SHAPES[paths // 8]
    rng = np.random.default_rng(D + paths)
    vols = rng.integers(0, 25, (2, H, W, D), dtype=np.uint8)
    before = _run(vols, 6, 64, paths, arith="mod256")
    assert last_kernel() == plain_name
    exact = _run(vols, 6, 64, paths)
    assert last_kernel() == _name(D)
    after = _run(vols, 6, 64, paths, arith="mod256")
    assert last_kernel() == plain_name
    _same(exact, before, "exact against plain")
    _same(after, before, "plain after exact")
    _same(exact, X.sgm_batch(vols, 6, 64, paths), "exact against the restatement")


@pytest.mark.parametrize("D,plain_name", [(64, "packed16/wrap"), (112, "packed16/wrap"), (300, "generic")])
def test_plain_and_exact_calls_interleaved(gpu_lib, D, plain_name):
    """one shape, the two arithmetics in turn: each keeps its plan, its kernels and its results"""
    W, H = SHAPES[0]
    vols, _, want = _case("random", W, H, D, 3, 77, 7, 100, 8)
    oracle = []
    for Cv in vols:
        S = pyoracle.epi_aggregate(Cv, 7, 100, 8)
        oracle.append(pyoracle.epi_wta(S, W, H, D, 1) + (S[:-1].reshape(H, W, D),))
    oracle = tuple(np.stack([o[k] for o in oracle]) for k in range(3))
    assert not np.array_equal(oracle[0], want[0])
    for turn in range(3):
        _same(_run(vols, 7, 100, 8, arith="mod256"), oracle, f"plain call, turn {turn}")
        assert last_kernel() == plain_name
        _same(_run(vols, 7, 100, 8), want, f"exact call, turn {turn}")
        assert last_kernel() == _name(D)


def _status(fn, *a):
    with pytest.raises(FsgmError) as e:
        fn(*a)
    return e.value.status


def test_plan_switch(gpu_lib):
    W, H, D = 37, 11, 64
    vols, _, want = _case("random", W, H, D, 3, 77, 7, 100, 8)
    with EpiPlan(W, H, D, 3, paths=8, vz_to_disp=0) as plan:
        plan.set_agg_mode(4)
        assert _status(plan.set_exact, 1) == FSGM_ERR_UNSUPPORTED and plan.exact == 0
        plan.set_agg_mode(0)
        plan.set_runner_up(1)
        assert _status(plan.set_exact, 1) == FSGM_ERR_UNSUPPORTED and plan.exact == 0
        plan.set_runner_up(0)
        plan.set_exact(1)
        assert plan.kernel_name == "packed16/exact"
        assert _status(plan.set_runner_up, 1) == FSGM_ERR_UNSUPPORTED
        for mode in range(2, 7):
            assert _status(plan.set_agg_mode, mode) == FSGM_ERR_UNSUPPORTED
        assert _status(plan.set_penalties, 7, 256) == FSGM_ERR_INVALID
        assert _status(plan.set_penalties, -1, 100) == FSGM_ERR_INVALID
        plan.set_penalties(7, 100)
        for f in range(3):
            plan.upload_cost(f, vols[f])
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        assert plan.kernel_name == "packed16/exact"
        for f in range(3):
            _same(plan.download(f) + (plan.download_sum(f),), tuple(w[f] for w in want), f"plan, frame {f}")
        plan.set_exact(0)                                        # off: the plan is what it was
        assert plan.kernel_name == "packed16/wrap"
        plan.run(STAGE_AGGREGATE | STAGE_WTA)
        S = pyoracle.epi_aggregate(vols[1], 7, 100, 8)
        assert np.array_equal(plan.download_sum(1).reshape(-1), S[:-1])
    with EpiPlan(W, H, 24, 1, paths=4, vz_to_disp=0) as plan:
        plan.set_exact(1)
        assert plan.kernel_name == "generic/exact"
