"""Every interchangeable form of the hint-map matcher (calc_pyd_cost_sgm_ng, ng_kernels.hip) at 9, 81 and 441 candidates a pixel,
with 4-byte keys and with 12-byte entries, against the CPU oracle -- bit for bit on S (one frame), minC and the flow -- and, since
all forms give the same bits, with the name of the kernel that ran (fsgm_ng_last_decision) asserted after every run.

Frames: tests/ng_helpers.py (image pair of seed 50 + i, hint map of seed 60 + i).  Mean / longest distinct-(vector, cost) list of
the oracle's candidate volumes, three frames (one frame within 0.1 of these), the same for aggSize 0, 2 and 4 -- with whole-number
hints equal vectors sample equal places, so the count of distinct entries is the count of distinct vectors:
  61 x 37, D = 81: 'zero' 9.00 / 9; 'int' amp 1 22.50 / 25; 'int' amp 2 36.15 / 48; 'int' amp 3 48.03 / 67
  17 x 40, D = 81, one frame: 'int' amp 2 36.36 / 48
  D = 9 ('zero' / 'int' amp 2 / 'general' amp 0.8): 61 x 37 1.00, 7.53, 3.09; 29 x 28 1.00, 7.33, 3.12; 28 x 57 1.00, 7.47, 3.04;
  27 x 5 1.00, 6.65, 2.86; 1 x 12 and 12 x 1 1.00, 2.72, 1.75 / 1.53 -- no list of 9 candidates can reach the rule's first
  threshold (14), so at D = 9 every expectation follows from the frame count and the switches alone.
Where an expectation rests on the rule's thresholds the test computes the mean from the oracle's volume and requires it a quarter
of the band inside the band (ng_helpers.inside_band)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth  # noqa: E402  (torch first, then the library)
from fsgm_amd._lib import FsgmError  # noqa: E402
from tests import edge_inputs as E  # noqa: E402
from tests import flow_pp_restatement as R  # noqa: E402
from tests.ng_helpers import decision, inside_band, list_stats, ng_frames, run_and_compare  # noqa: E402

pytestmark = pytest.mark.gpu
FSGM_ERR_UNSUPPORTED = 4
SWITCHES = ("SPLIT", "DEDUPE", "GRID", "COMPACT", "COMPACT_G", "COST_HINT", "K4")
W0, H0 = 61, 37
PENALTIES = ((6, 32), (90, 120))


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv("FSGM_NG_" + name, raising=False)


def _env(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv("FSGM_NG_" + name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("FSGM_NG_" + k, v)


def _run(oracle, W, H, n, kind, amp, expect, *, r=1, sub=0, agg=2, P1=6, P2=32, mv_shape=None, band=None, what=""):
    """n frames through the single call (n = 1: S as well) or the batch call, against the oracle; then the name of the kernel"""
    D = 9 * (2 * r + 1) ** 2
    frames, want = ng_frames(oracle, W, H, n, kind, amp, r=r, sub=sub, agg=agg, P1=P1, P2=P2, mv_shape=mv_shape)
    what = f"{what} {W}x{H} D{D} n{n} {kind} {amp} sub{sub} agg{agg} P{P1},{P2}"
    if band is not None:
        mean, longest = list_stats(want)
        print(f"{what}: mean list length {mean:.2f}, longest {longest}, band {band}")
        assert inside_band(mean, band, D), (what, mean, band)
    run_and_compare(frames, want, r=r, sub=sub, agg=agg, P1=P1, P2=P2, what=what)
    name, s, npx, flags = decision(W, H, D, n)
    assert name == expect, (what, name, s, npx, flags)
    return name, s, npx, flags


# ================================================================================================ A. D = 9
def _nine(n):
    """default switches at D = 9: one line a wave for one or two frames, 16 lanes a line for a batch (lists of at most 9 entries)"""
    return "compact64" if n <= 2 else "compact16"


HINTS9 = (("zero", 1.0), ("int", 2.0), ("general", 0.8))


@pytest.mark.parametrize("n", (1, 2, 3, 4, 8))
@pytest.mark.parametrize("kind,amp", HINTS9, ids=[h[0] for h in HINTS9])
def test_nine_candidates_default_switches(gpu_lib, oracle, kind, amp, n):
    """halfSearchWinSize 0 (12-byte entries, the generic cost kernel, the dedupe kernel's lanes 9 .. 127 without an entry): the
    compact kernels by the rule, both sub-pixel settings, plain and wrapping penalties.  Three frames or more failed before the
    grid kernel left the set at D < 16 (280 672 B of LDS)."""
    for sub in (0, 1):
        for P1, P2 in PENALTIES:
            _run(oracle, W0, H0, n, kind, amp, _nine(n), r=0, sub=sub, P1=P1, P2=P2, band=(None, 40) if n <= 2 else (None, 14))


@pytest.mark.parametrize("mv_shape", ((50, 30), (70, 45)), ids=["smaller", "larger"])
def test_nine_candidates_hint_map_of_another_size(gpu_lib, oracle, mv_shape):
    for n in (1, 3):
        _run(oracle, W0, H0, n, "general", 0.8, _nine(n), r=0, sub=1, mv_shape=mv_shape)


# lines a workgroup at D = 9: 28 for the lines and split kernels (256 / D; 252 of 256 threads hold a candidate), 16 / 8 / 4 for
# the compact classes.  Line counts of 1, 5, 12, 27, 28, 29 and 57: below, at, one past and twice past 28.
SHAPES9 = ((29, 28), (28, 57), (27, 5), (1, 12), (12, 1))
FORMS9 = [
    ({}, _nine),
    ({"COMPACT_G": "32"}, lambda n: "compact32"),
    ({"COMPACT": "0"}, lambda n: "split2" if n <= 2 else "lines"),
    ({"COMPACT": "0", "SPLIT": "0"}, lambda n: "lines"),
    ({"COMPACT": "0", "SPLIT": "3"}, lambda n: "split3" if n <= 2 else "lines"),
    ({"COMPACT": "0", "SPLIT": "4"}, lambda n: "split4" if n <= 2 else "lines"),
    ({"DEDUPE": "0"}, lambda n: "split2" if n <= 2 else "lines"),
]


@pytest.mark.parametrize("W,H", SHAPES9, ids=[f"{w}x{h}" for w, h in SHAPES9])
def test_nine_candidates_line_counts_around_28(gpu_lib, oracle, monkeypatch, W, H):
    for env, expect in FORMS9:
        _env(monkeypatch, env)
        for n in (1, 3):
            for kind, amp in (("int", 2.0), ("general", 0.8)):
                _run(oracle, W, H, n, kind, amp, expect(n), r=0, sub=1, what=str(env))


SWITCHES9 = ([
    ({"COMPACT_G": "16"}, {1: "compact16", 3: "compact16"}),
    ({"COMPACT_G": "32"}, {1: "compact32", 3: "compact32"}),
    ({"COMPACT_G": "64"}, {1: "compact64", 3: "compact64"}),
    ({"COMPACT": "0"}, {3: "lines"}),                         # no grid kernel at D < 16: the lines kernel is the set's only member
    ({"COMPACT": "0", "GRID": "0"}, {3: "lines"}),
    ({"COMPACT": "0", "SPLIT": "0"}, {1: "lines", 2: "lines"}),
    ({"COMPACT": "0", "SPLIT": "2"}, {1: "split2", 2: "split2"}),
    ({"COMPACT": "0", "SPLIT": "3"}, {1: "split3", 2: "split3"}),
    ({"COMPACT": "0", "SPLIT": "4"}, {1: "split4", 2: "split4"}),
    ({"GRID": "1"}, {1: "compact64", 3: "compact16"}),        # FSGM_NG_GRID=1 at D < 16 leaves the set as without it
    ({"GRID": "1", "COMPACT": "0"}, {1: "split2", 3: "lines"}),
    ({"DEDUPE": "0"}, {1: "split2", 3: "lines"}),
])
SWITCHES9_IDS = [",".join(f"{k}={v}" for k, v in c[0].items()) for c in SWITCHES9]


@pytest.mark.parametrize("env,expect", SWITCHES9, ids=SWITCHES9_IDS)
def test_nine_candidates_every_switch(gpu_lib, oracle, monkeypatch, env, expect):
    _env(monkeypatch, env)
    for n, name in expect.items():
        for kind, amp in HINTS9:
            _run(oracle, W0, H0, n, kind, amp, name, r=0, sub=1, what=str(env))
            _run(oracle, W0, H0, n, kind, amp, name, r=0, sub=0, P1=90, P2=120, what=str(env))


def test_nine_and_81_candidates_back_to_back(gpu_lib, oracle):
    """One process, D = 9, D = 81 and D = 9 again on the cached buffers (the arena is carved anew by every call), each twice:
    results and decisions repeat."""
    seen = []
    for r, expect in ((0, "compact16"), (0, "compact16"), (1, "compact32"), (1, "compact32"), (0, "compact16"), (0, "compact16")):
        seen.append(_run(oracle, W0, H0, 3, "int", 2.0 if r == 0 else 1.0, expect, r=r, sub=1))
    assert seen[0] == seen[1] == seen[4] == seen[5] and seen[2] == seen[3]
    seen = []
    for r, expect in ((0, "compact64"), (0, "compact64"), (1, "split2"), (1, "split2"), (0, "compact64"), (0, "compact64")):
        seen.append(_run(oracle, W0, H0, 1, "int", 2.0 if r == 0 else 3.0, expect, r=r))
    assert seen[0] == seen[1] == seen[4] == seen[5] and seen[2] == seen[3]


# ================================================================================================ B. D = 81, 12-byte entries
# four ways to 12-byte entries while every key would have fit (ng_level_enqueue: keys only with r = 1, rAgg = 1 and the three
# switches on): (aggSize, environment)
ENTRY12 = {"agg4": (4, {}), "agg0": (0, {}), "K4=0": (2, {"K4": "0"}), "COST_HINT=0": (2, {"COST_HINT": "0"})}
# (environment, hints, amplitude, frames, expected kernel, band of the mean the expectation rests on, a list beyond 64 entries)
CELLS81 = [
    ({}, "zero", 1.0, 3, "compact16", (None, 14), False),
    ({}, "int", 1.0, 3, "compact32", (14, 28), False),
    ({}, "zero", 1.0, 1, "compact64", (None, 40), False),
    ({}, "int", 1.0, 1, "compact64", (None, 40), False),
    ({"COMPACT_G": "16"}, "zero", 1.0, 1, "compact16", (None, 40), False),
    ({"COMPACT_G": "16"}, "int", 1.0, 3, "compact16", (None, 40), False),       # lists of up to 25 entries on 16 lanes: two rounds
    ({"COMPACT_G": "32"}, "int", 1.0, 1, "compact32", (None, 40), False),
    ({"COMPACT_G": "32"}, "zero", 1.0, 3, "compact32", (None, 40), False),
    ({"COMPACT_G": "64"}, "zero", 1.0, 3, "compact64", (None, 40), False),
    ({"COMPACT_G": "64"}, "int", 1.0, 3, "compact64", (None, 40), False),
    ({}, "int", 3.0, 3, "grid", (16, None), True),                              # the dedupe kernel makes the boxes itself
    ({"COMPACT": "0"}, "zero", 1.0, 3, "list", (None, 16), False),
    ({"COMPACT": "0", "GRID": "0"}, "zero", 1.0, 3, "lines", None, False),
    ({"COMPACT": "0", "GRID": "0"}, "int", 3.0, 3, "lines", None, True),
    ({}, "int", 3.0, 1, "split2", None, True),
]


@pytest.mark.parametrize("cell", range(len(CELLS81)), ids=[f"{c[4]}-{c[1]}{c[2]:g}-n{c[3]}" + "".join(f"-{k}{v}" for k, v in c[0].items()) for c in CELLS81])
@pytest.mark.parametrize("mode", list(ENTRY12))
def test_81_candidates_twelve_byte_entries(gpu_lib, oracle, monkeypatch, mode, cell):
    """Every form at D = 81 reading the 12-byte list although all keys fit (flag bit 1 clear): the compact kernels and the WTA on
    a.C instead of the keys, the dedupe kernel building its own keys and boxes, S zeroed by the level instead of behind the keys."""
    agg, env12 = ENTRY12[mode]
    env, kind, amp, n, expect, band, over64 = CELLS81[cell]
    _env(monkeypatch, {**env12, **env})
    frames, want = ng_frames(oracle, W0, H0, n, kind, amp, sub=1, agg=agg)
    assert (list_stats(want)[1] > 64) == over64
    name, s, npx, flags = _run(oracle, W0, H0, n, kind, amp, expect, sub=1, agg=agg, band=band, what=mode)
    assert flags & 2 == 0, (mode, flags)
    if npx:                                                   # (a set of one member reports no statistics)
        assert bool(flags & 1) == over64


@pytest.mark.parametrize("W,H", ((61, 37), (17, 40)))
@pytest.mark.parametrize("parts", ("3", "4"))
def test_81_candidates_three_and_four_way_split(gpu_lib, oracle, monkeypatch, parts, W, H):
    """FSGM_NG_SPLIT 3 and 4 (one and two frames; lists of up to 48 entries cut 3 and 4 ways) with 4-byte keys and with 12-byte
    entries, the compact kernels out of the set."""
    for mode, (agg, env12) in (("keys", (2, {})), ("K4=0", ENTRY12["K4=0"]), ("agg4", ENTRY12["agg4"])):
        _env(monkeypatch, {**env12, "COMPACT": "0", "SPLIT": parts})
        for n in (1, 2):
            for sub in (0, 1):
                flags = _run(oracle, W, H, n, "int", 2.0, "split" + parts, sub=sub, agg=agg, what=mode)[3]
                assert flags & 2 == 0


# ================================================================================================ C. D = 441
@pytest.mark.parametrize("sub", (0, 1))
@pytest.mark.parametrize("P1,P2", PENALTIES)
def test_441_candidates_are_generic(gpu_lib, oracle, P1, P2, sub):
    """halfSearchWinSize 3: ng_agg_kernel, 441 candidates on the 64 lanes of a wave (seven rounds, the last with 57 lanes), the
    WTA over all 441."""
    for W, H in ((21, 15), (1, 12), (12, 1)):
        for n in (1, 3):
            assert _run(oracle, W, H, n, "int", 2.0, "generic", r=3, sub=sub, P1=P1, P2=P2) == ("generic", 0, 0, 0)


def test_729_candidates_are_refused_by_every_entry_point(gpu_lib):
    """halfSearchWinSize 4 = 729 candidates, beyond FSGM_NG_MAX_D: FSGM_ERR_UNSUPPORTED from the argument checks."""
    W, H = 21, 15
    I1, I2 = synth.image_pair(W, H, 16, seed=50)
    mv = synth.hint_map(W, H, "zero")
    calls = {
        "single": lambda: fsgm_amd.calc_pyd_cost_sgm_ng(I1, I2, mv, 4, 2, 0, 6, 32),
        "batch": lambda: fsgm_amd.calc_pyd_cost_sgm_ng_batch([(I1, I2, mv)] * 3, 4, 2, 0, 6, 32),
        "plan": lambda: fsgm_amd.NgPyramidPlan(W, H, 1, 2, batch=3, halfSearchWinSize=4),
        "torch": lambda: torch_ops.pyramidal_sgm_ng(torch.from_numpy(I1).to("cuda:0"), torch.from_numpy(I2).to("cuda:0"), 2,
                                                    check=True, halfSearchWinSize=4),
    }
    for who, call in calls.items():
        with pytest.raises(FsgmError) as ei:
            call()
        assert ei.value.status == FSGM_ERR_UNSUPPORTED, who


# ================================================================================================ D. the drivers, D = 9, 3+ frames
# (NgPyramidPlan with batches of 3 and 4: test_gpu_edge_sweeps.py::test_ng_batch_half0.  The drivers keep no decision to ask for;
# by the single-level tests above a level of three or more frames of 9 candidates runs compact16.)
def test_torch_op_nine_candidates_batch_of_three(gpu_lib, oracle):
    W, H, numPyd = 29, 28, 2
    r = E.rng(77)
    pairs = [E.image_pair(r, W, H, 1, seed=70 + f) for f in range(3)]
    I0, I1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    for sub in (0, 1):
        fl, mc = torch_ops.pyramidal_sgm_ng(torch.from_numpy(I0).to("cuda:0"), torch.from_numpy(I1).to("cuda:0"), numPyd, batch=True,
                                            check=True, halfSearchWinSize=0, subPixelRefine=sub)
        for f, (a, b) in enumerate(pairs):
            want, want_mc = E.oracle_pyramidal_ng(oracle, a, b, numPyd, 0, 2, sub, 6, 32)
            np.testing.assert_array_equal(fl[f].cpu().numpy(), want[-1], err_msg=f"sub {sub} frame {f} flow")
            np.testing.assert_array_equal(mc[f].cpu().numpy(), want_mc, err_msg=f"sub {sub} frame {f} minC")


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(np.nan_to_num(got), np.nan_to_num(want), err_msg=what)


def test_flow_pp_nine_candidates_two_pairs(gpu_lib, oracle):
    """pyramidal_flow_pp(matcher="ng") runs 2n frames a level (forward and backward): two pairs are four frames of 9 candidates.
    Flows and minC against the oracle's level loop, the chain against the numpy restatement."""
    W, H, numPyd = 40, 30, 2
    r = E.rng(78)
    pairs = [E.image_pair(r, W, H, 1, seed=80 + f) for f in range(2)]
    I0, I1 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    out = fsgm_amd.pyramidal_flow_pp(I0, I1, numPyd, "ng", halfSearchWinSize=0)
    for f, (a, b) in enumerate(pairs):
        fwd, minC = E.oracle_pyramidal_ng(oracle, a, b, numPyd, 0, 2, 0, 6, 32)
        bwd, _ = E.oracle_pyramidal_ng(oracle, b, a, numPyd, 0, 2, 0, 6, 32)
        pp, checked, gf, gb, gm = (o[f] for o in out)
        _same(gf, fwd[-1], f"pair {f} flow_fwd")
        _same(gb, bwd[-1], f"pair {f} flow_bwd")
        np.testing.assert_array_equal(gm, minC, err_msg=f"pair {f} minC")
        want_pp, want_c, _ = R.chain(fwd[-1], bwd[-1])
        _same(checked, want_c, f"pair {f} flow_checked")
        _same(pp, want_pp, f"pair {f} flow_pp")
