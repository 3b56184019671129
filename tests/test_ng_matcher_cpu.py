"""Which aggregation kernel a level of the neighbour-guided matcher takes (fsgm_ng_auto_matcher: the host's matcher set followed by
the rule the device applies, ng_choose), fed with list statistics directly: no device is needed.  The sample's pixel count comes
from the library (ng.sample_pixels), so the formula lives in one place."""
import pytest

from fsgm_amd import ng

W, H, D = 83, 58, 81
COMPACT = ("compact16", "compact32", "compact64")
MEANS = (1, 9, 13, 14, 20, 28, 39, 40, 64, 81)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("SPLIT", "DEDUPE", "GRID", "COMPACT", "COMPACT_G", "COST_HINT", "K4"):
        monkeypatch.delenv("FSGM_NG_" + name, raising=False)


def pick(frames, mean, flags=0, below=False, w=W, h=H, d=D):
    """the matcher for lists of `mean` entries per sampled pixel (below: one entry short of that in the whole sample)"""
    n = ng.sample_pixels(w * h * frames)
    return ng.auto_matcher(w, h, d, frames, mean * n - (1 if below else 0), n, flags)


def test_sample_is_every_sixteenth_workgroup_of_four_pixels():
    assert [ng.sample_pixels(n) for n in (1, 4, 64, 65, 83 * 58)] == [4, 4, 4, 8, 304]


def test_thresholds_of_a_batch():
    assert (pick(3, 14, below=True), pick(3, 14)) == ("compact16", "compact32")
    assert (pick(3, 28, below=True), pick(3, 28)) == ("compact32", "compact64")
    assert (pick(3, 40, below=True), pick(3, 40)) == ("compact64", "grid")
    for flags in (1, 2, 3):                                   # a list beyond 64 entries / a key out of range: never compact
        assert (pick(3, 16, flags, below=True), pick(3, 16, flags)) == ("list", "grid")
        assert all(pick(3, m, flags) not in COMPACT for m in MEANS)
    assert pick(3, 9, 4 | 8) == "compact16"                   # the other bits of the flags word are not the rule's


@pytest.mark.parametrize("frames", (1, 2))
def test_one_or_two_frames_take_one_line_a_wave(frames):
    for mean in MEANS:
        assert pick(frames, mean) == ("compact64" if mean < 40 else "split2"), mean
        assert pick(frames, mean, 1) == pick(frames, mean, 2) == "split2", mean
    assert (pick(frames, 40, below=True), pick(frames, 40)) == ("compact64", "split2")


def test_switch_compact_off(monkeypatch):
    monkeypatch.setenv("FSGM_NG_COMPACT", "0")
    assert [pick(3, m) for m in (5, 15, 16, 50)] == ["list", "list", "grid", "grid"]
    assert [pick(1, m) for m in (5, 50)] == ["split2", "split2"]


@pytest.mark.parametrize("g", (16, 32, 64))
def test_switch_compact_class(monkeypatch, g):
    monkeypatch.setenv("FSGM_NG_COMPACT_G", str(g))
    for frames in (1, 3):
        assert all(pick(frames, m) == f"compact{g}" for m in MEANS if m < 40)
        assert pick(frames, 40) == ("grid" if frames == 3 else "split2")
        for flags in (1, 2):                                  # lists the class cannot hold
            assert pick(frames, 30, flags) == ("grid" if frames == 3 else "split2")
            assert pick(frames, 9, flags) == ("list" if frames == 3 else "split2")


def test_switch_grid(monkeypatch):
    monkeypatch.setenv("FSGM_NG_GRID", "0")
    assert [pick(3, m) for m in (9, 20, 30, 50)] == ["compact16", "compact32", "compact64", "lines"]
    assert [pick(3, m, 1) for m in (9, 50)] == ["lines", "lines"]
    monkeypatch.setenv("FSGM_NG_GRID", "1")
    for frames in (1, 3):
        for flags in (0, 1, 2):
            assert all(pick(frames, m, flags) == "grid" for m in MEANS)


def test_switch_split(monkeypatch):
    """One frame, lists too long for the compact kernel.  Without a split the grid kernel joins the set (as for a batch), so the
    lines kernel is reached as "list" below a mean of 16 and as "lines" only with the grid kernel switched off."""
    for parts, name in (("0", "lines"), ("1", "lines"), ("2", "split2"), ("3", "split3"), ("4", "split4"), ("5", "lines")):
        monkeypatch.setenv("FSGM_NG_SPLIT", parts)
        monkeypatch.setenv("FSGM_NG_GRID", "0")
        assert pick(1, 50) == pick(2, 50) == pick(1, 9, 1) == name
        assert pick(1, 9) == "compact64"
        assert pick(3, 50) == "lines"                         # a batch is never split
        monkeypatch.delenv("FSGM_NG_GRID")
        assert pick(1, 50) == (name if name != "lines" else "grid")
        assert pick(1, 9, 1) == (name if name != "lines" else "list")


def test_switch_dedupe_off(monkeypatch):
    monkeypatch.setenv("FSGM_NG_DEDUPE", "0")
    for flags in (0, 1):
        assert all(pick(3, m, flags) == "lines" for m in MEANS)
        assert all(pick(1, m, flags) == "split2" for m in MEANS)
    monkeypatch.setenv("FSGM_NG_GRID", "1")                   # no statistics, no boxes: no grid kernel either
    assert pick(3, 20) == "lines"


def test_wide_search_window_is_generic(monkeypatch):
    for frames in (1, 3):
        assert all(pick(frames, m, d=225) == "generic" for m in MEANS)
    monkeypatch.setenv("FSGM_NG_GRID", "1")
    assert pick(3, 20, d=225) == "generic"
    assert ng.auto_matcher(0, H, D, 1, 0, 0) == ""


@pytest.mark.parametrize("frames", (1, 3, 8))
def test_no_compact_kernel_beyond_32_bit_offsets(monkeypatch, frames):
    """The compact kernels walk a frame with 32-bit byte offsets: W*H*D < 2^30 entries and W*H < 2^23 pixels.  2896 x 2896 is the
    largest square below 2^23 pixels (8 386 816; 2897^2 = 8 392 609), so the pixel gate is pinned from both sides there and at
    4096 x 2048 = 2^23.  With D <= 128 the pixel gate is the tighter one; a frame with W*H*D >= 2^30 below it has D = 225."""
    for g in (None, "16", "64"):
        if g:
            monkeypatch.setenv("FSGM_NG_COMPACT_G", g)
        for mean in MEANS:
            assert pick(frames, mean, w=4096, h=2048) not in COMPACT, (g, mean)
            assert pick(frames, mean, w=2897, h=2897) not in COMPACT, (g, mean)
            assert pick(frames, mean, w=4096, h=2047, d=225) == "generic", (g, mean)
    monkeypatch.delenv("FSGM_NG_COMPACT_G")
    assert pick(frames, 9, w=4096, h=2048) == ("list" if frames > 2 else "split2")
    assert pick(frames, 9, w=4096, h=2047) == pick(frames, 9, w=2896, h=2896) == ("compact16" if frames > 2 else "compact64")


# ---- 9 candidates (halfSearchWinSize 0): no list is longer than 9 entries, so a mean beyond 9 cannot occur; the rule is asked anyway
MEANS9 = (1, 5, 9)


def test_nine_candidates_never_name_the_grid_kernel(monkeypatch):
    """Below 16 candidates (the mean list length from which the rule names it) the grid kernel is no member of the set: with 28
    lines a workgroup it would ask for 280 672 bytes of LDS.  FSGM_NG_GRID=1 there leaves the set as it is without the switch."""
    for grid in (None, "1", "0"):
        if grid:
            monkeypatch.setenv("FSGM_NG_GRID", grid)
        for m in MEANS9 + (16, 50):                           # (means no level of 9 candidates can have: still no grid kernel)
            for flags in (0, 1, 2):
                for frames in (1, 2, 3, 8):
                    assert pick(frames, m, flags, d=9) not in ("grid", "list"), (grid, m, flags, frames)
        for m in MEANS9:
            assert pick(1, m, d=9) == pick(2, m, d=9) == "compact64"
            assert pick(3, m, d=9) == pick(8, m, d=9) == "compact16"
            assert pick(1, m, 2, d=9) == "split2" and pick(3, m, 2, d=9) == "lines"
    monkeypatch.setenv("FSGM_NG_GRID", "1")
    assert pick(3, 20, d=15) == "compact32" and pick(3, 20, d=16) == "grid"    # the gate is D < 16


def test_nine_candidates_switches(monkeypatch):
    for g in (16, 32, 64):
        monkeypatch.setenv("FSGM_NG_COMPACT_G", str(g))
        assert all(pick(frames, m, d=9) == f"compact{g}" for frames in (1, 3) for m in MEANS9)
    monkeypatch.delenv("FSGM_NG_COMPACT_G")
    monkeypatch.setenv("FSGM_NG_COMPACT", "0")
    for m in MEANS9:
        assert pick(3, m, d=9) == "lines" and pick(1, m, d=9) == pick(2, m, d=9) == "split2"
    for grid in ("0", "1"):
        monkeypatch.setenv("FSGM_NG_GRID", grid)
        assert pick(3, 9, d=9) == "lines" and pick(1, 9, d=9) == "split2"
    monkeypatch.delenv("FSGM_NG_GRID")
    for parts, name in (("0", "lines"), ("1", "lines"), ("2", "split2"), ("3", "split3"), ("4", "split4"), ("5", "lines")):
        monkeypatch.setenv("FSGM_NG_SPLIT", parts)
        assert pick(1, 9, d=9) == pick(2, 9, d=9) == name
        assert pick(3, 9, d=9) == "lines"
    monkeypatch.delenv("FSGM_NG_SPLIT")
    monkeypatch.delenv("FSGM_NG_COMPACT")
    monkeypatch.setenv("FSGM_NG_DEDUPE", "0")
    assert all(pick(1, m, d=9) == "split2" and pick(3, m, d=9) == "lines" for m in MEANS9)


def test_dynamic_lds_of_every_set_fits_a_workgroup(monkeypatch):
    """The lines, grid and split kernels size their LDS at launch (256 / D lines a workgroup) and none raises its limit: 64 KiB.
    ng_level_enqueue refuses a level whose set asks for more before anything is queued; with the candidate counts the entry points
    accept below 128 (9 and 81) no set does, under any switch.  The grid kernel at D = 9 would: 280 672 bytes, the request that
    failed every batch of three frames before the kernel left the set there; at D = 16, the smallest D it is a member at, 16 lines
    ask for (16 * 8 * 16 + 16 * 6 * 400 + 16 * 8 + 2 * 16) * 4 = 162 432 bytes -- such a level would be refused, not launched."""
    LIMIT = 64 * 1024
    for d in (9, 81):
        for env in ({}, {"COMPACT": "0"}, {"GRID": "0"}, {"GRID": "1"}, {"DEDUPE": "0"}, {"SPLIT": "0"}, {"SPLIT": "3"}, {"SPLIT": "4"}):
            for k, v in env.items():
                monkeypatch.setenv("FSGM_NG_" + k, v)
            for frames in (1, 2, 3, 8):
                assert 0 < ng.auto_matcher_lds(W, H, d, frames) <= LIMIT, (d, env, frames)
            for k in env:
                monkeypatch.delenv("FSGM_NG_" + k)
    assert ng.auto_matcher_lds(W, H, 9, 3) == (28 * 8 * 12 + 28 * 8) * 4                       # the lines kernel alone
    assert ng.auto_matcher_lds(W, H, 81, 3) == (3 * 8 * 84 + 3 * 6 * 400 + 3 * 8 + 2 * 3) * 4   # the grid kernel: 36 984 bytes
    assert ng.auto_matcher_lds(W, H, 81, 1) == (3 * (10 * 84 + 8) + 3 * 84 * 2) * 4             # two-way split
    monkeypatch.setenv("FSGM_NG_SPLIT", "4")
    assert ng.auto_matcher_lds(W, H, 9, 1) == (28 * (10 * 12 + 8) + 3 * 28 * 12 * 2) * 4
    monkeypatch.delenv("FSGM_NG_SPLIT")
    assert ng.auto_matcher_lds(W, H, 16, 3) == 162432 > LIMIT
    assert ng.auto_matcher_lds(W, H, 225, 3) == ng.auto_matcher_lds(W, H, 441, 1) == 0         # ng_agg_kernel: static LDS only


def test_729_candidates_are_refused_without_a_device():
    """halfSearchWinSize 4 is beyond FSGM_NG_MAX_D (512): the single call, the batch call and the plan answer FSGM_ERR_UNSUPPORTED
    from their argument checks, before a device is looked for (this test runs without one)."""
    import numpy as np
    import fsgm_amd
    from fsgm_amd._lib import FsgmError
    I = np.zeros((15, 21), np.uint8)
    mv = np.zeros((2, 15, 21))
    for call in (lambda: fsgm_amd.calc_pyd_cost_sgm_ng(I, I, mv, 4, 2, 0, 6, 32),
                 lambda: fsgm_amd.calc_pyd_cost_sgm_ng_batch([(I, I, mv)] * 3, 4, 2, 0, 6, 32),
                 lambda: fsgm_amd.NgPyramidPlan(21, 15, 1, 2, batch=3, halfSearchWinSize=4)):
        with pytest.raises(FsgmError) as ei:
            call()
        assert ei.value.status == 4 and "729" in str(ei.value)
