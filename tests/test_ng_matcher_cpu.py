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
