"""Shared by the GPU tests of the neighbour-guided level (test_gpu_ng.py, test_gpu_ng_forms.py) and the CPU tests beside them:
the frames, the oracle's results for them (computed once per frame and parameter set, shared and left unchanged), the comparison
and the check of the matcher's name.  Every form of the aggregation gives the same results, so only fsgm_ng_last_decision can tell
which one a test ran."""
import numpy as np

from fsgm_amd import synth

COMPACT_NAMES = ("compact16", "compact32", "compact64")
_oracle_cache = {}


def kept(Cc):
    """per pixel, the number of distinct (vector, cost) entries in the oracle's candidate volume: the list the matchers stage"""
    k = (Cc["mvx"].astype(np.int64) << 40) ^ ((Cc["mvy"].astype(np.int64) & 0xFFFFFFFF) << 8) ^ Cc["cost"].astype(np.int64)
    k = np.sort(k.reshape(-1, k.shape[-1]), axis=1)
    return 1 + (np.diff(k, axis=1) != 0).sum(axis=1)


def decision(W, H, D, frames):
    """The device and the host apply one rule to the same numbers: the name of the choice word is what auto_matcher answers
    for the statistics the level left behind."""
    from fsgm_amd import ng
    name, s, n, flags = ng.last_decision()
    assert name == ng.auto_matcher(W, H, D, frames, s, n, flags), (name, s, n, flags)
    if n:
        assert n == ng.sample_pixels(W * H * frames)
    return name, s, n, flags


def ng_frame(W, H, i, kind, amp, edit=None, mv_shape=None):
    """frame i of a batch: image pair of seed 50 + i, hint map of seed 60 + i (mv_shape: (mvW, mvH) other than the image's)"""
    I1, I2 = synth.image_pair(W, H, 16, seed=50 + i)
    mvW, mvH = mv_shape or (W, H)
    mv = synth.hint_map(mvW, mvH, kind, seed=60 + i, amp=amp)
    if edit:
        edit(mv)
    return I1, I2, mv


def ng_frames(oracle, W, H, n, kind, amp, r=1, sub=0, edit=None, agg=2, P1=6, P2=32, mv_shape=None):
    """n frames and the oracle's (minC, flow, candidate volume, S) for each; frame i is the same in every batch size, and its
    oracle run is shared by all tests of a process"""
    frames, want = [], []
    for i in range(n):
        key = (W, H, i, kind, amp, r, sub, edit.__name__ if edit else None, agg, P1, P2, mv_shape)
        if key not in _oracle_cache:
            f = ng_frame(W, H, i, kind, amp, edit, mv_shape)
            w = oracle.calc_pyd_cost_sgm_ng(*f, r, agg, sub, P1, P2, want_volumes=True)
            for a in w[:2] + (w[3],):
                a.setflags(write=False)
            _oracle_cache[key] = (f, w)
        f, w = _oracle_cache[key]
        frames.append(f)
        want.append(w)
    return frames, want


def run_and_compare(frames, want, r=1, sub=0, agg=2, P1=6, P2=32, what=""):
    """one frame: S, minC and flow through the single call; more: minC and flow through the batch call"""
    from fsgm_amd import calc_pyd_cost_sgm_ng, calc_pyd_cost_sgm_ng_batch
    if len(frames) == 1:
        gmc, gfl, gS = calc_pyd_cost_sgm_ng(*frames[0], r, agg, sub, P1, P2, return_sum=True)
        np.testing.assert_array_equal(gS, want[0][3], err_msg=f"{what} S")
        got = [(gmc, gfl)]
    else:
        got = calc_pyd_cost_sgm_ng_batch(frames, r, agg, sub, P1, P2)
    for i, ((gmc, gfl), w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(gmc, w[0], err_msg=f"{what} frame {i} minC")
        np.testing.assert_array_equal(gfl, w[1], err_msg=f"{what} frame {i} flow")


def list_stats(want):
    """(mean, longest) distinct-(vector, cost) list of the oracle's candidate volumes of a batch"""
    k = np.concatenate([kept(w[2]) for w in want])
    return float(k.mean()), int(k.max())


def inside_band(mean, band, D=81):
    """The mean list length lies at least a quarter of the band's width inside [lo, hi); an end that is no threshold of the rule
    is None and counts as 1 or D, the shortest and the longest list there is."""
    lo, hi = band
    quarter = ((hi or D) - (lo or 1)) / 4
    return (lo is None or mean >= lo + quarter) and (hi is None or mean <= hi - quarter)
