"""Inputs for the comparisons with the reference's compiled MEX code: the case lists of tests/test_oracle_ref_parity.py (taken
from the GPU suite's own parametrisations, the random-configuration draws and the edge values) and the small fixture cases of
tests/golden/make_ref_mex_golden.py.

A case is (id, build): build() returns the positional arguments of the matching oracle/pyref.py call_* function (for
calc_cost_sgm_ng: I1, I2, P1, P2, seed).  What has no MEX argument to map to (synthetic cost volumes, batch sizes, path counts,
kernel selections) is dropped: the MEX files take images and compute their own costs, one frame a call.
calc_pyd_cost_sgm reads its hint map at the image's own coordinates without a clamp (calc_pyd_cost_sgm.cpp:388-389), so its
hint maps are never smaller than the image; calc_pyd_cost_sgm_ng clamps (:392-393), so there both occur."""
import numpy as np

from fsgm_amd import synth
from tests import budget_volumes
from tests import edge_inputs as E
from tests import fuzz_configs


def marks(fn, first):
    """The value list of fn's parametrize mark whose first argument name is `first`."""
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize" and m.args[0].split(",")[0].strip() == first:
            return list(m.args[1])
    raise LookupError(f"{fn.__name__}: no parametrize mark starting with {first}")


def _dedupe(cases):
    seen, out = set(), []
    for cid, build in cases:
        if cid not in seen:
            seen.add(cid)
            out.append((cid, build))
    return out


class _EveryBranch:
    """A stand-in generator for E.image_pair that takes each of its branches: strong gradients in the first image, the top third
    of the second saturated (a flat area of 255)."""
    def rand(self):
        return 0.0


def _images(W, H, D, iseed, edge):
    return E.image_pair(_EveryBranch(), W, H, 1, seed=iseed) if edge else synth.image_pair(W, H, D, seed=iseed)


# ------------------------------------------------------------------------------------------------ calc_cost_sgm
def _epi(W, H, D, kind, P1, P2, iseed, mseed, vMax=0.3, edit=None):
    def build():
        I1, I2 = synth.image_pair(W, H, D, seed=iseed)
        pd0, nd, off = synth.epi_maps(W, H, kind, seed=mseed)
        if edit:
            edit(pd0, nd, off)
        return I1, I2, D, vMax, pd0, nd, off, P1, P2
    return f"{W}x{H}x{D}-{kind}-P{P1}_{P2}-s{iseed}_{mseed}" + (f"-{edit.__name__}" if edit else ""), build


def out_of_range(pd0, nd, off):
    """test_gpu_epi.py::test_cost_volume_out_of_range_geometry's planted values, placed relative to the frame."""
    H, W = off.shape
    off[3 % H, 4 % W] = 1e12
    off[5 % H, 6 % W] = -1e12
    off[7 % H, 8 % W] = 1e300
    pd0[0, 9 % H, 9 % W] = np.inf
    pd0[1, 10 % H, 10 % W] = np.nan


ROUND_SPECIALS = [0.5, 1.5, 2.5, -0.5, -1.5, 0.49999999999999994, -0.49999999999999994, 1.4999999999999998,
                  2147483647.5, 2147483647.4, 2147483648.0, -2147483648.0, -2147483648.5, -2147483649.0,
                  4294967296.0, 1e300, -1e300, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 38.5, 39.5, 39.49999999999999]


def rounding(pd0, nd, off):
    """test_gpu_epi.py::test_cost_volume_rounding_edge_cases: sample position = Pd0 - 1 exactly, on the hard cases of
    (int)round(v)."""
    H, W = off.shape
    nd[0][:] = 1.0
    nd[1][:] = 0.0
    off[:] = 0.0
    for i, v in enumerate(ROUND_SPECIALS):
        pd0[0, i % H, (3 * i) % W] = v + 1.0 if np.isfinite(v) and abs(v) < 1e15 else v
        pd0[1, (i + 5) % H, (3 * i + 1) % W] = v + 1.0 if np.isfinite(v) and abs(v) < 1e15 else v


KITTI_EPI = _epi(1242, 375, 64, "general", 6, 64, 2, 4)
KITTI_EPI_CPU = _epi(1242, 64, 64, "general", 6, 64, 2, 4)       # the CPU suite's share of it: full width, 64 rows


def epi_cases():
    from tests import test_gpu_epi as T
    c = []
    c += [_epi(W, H, D, kind, 6, 64, W + D, H) for W, H, D, kind in marks(T.test_cost_volume_bit_exact, "W")]
    c += [_epi(48, 32, 16, "general", 6, 64, 5, 9, edit=out_of_range), _epi(40, 24, 16, "axis", 6, 64, 8, 7, edit=rounding)]
    c += [_epi(W, H, D, "general", P1, P2, W * 7 + D, H) for W, H, D, P1, P2, _, _ in T.AGG_CASES]
    c += [_epi(W, H, D, kind, 6, 64, 2, 4) for W, H, D, kind in marks(T.test_calc_cost_sgm_whole_mex, "W")]
    c += [_epi(W, H, D, "general", 6, 64, W + H, H) for W, H, D, _ in marks(T.test_pairs_pipeline_4_paths, "W")]
    c += [_epi(W, H, D, "general", 6, 64, W + H, H) for W, H, D in marks(T.test_sweep_blocks_and_columns, "W")]
    c += [_epi(W, H, D, "general", 6, 64, W + 10 * H, H) for W, H in [(1, 1), (1, 9), (9, 1), (2, 2), (8, 3), (3, 8)] for D in (16, 128)]
    c += [_epi(W, H, D, "general", 6, 64, 11, 3) for W, H, D in marks(T.test_wta_subpixel_bit_exact, "W")]
    c += [_epi(W, H, D, kind, 6, 64, 5, 6) for W, H, D, kind, _ in marks(T.test_forward_backward_check, "W")]
    c += [_epi(96, 64, 64, "general", 6, 64, 1, 2)]                                   # test_batch_matches_single_frames' shape
    c += [_epi(W, H, D, "general", 6, 64, W + H, H) for W, H, D, _ in marks(T.test_parallel_sweeps_match_the_oracle, "W")]
    c += [_epi(W, H, D, "general", 6, 64, W + H, H)
          for W, H, D in marks(T.test_line_kernels_hand_written_steps_at_their_loop_boundaries, "W")]
    c += [_epi(W, H, D, "general", P1, P2, W, H) for W, H, D, P1, P2, _ in marks(T.test_sgm_call_shape, "W")]
    # wrapping penalties up to 255, degenerate shapes, other vMax
    c += [_epi(19, 13, 16, "general", P1, P2, 3, 4) for P1, P2 in ((255, 255), (255, 0), (0, 255), (0, 0), (128, 127))]
    c += [_epi(W, H, 20, "radial", 6, 64, 3, 4, vMax=0.25) for W, H in ((1, 14), (14, 1), (2, 2), (31, 17))]
    # the 4-path penalty sets of tests/test_gpu_fused_budgets.py (P1 + P2 = 127, P1 = 0, P1 = P2, ...): the oracle's 4-path row at
    # them, on the costs the MEX computes from the images itself
    c += [_epi(23, 11, D, "general", P1, P2, 6, 7) for P1, P2 in budget_volumes.PAIR_PENALTIES for D in (16, 128)]
    return _dedupe(c)


def epi_edge_geometry_cases():
    """Every frame of test_gpu_edge_sweeps.py::test_epipolar_random_geometries' ten seeds (tests/edge_inputs.py: E.epi_shape,
    E.epi_geometry through the oracle's epipolar_maps, E.image_pair; RGB pairs through the oracle's rgb2gray, as
    epipolar_sgm_of does), with that test's D and vMax and the penalties of epipolar_sgm_of.m (6, 64): epipoles inside, outside,
    far away and on a pixel (NaN direction, zero offset), H = I, either direction flag, flat and saturated image areas.  The
    maps are inputs here, whatever made them: what is compared is what the MEX file does with them."""
    from oracle import pyoracle
    c = []
    for seed in range(10):
        def frames(seed=seed):
            _, W, H, D, vMax, _, ch, B, geos, pairs = E.epi_random_case(seed, pyoracle)
            out = []
            for g, (I0, I1) in zip(geos, pairs):
                with np.errstate(all="ignore"):
                    pd0, nd, off, _ = pyoracle.epipolar_maps(*g[:4], W, H)
                if ch == 3:
                    I0, I1 = pyoracle.rgb2gray(I0), pyoracle.rgb2gray(I1)
                out.append((np.ascontiguousarray(I0), np.ascontiguousarray(I1), D, vMax, pd0, nd, off, 6, 64))
            return out
        B = len(frames())
        c += [(f"edge_geometry-seed{seed}-frame{f}", (lambda frames=frames, f=f: frames()[f])) for f in range(B)]
    return c


def epi_fuzz_cases():
    c = []
    for seed in range(24):
        g = fuzz_configs.epi_config(seed)
        c.append(_epi(g["W"], g["H"], g["D"], "general", g["P1"], g["P2"], seed * 10, seed))
    for seed in range(16):
        g = fuzz_configs.epi_tall_config(seed)
        c.append(_epi(g["W"], g["H"], g["D"], "general", g["P1"], g["P2"], seed * 10, seed))
    return _dedupe(c)


# ------------------------------------------------------------------------------------------------ calc_pyd_cost_sgm
def window_hints(mvW, mvH, kind, seed, amp=3.0):
    """synth.hint_map's kinds, "far" (whole numbers up to +-14), "zigzag" (x mod 2, y mod 2: +-1 from pixel to pixel) and three
    maps for the large search windows:
    "outside": every value beyond +-100, either sign: with a window side up to 63 and frames up to 24 pixels every sample of
               every candidate falls outside the second image;
    "jumpy":   levels 70 apart that change between any two pixels a path joins (x by (x + 2y) mod 4, y by (2x + y) mod 4), plus
               a fraction: every difference along a path exceeds side + 3 in one axis at least, in either sign, so both clamps
               of the shift tables are hit and every shifted centre is absent;
    "steps":   x by 80 * [x mod 4 in (1, 2)], y by 80 * [y mod 4 in (1, 2)]: a path meets a step beyond any window, then a
               pixel with the same hint as the one before (tests/test_gpu_pyd_windows.py's penalty budgets)."""
    if kind == "far":
        return synth.hint_map(mvW, mvH, "int", seed=seed, amp=14.0)
    yy, xx = np.mgrid[0:mvH, 0:mvW]
    if kind == "outside":
        u = synth.uniform_f64(seed, (2, mvH, mvW))
        sign = np.where(synth.uniform_f64(seed + 1, (2, mvH, mvW)) < 0.5, -1.0, 1.0)
        return np.ascontiguousarray(sign * (100.0 + np.round(u * 80.0) / 4))
    if kind == "jumpy":
        lv = np.stack([(xx + 2 * yy) % 4, (2 * xx + yy) % 4]).astype(np.float64)
        return np.ascontiguousarray(70.0 * lv + np.round(synth.uniform_f64(seed, (2, mvH, mvW)) * 8.0) / 4 - 1.0)
    if kind == "steps":
        return np.ascontiguousarray(80.0 * np.stack([(xx % 4 == 1) | (xx % 4 == 2), (yy % 4 == 1) | (yy % 4 == 2)]).astype(np.float64))
    if kind == "zigzag":
        return np.ascontiguousarray(np.stack([xx % 2, yy % 2]).astype(np.float64))
    return synth.hint_map(mvW, mvH, kind, seed=seed, amp=amp)


def _pyd(W, H, mvW, mvH, rX, rY, rAgg, sub, P1, P2, diag, passes, adaptive, kind, iseed, mseed, amp=3.0, grad=1, edge=False):
    def build():
        I1, I2 = _images(W, H, 16, iseed, edge)
        if grad != 1:
            I1 = (I1.astype(np.int32) * grad % 256).astype(np.uint8)              # larger gradients: adaptive P2 branch taken
        mv = window_hints(mvW, mvH, kind, mseed, amp)
        return I1, I2, mv, rX, rY, rAgg, sub, P1, P2, diag, passes, adaptive
    return (f"{W}x{H}-mv{mvW}x{mvH}-r{rX}_{rY}_{rAgg}-sub{sub}-P{P1}_{P2}-d{diag}p{passes}a{adaptive}-{kind}{amp}-g{grad}-s{iseed}_{mseed}" + ("-edgeimg" if edge else ""),
            build)


KITTI_PYD = _pyd(1242, 375, 1243, 376, 2, 2, 2, 1, 6, 32, 1, 2, 0, "general", 9, 2)
KITTI_PYD_CPU = _pyd(1242, 32, 1243, 33, 2, 2, 2, 1, 6, 32, 1, 2, 0, "general", 9, 2)


def pyd_cases():
    from tests import test_gpu_pyd as T
    c = []
    c += [_pyd(W, H, max(mvW, W), max(mvH, H), rX, rY, rAgg, 1, 6, 32, 1, 2, 0, kind, W, H)
          for W, H, mvW, mvH, rX, rY, rAgg, kind in marks(T.test_pyd_cost_volume_bit_exact, "W")]
    c += [_pyd(W, H, W + 2, H + 1, rX, rY, 2, 1, P1, P2, diag, passes, adaptive, kind, 3, 5, amp=4.0, grad=3)
          for W, H, rX, rY, P1, P2, _, diag, passes, adaptive, kind in T.AGG]
    c += [_pyd(W, H, W + 1, H + 1, 5, 5, 2, sub, 6, 32, 1, 2, 0, kind, 9, 2) for W, H, kind, sub in marks(T.test_calc_pyd_cost_sgm_whole_mex, "W")]
    # edge values: penalties up to 255, totalPass 1 / 2 / 3, diagonals and adaptive P2 either way, degenerate shapes
    for P1, P2 in ((255, 255), (255, 0), (0, 255)):
        for passes in (1, 2, 3):
            c.append(_pyd(17, 12, 18, 14, 2, 1, 1, 1, P1, P2, passes % 2, passes, (passes + 1) % 2, "general", 6, 7, amp=4.0, grad=3))
    c += [_pyd(W, H, W, H, 2, 2, 2, 1, 6, 32, 1, 2, 1, "general", 4, 5, grad=3) for W, H in ((1, 13), (13, 1), (2, 2), (1, 1))]
    # tests/edge_inputs.py's image pairs: strong gradients, a saturated flat area
    c += [_pyd(33, 21, 34, 22, 2, 2, 2, 1, 6, 32, 1, 2, a, "general", 8, 9, grad=1, edge=True) for a in (0, 1)]
    return _dedupe(c)


def pyd_fuzz_cases():
    c = []
    for seed in range(12):
        g = fuzz_configs.pyd_config(seed)
        c.append(_pyd(g["W"], g["H"], g["mvW"], g["mvH"], g["rX"], g["rY"], g["rAgg"], g["sub"], g["P1"], g["P2"], g["diag"],
                      g["passes"], g["adaptive"], g["kind"], seed, seed, amp=g["amp"], grad=3))
    return c


# ---- search windows from 13 to 63 candidates a side (tests/test_gpu_pyd_windows.py; the lists are shared with it)
# half sizes (rX, rY) of 13x9, 15x17, 17x15, 17x17, 31x33, 63x15, 15x63, 63x1, 1x63, 11x13, 13x11
WINDOWS = [(6, 4), (7, 8), (8, 7), (8, 8), (15, 16), (31, 7), (7, 31), (31, 0), (0, 31), (5, 6), (6, 5)]
# line counts 1, 4, 5 and 7 (the generic aggregation kernel advances 4 lines a workgroup), more than one workgroup (9, 13)
WINDOW_FRAMES = [(9, 7), (13, 5), (5, 13), (8, 4), (1, 6), (6, 1)]
# the smallest aggregation radius at which an accepted window leaves the patch kernel, the window there with the fewest
# candidates, and the nearest radius that still takes the patch kernel (tests/test_pyd_limits_cpu.py checks both by enumeration)
COST_FALLBACK = (7, 30, 29)            # rX, rY, rAgg: 15x61
COST_LAST_PATCH = (7, 30, 28)
COST_PATCH_AT_BOUND = (20, 11, 30)     # 41x23: the patch kernel's request is 49152 bytes, the bound itself


def window_cost_cases():
    """(W, H, rX, rY, rAgg, hint kind): every window at aggregation radius 0, 2 and 3 with each hint map, the frames in rotation;
    then the per-candidate kernel's case, its neighbour and the patch kernel at its bound on a frame of six pixels."""
    c, n = [], 0
    for rX, rY in WINDOWS:
        for rAgg in (0, 2, 3):
            for kind in ("general", "int", "outside"):
                c.append(WINDOW_FRAMES[n % len(WINDOW_FRAMES)] + (rX, rY, rAgg, kind))
                n += 1
    c += [(3, 2) + w + ("general",) for w in (COST_FALLBACK, COST_LAST_PATCH, COST_PATCH_AT_BOUND)]
    return c


# diagonals, totalPass, adaptive P2, hint kind: each value of each with either penalty set (the whole-MEX counterparts)
WINDOW_AGG_COMBOS = [(1, 2, 0, "general"), (0, 1, 1, "int"), (1, 3, 1, "jumpy"), (0, 2, 0, "jumpy"), (1, 1, 0, "int"), (0, 3, 1, "general")]
# and their full cross, which the GPU test runs
WINDOW_AGG_CROSS = [(diag, passes, adaptive, kind) for diag in (1, 0) for passes in (1, 2, 3) for adaptive in (0, 1)
                    for kind in ("general", "int", "jumpy")]
WINDOW_PENALTIES = [(6, 32, 24), (100, 200, 255)]          # P1, P2, the uploaded volume's maximum: no-wrap and wrapping


def window_agg_cases(combos=WINDOW_AGG_COMBOS):
    """(W, H, rX, rY, P1, P2, cmax, diagonals, totalPass, adaptive, hint kind)"""
    c, n = [], 0
    for rX, rY in WINDOWS:
        for pen in WINDOW_PENALTIES:
            for combo in combos:
                c.append(WINDOW_FRAMES[n % len(WINDOW_FRAMES)] + (rX, rY) + pen + combo)
                n += 1
            n += 1                                            # (so that the two penalty sets meet different frames)
    return c


def window_whole_cases():
    """(W, H, rX, rY, rAgg, sub, P1, P2, diagonals, totalPass, adaptive, hint kind): one whole call a window"""
    return [WINDOW_FRAMES[i % len(WINDOW_FRAMES)] + (rX, rY, 2, 1, 6, 32, 1, 2, i % 2, "general" if i % 3 else "int")
            for i, (rX, rY) in enumerate(WINDOWS)]


# totalPass around the row-packed WTA's bound (sum of weights * 255 <= 65535: 64 with diagonals, 128 without), a weight above
# a byte (257), and no pass at all
WINDOW_PASSES = [(1, 64), (1, 65), (1, 257), (0, 128), (0, 129), (1, 0), (0, 0)]      # diagonals, totalPass
RULE_WINDOWS = [(5, 5), (2, 2)]                                                      # the reference's 11x11, and 5x5
RULE_FRAMES = [(5, 4), (6, 3)]


def _window(W, H, rX, rY, rAgg, sub, P1, P2, diag, passes, adaptive, kind, grad=1):
    return _pyd(W, H, W + 2, H + 1, rX, rY, rAgg, sub, P1, P2, diag, passes, adaptive, kind, 3 + rX, 5 + rY, amp=4.0, grad=grad)


def pyd_window_cases():
    """The whole-MEX counterparts of tests/test_gpu_pyd_windows.py: its cost cases with the reference's penalties, its aggregation
    cases with the volume the MEX computes itself (so its maximum is 24 whatever the GPU case uploads), its whole calls, and the
    totalPass values and penalty sets of its rule boundaries."""
    c = [_window(W, H, rX, rY, rAgg, 1, 6, 32, 1, 2, 0, kind) for W, H, rX, rY, rAgg, kind in window_cost_cases()]
    c += [_window(W, H, rX, rY, 2, 1, P1, P2, diag, passes, adaptive, kind, grad=3)
          for W, H, rX, rY, P1, P2, _, diag, passes, adaptive, kind in window_agg_cases()]
    c += [_window(*a) for a in window_whole_cases()]
    for (rX, rY), (W, H) in zip(RULE_WINDOWS, RULE_FRAMES):
        c += [_window(W, H, rX, rY, 2, 1, P1, P2, diag, passes, a, "general", grad=3)
              for diag, passes in WINDOW_PASSES for a, (P1, P2) in enumerate(((0, 0), (6, 32)))]
        c += [_window(W, H, rX, rY, 0, 1, P1, P2, 1, 2, 0, kind)
              for P1, P2 in ((6, 100), (200, 31), (201, 31), (116, 115), (117, 115)) for kind in ("steps", "zigzag")]
    return _dedupe(c)


def budget_images(W, H):
    """An image pair whose census codes differ in all 24 bits wherever both pixels have their whole 5x5 neighbourhood inside
    the image: a strictly increasing ramp (W * H <= 256) and its complement."""
    assert W * H <= 256
    I1 = np.arange(W * H, dtype=np.uint8).reshape(H, W)
    return np.ascontiguousarray(I1), np.ascontiguousarray(255 - I1)


# ------------------------------------------------------------------------------------------------ calc_pyd_cost_sgm_ng
def _ng(W, H, mvW, mvH, r, agg, sub, P1, P2, kind, iseed, mseed, amp, edit=None, edge=False):
    def build():
        I1, I2 = _images(W, H, 16, iseed, edge)
        mv = synth.hint_map(mvW, mvH, kind, seed=mseed, amp=amp)
        if edit:
            edit(mv)
        return I1, I2, mv, r, agg, sub, P1, P2
    return (f"{W}x{H}-mv{mvW}x{mvH}-h{r}-agg{agg}-sub{sub}-P{P1}_{P2}-{kind}{amp}-s{iseed}_{mseed}" + (f"-{edit.__name__}" if edit else "") + ("-edgeimg" if edge else ""),
            build)


def extreme_hints(mv):
    """test_gpu_ng.py::test_calc_pyd_cost_sgm_ng_extreme_hints (a 48x20 map)."""
    mv[0, 3:9, 10:20] = 2147483646.0
    mv[1, 5:12, 22:30] = -2147483647.0
    mv[0, 10:14, 30:40] = 3.0e9                           # converts to INT_MIN like cvttsd2si
    mv[1, 0:4, 0:6] = 1073741823.0


def packed_key_range(mv):
    """The +-0x3FF0 regions of test_gpu_configs_full_size.py::_smooth_hints(big=True), scaled from 1242x375 to a small frame
    (regions keep their places relative to the frame), and the band 4096 <= |mv| < 0x3FF0 between the grid box and that range."""
    _, H, W = mv.shape
    def box(y0, y1, x0, x1):
        return slice(y0 * H // 375, max(y1 * H // 375, y0 * H // 375 + 1)), slice(x0 * W // 1242, max(x1 * W // 1242, x0 * W // 1242 + 1))
    mv[(0, *box(40, 80, 100, 300))] = 16360.0                  # just inside 0x3FF0 = 16368
    mv[(1, *box(40, 80, 100, 300))] = -16365.0
    mv[(0, *box(200, 240, 600, 900))] = 16366.0                # candidates 16365..16367 inside, hints of neighbours cross
    mv[(1, *box(200, 230, 700, 800))] = 16370.0                # beyond the range
    mv[(0, *box(300, 330, 20, 120))] = -20000.0
    mv[(0, *box(120, 160, 900, 1100))] = 4096.0                # the band above +-4095
    mv[(1, *box(120, 160, 950, 1150))] = -4097.0
    mv[(0, *box(260, 300, 300, 500))] = -8191.0
    mv[(1, *box(280, 320, 350, 550))] = 12000.5


KITTI_NG_CPU = _ng(1242, 8, 1242, 8, 1, 2, 1, 6, 32, "int", 41, 2, 2.0)


def ng_cases():
    from tests import test_gpu_ng as T
    c = []
    c += [_ng(W, H, mvW, mvH, r, agg, sub, P1, P2, kind, W + r, H, 6.0)
          for W, H, mvW, mvH, r, agg, sub, P1, P2, kind in marks(T.test_calc_pyd_cost_sgm_ng_bit_exact, "W")]
    c += [_ng(48, 20, 48, 20, 1, 2, 0, 6, 32, "int", 7, 3, 5.0, edit=extreme_hints)]
    c += [_ng(45, 38, 45, 38, 1, 2, 1, 6, 32, "int", 6, 9, 2.0)]                                  # matcher_split
    c += [_ng(83, 58, 83, 58, 1, 2, sub, P1, P2, kind, 13, 17, amp)
          for kind, amp, sub, P1, P2, _ in marks(T.test_calc_pyd_cost_sgm_ng_repeated_candidates, "kind")]
    c += [_ng(W, H, W, H, 1, 2, sub, P1, P2, kind, W, H + 3, amp)
          for kind, amp, sub, P1, P2 in marks(T.test_calc_pyd_cost_sgm_ng_grid_matcher, "kind") for W, H in ((83, 58), (17, 40), (200, 9))]
    c += [_ng(61, 37, 61, 37, 1, 2, 1, 6, 32, kind, 50 + i, 60 + i, amp)
          for kind, amp in marks(T.test_calc_pyd_cost_sgm_ng_batch_picks_a_matcher_on_the_device, "kind") for i in range(3)]
    c += [_ng(83, 58, 83, 58, 1, 2, sub, P1, P2, kind, 13 + i, 17 + i, amp)
          for kind, amp, sub, P1, P2, n in marks(T.test_calc_pyd_cost_sgm_ng_compact_kernel, "kind") for i in range(n)]
    c += [_ng(52, 31, 52, 31, 1, 2, 1, 6, 32, ("int", "zero", "general")[i], 20 + i, 30 + i, 2.0) for i in range(3)]
    # edge values: halfSearchWinSize 0 / 1 / 2, hint maps smaller and larger, penalties up to 255, degenerate shapes, the packed
    # key's range on a small frame
    for half in (0, 1, 2):
        c += [_ng(15, 11, mvW, mvH, half, 2, half % 2, P1, P2, "general", 5, 6, 3.0)
              for (mvW, mvH), (P1, P2) in zip(((11, 7), (19, 14), (15, 11)), ((255, 255), (255, 0), (0, 255)))]
    c += [_ng(W, H, W, H, 1, 2, 1, 6, 32, "int", 3, 4, 2.0) for W, H in ((1, 13), (13, 1), (2, 2), (1, 1))]
    c += [_ng(124, 38, 124, 38, 1, 2, 1, 6, 32, "int", 41, 1, 6.0, edit=packed_key_range)]
    c += [_ng(33, 21, 33, 21, 1, 2, sub, 6, 32, "general", 8, 9, 2.0, edge=True) for sub in (0, 1)]   # tests/edge_inputs.py's image pairs
    return _dedupe(c)


def ng_fuzz_cases():
    c = []
    for seed in range(16):
        g = fuzz_configs.ng_config(seed)
        c.append(_ng(g["W"], g["H"], g["mvW"], g["mvH"], g["half"], g["agg"], g["sub"], g["P1"], g["P2"], g["kind"], seed + 50, seed, g["amp"]))
    return c


# ------------------------------------------------------------------------------------------------ calc_cost_sgm_ng
def _otf(W, H, P1, P2, iseed, rseed, grad=5, crop=None, edge=False):
    def build():
        I1, I2 = _images(*(crop or (W, H)), 16, iseed, edge)
        if crop:
            I1, I2 = np.ascontiguousarray(I1[:H, :W]), np.ascontiguousarray(I2[:H, :W])
        if grad != 1:
            I1 = (I1.astype(np.int32) * grad % 256).astype(np.uint8)              # strong gradients: adaptive P2 both ways
        return I1, I2, P1, P2, rseed
    return f"{W}x{H}-P{P1}_{P2}-g{grad}-s{iseed}-srand{rseed}" + (f"-of{crop[0]}x{crop[1]}" if crop else "") + ("-edgeimg" if edge else ""), build


KITTI_OTF = _otf(160, 120, 6, 32, 160 * 120, 1)      # the largest size the GPU suite runs the on-the-fly variant at


def otf_cases():
    from tests import test_gpu_ng as T
    c = [_otf(W, H, P1, P2, W * H, 1) for W, H, P1, P2 in marks(T.test_calc_cost_sgm_ng_bit_exact, "W") if (W, H) != (160, 120)]
    c += [_otf(20, 12, 6, 32, 4, 1, grad=1), _otf(37, 21, 6, 32, 11, 1, grad=1)]            # the libc-draws and exact-matcher tests
    c += [_otf(23, 14, 6, 32, 40 + i, 7 + i, grad=1) for i in range(3)]                        # test_ng_batches_match_single_calls
    c += [_otf(14, 9, P1, P2, 5, 3) for P1, P2 in ((255, 255), (255, 0), (0, 255))]
    c += [_otf(33, 21, 6, 32, 8, 2, grad=1, edge=True)]                                        # tests/edge_inputs.py's image pairs
    return _dedupe(c)


def otf_fuzz_cases():
    c = []
    for seed in range(16):
        g = fuzz_configs.ng_config(seed)
        c.append(_otf(min(g["W"], 24), min(g["H"], 16), g["P1"], g["P2"], seed + 50, seed + 1, grad=1, crop=(g["W"], g["H"])))
    return c


# ------------------------------------------------------------------------------------------------ fixture cases
def far_hints(mv):
    """Hints beyond the 12x12 grid box next to near ones, repeated candidates (a constant patch), and the band
    4096 <= |mv| < 0x3FF0 with its two borders."""
    _, H, W = mv.shape
    mv[:, : H // 2, : W // 3] = 1.0
    mv[0, H // 2:, : W // 4] = 4095.0
    mv[1, H // 2:, W // 4: W // 2] = -4096.0
    mv[0, : H // 3, W // 2:] = 9000.0
    mv[1, H // 3: 2 * H // 3, 2 * W // 3:] = -16367.0
    mv[0, 2 * H // 3:, 2 * W // 3:] = 16368.0
    mv[1, -2:, -3:] = 20000.5


def golden_cases(name):
    """The small cases of tests/golden/ref_mex_<name>.npz: between them every flag value the parity tests sweep."""
    if name == "calc_cost_sgm":
        return [_epi(24, 16, 16, "general", 6, 64, 1, 2), _epi(21, 13, 32, "general", 6, 32, 3, 4), _epi(17, 11, 64, "axis", 6, 64, 5, 6),
                _epi(13, 9, 128, "radial", 6, 64, 7, 8), _epi(16, 10, 20, "general", 100, 200, 9, 10), _epi(1, 9, 16, "general", 6, 64, 11, 12),
                _epi(9, 1, 16, "general", 6, 64, 13, 14), _epi(2, 2, 16, "general", 255, 255, 15, 16),
                _epi(40, 24, 16, "axis", 6, 64, 8, 7, edit=rounding), _epi(15, 11, 7, "radial", 0, 255, 17, 18, vMax=0.25),
                _epi(20, 12, 16, "general", 255, 0, 5, 9, edit=out_of_range)]
    if name == "calc_pyd_cost_sgm":
        return [_pyd(24, 18, 24, 18, 2, 2, 2, 1, 6, 32, 1, 2, 0, "zero", 1, 2), _pyd(21, 15, 25, 19, 3, 1, 2, 1, 6, 32, 1, 2, 1, "general", 3, 4, grad=3),
                _pyd(20, 14, 21, 14, 1, 3, 1, 0, 255, 255, 0, 2, 0, "int", 5, 6, amp=4.0), _pyd(1, 12, 1, 12, 2, 2, 2, 1, 6, 32, 1, 2, 1, "general", 7, 8),
                _pyd(12, 1, 13, 2, 2, 2, 2, 1, 6, 32, 1, 2, 0, "general", 9, 10), _pyd(2, 2, 2, 2, 1, 1, 1, 1, 6, 32, 1, 2, 0, "int", 11, 12),
                _pyd(19, 13, 19, 13, 2, 3, 2, 1, 0, 255, 1, 1, 0, "general", 13, 14, grad=3),
                _pyd(19, 13, 20, 15, 2, 3, 2, 1, 100, 200, 1, 3, 1, "even", 15, 16, grad=3), _pyd(16, 12, 16, 12, 0, 0, 0, 0, 6, 32, 0, 3, 1, "general", 17, 18),
                _pyd(22, 12, 24, 13, 5, 5, 2, 1, 255, 0, 1, 2, 0, "far", 19, 20), _pyd(18, 11, 18, 11, 6, 2, 3, 0, 6, 32, 0, 1, 1, "int", 21, 22, amp=4.0, grad=3),
                # search windows of 17x17 (the smallest with 16 candidates a lane), 31x33 (1023 candidates), 63x15, 15x63, 1x63
                # and 63x1, and totalPass on either side of the row-packed WTA's bound at 11x11
                _window(9, 7, 8, 8, 2, 1, 6, 32, 1, 2, 0, "general"), _window(13, 5, 15, 16, 2, 1, 100, 200, 1, 3, 1, "int", grad=3),
                _window(5, 13, 31, 7, 3, 1, 6, 32, 0, 2, 0, "jumpy"), _window(8, 4, 7, 31, 0, 1, 6, 32, 1, 1, 1, "general", grad=3),
                _window(6, 1, 0, 31, 2, 1, 6, 32, 1, 2, 0, "int"), _window(1, 6, 31, 0, 2, 1, 100, 200, 1, 2, 0, "general"),
                _window(5, 4, 5, 5, 2, 1, 6, 32, 1, 64, 0, "general"), _window(5, 4, 5, 5, 2, 1, 6, 32, 1, 65, 1, "general", grad=3),
                _window(6, 3, 5, 5, 2, 1, 0, 0, 0, 129, 0, "int"), _window(6, 3, 2, 2, 2, 1, 6, 32, 1, 257, 0, "general")]
    if name == "calc_pyd_cost_sgm_ng":
        return [_ng(20, 14, 20, 14, 1, 2, 0, 6, 32, "zero", 1, 2, 1.0), _ng(22, 16, 15, 10, 1, 5, 1, 6, 32, "general", 3, 4, 6.0),
                _ng(19, 13, 24, 17, 1, 2, 1, 90, 120, "int", 5, 6, 2.0), _ng(14, 10, 14, 10, 2, 3, 0, 6, 32, "even", 7, 8, 3.0),
                _ng(16, 11, 16, 11, 0, 0, 1, 255, 255, "general", 9, 10, 0.8), _ng(1, 12, 1, 12, 1, 2, 1, 6, 32, "general", 11, 12, 6.0),
                _ng(12, 1, 12, 1, 1, 2, 0, 0, 255, "int", 13, 14, 9.0), _ng(2, 2, 2, 2, 1, 2, 1, 255, 0, "int", 15, 16, 2.0),
                _ng(48, 20, 48, 20, 1, 2, 0, 6, 32, "int", 7, 3, 5.0, edit=extreme_hints),
                _ng(62, 19, 62, 19, 1, 2, 1, 6, 32, "int", 41, 1, 6.0, edit=packed_key_range),
                _ng(30, 18, 30, 18, 1, 2, 1, 6, 32, "int", 17, 18, 9.0, edit=far_hints), _ng(17, 12, 17, 12, 2, 1, 1, 6, 32, "int", 19, 20, 9.0, edit=far_hints)]
    if name == "calc_cost_sgm_ng":
        return [_otf(20, 12, 6, 32, 1, 1), _otf(17, 9, 6, 32, 2, 2, grad=1), _otf(12, 10, 100, 200, 3, 1), _otf(7, 3, 6, 32, 4, 5), _otf(2, 2, 6, 32, 5, 1),
                _otf(1, 5, 6, 32, 6, 1), _otf(5, 1, 6, 32, 7, 9), _otf(4, 6, 255, 255, 8, 3), _otf(3, 4, 0, 255, 9, 1), _otf(16, 12, 255, 0, 10, 12345)]
    raise ValueError(name)
