"""The two-kernel form of the cost stage -- a raw-cost kernel into a volume in HBM, then a 5x5 box kernel -- at every D class,
row block and batch: what every dMax other than 16, 32, 64, 128, 256 runs (and those under FSGM_COST_FUSED=0).  Every voxel of
plan.download_cost() is compared for equality, epipolar plans with oracle.epi_cost (pinned to the reference's compiled code,
calc_cost_sgm.cpp:343-407), rectified plans with stereo_restatement.box_mean(rectified_raw_cost()); every case first asserts the
kernels it means to run by the name fsgm_amd.epi.cost_kernels gives (the launchers' own selector; its table:
tests/test_cost_kernels_cpu.py).

The box kernels' geometry, restated once (epi_cost.hip): a workgroup of 256 lanes covers BOX_ROWS = 32 rows of `cols` columns
and walks its rows in rounds of 5 through a ring of 5 horizontal sums, preloaded from rows y0 - 2 .. y0 + 1;

    box16 (D % 16 == 0): D / 16 lanes a pixel, cols = 256 // (D // 16)      D    16  48  80  96  112  144  160  224  256  1024
                                                                            cols 256  85  51  42   36   28   25   18   16     4
    box4  (D % 4 == 0):  D / 4 lanes a pixel,  cols = 256 // (D // 4)       D    20  24  100  516  1020
                                                                            cols 51  42   10    1     1
    box1  (any D):       a thread per pixel and four d, 25 taps, no rows or columns

Case ids per kernel (name as cost_kernels reports it) that reach: more than 32 rows | more than one column of workgroups (for the
kernels without columns: more than one workgroup) | a batch of three frames.  Ids without their test_ prefix, * for every value
of that place (a rectified case's id ends in its direction, -1 or 1)

    px      rows[48-7x33] rows[48-7x65] px_pixels[*-321]   | cols[48-173x6] cols[24-87x6] px_pixels[*-321] | batch_plan[48] batch_plan[24] batch_call[48]
    vec4    rows[20-7x33] rows[20-7x37] rows[20-7x65]      | cols[20-105x6] cols[100-23x6]                 | batch_plan[20] batch_call[20]
    scalar  rows[7-7x33] rows[7-7x65] scalar[*-7x33]       | rows[7-7x65] scalar[1023-7x33]                | batch_plan[7] batch_call[7]
    stereo  rectified[48-*] rectified[20-*] rectified[7-*] | rectified[48-*] (86 x 33 x 48 = 533 workgroups) | batch_rectified[48-*] batch_rectified[100-*]
    box16   rows[48-7x33] cols[*-*x33] rectified[48-*]     | cols[48-86x6] cols[1024-11x6] cols[16-257x6]  | batch_plan[48] batch_rectified[48-*]
    box4    rows[20-7x33] cols[20-52x33] cols[516-2x33]    | cols[20-52x6] cols[24-43x6] cols[1020-5x6]    | batch_plan[24] batch_plan[20] batch_rectified[100-*]
    box1    rows[7-7x33] rows[7-7x65] rectified[7-*]       | rows[7-7x65] scalar[1023-7x33]                | batch_plan[7] batch_call[7]
"""
import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import synth, EpiPlan, _lib
from fsgm_amd._lib import STAGE_COST
from fsgm_amd.epi import cost_kernels
from tests import stereo_restatement as R

pytestmark = pytest.mark.gpu

KINDS = ("axis", "general", "radial")
BOX16_COLS = {16: 256, 48: 85, 80: 51, 96: 42, 112: 36, 144: 28, 160: 25, 224: 18, 256: 16, 1024: 4}
BOX4_COLS = {20: 51, 24: 42, 100: 10, 516: 1, 1020: 1}
FUSED_D = (16, 32, 64, 128, 256)


def _name(D, rect=False):
    """the kernels of the two-kernel form by the divisibility of D, for frames below 2^22 columns and 2^24 rows"""
    raw = "stereo" if rect else "px" if D % 8 == 0 else "vec4" if D % 4 == 0 else "scalar"
    return raw + "+" + ("box16" if D % 16 == 0 else "box4" if D % 4 == 0 else "box1")


def _images(W, H, D, seed):
    """synth.image_pair with rows 30 .. 34 of the second image replaced by noise of their own: the raw costs of the rows either
    side of the box kernels' block boundary at y = 32 differ from row to row, so a ring restarted with the wrong rows shows"""
    I1, I2 = synth.image_pair(W, H, D, seed=seed)
    for y in range(30, min(35, H)):
        I2[y] = synth.uniform_u8(1000 * seed + y, (W,))
    return I1, I2


def _frame(W, H, D, seed, kind):
    return _images(W, H, D, seed) + synth.epi_maps(W, H, kind, seed=seed + 3)


def _plan_cost(W, H, D, frames, name):
    """C of every frame through an epipolar plan that runs `name` (frames: list of (I1, I2, pd0, nd, off))"""
    assert cost_kernels(W, H, D) == name
    with EpiPlan(W, H, D, len(frames), paths=8) as plan:
        plan.set_penalties(6, 64, 0.3)
        for f, fr in enumerate(frames):
            plan.upload(f, *fr)
        plan.run(STAGE_COST)
        return [plan.download_cost(f) for f in range(len(frames))]


def _rect_cost(W, H, D, pairs, direction, name):
    assert cost_kernels(W, H, D, _lib.SAMPLING_RECTIFIED) == name
    with EpiPlan(W, H, D, len(pairs), sampling=_lib.SAMPLING_RECTIFIED, direction=direction) as plan:
        for f, (I1, I2) in enumerate(pairs):
            plan.upload_images(f, I1, I2)
        plan.run(STAGE_COST)
        return [plan.download_cost(f) for f in range(len(pairs))]


def _check(oracle, W, H, D, seed, kind, name):
    fr = _frame(W, H, D, seed, kind)
    want = oracle.epi_cost(fr[0], fr[1], D, 0.3, *fr[2:])
    got = _plan_cost(W, H, D, [fr], name)[0]
    np.testing.assert_array_equal(got, want, err_msg=f"{W}x{H}x{D} {kind} {name}")


# ---- row blocks: fewer rows than the window (1, 2, 4), one round of the ring (5), either side of a block (31, 32, 33), a second
# block that ends inside a round (37), a third block of one row (65); 7 columns
@pytest.mark.parametrize("D,H", [pytest.param(D, H, id=f"{D}-7x{H}") for D in (48, 20, 7) for H in (1, 2, 4, 5, 31, 32, 33, 37, 65)])
def test_rows(gpu_lib, oracle, D, H):
    _check(oracle, 7, H, D, seed=D + H, kind=KINDS[H % 3], name=_name(D))


# ---- columns a workgroup: one short of, exactly, one past a workgroup's columns and two workgroups with a ragged third (6 rows),
# and one past with a second row block (33 rows).  cols == 1 has no frame one short of it.
def _col_cases():
    out = []
    for D, cols in list(BOX16_COLS.items()) + list(BOX4_COLS.items()):
        for W, H in [(cols - 1, 6), (cols, 6), (cols + 1, 6), (2 * cols + 3, 6), (cols + 1, 33)]:
            if W >= 1:
                out.append(pytest.param(D, W, H, id=f"{D}-{W}x{H}"))
    return out


@pytest.mark.parametrize("D,W,H", _col_cases())
def test_cols(gpu_lib, oracle, monkeypatch, D, W, H):
    cols = BOX16_COLS.get(D) or BOX4_COLS[D]
    assert cols == 256 // (D // 16 if D % 16 == 0 else D // 4)
    assert W * H * D < 2_000_000
    if D in FUSED_D:
        monkeypatch.setenv("FSGM_COST_FUSED", "0")
    _check(oracle, W, H, D, seed=D + W, kind=KINDS[(W + H) % 3], name=_name(D))


# ---- the raw-cost kernels.  px: a wave is 64 pixels, a workgroup 256; segments of 128 candidates, the last of 8 (136, 264), 120
# (1016) or whole (1024); a column and a row of NP pixels
@pytest.mark.parametrize("D,NP", [pytest.param(D, NP, id=f"{D}-{NP}") for D in (8, 24, 136, 264, 1016, 1024)
                                  for NP in (63, 64, 65, 255, 256, 257, 321)])
def test_px_pixels(gpu_lib, oracle, D, NP):
    _check(oracle, NP, 1, D, seed=D + NP, kind=KINDS[NP % 3], name=_name(D))
    _check(oracle, 1, NP, D, seed=D + NP + 1, kind=KINDS[(NP + 1) % 3], name=_name(D))


@pytest.mark.parametrize("D,W,H", [pytest.param(D, W, H, id=f"{D}-{W}x{H}") for D in (4, 12, 20, 100) for W, H in ((1, 1), (13, 5), (7, 33))])
def test_vec4(gpu_lib, oracle, D, W, H):
    assert _name(D) == "vec4+box4"
    _check(oracle, W, H, D, seed=D + W, kind=KINDS[(D // 4 + W) % 3], name="vec4+box4")


@pytest.mark.parametrize("D,W,H", [pytest.param(D, W, H, id=f"{D}-{W}x{H}") for D in (1, 2, 3, 5, 50, 257, 1023)
                                   for W, H in ((1, 1), (13, 5), (7, 33))])
def test_scalar(gpu_lib, oracle, D, W, H):
    assert _name(D) == "scalar+box1"
    _check(oracle, W, H, D, seed=D + W, kind=KINDS[(D + W) % 3], name="scalar+box1")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [48, 24, 20, 7])
def test_direction_fields(gpu_lib, oracle, D, kind):
    """all three direction fields through every raw / box pair, two row blocks"""
    _check(oracle, 23, 34, D, seed=D + len(kind), kind=kind, name=_name(D))


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("D,W,H", [pytest.param(48, 86, 33, id="48-86x33"), pytest.param(20, 52, 33, id="20-52x33"),
                                   pytest.param(7, 9, 33, id="7-9x33")])
def test_rectified(gpu_lib, D, W, H, direction):
    """stereo_rawcost_kernel in front of each box kernel: one column past a workgroup's, two row blocks"""
    I1, I2 = _images(W, H, D, seed=D + 1)
    got = _rect_cost(W, H, D, [(I1, I2)], direction, _name(D, rect=True))[0]
    np.testing.assert_array_equal(got, R.box_mean(R.rectified_raw_cost(I1, I2, D, direction)))


# ---- batches: three frames with images and maps of their own, every frame compared: the frame strides of pd0, nd, off, Craw, C
BATCH = (23, 34)


def _batch_frames(D):
    W, H = BATCH
    return [_frame(W, H, D, seed=10 * D + i, kind=KINDS[(D + i) % 3]) for i in range(3)]


@pytest.mark.parametrize("D", [48, 24, 20, 7])
def test_batch_plan(gpu_lib, oracle, D):
    W, H = BATCH
    frames = _batch_frames(D)
    got = _plan_cost(W, H, D, frames, _name(D))
    for i, fr in enumerate(frames):
        np.testing.assert_array_equal(got[i], oracle.epi_cost(fr[0], fr[1], D, 0.3, *fr[2:]), err_msg=f"frame {i}")


@pytest.mark.parametrize("D", [48, 24, 20, 7])
def test_batch_call(gpu_lib, oracle, D):
    W, H = BATCH
    frames = _batch_frames(D)
    assert cost_kernels(W, H, D) == _name(D)
    res = fsgm_amd.calc_cost_sgm_batch(frames, D, 0.3, 6, 64, return_volumes=True)
    for i, fr in enumerate(frames):
        np.testing.assert_array_equal(res[i][2], oracle.epi_cost(fr[0], fr[1], D, 0.3, *fr[2:]), err_msg=f"frame {i}")


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("D", [48, 100])
def test_batch_rectified(gpu_lib, D, direction):
    W, H = BATCH
    pairs = [_images(W, H, D, seed=7 * D + i) for i in range(3)]
    got = _rect_cost(W, H, D, pairs, direction, _name(D, rect=True))
    for i, (I1, I2) in enumerate(pairs):
        np.testing.assert_array_equal(got[i], R.box_mean(R.rectified_raw_cost(I1, I2, D, direction)), err_msg=f"frame {i}")


# ---- the general rounding body: a wave (px) or a thread (vec4, scalar) with a sample position that may reach 2^31 or is not
# finite takes the restated x86 conversion.  70 x 5: row 2 is pixels 140 .. 209, in the px kernel's waves 2 and 3; rows 1 and 3
# stay ordinary and share those waves
@pytest.mark.parametrize("D", [24, 48, 20, 7])
def test_general_rounding_body(gpu_lib, oracle, D):
    W, H = 70, 5
    I1, I2, pd0, nd, off = _frame(W, H, D, seed=5 + D, kind="general")
    off[2, 4] = 1e12
    pd0[0, 2, 9] = np.inf
    pd0[1, 2, 10] = np.nan
    pd0[0, 2, 61] = 2147483648.5
    nd[0, 2, 30] = np.nan
    want = oracle.epi_cost(I1, I2, D, 0.3, pd0, nd, off)
    got = _plan_cost(W, H, D, [(I1, I2, pd0, nd, off)], _name(D))[0]
    np.testing.assert_array_equal(got, want)


# ---- the top of the cost range: a strictly increasing ramp next to a flat area, and its complement.  Census codes of the ramp and
# of its complement differ in all 24 bits, those of the flat areas in none: raw costs of 24 and of 0 over whole 5x5 windows, the
# box kernels' 16-bit fields at their largest sum, 25 x 24 = 600
def _complement_pair():
    I1 = np.full((16, 32), 128, np.uint8)
    I1[:, :16] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return I1, np.ascontiguousarray(255 - I1)


@pytest.mark.parametrize("D", [48, 20, 7])
def test_cost_range(gpu_lib, oracle, D):
    W, H = 32, 16
    I1, I2 = _complement_pair()
    pd0, nd, off = synth.epi_maps(W, H, "general", seed=3)
    want, raw = oracle.epi_cost(I1, I2, D, 0.3, pd0, nd, off, want_raw=True)
    assert (want == 24).any() and (want == 0).any() and raw.max() == 24          # from the oracle alone
    assert set(np.unique(want).tolist()) == set(range(25))                       # and every mean in between
    got = _plan_cost(W, H, D, [(I1, I2, pd0, nd, off)], _name(D))[0]
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("D", [48, 20, 7])
def test_cost_range_rectified(gpu_lib, D, direction):
    I1, I2 = _complement_pair()
    want = R.box_mean(R.rectified_raw_cost(I1, I2, D, direction))
    assert (want == 24).any() and (want == 0).any()
    got = _rect_cost(32, 16, D, [(I1, I2)], direction, _name(D, rect=True))[0]
    np.testing.assert_array_equal(got, want)
