"""GPU parity tests of the fused block-sweep and pair pipelines (fsgm_amd/csrc/epi_sweep.hip) at the edges of their byte budgets,
with costs as large as the no-wrap condition admits: what a caller's own cost volume (sgm(C), cost_bound) can bring, where census
costs stop at 24.

choose_pipeline (fsgm_amd/csrc/capi_epi.hip) takes these pipelines for 0 <= P1 <= P2, cm + P2 + max(P1, P2) <= 255 and
3 * (P1 + P2) <= 255 (the sweeps: three y + P1 summed into one byte) or 2 * (P1 + P2) <= 255 (a pair: two).  Against the CPU oracle,
bit for bit and with no pixel excluded: S of every voxel (debug tap), minC and bestD of every pixel, for

  * penalty sets on the budgets (3 * (P1 + P2) = 255, P1 + P2 = 127), P1 = 0, P1 = P2, (0, 0) with S up to 8 * 255 = 2040 (the
    documented limit of the WTA keys), each at the largest cost the no-wrap condition admits;
  * five volumes a case (tests/budget_volumes.py): uniform, zeroed columns, one strong minimum a pixel, the constant volume (the
    largest sum bytes in nearly every voxel, every d tied: the first-minimum rule) and all zeros;
  * D = 16 .. 256 (1 .. 16 lanes a pixel) on the smallest frames that cross one column strip and one row block of the sweeps;
  * the small-batch sub-forms (5 frames) and the large-batch ones (17 frames) of epi_select_kernel;
  * penalty sets and costs just outside the budgets, which must take the line kernels and still match;
  * fsgm::sgm on a caller's volume with cost_bound at the case's largest cost.

Every case asserts the kernel it ran by name."""
import numpy as np
import pytest
import torch  # noqa: I001 -- before the library: its HIP runtime is the one libfsgm_hip.so binds to (fsgm_amd/torch_ops.py)

from fsgm_amd import torch_ops, synth, EpiPlan  # noqa: E402
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA  # noqa: E402
from fsgm_amd.sgm import last_kernel  # noqa: E402
from tests import budget_volumes as BV  # noqa: E402

pytestmark = pytest.mark.gpu

SWEEPS = ((2, "sweep16/nowrap"), (3, "sweep16par/nowrap"), (6, "sweep16mid/nowrap"))
PAIRS = ((2, "pairs16/nowrap"),)
DS = (16, 32, 64, 128, 256)


def _run_and_check(oracle, W, H, D, vols, paths, P1, P2, modes, kinds=BV.KINDS):
    """One plan, every mode of `modes` in turn: (mode, the kernel name it must report)."""
    B = len(vols)
    _, _, off = synth.epi_maps(W, H, "general", seed=5)
    want = []
    for v in vols:
        S = oracle.epi_aggregate(v, P1, P2, paths)
        bd, mc = oracle.epi_wta(S, W, H, D, 1)
        want.append((S[:-1].reshape(H, W, D), mc, oracle.epi_vz_to_disp(bd, off, 0.3, D + 1)))
    print(f"{paths} paths, P ({P1}, {P2}), {W}x{H}x{D}, {B} frames: max C {max(int(v.max()) for v in vols)}, "
          f"max S {max(int(w[0].max()) for w in want)}")
    with EpiPlan(W, H, D, B, paths=paths) as plan:
        plan.set_penalties(P1, P2, 0.3)
        for f in range(B):
            plan.upload_cost(f, vols[f])
            plan.upload_offset(f, off)
        for mode, name in modes:
            plan.set_agg_mode(mode)
            assert plan.kernel_name == name, f"mode {mode}"
            plan.run(STAGE_AGGREGATE | STAGE_WTA)
            for f in range(B):
                what = f"mode {mode} ({name}), frame {f} ({kinds[f % len(kinds)]})"
                np.testing.assert_array_equal(plan.download_sum(f), want[f][0], err_msg=f"{what}: S")
                gbd, gmc = plan.download(f)
                np.testing.assert_array_equal(gmc, want[f][1], err_msg=f"{what}: minC")
                np.testing.assert_array_equal(gbd, want[f][2], err_msg=f"{what}: bestD")
        plan.sync()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P1,P2", BV.SWEEP_PENALTIES)
def test_sweeps_at_the_largest_cost(gpu_lib, oracle, P1, P2, D):
    W, H = BV.sweep_shape(D)
    cmax = BV.nowrap_cmax(P1, P2)
    assert 3 * (P1 + P2) <= 255 and 0 <= P1 <= P2
    vols = BV.volumes(W, H, D, cmax, seed=7 * P1 + P2 + D)
    assert max(int(v.max()) for v in vols[:4]) == min(int(v.max()) for v in vols[:4]) == cmax
    _run_and_check(oracle, W, H, D, vols, 8, P1, P2, SWEEPS)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P1,P2", BV.PAIR_PENALTIES)
def test_pairs_at_the_largest_cost(gpu_lib, oracle, P1, P2, D):
    W, H = BV.sweep_shape(D)
    cmax = BV.nowrap_cmax(P1, P2)
    assert 2 * (P1 + P2) <= 255 and 0 <= P1 <= P2
    vols = BV.volumes(W, H, D, cmax, seed=7 * P1 + P2 + D)
    assert max(int(v.max()) for v in vols[:4]) == min(int(v.max()) for v in vols[:4]) == cmax
    _run_and_check(oracle, W, H, D, vols, 4, P1, P2, PAIRS)


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("paths,P1,P2,modes", [(8, 21, 64, SWEEPS), (4, 63, 64, PAIRS)])
def test_large_batch_forms_at_the_largest_cost(gpu_lib, oracle, paths, P1, P2, modes, D):
    """17 frames: past every small-batch switch of epi_select_kernel (the along-x pair's finer split below 16 frames, or up to 10;
    8-wave workgroups up to 10; the along-x pair as line kernels up to 5) -- the coarse, non-tall forms without x lines."""
    W, H = BV.sweep_shape(D)
    vols = BV.volumes(W, H, D, BV.nowrap_cmax(P1, P2), seed=1000 + D, n=17)
    _run_and_check(oracle, W, H, D, vols, paths, P1, P2, modes)


OUTSIDE = [
    # paths, P1, P2, cmax, modes, the line kernels that must run
    (8, 22, 64, 127, (2, 3, 6), "packed16/nowrap"),     # 3 * 86 = 258
    (4, 64, 64, 127, (2,), "packed16/nowrap"),          # 2 * 128 = 256
    (8, 21, 64, 128, (2,), "packed16/wrap"),            # one above the no-wrap budget
    (4, 21, 64, 128, (2,), "packed16/wrap"),
    (8, 10, 9, 24, (2,), "packed16/nowrap"),            # P1 > P2
]


@pytest.mark.parametrize("D", (16, 128))
@pytest.mark.parametrize("paths,P1,P2,cmax,modes,name", OUTSIDE)
def test_just_outside_the_budgets(gpu_lib, oracle, paths, P1, P2, cmax, modes, name, D):
    """A forced fused mode on a configuration one unit outside a budget runs the named line kernels, and matches."""
    W, H = BV.sweep_shape(D)
    kinds = ("uniform", "constant")
    vols = [BV.volume(k, W, H, D, cmax, seed=3 * P1 + D + i) for i, k in enumerate(kinds)]
    assert all(int(v.max()) == cmax for v in vols)
    _run_and_check(oracle, W, H, D, vols, paths, P1, P2, tuple((m, name) for m in modes), kinds)


FRONT_DOOR = [(2, 8, 21, 64, "sweep16/nowrap"), (3, 8, 0, 85, "sweep16par/nowrap"), (6, 8, 42, 43, "sweep16mid/nowrap"),
              (2, 4, 63, 64, "pairs16/nowrap")]


@pytest.mark.parametrize("mode,paths,P1,P2,kernel", FRONT_DOOR)
def test_callers_volume_at_the_bound(gpu_lib, oracle, mode, paths, P1, P2, kernel):
    """fsgm::sgm on (N, D, H, W) volumes whose costs reach cost_bound, the largest the fused pipeline admits"""
    W, H, D, n = 40, 12, 16, 4
    cmax = BV.nowrap_cmax(P1, P2)
    vols = np.stack(BV.volumes(W, H, D, cmax, seed=50 + P1, n=n))                  # uniform, columns, minimum, constant
    assert all(int(v.max()) == cmax for v in vols)
    Ct = torch.from_numpy(np.ascontiguousarray(vols.transpose(0, 3, 1, 2))).to("cuda:0")
    bestD, minC, S, status = torch_ops.sgm(Ct, P1, P2, layout="dhw", paths=paths, cost_bound=cmax, agg_mode=mode,
                                           return_sum=True, return_status=True)
    torch.cuda.synchronize()
    assert last_kernel() == kernel
    assert int(status.item()) == 0
    for f in range(n):
        wS = oracle.epi_aggregate(vols[f], P1, P2, paths)
        wbd, wmc = oracle.epi_wta(wS, W, H, D, 1)
        np.testing.assert_array_equal(S[f].cpu().numpy(), wS[:-1].reshape(H, W, D), err_msg=f"frame {f}: S")
        np.testing.assert_array_equal(minC[f].cpu().numpy(), wmc, err_msg=f"frame {f}: minC")
        np.testing.assert_array_equal(bestD[f].cpu().numpy(), wbd, err_msg=f"frame {f}: bestD")
