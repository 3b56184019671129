"""Seeded random-configuration parity sweep: GPU (through the C ABI) vs CPU oracle over random
shapes, disparity ranges, penalties, hint maps and switches -- shapes that are not multiples of
any tile (strip, wave, row block) and parameters on both sides of the no-wrap boundary."""
import os

import numpy as np
import pytest

from fsgm_amd import synth, EpiPlan, PydPlan, calc_pyd_cost_sgm_ng, calc_cost_sgm_ng
from fsgm_amd._lib import STAGE_AGGREGATE, STAGE_WTA, STAGE_ALL

from tests import fuzz_configs          # the draws, shared with tests/test_oracle_ref_parity.py

pytestmark = pytest.mark.gpu

# FSGM_FUZZ_SEEDS=N in the environment runs every sweep below with N seeds instead of its default count (a soak run)
_SOAK = int(os.environ.get("FSGM_FUZZ_SEEDS", "0"))


def _seeds(default):
    return range(_SOAK if _SOAK > 0 else default)


@pytest.mark.parametrize("seed", _seeds(24))
def test_epi_random_configs(gpu_lib, oracle, seed):
    c = fuzz_configs.epi_config(seed)
    D, W, H, paths, P1, P2, cmax, sub, vz, B = (c[k] for k in ("D", "W", "H", "paths", "P1", "P2", "cmax", "sub", "vz", "B"))
    vols = [synth.cost_volume(W, H, D, seed=seed * 10 + f, cmax=cmax) for f in range(B)]
    _, _, off = synth.epi_maps(W, H, "general", seed=seed)
    with EpiPlan(W, H, D, B, paths=paths, subpixel=sub, vz_to_disp=vz) as plan:
        plan.set_penalties(P1, P2, 0.3)
        for f in range(B):
            plan.upload_cost(f, vols[f])
            plan.upload_offset(f, off)
        for mode in (1, 2, 3, 6, 4, 5):                      # a mode whose pipeline does not cover the configuration falls back
            plan.set_agg_mode(mode)
            plan.run(STAGE_AGGREGATE | STAGE_WTA)
            for f in range(B):
                S = oracle.epi_aggregate(vols[f], P1, P2, paths)
                bd, mc = oracle.epi_wta(S, W, H, D, sub)
                if vz:
                    bd = oracle.epi_vz_to_disp(bd, off, 0.3, D + 1)
                gbd, gmc = plan.download(f)
                msg = f"seed {seed} mode {mode} {plan.kernel_name} W{W} H{H} D{D} paths{paths} P{P1},{P2} frame {f}"
                np.testing.assert_array_equal(gmc, mc, err_msg=msg)
                np.testing.assert_array_equal(gbd, bd, err_msg=msg)
                np.testing.assert_array_equal(plan.download_sum(f), S[:-1].reshape(H, W, D), err_msg=msg)


@pytest.mark.parametrize("seed", _seeds(16))
def test_epi_random_tall_configs(gpu_lib, oracle, seed):
    """Tall narrow frames: several bands of the band sweeps (both forms), several row blocks of the block sweeps."""
    c = fuzz_configs.epi_tall_config(seed)
    D, W, H, paths, P1, P2, sub, vz, B = (c[k] for k in ("D", "W", "H", "paths", "P1", "P2", "sub", "vz", "B"))
    vols = [synth.cost_volume(W, H, D, seed=seed * 10 + f, cmax=24) for f in range(B)]
    for v in vols:
        v[:, ::4, :] = 0
    _, _, off = synth.epi_maps(W, H, "general", seed=seed)
    want = []
    for f in range(B):
        S = oracle.epi_aggregate(vols[f], P1, P2, paths)
        bd, mc = oracle.epi_wta(S, W, H, D, sub)
        want.append((oracle.epi_vz_to_disp(bd, off, 0.3, D + 1) if vz else bd, mc, S[:-1].reshape(H, W, D)))
    with EpiPlan(W, H, D, B, paths=paths, subpixel=sub, vz_to_disp=vz) as plan:
        plan.set_penalties(P1, P2, 0.3)
        for f in range(B):
            plan.upload_cost(f, vols[f])
            plan.upload_offset(f, off)
        for mode in (4, 5, 2, 6, 1, 5, 4):
            plan.set_agg_mode(mode)
            plan.run(STAGE_AGGREGATE | STAGE_WTA)
            for f in range(B):
                gbd, gmc = plan.download(f)
                msg = f"seed {seed} mode {mode} {plan.kernel_name} W{W} H{H} D{D} paths{paths} P{P1},{P2} frame {f}"
                np.testing.assert_array_equal(gmc, want[f][1], err_msg=msg)
                np.testing.assert_array_equal(gbd, want[f][0], err_msg=msg)
            np.testing.assert_array_equal(plan.download_sum(B - 1), want[B - 1][2], err_msg=f"seed {seed} mode {mode} S")
        plan.sync()


@pytest.mark.parametrize("seed", _seeds(12))
def test_pyd_random_configs(gpu_lib, oracle, seed):
    c = fuzz_configs.pyd_config(seed)
    W, H, rX, rY, rAgg, mvW, mvH, kind = (c[k] for k in ("W", "H", "rX", "rY", "rAgg", "mvW", "mvH", "kind"))
    P1, P2, diag, passes, adaptive, sub = (c[k] for k in ("P1", "P2", "diag", "passes", "adaptive", "sub"))
    I1, I2 = synth.image_pair(W, H, 16, seed=seed)
    I1 = (I1.astype(np.int32) * 3 % 256).astype(np.uint8)
    mv = synth.hint_map(mvW, mvH, kind, seed=seed, amp=c["amp"])
    bd, mc, ms, Cv, S = oracle.calc_pyd_cost_sgm(I1, I2, mv, rX, rY, rAgg, sub, P1, P2, diag, passes, adaptive, want_volumes=True)
    with PydPlan(W, H, mvW, mvH, rX, rY, rAgg) as plan:
        plan.set_params(P1, P2, diag, passes, adaptive, sub)
        plan.upload(0, I1, I2, mv)
        plan.run(STAGE_ALL)
        msg = f"seed {seed} W{W} H{H} r{rX},{rY},{rAgg} {kind} P{P1},{P2} diag{diag} passes{passes} ad{adaptive}"
        np.testing.assert_array_equal(plan.download_cost(0), Cv, err_msg=msg)
        np.testing.assert_array_equal(plan.download_sum(0), S, err_msg=msg)
        gbd, gmc, gms = plan.download(0)
    np.testing.assert_array_equal(gbd, bd, err_msg=msg)
    np.testing.assert_array_equal(gmc, mc, err_msg=msg)
    np.testing.assert_array_equal(gms, ms, err_msg=msg)


@pytest.mark.parametrize("seed", _seeds(16))
def test_ng_random_configs(gpu_lib, oracle, seed):
    c = fuzz_configs.ng_config(seed)
    W, H, mvW, mvH, P1, P2, half, agg, sub, kind, amp = (c[k] for k in ("W", "H", "mvW", "mvH", "P1", "P2", "half", "agg", "sub", "kind", "amp"))
    I1, I2 = synth.image_pair(W, H, 16, seed=seed + 50)
    mv = synth.hint_map(mvW, mvH, kind, seed=seed, amp=amp)
    mc, fl, _, S = oracle.calc_pyd_cost_sgm_ng(I1, I2, mv, half, agg, sub, P1, P2, want_volumes=True)
    gmc, gfl, gS = calc_pyd_cost_sgm_ng(I1, I2, mv, half, agg, sub, P1, P2, return_sum=True)
    msg = f"seed {seed} W{W} H{H} mv{mvW}x{mvH} half{half} agg{agg} P{P1},{P2} {kind} amp{amp}"
    np.testing.assert_array_equal(gS, S, err_msg=msg)
    np.testing.assert_array_equal(gmc, mc, err_msg=msg)
    np.testing.assert_array_equal(gfl, fl, err_msg=msg)
    W2, H2 = min(W, 24), min(H, 16)
    I1, I2 = np.ascontiguousarray(I1[:H2, :W2]), np.ascontiguousarray(I2[:H2, :W2])
    rs = oracle.glibc_rand_stream(oracle.sgm_ng_rand_draws(W2, H2), seed=seed + 1)
    mc, fl = oracle.calc_cost_sgm_ng(I1, I2, P1, P2, rs)
    gmc, gfl = calc_cost_sgm_ng(I1, I2, None, 1, 2, 0, P1, P2, rand_stream=rs)
    np.testing.assert_array_equal(gmc, mc, err_msg=msg)
    np.testing.assert_array_equal(gfl, fl, err_msg=msg)
