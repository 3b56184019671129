"""Footprint of the four float device-pointer entries (fsgm_sgm_float_dptr, fsgm_sgm2d_float_dptr and the two float plan
ingests): the check of tests/test_gpu_footprint.py -- same results, no stray write, no stray read, fully written -- on float
volumes carved from the guarded arenas of tests/footprint.py.  The `minimal` placement starts a tensor on its element size and
not on twice that: a float32 volume at 4 mod 8, a 16-bit one at 2 mod 4, which is all the entries' check tables ask of C.  The
guards of the second arena hold 0xFF bytes -- NaN in each of the three types, which would raise the ingest flag and change the
status word: a load beyond the volume's last element is seen."""
import numpy as np
import pytest

import torch  # noqa: I001 -- before the library
from fsgm_amd import torch_ops, synth, EpiPlan, PydPlan  # noqa: E402
from tests import footprint as F  # noqa: E402
from tests import test_gpu_footprint as FP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRIES = ("fsgm_epi_plan_ingest_float_dptr", "fsgm_pyd_plan_ingest_float_dptr", "fsgm_sgm2d_float_dptr", "fsgm_sgm_float_dptr")
CASES = []


def case(entry, ident):
    def deco(fn):
        CASES.append(pytest.param(entry, fn, id=f"{entry}-{ident}"))
        return fn
    return deco


def _float_volumes(W, H, D, n, seed, cmax, dtype, dhw):
    """x = 2 v (+ 0.25 where the type holds it) for bytes v <= cmax: with scale 0.5 every voxel quantises to v, none is flagged"""
    v = np.stack([synth.cost_volume(W, H, D, seed + 13 * f, cmax) for f in range(n)]).astype(np.float32) * 2
    if dtype != torch.bfloat16:
        v += 0.25
    t = torch.from_numpy(v).to(dtype)
    return (t.permute(0, 3, 1, 2) if dhw else t).contiguous().to(DEV)


def _guide(n, H, W):
    return torch.from_numpy(np.stack([synth.uniform_u8(5 + f, (H, W)) for f in range(n)])).to(DEV)


def _sgm_case(ident, W, H, D, n, layout, dtype, *, P=(7, 100), bound=255, adaptive=0, **kw):
    @case("fsgm_sgm_float_dptr", ident)
    def fn(ctx):
        Cv = _float_volumes(W, H, D, n, 3 + W + D, bound, dtype, layout == "dhw")
        guide = _guide(n, H, W) if adaptive else None
        outs = torch_ops.sgm_float(Cv, 0.5, 0.0, *P, layout=layout, cost_bound=bound, adaptive_p2=adaptive, guide=guide, return_sum=True,
                                   return_status=True, **kw)
        names = ("bestD", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("S", "status")
        return dict(inputs={"C": Cv, **({"guide": guide} if adaptive else {})}, outputs=dict(zip(names, outs)))


_sgm_case("f32-dhw-D16", 37, 11, 16, 3, "dhw", torch.float32, paths=8)
_sgm_case("f16-dhw-D48-exact-guide", 65, 11, 48, 1, "dhw", torch.float16, arith="exact", adaptive=1)
_sgm_case("bf16-hwd-D24-runner-up", 37, 1, 24, 3, "hwd", torch.bfloat16, runner_up=True)
_sgm_case("f32-hwd-D21-one-column", 1, 11, 21, 1, "hwd", torch.float32)
_sgm_case("f16-dhw-D16-sweeps", 37, 11, 16, 3, "dhw", torch.float16, P=(6, 32), paths=8, bound=24, agg_mode=2)


def _sgm2d_case(ident, W, H, rX, rY, n, layout, dtype, *, bound=24, hints=True, adaptive=0, **kw):
    @case("fsgm_sgm2d_float_dptr", ident)
    def fn(ctx):
        Sx, Sy = 2 * rX + 1, 2 * rY + 1
        Cv = _float_volumes(W, H, Sx * Sy, n, 3 + rX, bound, dtype, layout != "hwd")
        hm = (torch.from_numpy(np.stack([synth.hint_map(W + 3, H + 3, "general", seed=40 + 5 * f, amp=3.0) for f in range(n)])).to(DEV)
              if hints else None)
        guide = _guide(n, H, W) if adaptive else None
        outs = torch_ops.sgm2d_float(Cv, rX, rY, 0.5, 0.0, 6, 32, layout=layout, hints=hm, guide=guide, cost_bound=bound, adaptive_p2=adaptive,
                                     return_flow=True, return_sum=True, return_status=True, **kw)
        names = ("bestD", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("mvSub", "flow", "S", "status")
        ins = {"C": Cv, **({"preMv": hm} if hints else {}), **({"guide": guide} if adaptive else {})}
        return dict(inputs=ins, outputs=dict(zip(names, outs)))


_sgm2d_case("f32-dhw_yx-3x5-hints", 37, 11, 1, 2, 3, "dhw_yx", torch.float32)
_sgm2d_case("bf16-hwd-3x5-padded-rows-exact-ru", 37, 11, 1, 2, 3, "hwd", torch.bfloat16, adaptive=1, runner_up=True, arith="exact")
_sgm2d_case("f16-hwd-13x9-guide", 65, 11, 6, 4, 1, "hwd", torch.float16, hints=False, adaptive=1)
_sgm2d_case("f16-dhw-5x3-one-row", 37, 1, 2, 1, 3, "dhw", torch.float16, bound=255, runner_up=True)


def _ingest_case(entry, ident, make_plan, ingest, D, layout, dtype):
    @case(entry, ident)
    def fn(ctx):
        plan = ctx.enter_context(make_plan())
        n, H, W = plan.batch, plan.H, plan.W
        Cv = _float_volumes(W, H, D, n, 9, 255, dtype, layout != "hwd")
        zero = torch.zeros_like(Cv)
        status = ingest(plan, Cv, 0.5, 0.0, layout=layout, cost_bound=255, return_status=True)

        def probe():
            torch.cuda.synchronize()
            return np.stack([plan.download_cost(f) for f in range(n)])

        def reset():                                              # the plan's volumes hold something else before each replay
            ingest(plan, zero, 0.5, 0.0, layout=layout, cost_bound=255, check=True)
            assert not probe().any()
        return dict(inputs={"C": Cv}, outputs={"status": status}, opaque=[plan._h.value], probe=probe, reset=reset)


_ingest_case(ENTRIES[0], "f16-D48-dhw", lambda: EpiPlan(37, 11, 48, 3, vz_to_disp=0), torch_ops.ingest_cost_float, 48, "dhw", torch.float16)
_ingest_case(ENTRIES[0], "f32-D17-hwd", lambda: EpiPlan(65, 1, 17, 1, vz_to_disp=0), torch_ops.ingest_cost_float, 17, "hwd", torch.float32)
_ingest_case(ENTRIES[0], "bf16-D21-dhw", lambda: EpiPlan(130, 3, 21, 1, vz_to_disp=0), torch_ops.ingest_cost_float, 21, "dhw", torch.bfloat16)
_ingest_case(ENTRIES[1], "bf16-3x5-dhw_yx", lambda: PydPlan(37, 11, 37, 11, 1, 2, 0, batch=3), torch_ops.ingest_cost2d_float, 15, "dhw_yx",
             torch.bfloat16)
_ingest_case(ENTRIES[1], "f32-3x5-hwd-padded-rows", lambda: PydPlan(37, 11, 37, 11, 1, 2, 0, batch=3), torch_ops.ingest_cost2d_float, 15, "hwd",
             torch.float32)
_ingest_case(ENTRIES[1], "f16-13x9-hwd", lambda: PydPlan(65, 1, 65, 1, 6, 4, 0, batch=1), torch_ops.ingest_cost2d_float, 117, "hwd",
             torch.float16)

assert sorted({p.values[0] for p in CASES}) == sorted(ENTRIES)


def test_the_minimal_placement_is_the_element_size():
    """what the float volumes' check-table rows ask for (their `align` is the element-size expression) is what the arena gives"""
    for esize in (2, 4):
        s = F.place(65536, 1000 * esize, esize, "minimal")
        assert s % esize == 0 and s % (2 * esize) != 0


@pytest.mark.parametrize("placement", F.PLACEMENTS)
@pytest.mark.parametrize("entry,fn", CASES)
def test_footprint_float(gpu_lib, entry, fn, placement):
    FP.test_footprint(gpu_lib, entry, fn, placement)
