"""Footprint of the device-pointer entries of the second view (fsgm_sgm_view2_dptr, fsgm_stereo_sgm_view2_dptr,
fsgm_view2_check_dptr): the check of tests/test_gpu_footprint.py -- same results, no stray write, no stray read, fully written --
with every tensor carved from the guarded arenas of tests/footprint.py.  Their names end in _dptr, so the table of *_device*
entries does not list them; this file is their coverage."""
import numpy as np
import pytest

import torch  # noqa: I001 -- before the library
from fsgm_amd import torch_ops, synth  # noqa: E402
from tests import footprint as F  # noqa: E402
from tests import test_gpu_footprint as FP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRIES = ("fsgm_sgm_view2_dptr", "fsgm_stereo_sgm_view2_dptr", "fsgm_view2_check_dptr")
CASES = []


def case(entry, ident):
    def deco(fn):
        CASES.append(pytest.param(entry, fn, id=f"{entry}-{ident}"))
        return fn
    return deco


def _sgm_case(ident, W, H, D, n, layout, *, P=(7, 100), bound=255, adaptive=0, **kw):
    @case(ENTRIES[0], ident)
    def fn(ctx):
        v = np.stack([synth.cost_volume(W, H, D, 3 + W + D + 13 * f, bound) for f in range(n)])
        Cv = torch.from_numpy(v if layout == "hwd" else np.ascontiguousarray(v.transpose(0, 3, 1, 2))).to(DEV)
        guide = torch.from_numpy(np.stack([synth.uniform_u8(5 + f, (H, W)) for f in range(n)])).to(DEV) if adaptive else None
        outs = torch_ops.sgm(Cv, *P, layout=layout, cost_bound=bound, adaptive_p2=adaptive, guide=guide, return_sum=True, return_status=True,
                             second_view=True, **kw)
        names = ("bestD", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("S", "disp2", "minC_v2", "conf", "status")
        return dict(inputs={"C": Cv, **({"guide": guide} if adaptive else {})}, outputs=dict(zip(names, outs)))


_sgm_case("dhw-D16-tile256", 259, 3, 16, 2, "dhw", paths=8, d_min=5)
_sgm_case("hwd-D48-runner-up", 65, 11, 48, 1, "hwd", runner_up=True, direction=1, d_min=-3)
_sgm_case("dhw-D144-exact-guide", 67, 3, 144, 1, "dhw", arith="exact", adaptive=1)
_sgm_case("hwd-D21-bytes-one-column", 1, 11, 21, 3, "hwd")
_sgm_case("dhw-D272-generic", 37, 3, 272, 1, "dhw", direction=1, d_min=5)


def _stereo_case(ident, W, H, n, D, **kw):
    @case(ENTRIES[1], ident)
    def fn(ctx):
        pairs = [synth.image_pair(W, H, D, seed=7 + f) for f in range(n)]
        a = torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV)
        b = torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV)
        outs = torch_ops.stereo_sgm(a, b, D, 6, 64, second_view=True, return_status=True, **kw)
        names = ("disp", "minC") + (("minC2",) if kw.get("runner_up") else ()) + ("disp2", "minC_v2", "conf", "status")
        return dict(inputs={"I1": a, "I2": b}, outputs=dict(zip(names, outs)))


_stereo_case("61x47x2-D24", 61, 47, 2, 24, paths=8, d_min=-3)
_stereo_case("37x11x1-D40-runner-up", 37, 11, 1, 40, runner_up=True, direction=1, d_min=5)


def _check_case(ident, W, H, n, direction):
    @case(ENTRIES[2], ident)
    def fn(ctx):
        rng = np.random.default_rng(W + H)
        d1 = torch.from_numpy(rng.integers(-2000, 6000, (n, H, W)).astype(np.int32)).to(DEV)
        d2v = rng.integers(-2000, 6000, (n, H, W)).astype(np.int32)
        d2v[rng.random((n, H, W)) < 0.2] = -2 ** 31
        d2 = torch.from_numpy(d2v).to(DEV)
        conf, status = torch.ops.fsgm_view2.check(d1, d2, direction, 700)
        return dict(inputs={"disp": d1, "disp2": d2}, outputs={"conf": conf, "status": status})


_check_case("37x11x3", 37, 11, 3, -1)
_check_case("1x5x1", 1, 5, 1, 1)

assert sorted({p.values[0] for p in CASES}) == sorted(ENTRIES)


@pytest.mark.parametrize("placement", F.PLACEMENTS)
@pytest.mark.parametrize("entry,fn", CASES)
def test_footprint_view2(gpu_lib, entry, fn, placement):
    FP.test_footprint(gpu_lib, entry, fn, placement)
