"""GPU tests of adaptive_p2 through the torch ops: device tensors in, device tensors out, equal to the host entry points and to
the restatement; a batch of three frames with images of their own (a wrong frame stride of the pixel loads would show)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth  # noqa: E402  (torch first, then the library)
from tests import adaptive_p2_restatement as A  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _eq(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"{what}: output {k}")


W, H, D, N = 37, 19, 32, 3
PAIRS = [synth.image_pair(W, H, D, seed=40 + f) for f in range(N)]
MAPS = [synth.epi_maps(W, H, "general", seed=50 + f) for f in range(N)]


@pytest.mark.parametrize("paths", [4, 8])
def test_torch_calc_cost_sgm_adaptive_batch(gpu_lib, paths):
    args = [_t(np.stack(x)) for x in ([p[0] for p in PAIRS], [p[1] for p in PAIRS], [m[0] for m in MAPS], [m[1] for m in MAPS], [m[2] for m in MAPS])]
    outs = torch_ops.calc_cost_sgm(args[0], args[1], D, 0.3, args[2], args[3], args[4], 6, 64, paths=paths, adaptive_p2=1, check=True)
    assert all(o.is_cuda and o.shape == (N, H, W) for o in outs)
    plain = torch_ops.calc_cost_sgm(args[0], args[1], D, 0.3, args[2], args[3], args[4], 6, 64, paths=paths, check=True)
    assert (outs[1].cpu().numpy() != plain[1].cpu().numpy()).any()   # the switch does something on these frames
    for f in range(N):
        host = fsgm_amd.calc_cost_sgm(*PAIRS[f], D, 0.3, *MAPS[f], 6, 64, paths=paths, adaptive_p2=1)
        _eq([o[f] for o in outs], host, f"frame {f} against the host call")
        _eq([o[f] for o in outs], A.calc_cost_sgm(*PAIRS[f], D, 0.3, *MAPS[f], 6, 64, paths=paths, adaptive=1), f"frame {f} against the restatement")
        _eq([o[f] for o in plain], fsgm_amd.calc_cost_sgm(*PAIRS[f], D, 0.3, *MAPS[f], 6, 64, paths=paths), f"frame {f}, adaptive off")


def test_torch_linear_and_stereo_adaptive_batch(gpu_lib):
    L, R = np.stack([p[0] for p in PAIRS]), np.stack([p[1] for p in PAIRS])
    pd0, nd = fsgm_amd.stereo_maps(W, H)
    st = torch_ops.stereo_sgm(_t(L), _t(R), D, paths=8, adaptive_p2=1, fb_check=1, check=True)
    _eq(st, fsgm_amd.stereo_sgm(L, R, D, paths=8, adaptive_p2=1, fb_check=1), "stereo against the host call")
    ln = torch_ops.calc_cost_sgm_linear(_t(L), _t(R), D, _t(np.stack([pd0] * N)), _t(np.stack([nd] * N)), 6, 64, paths=8, adaptive_p2=1, check=True)
    _eq(ln, [o.cpu().numpy() for o in st[:2]], "linear against stereo")
    for f in range(N):
        _eq([o[f] for o in ln], A.calc_cost_sgm_linear(*PAIRS[f], D, pd0, nd, 6, 64, paths=8, adaptive=1), f"frame {f} against the restatement")
    one = torch.ops.fsgm.stereo_sgm(_t(L), _t(R), D, 6, 64, 8, 1, -1, 0)                       # the schema's default: adaptive off
    _eq(one[:2], fsgm_amd.stereo_sgm(L, R, D, paths=8), "nine positional arguments as before")
    with pytest.raises(ValueError, match="adaptive_p2"):
        torch_ops.stereo_sgm(_t(L), _t(R), D, adaptive_p2=3)
