"""GPU tests of torch_ops.stereo_sgm and torch_ops.calc_cost_sgm_linear: a batch equals frame by frame and the host entry
points, outputs stay on the device, a non-default stream works, host memory is refused before anything is queued."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth  # noqa: E402  (torch first, then the library)

pytestmark = pytest.mark.gpu
FSGM_ERR_INVALID = 1


def _eq(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("fb", [0, 1])
def test_torch_stereo_sgm_batch_equals_frame_by_frame(gpu_lib, fb):
    W, H, D, n = 61, 17, 32, 3
    pairs = [synth.image_pair(W, H, D, seed=20 + f) for f in range(n)]
    L, Rt = _t(np.stack([p[0] for p in pairs])), _t(np.stack([p[1] for p in pairs]))
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # a non-default stream
        outs = torch_ops.stereo_sgm(L, Rt, D, paths=8, fb_check=fb, return_status=True)
    side.synchronize()
    assert int(outs[-1].item()) == 0
    assert all(o.is_cuda and o.shape == (n, H, W) for o in outs[:-1])
    want = fsgm_amd.stereo_sgm(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), D, paths=8, fb_check=fb)
    for f in range(n):
        one = torch_ops.stereo_sgm(L[f], Rt[f], D, paths=8, fb_check=fb, check=True)
        for k in range(len(want)):
            assert one[k].is_cuda and one[k].shape == (H, W)
            _eq(outs[k][f].cpu().numpy(), one[k].cpu().numpy(), f"output {k} of frame {f}: batch vs single")
            _eq(outs[k][f].cpu().numpy(), want[k][f], f"output {k} of frame {f}: torch vs host entry point")


def test_torch_calc_cost_sgm_linear_matches_the_host_entry_point(gpu_lib):
    W, H, D, n = 47, 13, 16, 3
    pairs = [synth.image_pair(W, H, D, seed=30 + f) for f in range(n)]
    maps = [synth.epi_maps(W, H, "general", seed=40 + f)[:2] for f in range(n)]
    want = fsgm_amd.calc_cost_sgm_linear_batch([p + m for p, m in zip(pairs, maps)], D, 6, 64, fb_check=1)
    args = [_t(np.stack([p[k] for p in pairs])) for k in range(2)] + [_t(np.stack([m[k] for m in maps])) for k in range(2)]
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = torch_ops.calc_cost_sgm_linear(args[0], args[1], D, args[2], args[3], 6, 64, fb_check=1, check=True)
    assert all(g.is_cuda for g in got)
    for f in range(n):
        one = torch_ops.calc_cost_sgm_linear(args[0][f], args[1][f], D, args[2][f], args[3][f], 6, 64, fb_check=1, check=True)
        for k in range(4):
            _eq(got[k][f].cpu().numpy(), want[f][k], f"output {k} of frame {f}")
            _eq(one[k].cpu().numpy(), want[f][k], f"output {k} of frame {f}, single call")


def test_device_entry_points_refuse_host_memory_before_anything_is_queued(gpu_lib):
    W, H, D = 24, 9, 16
    I1, I2 = synth.image_pair(W, H, D)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.stereo_sgm(torch.from_numpy(I1), _t(I2), D)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.stereo_sgm(_t(I1), torch.from_numpy(I2), D)
    # the C entry point itself: a pinned host image is FSGM_ERR_INVALID and the output stays as it was
    pinned = torch.from_numpy(I1).pin_memory()
    dI2, disp, minC = _t(I2), torch.full((H, W), 7, dtype=torch.int32, device="cuda:0"), torch.full((H, W), 7, dtype=torch.int32, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    st = gpu_lib.fsgm_stereo_sgm_device(1, p(pinned), p(dI2), W, H, D, 6, 64, None, p(disp), p(minC), None, None, None, None)
    assert st == FSGM_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((disp == 7).all()) and bool((minC == 7).all())
