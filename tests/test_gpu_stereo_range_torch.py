"""GPU tests of torch_ops.stereo_sgm(..., d_min=) / fsgm::stereo_sgm_range: the op on CUDA tensors equals the numpy path, outputs
are int32 and stay on the device, a non-default stream works, host memory is refused before anything is queued."""
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


@pytest.mark.parametrize("fb,d_min,direction", [(0, -17, -1), (1, 7, +1), (1, 0, -1)])
def test_torch_stereo_range_equals_the_numpy_path(gpu_lib, fb, d_min, direction):
    W, H, D, n = 61, 17, 32, 3
    pairs = [synth.image_pair(W, H, D, seed=20 + f) for f in range(n)]
    L, Rt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    tL, tR = _t(L), _t(Rt)
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # a non-default stream
        outs = torch_ops.stereo_sgm(tL, tR, D, paths=8, direction=direction, fb_check=fb, d_min=d_min, return_status=True)
    side.synchronize()
    assert int(outs[-1].item()) == 0
    assert all(o.is_cuda and o.shape == (n, H, W) for o in outs[:-1])
    dtypes = [torch.int32, torch.uint32] + ([torch.uint8, torch.int32] if fb else [])
    assert [o.dtype for o in outs[:-1]] == dtypes
    want = fsgm_amd.stereo_sgm(L, Rt, D, paths=8, direction=direction, fb_check=fb, d_min=d_min)
    for f in range(n):
        one = torch_ops.stereo_sgm(tL[f], tR[f], D, paths=8, direction=direction, fb_check=fb, d_min=d_min, check=True)
        for k in range(len(want)):
            assert one[k].is_cuda and one[k].shape == (H, W) and one[k].dtype == dtypes[k]
            _eq(outs[k][f].cpu().numpy(), one[k].cpu().numpy(), f"output {k} of frame {f}: batch vs single")
            _eq(outs[k][f].cpu().numpy(), want[k][f], f"output {k} of frame {f}: torch vs host entry point")
    # the op without d_min on the same shape afterwards: the uint32 outputs it always had
    old = torch_ops.stereo_sgm(tL, tR, D, paths=8, direction=direction, fb_check=fb, check=True)
    ref = fsgm_amd.stereo_sgm(L, Rt, D, paths=8, direction=direction, fb_check=fb)
    assert old[0].dtype == torch.uint32
    for k in range(len(ref)):
        _eq(old[k].cpu().numpy(), ref[k], f"output {k} without d_min")


def test_range_device_entry_point_refuses_host_memory_before_anything_is_queued(gpu_lib):
    W, H, D = 24, 9, 16
    I1, I2 = synth.image_pair(W, H, D)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.stereo_sgm(torch.from_numpy(I1), _t(I2), D, d_min=3)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.stereo_sgm(_t(I1), torch.from_numpy(I2), D, d_min=3)
    pinned = torch.from_numpy(I1).pin_memory()
    dI1, dI2 = _t(I1), _t(I2)
    disp, minC = torch.full((H, W), 7, dtype=torch.int32, device="cuda:0"), torch.full((H, W), 7, dtype=torch.int32, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    st = gpu_lib.fsgm_stereo_sgm_device_range(1, p(pinned), p(dI2), W, H, D, 6, 64, None, None, 3, p(disp), p(minC), None, None, None, None)
    assert st == FSGM_ERR_INVALID
    st = gpu_lib.fsgm_stereo_sgm_device_range(1, p(dI1), p(dI2), W, H, D, 6, 64, None, None, 1025, p(disp), p(minC), None, None, None, None)
    assert st == FSGM_ERR_INVALID and b"d_min" in gpu_lib.fsgm_last_error()
    torch.cuda.synchronize()
    assert bool((disp == 7).all()) and bool((minC == 7).all())
