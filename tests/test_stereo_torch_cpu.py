"""CPU tests of the torch entry points of rectified stereo and of the linear build of calc_cost_sgm: argument validation, which
answers before a device is touched, and the ops' fake-tensor forms."""
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
from fsgm_amd import synth  # noqa: E402
import fsgm_amd  # noqa: E402


def test_torch_entry_points_validate_and_have_fake_forms():
    from torch._subclasses.fake_tensor import FakeTensorMode
    I1, I2 = (torch.from_numpy(a) for a in synth.image_pair(12, 8, 16))
    pd0, nd = (torch.from_numpy(a) for a in fsgm_amd.stereo_maps(12, 8))
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.stereo_sgm(I1, I2, 16)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.calc_cost_sgm_linear(I1, I2, 16, pd0, nd, 6, 64)
    with pytest.raises(TypeError):
        torch_ops.stereo_sgm(I1.numpy(), I2, 16)
    with FakeTensorMode():
        for lead in ((), (3,)):
            L = torch.empty(lead + (8, 12), dtype=torch.uint8, device="cuda")
            m = torch.empty(lead + (2, 8, 12), dtype=torch.float64, device="cuda")
            with pytest.raises(ValueError, match="direction"):
                torch_ops.stereo_sgm(L, L, 16, direction=2)
            with pytest.raises(TypeError):
                torch_ops.stereo_sgm(L, L[..., :-1], 16)
            with pytest.raises(TypeError):
                torch_ops.calc_cost_sgm_linear(L, L, 16, m[..., :1, :, :], m, 6, 64)
            r = torch_ops.stereo_sgm(L, L, 16, return_status=True)
            assert [(tuple(t.shape), t.dtype) for t in r] == [(lead + (8, 12), torch.uint32)] * 2 + [((), torch.int32)]
            r = torch_ops.stereo_sgm(L, L, 16, fb_check=1)
            assert [(tuple(t.shape), t.dtype) for t in r] == [(lead + (8, 12), t) for t in (torch.uint32, torch.uint32, torch.uint8, torch.uint32)]
            r = torch_ops.calc_cost_sgm_linear(L, L, 16, m, m, 6, 64, fb_check=1)
            assert [(tuple(t.shape), t.dtype) for t in r] == [(lead + (8, 12), t) for t in (torch.uint32, torch.uint32, torch.uint8, torch.uint32)]
