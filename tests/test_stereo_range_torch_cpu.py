"""CPU tests of torch_ops.stereo_sgm's d_min: validation before a device is touched, the fake-tensor form of fsgm::stereo_sgm_range
(int32 disparities), and the unchanged schema of fsgm::stereo_sgm."""
import inspect

import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)


def test_torch_wrapper_accepts_d_min_and_returns_int32():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert inspect.signature(torch_ops.stereo_sgm).parameters["d_min"].default is None
    with FakeTensorMode():
        for lead in ((), (3,)):
            L = torch.empty(lead + (8, 12), dtype=torch.uint8, device="cuda")
            with pytest.raises(ValueError, match="d_min"):
                torch_ops.stereo_sgm(L, L, 16, d_min=2000)
            r = torch_ops.stereo_sgm(L, L, 16, d_min=0, return_status=True)                  # the dtype follows the argument, not its value
            assert [(tuple(t.shape), t.dtype) for t in r] == [(lead + (8, 12), torch.int32), (lead + (8, 12), torch.uint32), ((), torch.int32)]
            r = torch_ops.stereo_sgm(L, L, 16, d_min=-40, fb_check=1)
            assert [(tuple(t.shape), t.dtype) for t in r] == [(lead + (8, 12), t) for t in (torch.int32, torch.uint32, torch.uint8, torch.int32)]
            r = torch_ops.stereo_sgm(L, L, 16, fb_check=1)                                    # None: the outputs this op always had
            assert [(tuple(t.shape), t.dtype) for t in r] == [(lead + (8, 12), t) for t in (torch.uint32, torch.uint32, torch.uint8, torch.uint32)]
    # the schema of fsgm::stereo_sgm is what it was
    assert str(torch.ops.fsgm.stereo_sgm.default._schema) == (
        "fsgm::stereo_sgm(Tensor left, Tensor right, SymInt dMax, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, SymInt direction, "
        "SymInt fb_check, SymInt adaptive_p2=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
