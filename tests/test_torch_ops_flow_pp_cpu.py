"""Fake-tensor shapes and dtypes of the filtered-flow torch ops (no GPU)."""
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)


def _fake_mode():
    from torch._subclasses.fake_tensor import FakeTensorMode
    return FakeTensorMode()


def _meta(ts):
    return [(tuple(t.shape), t.dtype, t.device.type) for t in ts]


@pytest.mark.parametrize("N", [None, 4])
@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("matcher", ["pyd", "ng"])
def test_fake_pyramidal_flow_pp(N, rgb, matcher):
    lead = () if N is None else (N,)
    with _fake_mode():
        I = torch.empty(lead + ((3,) if rgb else ()) + (47, 83), dtype=torch.uint8, device="cuda")
        r = torch_ops.pyramidal_flow_pp(I, I, 3, matcher, batch=N is not None, return_status=True, fb_thr=1.5, P2=40)
        f2 = (lead + (2, 47, 83), torch.float64, "cuda")
        assert _meta(r) == [(lead + (3, 47, 83), torch.float64, "cuda"), f2, f2, f2, (lead + (47, 83), torch.uint32, "cuda"),
                            ((), torch.int32, "cuda")]
        with pytest.raises(TypeError, match="unknown"):
            torch_ops.pyramidal_flow_pp(I, I, 3, matcher, batch=N is not None, no_such_parameter=1)
        with pytest.raises(ValueError, match="matcher"):
            torch_ops.pyramidal_flow_pp(I, I, 3, "census")


@pytest.mark.parametrize("N", [None, 4])
def test_fake_flow_fb_check(N):
    lead = () if N is None else (N,)
    with _fake_mode():
        f = torch.empty(lead + (2, 47, 83), dtype=torch.float64, device="cuda")
        assert _meta([torch_ops.flow_fb_check(f, f, 2.0)]) == [(lead + (2, 47, 83), torch.float64, "cuda")]
        with pytest.raises(TypeError, match="shape"):
            torch_ops.flow_fb_check(f, f[..., :8])
        with pytest.raises(TypeError, match="float64"):
            torch_ops.flow_fb_check(f, f.float())


def test_flow_ops_refuse_cpu_tensors():
    f = torch.zeros((2, 4, 5), dtype=torch.float64)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.flow_fb_check(f, f)
    I = torch.zeros((4, 5), dtype=torch.uint8)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.pyramidal_flow_pp(I, I, 3)
