"""CPU-side tests of the batched post-processing chain and test.m's frame body (fsgm_epi_postprocess_batch_host,
fsgm_epi_postprocess_device, fsgm_vmf_device, fsgm_epipolar_flow_pp_*): the torch ops' fake implementations and the C entry
points' argument checks, which all answer before any device is touched."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
from fsgm_amd import _lib  # noqa: E402
from fsgm_amd.epi import EpiGeometry, _params, _bind_driver  # noqa: E402

FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below fails its argument checks first
W, H = 83, 47


def _fake_mode():
    from torch._subclasses.fake_tensor import FakeTensorMode
    return FakeTensorMode()


def _meta(ts):
    return [(tuple(t.shape), t.dtype, t.device.type) for t in ts]


def _err(lib):
    return lib.fsgm_last_error().decode()


@pytest.mark.parametrize("N", [None, 5])
def test_fake_epi_postprocess(N):
    lead = () if N is None else (N,)
    with _fake_mode():
        D1 = torch.empty(lead + (H, W), dtype=torch.float64, device="cuda")
        m = torch.empty(lead + (2, H, W), dtype=torch.float64, device="cuda")
        r = torch_ops.epi_postprocess(D1, m, m, D1, 0.3, 65, 64, return_status=True)
        assert _meta(r) == [(lead + (H, W), torch.float64, "cuda")] * 3 + [((), torch.int32, "cuda")]
        r = torch_ops.epi_postprocess(D1, m, m, D1, 0.3, 65, 64)
        assert len(r) == 3
        n = N or 1
        raw = torch.ops.fsgm.epi_postprocess(D1.reshape(n, H, W), m.reshape(n, 2, H, W), m.reshape(n, 2, H, W), D1.reshape(n, H, W),
                                             0.3, 65.0, 64.0)
        assert _meta(raw) == [((n, H, W), torch.float64, "cuda")] * 3 + [((), torch.int32, "cuda")]


@pytest.mark.parametrize("lead", [(), (4,)])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_fake_vmf(lead, ch):
    with _fake_mode():
        flow = torch.empty(lead + (ch, H, W), dtype=torch.float64, device="cuda")
        assert _meta([torch_ops.vmf(flow)]) == [(lead + (ch, H, W), torch.float64, "cuda")]
        assert _meta([torch.ops.fsgm.vmf(flow.reshape(-1, ch, H, W))]) == [((lead or (1,)) + (ch, H, W), torch.float64, "cuda")]


@pytest.mark.parametrize("N", [None, 3])
@pytest.mark.parametrize("rgb", [False, True])
def test_fake_epipolar_flow_pp(N, rgb):
    lead = () if N is None else (N,)
    planes = (3,) if rgb else ()
    F, Hm = np.eye(3), np.eye(3)
    geo = (F, Hm, (40.0, 20.0), 0) if N is None else ([F] * N, [Hm] * N, [(40.0, 20.0)] * N, [0] * N)
    with _fake_mode():
        I = torch.empty(lead + planes + (H, W), dtype=torch.uint8, device="cuda")
        r = torch_ops.epipolar_flow_pp(I, I, *geo, return_status=True)
        assert _meta(r) == [(lead + (3, H, W), torch.float64, "cuda")] * 2 + [(lead + (H, W), torch.float64, "cuda"),
                                                                             (lead + (H, W), torch.uint32, "cuda"), ((), torch.int32, "cuda")]


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    D1 = torch.zeros((H, W), dtype=torch.float64)
    m = torch.zeros((2, H, W), dtype=torch.float64)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.epi_postprocess(D1, m, m, D1, 0.3, 65, 64)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.vmf(m)
    with _fake_mode():
        g = torch.empty((H, W), dtype=torch.float64, device="cuda")
        gm = torch.empty((2, H, W), dtype=torch.float64, device="cuda")
        with pytest.raises(TypeError, match="shape"):
            torch_ops.epi_postprocess(g, gm[0], gm, g, 0.3, 65, 64)
        with pytest.raises(TypeError, match="float64"):
            torch_ops.epi_postprocess(g.float(), gm, gm, g, 0.3, 65, 64)
        with pytest.raises(TypeError, match="1..3"):
            torch_ops.vmf(torch.empty((4, H, W), dtype=torch.float64, device="cuda"))


# ---- the C entry points' argument checks: they answer before any device or pointer query ----
def _post_args(n=1, Wd=W, Hd=H, D1=FAKE, f1=FAKE):
    return (n, D1, Wd, Hd, FAKE, FAKE, FAKE, 0.3, 65.0, 64.0, f1, None, None, 0)


def test_postprocess_batch_argument_checks():
    lib = _lib.load()
    dev_tail = (None, None)                                     # stream, status of the device form
    for fn, tail in ((lib.fsgm_epi_postprocess_batch_host, ()), (lib.fsgm_epi_postprocess_device, dev_tail)):
        assert fn(*_post_args(n=0), *tail) == FSGM_ERR_INVALID and "n_frames" in _err(lib)
        assert fn(*_post_args(D1=None), *tail) == FSGM_ERR_INVALID and "null argument" in _err(lib)
        assert fn(*_post_args(f1=None), *tail) == FSGM_ERR_INVALID and "null argument" in _err(lib)
        assert fn(*_post_args(Wd=0), *tail) == FSGM_ERR_INVALID and "width/height" in _err(lib)
        assert fn(*_post_args(n=2, Wd=40000, Hd=30000), *tail) == FSGM_ERR_UNSUPPORTED and "2^31" in _err(lib)
        assert fn(*_post_args(n=16, Wd=4096, Hd=32768), *tail) == FSGM_ERR_UNSUPPORTED     # exactly 2^31
    vmf = lib.fsgm_vmf_device
    assert vmf(0, FAKE, W, H, 3, FAKE, 0, None) == FSGM_ERR_INVALID and "n_frames" in _err(lib)
    assert vmf(1, None, W, H, 3, FAKE, 0, None) == FSGM_ERR_INVALID and "null argument" in _err(lib)
    assert vmf(1, FAKE, W, H, 3, None, 0, None) == FSGM_ERR_INVALID and "null argument" in _err(lib)
    assert vmf(1, FAKE, W, H, 4, FAKE, 0, None) == FSGM_ERR_INVALID and "channels" in _err(lib)
    assert vmf(1, FAKE, W, H, 0, FAKE, 0, None) == FSGM_ERR_INVALID and "channels" in _err(lib)
    assert vmf(3, FAKE, 32768, 32768, 1, FAKE, 0, None) == FSGM_ERR_UNSUPPORTED and "2^31" in _err(lib)


def test_flow_pp_argument_checks():
    lib = _lib.load()
    _bind_driver(lib)
    g = (EpiGeometry * 4)()
    fb = _params(4, 1, 0, 0, 1)

    def args(n=1, ch=1, Wd=W, Hd=H, D=64, prm=None, flow=FAKE, flow2=FAKE, geo=g):
        return (n, FAKE, FAKE, Wd, Hd, ch, geo, D, 0.3, None if prm is None else C.byref(prm), flow, flow2, None, None)

    for fn, tail in ((lib.fsgm_epipolar_flow_pp_host, ()), (lib.fsgm_epipolar_flow_pp_device, (None, None))):
        assert fn(*args(n=0), *tail) == FSGM_ERR_INVALID and "n_frames" in _err(lib)
        assert fn(*args(ch=2), *tail) == FSGM_ERR_INVALID and "channels" in _err(lib)
        assert fn(*args(flow=None), *tail) == FSGM_ERR_INVALID and "null argument" in _err(lib)
        assert fn(*args(flow2=None), *tail) == FSGM_ERR_INVALID and "null argument" in _err(lib)
        assert fn(*args(geo=None), *tail) == FSGM_ERR_INVALID and "null argument" in _err(lib)
        assert fn(*args(Wd=0), *tail) == FSGM_ERR_INVALID and "width/height" in _err(lib)
        assert fn(*args(D=0), *tail) == FSGM_ERR_INVALID and "dMax" in _err(lib)
        assert fn(*args(prm=fb), *tail) == FSGM_ERR_INVALID and "fb_check" in _err(lib)
        assert fn(*args(n=3, Wd=32768, Hd=32768), *tail) == FSGM_ERR_UNSUPPORTED and "2^31" in _err(lib)
