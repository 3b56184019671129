"""CPU-side tests of sgm(C) on caller-supplied volumes (fsgm_sgm_batch_host / fsgm_sgm_device, fsgm::sgm): every refusal that
needs no device, the parameter defaults, the ingest kernel's LDS request and the torch op's fake implementation."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
from fsgm_amd import _lib  # noqa: E402
from fsgm_amd.sgm import SgmParams, _bind, ingest_lds, last_kernel, sgm_batch  # noqa: E402

FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below fails its argument checks first


@pytest.fixture(scope="module")
def lib():
    return _bind(_lib.load())


def _err(lib):
    return lib.fsgm_last_error().decode()


def _host(lib, prm=None, n=1, Cp=FAKE, W=32, H=24, D=16, guide=None, bestD=FAKE, minC=FAKE):
    return lib.fsgm_sgm_batch_host(n, Cp, W, H, D, 7, 100, None if prm is None else C.byref(prm), guide, bestD, minC, None)


def _device(lib, prm=None, n=1, Cp=FAKE, W=32, H=24, D=16, guide=None, bestD=FAKE, minC=FAKE):
    return lib.fsgm_sgm_device(n, Cp, W, H, D, 7, 100, None if prm is None else C.byref(prm), guide, bestD, minC, None, None, None)


def test_params_default(lib):
    p = lib.fsgm_sgm_params_default()
    assert (p.paths, p.subpixel, p.device, p.agg_mode, p.layout, p.cost_bound, p.adaptive_p2) == (4, 1, 0, 0, 0, 255, 0)
    assert list(p.reserved) == [0] * 5
    assert C.sizeof(SgmParams) == 12 * 4


@pytest.mark.parametrize("call", [_host, _device], ids=["host", "device"])
def test_refusals_without_a_device(lib, call):
    bad = lambda **kw: call(lib, **kw)  # noqa: E731
    assert bad(n=0) == FSGM_ERR_INVALID and "n_frames" in _err(lib)
    assert bad(n=-3) == FSGM_ERR_INVALID and "n_frames" in _err(lib)
    for null in ("Cp", "bestD", "minC"):
        assert bad(**{null: None}) == FSGM_ERR_INVALID and "null argument" in _err(lib)
    assert bad(W=0) == FSGM_ERR_INVALID and "width/height" in _err(lib)
    assert bad(H=0) == FSGM_ERR_INVALID and "width/height" in _err(lib)
    for D in (0, -1, 1025):
        assert bad(D=D) == FSGM_ERR_INVALID and "dMax" in _err(lib)

    def prm(**kw):
        p = lib.fsgm_sgm_params_default()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    for layout in (-1, 2):
        assert bad(prm=prm(layout=layout)) == FSGM_ERR_INVALID and "layout" in _err(lib)
    for bound in (0, 256, -1):
        assert bad(prm=prm(cost_bound=bound)) == FSGM_ERR_INVALID and "cost_bound" in _err(lib)
    for paths in (0, 5, 16):
        assert bad(prm=prm(paths=paths)) == FSGM_ERR_INVALID and "paths" in _err(lib)
    for mode in (-1, 7):
        assert bad(prm=prm(agg_mode=mode)) == FSGM_ERR_INVALID and "agg_mode" in _err(lib)
    assert bad(prm=prm(adaptive_p2=2)) == FSGM_ERR_INVALID and "adaptive_p2" in _err(lib)
    assert bad(prm=prm(subpixel=2)) == FSGM_ERR_INVALID and "subpixel" in _err(lib)
    for slot in range(5):
        p = prm()
        p.reserved[slot] = 1
        assert bad(prm=p) == FSGM_ERR_INVALID and "reserved" in _err(lib)
    assert bad(prm=prm(adaptive_p2=1)) == FSGM_ERR_INVALID and "guide" in _err(lib)
    for mode in range(2, 7):
        assert bad(prm=prm(adaptive_p2=1, agg_mode=mode), guide=FAKE) == FSGM_ERR_UNSUPPORTED and "line kernels" in _err(lib)


def test_host_form_refuses_a_volume_above_its_bound_before_any_device(lib):
    """The scan of the volume happens on the host, ahead of the plan: outputs untouched."""
    Cv = np.full((5, 7, 16), 24, np.uint8)
    Cv[3, 2, 9] = 25
    bestD = np.full((1, 5, 7), 0xDEADBEEF, np.uint32)
    minC = bestD.copy()
    p = lib.fsgm_sgm_params_default()
    p.cost_bound = 24
    assert lib.fsgm_sgm_batch_host(1, _lib.ptr(Cv), 7, 5, 16, 6, 32, C.byref(p), None, _lib.ptr(bestD), _lib.ptr(minC), None) == FSGM_ERR_INVALID
    assert "cost_bound 24" in _err(lib) and "25" in _err(lib)
    assert (bestD == 0xDEADBEEF).all() and (minC == 0xDEADBEEF).all()
    with pytest.raises(_lib.FsgmError) as e:
        sgm_batch(Cv, 6, 32, cost_bound=24)
    assert e.value.status == FSGM_ERR_INVALID


def test_python_wrapper_argument_checks():
    Cv = np.zeros((5, 7, 16), np.uint8)
    with pytest.raises(ValueError, match="layout"):
        sgm_batch(Cv, layout="whd")
    with pytest.raises(TypeError, match="uint8"):
        sgm_batch(Cv.astype(np.float32))
    with pytest.raises(TypeError, match="N, H, W, D"):
        sgm_batch(Cv[0])
    with pytest.raises(TypeError, match="guide"):
        sgm_batch(Cv, adaptive_p2=1, guide=np.zeros((5, 8), np.uint8))
    assert isinstance(last_kernel(), str)


@pytest.mark.parametrize("dMax", [1, 16, 129, 1024])
def test_ingest_lds(lib, dMax):
    assert ingest_lds("hwd", dMax) == 0
    assert 0 < ingest_lds("dhw", dMax) <= 64 * 1024
    b = C.c_uint64()
    assert lib.fsgm_sgm_ingest_lds(2, dMax, C.byref(b)) == FSGM_ERR_INVALID and "layout" in _err(lib)
    assert lib.fsgm_sgm_ingest_lds(1, dMax, None) == FSGM_ERR_INVALID


def test_ingest_lds_refuses_dmax_out_of_range(lib):
    b = C.c_uint64()
    for D in (0, 1025):
        assert lib.fsgm_sgm_ingest_lds(1, D, C.byref(b)) == FSGM_ERR_INVALID and "dMax" in _err(lib)


def _fake_mode():
    from torch._subclasses.fake_tensor import FakeTensorMode
    return FakeTensorMode()


def _meta(ts):
    return [(tuple(t.shape), t.dtype, t.device.type) for t in ts]


def test_op_is_registered():
    assert hasattr(torch.ops.fsgm, "sgm")
    schema = str(torch.ops.fsgm.sgm.default._schema)
    assert "cost_bound" in schema and "layout" in schema


@pytest.mark.parametrize("N", [None, 3])
@pytest.mark.parametrize("layout", ["dhw", "hwd"])
def test_fake_sgm(N, layout):
    H, W, D = 9, 33, 16
    lead = () if N is None else (N,)
    shape = lead + ((D, H, W) if layout == "dhw" else (H, W, D))
    with _fake_mode():
        Cv = torch.empty(shape, dtype=torch.uint8, device="cuda")
        r = torch_ops.sgm(Cv, 6, 32, layout=layout, paths=8, return_status=True)
        assert _meta(r) == [(lead + (H, W), torch.uint32, "cuda")] * 2 + [((), torch.int32, "cuda")]
        r = torch_ops.sgm(Cv, 6, 32, layout=layout, return_sum=True)
        assert _meta(r) == [(lead + (H, W), torch.uint32, "cuda")] * 2 + [(lead + (H, W, D), torch.uint32, "cuda")]
        g = torch.empty(lead + (H, W), dtype=torch.uint8, device="cuda")
        r = torch_ops.sgm(Cv, 6, 32, layout=layout, adaptive_p2=1, guide=g)
        assert _meta(r) == [(lead + (H, W), torch.uint32, "cuda")] * 2
        n = N or 1
        raw = torch.ops.fsgm.sgm(Cv.reshape((n,) + shape[-3:]), g.reshape(n, H, W), 6, 32, 4, int(layout == "dhw"), 255, 0, 0, 1, 0)
        assert _meta(raw) == [((n, H, W), torch.uint32, "cuda")] * 2 + [((0,), torch.uint32, "cuda"), ((), torch.int32, "cuda")]


def test_wrapper_refuses_what_is_not_a_cuda_uint8_tensor():
    Cv = torch.zeros((16, 9, 33), dtype=torch.uint8)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.sgm(Cv)
    with pytest.raises(TypeError, match="torch.Tensor"):
        torch_ops.sgm(Cv.numpy())
    with _fake_mode():
        g = torch.empty((16, 9, 33), dtype=torch.uint8, device="cuda")
        with pytest.raises(TypeError, match="uint8"):
            torch_ops.sgm(g.float())
        with pytest.raises(TypeError, match="layout"):
            torch_ops.sgm(g[0], layout="dhw")
        with pytest.raises(ValueError, match="layout"):
            torch_ops.sgm(g, layout="dwh")
        with pytest.raises(TypeError, match="shape"):
            torch_ops.sgm(g, adaptive_p2=1, guide=torch.empty((9, 32), dtype=torch.uint8, device="cuda"))
