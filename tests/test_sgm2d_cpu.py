"""CPU-side tests of the 2-D matcher on caller-supplied volumes (fsgm_sgm2d_batch_host / fsgm_sgm2d_device, fsgm::sgm2d): every
refusal that needs no device, the boundary values just inside, the parameter defaults, the ingest kernel's LDS request, the
Python wrappers' argument checks and the torch op's fake implementation."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
from fsgm_amd import _lib, sgm2d_batch  # noqa: E402
from fsgm_amd.sgm2d import Sgm2dParams, _bind, ingest_lds, last_kernel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FSGM_ERR_INVALID, FSGM_ERR_HIP, FSGM_ERR_UNSUPPORTED = 1, 2, 4
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call it is passed to fails its argument checks first
TILE_LDS = 64 * 68 + 4           # INGEST_TD rows of INGEST_PITCH bytes and the flag word (fsgm_amd/csrc/sgm_ingest.h)


@pytest.fixture(scope="module")
def lib():
    return _bind(_lib.load())


def _err(lib):
    return lib.fsgm_last_error().decode()


def _args(prm, n, Cp, W, H, rX, rY, preMv, mvW, mvH, guide, bestD, minC, mvSub):
    return (n, Cp, W, H, rX, rY, 6, 32, None if prm is None else C.byref(prm), preMv, mvW, mvH, guide, bestD, minC, mvSub, None, None)


def _host(lib, prm=None, n=1, Cp=FAKE, W=32, H=24, rX=1, rY=2, preMv=None, mvW=0, mvH=0, guide=None, bestD=FAKE, minC=FAKE, mvSub=FAKE):
    return lib.fsgm_sgm2d_batch_host(*_args(prm, n, Cp, W, H, rX, rY, preMv, mvW, mvH, guide, bestD, minC, mvSub))


def _device(lib, prm=None, n=1, Cp=FAKE, W=32, H=24, rX=1, rY=2, preMv=None, mvW=0, mvH=0, guide=None, bestD=FAKE, minC=FAKE, mvSub=FAKE):
    return lib.fsgm_sgm2d_device(*_args(prm, n, Cp, W, H, rX, rY, preMv, mvW, mvH, guide, bestD, minC, mvSub), None, None)


def _prm(lib, **kw):
    p = lib.fsgm_sgm2d_params_default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_params_default(lib):
    p = lib.fsgm_sgm2d_params_default()
    assert (p.diagonal, p.totalPass, p.adaptive_p2, p.subpixel, p.device, p.layout, p.cost_bound) == (1, 2, 0, 1, 0, 0, 255)
    assert list(p.reserved) == [0] * 5
    assert C.sizeof(Sgm2dParams) == 48


@pytest.mark.parametrize("call", [_host, _device], ids=["host", "device"])
def test_refusals_without_a_device(lib, call):
    bad = lambda **kw: call(lib, **kw)  # noqa: E731
    for n in (0, -3):
        assert bad(n=n) == FSGM_ERR_INVALID and "n_frames" in _err(lib)
    assert bad(W=0) == FSGM_ERR_INVALID and "width/height" in _err(lib)
    assert bad(H=-1) == FSGM_ERR_INVALID and "width/height" in _err(lib)
    assert bad(rX=-1) == FSGM_ERR_INVALID and "halfX/halfY" in _err(lib)
    assert bad(rY=-1) == FSGM_ERR_INVALID and "halfX/halfY" in _err(lib)
    assert bad(rX=32, rY=0) == FSGM_ERR_UNSUPPORTED and "side exceeds 64" in _err(lib)          # a side of 65
    assert bad(rX=0, rY=32) == FSGM_ERR_UNSUPPORTED and "side exceeds 64" in _err(lib)
    assert bad(rX=16, rY=16) == FSGM_ERR_UNSUPPORTED and "1089 candidates" in _err(lib)          # 33 x 33
    assert bad(W=16384, H=16384, rX=1, rY=1) == FSGM_ERR_UNSUPPORTED and "2^31" in _err(lib)     # 2^28 pixels x 9 candidates
    assert bad(W=32768, H=65536, rX=0, rY=0) == FSGM_ERR_UNSUPPORTED and "2^31" in _err(lib)     # exactly 2^31
    for layout in (-1, 3):
        assert bad(prm=_prm(lib, layout=layout)) == FSGM_ERR_INVALID and "layout" in _err(lib)
    for bound in (0, 256, -1):
        assert bad(prm=_prm(lib, cost_bound=bound)) == FSGM_ERR_INVALID and "cost_bound" in _err(lib)
    for passes in (0, 3, -1):
        assert bad(prm=_prm(lib, totalPass=passes)) == FSGM_ERR_INVALID and "totalPass" in _err(lib)
    for field in ("diagonal", "adaptive_p2", "subpixel"):
        for v in (2, -1):
            assert bad(prm=_prm(lib, **{field: v})) == FSGM_ERR_INVALID and field in _err(lib)
    for slot in range(5):
        p = _prm(lib)
        p.reserved[slot] = 1
        assert bad(prm=p) == FSGM_ERR_INVALID and "reserved" in _err(lib)
    for null in ("Cp", "bestD", "minC", "mvSub"):
        assert bad(**{null: None}) == FSGM_ERR_INVALID and "null argument" in _err(lib)
    assert bad(preMv=FAKE, mvW=31, mvH=24) == FSGM_ERR_INVALID and "preMv (31 x 24)" in _err(lib)
    assert bad(preMv=FAKE, mvW=32, mvH=23) == FSGM_ERR_INVALID and "preMv (32 x 23)" in _err(lib)
    assert bad(prm=_prm(lib, adaptive_p2=1)) == FSGM_ERR_INVALID and "guide" in _err(lib)


# (halfX, halfY, cost_bound, totalPass): sides of 63, 31 x 33 = 1023 candidates, both ends of cost_bound and of totalPass
BOUNDARIES = [(31, 0, 255, 2), (0, 31, 255, 2), (15, 16, 255, 2), (1, 2, 1, 2), (1, 2, 255, 1), (1, 2, 255, 2)]


@pytest.mark.parametrize("rX,rY,bound,passes", BOUNDARIES)
def test_boundary_values_pass_the_argument_checks(lib, rX, rY, bound, passes):
    """Real (host) memory everywhere, a 2 x 1 image with a hint map of exactly its size.  Without a device both forms get as far
    as asking for one (FSGM_ERR_HIP); with one the host form runs, and the device form gets as far as its pointer checks, which
    refuse host memory by name."""
    W, H, D = 2, 1, (2 * rX + 1) * (2 * rY + 1)
    Cv = np.zeros((H, W, D), np.uint8)
    mv = np.zeros((2, H, W), np.float64)
    bestD, minC, mvSub = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32), np.zeros((2, H, W), np.float64)
    p = _lib.ptr
    kw = dict(prm=_prm(lib, cost_bound=bound, totalPass=passes), Cp=p(Cv), W=W, H=H, rX=rX, rY=rY, preMv=p(mv), mvW=W, mvH=H, bestD=p(bestD),
              minC=p(minC), mvSub=p(mvSub))
    have_gpu = lib.fsgm_device_count() >= 1
    st = _host(lib, **kw)
    assert st == (0 if have_gpu else FSGM_ERR_HIP), _err(lib)
    st = _device(lib, **kw)
    if have_gpu:
        assert st == FSGM_ERR_INVALID and "C (" in _err(lib) and "fsgm_sgm2d_device" in _err(lib), _err(lib)
    else:
        assert st == FSGM_ERR_HIP, _err(lib)


def test_host_form_refuses_a_volume_above_its_bound_before_any_device(lib):
    """The scan of the volume happens on the host, ahead of the plan: outputs untouched."""
    Cv = np.full((5, 7, 15), 24, np.uint8)
    Cv[3, 2, 9] = 25
    bestD = np.full((1, 5, 7), 0xDEADBEEF, np.uint32)
    minC = bestD.copy()
    mvSub = np.full((1, 2, 5, 7), -7.0)
    p = _lib.ptr
    st = _host(lib, prm=_prm(lib, cost_bound=24), Cp=p(Cv), W=7, H=5, bestD=p(bestD), minC=p(minC), mvSub=p(mvSub))
    assert st == FSGM_ERR_INVALID and "cost_bound 24" in _err(lib) and "25" in _err(lib)
    assert (bestD == 0xDEADBEEF).all() and (minC == 0xDEADBEEF).all() and (mvSub == -7.0).all()
    with pytest.raises(_lib.FsgmError) as e:
        sgm2d_batch(Cv, 1, 2, layout="hwd", cost_bound=24)
    assert e.value.status == FSGM_ERR_INVALID


def test_ingest_lds_refusals(lib):
    b = C.c_uint64()
    for layout in (-1, 3):
        assert lib.fsgm_sgm2d_ingest_lds(layout, 1, 1, C.byref(b)) == FSGM_ERR_INVALID and "layout" in _err(lib)
    assert lib.fsgm_sgm2d_ingest_lds(1, 1, 1, None) == FSGM_ERR_INVALID
    assert lib.fsgm_sgm2d_ingest_lds(1, -1, 1, C.byref(b)) == FSGM_ERR_INVALID and "half sizes" in _err(lib)
    assert lib.fsgm_sgm2d_ingest_lds(1, 1, -1, C.byref(b)) == FSGM_ERR_INVALID and "half sizes" in _err(lib)
    assert lib.fsgm_sgm2d_ingest_lds(1, 32, 0, C.byref(b)) == FSGM_ERR_UNSUPPORTED and "side exceeds" in _err(lib)
    assert lib.fsgm_sgm2d_ingest_lds(2, 16, 16, C.byref(b)) == FSGM_ERR_UNSUPPORTED and "candidates" in _err(lib)


@pytest.mark.parametrize("half", [(0, 0), (1, 2), (2, 1), (4, 4), (5, 5), (6, 4), (15, 16), (31, 0), (0, 31)])
def test_ingest_lds(half):
    assert ingest_lds("hwd", *half) == 0                     # the copy, and the padded repack in registers
    assert ingest_lds("dhw", *half) == ingest_lds("dhw_yx", *half) == TILE_LDS


def test_python_wrapper_argument_checks():
    Cv = np.zeros((15, 5, 7), np.uint8)                       # (D, H, W) of a 3 x 5 window
    with pytest.raises(ValueError, match="layout"):
        sgm2d_batch(Cv, 1, 2, layout="whd")
    with pytest.raises(TypeError, match="uint8"):
        sgm2d_batch(Cv.astype(np.float32), 1, 2)
    with pytest.raises(TypeError, match="N, D, H, W"):
        sgm2d_batch(Cv[0], 1, 2)
    with pytest.raises(ValueError, match="15 candidates"):    # the volume's count against a 5 x 5 window's
        sgm2d_batch(Cv, 2, 2)
    with pytest.raises(ValueError, match="25"):
        sgm2d_batch(Cv, 2, 2, layout="dhw_yx")
    with pytest.raises(ValueError, match="candidates"):       # an (H, W, D) reading of the same bytes
        sgm2d_batch(Cv, 1, 2, layout="hwd")
    with pytest.raises(ValueError, match="non-negative"):
        sgm2d_batch(Cv, -1, 2)
    with pytest.raises(TypeError, match="hints"):
        sgm2d_batch(Cv, 1, 2, hints=np.zeros((2, 5, 7), np.float32))
    with pytest.raises(TypeError, match="hints"):
        sgm2d_batch(Cv, 1, 2, hints=np.zeros((3, 5, 7)))
    with pytest.raises(TypeError, match="hints"):
        sgm2d_batch(Cv, 1, 2, hints=np.zeros((1, 2, 5, 7)))  # a batch's hints with one volume
    with pytest.raises(ValueError, match="at least as large"):
        sgm2d_batch(Cv, 1, 2, hints=np.zeros((2, 5, 6)))
    with pytest.raises(TypeError, match="guide"):
        sgm2d_batch(Cv, 1, 2, adaptive_p2=1, guide=np.zeros((5, 8), np.uint8))
    assert isinstance(last_kernel(), str)


def test_import_fsgm_amd_leaves_torch_out():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = "import sys, fsgm_amd; assert callable(fsgm_amd.sgm2d_batch); import fsgm_amd.sgm2d; assert 'torch' not in sys.modules"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def _fake_mode():
    from torch._subclasses.fake_tensor import FakeTensorMode
    return FakeTensorMode()


def _meta(ts):
    return [(tuple(t.shape), t.dtype, t.device.type) for t in ts]


def test_op_is_registered():
    assert hasattr(torch.ops.fsgm, "sgm2d")
    schema = str(torch.ops.fsgm.sgm2d.default._schema)
    assert "cost_bound" in schema and "layout" in schema and "hints" in schema and "half_x" in schema


@pytest.mark.parametrize("N", [None, 3])
@pytest.mark.parametrize("layout", ["dhw", "dhw_yx", "hwd"])
def test_fake_sgm2d(N, layout):
    H, W, rX, rY = 9, 33, 1, 2
    D = 15
    lead = () if N is None else (N,)
    shape = lead + ((H, W, D) if layout == "hwd" else (D, H, W))
    maps, planes = (lead + (H, W), torch.uint32, "cuda"), (lead + (2, H, W), torch.float64, "cuda")
    with _fake_mode():
        Cv = torch.empty(shape, dtype=torch.uint8, device="cuda")
        r = torch_ops.sgm2d(Cv, rX, rY, layout=layout, return_status=True)
        assert _meta(r) == [maps, maps, planes, ((), torch.int32, "cuda")]
        hints = torch.empty(lead + (2, H + 1, W + 2), dtype=torch.float64, device="cuda")
        r = torch_ops.sgm2d(Cv, rX, rY, layout=layout, hints=hints, return_flow=True, return_sum=True)
        assert _meta(r) == [maps, maps, planes, planes, (lead + (H, W, D), torch.uint32, "cuda")]
        g = torch.empty(lead + (H, W), dtype=torch.uint8, device="cuda")
        r = torch_ops.sgm2d(Cv, rX, rY, layout=layout, adaptive_p2=1, guide=g, return_sum=True)
        assert _meta(r) == [maps, maps, planes, (lead + (H, W, D), torch.uint32, "cuda")]
        n = N or 1
        none64, none8 = torch.empty((0,), dtype=torch.float64, device="cuda"), torch.empty((0,), dtype=torch.uint8, device="cuda")
        code = {"hwd": 0, "dhw": 1, "dhw_yx": 2}[layout]
        raw = torch.ops.fsgm.sgm2d(Cv.reshape((n,) + shape[-3:]), none64, none8, rX, rY, 6, 32, code, 255, 1, 2, 0, 1, 0, 0)
        assert _meta(raw) == [((n, H, W), torch.uint32, "cuda")] * 2 + [((n, 2, H, W), torch.float64, "cuda"), ((0,), torch.float64, "cuda"),
                                                                       ((0,), torch.uint32, "cuda"), ((), torch.int32, "cuda")]


def test_wrapper_refuses_what_is_not_a_contiguous_cuda_uint8_tensor():
    Cv = torch.zeros((15, 9, 33), dtype=torch.uint8)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.sgm2d(Cv, 1, 2)
    with pytest.raises(TypeError, match="torch.Tensor"):
        torch_ops.sgm2d(Cv.numpy(), 1, 2)
    with _fake_mode():
        g = torch.empty((15, 9, 33), dtype=torch.uint8, device="cuda")
        with pytest.raises(TypeError, match="uint8"):
            torch_ops.sgm2d(g.float(), 1, 2)
        with pytest.raises(TypeError, match="contiguous"):
            torch_ops.sgm2d(torch.empty((9, 33, 15), dtype=torch.uint8, device="cuda").permute(2, 0, 1), 1, 2)
        with pytest.raises(TypeError, match="layout"):
            torch_ops.sgm2d(g[0], 1, 2, layout="dhw")
        with pytest.raises(ValueError, match="layout"):
            torch_ops.sgm2d(g, 1, 2, layout="dwh")
        with pytest.raises(ValueError, match="candidates"):
            torch_ops.sgm2d(g, 2, 2)
        with pytest.raises(TypeError, match="float64"):
            torch_ops.sgm2d(g, 1, 2, hints=torch.empty((2, 9, 33), dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError, match="at least as large"):
            torch_ops.sgm2d(g, 1, 2, hints=torch.empty((2, 9, 32), dtype=torch.float64, device="cuda"))
        with pytest.raises(TypeError, match="shape"):
            torch_ops.sgm2d(g, 1, 2, adaptive_p2=1, guide=torch.empty((9, 32), dtype=torch.uint8, device="cuda"))
