"""CPU-side tests of the device-pointer interface: the torch ops' fake implementations, the one-runtime rule and the C entry
points' argument checks (all of which answer before any device is touched)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
from fsgm_amd import _lib, synth  # noqa: E402
from fsgm_amd.epi import EpiGeometry  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4


def _fake_mode():
    from torch._subclasses.fake_tensor import FakeTensorMode
    return FakeTensorMode()


def _meta(ts):
    return [(tuple(t.shape), t.dtype, t.device.type) for t in ts]


@pytest.mark.parametrize("N", [None, 8])
def test_fake_calc_cost_sgm(N):
    lead = () if N is None else (N,)
    with _fake_mode():
        I = torch.empty(lead + (47, 83), dtype=torch.uint8, device="cuda")
        m = torch.empty(lead + (2, 47, 83), dtype=torch.float64, device="cuda")
        o = torch.empty(lead + (47, 83), dtype=torch.float64, device="cuda")
        r = torch_ops.calc_cost_sgm(I, I, 64, 0.3, m, m, o, 6, 64, paths=8, return_status=True)
        assert _meta(r) == [(lead + (47, 83), torch.uint32, "cuda")] * 2 + [((), torch.int32, "cuda")]
        r = torch_ops.calc_cost_sgm(I, I, 64, 0.3, m, m, o, 6, 64, fb_check=1)
        assert _meta(r) == [(lead + (47, 83), t, "cuda") for t in (torch.uint32, torch.uint32, torch.uint8, torch.uint32)]
        n = N or 1
        raw = torch.ops.fsgm.calc_cost_sgm(I.reshape(n, 47, 83), I.reshape(n, 47, 83), m.reshape(n, 2, 47, 83), m.reshape(n, 2, 47, 83),
                                           o.reshape(n, 47, 83), 64, 0.3, 6, 64, 4, 1, 1, 0)
        assert _meta(raw) == [((n, 47, 83), torch.uint32, "cuda")] * 2 + [((0,), torch.uint8, "cuda"), ((0,), torch.uint32, "cuda"),
                                                                         ((), torch.int32, "cuda")]


@pytest.mark.parametrize("N", [None, 8])
@pytest.mark.parametrize("rgb", [False, True])
def test_fake_epipolar_and_pyramids(N, rgb):
    lead = () if N is None else (N,)
    planes = (3,) if rgb else ()
    F, Hm = np.eye(3), np.eye(3)
    geo = (F, Hm, (40.0, 20.0), 0) if N is None else ([F] * N, [Hm] * N, [(40.0, 20.0)] * N, [0] * N)
    with _fake_mode():
        I = torch.empty(lead + planes + (47, 83), dtype=torch.uint8, device="cuda")
        flow, minC = torch_ops.epipolar_sgm_of(I, I, *geo)
        assert _meta((flow, minC)) == [(lead + (3, 47, 83), torch.float64, "cuda"), (lead + (47, 83), torch.uint32, "cuda")]
        for fn in (torch_ops.pyramidal_sgm, torch_ops.pyramidal_sgm_ng):
            mv, mc, st = fn(I, I, 3, batch=N is not None, return_status=True)
            assert _meta((mv, mc, st)) == [(lead + (2, 47, 83), torch.float64, "cuda"), (lead + (47, 83), torch.uint32, "cuda"),
                                           ((), torch.int32, "cuda")]


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    I1, I2 = (torch.from_numpy(a) for a in synth.image_pair(32, 24, 16))
    pd0, nd, off = (torch.from_numpy(a) for a in synth.epi_maps(32, 24))
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.calc_cost_sgm(I1, I2, 16, 0.3, pd0, nd, off, 6, 64)
    with pytest.raises(TypeError, match="GPU"):
        torch_ops.pyramidal_sgm(I1, I2, 3)
    with _fake_mode() as mode:
        g = [mode.from_tensor(t).to("cuda") for t in (I1, I2, pd0, nd, off)]
        with pytest.raises(TypeError, match="float64"):
            torch_ops.calc_cost_sgm(g[0], g[1], 16, 0.3, g[2].float(), g[3], g[4], 6, 64)
        with pytest.raises(TypeError, match="shape"):
            torch_ops.calc_cost_sgm(g[0], g[1], 16, 0.3, g[2][0], g[3], g[4], 6, 64)
        with pytest.raises(TypeError, match="shape"):
            torch_ops.calc_cost_sgm(g[0], g[1][:, :8], 16, 0.3, g[2], g[3], g[4], 6, 64)


def _python(code):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_import_torch_ops_maps_one_hip_runtime():
    r = _python("import fsgm_amd.torch_ops as t; r = t.hip_runtimes(); assert len(r) == 1, r; print(r[0])")
    assert r.returncode == 0, r.stderr
    assert "libamdhip64" in r.stdout


def test_library_loaded_before_torch_is_refused():
    r = _python("import fsgm_amd\nfsgm_amd.load_library()\ntry:\n    import fsgm_amd.torch_ops\nexcept ImportError as e:\n"
                "    print('REFUSED', e)\nelse:\n    print('ACCEPTED')")
    assert r.returncode == 0, r.stderr
    assert "REFUSED" in r.stdout and "loaded before torch" in r.stdout and "Import torch" in r.stdout, r.stdout


def test_import_fsgm_amd_does_not_import_torch():
    r = _python("import fsgm_amd; import sys; assert 'torch' not in sys.modules")
    assert r.returncode == 0, r.stderr


# ---- the C entry points' argument checks: they answer before any device or pointer query ----
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call below fails its argument checks first


def _epi_args(W=32, H=24, D=16):
    e, o = _lib.EpiIn(), _lib.EpiOut()
    e.I1 = e.I2 = e.pixelPosD0 = e.normDir = e.offset = FAKE
    e.width, e.height, e.dMax, e.vMax, e.P1, e.P2 = W, H, D, 0.3, 6, 64
    o.bestD = o.minC = FAKE
    return e, o


def _err(lib):
    return lib.fsgm_last_error().decode()


def test_calc_cost_sgm_device_argument_checks():
    lib = _lib.load()
    e, o = _epi_args()
    assert lib.fsgm_calc_cost_sgm_device(0, C.byref(e), C.byref(o), None, None, None) == FSGM_ERR_INVALID
    assert "n_frames" in _err(lib)
    assert lib.fsgm_calc_cost_sgm_device(1, None, C.byref(o), None, None, None) == FSGM_ERR_INVALID
    assert "null argument" in _err(lib)
    e.offset = None
    assert lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), None, None, None) == FSGM_ERR_INVALID
    assert "null input" in _err(lib)
    e, o = _epi_args()
    o.minC = None
    assert lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), None, None, None) == FSGM_ERR_INVALID
    assert "null output" in _err(lib)
    e, o = _epi_args(W=0)
    assert lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), None, None, None) == FSGM_ERR_INVALID
    assert "width/height" in _err(lib)
    for tap in ("C", "S"):
        e, o = _epi_args()
        setattr(o, tap, FAKE)
        assert lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), None, None, None) == FSGM_ERR_UNSUPPORTED
        assert "debug taps" in _err(lib)
    e, o = _epi_args()
    assert lib.fsgm_epi_plan_run_device(None, 1, C.byref(e), C.byref(o), None, None) == FSGM_ERR_INVALID
    assert "null plan" in _err(lib)


def test_driver_device_argument_checks():
    lib = _lib.load()
    g = EpiGeometry()
    args = lambda n, ch, flow=FAKE: (n, FAKE, FAKE, 32, 24, ch, C.byref(g), 16, 0.3, None, flow, None, None, None)  # noqa: E731
    assert lib.fsgm_epipolar_sgm_of_device(*args(0, 1)) == FSGM_ERR_INVALID and "n_frames" in _err(lib)
    assert lib.fsgm_epipolar_sgm_of_device(*args(1, 2)) == FSGM_ERR_INVALID and "channels" in _err(lib)
    assert lib.fsgm_epipolar_sgm_of_device(*args(1, 1, None)) == FSGM_ERR_INVALID and "null argument" in _err(lib)
    prm = lib.fsgm_pyramid_params_default()
    nprm = lib.fsgm_ng_pyramid_params_default()
    for fn, p in ((lib.fsgm_pyramidal_sgm_device, prm), (lib.fsgm_pyramidal_sgm_ng_device, nprm)):
        assert fn(0, FAKE, FAKE, 32, 24, 1, C.byref(p), FAKE, None, None, None) == FSGM_ERR_INVALID and "n_frames" in _err(lib)
        assert fn(1, FAKE, FAKE, 32, 24, 2, C.byref(p), FAKE, None, None, None) == FSGM_ERR_INVALID and "channels" in _err(lib)
        assert fn(1, FAKE, FAKE, 0, 24, 1, C.byref(p), FAKE, None, None, None) == FSGM_ERR_INVALID and "width/height" in _err(lib)
        assert fn(1, FAKE, FAKE, 32, 24, 1, None, FAKE, None, None, None) == FSGM_ERR_INVALID and "null argument" in _err(lib)
        assert fn(1, FAKE, FAKE, 32, 24, 1, C.byref(p), None, None, None, None) == FSGM_ERR_INVALID and "null argument" in _err(lib)


def test_cached_plan_entries_refuse_plan_arguments_before_any_device():
    """What plan creation refuses without a GPU, the device entries on cached plans refuse before the device and pointer checks
    (their plan is looked up only after those): the same status and message with or without a device, FAKE never queried."""
    from fsgm_amd.epi import _params
    lib = _lib.load()
    e, o = _epi_args()
    prm = _params(5, 1, 1, 0)
    assert lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), C.byref(prm), None, None) == FSGM_ERR_INVALID and "paths" in _err(lib)
    prm = _params(4, 1, 1, 64)
    assert lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), C.byref(prm), None, None) == FSGM_ERR_INVALID
    assert _err(lib) == "device 64 out of range"
    e, o = _epi_args(D=1025)
    assert lib.fsgm_calc_cost_sgm_device(1, C.byref(e), C.byref(o), None, None, None) == FSGM_ERR_UNSUPPORTED and "maximum" in _err(lib)
    g = EpiGeometry()
    assert lib.fsgm_epipolar_sgm_of_device(1, FAKE, FAKE, 32, 24, 1, C.byref(g), 1025, 0.3, None, FAKE, None, None, None) == FSGM_ERR_UNSUPPORTED
    assert "maximum" in _err(lib)
    prm = lib.fsgm_pyramid_params_default()
    prm.numPyd = 17
    assert lib.fsgm_pyramidal_sgm_device(1, FAKE, FAKE, 32, 24, 1, C.byref(prm), FAKE, None, None, None) == FSGM_ERR_INVALID
    assert "numPyd" in _err(lib)
