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


# ---- the op surface: every fsgm:: op's schema and its fake's outputs, as recorded on the commit before the bodies were shared ----
SCHEMAS = {'calc_cost_sgm': 'fsgm::calc_cost_sgm(Tensor I1, Tensor I2, Tensor pd0, Tensor nd, Tensor off, SymInt dMax, float vMax, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, SymInt '
                  'vz_to_disp, SymInt fb_check, SymInt adaptive_p2=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor)',
 'calc_cost_sgm_linear': 'fsgm::calc_cost_sgm_linear(Tensor I1, Tensor I2, Tensor pd0, Tensor nd, SymInt dMax, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, SymInt fb_check, SymInt '
                         'adaptive_p2=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor)',
 'epi_postprocess': 'fsgm::epi_postprocess(Tensor D1, Tensor Pd0, Tensor nd, Tensor O, float vMax, float n, float dMax) -> (Tensor, Tensor, Tensor, Tensor)',
 'epipolar_flow_pp': 'fsgm::epipolar_flow_pp(Tensor I0, Tensor I1, float[] geometry, SymInt dMax, float vMax, SymInt paths) -> (Tensor, Tensor, Tensor, Tensor, Tensor)',
 'epipolar_sgm_of': 'fsgm::epipolar_sgm_of(Tensor I0, Tensor I1, float[] geometry, SymInt dMax, float vMax, SymInt paths) -> (Tensor, Tensor, Tensor)',
 'flow_fb_check': 'fsgm::flow_fb_check(Tensor f, Tensor b, float thr) -> Tensor',
 'flow_level_hints': 'fsgm::flow_level_hints(Tensor flow, SymInt size) -> Tensor',
 'pyramidal_flow_pp': 'fsgm::pyramidal_flow_pp(Tensor I0, Tensor I1, SymInt matcher, SymInt numPyd, SymInt[] params, float[] chain, SymInt median) -> (Tensor, Tensor, Tensor, Tensor, '
                      'Tensor, Tensor)',
 'pyramidal_flow_pp_lm': 'fsgm::pyramidal_flow_pp_lm(Tensor I0, Tensor I1, SymInt matcher, SymInt numPyd, SymInt[] params, float[] chain, SymInt median, SymInt uniqueness_ratio, bool '
                         'want_minC2, SymInt level_median) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
 'pyramidal_flow_pp_u': 'fsgm::pyramidal_flow_pp_u(Tensor I0, Tensor I1, SymInt matcher, SymInt numPyd, SymInt[] params, float[] chain, SymInt median, SymInt uniqueness_ratio) -> (Tensor, '
                        'Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
 'pyramidal_sgm': 'fsgm::pyramidal_sgm(Tensor I0, Tensor I1, SymInt numPyd, SymInt[] params) -> (Tensor, Tensor, Tensor)',
 'pyramidal_sgm_lm': 'fsgm::pyramidal_sgm_lm(Tensor I0, Tensor I1, SymInt numPyd, SymInt[] params, SymInt level_median, bool runner_up) -> (Tensor, Tensor, Tensor, Tensor)',
 'pyramidal_sgm_ng': 'fsgm::pyramidal_sgm_ng(Tensor I0, Tensor I1, SymInt numPyd, SymInt[] params) -> (Tensor, Tensor, Tensor)',
 'pyramidal_sgm_ng_lm': 'fsgm::pyramidal_sgm_ng_lm(Tensor I0, Tensor I1, SymInt numPyd, SymInt[] params, SymInt level_median, bool runner_up) -> (Tensor, Tensor, Tensor, Tensor)',
 'pyramidal_sgm_ng_ru': 'fsgm::pyramidal_sgm_ng_ru(Tensor I0, Tensor I1, SymInt numPyd, SymInt[] params) -> (Tensor, Tensor, Tensor, Tensor)',
 'pyramidal_sgm_ru': 'fsgm::pyramidal_sgm_ru(Tensor I0, Tensor I1, SymInt numPyd, SymInt[] params) -> (Tensor, Tensor, Tensor, Tensor)',
 'sgm': 'fsgm::sgm(Tensor C_, Tensor guide, SymInt P1, SymInt P2, SymInt paths, SymInt layout, SymInt cost_bound, SymInt agg_mode, SymInt adaptive_p2, SymInt subpixel, SymInt return_sum) '
        '-> (Tensor, Tensor, Tensor, Tensor)',
 'sgm2d': 'fsgm::sgm2d(Tensor C_, Tensor hints, Tensor guide, SymInt half_x, SymInt half_y, SymInt P1, SymInt P2, SymInt layout, SymInt cost_bound, SymInt diagonal, SymInt total_pass, '
          'SymInt adaptive_p2, SymInt subpixel, SymInt return_flow, SymInt return_sum) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
 'sgm2d_exact': 'fsgm::sgm2d_exact(Tensor C_, Tensor hints, Tensor guide, SymInt half_x, SymInt half_y, SymInt P1, SymInt P2, SymInt layout, SymInt cost_bound, SymInt diagonal, SymInt '
                'total_pass, SymInt adaptive_p2, SymInt subpixel, SymInt return_flow, SymInt return_sum, bool runner_up) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
 'sgm2d_ru': 'fsgm::sgm2d_ru(Tensor C_, Tensor hints, Tensor guide, SymInt half_x, SymInt half_y, SymInt P1, SymInt P2, SymInt layout, SymInt cost_bound, SymInt diagonal, SymInt '
             'total_pass, SymInt adaptive_p2, SymInt subpixel, SymInt return_flow, SymInt return_sum) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
 'sgm_exact': 'fsgm::sgm_exact(Tensor C_, Tensor guide, SymInt P1, SymInt P2, SymInt paths, SymInt layout, SymInt cost_bound, SymInt agg_mode, SymInt adaptive_p2, SymInt subpixel, SymInt '
              'return_sum) -> (Tensor, Tensor, Tensor, Tensor)',
 'sgm_ru': 'fsgm::sgm_ru(Tensor C_, Tensor guide, SymInt P1, SymInt P2, SymInt paths, SymInt layout, SymInt cost_bound, SymInt agg_mode, SymInt adaptive_p2, SymInt subpixel, SymInt '
           'return_sum) -> (Tensor, Tensor, Tensor, Tensor, Tensor)',
 'stereo_fb_check': 'fsgm::stereo_fb_check(Tensor D1, Tensor D2, SymInt fused, SymInt d_min, SymInt direction, float thr) -> (Tensor, Tensor, Tensor)',
 'stereo_sgm': 'fsgm::stereo_sgm(Tensor left, Tensor right, SymInt dMax, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, SymInt direction, SymInt fb_check, SymInt adaptive_p2=0) -> '
               '(Tensor, Tensor, Tensor, Tensor, Tensor)',
 'stereo_sgm_pp': 'fsgm::stereo_sgm_pp(Tensor left, Tensor right, SymInt dMax, SymInt d_min, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, SymInt direction, SymInt adaptive_p2, '
                  'float[] chain, SymInt in_fill) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
 'stereo_sgm_range': 'fsgm::stereo_sgm_range(Tensor left, Tensor right, SymInt dMax, SymInt d_min, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, SymInt direction, SymInt fb_check, '
                     'SymInt adaptive_p2=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor)',
 'stereo_sgm_ru': 'fsgm::stereo_sgm_ru(Tensor left, Tensor right, SymInt dMax, SymInt d_min, SymInt P1, SymInt P2, SymInt paths, SymInt subpixel, SymInt direction, SymInt fb_check, SymInt '
                  'adaptive_p2=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)',
 'uniqueness_filter': 'fsgm::uniqueness_filter(Tensor map_, Tensor minC, Tensor minC2, SymInt ratio) -> (Tensor, Tensor)',
 'uniqueness_filter_planes': 'fsgm::uniqueness_filter_planes(Tensor map_, Tensor minC, Tensor minC2, SymInt ratio, SymInt planes) -> (Tensor, Tensor)',
 'vmf': 'fsgm::vmf(Tensor flow) -> Tensor'}

FAKE_OUTPUTS = {'calc_cost_sgm fb_check=0': 'uint32[2,8,8] uint32[2,8,8] uint8[0] uint32[0] int32[]',
 'calc_cost_sgm_linear fb_check=0': 'uint32[2,8,8] uint32[2,8,8] uint8[0] uint32[0] int32[]',
 'stereo_sgm fb_check=0': 'uint32[2,8,8] uint32[2,8,8] uint8[0] uint32[0] int32[]',
 'stereo_sgm_range fb_check=0': 'int32[2,8,8] uint32[2,8,8] uint8[0] int32[0] int32[]',
 'stereo_sgm_ru fb_check=0': 'int32[2,8,8] uint32[2,8,8] uint32[2,8,8] uint8[0] int32[0] int32[]',
 'calc_cost_sgm fb_check=1': 'uint32[2,8,8] uint32[2,8,8] uint8[2,8,8] uint32[2,8,8] int32[]',
 'calc_cost_sgm_linear fb_check=1': 'uint32[2,8,8] uint32[2,8,8] uint8[2,8,8] uint32[2,8,8] int32[]',
 'stereo_sgm fb_check=1': 'uint32[2,8,8] uint32[2,8,8] uint8[2,8,8] uint32[2,8,8] int32[]',
 'stereo_sgm_range fb_check=1': 'int32[2,8,8] uint32[2,8,8] uint8[2,8,8] int32[2,8,8] int32[]',
 'stereo_sgm_ru fb_check=1': 'int32[2,8,8] uint32[2,8,8] uint32[2,8,8] uint8[2,8,8] int32[2,8,8] int32[]',
 'sgm layout=0 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'sgm layout=0 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8,4] int32[]',
 'sgm layout=1 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'sgm layout=1 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8,4] int32[]',
 'sgm_exact layout=0 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'sgm_exact layout=0 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8,4] int32[]',
 'sgm_exact layout=1 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'sgm_exact layout=1 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8,4] int32[]',
 'sgm_ru layout=0 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'sgm_ru layout=0 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] uint32[2,8,8,4] int32[]',
 'sgm_ru layout=1 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'sgm_ru layout=1 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] uint32[2,8,8,4] int32[]',
 'sgm2d layout=0 return_flow=1 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8,9] int32[]',
 'sgm2d layout=1 return_flow=0 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[0] uint32[0] int32[]',
 'sgm2d layout=1 return_flow=1 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[0] int32[]',
 'sgm2d layout=1 return_flow=0 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[0] uint32[2,8,8,9] int32[]',
 'sgm2d layout=2 return_flow=1 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8,9] int32[]',
 'sgm2d_ru layout=0 return_flow=1 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8,9] int32[]',
 'sgm2d_ru layout=1 return_flow=0 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[0] uint32[0] int32[]',
 'sgm2d_ru layout=1 return_flow=1 return_sum=0': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[0] int32[]',
 'sgm2d_ru layout=1 return_flow=0 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[0] uint32[2,8,8,9] int32[]',
 'sgm2d_ru layout=2 return_flow=1 return_sum=1': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8,9] int32[]',
 'sgm2d_exact layout=0 return_flow=1 return_sum=1 runner_up=False': 'uint32[2,8,8] uint32[2,8,8] uint32[0] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8,9] int32[]',
 'sgm2d_exact layout=0 return_flow=1 return_sum=1 runner_up=True': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8,9] int32[]',
 'sgm2d_exact layout=1 return_flow=0 return_sum=0 runner_up=False': 'uint32[2,8,8] uint32[2,8,8] uint32[0] float64[2,2,8,8] float64[0] uint32[0] int32[]',
 'sgm2d_exact layout=1 return_flow=0 return_sum=0 runner_up=True': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[0] uint32[0] int32[]',
 'sgm2d_exact layout=1 return_flow=1 return_sum=0 runner_up=False': 'uint32[2,8,8] uint32[2,8,8] uint32[0] float64[2,2,8,8] float64[2,2,8,8] uint32[0] int32[]',
 'sgm2d_exact layout=1 return_flow=1 return_sum=0 runner_up=True': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[0] int32[]',
 'sgm2d_exact layout=1 return_flow=0 return_sum=1 runner_up=False': 'uint32[2,8,8] uint32[2,8,8] uint32[0] float64[2,2,8,8] float64[0] uint32[2,8,8,9] int32[]',
 'sgm2d_exact layout=1 return_flow=0 return_sum=1 runner_up=True': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[0] uint32[2,8,8,9] int32[]',
 'sgm2d_exact layout=2 return_flow=1 return_sum=1 runner_up=False': 'uint32[2,8,8] uint32[2,8,8] uint32[0] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8,9] int32[]',
 'sgm2d_exact layout=2 return_flow=1 return_sum=1 runner_up=True': 'uint32[2,8,8] uint32[2,8,8] uint32[2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8,9] int32[]',
 'epipolar_sgm_of gray': 'float64[2,3,8,8] uint32[2,8,8] int32[]',
 'epipolar_flow_pp gray': 'float64[2,3,8,8] float64[2,3,8,8] float64[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm gray': 'float64[2,2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_ng gray': 'float64[2,2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_ru gray': 'float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_ng_ru gray': 'float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_lm gray runner_up=False': 'float64[2,2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'pyramidal_sgm_ng_lm gray runner_up=False': 'float64[2,2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'pyramidal_sgm_lm gray runner_up=True': 'float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_ng_lm gray runner_up=True': 'float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp gray matcher=0': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp_u gray matcher=0': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp_lm gray matcher=0 want_minC2=False': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'pyramidal_flow_pp_lm gray matcher=0 want_minC2=True': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp gray matcher=1': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp_u gray matcher=1': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp_lm gray matcher=1 want_minC2=False': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'pyramidal_flow_pp_lm gray matcher=1 want_minC2=True': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'epipolar_sgm_of rgb': 'float64[2,3,8,8] uint32[2,8,8] int32[]',
 'epipolar_flow_pp rgb': 'float64[2,3,8,8] float64[2,3,8,8] float64[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm rgb': 'float64[2,2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_ng rgb': 'float64[2,2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_ru rgb': 'float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_ng_ru rgb': 'float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_lm rgb runner_up=False': 'float64[2,2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'pyramidal_sgm_ng_lm rgb runner_up=False': 'float64[2,2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'pyramidal_sgm_lm rgb runner_up=True': 'float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_sgm_ng_lm rgb runner_up=True': 'float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp rgb matcher=0': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp_u rgb matcher=0': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp_lm rgb matcher=0 want_minC2=False': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'pyramidal_flow_pp_lm rgb matcher=0 want_minC2=True': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp rgb matcher=1': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp_u rgb matcher=1': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'pyramidal_flow_pp_lm rgb matcher=1 want_minC2=False': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[0] int32[]',
 'pyramidal_flow_pp_lm rgb matcher=1 want_minC2=True': 'float64[2,3,8,8] float64[2,2,8,8] float64[2,2,8,8] float64[2,2,8,8] uint32[2,8,8] uint32[2,8,8] int32[]',
 'epi_postprocess': 'float64[2,8,8] float64[2,8,8] float64[2,8,8] int32[]',
 'vmf': 'float64[2,2,8,8]',
 'flow_level_hints': 'float64[2,2,16,16]',
 'flow_fb_check': 'float64[2,2,8,8]',
 'stereo_sgm_pp': 'float64[2,8,8] float64[2,8,8] int32[2,8,8] uint32[2,8,8] float64[2,8,8] int32[]',
 'stereo_fb_check fused=0': 'float64[2,8,8] float64[0] int32[]',
 'stereo_fb_check fused=1': 'float64[2,8,8] float64[2,8,8] int32[]',
 'uniqueness_filter': 'float64[2,8,8] int32[]',
 'uniqueness_filter_planes planes=1': 'float64[2,8,8] int32[]',
 'uniqueness_filter_planes planes=2': 'float64[2,2,8,8] int32[]'}

N_, H_, W_, D_ = 2, 8, 8, 4                # 8x8 images, 4 disparities, a batch of 2; the 2-D ops search a 3x3 window (9 candidates)
PYD_PARAMS, NG_PARAMS, CHAIN = [6, 32, 2, 5, 5, 1, 2, 0], [6, 32, 1, 2, 0], [2.0, 100.0, 2.0, 0.1]


def _fake_cases():
    """(label, op name, arguments) for every op, once per value of each switch that changes its outputs; call under a fake mode"""
    def t(dtype, *shape):
        return torch.empty(shape, dtype=dtype, device="cuda")
    u8, u32, f64 = torch.uint8, torch.uint32, torch.float64
    img, rgb, cost = t(u8, N_, H_, W_), t(u8, N_, 3, H_, W_), t(u32, N_, H_, W_)
    m1, m2, none8, none64 = t(f64, N_, H_, W_), t(f64, N_, 2, H_, W_), t(u8, 0), t(f64, 0)
    cases = []
    for fb in (0, 1):
        cases += [(f"calc_cost_sgm fb_check={fb}", "calc_cost_sgm", (img, img, m2, m2, m1, D_, 0.3, 6, 64, 4, 1, 1, fb, 0)),
                  (f"calc_cost_sgm_linear fb_check={fb}", "calc_cost_sgm_linear", (img, img, m2, m2, D_, 6, 64, 4, 1, fb, 0)),
                  (f"stereo_sgm fb_check={fb}", "stereo_sgm", (img, img, D_, 6, 64, 4, 1, -1, fb, 0)),
                  (f"stereo_sgm_range fb_check={fb}", "stereo_sgm_range", (img, img, D_, 0, 6, 64, 4, 1, -1, fb, 0)),
                  (f"stereo_sgm_ru fb_check={fb}", "stereo_sgm_ru", (img, img, D_, 0, 6, 64, 4, 1, -1, fb, 0))]
    for op in ("sgm", "sgm_exact", "sgm_ru"):
        for layout, vol in ((0, t(u8, N_, H_, W_, D_)), (1, t(u8, N_, D_, H_, W_))):
            for rs in (0, 1):
                cases.append((f"{op} layout={layout} return_sum={rs}", op, (vol, none8, 7, 100, 4, layout, 255, 0, 0, 1, rs)))
    for op in ("sgm2d", "sgm2d_ru", "sgm2d_exact"):
        for layout, vol in ((0, t(u8, N_, H_, W_, 9)), (1, t(u8, N_, 9, H_, W_)), (2, t(u8, N_, 9, H_, W_))):
            for rf, rs in ((0, 0), (1, 0), (0, 1)) if layout == 1 else ((1, 1),):
                args = (vol, none64, none8, 1, 1, 6, 32, layout, 255, 1, 2, 0, 1, rf, rs)
                if op != "sgm2d_exact":
                    cases.append((f"{op} layout={layout} return_flow={rf} return_sum={rs}", op, args))
                else:
                    cases += [(f"{op} layout={layout} return_flow={rf} return_sum={rs} runner_up={ru}", op, args + (ru,)) for ru in (False, True)]
    for name, I in (("gray", img), ("rgb", rgb)):
        cases += [(f"epipolar_sgm_of {name}", "epipolar_sgm_of", (I, I, [0.0] * (N_ * torch_ops.GEOMETRY_NUMBERS), D_, 0.3, 4)),
                  (f"epipolar_flow_pp {name}", "epipolar_flow_pp", (I, I, [0.0] * (N_ * torch_ops.GEOMETRY_NUMBERS), D_, 0.3, 4)),
                  (f"pyramidal_sgm {name}", "pyramidal_sgm", (I, I, 2, PYD_PARAMS)),
                  (f"pyramidal_sgm_ng {name}", "pyramidal_sgm_ng", (I, I, 2, NG_PARAMS)),
                  (f"pyramidal_sgm_ru {name}", "pyramidal_sgm_ru", (I, I, 2, PYD_PARAMS)),
                  (f"pyramidal_sgm_ng_ru {name}", "pyramidal_sgm_ng_ru", (I, I, 2, NG_PARAMS))]
        for ru in (False, True):
            cases += [(f"pyramidal_sgm_lm {name} runner_up={ru}", "pyramidal_sgm_lm", (I, I, 2, PYD_PARAMS, 3, ru)),
                      (f"pyramidal_sgm_ng_lm {name} runner_up={ru}", "pyramidal_sgm_ng_lm", (I, I, 2, NG_PARAMS, 3, ru))]
        for matcher, prm in ((0, PYD_PARAMS), (1, NG_PARAMS)):
            cases += [(f"pyramidal_flow_pp {name} matcher={matcher}", "pyramidal_flow_pp", (I, I, matcher, 2, prm, CHAIN, 0)),
                      (f"pyramidal_flow_pp_u {name} matcher={matcher}", "pyramidal_flow_pp_u", (I, I, matcher, 2, prm, CHAIN, 0, 5))]
            cases += [(f"pyramidal_flow_pp_lm {name} matcher={matcher} want_minC2={want}", "pyramidal_flow_pp_lm",
                       (I, I, matcher, 2, prm, CHAIN, 0, 5 if want else 0, want, 3)) for want in (False, True)]
    cases += [("epi_postprocess", "epi_postprocess", (m1, m2, m2, m1, 0.3, 1.0, float(D_))),
              ("vmf", "vmf", (m2,)),
              ("flow_level_hints", "flow_level_hints", (m2, 3)),
              ("flow_fb_check", "flow_fb_check", (m2, m2, 2.0)),
              ("stereo_sgm_pp", "stereo_sgm_pp", (img, img, D_, 0, 6, 64, 4, 1, -1, 0, [0.0] * len(torch_ops.STEREO_PP_FIELDS), 1)),
              ("stereo_fb_check fused=0", "stereo_fb_check", (m1, m1, 0, 0, -1, 2.0)),
              ("stereo_fb_check fused=1", "stereo_fb_check", (m1, m1, 1, 0, -1, 2.0)),
              ("uniqueness_filter", "uniqueness_filter", (m1, cost, cost, 5)),
              ("uniqueness_filter_planes planes=1", "uniqueness_filter_planes", (m1, cost, cost, 5, 1)),
              ("uniqueness_filter_planes planes=2", "uniqueness_filter_planes", (m2, cost, cost, 5, 2))]
    return cases


def _live_schemas():
    return {name: str(getattr(torch.ops.fsgm, name).default._schema) for name in dir(torch.ops.fsgm)
            if hasattr(getattr(torch.ops.fsgm, name), "default")}


def _live_fake_outputs():
    with _fake_mode():
        res = {}
        for label, op, args in _fake_cases():
            r = getattr(torch.ops.fsgm, op)(*args)
            res[label] = " ".join(str(o.dtype).removeprefix("torch.") + str(list(o.shape)).replace(" ", "")
                                  for o in (r if isinstance(r, tuple) else (r,)))
    return res


def test_every_op_keeps_its_schema_and_its_fakes_outputs():
    """SCHEMAS and FAKE_OUTPUTS were printed by _live_schemas() / _live_fake_outputs() on the commit before the op bodies were shared
    (every op of the package is in both), so a change of an op's name, arguments, defaults or outputs shows here."""
    live = _live_schemas()
    assert sorted(live) == sorted(SCHEMAS)
    for name in SCHEMAS:
        assert live[name] == SCHEMAS[name], name
    with _fake_mode():
        assert {op for _, op, _ in _fake_cases()} == set(SCHEMAS)
    got = _live_fake_outputs()
    assert list(got) == list(FAKE_OUTPUTS)
    for label in FAKE_OUTPUTS:
        assert got[label] == FAKE_OUTPUTS[label], label
