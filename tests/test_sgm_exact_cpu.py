"""CPU-side tests of sgm(C) with exact path arithmetic (fsgm_sgm_batch_host_exact / fsgm_sgm_device_exact, fsgm::sgm_exact):
the yardstick of the GPU tests (tests/sgm_exact_restatement.py) tied to the pinned oracle where the two must agree, the proof
that they disagree where the GPU tests look, and every refusal of the new entries that needs no device."""
import ctypes as C

import numpy as np
import pytest

try:                                     # torch first where it is installed: the library must bind to its HIP runtime
    import torch  # noqa: F401
except ImportError:                      # (only the torch test at the end needs it)
    torch = None

from fsgm_amd import _lib  # noqa: E402
from fsgm_amd.sgm import _bind, sgm_batch  # noqa: E402
from oracle import pyoracle  # noqa: E402
from tests import adaptive_p2_restatement as A  # noqa: E402
from tests import sgm_exact_restatement as X  # noqa: E402

FSGM_ERR_INVALID, FSGM_ERR_UNSUPPORTED = 1, 4
FAKE = C.c_void_p(0x1000)        # never dereferenced: every call it goes into fails its argument checks first
# the shapes and disparity ranges of tests/test_gpu_sgm_exact.py
GPU_SHAPES = ((37, 11), (9, 21))
GPU_DMAX = (16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 224, 256, 24, 300)


@pytest.fixture(scope="module")
def lib():
    return _bind(_lib.load())


def _err(lib):
    return lib.fsgm_last_error().decode()


def _oracle_sgm(Cv, P1, P2, paths, guide):
    """the mod-256 rule: the C++ oracle, with adaptive P2 its pinned restatement (the oracle's aggregation has no such switch)"""
    H, W, D = Cv.shape
    S = A.aggregate(Cv, guide, P1, P2, paths, 1) if guide is not None else pyoracle.epi_aggregate(Cv, P1, P2, paths)
    return pyoracle.epi_wta(S, W, H, D, 1) + (S[:-1].reshape(H, W, D),)


# ---- 1. inside the no-wrap budget the restatement IS the pinned oracle ----
@pytest.mark.parametrize("adaptive", [0, 1], ids=["plain", "adaptive"])
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("dMax", [16, 48, 24])
@pytest.mark.parametrize("cmax,P1,P2", [(24, 6, 64), (55, 7, 100)])
def test_restatement_equals_the_oracle_inside_the_budget(cmax, P1, P2, dMax, paths, adaptive):
    assert cmax + P2 + max(P1, P2) <= 255
    rng = np.random.default_rng(1000 * cmax + 10 * dMax + paths + adaptive)
    for W, H in GPU_SHAPES:
        Cv = rng.integers(0, cmax + 1, (H, W, dMax), dtype=np.uint8)
        Cv[rng.integers(0, H), rng.integers(0, W)] = cmax       # the bound is reached
        guide = rng.choice(np.array([10, 30, 40, 70, 200], np.uint8), (H, W)) if adaptive else None   # steps of 10 and 20, 30 and more
        bd, mc, S = X.sgm(Cv, P1, P2, paths, guide)
        obd, omc, oS = _oracle_sgm(Cv, P1, P2, paths, guide)
        assert np.array_equal(S, oS) and np.array_equal(mc, omc) and np.array_equal(bd, obd)


# ---- 2. outside it the two differ, at every shape the GPU tests use ----
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("dMax", GPU_DMAX)
def test_mod256_and_exact_disagree_on_random_bytes(dMax, paths):
    """Uniform random bytes at sgm.m's P1 = 7, P2 = 100: were the exact entries to run the old kernels, the GPU comparisons with
    the restatement could not pass.  (Share of pixels whose bestD differs: DESIGN_LOG.md.)"""
    rng = np.random.default_rng(7 * dMax + paths)
    for W, H in GPU_SHAPES:
        Cv = rng.integers(0, 256, (H, W, dMax), dtype=np.uint8)
        bd, _, _ = X.sgm(Cv, 7, 100, paths)
        obd, _, _ = _oracle_sgm(Cv, 7, 100, paths, None)
        n = int((bd != obd).sum())
        print(f"dMax {dMax} paths {paths} {W}x{H}: bestD differs at {n} of {W * H} pixels ({100.0 * n / (W * H):.1f} %)")
        assert n > 0


# ---- 3. refusals without a device ----
def _host(lib, name="fsgm_sgm_batch_host_exact", prm=None, P1=7, P2=100, Cp=FAKE, bestD=FAKE, minC=FAKE, guide=None):
    return getattr(lib, name)(1, Cp, 32, 24, 16, P1, P2, None if prm is None else C.byref(prm), guide, bestD, minC, None)


def _device(lib, name="fsgm_sgm_device_exact", prm=None, P1=7, P2=100, Cp=FAKE, bestD=FAKE, minC=FAKE, guide=None):
    return getattr(lib, name)(1, Cp, 32, 24, 16, P1, P2, None if prm is None else C.byref(prm), guide, bestD, minC, None, None, None)


@pytest.mark.parametrize("call", [_host, _device], ids=["host", "device"])
def test_exact_entries_refuse_without_a_device(lib, call):
    for P1 in (-1, 256, 1000):
        assert call(lib, P1=P1) == FSGM_ERR_INVALID and "P1 in 0..255" in _err(lib)
    for P2 in (-1, 256, -100):
        assert call(lib, P2=P2) == FSGM_ERR_INVALID and "P2 in 0..255" in _err(lib)
    for mode in range(2, 7):
        p = lib.fsgm_sgm_params_default()
        p.agg_mode = mode
        assert call(lib, prm=p) == FSGM_ERR_UNSUPPORTED and "line kernels" in _err(lib)
    for null in ("Cp", "bestD", "minC"):
        assert call(lib, **{null: None}) == FSGM_ERR_INVALID and "null argument" in _err(lib)
    p = lib.fsgm_sgm_params_default()
    p.reserved[0] = 1                                            # (no reserved word was spent on the switch)
    assert call(lib, prm=p) == FSGM_ERR_INVALID and "reserved" in _err(lib)


FSGM_ERR_HIP = 2


@pytest.mark.parametrize("P1,P2", [(-1, 100), (256, 100), (7, 256), (7, -100), (300, 1000)])
def test_plain_entries_accept_the_penalties_they_always_did(lib, P1, P2):
    """The range check belongs to the exact entries alone.  With penalties that the exact entries refuse, the plain ones get
    past every argument check and stop exactly where they stop with P1 = 7, P2 = 100: without a device at the missing device
    (status 2); with one, the host form runs (status 0) and the device form refuses the pointer that is no device memory."""
    # the host form scans C before it asks for a device: a real volume and real outputs
    Cv = np.zeros((24, 32, 16), np.uint8)
    bd, mc = np.zeros((1, 24, 32), np.uint32), np.zeros((1, 24, 32), np.uint32)
    real = dict(Cp=_lib.ptr(Cv), bestD=_lib.ptr(bd), minC=_lib.ptr(mc))
    assert _host(lib, P1=P1, P2=P2, **real) == FSGM_ERR_INVALID and "0..255" in _err(lib)      # the exact entries refuse them
    assert _device(lib, P1=P1, P2=P2) == FSGM_ERR_INVALID and "0..255" in _err(lib)
    have_device = lib.fsgm_device_count() >= 1
    for P in ((7, 100), (P1, P2)):
        st = _host(lib, "fsgm_sgm_batch_host", P1=P[0], P2=P[1], **real)
        if have_device:
            assert st == 0, _err(lib)
        else:
            assert st == FSGM_ERR_HIP and "no HIP device" in _err(lib)
        st = _device(lib, "fsgm_sgm_device", P1=P[0], P2=P[1])
        if have_device:
            assert st == FSGM_ERR_INVALID and "C (0x1000)" in _err(lib) and "memory" in _err(lib)
        else:
            assert st == FSGM_ERR_HIP and "no HIP device" in _err(lib)


def test_python_wrappers():
    Cv = np.zeros((5, 7, 16), np.uint8)
    with pytest.raises(ValueError, match="arith"):
        sgm_batch(Cv, arith="saturate")
    with pytest.raises(ValueError, match="runner"):
        sgm_batch(Cv, arith="exact", runner_up=True)
    with pytest.raises(_lib.FsgmError) as e:
        sgm_batch(Cv, 7, 256, arith="exact")
    assert e.value.status == FSGM_ERR_INVALID
    with pytest.raises(_lib.FsgmError) as e:
        sgm_batch(Cv, 7, 100, arith="exact", agg_mode=4)
    assert e.value.status == FSGM_ERR_UNSUPPORTED


def test_torch_op_is_registered_and_has_a_fake():
    pytest.importorskip("torch")
    from torch._subclasses.fake_tensor import FakeTensorMode
    from fsgm_amd import torch_ops
    assert hasattr(torch.ops.fsgm, "sgm_exact")
    assert str(torch.ops.fsgm.sgm_exact.default._schema).split("(", 1)[1] == str(torch.ops.fsgm.sgm.default._schema).split("(", 1)[1]
    with FakeTensorMode():
        Cv = torch.empty((3, 16, 9, 33), dtype=torch.uint8, device="cuda")
        r = torch_ops.sgm(Cv, 7, 100, paths=8, arith="exact", return_sum=True, return_status=True)
        assert [(tuple(t.shape), t.dtype) for t in r] == [((3, 9, 33), torch.uint32)] * 2 + [((3, 9, 33, 16), torch.uint32), ((), torch.int32)]
        with pytest.raises(ValueError, match="runner"):
            torch_ops.sgm(Cv, arith="exact", runner_up=True)
        with pytest.raises(ValueError, match="arith"):
            torch_ops.sgm(Cv, arith="exact256")
