"""CPU tests of adaptive P2 for the 1-D matcher: the numpy restatement (tests/adaptive_p2_restatement.py) against the
reference's own code compiled with `adpativeP2` / `enableDiagnalPath` set (tests/golden/ref_mex_calc_cost_sgm_adaptive.npz),
against the unchanged oracle with the flag off, the fixture's 8-path pin of the oracle, the new options struct, and the Python
keyword reaching the library -- all without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import _lib, synth
from oracle import pyoracle, pyref
from tests import adaptive_p2_restatement as A
from tests import stereo_restatement as SR

HERE = os.path.dirname(os.path.abspath(__file__))
N_CASES = A.golden_count()
CASES = [A.golden_case(i) for i in range(N_CASES)]
IDS = [c["id"] for c, _ in CASES]


def test_fixture_holds_the_cases_the_kernels_can_go_wrong_at():
    variants = {(c["linear"], c["paths"], c["adaptive"]) for c, _ in CASES}
    assert variants == {(0, 4, 1), (0, 8, 1), (1, 4, 1), (1, 8, 1), (0, 8, 0), (1, 8, 0)}
    shapes = {(c["I1"].shape[1], c["I1"].shape[0], c["D"], c["P1"], c["P2"]) for c, _ in CASES}
    for want in ((24, 16, 16, 6, 64), (33, 9, 32, 6, 64), (17, 11, 64, 6, 32), (150, 4, 128, 6, 64), (37, 21, 16, 6, 35),
                 (16, 10, 20, 100, 200), (20, 12, 16, 255, 0), (1, 9, 16, 6, 64), (9, 1, 16, 6, 64), (5, 7, 16, 6, 64)):
        assert want in shapes, want
    assert any("flat" in s for s in IDS) and any("stripes" in s for s in IDS)
    for c, _ in CASES:
        if "stripes" in c["id"]:
            assert (np.abs(np.diff(c["I1"].astype(int), axis=1)) > A.THRESHOLD).all()           # every horizontal step adaptive
        if "flat" in c["id"]:
            assert np.ptp(c["I1"]) == 0
    path = os.path.join(HERE, "golden")
    assert os.path.getsize(A.GOLDEN_PATH) <= os.path.getsize(os.path.join(path, "ref_mex_calc_cost_sgm.npz"))


@pytest.mark.parametrize("i", range(N_CASES), ids=IDS)
def test_restatement_matches_the_reference_built_with_the_flags(i):
    c, (bestD, minC, conf, bestD2) = CASES[i]
    rb, rm = A.restate(c)
    assert np.array_equal(rm, minC), c["id"]
    assert np.array_equal(rb, bestD), c["id"]                    # every pixel
    assert not conf.any() and not bestD2.any()                   # the reference's check is commented out (:589-590)


def test_adaptive_changes_the_fixture_frames_and_nothing_without_an_edge():
    by = {(c["frame"], c["linear"], c["paths"], c["adaptive"]): o for c, o in CASES}
    changed = 0
    for (j, lin, paths, ad), o in by.items():
        off = by.get((j, lin, paths, 0))
        if ad and off is not None:
            same = all(np.array_equal(x, y) for x, y in zip(o, off))
            flat = "flat" in next(c["id"] for c, _ in CASES if c["frame"] == j)
            assert same == flat, (j, lin, paths)
            changed += not same
    assert changed >= 2


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("W,H,D,P1,P2", [(24, 16, 16, 6, 64), (16, 10, 20, 100, 200), (9, 1, 16, 6, 64), (1, 9, 16, 255, 0)])
def test_restatement_with_the_flag_off_is_the_oracle(W, H, D, P1, P2, paths):
    I1, I2 = synth.image_pair(W, H, D, seed=W)
    pd0, nd, off = synth.epi_maps(W, H, "general")
    bd, mc = A.calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, P1, P2, paths=paths, adaptive=0)
    rbd, rmc = pyoracle.calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, P1, P2, paths)
    assert np.array_equal(mc, rmc) and np.array_equal(bd, rbd)
    Cv = pyoracle.epi_cost(I1, I2, D, 0.3, pd0, nd, off)
    assert np.array_equal(A.aggregate(Cv, I1, P1, P2, paths, 0), pyoracle.epi_aggregate(Cv, P1, P2, paths))


@pytest.mark.parametrize("i", [i for i in range(N_CASES) if not CASES[i][0]["adaptive"]], ids=lambda i: IDS[i])
def test_fixture_pins_the_oracles_eight_paths(i):
    c, (bestD, minC, _, _) = CASES[i]
    assert c["paths"] == 8
    if c["linear"]:
        bd, mc = SR.calc_cost_sgm_linear(c["I1"], c["I2"], c["D"], c["pd0"], c["nd"], c["P1"], c["P2"], paths=8)
    else:
        bd, mc = pyoracle.calc_cost_sgm(c["I1"], c["I2"], c["D"], c["vMax"], c["pd0"], c["nd"], c["off"], c["P1"], c["P2"], 8)
    assert np.array_equal(mc, minC) and np.array_equal(bd, bestD)


def test_c_div_truncates_like_c():
    assert [A.c_div(v, 8) for v in (64, 35, 7, 0, -7, -8, -9, -35)] == [8, 4, 0, 0, 0, -1, -1, -4]


@pytest.mark.parametrize("seed", [101, 202])
def test_live_reference_on_fresh_seeds(seed):
    """where oracle/_ref and the reference tree are present: the builds of the fixture's generator, made afresh"""
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location("make_ref_adaptive_golden", os.path.join(HERE, "golden", "make_ref_adaptive_golden.py"))
    if not pyref.available("calc_cost_sgm"):
        pytest.skip("oracle/_ref is not built")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if not os.path.exists(os.path.join(gen.lin.REF, "calc_cost_sgm.cpp")):
        pytest.skip("the reference tree is not present")
    W, H, D = 21, 13, 32
    I1, I2 = synth.image_pair(W, H, D, seed=seed)
    pd0, nd, off = synth.epi_maps(W, H, "general", seed=seed)
    with tempfile.TemporaryDirectory(prefix="fsgm_ref_adaptive_live_") as tmp:
        for variant in (gen.VZ8A, gen.LIN4A):
            tag, so = gen.build(tmp, variant)
            (bestD, minC, _, _), _ = gen.call(f"live{seed}_{tag}", so, I1, I2, D, pd0, nd, 6, 64, 0.3, off)
            c = dict(I1=I1, I2=I2, D=D, vMax=0.3, pd0=pd0, nd=nd, off=off, P1=6, P2=64, linear=variant[0], paths=variant[1], adaptive=1)
            rb, rm = A.restate(c)
            assert np.array_equal(rm, minC) and np.array_equal(rb, bestD), variant


def test_structs_keep_their_size_and_the_options_struct_is_32_bytes():
    lib = _lib.load()
    assert C.sizeof(_lib.EpiParams) == 20 and C.sizeof(_lib.StereoParams) == 20
    assert C.sizeof(_lib.EpiOptions) == 32
    assert [f[0] for f in _lib.EpiOptions._fields_] == ["adaptive_p2", "reserved"]
    o = lib.fsgm_epi_options_default()
    assert o.adaptive_p2 == 0 and not any(o.reserved)


def test_new_entry_points_validate_before_touching_a_device():
    lib = _lib.load()
    assert lib.fsgm_calc_cost_sgm_host_opts(None, None, None, None) == 1
    assert lib.fsgm_calc_cost_sgm_linear_batch_host_opts(0, None, None, None, None) == 1
    assert lib.fsgm_epi_plan_set_adaptive_p2(None, 1) == 1
    I = np.zeros((4, 5), np.uint8)
    o = np.zeros((4, 5), np.uint32)
    opt = _lib.options(2)
    args = (1, _lib.ptr(I), _lib.ptr(I), 5, 4, 16, 6, 64, None)
    assert lib.fsgm_stereo_sgm_host_opts(*args, C.byref(opt), _lib.ptr(o), _lib.ptr(o), None, None) == 1
    assert b"adaptive_p2" in lib.fsgm_last_error()
    opt = _lib.options(1)
    opt.reserved[3] = 1
    assert lib.fsgm_stereo_sgm_host_opts(*args, C.byref(opt), _lib.ptr(o), _lib.ptr(o), None, None) == 1
    assert b"reserved" in lib.fsgm_last_error()
    # the answer of auto mode, no device needed: 40 frames go to a fused pipeline, adaptive ones stay on the line kernels
    assert fsgm_amd.epi.auto_pipeline(1242, 375, 128, 40, paths=8) not in ("packed16/nowrap", "packed16/wrap", "generic")
    assert fsgm_amd.epi.auto_pipeline(1242, 375, 128, 40, paths=8, adaptive_p2=1) == "packed16/nowrap"
    assert fsgm_amd.epi.auto_pipeline(1242, 375, 128, 40, paths=4, P1=100, P2=200, adaptive_p2=1) == "packed16/wrap"
    assert fsgm_amd.epi.auto_pipeline(64, 48, 20, 40, adaptive_p2=1) == "generic"


def test_python_keyword_reaches_the_library():
    """adaptive_p2=2 passes every Python check and is refused by the library's own (status 1, before a device is touched)"""
    I1, I2 = synth.image_pair(12, 8, 16)
    pd0, nd, off = synth.epi_maps(12, 8)
    for call in (lambda: fsgm_amd.calc_cost_sgm(I1, I2, 16, 0.3, pd0, nd, off, 6, 64, adaptive_p2=2),
                 lambda: fsgm_amd.calc_cost_sgm_linear(I1, I2, 16, pd0, nd, 6, 64, adaptive_p2=2),
                 lambda: fsgm_amd.stereo_sgm(I1, I2, 16, adaptive_p2=2)):
        with pytest.raises(_lib.FsgmError, match="adaptive_p2") as e:
            call()
        assert e.value.status == 1
    with pytest.raises(ValueError, match="device list"):
        fsgm_amd.epi.calc_cost_sgm_batch([(I1, I2, pd0, nd, off)], 16, 0.3, 6, 64, devices=[0], adaptive_p2=1)
