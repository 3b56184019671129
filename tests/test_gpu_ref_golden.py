"""The HIP library against what the reference's own compiled MEX code computed -- the oracle is not in the loop.

Fixtures: tests/golden/ref_mex_<file>.npz hold inputs and the outputs of the reference's mexFunction (a Linux g++ build of the
unmodified sources, tests/golden/make_ref_mex_golden.py).  Every case goes through the public entry points the parity tests use
-- calc_cost_sgm(paths=4), calc_pyd_cost_sgm, calc_pyd_cost_sgm_ng, calc_cost_sgm_ng(rand_stream=the stored libc draws) --, the
neighbour-guided ones under every forced matcher form, the epipolar ones under every aggregation mode of a plan.  Exact equality,
NaN placement included; no pixel is excluded.

Reference-direct cases at full size run when oracle/_ref/ref_*.so came along with the tree (they call the reference on the CPU
through oracle/pyref.py and never read the reference tree); they skip with a reason otherwise."""
import ctypes

import numpy as np
import pytest

from fsgm_amd import synth, EpiPlan, calc_cost_sgm, calc_pyd_cost_sgm, calc_pyd_cost_sgm_ng, calc_cost_sgm_ng
from fsgm_amd._lib import STAGE_ALL
from oracle import pyref
from tests import ref_golden as G

pytestmark = pytest.mark.gpu

# the forced forms of the neighbour-guided aggregation (tests/test_gpu_ng.py); {} = what the library picks itself
NG_FORMS = [{}, {"FSGM_NG_GRID": "1"}, {"FSGM_NG_COMPACT_G": "16"}, {"FSGM_NG_COMPACT_G": "32"}, {"FSGM_NG_COMPACT": "0"},
            {"FSGM_NG_SPLIT": "0"}, {"FSGM_NG_SPLIT": "2"}]
_NG_VARS = ("FSGM_NG_GRID", "FSGM_NG_COMPACT_G", "FSGM_NG_COMPACT", "FSGM_NG_SPLIT")
EPI_MODES = (0, 1, 2, 3, 6, 4, 5)          # EpiPlan.set_agg_mode: a mode whose pipeline does not cover the configuration falls back


def _same(got, want, names, tag=""):
    assert len(got) == len(want) == len(names)
    for g, w, n in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, n
        np.testing.assert_array_equal(g, w, err_msg=f"{n} {tag}")


def _set_form(monkeypatch, form):
    for k in _NG_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in form.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name,i", G.ids("calc_cost_sgm"))
def test_calc_cost_sgm(gpu_lib, name, i):
    c = G.case(name, i)
    D, vMax, P1, P2 = int(c["args"][0]), float(c["args"][1]), int(c["args"][2]), int(c["args"][3])
    want = c["outs"][:2]
    _same(calc_cost_sgm(c["I1"], c["I2"], D, vMax, c["pd0"], c["nd"], c["off"], P1, P2, paths=4), want, ("bestD", "minC"), "host call")
    H, W = c["I1"].shape
    with EpiPlan(W, H, D, 2, paths=4) as plan:                       # two frames: the batched pipelines have a batch to work on
        plan.set_penalties(P1, P2, vMax)
        for f in range(2):
            plan.upload(f, c["I1"], c["I2"], c["pd0"], c["nd"], c["off"])
        for mode in EPI_MODES:
            plan.set_agg_mode(mode)
            plan.run(STAGE_ALL)
            for f in range(2):
                _same(plan.download(f), want, ("bestD", "minC"), f"mode {mode} {plan.kernel_name} frame {f}")


@pytest.mark.parametrize("wide", ["", "0", "2"])
@pytest.mark.parametrize("name,i", G.ids("calc_pyd_cost_sgm"))
def test_calc_pyd_cost_sgm(gpu_lib, monkeypatch, name, i, wide):
    """Under the default and both forced mappings of the row-packed aggregation kernel (FSGM_PYD_WIDE, tests/test_gpu_pyd.py)."""
    c = G.case(name, i)
    monkeypatch.delenv("FSGM_PYD_WIDE", raising=False)
    if wide:
        monkeypatch.setenv("FSGM_PYD_WIDE", wide)
    _same(calc_pyd_cost_sgm(c["I1"], c["I2"], c["preMv"], *G.ints(c["args"])), c["outs"], ("bestD", "minC", "mvSub"))


def _form_id(form):
    return "-".join(f"{k[8:]}{v}" for k, v in form.items()) or "auto"


def _ng_pairs():
    """Every (fixture case, forced form) pair.  The halfSearchWinSize-0 case runs under every form too: with 9 candidates the grid
    kernel is no member of the matcher set (ng_matcher_set), so FSGM_NG_GRID=1 and FSGM_NG_SPLIT=0 run the compact kernel there
    (tests/test_gpu_ng_forms.py names the kernel of every form at that window)."""
    return [pytest.param(name, i, form, id=f"{i}-{_form_id(form)}") for name, i in G.ids("calc_pyd_cost_sgm_ng") for form in NG_FORMS]


@pytest.mark.parametrize("name,i,form", _ng_pairs())
def test_calc_pyd_cost_sgm_ng(gpu_lib, monkeypatch, name, i, form):
    """Every fixture case under every forced matcher form."""
    c = G.case(name, i)
    _set_form(monkeypatch, form)
    _same(calc_pyd_cost_sgm_ng(c["I1"], c["I2"], c["preMv"], *G.ints(c["args"])), c["outs"], ("minC", "flow"))


@pytest.mark.parametrize("exact", ["", "1"])
@pytest.mark.parametrize("name,i", G.ids("calc_cost_sgm_ng"))
def test_calc_cost_sgm_ng(gpu_lib, monkeypatch, name, i, exact):
    """The stored libc draws as rand_stream, in the packed and in the forced exact form of the matcher (FSGM_OTF_EXACT=1)."""
    c = G.case(name, i)
    P1, P2, _ = G.ints(c["args"])
    monkeypatch.delenv("FSGM_OTF_EXACT", raising=False)
    if exact:
        monkeypatch.setenv("FSGM_OTF_EXACT", exact)
    _same(calc_cost_sgm_ng(c["I1"], c["I2"], None, 1, 2, 0, P1, P2, rand_stream=c["rand"]), c["outs"], ("minC", "flow"))


@pytest.mark.parametrize("name,i", G.ids("calc_cost_sgm_ng")[:3])
def test_calc_cost_sgm_ng_through_srand(gpu_lib, name, i):
    """No stream given: the library draws from libc rand() itself, after the srand the fixture records."""
    c = G.case(name, i)
    P1, P2, seed = G.ints(c["args"])
    ctypes.CDLL(None).srand(ctypes.c_uint(seed))
    _same(calc_cost_sgm_ng(c["I1"], c["I2"], None, 1, 2, 0, P1, P2), c["outs"], ("minC", "flow"))


# ------------------------------------------------------------------------------------------------ reference-direct, full size
def _need(name):
    if not pyref.available(name):
        pytest.skip(f"oracle/_ref/ref_{name}.so did not come along with the tree (built only where the reference tree is present)")


def test_calc_cost_sgm_full_size_against_the_reference(gpu_lib):
    """1242x375, D = 128, 4 paths: the host call and a plan in every aggregation mode against the reference's mexFunction."""
    _need("calc_cost_sgm")
    W, H, D = 1242, 375, 128
    I1, I2 = synth.image_pair(W, H, D, seed=2)
    pd0, nd, off = synth.epi_maps(W, H, "general", seed=4)
    (ref, _) = pyref.call_calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, 6, 64)
    _same(calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, 6, 64, paths=4), ref[:2], ("bestD", "minC"), "host call")
    with EpiPlan(W, H, D, 1, paths=4) as plan:
        plan.set_penalties(6, 64, 0.3)
        plan.upload(0, I1, I2, pd0, nd, off)
        for mode in EPI_MODES:
            plan.set_agg_mode(mode)
            plan.run(STAGE_ALL)
            _same(plan.download(0), ref[:2], ("bestD", "minC"), f"mode {mode} {plan.kernel_name}")


def test_config4_single_level_full_size_against_the_reference(gpu_lib, monkeypatch):
    """The config-4 level of tests/test_gpu_configs_full_size.py (1242x375, 81 candidates, hints with regions around +-0x3FF0)
    against the reference's mexFunction: what the library picks, the grid form forced, and the compact kernel taken out."""
    _need("calc_pyd_cost_sgm_ng")
    from tests.test_gpu_configs_full_size import _smooth_hints
    W, H = 1242, 375
    I1, I2 = synth.image_pair(W, H, 16, seed=41)
    mv = _smooth_hints(W, H, 1, big=True)
    (ref, _) = pyref.call_calc_pyd_cost_sgm_ng(I1, I2, mv, 1, 2, 1, 6, 32)
    for form in ({}, {"FSGM_NG_GRID": "1"}, {"FSGM_NG_COMPACT": "0"}):
        _set_form(monkeypatch, form)
        _same(calc_pyd_cost_sgm_ng(I1, I2, mv, 1, 2, 1, 6, 32), ref, ("minC", "flow"), str(form))
