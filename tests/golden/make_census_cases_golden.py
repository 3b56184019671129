"""Generates tests/golden/census_ref_cases.npz: the REFERENCE's own census() (common.cpp:3-27,
compiled unmodified into oracle/_ref/ by oracle/Makefile) on the shapes and seeds of
tests/test_oracle_epi.py::test_census_matches_reference_build, so that test holds wherever the
reference tree is absent.  Run where oracle/_ref/ has been built:
    python tests/golden/make_census_cases_golden.py
The fixture holds data only: each input image and the census codes the reference produced."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fsgm_amd import synth          # noqa: E402
from oracle import pyoracle         # noqa: E402

CASES = [(1, 1, 1), (2, 3, 2), (5, 5, 3), (64, 48, 4), (131, 7, 5), (3, 97, 6)]

if __name__ == "__main__":
    assert pyoracle.ref_census_available(), "oracle/_ref not built: run `make -C oracle` where the reference tree is present"
    out = {}
    for (W, H, seed) in CASES:
        img = synth.uniform_u8(seed, (H, W))
        out[f"img_{W}x{H}_{seed}"] = img
        out[f"cen_{W}x{H}_{seed}"] = pyoracle.ref_census(img)
    flat = np.full((9, 11), 77, np.uint8)
    out["img_flat"] = flat
    out["cen_flat"] = pyoracle.ref_census(flat)
    np.savez_compressed(os.path.join(os.path.dirname(__file__), "census_ref_cases.npz"), **out)
    print("wrote census_ref_cases.npz", len(out) // 2, "cases")
