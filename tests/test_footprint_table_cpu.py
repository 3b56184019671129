"""Coverage of tests/test_gpu_footprint.py is a condition: every device-pointer function of include/fsgm.h is in
tests/footprint_table.py (checked here without the built library), and the GPU file's rows cover exactly that table.  Also the
arena's placement rule, and the fact it rests on: every row of every entry's check table aligns a pointer on its element size."""
import glob
import os
import re

import pytest

from tests import footprint as F
from tests.footprint_table import DEVICE_ENTRIES, NOT_DEVICE_POINTER_ENTRIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fsgm.h")


def device_entries(text):
    """every function whose name matches fsgm_\\w+_device\\w*, the *_batch_devices_host forms (host memory) left out"""
    names = set(re.findall(r"\b(fsgm_\w+_device\w*)\s*\(", text))
    return sorted(n for n in names if not n.endswith("_batch_devices_host") and n not in NOT_DEVICE_POINTER_ENTRIES)


def test_every_device_entry_is_in_the_table():
    with open(HEADER) as f:
        declared = device_entries(f.read())
    assert "fsgm_sgm_device" in declared and "fsgm_vmf_device" in declared           # (the pattern still finds them)
    missing = [n for n in declared if n not in DEVICE_ENTRIES]
    assert not missing, f"device entries of include/fsgm.h without a footprint case (tests/footprint_table.py, tests/test_gpu_footprint.py): {missing}"
    unknown = [n for n in DEVICE_ENTRIES if n not in declared]
    assert not unknown, f"tests/footprint_table.py names functions that include/fsgm.h does not declare: {unknown}"


def test_the_gpu_rows_cover_the_table():
    from tests import test_gpu_footprint                                           # (asserts the same on import)
    assert test_gpu_footprint.ENTRIES == sorted(DEVICE_ENTRIES)


def test_a_missing_row_is_named():
    text = "fsgm_status fsgm_new_thing_device_x(int32_t n);\nfsgm_status fsgm_a_batch_devices_host(int n);\nint32_t fsgm_device_count(void);"
    assert device_entries(text) == ["fsgm_new_thing_device_x"]


# the element size behind every name a check table uses; disp / disp2 are u32 / i32 maps in the matchers and f64 maps in the chains
ESIZE = {1: {"I0", "I1", "I2", "C", "conf", "guide"},
         4: {"bestD", "bestD2", "minC", "minC2", "S", "status", "disp", "disp2"},
         8: {"D1", "D2", "O", "Pd0", "b", "f", "disp", "disp2", "disp_checked", "disp_pp", "filterD1", "filterD2", "flow", "flow2", "flowMed",
             "flow_bwd", "flow_checked", "flow_fwd", "flow_pp", "map", "mvSub", "next", "normDir", "normDirect", "offset", "out",
             "pixelPosD0", "preMv", "D1checked", "D2out", "flowFiltered", "flowFilled", "fChecked", "mv"}}
ROW = re.compile(r',\s*(\d+),\s*[^,{}]+,\s*"(\w+)"\}')


def test_every_check_table_aligns_on_the_element_size():
    """the `minimal` placement starts a tensor on its element size: that is every DevicePtr row's `align` only while this holds"""
    rows = []
    for path in sorted(glob.glob(os.path.join(ROOT, "fsgm_amd", "csrc", "*.h*"))):
        with open(path) as f:
            text = f.read()
        if "device_check_args" in text:
            rows += [(os.path.basename(path), int(a), name) for a, name in ROW.findall(text)]
    assert len(rows) >= 60, len(rows)                                              # (the pattern still finds the tables)
    for path, align, name in rows:
        sizes = [e for e, names in ESIZE.items() if name in names]
        assert sizes, f"{path}: a check-table row for {name!r}, whose element size this test does not know: add it to ESIZE"
        assert align in sizes, f"{path}: {name} is aligned on {align}, its element size is {sizes}: tests/footprint.py places it on the element size"


@pytest.mark.parametrize("esize", [1, 4, 8])
@pytest.mark.parametrize("nbytes_in_elements", [1, 2, 3, 4, 5, 8, 15, 16, 17, 407, 4096])
@pytest.mark.parametrize("cursor", [65536, 65537, 65540, 65544, 65551, 70000])
def test_minimal_placement(esize, nbytes_in_elements, cursor):
    nbytes = nbytes_in_elements * esize
    s = F.place(cursor, nbytes, esize, "minimal")
    assert cursor <= s < cursor + 64 and s % esize == 0 and s % (2 * esize) != 0
    if esize < 8 or nbytes % 16 == 0:
        assert (s + nbytes) % 16 != 0
    assert F.place(cursor, nbytes, esize, "aligned") % 256 == 0
