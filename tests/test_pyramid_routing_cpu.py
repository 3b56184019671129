"""Which C entry the pyramid one-shots reach, against a stub in place of the loaded library: a call with every newer switch off
touches the plain entry alone (so it also runs on an older build behind FSGM_LIB_PATH, which has none of the others), runner_up /
uniqueness_ratio alone take _ru / _u, level_median takes _lm.  No GPU, no library call."""
import numpy as np
import pytest

import fsgm_amd
from fsgm_amd import _lib, pyramid

PYD, NG, PP = "fsgm_pyramidal_sgm_host", "fsgm_pyramidal_sgm_ng_host", "fsgm_pyramidal_flow_pp_host"
NEWER = (PYD + "_ru", PYD + "_lm", NG + "_ru", NG + "_lm", PP + "_u", PP + "_lm")
# the number of arguments of each entry (include/fsgm.h)
ARGS = {PYD: 9, PYD + "_ru": 10, PYD + "_lm": 11, NG: 9, NG + "_ru": 10, NG + "_lm": 11, PP: 12, PP + "_u": 14, PP + "_lm": 15}


class StubLib:
    """Entry points that record their name and argument count and return 0; marked as bound, so no argument types are declared."""
    _pyramid_bound = _ng_pyramid_bound = _flow_pp_bound = True
    fsgm_pyramid_params_default = staticmethod(pyramid.PyramidParams)
    fsgm_ng_pyramid_params_default = staticmethod(pyramid.NgPyramidParams)

    def __init__(self, entries):
        self.calls = []
        for name in entries:
            setattr(self, name, lambda *a, _name=name: self.calls.append((_name, len(a))) or 0)

    @staticmethod
    def fsgm_flow_pp_params_default(matcher):
        return pyramid.FlowPPParams(matcher=matcher)


@pytest.fixture
def stub(monkeypatch):
    def install(entries):
        lib = StubLib(entries)
        monkeypatch.setattr(_lib, "load", lambda: lib)
        return lib
    return install


I = np.zeros((8, 8), np.uint8)
ONE_SHOTS = ((fsgm_amd.pyramidal_sgm, PYD, "_ru", "runner_up", True), (fsgm_amd.pyramidal_sgm_ng, NG, "_ru", "runner_up", True),
             (fsgm_amd.pyramidal_flow_pp, PP, "_u", "uniqueness_ratio", 5))


@pytest.mark.parametrize("fn,plain,second,keyword,value", ONE_SHOTS)
def test_a_plain_call_reaches_the_plain_entry_alone(stub, fn, plain, second, keyword, value):
    lib = stub((PYD, NG, PP))                                    # an older build: none of the newer entries
    assert not any(hasattr(lib, name) for name in NEWER)
    res = fn(I, I, 2)
    assert lib.calls == [(plain, ARGS[plain])]
    assert len(res) == (5 if plain == PP else 3)
    lib.calls.clear()
    fn(I, I, 2, level_median=0)                                  # the switch named but off
    assert lib.calls == [(plain, ARGS[plain])]


@pytest.mark.parametrize("fn,plain,second,keyword,value", ONE_SHOTS)
def test_each_switch_reaches_its_own_entry(stub, fn, plain, second, keyword, value):
    lib = stub((PYD, NG, PP) + NEWER)
    for kw, suffix, extra in (({}, "", 0), ({keyword: value}, second, 1), ({"level_median": 3}, "_lm", 0),
                              ({"level_median": 3, keyword: value}, "_lm", 1), ({"level_median": 5, keyword: value}, "_lm", 1)):
        lib.calls.clear()
        res = fn(I, I, 2, **kw)
        assert lib.calls == [(plain + suffix, ARGS[plain + suffix])], kw
        assert len(res) == (5 if plain == PP else 3) + extra, kw
