"""GPU tests of the torch ops of the median between pyramid levels: on a side stream, outputs left on the device, equal to the
host forms (which tests/test_gpu_level_median.py pins to the restatement), with and without a leading batch dimension."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops  # noqa: E402  (torch first, then the library)
from tests import edge_inputs as E  # noqa: E402
from tests import level_median_restatement as LM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, NUMPYD = 61, 47, 3


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    np.testing.assert_array_equal(np.nan_to_num(got), np.nan_to_num(want), err_msg=what)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _pairs(ch, n=2):
    pairs = [E.image_pair(E.rng(11 + k), W, H, ch, seed=11 + k) for k in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.mark.parametrize("s", [3, 5])
def test_flow_level_hints_on_a_side_stream(gpu_lib, s):
    flows = E.vmf_flows(E.rng(40 + s), 65, 5, 3, 2)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = _t(flows) + 0.0                                      # produced by a kernel on the stream
        got = torch_ops.flow_level_hints(d, s)
        one = torch_ops.flow_level_hints(d[1], s)
        plain = torch_ops.flow_level_hints(d, 0)
        nans = torch.isnan(got).sum()                            # consumed by a kernel on the stream
    stream.synchronize()
    assert got.is_cuda and tuple(got.shape) == (3, 2, 10, 130)
    want = np.stack([LM.level_hints(f, s) for f in flows])
    _same(_n(got), want)
    _same(_n(one), want[1])
    _same(_n(plain), 2.0 * np.repeat(np.repeat(flows, 2, axis=2), 2, axis=3))
    assert int(nans) == int(np.isnan(want).sum())


@pytest.mark.parametrize("matcher", ["pyd", "ng"])
def test_pyramids_on_a_side_stream(gpu_lib, matcher):
    host_fn = fsgm_amd.pyramidal_sgm if matcher == "pyd" else fsgm_amd.pyramidal_sgm_ng
    op = torch_ops.pyramidal_sgm if matcher == "pyd" else torch_ops.pyramidal_sgm_ng
    I0, I1 = _pairs(1)
    want = [host_fn(a, b, NUMPYD, level_median=3, runner_up=True) for a, b in zip(I0, I1)]
    off = host_fn(I0[0], I1[0], NUMPYD)
    assert (want[0][0] != off[0]).any()                          # the median changes level 1 of this pair
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d0 = (_t(I0).to(torch.int16) + 0).to(torch.uint8)        # produced by kernels on the stream
        flow, minC, status = op(d0, _t(I1), NUMPYD, level_median=3, return_status=True)
        flow_ru, minC_ru, minC2 = op(d0, _t(I1), NUMPYD, level_median=3, runner_up=True)
        plain = op(d0, _t(I1), NUMPYD)
        total = minC.to(torch.int64).sum()                       # consumed by a kernel on the stream (integers: no summation order)
    stream.synchronize()
    assert flow.is_cuda and int(status.item()) == 0 and tuple(flow.shape) == (2, 2, H, W)
    for k in range(2):
        np.testing.assert_array_equal(_n(flow[k]), want[k][0])
        np.testing.assert_array_equal(_n(minC[k]), want[k][2])
        np.testing.assert_array_equal(_n(flow_ru[k]), want[k][0])
        np.testing.assert_array_equal(_n(minC_ru[k]), want[k][2])
        np.testing.assert_array_equal(_n(minC2[k]), want[k][3])
    assert int(total) == int(sum(w[2].astype(np.int64).sum() for w in want))
    np.testing.assert_array_equal(_n(plain[0][0]), off[0])       # the plain op keeps its own plan
    one = op(_t(I0[1]), _t(I1[1]), NUMPYD, level_median=3, check=True)
    np.testing.assert_array_equal(_n(one[0]), want[1][0])


@pytest.mark.parametrize("ratio", [None, 15])
@pytest.mark.parametrize("matcher", ["pyd", "ng"])
def test_flow_pp_on_a_side_stream(gpu_lib, matcher, ratio):
    I0, I1 = _pairs(3)
    kw = {} if ratio is None else {"uniqueness_ratio": ratio}
    host = fsgm_amd.pyramidal_flow_pp(I0, I1, NUMPYD, matcher, level_median=3, **kw)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = torch_ops.pyramidal_flow_pp(_t(I0), _t(I1), NUMPYD, matcher, level_median=3, return_status=True, **kw)
        one = torch_ops.pyramidal_flow_pp(_t(I0[0]), _t(I1[0]), NUMPYD, matcher, level_median=3, **kw)
    stream.synchronize()
    assert int(dev[-1].item()) == 0 and len(dev) - 1 == len(host) == (5 if ratio is None else 6)
    for g, o, w in zip(dev[:-1], one, host):
        assert g.is_cuda
        _same(_n(g), w)
        _same(_n(o), w[0])
