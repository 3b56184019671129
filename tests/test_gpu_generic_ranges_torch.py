"""torch_ops.calc_cost_sgm at a disparity range of the generic kernels (300): a batch of two on the caller's stream equals the numpy
path.  (A file of its own: torch is imported before the library is loaded.)"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth  # noqa: E402  (torch first, then the library)
from fsgm_amd.epi import auto_pipeline  # noqa: E402

pytestmark = pytest.mark.gpu


def test_torch_calc_cost_sgm_batch_of_two_on_a_side_stream_equals_the_numpy_path(gpu_lib):
    W, H, D = 37, 21, 300
    frames = [synth.image_pair(W, H, D, seed=70 + f) + synth.epi_maps(W, H, "general", seed=7 + f) for f in range(2)]
    assert auto_pipeline(W, H, D, 2, 8, 6, 64) == "generic"
    want = fsgm_amd.calc_cost_sgm_batch(frames, D, 0.3, 6, 64, paths=8, fb_check=1)
    host = [torch.from_numpy(np.stack([fr[k] for fr in frames])) for k in range(5)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                   # inputs, the op and a consumer on s, nothing in between
        I1, I2, pd0, nd, off = (h.to("cuda:0") for h in host)
        got = torch_ops.calc_cost_sgm(I1, I2, D, 0.3, pd0, nd, off, 6, 64, paths=8, fb_check=1, return_status=True)
        copies = [g.clone() for g in got]
    s.synchronize()
    assert len(got) == 5 and int(copies[4].item()) == 0
    for k, name in enumerate(("bestD", "minC", "conf", "bestD2")):
        assert got[k].is_cuda and got[k].shape == (2, H, W)
        for f in range(2):
            np.testing.assert_array_equal(copies[k][f].cpu().numpy(), want[f][k], err_msg=f"{name} of frame {f}")
    assert (want[0][1] != want[1][1]).any()                      # two distinct frames
