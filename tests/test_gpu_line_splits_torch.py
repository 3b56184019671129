"""torch_ops.stereo_sgm at a disparity range of the 12-costs-a-lane split (96): a batch of two on the GPU equals the numpy path.
(A file of its own: torch is imported before the library is loaded.)"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402
from fsgm_amd import torch_ops, synth  # noqa: E402  (torch first, then the library)
from fsgm_amd.epi import auto_pipeline  # noqa: E402

pytestmark = pytest.mark.gpu


def test_torch_stereo_sgm_batch_of_two_equals_the_numpy_path(gpu_lib):
    W, H, D = 40, 12, 96
    pairs = [synth.image_pair(W, H, 16, seed=60 + f) for f in range(2)]
    L, Rt = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    assert auto_pipeline(W, H, D, 2, 8, 6, 64) == "packed16/nowrap"
    want = fsgm_amd.stereo_sgm(L, Rt, D, paths=8, fb_check=1)
    got = torch_ops.stereo_sgm(torch.from_numpy(L).to("cuda:0"), torch.from_numpy(Rt).to("cuda:0"), D, paths=8, fb_check=1, check=True)
    assert len(got) == len(want) == 4
    for k in range(4):
        assert got[k].is_cuda and got[k].shape == (2, H, W)
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg=f"output {k}")
    assert (want[0][0] != want[0][1]).any()                      # two distinct frames
