"""The fsgm_view2:: ops behind torch_ops.sgm(second_view=True), torch_ops.stereo_sgm(second_view=True) and torch_ops.view2_check, on a
side stream: bit for bit the numpy forms' outputs, which tests/test_gpu_view2.py ties to the restatement; the other outputs those
of the ops without the switch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fsgm_amd  # noqa: E402  (torch first, then the library)
from fsgm_amd import torch_ops, synth  # noqa: E402
from tests.view2_restatement import check_sgm, check_true, view2 as restate  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("D,W,layout,kw", [
    (48, 70, "dhw", dict(paths=8, runner_up=True)),
    (128, 131, "hwd", dict(arith="exact", direction=1, d_min=5, max_diff=100)),
    (272, 67, "dhw", dict(direction=-1, d_min=-3, subpixel=0)),
    (16, 257, "dhw", dict(adaptive_p2=1, paths=8, d_min=5)),
])
def test_sgm_op(D, W, layout, kw):
    n, H = 2, 3
    rng = np.random.default_rng(D + W)
    Cv = rng.integers(0, 256 if kw.get("arith") else 25, (n, H, W, D), dtype=np.uint8)
    P = (7, 255) if kw.get("arith") else (6, 64)
    guide = rng.integers(0, 256, (n, H, W), dtype=np.uint8) if kw.get("adaptive_p2") else None
    nkw = dict(kw, layout=layout, guide=guide, return_sum=True)
    vol = Cv if layout == "hwd" else np.ascontiguousarray(Cv.transpose(0, 3, 1, 2))
    want = fsgm_amd.sgm_batch(vol, *P, second_view=True, **nkw)
    tkw = dict(nkw, guide=None if guide is None else torch.from_numpy(guide).to(DEV))
    view = {k: tkw.pop(k) for k in ("direction", "d_min", "max_diff") if k in tkw}
    stream = torch.cuda.Stream(device=DEV)
    dC = torch.from_numpy(vol).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got = torch_ops.sgm(dC, *P, second_view=True, check=True, **tkw, **view)
        plain = torch_ops.sgm(dC, *P, check=True, **tkw)
    stream.synchronize()
    assert len(got) == len(want) == len(plain) + 3
    for a, b in zip(want, got):
        assert np.array_equal(a, host(b))
    for a, b in zip(plain, got):
        assert torch.equal(a, b)
    S, disp2, mv, conf = host(got[len(plain) - 1]), host(got[-3]), host(got[-2]), host(got[-1])
    rd2, rmc = restate(S, view.get("direction", -1), view.get("d_min", 0), kw.get("subpixel", 1))
    assert np.array_equal(disp2, rd2) and np.array_equal(mv, rmc)
    assert np.array_equal(conf, check_sgm(host(got[0]), disp2, view.get("direction", -1), view.get("d_min", 0), view.get("max_diff", 256),
                                          kw.get("subpixel", 1)))
    one = torch_ops.sgm(dC[0], *P, second_view=True, **tkw | ({"guide": tkw["guide"][0]} if guide is not None else {}), **view)
    for a, b in zip(got, one):
        assert torch.equal(a[0], b)


@pytest.mark.parametrize("direction,d_min,runner_up", [(-1, None, False), (1, 5, True), (-1, -3, True)])
def test_stereo_op_and_check(direction, d_min, runner_up):
    W, H, D = 61, 47, 24
    pairs = [synth.image_pair(W, H, D, seed=s) for s in (3, 4)]
    I1, I2 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    kw = dict(paths=8, direction=direction, d_min=d_min, runner_up=runner_up)
    want = fsgm_amd.stereo_sgm(I1, I2, D, 6, 64, second_view=True, max_diff=300, **kw)
    a, b = torch.from_numpy(I1).to(DEV), torch.from_numpy(I2).to(DEV)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got = torch_ops.stereo_sgm(a, b, D, 6, 64, second_view=True, max_diff=300, check=True, **kw)
        conf = torch_ops.view2_check(got[0], got[-3], direction=direction, max_diff=300)
        one = torch_ops.view2_check(got[0][1], got[-3][1], direction=direction, max_diff=300)
    stream.synchronize()
    assert len(got) == len(want)
    for x, y in zip(want, got):
        assert x.dtype == host(y).dtype and np.array_equal(x, host(y))
    assert torch.equal(conf, got[-1]) and torch.equal(one, conf[1])
    assert np.array_equal(host(conf), check_true(host(got[0]), host(got[-3]), direction, 300))
    assert host(conf).any() and not host(conf).all()
