"""The body of tests/test_gpu_resize_filters.py::test_decode_to_tensors_with_resample, run as a program in a process of its own: torch is
imported FIRST, so that this process has one HIP runtime (torch's, where torch ships one) for torch and for libjpegdec_amd.so alike.
decode_to_tensors(size=..., resample=...) against the numpy twin of Pillow's filters (tests/resize_filter_util.py) over the oracle's canvas;
prints "resize_filters_torch_child ok"."""
import os
import sys

import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from oracle.loader import OracleDecoder  # noqa: E402
from tests import resize_filter_util as F  # noqa: E402
from tests.cases import jpeg_for  # noqa: E402
from tests.test_gpu_resize import visible_pixels  # noqa: E402

H, W = 24, 24


def launches(signed):
    return sum(v for k, v in J.kernel_launch_counts().items() if "jda_resize_tiles" in k and ("jda_resize_tiles_signed" in k) == signed)


def main():
    oracle = OracleDecoder()
    ctx = J.Context(0)
    names = ("c420_333x217", "c440_200x120", "c444_384x192_q100_rst7")
    files = [jpeg_for(n) for n in names]
    vis = [visible_pixels(oracle, f, J.RGB8888, 0) for f in files]
    crops = [(10, 20, 300, 150), (0, 0, 200, 120), (300, 100, 40, 60)]
    for resample, f, signed in (("bicubic", F.BICUBIC, True), (J.RESIZE_LANCZOS, F.LANCZOS, True), ("Hamming", F.HAMMING, False), ("box", F.BOX, False)):
        before = launches(True), launches(False)
        t = J.decode_to_tensors(ctx, files, size=(H, W), resample=resample)
        assert isinstance(t, torch.Tensor) and tuple(t.shape) == (3, 3, H, W) and t.dtype == torch.uint8
        assert (launches(True) - before[0], launches(False) - before[1]) == ((1, 0) if signed else (0, 1)), resample
        host = t.cpu().numpy()
        for k in range(3):
            assert np.array_equal(host[k], F.resize(vis[k], W, H, None, f)[:, :, :3].transpose(2, 0, 1)), (resample, names[k])
        t = J.decode_to_tensors(ctx, files, layout="HWC", size=(H, W), crops=crops, resample=resample)
        host = t.cpu().numpy()
        for k in range(3):
            assert np.array_equal(host[k], F.resize(vis[k], W, H, crops[k], f)[:, :, :3]), (resample, names[k])
    # the default is the triangle, as before the argument was there
    a, b = J.decode_to_tensors(ctx, files, size=(H, W)), J.decode_to_tensors(ctx, files, size=(H, W), resample="bilinear")
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy()[0], F.resize(vis[0], W, H, None, F.BILINEAR)[:, :, :3].transpose(2, 0, 1))
    # a ratio beyond the filter's cap (217 rows to 5 is 43 : 1; the triangle's is 80 : 1): the library's code
    J.decode_to_tensors(ctx, files[:1], size=(5, W))
    try:
        J.decode_to_tensors(ctx, files[:1], size=(5, W), resample="bicubic")
    except J.JdaError as e:
        assert e.code == 3, e.code
    else:
        raise AssertionError("not refused")
    ctx.close()
    print("resize_filters_torch_child ok")


if __name__ == "__main__":
    main()
