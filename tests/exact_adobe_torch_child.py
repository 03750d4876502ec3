"""The body of tests/test_gpu_exact_adobe.py::test_decode_to_tensors_with_colour_models_is_pillow, run as a program in a process of its own:
torch is imported FIRST, so that this process has one HIP runtime for torch and for libjpegdec_amd.so alike.
decode_to_tensors(files, size=(32, 32), resample="bicubic", decoder="libjpeg", colour_models=True) over a mixed list -- gray, YCbCr,
Photoshop's Adobe transform 1, RGB-coded, CMYK and YCCK files, baseline and progressive -- against Pillow itself:
Image.open(f).convert("RGB").resize((32, 32), Image.BICUBIC), bit for bit; prints "exact adobe tensors ok"."""
import io
import os
import sys

import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from tests import exact_adobe_util as A  # noqa: E402
from tests import exact_util as X  # noqa: E402


def main():
    ctx = J.Context(0)
    c420, c422, c440 = dict(A.grid4("4:2:0")), dict(A.grid4("4:2:2")), dict(A.grid4("4:4:0"))
    files = [dict(X.grid("gray"))["baseline_33x31_q90"], dict(X.grid("4:2:0"))["progressive_75x53_q30"], A.pillow_rgb3(45, 53, "4:2:0", 75, "adobe1"),
             A.pillow_rgb3(33, 31, "4:2:2", 90, "adobe0", True), A.pillow_rgb3(64, 48, "4:4:4", 75, "ids"), A.pillow_rgb3(17, 9, "4:2:0", 90, "both")]
    files += [f for nm, f in c420.items() if "75x53" in nm or "45x53" in nm] + [f for nm, f in c422.items() if "64x48" in nm] + [f for nm, f in c440.items() if "33x31" in nm]
    models = {A.model(f) for f in files}
    assert models == {A.GRAY, A.YCBCR, A.RGB, A.CMYK, A.YCCK}, models
    assert {A.header(f)["sof"] for f in files if A.header(f)["ncomp"] == 4} >= {0xC0, 0xC2}
    t = J.decode_to_tensors(ctx, files, size=(32, 32), resample="bicubic", decoder="libjpeg", colour_models=True)
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (len(files), 3, 32, 32) and t.dtype == torch.uint8
    host = t.cpu().numpy()
    for k, f in enumerate(files):
        want = np.asarray(Image.open(io.BytesIO(f)).convert("RGB").resize((32, 32), Image.BICUBIC))
        assert np.array_equal(host[k].transpose(1, 2, 0), want), (k, A.model(f), int(np.count_nonzero(host[k].transpose(1, 2, 0) != want)))
    # without size=: the decoded pixels themselves, a tensor a file
    ts = J.decode_to_tensors(ctx, files, layout="HWC", decoder="libjpeg", colour_models=True)
    for k, f in enumerate(files):
        assert np.array_equal(ts[k].cpu().numpy(), A.pillow(f, "RGB")), k
    # without colour_models the list is refused as ever: a gray file among colour ones, and then the first file with an Adobe segment
    for bad in (files, files[2:]):
        try:
            J.decode_to_tensors(ctx, bad, size=(32, 32), decoder="libjpeg")
        except (ValueError, J.JdaError):
            pass
        else:
            raise AssertionError("not refused")
    ctx.close()
    print("exact adobe tensors ok")


if __name__ == "__main__":
    main()
