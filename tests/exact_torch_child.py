"""The body of tests/test_gpu_exact.py::test_decode_to_tensors_libjpeg_is_pillow, run as a program in a process of its own: torch is
imported FIRST, so that this process has one HIP runtime for torch and for libjpegdec_amd.so alike.
decode_to_tensors(files, size=(32, 32), resample="bicubic", decoder="libjpeg") over a mixed baseline / progressive list against Pillow itself:
Image.open(f).convert("RGB").resize((32, 32), Image.BICUBIC), bit for bit; prints "exact tensors ok"."""
import io
import os
import sys

import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from tests import exact_util as X  # noqa: E402


def pillow_resized(f, size, resample, mode="RGB"):
    return np.asarray(Image.open(io.BytesIO(f)).convert(mode).resize(size, resample))


def main():
    ctx = J.Context(0)
    picks = (("4:2:0", "baseline_33x31_q90"), ("4:2:0", "progressive_75x53_q30"), ("4:4:4", "optimize_45x53_q100"), ("4:2:2", "restart_64x48_q90"),
             ("4:4:0", "written_161x17_q100"), ("4:2:2", "progressive_45x53_q100"), ("4:2:0", "dense60"))
    files = [dict(X.grid(s))[name] for s, name in picks]
    for f in files:
        assert X.in_window(X.twin(f))
    t = J.decode_to_tensors(ctx, files, size=(32, 32), resample="bicubic", decoder="libjpeg")
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (len(files), 3, 32, 32) and t.dtype == torch.uint8
    host = t.cpu().numpy()
    for k, f in enumerate(files):
        want = pillow_resized(f, (32, 32), Image.BICUBIC)
        assert np.array_equal(host[k].transpose(1, 2, 0), want), (picks[k], int(np.count_nonzero(host[k].transpose(1, 2, 0) != want)))
    # without size=: the decoded pixels themselves, a tensor a file
    ts = J.decode_to_tensors(ctx, files[:3], layout="HWC", decoder="libjpeg")
    for k in range(3):
        assert np.array_equal(ts[k].cpu().numpy(), X.pillow(files[k], "RGB")), picks[k]
    # crops and another filter, and gray files through draft("L")'s pixels
    crops = [(1, 2, 20, 25)] * len(files[:2])
    t = J.decode_to_tensors(ctx, files[:2], layout="HWC", size=(16, 24), crops=crops, resample="lanczos", decoder="libjpeg")
    for k in range(2):
        want = np.asarray(Image.open(io.BytesIO(files[k])).convert("RGB").resize((24, 16), Image.LANCZOS, box=(1, 2, 21, 27)))
        assert np.array_equal(t[k].cpu().numpy(), want), picks[k]
    grays = [dict(X.grid("gray"))[n] for n in ("baseline_33x31_q90", "progressive_75x53_q30")]
    t = J.decode_to_tensors(ctx, grays, size=(32, 32), resample="bicubic", decoder="libjpeg")
    for k, f in enumerate(grays):
        assert np.array_equal(t[k, 0].cpu().numpy(), pillow_resized(f, (32, 32), Image.BICUBIC, "L")), k
    # the default is today's path, and decoder="reference" names it
    a, b = J.decode_to_tensors(ctx, files[:1] + files[2:4], size=(32, 32)), J.decode_to_tensors(ctx, files[:1] + files[2:4], size=(32, 32), decoder="reference")
    assert torch.equal(a, b) and not torch.equal(a, J.decode_to_tensors(ctx, files[:1] + files[2:4], size=(32, 32), decoder="libjpeg"))
    for kw in (dict(prescale=True, size=(8, 8)), dict(options=J.SCALE_HALF), dict(decoder="turbo")):
        try:
            J.decode_to_tensors(ctx, files[:1], **dict(dict(decoder="libjpeg"), **kw))
        except ValueError:
            pass
        else:
            raise AssertionError("not refused: %r" % (kw,))
    ctx.close()
    print("exact tensors ok")


if __name__ == "__main__":
    main()
