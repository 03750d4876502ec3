"""The body of tests/test_gpu_exact_scaled.py::test_decode_to_tensors_draft_is_pillow, run as a program in a process of its own: torch is
imported FIRST, so that this process has one HIP runtime for torch and for libjpegdec_amd.so alike.
decode_to_tensors(files, size=(32, 32), resample="bicubic", decoder="libjpeg", draft=True) over a mixed baseline / progressive list of
mixed sizes -- so that the files take different scales -- against Pillow itself: Image.open(f), draft("RGB", (32, 32)), convert("RGB"),
resize((32, 32), Image.BICUBIC), bit for bit; prints "exact scaled tensors ok"."""
import io
import os
import sys

import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from tests import cases  # noqa: E402
from tests import exact_scaled_util as S  # noqa: E402
from tests import exact_util as X  # noqa: E402


def pillow_drafted(f, request, size, resample, mode="RGB"):
    """request, size: (w, h) as Pillow's -> (the scale Pillow chose, the resized pixels)"""
    im = Image.open(io.BytesIO(f))
    im.draft(mode, request)
    scale = im.decoderconfig[0] if im.decoderconfig else 1
    return scale, np.asarray(im.convert(mode).resize(size, resample))


def main():
    ctx = J.Context(0)
    # 4:2:0 and 4:4:4 files wider than 4 pixels: where a file stays at full size, the full-size road's pixels are Pillow's too
    # (and no side more than 40 times the tensor's: the resize's tap cap, JDA_RESIZE_MAX_KSIZE, is not this test's subject)
    picks = (("4:2:0", (45, 53)), ("4:2:0", (100, 37)), ("4:2:0", (75, 53)), ("4:4:4", (161, 17)), ("4:2:2", (100, 37)), ("4:4:0", (31, 65)), ("4:2:0", (33, 31)),
             ("4:4:4", (64, 48)))
    files = [[f for name, f, wh in S.grid(s) if wh == want][0] for s, want in picks]
    fixtures = ("c420_333x217", "c444_333x217", "c422_333x217", "c440_200x120")      # (large enough for 1/4 and 1/8 at 32 x 32)
    files += [cases.jpeg_for(name) for name in fixtures]
    picks += tuple((name, None) for name in fixtures)
    for size, draft, request in (((8, 8), True, (8, 8)), ((32, 32), True, (32, 32)), ((5, 40), True, (40, 5)), ((16, 16), (4, 9), (9, 4))):
        t = J.decode_to_tensors(ctx, files, size=size, resample="bicubic", decoder="libjpeg", draft=draft)
        assert isinstance(t, torch.Tensor) and tuple(t.shape) == (len(files), 3) + size and t.dtype == torch.uint8
        host = t.cpu().numpy()
        scales = set()
        for k, f in enumerate(files):
            scale, want = pillow_drafted(f, request, size[::-1], Image.BICUBIC)
            assert scale == J.exact_draft_scale(f, request)
            assert X.in_window(S.twin_scaled(f, scale))
            scales.add(scale)
            assert np.array_equal(host[k].transpose(1, 2, 0), want), (picks[k], size, scale, int(np.count_nonzero(host[k].transpose(1, 2, 0) != want)))
        assert len(scales) >= 2, scales
    # gray files through draft("L")'s pixels, HWC, another filter
    grays = [[f for name, f, wh in S.grid("gray") if wh == want][0] for want in ((75, 53), (161, 17), (100, 37))]
    t = J.decode_to_tensors(ctx, grays, layout="HWC", size=(8, 12), resample="lanczos", decoder="libjpeg", draft=True)
    for k, f in enumerate(grays):
        scale, want = pillow_drafted(f, (12, 8), (12, 8), Image.LANCZOS, "L")
        assert scale > 1 and np.array_equal(t[k, ..., 0].cpu().numpy(), want), k
    # without draft the call is what it was: full-size decode, then the resize
    a = J.decode_to_tensors(ctx, files[:3], size=(8, 8), resample="bicubic", decoder="libjpeg")
    b = J.decode_to_tensors(ctx, files[:3], size=(8, 8), resample="bicubic", decoder="libjpeg", draft=None)
    c = J.decode_to_tensors(ctx, files[:3], size=(8, 8), resample="bicubic", decoder="libjpeg", draft=True)
    assert torch.equal(a, b) and not torch.equal(a, c)
    for k in range(3):
        assert np.array_equal(a[k].cpu().numpy().transpose(1, 2, 0), np.asarray(Image.open(io.BytesIO(files[k])).convert("RGB").resize((8, 8), Image.BICUBIC)))
    for kw in (dict(decoder="reference", draft=True, size=(8, 8)), dict(decoder="libjpeg", draft=True), dict(decoder="libjpeg", draft=True, size=(8, 8), crops=[(0, 0, 4, 4)]),
               dict(decoder="libjpeg", draft=True, size=(8, 8), prescale=True), dict(decoder="libjpeg", draft=True, size=(8, 8), options=J.SCALE_HALF)):
        try:
            J.decode_to_tensors(ctx, files[:1], **kw)
        except ValueError:
            pass
        else:
            raise AssertionError("not refused: %r" % (kw,))
    ctx.close()
    print("exact scaled tensors ok")


if __name__ == "__main__":
    main()
