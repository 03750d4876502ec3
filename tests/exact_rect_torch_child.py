"""The body of tests/test_gpu_exact_rect.py::test_decode_to_tensors_crops_are_pillows_resize_box, run as a program in a process of its own:
torch is imported FIRST, so that this process has one HIP runtime for torch and for libjpegdec_amd.so alike.
decode_to_tensors(files, size=, crops=, decoder="libjpeg", resample=F) over a mixed baseline / progressive list against Pillow itself:
Image.open(f).convert("RGB").resize(size, F, box=crop), bit for bit; the rectangles the call hands to exact_decode are the ones the filter's
taps read, and their MCU rectangles hold fewer planes-stage tiles than the whole files; prints "exact rect tensors ok"."""
import io
import os
import sys

import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from jpegdec_amd import binding as B  # noqa: E402
from tests import cases  # noqa: E402
from tests import exact_scaled_util as S  # noqa: E402
from tests import exact_util as X  # noqa: E402

def main():
    ctx = J.Context(0)
    fixtures = ("c420_333x217", "c444_333x217", "c422_333x217", "c440_200x120")
    files = [cases.jpeg_for(name) for name in fixtures]
    files += [[f for name, f, wh in S.grid(s) if wh == want and name.startswith(kind)][0] for s, want, kind in (("4:2:0", (45, 53), "progressive"), ("4:2:0", (100, 37), ""),
                                                                                                                ("4:4:4", (64, 48), ""))]
    sizes = [Image.open(io.BytesIO(f)).size for f in files]
    for f in files:
        assert X.in_window(X.twin(f))
    rng = np.random.default_rng(20)
    seen = []
    keep = B.exact_decode

    def spy(ctx_, sources, outs, pts, scales=None, colour_models=False, rects=None):
        seen.append((list(outs), None if rects is None else list(rects)))
        return keep(ctx_, sources, outs, pts, scales, colour_models, rects)
    B.exact_decode = spy
    try:
        for size, resample, pf in (((32, 32), "bicubic", Image.BICUBIC), ((24, 40), "bilinear", Image.BILINEAR), ((16, 16), "lanczos", Image.LANCZOS), ((9, 7), "box", Image.BOX)):
            crops = []
            for w, h in sizes:                                          # a random-resized-crop box an image, fixed seed
                cw, ch = int(rng.integers(max(2, w // 6), w + 1)), int(rng.integers(max(2, h // 6), h + 1))
                crops.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
            crops[0] = (0, 0) + sizes[0]                                 # (one crop is the whole image)
            crops[1] = (41, 37, 60, 50)
            t = J.decode_to_tensors(ctx, files, size=size, crops=crops, resample=resample, decoder="libjpeg")
            assert isinstance(t, torch.Tensor) and tuple(t.shape) == (len(files), 3) + size and t.dtype == torch.uint8
            host = t.cpu().numpy()
            for k, (f, (x, y, w, h)) in enumerate(zip(files, crops)):
                want = np.asarray(Image.open(io.BytesIO(f)).convert("RGB").resize(size[::-1], pf, box=(x, y, x + w, y + h)))
                got = host[k].transpose(1, 2, 0)
                assert np.array_equal(got, want), (k, size, resample, crops[k], int(np.count_nonzero(got != want)))
            outs, rects = seen[-1]
            assert rects is not None and len(rects) == len(files)
            fewer = 0
            for k, (f, r) in enumerate(zip(files, rects)):
                x0, y0, x1, y1 = J.resize_reads(sizes[k], crops[k], size[::-1], B.resize_filter(resample))
                assert tuple(r) == (x0, y0, x1 - x0, y1 - y0)
                assert outs[k][2] == r[2] and outs[k][3] == r[3]                     # the surface holds the rectangle, not the image
                assert r[0] <= crops[k][0] and r[1] <= crops[k][1] and r[0] + r[2] >= crops[k][0] + crops[k][2] and r[1] + r[3] >= crops[k][1] + crops[k][3]
                info = J.parse(f)
                mx0, my0, mx1, my1 = J.exact_rect_mcus(f, r)
                fewer += (mx1 - mx0) * (my1 - my0) < info["mcus_x"] * info["mcus_y"]
            assert fewer >= 3, fewer
        # gray files, one channel, HWC
        grays = [cases.jpeg_for("gray_333x217"), [f for name, f, wh in S.grid("gray") if wh == (75, 53)][0]]
        crops = [(100, 50, 120, 90), (3, 5, 40, 31)]
        t = J.decode_to_tensors(ctx, grays, layout="HWC", size=(20, 28), crops=crops, resample="hamming", decoder="libjpeg")
        for k, (f, (x, y, w, h)) in enumerate(zip(grays, crops)):
            im = Image.open(io.BytesIO(f))
            assert np.array_equal(t[k, ..., 0].cpu().numpy(), np.asarray(im.resize((28, 20), Image.HAMMING, box=(x, y, x + w, y + h)))), k
        # draft= with crops= stays refused
        try:
            J.decode_to_tensors(ctx, files[:1], size=(8, 8), crops=[(0, 0, 8, 8)], decoder="libjpeg", draft=True)
        except ValueError:
            pass
        else:
            raise AssertionError("draft with crops was not refused")
    finally:
        B.exact_decode = keep
    ctx.close()
    print("exact rect tensors ok")


if __name__ == "__main__":
    main()
