"""The body of tests/test_gpu_resize.py::test_decode_to_tensors_with_size, run as a program in a process of its own: torch is imported FIRST,
so that this process has one HIP runtime (torch's, where torch ships one) for torch and for libjpegdec_amd.so alike.
decode_to_tensors(size=...) against the numpy twin over the oracle's canvas, numpy's pack and the table; prints "resize_torch_child ok"."""
import ctypes as C
import os
import sys

import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from jpegdec_amd.binding import ImageInfo  # noqa: E402
from oracle.loader import OracleDecoder  # noqa: E402
from tests import resize_util as R  # noqa: E402
from tests.cases import jpeg_for  # noqa: E402
from tests.test_gpu_resize import visible_pixels  # noqa: E402

H, W = 32, 48


def expected(oracle, jpeg, options, layout, crop=None, bgr=False, size=(H, W)):
    """[C, H, W] or [H, W, C] uint8: the twin over the oracle's visible pixels, the alpha byte dropped, permuted by numpy"""
    info = ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    gray = info.ncomp == 1 or bool(options & J.LUMA_ONLY)
    vis = visible_pixels(oracle, jpeg, J.GRAY8 if gray else J.RGB8888, options)
    out = R.resize(vis, size[1], size[0], crop)[:, :, :1 if gray else 3]
    if bgr:
        out = out[:, :, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1) if layout == "CHW" else out)


def main():
    oracle = OracleDecoder()
    ctx = J.Context(0)
    names = ("c420_333x217", "c440_200x120", "c444_384x192_q100_rst7")
    files = [jpeg_for(n) for n in names]
    # mixed sizes in, ONE tensor out
    for layout, shape in (("CHW", (3, 3, H, W)), ("HWC", (3, H, W, 3))):
        t = J.decode_to_tensors(ctx, files, layout=layout, size=(H, W))
        assert isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == torch.uint8 and t.is_contiguous() and t.device == torch.device("cuda", ctx.device)
        host = t.cpu().numpy()
        for k, f in enumerate(files):
            assert np.array_equal(host[k], expected(oracle, f, 0, layout)), (layout, names[k])
    # crops, in pixels of each file's visible size; BGR
    crops = [(10, 20, 300, 150), (0, 0, 200, 120), (383, 191, 1, 1)]
    t = J.decode_to_tensors(ctx, files, layout="HWC", size=(H, W), crops=crops, bgr=True)
    host = t.cpu().numpy()
    for k, f in enumerate(files):
        assert np.array_equal(host[k], expected(oracle, f, 0, "HWC", crops[k], bgr=True)), names[k]
    # float32 through normalise_table: the table's values of the twin's bytes
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    table = J.normalise_table(mean, std, torch.float32)
    for layout in ("CHW", "HWC"):
        t = J.decode_to_tensors(ctx, files, layout=layout, dtype=torch.float32, table=table, size=(H, W), crops=crops)
        assert t.dtype == torch.float32 and tuple(t.shape) == ((3, 3, H, W) if layout == "CHW" else (3, H, W, 3))
        host = t.cpu().numpy()
        for k, f in enumerate(files):
            px = expected(oracle, f, 0, "HWC", crops[k])
            want = np.stack([table[c][px[..., c]] for c in range(3)], axis=2)
            assert np.array_equal(host[k], want.transpose(2, 0, 1) if layout == "CHW" else want), (layout, names[k])
    # a scale bit of the caller's: the crop is in the scaled image's pixels; gray files: one channel; one file: still a batch of one
    t = J.decode_to_tensors(ctx, files[:2], size=(H, W), options=J.SCALE_HALF, crops=[(1, 2, 160, 100), (0, 0, 100, 60)])
    for k, f in enumerate(files[:2]):
        assert np.array_equal(t.cpu().numpy()[k], expected(oracle, f, J.SCALE_HALF, "CHW", [(1, 2, 160, 100), (0, 0, 100, 60)][k])), names[k]
    g = J.decode_to_tensors(ctx, [jpeg_for("gray_333x217")], layout="HWC", size=(H, W))
    assert tuple(g.shape) == (1, H, W, 1) and np.array_equal(g.cpu().numpy()[0], expected(oracle, jpeg_for("gray_333x217"), 0, "HWC"))
    # prescale: the largest of 1/2, 1/4, 1/8 whose visible size is still at least W x H on both axes -- 333 x 217 is 42 x 28 at 1/8 and
    # 84 x 55 at 1/4, so size (H, W) = (20, 30) takes 1/8 and (30, 20), whose 30 rows 1/8 no longer has, takes 1/4; upscaling takes none
    f = jpeg_for("c420_333x217")
    info = ImageInfo()
    assert J.load_library().jda_parse(f, len(f), C.byref(info)) == 0
    for size, bit in (((20, 30), J.SCALE_EIGHTH), ((30, 20), J.SCALE_QUARTER), ((28, 42), J.SCALE_EIGHTH), ((29, 42), J.SCALE_QUARTER), ((109, 167), J.SCALE_HALF),
                      ((110, 167), 0), ((400, 400), 0)):
        by_rule = 0
        for b, shift in ((J.SCALE_EIGHTH, 3), (J.SCALE_QUARTER, 2), (J.SCALE_HALF, 1)):
            if (333 + (1 << shift) - 1) >> shift >= size[1] and (217 + (1 << shift) - 1) >> shift >= size[0]:
                by_rule = b
                break
        assert by_rule == bit == J.tensors.prescale_option(info, J.RGB8888, 0, size), (size, by_rule)
        if size[0] > 200:
            continue
        t = J.decode_to_tensors(ctx, [f, f], size=size, prescale=True)
        assert tuple(t.shape) == (2, 3) + size
        want = expected(oracle, f, bit, "CHW", size=size)
        assert np.array_equal(t.cpu().numpy()[0], want) and np.array_equal(t.cpu().numpy()[1], want), size
        if bit:
            assert not np.array_equal(want, expected(oracle, f, 0, "CHW", size=size))        # (it changes pixels: that is why it is opt-in)
    # size=None: as before -- a list for mixed sizes
    out = J.decode_to_tensors(ctx, files)
    assert isinstance(out, list) and [tuple(x.shape) for x in out] == [(3, 217, 333), (3, 120, 200), (3, 192, 384)]
    # a rectangle that leaves the image, a ratio beyond the cap: the library's codes
    for kw, code in ((dict(size=(H, W), crops=[(0, 0, 334, 10)] * 3), 1), (dict(size=(2, W)), 3)):
        try:
            J.decode_to_tensors(ctx, files, **kw)
        except J.JdaError as e:
            assert e.code == code, (kw, e.code)
        else:
            raise AssertionError("not refused: %r" % (kw,))
    ctx.close()
    print("resize_torch_child ok")


if __name__ == "__main__":
    main()
