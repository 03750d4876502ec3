"""The body of tests/test_gpu_unpack.py::test_encode_tensors, run as a program in a process of its own: torch is imported FIRST, so that this
process has one HIP runtime (torch's, where torch ships one) for torch and for libjpegdec_amd.so alike.  encode_tensors against the
encoders' twins (tests/encode_util.py and its siblings) over the tensors' own pixels; prints "unpack_torch_child ok"."""
import io
import os
import sys

import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from tests import encode_opt_util as O  # noqa: E402
from tests import encode_prog_util as P  # noqa: E402
from tests import encode_util as E  # noqa: E402
from tests.cases import jpeg_for  # noqa: E402

_TWINS = {}


def raises(kind, fn):
    try:
        fn()
    except kind as e:
        return e
    raise AssertionError("%s not raised" % kind.__name__)


def twin(rgb, sampling, q, ri=0, form="baseline"):
    """rgb: [h, w, 3] or [h, w] uint8 -> the file the encoder's twin makes of it"""
    key = (rgb.tobytes(), rgb.shape, sampling, q, ri, form)
    if key not in _TWINS:
        px = rgb if rgb.ndim == 2 else np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)
        _TWINS[key] = (E.file_bytes(px, sampling, q, ri) if form == "baseline" else O.file_bytes_opt(px, sampling, q, ri) if form == "optimize"
                       else P.file_bytes_prog(px, sampling, q))
    return _TWINS[key]


def opens(f, w, h):
    from PIL import Image
    im = Image.open(io.BytesIO(f))
    im.load()
    assert im.size == (w, h), (im.size, w, h)


def main():
    ctx = J.Context(0)
    dev = torch.device("cuda", ctx.device)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    # one [N,3,H,W] uint8 tensor whose images begin at odd offsets (3 * 217 * 333 is odd)
    same = [jpeg_for("c420_333x217"), jpeg_for("c444_333x217"), jpeg_for("c420_333x217")]
    t = J.decode_to_tensors(ctx, same)
    assert tuple(t.shape) == (3, 3, 217, 333) and t.dtype == torch.uint8
    host = t.cpu().numpy()
    files = J.encode_tensors(ctx, t, quality=80, sampling="4:2:0")
    assert isinstance(files, list) and len(files) == 3 and all(isinstance(f, bytes) for f in files)
    for k in range(3):
        assert files[k] == twin(np.ascontiguousarray(host[k].transpose(1, 2, 0)), "4:2:0", 80), k
        opens(files[k], 333, 217)
    # a list of mixed sizes, HWC + BGR, with a restart interval
    names = ("c420_333x217", "c440_200x120", "c444_384x192_q100_rst7")
    mixed = J.decode_to_tensors(ctx, [jpeg_for(n) for n in names], layout="HWC", bgr=True)
    files = J.encode_tensors(ctx, mixed, quality=60, sampling="4:2:2", restart_interval=3, layout="HWC", bgr=True)
    for x, f, (w, h) in zip(mixed, files, ((333, 217), (200, 120), (384, 192))):
        assert f == twin(np.ascontiguousarray(x.cpu().numpy()[..., ::-1]), "4:2:2", 60, 3), (w, h)
        opens(f, w, h)
    # a view that is not contiguous: a crop of every image of the batch, and a permuted one
    crop = t[:, :, 5:100, 7:120]
    assert not crop.is_contiguous()
    files = J.encode_tensors(ctx, crop, quality=75, sampling="4:4:4")
    for k in range(3):
        assert files[k] == twin(np.ascontiguousarray(host[k, :, 5:100, 7:120].transpose(1, 2, 0)), "4:4:4", 75), k
        opens(files[k], 113, 95)
    hwc_view = t[0].permute(1, 2, 0)
    assert not hwc_view.is_contiguous()
    assert J.encode_tensors(ctx, [hwc_view], quality=80, layout="HWC") == [twin(np.ascontiguousarray(host[0].transpose(1, 2, 0)), "4:2:0", 80)]
    # float16 and float32: decode_to_tensors(table=normalise_table) -> encode_tensors(scale_bias=denormalise_params) gives the files of the uint8 route
    want = J.encode_tensors(ctx, t, quality=80, sampling="4:2:0")
    for dt in (torch.float32, torch.float16):
        x = J.decode_to_tensors(ctx, same, layout="CHW", dtype=dt, table=J.normalise_table(mean, std, dt))
        assert x.dtype == dt and tuple(x.shape) == (3, 3, 217, 333)
        assert J.encode_tensors(ctx, x, quality=80, sampling="4:2:0", scale_bias=J.denormalise_params(mean, std)) == want, dt
    unit = (t.to(torch.float32) / 255.0)                                   # values in [0, 1]: the default scale and bias
    assert J.encode_tensors(ctx, unit, quality=80, sampling="4:2:0") == want
    # gray: one channel, the gray sampling whatever `sampling` says
    g = J.decode_to_tensors(ctx, [jpeg_for("gray_333x217"), jpeg_for("gray_64x64_rst3")], layout="HWC")
    files = J.encode_tensors(ctx, g, quality=75, sampling="4:2:0", layout="HWC")
    for x, f in zip(g, files):
        assert f == twin(np.ascontiguousarray(x.cpu().numpy()[..., 0]), "gray", 75)
        opens(f, x.shape[1], x.shape[0])
    # tables of the file's own, and progressive files
    small = mixed[1]
    rgb = np.ascontiguousarray(small.cpu().numpy()[..., ::-1])
    assert J.encode_tensors(ctx, [small], quality=75, layout="HWC", bgr=True, optimize=True) == [twin(rgb, "4:2:0", 75, 0, "optimize")]
    prog = J.encode_tensors(ctx, [small], quality=75, layout="HWC", bgr=True, progressive=True)
    assert prog == [twin(rgb, "4:2:0", 75, 0, "progressive")]
    opens(prog[0], 200, 120)
    # nothing to do, and what is refused before the GPU is touched
    assert J.encode_tensors(ctx, []) == []
    before = sum(v for k, v in J.kernel_launch_counts().items() if "jda_unpack_tiles" in k)
    u8 = t[0]
    for bad in (lambda: J.encode_tensors(ctx, [u8.cpu()]),                                         # not on the context's device
                lambda: J.encode_tensors(ctx, [u8, u8.to(torch.float32)]),                         # two dtypes
                lambda: J.encode_tensors(ctx, [u8.to(torch.int32)]),                               # no element type for it
                lambda: J.encode_tensors(ctx, [torch.zeros((2, 8, 8), dtype=torch.uint8, device=dev)]),      # two channels
                lambda: J.encode_tensors(ctx, [u8, g[0].permute(2, 0, 1)]),                        # colour and gray
                lambda: J.encode_tensors(ctx, [u8[0]]),                                            # two dimensions
                lambda: J.encode_tensors(ctx, t[0][0]),                                            # a tensor that is no batch
                lambda: J.encode_tensors(ctx, [g[0]], layout="HWC", bgr=True),                     # BGR of one channel
                lambda: J.encode_tensors(ctx, [u8], scale_bias=J.denormalise_params(mean, std)),   # scale and bias with bytes
                lambda: J.encode_tensors(ctx, [unit[0]], scale_bias=[1.0, 2.0]),                   # not 2 x C values
                lambda: J.encode_tensors(ctx, [unit[0]], scale_bias=[[1.0, float("inf"), 1.0], [0.0, 0.0, 0.0]]),
                lambda: J.encode_tensors(ctx, [u8], layout="NCHW"),
                lambda: J.encode_tensors(ctx, [u8], progressive=True, restart_interval=4),
                lambda: J.encode_tensors(ctx, [torch.zeros((3, 0, 8), dtype=torch.uint8, device=dev)])):
        raises(ValueError, bad)
    assert sum(v for k, v in J.kernel_launch_counts().items() if "jda_unpack_tiles" in k) == before
    ctx.close()
    print("unpack_torch_child ok")


if __name__ == "__main__":
    main()
