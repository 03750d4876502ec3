"""The body of tests/test_gpu_pack.py::test_decode_to_tensors, run as a program in a process of its own: torch is imported FIRST, so that
this process has one HIP runtime (torch's, where torch ships one) for torch and for libjpegdec_amd.so alike.  decode_to_tensors against
the oracle's canvas cut and permuted by numpy; prints "pack_torch_child ok"."""
import os
import sys

import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from oracle.loader import OracleDecoder  # noqa: E402
from tests.cases import jpeg_for  # noqa: E402
from tests.test_gpu_pack import expected_packed  # noqa: E402
from tests.test_pack_cpu import BGR, CHW, F16, F32, HWC, INVALID, U8  # noqa: E402


def raises(kind, fn):
    try:
        fn()
    except kind as e:
        return e
    raise AssertionError("%s not raised" % kind.__name__)


def main():
    oracle = OracleDecoder()
    ctx = J.Context(0)
    # mixed sizes: a list of tensors
    names = ("c420_333x217", "c440_200x120", "c444_384x192_q100_rst7")
    files = [jpeg_for(n) for n in names]
    out = J.decode_to_tensors(ctx, files)
    assert isinstance(out, list) and len(out) == 3
    for t, f, (w, h) in zip(out, files, ((333, 217), (200, 120), (384, 192))):
        assert t.dtype == torch.uint8 and tuple(t.shape) == (3, h, w) and t.device == torch.device("cuda", ctx.device) and t.is_contiguous()
        assert np.array_equal(t.cpu().numpy().reshape(-1), expected_packed(oracle, f, 0, CHW, U8, None)[0])
    out = J.decode_to_tensors(ctx, files, layout="HWC", bgr=True, options=J.SCALE_HALF)
    for t, f in zip(out, files):
        want, w, h, _ = expected_packed(oracle, f, J.SCALE_HALF, HWC | BGR, U8, None)
        assert tuple(t.shape) == (h, w, 3) and np.array_equal(t.cpu().numpy().reshape(-1), want)
    # equal sizes: ONE tensor, its images at their unaligned offsets (3 * 217 * 333 is odd)
    same = [jpeg_for("c420_333x217")] * 3
    t = J.decode_to_tensors(ctx, same)
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (3, 3, 217, 333) and t.dtype == torch.uint8 and t.is_contiguous()
    want = expected_packed(oracle, same[0], 0, CHW, U8, None)[0]
    host = t.cpu().numpy()
    for k in range(3):
        assert np.array_equal(host[k].reshape(-1), want), k
    # float through normalise_table: the table's bit patterns, and the formula on the oracle's bytes
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    mixed = same[:2] + [jpeg_for("c444_333x217")]
    for dt, elem in ((torch.float32, F32), (torch.float16, F16)):
        table = J.normalise_table(mean, std, dt)
        t = J.decode_to_tensors(ctx, mixed, layout="CHW", dtype=dt, table=table)
        assert tuple(t.shape) == (3, 3, 217, 333) and t.dtype == dt
        host = t.cpu().numpy()
        for k, f in enumerate(mixed):
            assert np.array_equal(host[k].reshape(-1).view(np.uint8), expected_packed(oracle, f, 0, CHW, elem, table)[0]), (dt, k)
    t = J.decode_to_tensors(ctx, [jpeg_for("c422_333x217")], layout="HWC", dtype=torch.float32, table=torch.from_numpy(J.normalise_table(mean, std)))
    assert tuple(t.shape) == (1, 217, 333, 3)
    pixels = expected_packed(oracle, jpeg_for("c422_333x217"), 0, HWC, U8, None)[0].reshape(217, 333, 3)
    formula = ((pixels.astype(np.float64) / 255.0 - np.array(mean)) / np.array(std)).astype(np.float32)
    assert np.array_equal(t.cpu().numpy()[0], formula)
    # gray files: one channel; gray and colour in one call, a float type without a table, a file that does not decode
    g = J.decode_to_tensors(ctx, [jpeg_for("gray_333x217"), jpeg_for("gray_64x64_rst3")], layout="HWC")
    assert [tuple(x.shape) for x in g] == [(217, 333, 1), (64, 64, 1)]
    assert np.array_equal(g[0].cpu().numpy().reshape(-1), expected_packed(oracle, jpeg_for("gray_333x217"), 0, HWC, U8, None)[0])
    assert J.decode_to_tensors(ctx, []) == []
    raises(ValueError, lambda: J.decode_to_tensors(ctx, [jpeg_for("gray_333x217"), same[0]]))
    assert raises(J.JdaError, lambda: J.decode_to_tensors(ctx, same, dtype=torch.float32)).code == INVALID
    raises(J.JdaError, lambda: J.decode_to_tensors(ctx, [same[0], same[0][:400]]))
    ctx.close()
    print("pack_torch_child ok")


if __name__ == "__main__":
    main()
