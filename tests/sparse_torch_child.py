"""The body of tests/test_gpu_sparse_coef.py::test_decode_to_tensors_progressive_full, run as a program in a process of its own: torch is
imported FIRST, so that this process has one HIP runtime for torch and for libjpegdec_amd.so alike.  decode_to_tensors(progressive="full")
against the oracle's visible rectangle of the (re-encoded) baseline permuted by numpy, with size= and a crop against tests/resize_util, and
the default keyword, which still gives the 1/8 thumbnail; prints "sparse_torch_child ok"."""
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
from tests import prog_cases as PC, resize_util as R  # noqa: E402


def visible(oracle, jpeg, options=0):
    """[h, w, 3] uint8: the oracle's canvas of the file cut to its visible size, the alpha byte dropped"""
    info = ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    g = J.output_geometry(info, J.RGB8888, options)
    rc, canvas, err = oracle.decode_canvas(jpeg, J.RGB8888, options)
    assert rc == 1
    return canvas.reshape(canvas.shape[0], -1, 4)[:g["out_h"], :g["out_w"], :3]


def main():
    oracle = OracleDecoder()
    ctx = J.Context(0)
    name = "c420_200x136_q50_rst"
    pj, tw = PC.files(name)
    base, events = PC.reencoded(name)
    assert events == 0
    want_b, want_p = visible(oracle, tw), visible(oracle, base)
    # a baseline file and its progressive twin, one size: ONE [2, 3, H, W] tensor
    t = J.decode_to_tensors(ctx, [tw, pj], progressive="full")
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == (2, 3, 136, 200) and t.dtype == torch.uint8 and t.device == torch.device("cuda", ctx.device)
    host = t.cpu().numpy()
    assert np.array_equal(host[0], want_b.transpose(2, 0, 1)) and np.array_equal(host[1], want_p.transpose(2, 0, 1))
    # size= and a crop: tests/resize_util.resize over that rectangle
    crops = [(10, 20, 150, 100), (3, 5, 190, 120)]
    t = J.decode_to_tensors(ctx, [tw, pj], progressive="full", size=(24, 32), crops=crops)
    assert tuple(t.shape) == (2, 3, 24, 32)
    host = t.cpu().numpy()
    for k, w in enumerate((want_b, want_p)):
        assert np.array_equal(host[k], R.resize(w, 32, 24, crops[k]).transpose(2, 0, 1)), k
    # prescale: no DCT-domain scale for the progressive file, it is decoded at full size and resized from there; the baseline file takes 1/4
    t = J.decode_to_tensors(ctx, [tw, pj], progressive="full", size=(24, 32), prescale=True)
    host = t.cpu().numpy()
    assert np.array_equal(host[1], R.resize(want_p, 32, 24).transpose(2, 0, 1))
    assert np.array_equal(host[0], R.resize(visible(oracle, tw, J.SCALE_QUARTER), 32, 24).transpose(2, 0, 1))
    # the default keyword: the progressive file still comes back at 1/8 size
    for kw in ({}, {"progressive": "thumbnail"}):
        t = J.decode_to_tensors(ctx, [pj], **kw)
        assert tuple(t.shape) == (1, 3, 17, 25)
        assert np.array_equal(t.cpu().numpy()[0], visible(oracle, pj).transpose(2, 0, 1))
    ctx.close()
    print("sparse_torch_child ok")


if __name__ == "__main__":
    main()
