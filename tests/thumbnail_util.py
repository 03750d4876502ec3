"""TEST INFRASTRUCTURE: Pillow's Image.thumbnail() restated in numpy and Python floats -- the three steps behind the draft decode.

reduce       Image.reduce((fx, fy), box): per byte ((sum + n // 2) * ((1 << 24) // n)) >> 24 over the n pixels of a cell, in uint32; the
             cells of the box's last column and row hold fewer pixels.  NOT the rounded mean (rounded_mean, kept for the test that says so).
resize_box   Image.resize(size, F, box = a float box): tests/resize_filter_util.py's taps and passes over fractional ends.  Pillow's C side
             holds the box as float, so the ends are float32 values, and the box's length is their difference rounded to float32 again;
             from there everything is double.  in0 + float32(in1 - in0) is exact in double, so axis_taps(.., in0, that sum, ..) works out
             (in1 - in0) / out_size and in0 + (xx + 0.5) * scale from exactly Pillow's operands.
plan         Image.thumbnail / JpegImageFile.draft / the reducing_gap branch of Image.resize / _get_safe_box, Pillow 12's, as a dict.
thumbnail    the three applied to the pixels a decode at the plan's scale gives.

numpy only (the GPU machine may have no Pillow; tests/test_thumbnail_cpu.py holds all of this to Pillow where Pillow is)."""
import math
import struct

import numpy as np

from tests import resize_filter_util as F

MAX_FACTOR = 32                                                       # JDA_REDUCE_MAX_FACTOR


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def reduced_size(bw, bh, fx, fy):
    return -(-bw // fx), -(-bh // fy)


def _cells(img, fx, fy, box):
    a = img[:, :, None] if img.ndim == 2 else img
    h, w = a.shape[:2]
    x0, y0, x1, y1 = box if box is not None else (0, 0, w, h)
    assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h and fx >= 1 and fy >= 1
    a = a[y0:y1, x0:x1].astype(np.uint32)
    ow, oh = reduced_size(x1 - x0, y1 - y0, fx, fy)
    pad = np.zeros((oh * fy, ow * fx, a.shape[2]), np.uint32)
    pad[:a.shape[0], :a.shape[1]] = a
    sums = pad.reshape(oh, fy, ow, fx, a.shape[2]).sum(axis=(1, 3), dtype=np.uint32)
    nx = np.minimum(fx, (x1 - x0) - np.arange(ow) * fx).astype(np.uint32)
    ny = np.minimum(fy, (y1 - y0) - np.arange(oh) * fy).astype(np.uint32)
    return sums, (ny[:, None] * nx[None, :])[:, :, None]


def reduce(img, fx, fy, box=None):
    """img [h, w, c] (or [h, w]) uint8, box = (x0, y0, x1, y1) or None: the whole image -> [ceil(bh / fy), ceil(bw / fx), c] uint8"""
    sums, n = _cells(img, fx, fy, box)
    out = (((sums + n // 2) * ((1 << 24) // n)) >> 24).astype(np.uint8)      # (uint32 throughout: (255 n + n / 2) * (2^24 // n) < 2^32)
    return np.ascontiguousarray(out[:, :, 0] if img.ndim == 2 else out)


def rounded_mean(img, fx, fy, box=None):
    """what Image.reduce is NOT: (sum + n // 2) // n"""
    sums, n = _cells(img, fx, fy, box)
    out = ((sums + n // 2) // n).astype(np.uint8)
    return np.ascontiguousarray(out[:, :, 0] if img.ndim == 2 else out)


def box_axis(f, in_size, in0, in1, out_size, double_box=False):
    """the taps of an axis with fractional ends.  double_box: the ends kept as Python floats -- what Pillow does NOT do"""
    if double_box:
        return F.axis_taps(f, in_size, float(in0), float(in1), out_size)
    a, b = f32(in0), f32(in1)
    return F.axis_taps(f, in_size, a, a + f32(b - a), out_size)


def resize_box(img, out_w, out_h, box, f, double_box=False):
    """img [h, w, c] (or [h, w]) uint8, box = (x0, y0, x1, y1) floats -> [out_h, out_w, c] (or [out_h, out_w]) uint8"""
    flat = img.ndim == 2
    a = img[:, :, None] if flat else img
    h, w = a.shape[:2]
    assert 0 <= box[0] < box[2] <= w and 0 <= box[1] < box[3] <= h
    hb, hk = box_axis(f, w, box[0], box[2], out_w, double_box)
    vb, vk = box_axis(f, h, box[1], box[3], out_h, double_box)
    r0, r1 = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
    tmp = F._pass(a[r0:r1], hb, hk)
    vb = vb.copy()
    vb[:, 0] -= r0
    out = F._pass(tmp.transpose(1, 0, 2), vb, vk).transpose(1, 0, 2)
    return np.ascontiguousarray(out[:, :, 0] if flat else out)


def draft_scale(w, h, rw, rh):
    k = min(w // rw, h // rh)
    return 8 if k >= 8 else 4 if k >= 4 else 2 if k >= 2 else 1


def plan(src_w, src_h, req, f, gap=2.0):
    """Image.open(a src_w x src_h JPEG).thumbnail(req, F, gap) as a dict: out (w, h), scale, draft (w, h), factors (fx, fy), reduce_box
    (x0, y0, x1, y1), reduced (w, h), resize (bool), box (four floats, not yet rounded to float32), tall (the > 100 : 1 case), tie (floor and
    ceil of the free side keep the aspect equally well: the floor was taken).  gap None or 0: no draft and no reduce."""
    gap = gap or None
    x, y = req
    p = dict(out=(src_w, src_h), scale=1, draft=(src_w, src_h), factors=(1, 1), reduce_box=(0, 0, src_w, src_h), reduced=(src_w, src_h), resize=False,
             box=(0.0, 0.0, float(src_w), float(src_h)), tall=False, tie=False)
    if x >= src_w and y >= src_h:
        return p

    def round_aspect(number, key):
        p["tie"] = math.floor(number) != math.ceil(number) and key(math.floor(number)) == key(math.ceil(number))
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = src_w / src_h
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    p["out"] = (x, y)
    if gap is not None:
        p["scale"] = draft_scale(src_w, src_h, int(req[0] * gap), int(req[1] * gap))
    s = p["scale"]
    p["draft"] = p["reduced"] = (-(-src_w // s), -(-src_h // s))
    box = (0, 0, src_w / s, src_h / s)
    p["box"] = box
    p["reduce_box"] = (0, 0) + p["draft"]
    if p["draft"] == p["out"]:
        return p
    p["resize"] = True
    if gap is not None:
        fx = int((box[2] - box[0]) / x / gap) or 1
        fy = int((box[3] - box[1]) / y / gap) or 1
        if fx > 1 or fy > 1:
            support = F.SUPPORT[f] - 0.5
            sx, sy = support * ((box[2] - box[0]) / x), support * ((box[3] - box[1]) / y)
            rb = (max(0, int(box[0] - sx)), max(0, int(box[1] - sy)), min(p["draft"][0], math.ceil(box[2] + sx)), min(p["draft"][1], math.ceil(box[3] + sy)))
            p["factors"], p["reduce_box"] = (fx, fy), rb
            p["reduced"] = reduced_size(rb[2] - rb[0], rb[3] - rb[1], fx, fy)
            p["box"] = ((box[0] - rb[0]) / fx, (box[1] - rb[1]) / fy, (box[2] - rb[0]) / fx, (box[3] - rb[1]) / fy)
    p["tall"] = p["reduced"][1] > p["reduced"][0] * 100 and y < p["reduced"][1]
    return p


def thumbnail(decode, src_w, src_h, req, f, gap=2.0):
    """decode(scale) -> the pixels [h, w(, c)] uint8 of the file at that scale; the thumbnail's pixels and the plan"""
    p = plan(src_w, src_h, req, f, gap)
    assert not p["tall"]
    img = decode(p["scale"])
    assert img.shape[:2] == (p["draft"][1], p["draft"][0])
    if p["factors"] != (1, 1):
        img = reduce(img, p["factors"][0], p["factors"][1], p["reduce_box"])
        assert img.shape[:2] == (p["reduced"][1], p["reduced"][0])
    if p["resize"]:
        img = resize_box(img, p["out"][0], p["out"][1], p["box"], f)
    return img, p
