"""TEST INFRASTRUCTURE: jda_resize_surfaces_ex restated in numpy -- Pillow's Image.resize((ow, oh), F, box=(x, y, x + w, y + h)) for its five
convolution filters (BILINEAR, BOX, HAMMING, BICUBIC, LANCZOS).

numpy only (the GPU machine may have no Pillow; tests/test_resize_filters_cpu.py holds this twin to Pillow where Pillow is).  Knows nothing
of tiles, lanes or LDS: per axis the taps of Pillow's precompute_coeffs / normalize_coeffs_8bpc, worked out in Python floats (IEEE double,
no fused multiply-add) in Pillow's order of operations with math.sin / math.cos (the C library's; numpy's vector code need not round like
it); then the horizontal pass over the source rows the vertical taps read, into 8-bit intermediates, and the vertical pass over those, both
with a signed sum, an arithmetic shift and a clip on both sides.  The grid (image_cases, SIZES, pitch_of) is tests/resize_util.py's."""
import math
import struct

import numpy as np

from tests import resize_util as R

PRECISION_BITS = R.PRECISION_BITS
MAX_KSIZE = R.MAX_KSIZE
BILINEAR, BOX, HAMMING, BICUBIC, LANCZOS = range(5)          # JDA_RESIZE_*
FILTERS = (BILINEAR, BOX, HAMMING, BICUBIC, LANCZOS)
SIGNED = (BICUBIC, LANCZOS)
NAMES = {BILINEAR: "bilinear", BOX: "box", HAMMING: "hamming", BICUBIC: "bicubic", LANCZOS: "lanczos"}
SUPPORT = {BILINEAR: 1.0, BOX: 0.5, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
UPSCALE_TAPS = {BILINEAR: 3, BOX: 3, HAMMING: 3, BICUBIC: 5, LANCZOS: 7}
# Pillow writes the Hamming window's constants as float literals (0.54f, 0.46f): they enter the double arithmetic with a float's bits
HAMMING_A, HAMMING_B = (struct.unpack("f", struct.pack("f", v))[0] for v in (0.54, 0.46))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def weight(f, x):
    if f == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if f == LANCZOS:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    x = abs(x)
    if f == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    if f == HAMMING:
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (HAMMING_A + HAMMING_B * math.cos(x))
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_taps = {}


def axis_taps(f, in_size, in0, in1, out_size):
    """(bounds [out_size, 2] int32 = {min, cnt}, k [out_size, ksize] int32) of one axis that takes [in0, in1) of in_size to out_size"""
    key = (f, in_size, in0, in1, out_size)
    if key in _taps:
        return _taps[key]
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[f] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(cnt):
            w.append(weight(f, (x + xmin - center + 0.5) * ss))
            ww += w[-1]
        for x in range(cnt):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(-0.5 + v * 4194304.0) if v < 0 else int(0.5 + v * 4194304.0)
        bounds[xx] = (xmin, cnt)
    bounds.setflags(write=False)
    k.setflags(write=False)
    _taps[key] = (bounds, k)
    return bounds, k


def ksize_of(f, in0, in1, out_size):
    return int(math.ceil(SUPPORT[f] * max((in1 - in0) / out_size, 1.0))) * 2 + 1


def _pass(src, bounds, k, sums=None):
    """src [n, in_size, c] uint8 resampled along axis 1 -> [n, out_size, c] uint8; sums (a list, or None): takes (min, max) of the sums
    before the clip, rounding term included"""
    out = np.zeros((src.shape[0], len(bounds), src.shape[2]), np.uint8)
    s = src.astype(np.int64)
    lo, hi = 1 << 62, -(1 << 62)
    for xx, (xmin, cnt) in enumerate(bounds):
        acc = (s[:, xmin:xmin + cnt, :] * k[xx, :cnt].astype(np.int64)[None, :, None]).sum(axis=1) + (1 << (PRECISION_BITS - 1))
        assert -(1 << 31) <= acc.min() and acc.max() < (1 << 31)                  # what the kernel's 32-bit sums lean on
        lo, hi = min(lo, int(acc.min())), max(hi, int(acc.max()))
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)                   # (>> of a negative int64 is arithmetic)
    if sums is not None:
        sums.append((lo, hi))
    return out


def resize(img, out_w, out_h, box=None, f=BILINEAR, sums=None):
    """img [h, w, c] (or [h, w]) uint8, box = (x, y, w, h) or None: the whole image -> [out_h, out_w, c] (or [out_h, out_w]) uint8.
    sums (a list, or None): takes (min, max) of the horizontal pass's sums, then of the vertical pass's."""
    flat = img.ndim == 2
    a = img[:, :, None] if flat else img
    h, w = a.shape[:2]
    x, y, bw, bh = box if box is not None else (0, 0, w, h)
    hb, hk = axis_taps(f, w, x, x + bw, out_w)
    vb, vk = axis_taps(f, h, y, y + bh, out_h)
    r0, r1 = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
    tmp = _pass(a[r0:r1], hb, hk, sums)                                # [rows the vertical taps read, out_w, c]
    vb = vb.copy()
    vb[:, 0] -= r0
    out = _pass(tmp.transpose(1, 0, 2), vb, vk, sums).transpose(1, 0, 2)
    return np.ascontiguousarray(out[:, :, 0] if flat else out)


def read_range(f, in_size, in0, in1, out_size):
    """[first, end) of the source coordinates the taps of an axis read"""
    b, _ = axis_taps(f, in_size, in0, in1, out_size)
    return int(b[0, 0]), int(b[-1, 0] + b[-1, 1])


def within_cap(f, axis):
    return ksize_of(f, axis[1], axis[2], axis[3]) <= MAX_KSIZE


def image_cases(f):
    """tests/resize_util.py's grid without its own job at the (triangle's) cap, and without the images an axis of which lies beyond this
    filter's cap (BICUBIC 40 : 1, LANCZOS 26.6 : 1: the N -> 1 axes from 63 and 65 on) -- those are refusals, beyond_cap_axes"""
    return [c for c in R.image_cases() if c != R.CAP_CASE
            and within_cap(f, (c[0], c[2][0], c[2][0] + c[2][2], c[3])) and within_cap(f, (c[1], c[2][1], c[2][1] + c[2][3], c[4]))]


def axis_cases(f):
    return [a for a in R.axis_cases() if within_cap(f, a)]


def beyond_cap_axes(f):
    return [a for a in tuple(R.axis_cases()) + tuple(R.BEYOND_CAP_AXES) if not within_cap(f, a)]


# the jobs at each filter's tap cap: 480 rows of a 33-pixel-wide picture to CAP_ROWS[f] rows -- 161 taps, one output row a tile -- and one
# step beyond it: BEYOND_ROWS[f] rows to as many
CAP_ROWS = {BOX: 3, BILINEAR: 6, HAMMING: 6, BICUBIC: 12, LANCZOS: 18}
BEYOND_ROWS = {BOX: 483, BILINEAR: 486, HAMMING: 486, BICUBIC: 481, LANCZOS: 481}


def cap_case(f):
    return (33, 480, (0, 0, 33, 480), 17, CAP_ROWS[f])


def beyond_cap_case(f):
    return (33, BEYOND_ROWS[f], (0, 0, 33, BEYOND_ROWS[f]), 17, CAP_ROWS[f])


def clip_pictures(bpp):
    """(name, img [h, w, bpp] uint8, out_w, out_h): pictures of 0 and 255 only, whose sums leave 0 .. 255 * 2^22 on both sides in both
    passes under a filter with negative taps: checkerboards of several periods, single bright and dark lines"""
    pics = []
    yy, xx = np.mgrid[0:48, 0:60]
    for p in (1, 2, 3):
        board = ((((xx // p) + (yy // p)) & 1) * 255).astype(np.uint8)
        pics.append(("checkerboard %d" % p, board, 83, 67))                      # up: the taps of the filter itself
        pics.append(("checkerboard %d down" % p, board, 41, 29))
    for v in (255, 0):
        lines = np.full((48, 60), 255 - v, np.uint8)
        lines[::7, :] = v
        lines[:, ::9] = v
        pics.append(("lines of %d" % v, lines, 97, 71))
        pics.append(("lines of %d down" % v, lines, 45, 31))
    return [(n, np.ascontiguousarray(np.repeat(a[:, :, None], bpp, axis=2)), ow, oh) for n, a, ow, oh in pics]
