"""TEST INFRASTRUCTURE: jda_resize_surfaces restated in numpy -- Pillow's Image.resize((ow, oh), Image.BILINEAR, box=(x, y, x + w, y + h)).

numpy only (the GPU machine may have no Pillow; tests/test_resize_cpu.py holds this twin to Pillow where Pillow is).  Knows nothing of
tiles, lanes or LDS: per axis the taps of Pillow's precompute_coeffs / normalize_coeffs_8bpc for the bilinear (triangle) filter, worked
out in Python floats (IEEE double, no fused multiply-add) in Pillow's order of operations; then the horizontal pass over the source rows
the vertical taps read, into 8-bit intermediates, and the vertical pass over those."""
import math

import numpy as np

PRECISION_BITS = 22
MAX_KSIZE = 161                      # JDA_RESIZE_MAX_KSIZE
MAX_TABLE_BYTES = 64 << 20           # JDA_RESIZE_MAX_TABLE_BYTES

# source and output sizes of the test grid, on each axis
SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 217, 333)


def axis_taps(in_size, in0, in1, out_size):
    """(bounds [out_size, 2] int32 = {min, cnt}, k [out_size, ksize] int32) of one axis that takes [in0, in1) of in_size to out_size"""
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    support = fs
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
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
            ww += w[-1]
        for x in range(cnt):
            k[xx, x] = int(0.5 + (w[x] / ww if ww != 0.0 else w[x]) * 4194304.0)
        bounds[xx] = (xmin, cnt)
    return bounds, k


def axis_cases():
    """(in_size, in0, in1, out_size) of the grid's pairs: every upscale and downscale class, equal sizes, N -> 1 (up to 65 -> 1; 217 -> 1
    and 333 -> 1 lie beyond the cap of 80 : 1 and are refusals, BEYOND_CAP_AXES), 1 -> N, and boxes that touch each edge, lie inside, or
    are one pixel"""
    cases = []
    for a in SIZES:
        for b in SIZES:
            if a == b or a == 1 or (b == 1 and a <= MAX_KSIZE // 2) or (a, b) in ((2, 3), (3, 2), (15, 16), (16, 17), (17, 15), (63, 64), (65, 64), (64, 17), (17, 64), (333, 217),
                                                      (217, 333), (333, 15), (15, 333), (217, 16), (16, 217), (217, 3), (3, 333), (65, 217), (333, 63)):
                cases.append((a, 0, a, b))
    for a, b in ((17, 16), (64, 15), (65, 3), (217, 64), (333, 65), (333, 333), (63, 217)):
        q = max(a // 4, 1)
        cases.append((a, 0, a - q, b))               # touches the left / top edge
        cases.append((a, q, a, b))                   # .. the right / bottom edge
        if a - 2 * q > 0:
            cases.append((a, q, a - q, b))           # inside
        cases.append((a, a // 2, a // 2 + 1, b))     # one pixel
        cases.append((a, 0, 1, b))
        cases.append((a, a - 1, a, b))
    return cases


def _pass(src, bounds, k):
    """src [n, in_size, c] uint8 resampled along axis 1 -> [n, out_size, c] uint8"""
    out = np.zeros((src.shape[0], len(bounds), src.shape[2]), np.uint8)
    s = src.astype(np.int64)
    for xx, (xmin, cnt) in enumerate(bounds):
        acc = (s[:, xmin:xmin + cnt, :] * k[xx, :cnt].astype(np.int64)[None, :, None]).sum(axis=1) + (1 << (PRECISION_BITS - 1))
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, out_w, out_h, box=None):
    """img [h, w, c] (or [h, w]) uint8, box = (x, y, w, h) or None: the whole image -> [out_h, out_w, c] (or [out_h, out_w]) uint8"""
    flat = img.ndim == 2
    a = img[:, :, None] if flat else img
    h, w = a.shape[:2]
    x, y, bw, bh = box if box is not None else (0, 0, w, h)
    hb, hk = axis_taps(w, x, x + bw, out_w)
    vb, vk = axis_taps(h, y, y + bh, out_h)
    r0, r1 = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
    tmp = _pass(a[r0:r1], hb, hk)                                      # [rows the vertical taps read, out_w, c]
    vb = vb.copy()
    vb[:, 0] -= r0
    out = _pass(tmp.transpose(1, 0, 2), vb, vk).transpose(1, 0, 2)
    return np.ascontiguousarray(out[:, :, 0] if flat else out)


def read_range(in_size, in0, in1, out_size):
    """[first, end) of the source coordinates the taps of an axis read"""
    b, _ = axis_taps(in_size, in0, in1, out_size)
    return int(b[0, 0]), int(b[-1, 0] + b[-1, 1])


# the job at the tap cap: 480 rows to 6 is 80 : 1, JDA_RESIZE_MAX_KSIZE = 161 taps, and two output rows' taps span more source rows than
# the LDS budget holds: one output row a tile; one step beyond the cap
CAP_CASE = (33, 480, (0, 0, 33, 480), 17, 6)
BEYOND_CAP_CASE = (33, 161, (0, 0, 33, 161), 17, 2)
BEYOND_CAP_AXES = ((161, 0, 161, 2), (217, 0, 217, 1), (333, 0, 333, 1), (333, 0, 333, 2), (333, 50, 300, 3))


def image_cases():
    """(w, h, (x, y, bw, bh), out_w, out_h): every axis case of the grid as the horizontal axis of one image and as the vertical axis of
    another (paired with a stride that is coprime to their number), then the job at the cap"""
    ax = axis_cases()
    n = len(ax)
    cases = []
    for i in range(n):
        (w, x0, x1, ow), (h, y0, y1, oh) = ax[i], ax[(i * 37 + 11) % n]
        cases.append((w, h, (x0, y0, x1 - x0, y1 - y0), ow, oh))
    cases.append(CAP_CASE)
    return cases


def pitch_of(width_px, bpp, extra=0):
    return ((width_px * bpp + 15) & ~15) + 16 * extra
