"""The libjpeg-exact decode of a pixel rectangle (jda_exact_decode_surfaces_rect) stated in numpy, the rectangles its tests
decode, and an independent computation of what a rectangle reads.

Definition: the rectangle call's pixels are the whole-image twin's, cropped -- tests/exact_util.py at scale 1, tests/exact_scaled_util.py at
1/2, 1/4, 1/8 -- with one exception stated openly: at scale 1 a horizontally subsampled chroma plane at most 2 samples wide is REPLICATED
(libjpeg's rule, jdsample.c), where exact_util.twin interpolates.  reference() follows libjpeg there, so it is Pillow's crop at every size.

read_set() derives the plane samples a rectangle reads pixel by pixel from the upsampling formulas themselves (pixel 2i of a fancy 2:1 axis
reads s[i-1] and s[i], pixel 2i+1 reads s[i] and s[i+1], clamped to the component's own extent), not from the closed form the C plan uses;
mcu_rect() is the smallest MCU rectangle that holds them."""
import functools
import io

import numpy as np

from tests import coef_jpeg
from tests import exact_scaled_util as S
from tests import exact_util as X
from tests import recode_util as R

NONE, REPLICATE, FANCY = 0, 1, 2
SUB = {"gray": (0, 1), "4:4:4": (0x11, 3), "4:2:2": (0x21, 3), "4:4:0": (0x12, 3), "4:2:0": (0x22, 3)}
PER_TILE = {"gray": 64, "4:4:4": 20, "4:2:2": 16, "4:4:0": 16, "4:2:0": 10}


def axis_kinds(w, h, sampling, s):
    """(horizontal, vertical) upsampling of the chroma planes of a w x h file at scale s"""
    if sampling == "gray":
        return NONE, NONE
    hs, vs = coef_jpeg.LUMA_HV[sampling]
    if s == 1:
        narrow = hs == 2 and -(-w // hs) <= 2
        return (NONE if hs == 1 else REPLICATE if narrow else FANCY), (NONE if vs == 1 else REPLICATE if narrow else FANCY)
    kind = S.upsampling_kind(w, h, sampling, s)
    return ({S.UP_H2V1_FANCY: FANCY, S.UP_H2V1_REPLICATE: REPLICATE}.get(kind, NONE), {S.UP_H1V2_FANCY: FANCY, S.UP_H1V2_REPLICATE: REPLICATE}.get(kind, NONE))


def extents(w, h, sampling, s):
    """[(rows, cols)] of each component's own extent at scale s"""
    return S.own_extents(w, h, sampling, s) if s > 1 else X.own_extents(w, h, sampling)


def _axis_reads(kind, p0, n, ext):
    out = set()
    for p in range(p0, p0 + n):
        if kind == NONE:
            out.add(p)
        elif kind == REPLICATE:
            out.add(min(p >> 1, ext - 1))
        else:
            i = p >> 1
            out.add(i)
            out.add(min(i + 1, ext - 1) if p & 1 else max(i - 1, 0))
    return out


def read_set(w, h, sampling, s, rect, luma_only=False):
    """per decoded component (set of columns, set of rows) of its plane that the pixels of rect = (x, y, w, h) read"""
    x, y, rw, rh = rect
    out = [(set(range(x, x + rw)), set(range(y, y + rh)))]
    if sampling != "gray" and not luma_only:
        kh, kv = axis_kinds(w, h, sampling, s)
        rows, cols = extents(w, h, sampling, s)[1]
        out += [(_axis_reads(kh, x, rw, cols), _axis_reads(kv, y, rh, rows))] * 2
    return out


def samples_per_mcu(sampling, s):
    """per component (columns, rows) of samples an MCU holds at scale s"""
    hs, vs = coef_jpeg.LUMA_HV[sampling]
    ss = S.component_sizes(sampling, s)
    return [(hs * ss[0], vs * ss[0])] + [(ss[-1], ss[-1])] * (len(ss) - 1)


def mcu_rect(w, h, sampling, s, rect, luma_only=False):
    """(mx0, my0, mx1, my1), half open: the smallest MCU rectangle that holds read_set()"""
    xs, ys = [], []
    for (cols, rows), (pw, ph) in zip(read_set(w, h, sampling, s, rect, luma_only), samples_per_mcu(sampling, s)):
        xs += [min(cols) // pw, max(cols) // pw]
        ys += [min(rows) // ph, max(rows) // ph]
    return min(xs), min(ys), max(xs) + 1, max(ys) + 1


@functools.lru_cache(maxsize=None)
def reference(jpeg, s):
    """the whole image the rectangles are cropped from: the twin of scale s, with libjpeg's narrow-plane rule at scale 1"""
    t = S.twin_scaled(jpeg, s)
    if s != 1 or len(t["planes"]) == 1:
        return t
    h, w = t["gray"].shape
    hs, vs = coef_jpeg.LUMA_HV[R.decode_any(jpeg)["sampling"]]
    if hs != 2 or t["planes"][1].shape[1] > 2:
        return t
    up =[np.repeat(np.repeat(p, hs, axis=1), vs, axis=0)[:h, :w] for p in t["planes"][1:]]
    t = dict(t)
    t.update(ycc=np.stack([t["planes"][0]] + up, axis=-1), rgb=X.colour(t["planes"][0], up[0], up[1]))
    return t


def crop(jpeg, s, rect, gray=False, clip=None):
    """the surface bytes of rect = (x, y, w, h) at scale s: rows x (4 w) RGBA bytes, or rows x w gray; clip = (width_px, rows)"""
    x, y, w, h = rect
    cw, cr = (w, h) if clip is None else (max(0, min(w, clip[0])), max(0, min(h, clip[1])))
    bpp = 1 if gray else 4
    return X.rgba(reference(jpeg, s), gray)[y:y + cr, x * bpp:(x + cw) * bpp]


def pillow_crop(jpeg, s, rect, mode="RGB"):
    """Pillow's Image.open(f).crop(box), with draft() in front for s > 1 -- "RGB" (convert) or "L" (the Y plane)"""
    from PIL import Image
    x, y, w, h = rect
    if s > 1:
        full = S.pillow_scaled(jpeg, s, mode)
        return full[y:y + h, x:x + w]
    im = Image.open(io.BytesIO(jpeg))
    if mode == "L" and im.mode != "L":
        im.draft("L", im.size)
    elif mode == "RGB":
        im = im.convert("RGB")
    return np.asarray(im.crop((x, y, x + w, y + h)))


SIZES = (1, 2, 3, 4, 5, 8, 17)


def rect_set(w, h, sampling, s, thin=True):
    """the rectangles of a w x h image (ALREADY at scale s) the tests decode: origins 0..40 / s x 0..36 / s with sizes of SIZES, rectangles that end
    on the last column and row, rectangles 5 before to 5 after every seam of the planes stage's tiles, full-width rows and full-height
    columns.  thin: a deterministic subset that keeps every (x mod 16, y mod 16, w mod 4) class."""
    out = []

    def add(x, y, rw, rh):
        if 0 <= x and 0 <= y and rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h:
            out.append((x, y, rw, rh))
    k = 0
    for x in range(0, 40 // s + 1):
        for y in range(0, 36 // s + 1):
            if thin:                                                    # a width of every class modulo 4 an origin, the sizes walking through SIZES
                for c, widths in enumerate(((4, 8), (1, 5, 17), (2,), (3,))):
                    add(x, y, widths[k % len(widths)], SIZES[(k // 3 + 2 * c) % 7])
                k += 1
            else:
                for rw in SIZES:
                    for rh in SIZES:
                        add(x, y, rw, rh)
    for n in SIZES:                                                      # the last column and row: odd own extents, the clamp acts
        for m in (1, 2, 5):
            add(w - n, h - m, n, m)
            add(w - n, 0, n, m)
            add(0, h - m, n, m)
    hs, vs = coef_jpeg.LUMA_HV[sampling]
    seam = PER_TILE[sampling] * 8 * hs // s                              # pixels a planes-stage tile of the whole image at this scale
    for m in range(1, w // max(seam, 1) + 1):
        for d in range(-5, 6):
            add(m * seam + d, (7 * d) % max(h - 3, 1), SIZES[(d + 5) % 7], 3)
            add(m * seam + d - 4, h // 2, 9, 2)
    for y in (0, h // 2, h - 1):
        add(0, y, w, 1)
    for x in (0, w // 2, w - 1):
        add(x, 0, 1, h)
    seen, uniq = set(), []
    for r in out:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    return uniq


@functools.lru_cache(maxsize=None)
def fixture(sampling):
    """the 333 x 217 file of a layout (4:4:0: from the suite's own writer, as the cases have no such file)"""
    from tests.cases import jpeg_for
    name = {"gray": "gray_333x217", "4:4:4": "c444_333x217", "4:2:0": "c420_333x217", "4:2:2": "c422_333x217"}.get(sampling)
    return jpeg_for(name) if name else X.written_file(333, 217, sampling, 90)


@functools.lru_cache(maxsize=None)
def small_files(sampling):
    """[(jpeg, (w, h))]: a 17 x 9 and a 5 x 7 file of the layout that the front end takes"""
    out = []
    for w, h in ((17, 9), (5, 7)):
        f = X.written_file(w, h, sampling, 100) if sampling == "4:4:0" else S.pillow_file(w, h, sampling, 95)
        if len(f) < 256 and sampling != "4:4:0":
            f = X.pillow_file(w, h, sampling, 100, "baseline", "noise")
        if len(f) >= 256:
            out.append((f, (w, h)))
    return out
