"""Crop-aware decode (an MCU rectangle handed to jda_append_strips): the images, rectangles, modes and the ONE reference both
tests/test_rect_cpu.py (the wave emulator) and tests/test_gpu_rect.py (the kernels) are held to.

The images are the smallest that give every MCU row two whole tiles and a short one, a partial last MCU column and row, and three
MCU rows -- so a rectangle can start and end on, one before and one behind every kind of tile edge.  The reference is the oracle's
canvas of the WHOLE image with everything outside the rectangle's decodable MCUs replaced by a guard byte: a tile that starts at
the wrong MCU, runs past the rectangle, or stores a byte outside its MCUs shows as a difference."""
import functools

import numpy as np

import jpegdec_amd as J
from jpegdec_amd.synth import synth_jpeg

# short name -> (sampling, width, height, MCU columns, MCU rows, MCUs per tile (jda_mcus_per_tile), MCU width, MCU height in pixels)
LAYOUTS = {
    "c420": ("4:2:0", 393, 40, 25, 3, 10, 16, 16),
    "c444": ("4:4:4", 357, 20, 45, 3, 20, 8, 8),
    "c422": ("4:2:2", 589, 20, 37, 3, 16, 16, 8),
    "c440": ("4:4:0", 293, 40, 37, 3, 16, 8, 16),
    "gray": ("gray", 1197, 20, 150, 3, 64, 8, 8),
}
SHORTS = tuple(LAYOUTS)
IMAGES = tuple((s, dri) for s in SHORTS for dri in (False, True))
RESTART_BLOCKS = 7

MODES = ((J.RGB8888, 0), (J.RGB565_LE, 0), (J.GRAY8, 0), (J.RGB565_BE, J.SCALE_HALF), (J.GRAY8, J.SCALE_QUARTER), (J.RGB565_LE, J.SCALE_QUARTER),
         (J.GRAY8, J.SCALE_EIGHTH), (J.RGB565_BE, J.SCALE_EIGHTH), (J.RGB8888, J.SCALE_EIGHTH))


def modes_of(short):
    """every mode; a gray file is not asked for RGB8888 (the reference draws RGB565 at 32 bpp there)"""
    return tuple(m for m in MODES if not (short == "gray" and m[0] == J.RGB8888))


@functools.lru_cache(maxsize=None)
def rect_jpeg(short, dri=False):
    sampling, w, h = LAYOUTS[short][:3]
    return synth_jpeg(w, h, sampling, seed=5, restart_blocks=RESTART_BLOCKS if dri else 0)


@functools.lru_cache(maxsize=None)
def other_tables_jpeg(short):
    """the same geometry with other quantisation tables and other pixels: a second table generation in a launch list"""
    sampling, w, h = LAYOUTS[short][:3]
    return synth_jpeg(w, h, sampling, seed=9, quality=60)


def rects_of(short):
    """the rectangles of the matrix, in MCUs, half open -- as the caller writes them (not clamped)"""
    mx, my, per = LAYOUTS[short][3:6]
    r = [(0, 0, mx, my),                       # the whole image
         (1, 0, 2, 1),                         # one MCU
         (per - 1, 1, per + 1, 2),             # straddles a whole-image tile edge
         (per, 0, 2 * per, my),                # exactly the second tile of every row
         (3, 1, mx, my),                       # off the boundary to the partial last column and row
         (mx - 1, my - 1, mx, my),             # the partial corner MCU
         (per + 3, 0, 2 * per + 5, my),        # a whole tile and a short one, both off the whole image's boundaries
         (1, 1, 1 + per, 2),                   # one whole tile one MCU off
         (2, 1, 2, 2),                         # empty
         (0, 0, mx + 5, my + 5)]               # clamped
    if short == "gray":
        # sub-dword starts at 1/4 and 1/8 scale (an MCU is 2 or 1 pixels wide there): the 1/4 kernel's shared store and the DC
        # thumbnail's packed path must hand over to their general paths
        for x0 in (1, 2, 3, 5, 63, 65, 67):
            r += [(x0, 2, x0 + 1, 3), (x0, 1, x0 + 3, 2), (x0, 1, x0 + 66, 3)]
    return r


# rectangles that leave the image, lie behind it or are inverted: jda_append_strips clamps the lower corner at 0 and the upper one
# into the image; what is left empty launches nothing
def odd_rects_of(short):
    mx, my, per = LAYOUTS[short][3:6]
    return [(-3, -2, 4, 2), (mx - 2, my - 1, mx + 9, my + 9), (5, 2, 3, 1), (mx + 1, 0, mx + 4, 1), (0, 0, -1, -1), (-5, -5, 0, 0),
            (per + 1, my, per + 5, my + 2), (-(1 << 20), 1, 1 << 20, 2)]


def clamp_rect(rect, mx, my):
    """jda_append_strips' clamp: (x0, y0, x1, y1); empty where x0 >= x1 or y0 >= y1"""
    x0, y0 = max(0, rect[0]), max(0, rect[1])
    x1 = 0 if rect[2] < 0 else min(rect[2], mx)
    y1 = 0 if rect[3] < 0 else min(rect[3], my)
    return x0, y0, x1, y1


def tile_count(rect, mx, my, per):
    """tiles with work of one rectangle: every MCU row of it is cut into runs of per MCUs from ITS first MCU"""
    x0, y0, x1, y1 = clamp_rect(rect, mx, my)
    if x0 >= x1 or y0 >= y1:
        return 0
    return (y1 - y0) * ((x1 - x0 + per - 1) // per)


def whole_tiles(mx, my, per):
    return my * ((mx + per - 1) // per)


def geometry_of(want, mx, my):
    """(MCU columns, MCU rows, bytes of an MCU in a canvas row, rows of an MCU) of an MCU-padded canvas"""
    assert want.shape[1] % mx == 0 and want.shape[0] % my == 0
    return mx, my, want.shape[1] // mx, want.shape[0] // my


def expected_surface(want, rect, geometry, nok=None, guard=0x33):
    """What a crop-aware decode leaves in a surface that held `guard` everywhere: the oracle's bytes (want: its MCU-padded canvas of
    the whole image, padding area included) in the MCUs of the clamped rectangle whose scan index is < nok (None: all are decodable),
    the guard in every other byte."""
    mx, my, mb, mr = geometry
    out = np.full_like(want, guard)
    x0, y0, x1, y1 = clamp_rect(rect, mx, my)
    if nok is None:
        nok = mx * my
    for y in range(y0, y1):
        xe = min(x1, nok - y * mx)          # MCUs of this row in front of the bad one
        if xe > x0:
            out[y * mr:(y + 1) * mr, x0 * mb:xe * mb] = want[y * mr:(y + 1) * mr, x0 * mb:xe * mb]
    return out


_canvas = {}


def oracle_canvas(oracle, key, jpeg, pt, opt, must_succeed=True):
    """the oracle's canvas of the whole image, computed once per (image, mode) and shared (read-only)"""
    k = (key, pt, opt)
    if k not in _canvas:
        rc, want, err = oracle.decode_canvas(jpeg, pt, opt)
        assert rc == 1 or not must_succeed, (key, pt, opt, err)
        want.setflags(write=False)
        _canvas[k] = want
    return _canvas[k]
