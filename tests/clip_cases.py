"""The output clip (jda_output::width_px x rows): the clips, the two surface shapes and the ONE reference both tests/test_clip_cpu.py
(the wave emulator) and tests/test_gpu_clip.py (the kernels) are held to.

A decode never writes a pixel at or behind min(width_px, canvas_w) in a row, nor a row at or behind min(rows, canvas_h).  The images and
modes are those of tests/rect_cases.py: every MCU row has two whole tiles and a short one, the last MCU column and row are partial.  The
clip lists put a clip on, one before and one behind the 4-pixel store group, the 8-pixel gray chunk, the 4:2:0 row pair (odd row counts),
the MCU edge, the tile edge, the visible edge and the canvas edge; a clip behind the canvas clamps to it, a clip of 0 writes nothing.
The reference is the guard byte everywhere except the oracle's canvas inside the clip."""
import ctypes as C
import functools

import numpy as np

import jpegdec_amd as J
from tests import rect_cases as R

BPP = {J.RGB8888: 4, J.RGB565_LE: 2, J.RGB565_BE: 2, J.GRAY8: 1}
SHAPES = ("wide", "tight")


def scale_shift(opt):
    return 1 if opt & J.SCALE_HALF else 2 if opt & J.SCALE_QUARTER else 3 if opt & J.SCALE_EIGHTH else 0


def align16(n):
    return (n + 15) & ~15


@functools.lru_cache(maxsize=None)
def visible_size(jpeg, pt, opt):
    """(out_w, out_h) of jda_output_geometry"""
    info = J.binding.ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    g = J.output_geometry(info, pt, opt)
    return g["out_w"], g["out_h"]


def geometry_of(mx, my, per, mw, mh, pt, opt, visible):
    """everything in OUTPUT pixels: s the scale shift, mwo x mho an MCU, tw a whole tile, cw x ch the canvas, vw x vh the visible size"""
    s = scale_shift(opt)
    mwo, mho = mw >> s, mh >> s
    return dict(s=s, bpp=BPP[pt], mx=mx, my=my, per=per, mwo=mwo, mho=mho, tw=per * mwo, cw=mx * mwo, ch=my * mho, vw=visible[0], vh=visible[1])


def file_geometry(jpeg, pt, opt):
    """the same of any baseline file (or a progressive one with PROGRESSIVE_FULL in opt), from its header"""
    i = J.parse(jpeg)
    per = {0x22: 10, 0x11: 20, 0x21: 16, 0x12: 16}[i["subsample"]] if i["ncomp"] == 3 else 64          # jda_mcus_per_tile
    return geometry_of(i["mcus_x"], i["mcus_y"], per, i["mcu_w"], i["mcu_h"], pt, opt, visible_size(jpeg, pt, opt))


def geometry(short, pt, opt):
    mx, my, per, mw, mh = R.LAYOUTS[short][3:8]
    return geometry_of(mx, my, per, mw, mh, pt, opt, visible_size(R.rect_jpeg(short), pt, opt))


def _merged(values):
    out = []
    for v in values:
        if v >= 0 and v not in out:
            out.append(v)
    return out


def widths_of(g):
    tw, mwo, vw, cw = g["tw"], g["mwo"], g["vw"], g["cw"]
    return _merged([0, 1, 3, 4, 5, 7, 8, 9, tw - 1, tw, tw + 1, tw + 3, 2 * tw - 1, 2 * tw, 2 * tw + mwo, vw, cw - 1, cw, cw + 9])


def rows_of(g):
    mho, vh, ch = g["mho"], g["vh"], g["ch"]
    return _merged([0, 1, 2, 3, mho - 1, mho, mho + 1, 2 * mho - 1, 2 * mho, vh, ch - 1, ch, ch + 9])


def clips_from(g):
    """(width_px, rows) pairs: not the cross product -- every width once, every row count once, and the three clips a caller writes most"""
    ws, rs = widths_of(g), rows_of(g)
    pairs = [(w, rs[(5 * i + 2) % len(rs)]) for i, w in enumerate(ws)]
    pairs += [(ws[(7 * j + 3) % len(ws)], r) for j, r in enumerate(rs)]
    pairs += [(0, g["ch"]), (g["cw"], 0), (g["vw"], g["vh"])]
    out = []
    for p in pairs:
        if p not in out:
            out.append(p)
    return out


def clips_of(short, pt, opt):
    return clips_from(geometry(short, pt, opt))


def rect_clips(g):
    """the clips that go with an MCU rectangle or a bad MCU: just behind the first tile and MCU row, one short of the canvas, the visible size"""
    return [(g["tw"] + 1, g["mho"] + 1), (g["cw"] - 1, g["ch"] - 1), (g["vw"], g["vh"])]


def clip_rects(short):
    """the rectangles of rects_of that go with a clip: straddling a tile edge, reaching the partial corner, clamped"""
    r = R.rects_of(short)
    return [r[2], r[4], r[9]]


def cuts(clips, g):
    """which of the decode kernel's internal edges the list cuts: a tile on the right (not at an MCU edge), a tile at the bottom (inside an
    MCU row), at an odd row, at a width that is no multiple of the 4-pixel store group, and the two no-ops"""
    cw, ch, tw, mho = g["cw"], g["ch"], g["tw"], g["mho"]
    inside = [(min(w, cw), min(r, ch)) for w, r in clips]
    return dict(right=any(0 < w < cw and w % tw and r > 0 for w, r in inside), bottom=any(0 < r < ch and (r % mho or mho == 1) and w > 0 for w, r in inside),
                odd_row=any(r & 1 and r < ch and w > 0 for w, r in inside), off_group=any(w % 4 and w < cw and r > 0 for w, r in inside),
                nothing=any(w == 0 for w, r in inside) and any(r == 0 for w, r in inside), clamped=any(w > cw for w, r in clips) and any(r > ch for w, r in clips))


def surface_shape(shape, w, rows, g):
    """(pitch, surface rows) of a clip's surface.  wide: the canvas row rounded up to 16 plus 32 bytes, two guard rows behind the canvas.
    tight: the clipped row rounded up to 16 (at least 16), one guard row behind the clipped rows -- surfaces that lie back to back"""
    if shape == "wide":
        return align16(g["cw"] * g["bpp"]) + 32, g["ch"] + 2
    assert shape == "tight"
    return max(16, align16(min(w, g["cw"]) * g["bpp"])), min(rows, g["ch"]) + 1


def expected_clipped(want, w, rows, bpp, pitch, surf_rows, rect=None, nok=None, guard=0x33, mcus=None, zeros=False):
    """What a decode under the clip (w, rows) leaves in a surface of surf_rows x pitch bytes that held `guard` everywhere: the oracle's bytes
    (want: its MCU-padded canvas of the whole image) in [0, min(rows, ch)) x [0, min(w, cw) * bpp), the guard in every other byte.  With an
    MCU rectangle or a bad MCU (nok: the MCUs in front of it; mcus = (MCU columns, MCU rows)) that region is cut down to what
    rect_cases.expected_surface leaves.  zeros: the one-call and pipeline paths' promise for a bad image -- zeros from the bad MCU on --,
    kept inside the clip as well."""
    ch, cwb = want.shape
    out = np.full((surf_rows, pitch), guard, np.uint8)
    rr, wb = min(max(rows, 0), ch), min(max(w, 0) * bpp, cwb)
    assert rr <= surf_rows and wb <= pitch
    src = want
    if rect is not None or nok is not None:
        mx, my = mcus
        src = R.expected_surface(want, rect if rect is not None else (0, 0, mx, my), R.geometry_of(want, mx, my), nok, 0 if zeros else guard)
    out[:rr, :wb] = src[:rr, :wb]
    return out


def hostsim_decode(sim, jpeg, pt, opt, surface, width_px=None, rows=None):
    """one emulated decode into `surface` (2-D uint8, C order, its row length is the pitch); the clip defaults to the whole canvas.
    -> the emulator's status"""
    if width_px is None or rows is None:
        info = J.parse(jpeg)
        s = scale_shift(opt | (J.SCALE_EIGHTH if info["jpeg_type"] == 1 else 0))
        width_px = info["mcus_x"] * (info["mcu_w"] >> s) if width_px is None else width_px
        rows = info["mcus_y"] * (info["mcu_h"] >> s) if rows is None else rows
    assert surface.dtype == np.uint8 and surface.flags["C_CONTIGUOUS"] and surface.ndim == 2
    return sim.hostsim_decode(jpeg, len(jpeg), pt, opt, surface.ctypes.data_as(C.c_void_p), surface.shape[1], width_px, rows)
