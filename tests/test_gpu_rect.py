"""Crop-aware decode on the GPU: jda_batch_create_rect (one rectangle of MCUs per image, tiles cut from the rectangle's first MCU)
and jda_decode_to_host_rect, bit-exact against the reference tests/test_rect_cpu.py holds the wave emulator to -- the oracle's canvas
of the whole image inside the rectangle's decodable MCUs, the guard byte everywhere else (tests/rect_cases.py: expected_surface).
Every device surface is filled with 0x5a before the decode and has a pitch wider than its rows, so a byte stored outside a
rectangle -- a zero included --, in the pitch padding or between two surfaces shows.  What only the GPU side has is in play: many
rectangles of one image in one launch list (the persistent tile-to-wavefront mapping), padding tiles between images, a shared table
generation, holes, and the clear and copy-back of a rectangle's rows in jda_decode_to_host_bands."""
import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.synth import synth_jpeg
from tests import orient_util as U
from tests import rect_cases as R
from tests.cases import coef_jpeg_for, jpeg_for
from tests.test_rect_cpu import bad_mcu_rects, window_rects

pytestmark = pytest.mark.gpu

FILL = 0x5a          # what every device surface holds before a decode
GUARD = 0x33         # what a host canvas holds before jda_decode_to_host_rect


class Resident:
    """files prepared and uploaded once: key -> (jpeg, DeviceImage, MCU columns, MCU rows, MCUs per tile)"""

    def __init__(self, ctx):
        self.ctx, self.items, self.preps = ctx, {}, []

    def add(self, key, jpeg, device_prescan=False, flags=0):
        p = J.PreparedImage(jpeg, device_prescan=device_prescan, flags=flags)
        self.preps.append(p)
        d = J.DeviceImage(self.ctx, p)
        per = {0x22: 10, 0x11: 20, 0x21: 16, 0x12: 16}[p.info.subsample] if p.info.ncomp == 3 else 64      # jda_mcus_per_tile
        self.items[key] = (jpeg, d, p.info.mcus_x, p.info.mcus_y, per)
        return p, d

    def close(self):
        for _, d, _, _, _ in self.items.values():
            d.close()
        for p in self.preps:
            p.close()


def check_plan(ctx, oracle, res, entries):
    """entries: (key of a resident file or None for a hole, pixel type, options, rectangle, MCUs in front of a bad one or None).
    ONE Batch over all of them, each with a surface of its own inside one allocation filled with 0x5a, ONE decode: the whole
    allocation must be what expected_surface says, the status index-aligned, the tile counts those of the rectangles."""
    outs, places, total = [], [], 0
    for key, pt, opt, rect, nok in entries:
        if key is None:
            row, rows = 48, 8                          # a hole's surface: never looked at by the plan
        else:
            g = J.output_geometry(res.items[key][1].info, pt, opt)
            row, rows = g["canvas_w"] * g["bpp"], g["canvas_h"]
        pitch = ((row + 15) & ~15) + 16                # wider than the row
        places.append((total, pitch, row, rows))
        total += (pitch * rows + 255) & ~255
    base = ctx.malloc(total)
    try:
        ctx.memset(base, FILL, total)
        for (key, pt, opt, rect, nok), (off, pitch, row, rows) in zip(entries, places):
            px = 12 if key is None else J.output_geometry(res.items[key][1].info, pt, opt)["canvas_w"]
            outs.append((base + off, pitch, px, rows))
        b = J.Batch(ctx, [None if e[0] is None else res.items[e[0]][1] for e in entries], outs, [e[1] for e in entries], [e[2] for e in entries],
                    mcu_rects=[e[3] for e in entries])
        try:
            b.decode()
            ctx.sync()
            status, stats = b.status(), dict(b.stats)
        finally:
            b.close()
        got = ctx.to_host(base, total)
    finally:
        ctx.free(base)
    exp = np.full(total, FILL, np.uint8)
    tiles = whole = 0
    for (key, pt, opt, rect, nok), (off, pitch, row, rows) in zip(entries, places):
        if key is None:
            continue
        jpeg, _, mx, my, per = res.items[key]
        want = R.oracle_canvas(oracle, key, jpeg, pt, opt, must_succeed=nok is None)
        assert want.shape == (rows, row), (key, pt, opt, want.shape, rows, row)
        exp[off:off + pitch * rows].reshape(rows, pitch)[:, :row] = R.expected_surface(want, rect, R.geometry_of(want, mx, my), nok, FILL)
        tiles += R.tile_count(rect, mx, my, per)
        whole += R.whole_tiles(mx, my, per)
    for i, ((key, pt, opt, rect, nok), (off, pitch, row, rows)) in enumerate(zip(entries, places)):
        a, e = got[off:off + pitch * rows], exp[off:off + pitch * rows]
        assert np.array_equal(a, e), (i, key, pt, opt, rect, int(np.count_nonzero(a != e)))
    assert np.array_equal(got, exp)                                                            # (.. and the bytes between the surfaces)
    assert status == [1 if e[0] is None else (0 if e[4] is None else 2) for e in entries], status
    # tiles: the tiles with work; tiles_whole_images: what the plan's images (holes not counted) would take as whole images
    assert (stats["tiles"], stats["tiles_whole_images"]) == (tiles, whole), (stats, tiles, whole)
    return stats


def plan_of(short, key, other, pt, opt, rects):
    """every rectangle as an entry of its own over the SAME resident image; in the middle an image with other tables, a hole and the
    empty rectangle"""
    mx, my, per = R.LAYOUTS[short][3:6]
    entries = [(key, pt, opt, r, None) for r in rects]
    mid = len(entries) // 2
    entries[mid:mid] = [(other, pt, opt, (2, 0, per + 3, my), None), (None, pt, opt, None, None), (key, pt, opt, (2, 1, 2, 2), None)]
    return entries


@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_one_plan_per_image_and_mode(short, dri, gpu_ctx, oracle):
    """4a: per mode ONE plan that holds every rectangle of the matrix (the same DeviceImage repeated -- accepted as it is, no copies
    are uploaded), and the rectangles that leave the image (4e)"""
    res = Resident(gpu_ctx)
    try:
        res.add((short, dri), R.rect_jpeg(short, dri))
        res.add((short, "other"), R.other_tables_jpeg(short))
        for pt, opt in R.modes_of(short):
            check_plan(gpu_ctx, oracle, res, plan_of(short, (short, dri), (short, "other"), pt, opt, R.rects_of(short) + R.odd_rects_of(short)))
    finally:
        res.close()


def test_one_mixed_plan(gpu_ctx, oracle):
    """4b: the five layouts with and without restart intervals, every mode, a rectangle per image, a stream with a bad MCU and a
    hole in ONE batch: several launch lists, each with images of different geometry and padding tiles between them"""
    res = Resident(gpu_ctx)
    try:
        entries = []
        bad, nok = U.bad_mcu_jpeg()
        res.add("bad_mcu", bad)
        for i, (short, dri) in enumerate(R.IMAGES):
            res.add((short, dri), R.rect_jpeg(short, dri))
            modes, rects = R.modes_of(short), R.rects_of(short)
            for k in range(len(modes)):
                entries.append(((short, dri), modes[(i + k) % len(modes)][0], modes[(i + k) % len(modes)][1], rects[(3 * i + 7 * k) % len(rects)], None))
            if i == 4:
                entries.append((None, J.RGB8888, 0, None, None))
                info = J.parse(bad)
                for k, rect in enumerate(bad_mcu_rects(info["mcus_x"], info["mcus_y"], nok)):
                    entries.append(("bad_mcu", R.MODES[k % len(R.MODES)][0], R.MODES[k % len(R.MODES)][1], rect, nok))
        assert len({(e[0], e[3]) for e in entries}) > 40
        st = check_plan(gpu_ctx, oracle, res, entries)
        assert st["n_launches"] >= 10, st
    finally:
        res.close()


def host_expected(want, rect, geometry, shape, nok=None):
    """a guard-filled host array after jda_decode_to_host_rect: the MCU rows of the (clamped) rectangle are written -- zeros left and
    right of it and from a bad MCU on, the oracle's bytes in it --, every other row, the pitch padding and rows behind the canvas keep the guard"""
    mx, my, mb, mr = geometry
    exp = np.full(shape, GUARD, np.uint8)
    x0, y0, x1, y1 = R.clamp_rect(rect, mx, my)
    if y1 > y0:
        exp[y0 * mr:y1 * mr, :want.shape[1]] = R.expected_surface(want, rect, geometry, nok, 0)[y0 * mr:y1 * mr]
    return exp


def check_to_host(ctx, oracle, key, jpeg, dirty, pt, opt, rect, mx, my, per, nok=None):
    want = R.oracle_canvas(oracle, key, jpeg, pt, opt, must_succeed=nok is None)
    # a whole decode of another image of the same geometry first: the pooled device canvas the rectangle is decoded into holds pixels
    rc, _, _ = J.decode_to_host(ctx, dirty, pt, opt)
    assert rc == 0
    host = np.full((want.shape[0] + 3, want.shape[1] + 24), GUARD, np.uint8)
    rc, got, g, tiles = J.binding.decode_to_host_rect(ctx, jpeg, pt, opt, rect, out=host)
    assert got is host and rc == (0 if nok is None else 2), (key, pt, opt, rect, rc)
    exp = host_expected(want, rect, R.geometry_of(want, mx, my), host.shape, nok)
    assert np.array_equal(host, exp), (key, pt, opt, rect, int(np.count_nonzero(host != exp)))
    assert tiles == (R.tile_count(rect, mx, my, per), R.whole_tiles(mx, my, per)), (key, pt, opt, rect, tiles)
    assert g["mcus_decoded"] == (mx * my if nok is None else nok)


@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_decode_to_host_rect(short, dri, gpu_ctx, oracle):
    """4c (and 4e through the one-call entry point): only the rectangle's MCU rows are cleared, decoded and copied back"""
    mx, my, per = R.LAYOUTS[short][3:6]
    for pt, opt in R.modes_of(short):
        for rect in R.rects_of(short) + R.odd_rects_of(short):
            check_to_host(gpu_ctx, oracle, (short, dri), R.rect_jpeg(short, dri), R.other_tables_jpeg(short), pt, opt, rect, mx, my, per)


def test_decode_to_host_rect_on_a_stream_with_a_bad_mcu(gpu_ctx, oracle):
    """zeros from the bad MCU on inside the rectangle's rows, JDA_DECODE_ERROR, the MCUs in front of the bad one reported"""
    jpeg, nok = U.bad_mcu_jpeg()
    info = J.parse(jpeg)
    mx, my = info["mcus_x"], info["mcus_y"]
    for pt, opt in R.MODES:
        for rect in bad_mcu_rects(mx, my, nok):
            check_to_host(gpu_ctx, oracle, "bad_mcu", jpeg, jpeg_for("c420_333x217"), pt, opt, rect, mx, my, 10, nok)


@pytest.mark.parametrize("short", ["c420", "c444"])
def test_rectangles_with_continuation_entries(short, gpu_ctx, oracle):
    """4d: JDA_PREPARE_CONT_ALWAYS images at RGB8888 (P1 in chunks): a tile that starts at any block finds its own entries"""
    res = Resident(gpu_ctx)
    try:
        res.add((short, "other"), R.other_tables_jpeg(short))
        for dri in (False, True):
            p, d = res.add((short, dri), R.rect_jpeg(short, dri), flags=J.PREPARE_CONT_ALWAYS)
            assert len(p.block_cont()[1]) > 0, (short, dri)
            check_plan(gpu_ctx, oracle, res, plan_of(short, (short, dri), (short, "other"), J.RGB8888, 0, R.rects_of(short)))
    finally:
        res.close()


@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_rectangles_over_a_device_made_index(short, dri, gpu_ctx, oracle):
    """4d: the per-block index made by the segment walk on the GPU (canonical reader phases)"""
    res = Resident(gpu_ctx)
    try:
        p, d = res.add((short, dri), R.rect_jpeg(short, dri), device_prescan=True)
        assert d.prescan_on_device, (short, dri)
        res.add((short, "other"), R.other_tables_jpeg(short), device_prescan=True)
        for pt, opt in R.modes_of(short):
            check_plan(gpu_ctx, oracle, res, plan_of(short, (short, dri), (short, "other"), pt, opt, R.rects_of(short)))
    finally:
        res.close()


@pytest.mark.parametrize("short", R.SHORTS)
def test_rectangles_on_the_window_stress_streams(short, gpu_ctx, oracle):
    """4d: the k_window_* files of tests/test_rect_cpu.py with rectangles shifted by half a tile, host index and device pre-scan: the
    layout was chosen from the whole image's tiling, a shifted tile's slice may be over its window and then reads HBM"""
    plain = J.GRAY8 if short == "gray" else J.RGB8888
    per = R.LAYOUTS[short][5]
    for device_prescan in (False, True):
        res = Resident(gpu_ctx)
        try:
            entries = []
            for kind in ("small_tight", "large"):
                name = "k_window_%s_%s" % (short, kind)
                p, d = res.add(name, coef_jpeg_for(name), device_prescan=device_prescan)
                for pt, opt in ((plain, 0), (J.RGB565_BE, J.SCALE_HALF), (J.GRAY8, J.SCALE_QUARTER)):
                    entries += [(name, pt, opt, rect, None) for rect in window_rects(p.info.mcus_x, p.info.mcus_y, per)]
            check_plan(gpu_ctx, oracle, res, entries)
        finally:
            res.close()


def test_gray_thumbnail_and_quarter_tiles_wider_than_four_tiles(gpu_ctx, oracle):
    """The DC thumbnail kernel packs four whole gray tiles side by side (256 pixels of a row) when the run starts at a multiple of four
    MCUs, and the 1/4 kernel stores a whole gray tile from shared rows when it starts on a dword: a file wide enough for both, with
    rectangles that start on and off those boundaries"""
    wide = synth_jpeg(2397, 20, "gray", seed=5)
    res = Resident(gpu_ctx)
    try:
        p, d = res.add("gray_wide", wide)
        mx, my = p.info.mcus_x, p.info.mcus_y
        assert (mx, my) == (300, 3)
        rects = [(0, 0, mx, my), (4, 0, 260, my), (1, 0, 257, my), (2, 1, mx, 2), (3, 0, 259 + 64, my), (64, 1, mx, my), (44, 0, mx, my), (8, 2, 8 + 255, my)]
        for pt, opt in ((J.GRAY8, J.SCALE_EIGHTH), (J.GRAY8, J.SCALE_QUARTER), (J.RGB565_LE, J.SCALE_EIGHTH), (J.RGB565_BE, J.SCALE_QUARTER)):
            check_plan(gpu_ctx, oracle, res, [("gray_wide", pt, opt, r, None) for r in rects])
    finally:
        res.close()
