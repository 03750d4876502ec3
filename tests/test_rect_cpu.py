"""Crop-aware decode without a GPU: the wave emulator (tests/hostsim) runs the tiles jda_append_strips cuts from an MCU rectangle
-- tiles whose boundaries are not the whole image's -- into a canvas filled with a guard byte.  The canvas must then hold the
oracle's bytes in the rectangle's MCUs and the guard in every other byte (tests/rect_cases.py: expected_surface): a tile that starts
at the wrong MCU, overruns the rectangle or stores outside its MCUs shows.  Five layouts, with and without restart intervals, nine
(pixel type, scale) pairs; the plain run, P1 in chunks, a 64-byte scan window with the tiles in reverse order, the device pre-scan's
index, a stream with a bad MCU and the scan-window stress streams with rectangles shifted by half a tile."""
import ctypes as C

import numpy as np
import pytest

import jpegdec_amd as J
from tests import orient_util as U
from tests import rect_cases as R
from tests.cases import coef_jpeg_for

GUARD = 0x33
MODE = {"gray": 0, "c444": 1, "c420": 2, "c422": 3, "c440": 4}              # JDA_MODE_*


@pytest.fixture(scope="module")
def sim(hostsim):
    hostsim.hostsim_set_rect.argtypes = [C.c_int] * 5
    hostsim.hostsim_set_rect.restype = None
    return hostsim


def rect_decode(sim, oracle, key, jpeg, pt, opt, rect, mx, my, nok=None):
    """one emulated decode of `rect` into a guard-filled canvas -> (rc, got, expected)"""
    want = R.oracle_canvas(oracle, key, jpeg, pt, opt, must_succeed=nok is None)
    got = np.full_like(want, GUARD)
    inf, cx, cy, mw, mh, bpp, sh = oracle.canvas_geometry(jpeg, pt, opt)
    assert (cx, cy) == (mx, my)
    sim.hostsim_set_rect(1, *rect)
    try:
        rc = sim.hostsim_decode(jpeg, len(jpeg), pt, opt, got.ctypes.data_as(C.c_void_p), got.shape[1], cx * mw, cy * mh)
    finally:
        sim.hostsim_set_rect(0, 0, 0, 0, 0)
    return rc, got, R.expected_surface(want, rect, R.geometry_of(want, mx, my), nok, GUARD)


def run_matrix(sim, oracle, short, dri, modes=None, after=None):
    """every mode x every rectangle of one image; -> the number of decodes"""
    jpeg = R.rect_jpeg(short, dri)
    mx, my = R.LAYOUTS[short][3:5]
    n = 0
    for pt, opt in (modes or R.modes_of(short)):
        for rect in R.rects_of(short) + R.odd_rects_of(short):
            rc, got, exp = rect_decode(sim, oracle, (short, dri), jpeg, pt, opt, rect, mx, my)
            assert rc == 0, (short, dri, pt, opt, rect, rc)
            assert np.array_equal(got, exp), (short, dri, pt, opt, rect, int(np.count_nonzero(got != exp)))
            if after:
                after()
            n += 1
    return n


def test_images_are_what_the_matrix_assumes(sim):
    """the sizes give the MCU counts and tile sizes the rectangles are written for: two whole tiles and a short one per MCU row, a
    partial last MCU column and row, three MCU rows; every rectangle of the list is distinct"""
    for short, (sampling, w, h, mx, my, per, mw, mh) in R.LAYOUTS.items():
        for dri in (False, True):
            p = J.PreparedImage(R.rect_jpeg(short, dri))
            try:
                assert (p.info.mcus_x, p.info.mcus_y, p.info.mcu_w, p.info.mcu_h) == (mx, my, mw, mh), (short, dri)
                assert p.info.restart_interval == (R.RESTART_BLOCKS if dri else 0), (short, dri)
            finally:
                p.close()
        out = (C.c_uint32 * 4)()
        assert sim.hostsim_lds_layout(MODE[short], 0, out) == 0 and out[0] == per, (short, tuple(out))
        assert 2 * per < mx < 3 * per and w % mw and h % mh and my == 3
        rects = R.rects_of(short)
        assert len(set(rects)) == len(rects) >= 10
    assert R.tile_count((3, 1, 25, 3), 25, 3, 10) == 6 and R.tile_count((2, 1, 2, 2), 25, 3, 10) == 0 and R.whole_tiles(25, 3, 10) == 9
    assert R.clamp_rect((-3, -2, 40, 2), 25, 3) == (0, 0, 25, 2) and R.clamp_rect((0, 0, -1, -1), 25, 3) == (0, 0, 0, 0)


@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_rectangles_equal_the_oracle_and_keep_the_guard(short, dri, sim, oracle):
    assert run_matrix(sim, oracle, short, dri) >= 8 * 18


@pytest.mark.parametrize("short,dri", [(s, d) for s, d in R.IMAGES if s in ("c420", "c444")])
def test_rectangles_with_p1_in_chunks(short, dri, sim, oracle):
    """continuation entries on every image (JDA_PREPARE_CONT_ALWAYS), full size: a tile that starts at any block finds its own entries"""
    sim.hostsim_set_chunked(1)
    sim.hostsim_chunk_items()
    try:
        run_matrix(sim, oracle, short, dri, modes=[m for m in R.modes_of(short) if m[1] == 0])
        assert sim.hostsim_chunk_items() > 0
    finally:
        sim.hostsim_set_chunked(0)


@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_rectangles_with_a_small_window_in_reverse_order(short, dri, sim, oracle):
    """a 64-byte scan window (the bit reader's HBM fall-back) and the tiles run backwards"""
    sim.hostsim_set_window(64)
    sim.hostsim_set_reverse(1)
    try:
        run_matrix(sim, oracle, short, dri)
    finally:
        sim.hostsim_set_reverse(0)
        sim.hostsim_set_window(1024)


@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_rectangles_over_the_device_prescan_index(short, dri, sim, oracle):
    """the index the segment walk makes (canonical reader phases), alone and with the small window and the reverse order"""
    def used():
        assert sim.hostsim_prescan_used() == 2 and sim.hostsim_index_equal() == 1, (short, dri)
    sim.hostsim_set_device_prescan(1)
    try:
        run_matrix(sim, oracle, short, dri, after=used)
        sim.hostsim_set_window(64)
        sim.hostsim_set_reverse(1)
        run_matrix(sim, oracle, short, dri, modes=R.modes_of(short)[1:4], after=used)
    finally:
        sim.hostsim_set_reverse(0)
        sim.hostsim_set_window(1024)
        sim.hostsim_set_device_prescan(0)


def bad_mcu_rects(mx, my, nok):
    """rectangles in front of, around and behind the bad MCU (scan index nok) of an image of mx x my MCUs"""
    by, bx = divmod(nok, mx)
    assert 2 <= by < my - 3 and 2 <= bx < mx - 2, (by, bx)
    return [(0, 0, mx, by), (2, 1, bx + 5, by),                                   # in front: complete
            (bx - 3, by - 1, bx + 7, by + 2), (0, by, mx, by + 1), (bx, by, bx + 1, by + 1), (bx - 1, by, bx + 1, by + 1),   # around
            (bx + 1, by, mx, by + 1), (0, by + 2, mx, by + 5), (3, by + 1, bx, my)]         # behind: nothing is decodable


def test_rectangles_on_a_stream_with_a_bad_mcu(sim, oracle):
    """MCUs at scan index >= n_mcus_ok are not written, wherever the rectangle lies; the decode answers JDA_DECODE_ERROR"""
    jpeg, nok = U.bad_mcu_jpeg()
    info = J.parse(jpeg)
    mx, my = info["mcus_x"], info["mcus_y"]
    for pt, opt in R.MODES:
        for rect in bad_mcu_rects(mx, my, nok):
            rc, got, exp = rect_decode(sim, oracle, "bad_mcu", jpeg, pt, opt, rect, mx, my, nok)
            assert rc == 2, (pt, opt, rect, rc)
            assert np.array_equal(got, exp), (pt, opt, rect, int(np.count_nonzero(got != exp)))
    want = R.oracle_canvas(oracle, "bad_mcu", jpeg, J.RGB8888, 0, must_succeed=False)
    g = R.geometry_of(want, mx, my)
    by, bx = divmod(nok, mx)
    assert (R.expected_surface(want, (0, by, mx, by + 1), g, nok, GUARD)[by * g[3]:(by + 1) * g[3], bx * g[2]:] == GUARD).all()
    assert (R.expected_surface(want, (0, 0, mx, my), g, nok, GUARD)[(by + 1) * g[3]:] == GUARD).all()


def window_rects(mx, my, per):
    """rectangles shifted by half a tile against the whole image's tiling (on which the image was routed to its layout)"""
    h = per // 2
    return [(h, 0, mx, my), (h, 1, h + 2 * per, 4), (per + h, 2, mx, my - 1), (h, my - 2, h + per, my)]


@pytest.mark.parametrize("short", R.SHORTS)
def test_rectangles_on_the_window_stress_streams(short, sim, oracle):
    """one k_window_*_small_tight and one k_window_*_large file per layout at both layouts' real window sizes: a shifted tile's scan
    slice is not the slice the stream was built around, and may be over the window of the layout the whole image's count chose"""
    per = R.LAYOUTS[short][5]
    plain = J.GRAY8 if short == "gray" else J.RGB8888
    try:
        for kind in ("small_tight", "large"):
            name = "k_window_%s_%s" % (short, kind)
            jpeg = coef_jpeg_for(name)
            info = J.parse(jpeg)
            mx, my = info["mcus_x"], info["mcus_y"]
            for big in (0, 1):
                out = (C.c_uint32 * 4)()
                assert sim.hostsim_lds_layout(MODE[short], big, out) == 0
                sim.hostsim_set_window(out[2])
                for pt, opt in ((plain, 0), (J.RGB565_BE, J.SCALE_HALF), (J.GRAY8, J.SCALE_QUARTER)):
                    for rect in window_rects(mx, my, per):
                        rc, got, exp = rect_decode(sim, oracle, name, jpeg, pt, opt, rect, mx, my)
                        assert rc == 0 and np.array_equal(got, exp), (name, big, pt, opt, rect, int(np.count_nonzero(got != exp)))
    finally:
        sim.hostsim_set_window(1024)
