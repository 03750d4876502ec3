"""The output clip without a GPU: the wave emulator (tests/hostsim) decodes every image and mode of tests/rect_cases.py under every clip
of tests/clip_cases.py into a guard-filled surface of either shape -- wide (the canvas's pitch and rows, and more) and tight (the
clipped row's pitch, one guard row) -- and the whole surface must be the guard except the oracle's bytes inside the clip
(clip_cases.expected_clipped).  Then the clip list with P1 in chunks and with a 64-byte scan window in reverse tile order, a clip
combined with an MCU rectangle, a clip on a stream with a bad MCU, and the coefficient stage's row-major twin, lane schedule and
sparse load phase under the full-size clip list."""
import ctypes as C
import os

import numpy as np
import pytest

import jpegdec_amd as J
from tests import clip_cases as K
from tests import orient_util as U
from tests import rect_cases as R

GUARD = 0x33
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim(hostsim):
    hostsim.hostsim_set_rect.argtypes = [C.c_int] * 5
    hostsim.hostsim_set_rect.restype = None
    return hostsim


@pytest.fixture(scope="module")
def coefsim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_coefsim.so"))
    lib.coefsim_decode.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def sparsesim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_coefsparsesim.so"))
    lib.coefsparsesim_run.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def clipped_decode(sim, want, jpeg, pt, opt, w, rows, shape, g, rect=None, nok=None, mcus=None):
    """one emulated decode under (w, rows) into a guard-filled surface of `shape` -> (rc, got, expected)"""
    pitch, surf_rows = K.surface_shape(shape, w, rows, g)
    got = np.full((surf_rows, pitch), GUARD, np.uint8)
    if rect is not None:
        sim.hostsim_set_rect(1, *rect)
    try:
        rc = K.hostsim_decode(sim, jpeg, pt, opt, got, w, rows)
    finally:
        if rect is not None:
            sim.hostsim_set_rect(0, 0, 0, 0, 0)
    return rc, got, K.expected_clipped(want, w, rows, g["bpp"], pitch, surf_rows, rect, nok, GUARD, mcus)


def run_clips(sim, oracle, short, dri, modes=None):
    """every mode x every clip x both shapes of one image; -> the number of decodes"""
    jpeg = R.rect_jpeg(short, dri)
    n = 0
    for pt, opt in (modes or R.modes_of(short)):
        want = R.oracle_canvas(oracle, (short, dri), jpeg, pt, opt)
        g = K.geometry(short, pt, opt)
        assert want.shape == (g["ch"], g["cw"] * g["bpp"])
        for w, rows in K.clips_of(short, pt, opt):
            for shape in K.SHAPES:
                rc, got, exp = clipped_decode(sim, want, jpeg, pt, opt, w, rows, shape, g)
                assert rc == 0, (short, dri, pt, opt, (w, rows), shape, rc)
                assert np.array_equal(got, exp), (short, dri, pt, opt, (w, rows), shape, int(np.count_nonzero(got != exp)))
                n += 1
    return n


def test_the_clip_lists_are_what_the_matrix_assumes(product_lib):
    """per (layout, mode): about 30 distinct clips; one cuts a tile on the right, one at the bottom, one at an odd row, one inside a 4-pixel
    store group; one writes nothing and one clamps to the canvas; the visible size is the image's size at the scale, rounded up"""
    total = 0
    for short, (sampling, w, h, mx, my, per, mw, mh) in R.LAYOUTS.items():
        for pt, opt in R.modes_of(short):
            g = K.geometry(short, pt, opt)
            s = g["s"]
            assert (g["vw"], g["vh"]) == ((w + (1 << s) - 1) >> s, (h + (1 << s) - 1) >> s) and g["vw"] <= g["cw"] and g["vh"] <= g["ch"], (short, pt, opt, g)
            assert (g["tw"], g["cw"], g["ch"]) == (per * (mw >> s), mx * (mw >> s), my * (mh >> s))
            assert K.visible_size(R.rect_jpeg(short, True), pt, opt) == (g["vw"], g["vh"])
            clips = K.clips_of(short, pt, opt)
            assert len(set(clips)) == len(clips) and 20 <= len(clips) <= 36, (short, pt, opt, len(clips))
            assert {c[0] for c in clips} >= set(K.widths_of(g)) and {c[1] for c in clips} >= set(K.rows_of(g))
            assert all(c in clips for c in ((0, g["ch"]), (g["cw"], 0), (g["vw"], g["vh"]), ))
            c = K.cuts(clips, g)
            assert all(c.values()), (short, pt, opt, c)
            c = K.cuts(K.rect_clips(g), g)
            assert c["right"] and c["bottom"], (short, pt, opt, c)
            total += 2 * len(clips)
    assert 2 * total >= 4500, total                        # both restart flavours of every layout
    # the two shapes: a wide surface holds the whole canvas and more, a tight one only the clipped rows at the clipped row's pitch
    g = K.geometry("c420", J.RGB8888, 0)
    assert K.surface_shape("wide", 5, 3, g) == (400 * 4 + 32, 48 + 2) and K.surface_shape("tight", 5, 3, g) == (32, 4)
    assert K.surface_shape("tight", 0, 0, g) == (16, 1) and K.surface_shape("tight", 409, 57, g) == (1600, 49)
    want = np.arange(48 * 1600, dtype=np.uint32).astype(np.uint8).reshape(48, 1600)
    e = K.expected_clipped(want, 5, 3, 4, 32, 4, guard=GUARD)
    assert np.array_equal(e[:3, :20], want[:3, :20]) and (e[3:] == GUARD).all() and (e[:, 20:] == GUARD).all()
    assert (K.expected_clipped(want, 0, 48, 4, 16, 49, guard=GUARD) == GUARD).all() and (K.expected_clipped(want, 400, 0, 4, 1600, 1, guard=GUARD) == GUARD).all()


@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_clips_equal_the_oracle_and_keep_the_guard(short, dri, sim, oracle):
    assert run_clips(sim, oracle, short, dri) >= 8 * 2 * 20


@pytest.mark.parametrize("short,dri", [(s, d) for s, d in R.IMAGES if s in ("c420", "c444")])
def test_clips_with_p1_in_chunks(short, dri, sim, oracle):
    """continuation entries on every image (JDA_PREPARE_CONT_ALWAYS), full size"""
    sim.hostsim_set_chunked(1)
    sim.hostsim_chunk_items()
    try:
        run_clips(sim, oracle, short, dri, modes=[m for m in R.modes_of(short) if m[1] == 0])
        assert sim.hostsim_chunk_items() > 0
    finally:
        sim.hostsim_set_chunked(0)


@pytest.mark.parametrize("short,dri", [(s, d) for s, d in R.IMAGES if s in ("c420", "c444")])
def test_clips_with_a_small_window_in_reverse_order(short, dri, sim, oracle):
    """a 64-byte scan window (the bit reader's HBM fall-back) and the tiles run backwards, full size"""
    sim.hostsim_set_window(64)
    sim.hostsim_set_reverse(1)
    try:
        run_clips(sim, oracle, short, dri, modes=[m for m in R.modes_of(short) if m[1] == 0])
    finally:
        sim.hostsim_set_reverse(0)
        sim.hostsim_set_window(1024)


@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_clips_with_rectangles(short, dri, sim, oracle):
    """a clip and an MCU rectangle together: what is written is the rectangle's MCUs inside the clip"""
    jpeg = R.rect_jpeg(short, dri)
    mx, my = R.LAYOUTS[short][3:5]
    for pt, opt in R.modes_of(short):
        want = R.oracle_canvas(oracle, (short, dri), jpeg, pt, opt)
        g = K.geometry(short, pt, opt)
        for rect in K.clip_rects(short):
            for w, rows in K.rect_clips(g):
                for shape in K.SHAPES:
                    rc, got, exp = clipped_decode(sim, want, jpeg, pt, opt, w, rows, shape, g, rect, None, (mx, my))
                    assert rc == 0, (short, dri, pt, opt, rect, (w, rows), shape, rc)
                    assert np.array_equal(got, exp), (short, dri, pt, opt, rect, (w, rows), shape, int(np.count_nonzero(got != exp)))
                    assert (exp != GUARD).any()


def test_clips_on_a_stream_with_a_bad_mcu(sim, oracle):
    """the status stays JDA_DECODE_ERROR; MCUs in front of the bad one are written inside the clip, nothing else is"""
    jpeg, nok = U.bad_mcu_jpeg()
    for pt, opt in R.MODES:
        want = R.oracle_canvas(oracle, "bad_mcu", jpeg, pt, opt, must_succeed=False)
        g = K.file_geometry(jpeg, pt, opt)
        assert g["my"] * g["mho"] == want.shape[0] and nok // g["mx"] >= 2
        for w, rows in K.rect_clips(g):
            for shape in K.SHAPES:
                rc, got, exp = clipped_decode(sim, want, jpeg, pt, opt, w, rows, shape, g, None, nok, (g["mx"], g["my"]))
                assert rc == 2, (pt, opt, (w, rows), shape, rc)
                assert np.array_equal(got, exp), (pt, opt, (w, rows), shape, int(np.count_nonzero(got != exp)))


COEF_MODES = ((J.RGB8888, 0), (J.RGB565_LE, 0), (J.RGB565_BE, 0), (J.GRAY8, 0))


@pytest.mark.parametrize("short", R.SHORTS)
def test_coefficient_stage_under_the_clips(short, product_lib, coefsim, sparsesim, oracle):
    """the image's own coefficients (as the reference's reader stores them) through jda_coef_image_from_coefficients: the row-major twin,
    the lane schedule of jda_coef_tiles and -- behind the sparse load phase -- that of jda_sparse_tiles, each under the full-size clip list"""
    jpeg = R.rect_jpeg(short)
    n, coefs, _, _, _ = oracle.entropy(jpeg)
    coefs = np.ascontiguousarray(coefs)
    for pt, opt in COEF_MODES:
        if short == "gray" and pt == J.RGB8888:
            continue
        want = R.oracle_canvas(oracle, (short, False), jpeg, pt, opt)
        g = K.geometry(short, pt, opt)
        for w, rows in K.clips_of(short, pt, opt):
            for shape in K.SHAPES:
                pitch, surf_rows = K.surface_shape(shape, w, rows, g)
                exp = K.expected_clipped(want, w, rows, g["bpp"], pitch, surf_rows, guard=GUARD)
                for which in ("twin", "lanes", "sparse"):
                    got = np.full((surf_rows, pitch), GUARD, np.uint8)
                    assert got.ctypes.data % 16 == 0
                    if which == "sparse":
                        rc = sparsesim.coefsparsesim_run(jpeg, len(jpeg), coefs.ctypes.data, len(coefs), pt, opt, None, got.ctypes.data, pitch, w, rows, None)
                    else:
                        rc = coefsim.coefsim_decode(jpeg, len(jpeg), coefs.ctypes.data, len(coefs), pt, opt, 1 if which == "twin" else 0, got.ctypes.data, pitch, w, rows, None)
                    assert rc == 0, (short, pt, which, (w, rows), shape, rc)
                    assert np.array_equal(got, exp), (short, pt, which, (w, rows), shape, int(np.count_nonzero(got != exp)))
