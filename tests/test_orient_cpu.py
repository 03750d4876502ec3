"""JPEG_AUTO_ROTATE without a GPU.

* the table of include/jpegdec_amd.h three ways: the row-major twin (tests/hostsim/orient_twin.h) = the numpy expressions = Pillow's
  Image.transpose;
* the kernel's tile schedule, lane by lane through the kernel's own code (tests/hostsim/orient_sim.cpp over jda_device_core.h), against
  the twin: every orientation, pixel size and size of the grid, pitches wider than the rows, poison that must survive outside the
  visible rectangle; the simulator also holds every access to the kernel's promises (alignment, extents, store widths, every byte once)
  and counts LDS bank conflicts -- none;
* jda_oriented_geometry against jda_output_geometry, refusals included; files made by with_orientation parse to what was written;
* JPEGDEC::decode with JPEG_AUTO_ROTATE through the class's CPU build (tests/class_cpu): draw sequence, bytes, refusals, and that
  nothing changes where the bit or the orientation says "as it is"."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import orient_util as U
from tests.cases import jpeg_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_CPU = os.path.join(ROOT, "tests", "class_cpu", "libjpegdec_class_cpu.so")
POISON = 0xA5
RGB565_LE, RGB565_BE, RGB8888, GRAY8 = 0, 1, 2, 3
LUMA_ONLY, EXIF_THUMBNAIL, USES_DMA = 64, 32, 128
INVALID, DECODE_ERROR, UNSUPPORTED = 1, 2, 3


@pytest.fixture(scope="module")
def sim(built_checkers):
    return C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_orientsim.so"))


@pytest.fixture(scope="module")
def class_cpu():
    import subprocess
    subprocess.run(["make", "classcpu"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return CLASS_CPU


def aligned(nbytes, fill):
    raw = np.empty(nbytes + 64, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + nbytes]
    a[:] = fill
    return a


def surfaces(rng, w, h, bpp, o, src_extra, dst_extra):
    """a random source of w x h pixels and a poisoned destination, pitches = the rows rounded up to 16 bytes + extra"""
    sp = ((w * bpp + 15) & ~15) + src_extra
    dw, dh = (h, w) if 5 <= o <= 8 else (w, h)
    dp = ((dw * bpp + 15) & ~15) + dst_extra
    src = aligned(sp * h, 0)
    src[:] = rng.randint(0, 256, sp * h)
    return src.reshape(h, sp), aligned(dp * dh, POISON).reshape(dh, dp), dw, dh


def p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("bpp", [1, 2, 4])
@pytest.mark.parametrize("o", U.ORIENTATIONS)
def test_row_major_twin_equals_numpy_and_pillow(o, bpp, sim):
    try:
        from PIL import Image                           # (held against Pillow where Pillow imports)
    except ImportError:
        Image = None
    rng = np.random.RandomState(100 * o + bpp)
    for w, h in ((1, 1), (2, 3), (17, 5), (64, 64), (130, 65), (333, 17)):
        src, dst, dw, dh = surfaces(rng, w, h, bpp, o, 16, 32)
        assert sim.orientsim_rowmajor(p(src), src.shape[1], w, h, bpp, o, p(dst), dst.shape[1]) == 0
        want = U.oriented(src, w, bpp, o)
        assert want.shape == (dh, dw * bpp)
        assert np.array_equal(dst[:, :dw * bpp], want) and np.all(dst[:, dw * bpp:] == POISON), (w, h)
        if Image is None:
            continue
        # Pillow on the same pixels: 1 byte = "L", 2 = "LA", 4 = "RGBA"
        img = Image.fromarray(np.ascontiguousarray(src[:, :w * bpp]).reshape((h, w) if bpp == 1 else (h, w, bpp)), {1: "L", 2: "LA", 4: "RGBA"}[bpp])
        if o in U.PILLOW:
            img = img.transpose(U.PILLOW[o])
        assert np.array_equal(np.asarray(img).reshape(dh, dw * bpp), want), (w, h)


@pytest.mark.parametrize("bpp", [1, 2, 4])
@pytest.mark.parametrize("o", U.ORIENTATIONS)
def test_lane_schedule_equals_row_major_twin(o, bpp, sim):
    rng = np.random.RandomState(7 * o + bpp)
    for w in U.SIZES:
        for h in U.SIZES:
            for src_extra, dst_extra in ((0, 0), (48, 0), (0, 32)):      # rows that fill the pitch, a wider source pitch, a wider destination pitch
                src, dst, dw, dh = surfaces(rng, w, h, bpp, o, src_extra, dst_extra)
                twin = dst.copy()
                conflicts = C.c_long(-1)
                rc = sim.orientsim_lanes(p(src), src.shape[1], w, h, bpp, o, p(dst), dst.shape[1], C.byref(conflicts))
                assert rc == 0, "the schedule broke a promise (%d) at %dx%d, pitches +%d +%d" % (rc, w, h, src_extra, dst_extra)
                assert conflicts.value == 0, "LDS bank conflicts at %dx%d: %d extra cycles" % (w, h, conflicts.value)
                assert sim.orientsim_rowmajor(p(src), src.shape[1], w, h, bpp, o, p(twin), twin.shape[1]) == 0
                assert np.array_equal(dst, twin), "differs from the row-major twin at %dx%d, pitches +%d +%d" % (w, h, src_extra, dst_extra)
                assert np.all(dst[:, dw * bpp:] == POISON), "wrote behind the visible row at %dx%d" % (w, h)


GEO_FILES = ("gray_333x217", "c444_333x217", "c420_333x217", "c422_333x217", "c440_200x120", "c420_1280x720", "pgray_100x100", "p420_200x120")


@pytest.mark.parametrize("name", GEO_FILES)
def test_oriented_geometry_against_output_geometry(name):
    import jpegdec_amd as J
    from jpegdec_amd.binding import ImageInfo
    lib = J.load_library()
    plain = jpeg_for(name)
    for file_o in (0, 6):
        jpeg = U.with_orientation(plain, file_o) if file_o else plain
        info = ImageInfo()
        assert lib.jda_parse(jpeg, len(jpeg), C.byref(info)) == 0 and info.orientation == file_o
        for pt in (RGB565_LE, RGB565_BE, RGB8888, GRAY8, 4, 5, 6, 7, -1):
            for opt in (0, 2, 4, 8, LUMA_ONLY, LUMA_ONLY | 2, 2 | 4, 4 | 8, 2 | 8):
                vals = [C.c_int32(0) for _ in range(5)]
                want_rc = lib.jda_output_geometry(C.byref(info), pt, opt, *[C.byref(v) for v in vals])
                for o in (None,) + U.ORIENTATIONS:
                    if want_rc != 0:                  # the same refusals, with the same codes
                        with pytest.raises(J.JdaError) as e:
                            J.oriented_geometry(info, pt, opt, o)
                        assert e.value.code == want_rc, (pt, opt, o)
                        continue
                    bpp, ow, oh = vals[0].value, vals[1].value, vals[2].value
                    eff = file_o if o is None else o
                    shift = 3 if info.jpeg_type == 1 and not (opt & 2) else 1 if opt & 2 else 2 if opt & 4 else 3 if opt & 8 else 0
                    g = J.oriented_geometry(info, pt, opt, o)
                    turned = 5 <= eff <= 8
                    assert g == {"bpp": bpp, "w": oh if turned else ow, "h": ow if turned else oh,
                                 "strip_rows": max(1, (info.mcu_w if turned else info.mcu_h) >> shift)}, (pt, opt, o)
    assert lib.jda_oriented_geometry(None, RGB8888, 0, 0, None, None, None, None) == INVALID


@pytest.mark.parametrize("big_endian", [False, True])
def test_with_orientation_files_parse_to_what_was_written(big_endian):
    import jpegdec_amd as J
    for name in ("gray_333x217", "c420_333x217", "p420_200x120"):
        plain = jpeg_for(name)
        base = J.parse(plain)
        assert base["status"] == 0 and base["orientation"] == 0
        for o in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 255):
            d = J.parse(U.with_orientation(plain, o, big_endian))
            assert d["status"] == 0 and d["orientation"] == o
            moved = ("orientation", "scan_offset")      # (the APP1 is 36 bytes in front of everything else)
            assert {k: v for k, v in d.items() if k not in moved} == {k: v for k, v in base.items() if k not in moved}
            assert d["scan_offset"] == base["scan_offset"] + 36


def expected(oracle, jpeg, pt, opt, o):
    """(oriented visible pixels, geometry) from the oracle's canvas of the unrotated decode"""
    import jpegdec_amd as J
    from jpegdec_amd.binding import ImageInfo
    info = ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    g = J.output_geometry(info, pt, opt)
    rc, canvas, err = oracle.decode_canvas(jpeg, GRAY8 if (opt & LUMA_ONLY) and pt < GRAY8 else pt, opt)
    assert rc == 1, err
    g.update(J.oriented_geometry(info, pt, opt, o))
    return U.oriented(canvas[:g["out_h"]], g["out_w"], g["bpp"], o), g


def check_both_modes(lib_path, oracle, jpeg, pt, opt, o, xy=(0, 0)):
    want, g = expected(oracle, jpeg, pt, opt, o)
    r = U.class_decode(lib_path, jpeg, pt, opt | U.AUTO_ROTATE, g["bpp"], xy=xy)
    assert (r["rc"], r["err"]) == (1, 0)
    ibpp = 32 if pt == RGB8888 and not (opt & LUMA_ONLY) else 8 if pt == GRAY8 or (opt & LUMA_ONLY) else 16
    strip = g["strip_rows"]
    assert r["log"] == [(xy[0], xy[1] + y, g["w"], min(strip, g["h"] - y), g["w"], ibpp) for y in range(0, g["h"], strip)]
    assert r["strips"] == U.strips_of(want, strip), "callback mode: bytes differ"
    assert r["getters"][2] == o
    fb = np.full(want.size + 64, POISON, np.uint8)
    r = U.class_decode(lib_path, jpeg, pt, opt | U.AUTO_ROTATE, g["bpp"], framebuffer=fb)
    assert (r["rc"], r["err"], r["log"]) == (1, 0, [])
    assert np.array_equal(fb[:want.size].reshape(want.shape), want), "framebuffer mode: bytes differ"
    assert np.all(fb[want.size:] == POISON), "framebuffer mode: wrote behind H' rows of W' * bpp bytes"
    return g


@pytest.mark.parametrize("o", range(2, 9))
@pytest.mark.parametrize("name", ["gray_333x217", "c420_333x217", "c422_333x217"])
def test_class_cpu_build_both_modes(name, o, class_cpu, oracle):
    plain = jpeg_for(name)
    for pt in (RGB565_LE, RGB565_BE, RGB8888, GRAY8):
        for opt in (0, 4):
            g = check_both_modes(class_cpu, oracle, U.with_orientation(plain, o, big_endian=bool(o & 1)), pt, opt, o)
            assert (g["w"], g["h"]) == ((g["out_h"], g["out_w"]) if o >= 5 else (g["out_w"], g["out_h"]))


def test_class_cpu_build_offsets_early_stop_and_options_that_do_not_matter(class_cpu, oracle):
    jpeg = U.with_orientation(jpeg_for("c420_333x217"), 6)
    check_both_modes(class_cpu, oracle, jpeg, RGB8888, 0, 6, xy=(3, 5))
    check_both_modes(class_cpu, oracle, jpeg, RGB565_LE, 2, 6, xy=(-7, 100))
    check_both_modes(class_cpu, oracle, jpeg, RGB8888, LUMA_ONLY, 6)
    check_both_modes(class_cpu, oracle, jpeg, RGB565_BE, 8 | USES_DMA, 6)      # JPEG_USES_DMA changes nothing
    want, g = expected(oracle, jpeg, RGB8888, 0, 6)
    # a callback that returns 0 ends the decode as it ends the unrotated one: the strips so far, return value 1, no error
    plain_stop = U.class_decode(class_cpu, jpeg_for("c420_333x217"), RGB8888, 0, 4, stop_after=2)
    r = U.class_decode(class_cpu, jpeg, RGB8888, U.AUTO_ROTATE, 4, stop_after=2)
    assert (r["rc"], r["err"]) == (plain_stop["rc"], plain_stop["err"]) == (1, 0)
    assert len(r["log"]) == 2 and r["strips"] == U.strips_of(want, g["strip_rows"])[:2]
    # setMaxOutputSize does not split the strips
    r = U.class_decode(class_cpu, jpeg, RGB8888, U.AUTO_ROTATE, 4, max_mcus=1)
    assert (r["rc"], r["err"]) == (1, 0) and r["strips"] == U.strips_of(want, g["strip_rows"])
    # a progressive file is its 1/8 thumbnail, turned
    check_both_modes(class_cpu, oracle, U.with_orientation(jpeg_for("p420_200x120"), 8, True), RGB565_LE, 0, 8)
    check_both_modes(class_cpu, oracle, U.with_orientation(jpeg_for("pgray_100x100"), 5), GRAY8, 2, 5)


def test_class_cpu_build_exif_thumbnail_takes_its_own_or_the_main_images_orientation(class_cpu, oracle):
    from tests.exif_util import with_exif_thumbnail
    main, thumb = jpeg_for("c444_256x256_q100_opt"), jpeg_for("c422_333x217")
    for thumb_o, main_o, eff in ((None, 6, 6), (3, 6, 3), (None, 1, 1)):
        t = thumb if thumb_o is None else U.with_orientation(thumb, thumb_o)
        jpeg = with_exif_thumbnail(main, t, 333, 217, orientation=main_o)
        want, g = expected(oracle, t, RGB8888, 0, eff)
        r = U.class_decode(class_cpu, jpeg, RGB8888, EXIF_THUMBNAIL | U.AUTO_ROTATE, 4)
        assert (r["rc"], r["err"]) == (1, 0)
        if eff == 1:                                    # nothing to turn: the unrotated thumbnail decode, call for call
            same = U.class_decode(class_cpu, jpeg, RGB8888, EXIF_THUMBNAIL, 4)
            assert (r["log"], r["strips"]) == (same["log"], same["strips"])
            continue
        assert b"".join(r["strips"]) == want.tobytes() and r["log"][0][2] == g["w"] == (217 if eff >= 5 else 333)
        assert r["getters"][:2] == (333, 217)           # the object describes the thumbnail now; width and height stay the file's


def test_class_cpu_build_refusals(class_cpu, oracle):
    jpeg = U.with_orientation(jpeg_for("c420_333x217"), 6)
    for fb in (None, np.zeros(333 * 217 * 4, np.uint8)):
        r = U.class_decode(class_cpu, jpeg, RGB8888, U.AUTO_ROTATE, 4, crop=(16, 16, 64, 64), framebuffer=fb)
        assert (r["rc"], r["err"], r["log"]) == (0, UNSUPPORTED, [])
        r = U.class_decode(class_cpu, jpeg, 6, U.AUTO_ROTATE, 4, framebuffer=fb)                       # a dithered pixel type: as without the bit
        assert (r["rc"], r["err"], r["log"]) == (0, UNSUPPORTED, [])
        r = U.class_decode(class_cpu, jpeg, RGB8888, U.AUTO_ROTATE | 2 | 4, 4, framebuffer=fb)         # two scale bits: as without the bit
        assert (r["rc"], r["err"], r["log"]) == (0, UNSUPPORTED, [])
        prog = U.with_orientation(jpeg_for("p420_200x120"), 6)
        r = U.class_decode(class_cpu, prog, GRAY8, U.AUTO_ROTATE, 1, framebuffer=fb)                    # colour progressive to gray: as without the bit
        assert (r["rc"], r["err"], r["log"]) == (0, UNSUPPORTED, [])
        r = U.class_decode(class_cpu, prog, RGB8888, U.AUTO_ROTATE | 4, 4, framebuffer=fb)              # 1/4 of a progressive file
        assert (r["rc"], r["err"], r["log"]) == (0, UNSUPPORTED, [])
    # the whole image as a crop rectangle is no crop (where the reference's MCU rounding leaves it the whole image)
    r = U.class_decode(class_cpu, U.with_orientation(jpeg_for("c420_1280x720"), 6), GRAY8, U.AUTO_ROTATE | 8, 1, crop=(0, 0, 1280, 720))
    assert (r["rc"], r["err"], len(r["log"])) == (1, 0, 80)


def test_class_cpu_build_bad_mcu_delivers_everything_then_fails(class_cpu, oracle):
    import jpegdec_amd as J
    plain, nok = U.bad_mcu_jpeg()
    info = J.parse(plain)
    rc, canvas, err = oracle.decode_canvas(plain, RGB565_LE, 0)      # (the MCUs in front of the bad one are there whatever it returns)
    want = U.oriented(U.zero_undecoded(canvas, info, nok)[:217], 333, 2, 6)
    assert want.any() and not want[:, :16 * 2].any()                 # the undecoded bottom of the image is the left edge now
    jpeg = U.with_orientation(plain, 6)
    r = U.class_decode(class_cpu, jpeg, RGB565_LE, U.AUTO_ROTATE, 2)
    assert (r["rc"], r["err"]) == (0, DECODE_ERROR)
    assert b"".join(r["strips"]) == want.tobytes() and len(r["log"]) == 21
    fb = np.full(want.size, POISON, np.uint8)
    r = U.class_decode(class_cpu, jpeg, RGB565_LE, U.AUTO_ROTATE, 2, framebuffer=fb)
    assert (r["rc"], r["err"]) == (0, DECODE_ERROR) and np.array_equal(fb.reshape(want.shape), want)


@pytest.mark.parametrize("name", ["gray_333x217", "c420_333x217", "c422_333x217"])
def test_class_cpu_build_nothing_changes_where_nothing_is_to_turn(name, class_cpu):
    """bit set on orientation 0, 1, 9; bit clear on orientation 6: today's output, call for call and byte for byte -- in both modes, with
    a crop, an offset and a strip limit"""
    import jpegdec_amd as J
    from jpegdec_amd.binding import ImageInfo
    plain = jpeg_for(name)
    for pt, opt, kw in ((RGB8888, 0, {}), (RGB565_LE, 2, dict(xy=(5, 9))), (GRAY8, 4, dict(max_mcus=3)), (RGB565_BE, 0, dict(crop=(16, 16, 64, 64))),
                        (RGB8888, USES_DMA, {}), (RGB565_LE, 8, dict(stop_after=2))):
        info = ImageInfo()
        assert J.load_library().jda_parse(plain, len(plain), C.byref(info)) == 0
        px = J.output_geometry(info, pt, opt)["bpp"]
        today = U.class_decode(class_cpu, plain, pt, opt, px, **kw)
        fb_today = np.full(400 * 240 * 4, POISON, np.uint8)
        U.class_decode(class_cpu, plain, pt, opt, px, framebuffer=fb_today, **kw)
        for o, bit in ((0, 1), (1, 1), (9, 1), (255, 1), (6, 0), (3, 0)):
            jpeg = U.with_orientation(plain, o) if o else plain
            r = U.class_decode(class_cpu, jpeg, pt, opt | bit, px, **kw)
            assert (r["rc"], r["err"], r["log"], r["strips"]) == (today["rc"], today["err"], today["log"], today["strips"]), (pt, opt, o, bit)
            fb = np.full(400 * 240 * 4, POISON, np.uint8)
            r = U.class_decode(class_cpu, jpeg, pt, opt | bit, px, framebuffer=fb, **kw)
            assert r["rc"] == 1 and np.array_equal(fb, fb_today), (pt, opt, o, bit)


def test_constants_and_exports():
    import jpegdec_amd as J
    assert J.AUTO_ROTATE == 1
    for name in ("oriented_geometry", "orient_surfaces", "decode_oriented_to_host"):
        assert callable(getattr(J, name))
