"""JPEG_AUTO_ROTATE on the GPU: jda_orient_surfaces on random bytes against the numpy expressions of the table (every orientation,
pixel size and size, one launch a pixel size), jda_decode_to_host_oriented, the drop-in class and the C flavour against the oracle's
unrotated canvas turned by numpy, and a streamed pipeline batch turned where it lies in HBM."""
import ctypes as C

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.binding import ImageInfo
from tests import orient_util as U
from tests.cases import jpeg_for
from tests.test_orient_cpu import DECODE_ERROR, INVALID, POISON, check_both_modes, expected

pytestmark = pytest.mark.gpu

PIXEL_TYPES = (J.RGB565_LE, J.RGB565_BE, J.RGB8888, J.GRAY8)
SCALES = (0, J.SCALE_HALF, J.SCALE_QUARTER, J.SCALE_EIGHTH)


def orient_launches():
    return sum(v for k, v in J.kernel_launch_counts().items() if "jda_orient_tiles" in k)


@pytest.mark.parametrize("bpp", [1, 2, 4])
def test_orient_surfaces_every_size_and_orientation_in_one_launch(bpp, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.RandomState(40 + bpp)
    plan, s_off, d_off = [], 0, 0
    for w in U.SIZES:
        for h in U.SIZES:
            for o in U.ORIENTATIONS:
                for src_extra, dst_extra in ((0, 0), (48, 0), (0, 32)):
                    dw, dh = (h, w) if o >= 5 else (w, h)
                    sp, dp = ((w * bpp + 15) & ~15) + src_extra, ((dw * bpp + 15) & ~15) + dst_extra
                    plan.append((w, h, o, sp, dp, dw, dh, s_off, d_off))
                    s_off += (sp * h + 255) & ~255
                    d_off += (dp * dh + 255) & ~255
    host_src = rng.randint(0, 256, s_off).astype(np.uint8)
    dsrc, ddst = ctx.malloc(s_off), ctx.malloc(d_off)
    ctx.from_host(dsrc, host_src)
    ctx.memset(ddst, POISON, d_off)
    before = orient_launches()
    J.orient_surfaces(ctx, [(dsrc + so, sp, w, h) for (w, h, o, sp, dp, dw, dh, so, do) in plan], bpp, [q[2] for q in plan],
                      [(ddst + do, dp, dw, dh) for (w, h, o, sp, dp, dw, dh, so, do) in plan])
    assert orient_launches() == before + 1, "one launch for the whole batch"
    got = ctx.to_host(ddst, d_off)
    assert np.array_equal(ctx.to_host(dsrc, s_off), host_src), "the sources are left as they are"
    ctx.free(dsrc)
    ctx.free(ddst)
    prev_end = 0
    for (w, h, o, sp, dp, dw, dh, so, do) in plan:
        src = host_src[so:so + sp * h].reshape(h, sp)
        dst = got[do:do + dp * dh].reshape(dh, dp)
        assert np.array_equal(dst[:, :dw * bpp], U.oriented(src, w, bpp, o)), (w, h, o, sp, dp)
        assert np.all(dst[:, dw * bpp:] == POISON), ("wrote behind the visible row", w, h, o, sp, dp)
        assert np.all(got[prev_end:do] == POISON), ("wrote between the surfaces", w, h, o)
        prev_end = do + dp * dh
    assert np.all(got[prev_end:] == POISON)


def test_orient_surfaces_invalid_parameters(gpu_ctx):
    ctx = gpu_ctx
    lib = ctx.lib
    a, b = ctx.malloc(1 << 16), ctx.malloc(1 << 16)

    def call(src, dst, bpp=4, o=6, n=1):
        from jpegdec_amd.binding import Output
        s = (Output * 1)(Output(*src)) if src else None
        d = (Output * 1)(Output(*dst)) if dst else None
        return lib.jda_orient_surfaces(ctx.handle, n, s, bpp, (C.c_int32 * 1)(o), d)
    good_src, good_dst = (a, 64, 10, 20), (b, 80, 20, 10)
    before = orient_launches()
    assert call(good_src, good_dst) == 0
    assert orient_launches() == before + 1
    assert call(good_src, good_dst, n=0) == 0 and call(None, None, n=0) == 0 and orient_launches() == before + 1      # nothing to do, nothing launched
    for what, rc in (("orientation 9", call(good_src, good_dst, o=9)), ("orientation -1", call(good_src, good_dst, o=-1)),
                     ("pixel size 3", call(good_src, good_dst, bpp=3)), ("pixel size 8", call(good_src, good_dst, bpp=8)),
                     ("dst not turned", call(good_src, (b, 80, 10, 20))), ("dst turned for orientation 3", call(good_src, good_dst, o=3)),
                     ("dst too few rows", call(good_src, (b, 80, 20, 9))), ("null src", call((0, 64, 10, 20), good_dst)), ("null dst", call(good_src, (0, 80, 20, 10))),
                     ("null arrays", call(None, None)), ("n < 0", call(good_src, good_dst, n=-1)),
                     ("misaligned src", call((a + 4, 64, 10, 20), good_dst)), ("misaligned dst", call(good_src, (b + 8, 80, 20, 10))),
                     ("src pitch not a multiple of 16", call((a, 72, 10, 20), good_dst)), ("dst pitch not a multiple of 16", call(good_src, (b, 88, 20, 10))),
                     ("src pitch too small", call((a, 32, 10, 20), good_dst)), ("dst pitch too small", call(good_src, (b, 64, 20, 10))),
                     ("empty src", call((a, 64, 0, 20), (b, 80, 20, 0))),
                     ("dst is src", call(good_src, (a, 80, 20, 10))), ("dst begins inside src", call(good_src, (a + 64 * 19, 80, 20, 10))),
                     ("src begins inside dst", call((b + 80 * 9, 64, 10, 20), good_dst))):
        assert rc == INVALID, what
    assert orient_launches() == before + 1, "a refused call launches nothing"
    assert call(good_src, (a + 64 * 20, 80, 20, 10)) == 0            # side by side is fine
    ctx.free(a)
    ctx.free(b)


def check_one_call(ctx, oracle, jpeg, pt, opt, o, by_file=False):
    want, g = expected(oracle, jpeg, pt, opt, o)
    rc, got, gg = J.decode_oriented_to_host(ctx, U.with_orientation(jpeg, o, bool(o & 1)) if by_file else jpeg, pt, opt, None if by_file else o)
    assert rc == 0, (rc, pt, opt, o)
    assert (gg["w"], gg["h"], gg["strip_rows"], gg["bpp"]) == (g["w"], g["h"], g["strip_rows"], g["bpp"])
    assert got.shape == want.shape and np.array_equal(got, want), (pt, opt, o, int(np.count_nonzero(got != want)))


@pytest.mark.parametrize("name", ["gray_333x217", "c444_333x217", "c420_333x217", "c422_333x217", "c440_200x120", "c420_1280x720"])
def test_one_call_equals_the_oracle_turned_by_numpy(name, gpu_ctx, oracle):
    jpeg = jpeg_for(name)
    for pt in PIXEL_TYPES:
        for opt in SCALES:
            for o in range(2, 9):
                check_one_call(gpu_ctx, oracle, jpeg, pt, opt, o, by_file=(o + pt) % 2 == 0)
    for o in range(2, 9):
        check_one_call(gpu_ctx, oracle, jpeg, J.RGB565_LE, J.LUMA_ONLY, o)
    for o in (0, 1, 9, 255):                            # "as it is": the visible rectangle of the unrotated decode
        want, g = expected(oracle, jpeg, J.RGB8888, 0, o)
        rc, got, gg = J.decode_oriented_to_host(gpu_ctx, U.with_orientation(jpeg, o), J.RGB8888, 0)
        assert rc == 0 and gg["orientation"] == o and np.array_equal(got, want), o


def test_one_call_progressive_bad_mcu_pitch_and_refusals(gpu_ctx, oracle):
    ctx = gpu_ctx
    for name, pts in (("p420_200x120", (J.RGB565_LE, J.RGB565_BE, J.RGB8888)), ("pgray_100x100", PIXEL_TYPES)):
        for pt in pts:
            for opt in (0, J.SCALE_HALF, J.SCALE_EIGHTH):
                for o in range(2, 9):
                    check_one_call(ctx, oracle, jpeg_for(name), pt, opt, o)
    # a stream with a bad MCU: zeros from the bad MCU on BEFORE the turn, the whole oriented canvas delivered, JDA_DECODE_ERROR
    bad, nok = U.bad_mcu_jpeg()
    info = J.parse(bad)
    for pt, bpp in ((J.RGB8888, 4), (J.GRAY8, 1)):
        orc, canvas, err = oracle.decode_canvas(bad, pt, 0)
        for o in (3, 6, 8):
            rc, got, g = J.decode_oriented_to_host(ctx, bad, pt, 0, o)
            assert rc == DECODE_ERROR and g["mcus_decoded"] == nok
            assert np.array_equal(got, U.oriented(U.zero_undecoded(canvas, info, g["mcus_decoded"])[:217], 333, bpp, o)), (pt, o)
    # a host pitch wider than the rows, more rows than needed: only W' * bpp x H' bytes are written
    jpeg = jpeg_for("c422_333x217")
    want, g = expected(oracle, jpeg, J.RGB565_BE, 0, 5)
    for pitch in (g["w"] * 2, g["w"] * 2 + 2, 1024):
        host = np.full((g["h"] + 3, pitch), POISON, np.uint8)
        rc = ctx.lib.jda_decode_to_host_oriented(ctx.handle, jpeg, len(jpeg), J.RGB565_BE, 0, 5, host.ctypes.data_as(C.c_void_p), pitch, g["h"] + 3, None)
        assert rc == 0 and np.array_equal(host[:g["h"], :g["w"] * 2], want)
        assert np.all(host[g["h"]:] == POISON) and np.all(host[:, g["w"] * 2:] == POISON), pitch
    host = np.zeros((g["h"], 1024), np.uint8)
    hp = host.ctypes.data_as(C.c_void_p)
    call = ctx.lib.jda_decode_to_host_oriented
    assert call(ctx.handle, jpeg, len(jpeg), J.RGB565_BE, 0, 5, hp, g["w"] * 2 - 1, g["h"], None) == INVALID          # pitch too small
    assert call(ctx.handle, jpeg, len(jpeg), J.RGB565_BE, 0, 5, hp, 1024, g["h"] - 1, None) == INVALID                 # too few rows
    assert call(ctx.handle, jpeg, len(jpeg), J.RGB565_BE, 0, 9, hp, 1024, g["h"], None) == INVALID                     # no such orientation
    assert call(ctx.handle, jpeg, len(jpeg), J.RGB565_BE, 0, 5, None, 1024, g["h"], None) == INVALID
    for pt in (J.FOUR_BIT_DITHERED, J.TWO_BIT_DITHERED, J.ONE_BIT_DITHERED, 7, -1):                                      # dithered types are not turned
        assert call(ctx.handle, jpeg, len(jpeg), pt, 0, 5, hp, 1024, g["h"], None) == INVALID
    assert call(ctx.handle, jpeg, len(jpeg), J.RGB8888, 2 | 4, 5, hp, 1024, g["h"], None) == 3                           # as jda_output_geometry refuses it
    # the existing entries keep ignoring option bit 1
    turned = U.with_orientation(jpeg, 6)
    rc0, plain_canvas, _ = J.decode_to_host(ctx, jpeg, J.RGB8888, 0)
    rc1, bit_canvas, _ = J.decode_to_host(ctx, turned, J.RGB8888, J.AUTO_ROTATE)
    assert rc0 == rc1 == 0 and np.array_equal(plain_canvas, bit_canvas)


@pytest.mark.parametrize("o", range(2, 9))
def test_class_both_modes(o, gpu_ctx, oracle):
    for name, pt, opt in (("gray_333x217", J.RGB8888, 0), ("c420_333x217", J.RGB565_LE, J.SCALE_QUARTER), ("c422_333x217", J.GRAY8, 0),
                          ("c444_333x217", J.RGB565_BE, J.SCALE_HALF), ("c440_200x120", J.RGB8888, J.SCALE_EIGHTH), ("c420_1280x720", J.RGB8888, 0)):
        check_both_modes(J.library_path(), oracle, U.with_orientation(jpeg_for(name), o, bool(o & 1)), pt, opt, o, xy=(o, -o))


def test_class_bad_mcu_thumbnail_and_untouched_paths(gpu_ctx, oracle):
    from tests import test_orient_cpu as T
    T.test_class_cpu_build_bad_mcu_delivers_everything_then_fails(J.library_path(), oracle)
    T.test_class_cpu_build_exif_thumbnail_takes_its_own_or_the_main_images_orientation(J.library_path(), oracle)
    T.test_class_cpu_build_refusals(J.library_path(), oracle)
    plain = jpeg_for("c420_333x217")
    today = U.class_decode(J.library_path(), plain, J.RGB8888, 0, 4)
    for o, bit in ((1, 1), (0, 1), (9, 1), (6, 0)):
        r = U.class_decode(J.library_path(), U.with_orientation(plain, o) if o else plain, J.RGB8888, bit, 4)
        assert (r["rc"], r["err"], r["log"], r["strips"]) == (today["rc"], today["err"], today["log"], today["strips"]), (o, bit)


class JPEGIMAGE(C.Structure):
    _fields_ = [("magic", C.c_uint32 * 2), ("file_owner", C.c_void_p), ("file_data", C.c_void_p), ("file_check", C.c_uint64), ("state", C.c_uint64 * 40)]


@pytest.mark.parametrize("name,pt,opt,o", [("c420_333x217", J.RGB8888, 0, 6), ("gray_333x217", J.RGB565_BE, J.SCALE_HALF, 7), ("c422_333x217", J.GRAY8, 0, 2),
                                           ("c444_333x217", J.RGB565_LE, J.SCALE_QUARTER, 8)])
def test_c_flavour_JPEG_decode(name, pt, opt, o, gpu_ctx, oracle):
    lib = C.CDLL(J.library_path())
    jpeg = U.with_orientation(jpeg_for(name), o)
    want, g = expected(oracle, jpeg, pt, opt, o)
    lib.JPEG_openRAM.argtypes = [C.c_void_p, C.c_void_p, C.c_int, U.DRAW_CB]
    lib.JPEG_setPixelType.argtypes = [C.c_void_p, C.c_int]
    lib.JPEG_setFramebuffer.argtypes = [C.c_void_p, C.c_void_p]
    lib.JPEG_decode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.JPEG_getLastError.argtypes = lib.JPEG_getOrientation.argtypes = lib.JPEG_getWidth.argtypes = [C.c_void_p]
    log, strips = [], []

    def cb(p):
        d = p.contents
        log.append((d.x, d.y, d.iWidth, d.iHeight, d.iWidthUsed))
        strips.append(C.string_at(d.pPixels, d.iWidth * g["bpp"] * d.iHeight))
        return 1
    keep = U.DRAW_CB(cb)
    src = C.create_string_buffer(jpeg, len(jpeg) + 64)
    img = JPEGIMAGE()
    assert lib.JPEG_openRAM(C.byref(img), src, len(jpeg), keep) == 1 and lib.JPEG_getOrientation(C.byref(img)) == o
    lib.JPEG_setPixelType(C.byref(img), pt)
    assert lib.JPEG_decode(C.byref(img), 2, 3, opt | J.AUTO_ROTATE) == 1 and lib.JPEG_getLastError(C.byref(img)) == 0
    assert log == [(2, 3 + y, g["w"], min(g["strip_rows"], g["h"] - y), g["w"]) for y in range(0, g["h"], g["strip_rows"])]
    assert b"".join(strips) == want.tobytes()
    assert lib.JPEG_getWidth(C.byref(img)) == J.parse(jpeg)["width"]
    fb = np.full(want.size + 16, POISON, np.uint8)
    lib.JPEG_setFramebuffer(C.byref(img), fb.ctypes.data_as(C.c_void_p))
    assert lib.JPEG_decode(C.byref(img), 0, 0, opt | J.AUTO_ROTATE) == 1
    assert np.array_equal(fb[:want.size].reshape(want.shape), want) and np.all(fb[want.size:] == POISON)


def test_pipeline_batch_then_orient_its_resident_outputs(gpu_ctx, oracle):
    ctx = gpu_ctx
    names = ["c420_1280x720", "c420_640x368_rstrow", "c444_384x192_q100_rst7", "c444_256x256_q100_opt", "c420_333x217", "c420_512x256_q98_rstrow", "c422_333x217"]
    files = [jpeg_for(n) for n in names]
    orients = [6, 3, 8, 5, 7, 2, 4]
    infos = []
    for f in files:
        info = ImageInfo()
        assert ctx.lib.jda_parse(f, len(f), C.byref(info)) == 0
        infos.append(info)
    geos = [J.output_geometry(i, J.RGB565_LE, 0) for i in infos]
    turned = [J.oriented_geometry(i, J.RGB565_LE, 0, o) for i, o in zip(infos, orients)]
    pit = [(g["canvas_w"] * 2 + 15) & ~15 for g in geos]
    tpit = [(t["w"] * 2 + 15) & ~15 for t in turned]
    offs, toffs, total = [], [], 0
    for g, p in zip(geos, pit):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    for t, p in zip(turned, tpit):
        toffs.append(total)
        total += (p * t["h"] + 255) & ~255
    base = ctx.malloc(total)
    ctx.memset(base, POISON, total)
    pipe = J.Pipeline(ctx, max_images=len(files), depth=2)
    outs = [(base + offs[i], pit[i], geos[i]["canvas_w"], geos[i]["canvas_h"]) for i in range(len(files))]
    st = pipe.wait(pipe.submit(files, outs, [J.RGB565_LE] * len(files), [0] * len(files)))
    assert list(st) == [0] * len(files), st
    # after the wait: the VISIBLE rectangles of the resident canvases, one launch
    before = orient_launches()
    J.orient_surfaces(ctx, [(base + offs[i], pit[i], geos[i]["out_w"], geos[i]["out_h"]) for i in range(len(files))], 2, orients,
                      [(base + toffs[i], tpit[i], turned[i]["w"], turned[i]["h"]) for i in range(len(files))])
    assert orient_launches() == before + 1
    for i, f in enumerate(files):
        want, g = expected(oracle, f, J.RGB565_LE, 0, orients[i])
        got = ctx.to_host(base + toffs[i], tpit[i] * turned[i]["h"]).reshape(turned[i]["h"], tpit[i])
        assert np.array_equal(got[:, :turned[i]["w"] * 2], want), names[i]
        assert np.all(got[:, turned[i]["w"] * 2:] == POISON), names[i]
    pipe.close()
    ctx.free(base)
