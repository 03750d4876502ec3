"""4 / 2 / 1-bpp dithered output on the GPU: the C-ABI (jda_decode_dither_to_host, jda_dither_surfaces), the drop-in class
(JPEGDEC::decodeDither) and the C flavour (JPEG_decodeDither) against the LIVE unmodified reference -- its decodeDither run here
through tests/ref_dither.py, packed bytes and draw logs -- and against the digests it recorded (tests/golden/dither)."""
import ctypes as C

import numpy as np
import pytest

import jpegdec_amd as J
from tests import ref_dither as R
from tests.ref_fixtures import ref_jpeg
from tests.test_dither_cpu import check_refusals, run_sim, seed_of, sim  # noqa: F401  (sim: the row-major twin, for the canvas the reference cannot take)

pytestmark = pytest.mark.gpu

SCALED = [(n, pt, o) for n in R.SYNTH_DITHER for pt in R.DITHER_TYPES for o in R.SCALES]
OTHERS = [c for c in R.recorded_cases() if c[0] not in R.SYNTH_DITHER]


def reference(jpeg, pt, opt, **kw):
    assert R.available(), "oracle/_ref is part of the build: the live reference must be here"
    rc, err, log, strips = R.ref_decode_dither(jpeg, pt, opt, **kw)
    return rc, err, log, R.clip_strips(strips, log)


def product_strips(ctx, jpeg, pt, opt, log):
    rc, packed, g = J.decode_dither_to_host(ctx, jpeg, pt, opt)
    assert rc == 0, rc
    assert g["canvas_w"] == log[0][2] and g["strip_rows"] * len(log) == g["canvas_h"] and g["bits"] == log[0][5]
    return R.clip_strips(R.strips_from_packed(packed, g["pitch"], g["canvas_h"], g["strip_rows"]), log)


@pytest.mark.parametrize("name,pt,opt", SCALED + OTHERS, ids=[R.case_key(*c) for c in SCALED + OTHERS])
def test_c_abi_and_class_equal_the_live_reference(name, pt, opt, gpu_ctx):
    jpeg = R.any_jpeg(name)
    rc, err, log, want = reference(jpeg, pt, opt)
    assert (rc, err) == (1, 0)
    rec = R.golden()[R.case_key(name, pt, opt)]
    assert R.digest(log, want) == {k: rec[k] for k in ("draws", "sha256", "bytes")}, "live reference and recorded digest disagree"
    got = product_strips(gpu_ctx, jpeg, pt, opt, log)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, "C-ABI: strip %d differs from the reference" % k
    crc, cerr, clog, cstrips = R.ref_decode_dither(jpeg, pt, opt, lib_path=J.library_path(), product=True)
    assert (crc, cerr) == (1, 0)
    assert clog == log, "class: draw sequence differs from the reference"
    assert R.clip_strips(cstrips, clog) == want, "class: packed bytes differ from the reference"


@pytest.mark.parametrize("pt", R.DITHER_TYPES)
def test_offsets_and_a_callback_that_stops(pt, gpu_ctx):
    jpeg = R.any_jpeg("c420_333x217")
    for kw, opt in ((dict(xy=(3, 5)), 0), (dict(stop_after=2), 2), (dict(xy=(-7, 100), stop_after=5), 0)):
        rc, err, log, want = reference(jpeg, pt, opt, **kw)
        crc, cerr, clog, cstrips = R.ref_decode_dither(jpeg, pt, opt, lib_path=J.library_path(), product=True, **kw)
        assert (crc, cerr, clog) == (rc, err, log), kw
        assert R.clip_strips(cstrips, clog) == want, kw


@pytest.mark.parametrize("pt", R.DITHER_TYPES)
def test_exif_thumbnail_starts_from_both_headers(pt, gpu_ctx):
    jpeg = R.exif_thumbnail_jpeg()
    rc, err, log, want = reference(jpeg, pt, R.JPEG_EXIF_THUMBNAIL)
    assert (rc, err) == (1, 0) and R.digest(log, want) == R.golden()["exifthumb:%d" % pt]
    crc, cerr, clog, cstrips = R.ref_decode_dither(jpeg, pt, R.JPEG_EXIF_THUMBNAIL, lib_path=J.library_path(), product=True)
    assert (crc, cerr, clog) == (1, 0, log)
    assert R.clip_strips(cstrips, clog) == want


def test_batch_of_mixed_sizes_in_one_launch(gpu_ctx):
    """jda_dither_surfaces: canvases of different sizes, layouts, strip heights and pixel types, resident in HBM, one launch."""
    ctx = gpu_ctx
    items = [("gray_333x217", R.ONE_BIT, 0), ("c420_333x217", R.FOUR_BIT, 0), ("c422_333x217", R.TWO_BIT, 2), ("d_gray_16x130", R.ONE_BIT, 0),
             ("d_c420_4090x144", R.ONE_BIT, 0), ("c440_200x120", R.FOUR_BIT, 8), ("d_gray_72x128", R.TWO_BIT, 0)]
    before = J.kernel_launch_counts()
    gray, packed, strips, seeds, geo, ptrs = [], [], [], [], [], []
    for name, pt, opt in items:
        jpeg = R.any_jpeg(name)
        rc, canvas, g = J.decode_to_host(ctx, jpeg, J.GRAY8, opt)
        assert rc == 0
        ch, cw = canvas.shape
        gp = (cw + 15) & ~15
        d = J.dither_geometry(cw, ch, pt)
        pp = (d["pitch"] + 3) & ~3
        dg, dp = ctx.malloc(gp * ch), ctx.malloc(pp * ch)
        padded = np.zeros((ch, gp), np.uint8)
        padded[:, :cw] = canvas
        ctx.from_host(dg, padded)
        ctx.memset(dp, 0x55, pp * ch)
        info = J.parse(jpeg)
        gray.append((dg, gp, cw, ch)); packed.append((dp, pp, cw, ch)); strips.append(ch // info["mcus_y"]); seeds.append(J.dither_seed(jpeg))
        geo.append((d["pitch"], pp, ch)); ptrs += [dg, dp]
    dither_before = sum(v for k, v in before.items() if "jda_dither_rows" in k)
    J.dither_surfaces(ctx, gray, strips, [pt for _, pt, _ in items], packed, seeds)
    after = J.kernel_launch_counts()
    assert sum(v for k, v in after.items() if "jda_dither_rows" in k) == dither_before + 1, "one launch for the whole batch"
    for (name, pt, opt), (pitch, pp, ch), (dp, _, _, _), strip in zip(items, geo, packed, strips):
        rc, err, log, want = reference(R.any_jpeg(name), pt, opt)
        rows = ctx.to_host(dp, pp * ch).reshape(ch, pp)
        assert np.all(rows[:, pitch:] == 0x55), name
        assert R.clip_strips(R.strips_from_packed(rows, pitch, ch, strip), log) == want, name
    for p in ptrs:
        ctx.free(p)


def test_padded_width_4096_parity_and_4112_row_major_twin(gpu_ctx, sim, oracle):  # noqa: F811
    jpeg = R.any_jpeg("d_c420_4090x144")                # padded width exactly 4096: the widest the reference's error row takes
    for pt in R.DITHER_TYPES:
        rc, err, log, want = reference(jpeg, pt, 0)
        assert log[0][2] == 4096
        assert product_strips(gpu_ctx, jpeg, pt, 0, log) == want
    jpeg = R.any_jpeg("d_gray_4112x72")                 # above it: no reference -- the product's own rule, the ROW-MAJOR TWIN's
    orc, gray, _ = oracle.decode_canvas(jpeg, 3, 0)
    assert orc == 1 and gray.shape[1] == 4112
    for pt in R.DITHER_TYPES:
        rc, packed, g = J.decode_dither_to_host(gpu_ctx, jpeg, pt, 0)
        assert rc == 0
        assert np.array_equal(packed, run_sim(sim, gray, 8, pt, seed_of(sim, jpeg), 0)), pt


def test_refusals_by_error_code(gpu_ctx):
    check_refusals(J.library_path())
    jpeg = R.any_jpeg("gray_333x217")
    lib = J.load_library()
    for pt in (J.RGB8888, J.GRAY8, 7):                  # the one-call form takes dithered types only
        out = np.zeros(1 << 16, np.uint8)
        assert lib.jda_decode_dither_to_host(gpu_ctx.handle, jpeg, len(jpeg), pt, 0, None, out.ctypes.data_as(C.c_void_p), 4096, 16, None) == 1
    for pt in R.DITHER_TYPES:                           # .. and the decode entry points none of them
        out = np.zeros(1 << 20, np.uint8)
        assert lib.jda_decode_to_host(gpu_ctx.handle, jpeg, len(jpeg), pt, 0, out.ctypes.data_as(C.c_void_p), 4096, 16) == 1
    rc, packed, g = J.decode_dither_to_host(gpu_ctx, ref_jpeg("corrupt2"), R.ONE_BIT, 0)      # a bad MCU: status as for GRAY8
    assert rc == 2


class JPEGIMAGE(C.Structure):
    _fields_ = [("magic", C.c_uint32 * 2), ("file_owner", C.c_void_p), ("file_data", C.c_void_p), ("file_check", C.c_uint64), ("state", C.c_uint64 * 40)]


@pytest.mark.parametrize("name,pt,opt", [("c420_333x217", R.ONE_BIT, 0), ("gray_333x217", R.FOUR_BIT, 2), ("squirrel_dither", R.TWO_BIT, 2)])
def test_c_flavour_JPEG_decodeDither(name, pt, opt, gpu_ctx):
    lib = C.CDLL(J.library_path())
    jpeg = R.any_jpeg(name)
    rc, err, log, want = reference(jpeg, pt, opt)
    img = JPEGIMAGE()
    glog, gstrips = [], []
    cb = R.recorder(glog, gstrips)
    src = C.create_string_buffer(jpeg, len(jpeg) + 64)
    lib.JPEG_openRAM.argtypes = [C.c_void_p, C.c_void_p, C.c_int, R.DRAW_CB]
    lib.JPEG_setPixelType.argtypes = [C.c_void_p, C.c_int]
    lib.JPEG_decodeDither.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.JPEG_getLastError.argtypes = [C.c_void_p]
    assert lib.JPEG_openRAM(C.byref(img), src, len(jpeg), cb) == 1
    lib.JPEG_setPixelType(C.byref(img), pt)
    buf = C.create_string_buffer((log[0][2] + 32) * 16)
    assert lib.JPEG_decodeDither(C.byref(img), buf, opt) == 1 and lib.JPEG_getLastError(C.byref(img)) == 0
    assert glog == log and R.clip_strips(gstrips, glog) == want
