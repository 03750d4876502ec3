"""JPEG_PROGRESSIVE_FULL on the GPU: the coefficient-tile kernel (jda_coef_tiles, every layout's instantiation) against the oracle, the one
call with the bit, the class and the C flavour, the default behaviour without the bit, and the refusals.

Every comparison is bit-exact.  Expected pixels of a progressive file: tests/prog_jpeg (pure Python) -> coef_jpeg.write_jpeg (baseline,
same DQT, no truncation event: asserted) -> the oracle (tests/prog_cases.py: Pillow's files; tests/prog_scripts.py: files written under
other scan scripts by tests/prog_write.py, every MCU layout among them).  This file sorts before test_gpu_zz_kernel_coverage.py, which
holds the process to every kernel of the code object: (a) below launches all five jda_coef_tiles instantiations."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpegdec_amd as J
from oracle.loader import RefDecoder
from tests import prog_cases as PC, prog_scripts as PS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = J.PROGRESSIVE_FULL
NAMES = sorted(PC.CASES)
WRITTEN = PS.NAMES + PS.LONG_NAMES
MODES = ((J.RGB8888, 0), (J.RGB565_LE, 0), (J.RGB565_BE, 0), (J.GRAY8, 0), (J.RGB565_LE, J.LUMA_ONLY))


@pytest.fixture(scope="module")
def product_class(product_lib):
    subprocess.run(["make", "classshim"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return RefDecoder(False, path=os.path.join(ROOT, "tests", "libjpegdec_class_shim.so"))


@pytest.fixture(scope="module")
def prog_user(product_lib):
    subprocess.run(["make", "proguser"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return os.path.join(ROOT, "tests", "capi_c", "prog_user")


def _info(jpeg):
    info = J.binding.ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    return info


# ---- (a) the kernel through jda_coef_image_from_coefficients ------------------------------------------------------------------
def test_coef_decode_surfaces_over_baseline_fixtures(gpu_ctx, oracle):
    """decode_coefs of existing baseline fixtures -> jda_coef_decode_surfaces, several images (of all five layouts) in one call, four
    pixel types plus LUMA_ONLY: the oracle's canvas of the file"""
    names = PC.BASELINE_FIXTURES + PC.STRESS_FIXTURES
    made = [PC.fixture_coefs(n, oracle) for n in names]
    images = [J.CoefImage(jpeg, coefs) for jpeg, coefs in made]
    before = J.kernel_launch_counts()
    try:
        for pt, opt in MODES:
            res = J.coef_decode(gpu_ctx, images, [pt] * len(images), [opt] * len(images))
            for n, (jpeg, _), (got, g) in zip(names, made, res):
                orc, want, err = oracle.decode_canvas(jpeg, pt, opt)
                assert orc == 1 and got.shape == want.shape, (n, pt, opt)
                assert np.array_equal(got, want), (n, pt, opt, int(np.count_nonzero(got != want)))
        # mixed pixel types in one call
        pts = [MODES[i % 4][0] for i in range(len(images))]
        for n, (jpeg, _), pt, (got, g) in zip(names, made, pts, J.coef_decode(gpu_ctx, images, pts)):
            assert np.array_equal(got, oracle.decode_canvas(jpeg, pt, 0)[1]), (n, pt)
    finally:
        for im in images:
            im.close()
    after = J.kernel_launch_counts()
    launched = {k: after[k] - before.get(k, 0) for k in after if "jda_coef_tiles" in k and after[k] > before.get(k, 0)}
    assert len(launched) == 5, launched                    # one instantiation per MCU layout, one launch of each per call
    assert all(v == len(MODES) + 1 for v in launched.values()), launched


def test_coef_decode_surfaces_arguments(gpu_ctx, oracle):
    jpeg, coefs = PC.fixture_coefs("c420_333x217", oracle)
    im = J.CoefImage(jpeg, coefs)
    try:
        assert J.coef_decode(gpu_ctx, [], []) == []
        with pytest.raises(J.JdaError) as e:               # full size only
            g = im.geometry(J.RGB8888, 0)
            base = gpu_ctx.malloc(g["canvas_w"] * 4 * g["canvas_h"])
            try:
                err = C.c_int32(0)
                d = gpu_ctx.lib.jda_coef_upload(gpu_ctx.handle, im.handle, C.byref(err))
                assert d and err.value == 0
                outs = (J.binding.Output * 1)(J.binding.Output(base, g["canvas_w"] * 4, g["canvas_w"], g["canvas_h"]))
                try:
                    gpu_ctx.check(gpu_ctx.lib.jda_coef_decode_surfaces(gpu_ctx.handle, 1, (C.c_void_p * 1)(d), outs, (C.c_int32 * 1)(J.RGB8888),
                                                                       (C.c_int32 * 1)(J.SCALE_HALF)), "jda_coef_decode_surfaces")
                finally:
                    gpu_ctx.lib.jda_dev_coef_free(gpu_ctx.handle, d)
            finally:
                gpu_ctx.free(base)
        assert e.value.code == 3
    finally:
        im.close()


# ---- (b) the one call with the bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + WRITTEN)
def test_one_call_with_the_bit(name, gpu_ctx, oracle):
    pj = PS.files(name)[0]
    base, events = PS.reencoded(name)
    assert events == 0, "the re-encoded baseline has %d truncation events" % events
    for pt, opt in MODES[:1] if name in PS.LONG_NAMES else MODES:
        orc, want, err = oracle.decode_canvas(base, pt, opt)
        rc, got, g = J.decode_to_host(gpu_ctx, pj, pt, opt | FULL)
        assert orc == 1 and rc == 0 and got.shape == want.shape, (name, pt, opt, rc)
        assert np.array_equal(got, want), (name, pt, opt, int(np.count_nonzero(got != want)))
    # jda_decode_to_host_ex: every MCU decoded; a clipped canvas (fewer rows, a narrower pitch) gets what fits
    info = _info(pj)
    orc, want, err = oracle.decode_canvas(base, J.RGB565_LE, 0)
    nok = C.c_int32(-1)
    part = np.full((want.shape[0] - 3, want.shape[1] - 6), 0x5A, np.uint8)
    rc = gpu_ctx.lib.jda_decode_to_host_ex(gpu_ctx.handle, pj, len(pj), J.RGB565_LE, FULL, part.ctypes.data_as(C.c_void_p), part.shape[1], part.shape[0], C.byref(nok))
    assert rc == 0 and nok.value == info.mcus_x * info.mcus_y
    assert np.array_equal(part, want[:part.shape[0], :part.shape[1]])
    # on the baseline twin the bit changes nothing
    tw = PS.files(name)[1]
    rc, got, g = J.decode_to_host(gpu_ctx, tw, J.RGB8888, FULL)
    assert rc == 0 and np.array_equal(got, oracle.decode_canvas(tw, J.RGB8888, 0)[1])


def test_files_cut_after_each_scan(gpu_ctx, oracle):
    """a file that ends behind a complete scan decodes to what its scans carry"""
    from tests import prog_jpeg
    name = "c420_200x136_q50_rst"
    pj, dec = PC.files(name)[0], PC.decoded(name)
    for k in (0, 1, 4, dec["n_scans"] - 2):
        cut = PC.cut_after_scan(pj, dec, k)
        base, events = PC.reencode_coefs(prog_jpeg.decode_coefs(cut))
        assert events == 0
        rc, got, g = J.decode_to_host(gpu_ctx, cut, J.RGB8888, FULL)
        assert rc == 0 and np.array_equal(got, oracle.decode_canvas(base, J.RGB8888, 0)[1]), k


def test_tables_between_the_scans(gpu_ctx, oracle):
    """Huffman tables of ids 2 and 3, and a DQT behind the first scan (every component's quantiser was latched by then): the pixels of the file as it was"""
    from tests.test_progressive_full_cpu import remap_table_ids, with_dqt_behind_first_scan
    name = "c420_200x136_q50_rst"
    pj = PC.files(name)[0]
    base, events = PC.reencoded(name)
    assert events == 0
    for variant in (remap_table_ids(pj), with_dqt_behind_first_scan(pj, 0, [255] * 64), with_dqt_behind_first_scan(pj, 1, [255] * 64)):
        assert variant != pj
        for pt in (J.RGB8888, J.RGB565_LE):
            rc, got, g = J.decode_to_host(gpu_ctx, variant, pt, FULL)
            assert rc == 0 and np.array_equal(got, oracle.decode_canvas(base, pt, 0)[1]), pt


def test_a_scan_that_cannot_be_decoded_delivers_nothing(gpu_ctx):
    from tests.test_progressive_full_cpu import _broken
    bad = _broken(PC.files("c420_200x136_q50_rst")[0])
    g = J.output_geometry(_info(bad), J.RGB565_LE, FULL)
    canvas = np.full((g["canvas_h"], g["canvas_w"] * 2), 0x5A, np.uint8)
    nok = C.c_int32(-1)
    rc = gpu_ctx.lib.jda_decode_to_host_ex(gpu_ctx.handle, bad, len(bad), J.RGB565_LE, FULL, canvas.ctypes.data_as(C.c_void_p), canvas.shape[1], canvas.shape[0], C.byref(nok))
    assert rc == 2 and nok.value == 0 and bool((canvas == 0x5A).all())


# ---- (c) the class and the C flavour ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gray_200x136_q85", "c444_333x217_q85", "c422_200x136_q50_rst", "c420_640x368_q85", "c420_17x9_q85_rst"] + PS.ONE_PER_LAYOUT)
def test_class_framebuffer_and_callbacks(name, product_class, oracle, gpu_ctx):
    pj = PS.files(name)[0]
    base, events = PS.reencoded(name)
    assert events == 0
    for pt, opt, max_mcus in ((J.RGB565_LE, 0, 0), (J.RGB8888, 0, 3), (J.GRAY8, 0, 0), (J.RGB565_BE, 128, 0), (J.RGB565_LE, 64, 0)):
        if PS.decoded(name)["sampling"] == "gray" and pt == J.RGB8888:
            continue
        orc, want, err = oracle.decode_canvas(base, pt, opt & 64)
        g = J.output_geometry(_info(base), pt, opt & 64)
        assert orc == 1 and want.shape == (g["canvas_h"], g["canvas_w"] * g["bpp"])
        shape = (g["canvas_h"], g["canvas_w"] + 64)
        a = product_class.decode_cb(pj, pt, opt | FULL, max_mcus=max_mcus, want_log=True, canvas_shape=shape)
        b = product_class.decode_cb(base, pt, opt, max_mcus=max_mcus, want_log=True, canvas_shape=shape)
        assert a["rc"] == 1 and b["rc"] == 1, (a["rc"], a["last_error"], b["rc"])
        assert np.array_equal(a["log"], b["log"]) and a["n_calls"] == b["n_calls"] and a["dma_reuse"] == b["dma_reuse"]
        if max_mcus == 0 and not (opt & 128):
            assert np.array_equal(a["log"], oracle.draw_plan(base, pt, opt & 64))      # the reference's strip plan for that geometry
        vis = g["out_h"]
        assert np.array_equal(a["canvas"][:vis, :want.shape[1]], want[:vis]), (name, pt, opt)
        assert np.array_equal(a["canvas"], b["canvas"])
        rc1, fb1 = product_class.decode_fb(pj, pt, opt | FULL, fill=0x5A)
        rc2, fb2 = product_class.decode_fb(base, pt, opt, fill=0x5A)
        assert rc1 == 1 and rc2 == 1 and np.array_equal(fb1, fb2), (name, pt, opt, rc1, rc2)


def test_class_refusals(product_class, gpu_ctx):
    from tests.orient_util import with_orientation
    from tests.test_progressive_full_cpu import _broken
    pj = PC.files("c420_200x136_q50_rst")[0]
    for kw in (dict(options=FULL, crop=(16, 16, 64, 64)), dict(options=FULL | 2), dict(options=FULL | 8), dict(options=FULL | 32)):
        r = product_class.decode_cb(pj, J.RGB565_LE, canvas_shape=(400, 2600), **kw)
        assert r["rc"] == 0 and r["last_error"] == 3, kw
    r = product_class.decode_cb(with_orientation(pj, 6), J.RGB565_LE, FULL | 1, canvas_shape=(400, 2600))
    assert r["rc"] == 0 and r["last_error"] == 3
    bad = _broken(pj)
    r = product_class.decode_cb(bad, J.RGB565_LE, FULL, want_log=True, canvas_shape=(400, 2600))
    assert r["rc"] == 0 and r["last_error"] == 2 and r["n_calls"] == 0
    rc, fb = product_class.decode_fb(bad, J.RGB565_LE, FULL, fill=0x5A)
    assert rc == 0 and product_class.last_error == 2 and bool((fb == 0x5A).all())


@pytest.mark.parametrize("name", ["gray_200x136_q85", "c420_333x217_q98", "c444_17x9_q50"] + PS.ONE_PER_LAYOUT)
def test_c_flavour(name, prog_user, oracle, gpu_ctx, tmp_path):
    """JPEG_decode with JPEG_PROGRESSIVE_FULL from a plain C program: callbacks (log == the oracle's draw plan of the re-encoded baseline,
    pixels == the expected ones) and framebuffer mode"""
    pj = PS.files(name)[0]
    base, events = PS.reencoded(name)
    assert events == 0
    f = tmp_path / "p.jpg"
    f.write_bytes(pj)
    for pt in (J.RGB565_LE, J.GRAY8) + (() if PS.decoded(name)["sampling"] == "gray" else (J.RGB8888,)):
        g = J.output_geometry(_info(base), pt, 0)
        orc, want, err = oracle.decode_canvas(base, pt, 0)
        out, log = tmp_path / "o.bin", tmp_path / "l.txt"
        r = subprocess.run([prog_user, str(f), str(pt), str(FULL), "0", str(g["canvas_w"]), str(g["canvas_h"]), str(g["bpp"]), "0", str(out), str(log)], timeout=120)
        assert r.returncode == 0
        rows = np.loadtxt(str(log), dtype=np.int32, ndmin=2)
        assert np.array_equal(rows, oracle.draw_plan(base, pt, 0))
        got = np.fromfile(str(out), np.uint8).reshape(g["canvas_h"], g["canvas_w"] * g["bpp"])
        assert np.array_equal(got[:g["out_h"]], want[:g["out_h"]]), (name, pt)
        # framebuffer mode: pitch = the image's width, MCU rows as the reference lays them out = the class's own framebuffer walk of the baseline
        r = subprocess.run([prog_user, str(f), str(pt), str(FULL), "1", str(g["canvas_w"]), str(g["canvas_h"] + 16), str(g["bpp"]), "0", str(out), str(log)], timeout=120)
        assert r.returncode == 0
        fb = np.fromfile(str(out), np.uint8)
        w = _info(base).width
        if w == g["canvas_w"]:                             # (a whole number of MCUs: the framebuffer IS the canvas)
            assert np.array_equal(fb[:want.size].reshape(want.shape), want), (name, pt)
    # a scale bit with it: JPEG_UNSUPPORTED_FEATURE; without the bit: success (the thumbnail)
    g = J.output_geometry(_info(base), J.RGB565_LE, 0)
    args = [str(g["canvas_w"]), str(g["canvas_h"]), "2", "0", str(tmp_path / "o.bin"), str(tmp_path / "l.txt")]
    assert subprocess.run([prog_user, str(f), "0", str(FULL | 2), "0"] + args, timeout=120).returncode == 3
    assert subprocess.run([prog_user, str(f), "0", "0", "0"] + args, timeout=120).returncode == 0


# ---- (d) without the bit: the 1/8 thumbnail, byte for byte ------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + PS.NAMES)
def test_without_the_bit_nothing_changes(name, gpu_ctx, oracle):
    """a written file too gets what the reference gives it: the thumbnail of its first scan -- whatever that scan is (Y alone in split_dc and
    pair) -- or the reference's refusal (tables: DC table ids 2 and 3 in the header)"""
    pj = PS.files(name)[0]
    gray = PS.decoded(name)["sampling"] == "gray"
    for pt, opt in ((J.RGB8888, 0), (J.RGB565_LE, 0), (J.RGB565_BE, J.SCALE_HALF), (J.RGB565_LE, J.SCALE_EIGHTH)) + (((J.GRAY8, 0),) if gray else ()):
        orc, want, err = oracle.decode_canvas(pj, pt, opt)
        rc, got, g = J.decode_to_host(gpu_ctx, pj, pt, opt)
        if name in PS.NEW and PS.NEW[name][1] not in PS.FIRST_SCAN_ALL_DC and orc != 1:
            assert rc == err and rc in (2, 3), (name, pt, opt, rc, orc, err)
            continue
        assert orc == 1 and rc == 0 and np.array_equal(got, want), (name, pt, opt)
        assert g == J.output_geometry(_info(pj), pt, opt | J.SCALE_EIGHTH)


# ---- (e) the refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx):
    pj, tw = PC.files("c420_200x136_q50_rst")
    lib = gpu_ctx.lib
    g = J.output_geometry(_info(pj), J.RGB565_LE, FULL)
    pitch = (g["canvas_w"] * 2 + 15) & ~15
    surf = gpu_ctx.malloc(pitch * g["canvas_h"] * 2)
    try:
        out = (surf, pitch, g["canvas_w"], g["canvas_h"])
        # jda_batch_create*
        prep = J.PreparedImage(pj)
        dimg = J.DeviceImage(gpu_ctx, prep)
        with pytest.raises(J.JdaError) as e:
            J.Batch(gpu_ctx, [dimg], [out], [J.RGB565_LE], [FULL])
        assert e.value.code == 3
        rect = (C.c_int32 * 4)(0, 0, 2, 2)
        err = C.c_int32(0)
        outs = (J.binding.Output * 1)(J.binding.Output(*out))
        h = lib.jda_batch_create_rect(gpu_ctx.handle, 1, (C.c_void_p * 1)(dimg.handle), outs, (C.c_int32 * 1)(J.RGB565_LE), (C.c_int32 * 1)(FULL), rect, C.byref(err))
        assert not h and err.value == 3
        dimg.close(); prep.close()
        # the pipeline: per image, in status[] -- the baseline twin with the bit decodes, the progressive file without it too
        pipe = J.Pipeline(gpu_ctx, max_images=4, depth=2)
        out2 = (surf + pitch * g["canvas_h"], pitch, g["canvas_w"], g["canvas_h"])
        st = pipe.wait(pipe.submit([pj, tw, pj], [out, out2, out], [J.RGB565_LE] * 3, [FULL, FULL, 0]))
        assert st == [3, 0, 0], st
        pipe.close()
        # the one-image entry points that have no full progressive path
        canvas = np.zeros((g["canvas_h"], g["canvas_w"] * 2), np.uint8)
        rc, part, gg, tiles = J.binding.decode_to_host_rect(gpu_ctx, pj, J.RGB565_LE, FULL, (0, 0, 2, 2))
        assert rc == 3
        rc, px, gg = J.decode_oriented_to_host(gpu_ctx, pj, J.RGB565_LE, FULL, 6)
        assert rc == 3
        rc, packed, gg = J.decode_dither_to_host(gpu_ctx, pj, J.ONE_BIT_DITHERED, FULL)
        assert rc == 3
        P = C.c_void_p
        lib.jda_decode_to_host_bands.argtypes = [P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, P, P, C.c_int32, C.c_int32, P, P, C.c_int32, C.c_int32, P, P]
        assert lib.jda_decode_to_host_bands(gpu_ctx.handle, pj, len(pj), J.RGB565_LE, FULL, None, canvas.ctypes.data, canvas.shape[1], canvas.shape[0], None, None, 0, 4, None, None) == 3
        lib.jda_decode_to_host_strips.argtypes = [P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P, C.c_size_t, P, C.c_int32, P, P]
        big = np.zeros(canvas.size * 2, np.uint8)
        assert lib.jda_decode_to_host_strips(gpu_ctx.handle, pj, len(pj), J.RGB565_LE, FULL, 4, big.ctypes.data, big.size, None, 1, None, None) == 3
        lib.jda_decode_to_host_flags.argtypes = [P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, P, P, C.c_int32, C.c_int32, P, P, C.c_int32]
        assert lib.jda_decode_to_host_flags(gpu_ctx.handle, pj, len(pj), J.RGB565_LE, FULL, rect, canvas.ctypes.data, canvas.shape[1], canvas.shape[0], None, None, 0) == 3
        assert lib.jda_decode_to_host_flags(gpu_ctx.handle, pj, len(pj), J.RGB565_LE, FULL, None, canvas.ctypes.data, canvas.shape[1], canvas.shape[0], None, None, 1) == 0
        # a scale bit together with the bit
        for scale in (2, 4, 8):
            assert lib.jda_decode_to_host(gpu_ctx.handle, pj, len(pj), J.RGB565_LE, FULL | scale, canvas.ctypes.data_as(P), canvas.shape[1], canvas.shape[0]) == 3
    finally:
        gpu_ctx.free(surf)
