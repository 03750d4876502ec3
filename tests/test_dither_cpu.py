"""4 / 2 / 1-bpp dithered output without a GPU.

* the kernel's per-pixel step and lane schedule (tests/hostsim/dither_sim.cpp: jda_dither_step of jda_device_core.h, rows dealt to
  lanes two pixels apart, 64-row groups dealt to wavefronts) against the row-major twin that knows nothing of it
  (tests/hostsim/dither_twin.h), and both against what the unmodified reference recorded (tests/golden/dither) and -- where
  oracle/_ref exists -- delivers live;
* JPEGDEC::decodeDither through the class's CPU build (tests/class_cpu): draw sequence, bytes and refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ref_dither as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASS_CPU = os.path.join(ROOT, "tests", "class_cpu", "libjpegdec_class_cpu.so")


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_dithersim.so"))
    lib.jda_dither_seed.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def class_cpu():
    import subprocess
    subprocess.run(["make", "classcpu"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return CLASS_CPU


def run_sim(sim, gray, strip, pt, seed, waves):
    """waves == 0: the row-major twin; otherwise the kernel's schedule with that many wavefronts."""
    gray = np.ascontiguousarray(gray)
    ch, cw = gray.shape
    pitch = (cw * R.BITS[pt] + 7) // 8
    out = np.full((ch, pitch + 3), 0x55, np.uint8)
    sp = None if seed is None else seed.ctypes.data_as(C.c_void_p)
    if waves == 0:
        rc = sim.dithersim_rowmajor(gray.ctypes.data_as(C.c_void_p), cw, cw, ch, strip, pt, sp, out.ctypes.data_as(C.c_void_p), out.shape[1])
    else:
        rc = sim.dithersim_skewed(gray.ctypes.data_as(C.c_void_p), cw, cw, ch, strip, pt, sp, out.ctypes.data_as(C.c_void_p), out.shape[1], waves)
    assert rc == 0
    assert np.all(out[:, pitch:] == 0x55), "wrote past the packed row"
    return out[:, :pitch]


def seed_of(sim, jpeg):
    seed = np.zeros(2184, np.uint8)
    assert sim.jda_dither_seed(jpeg, len(jpeg), 0, seed.ctypes.data_as(C.c_void_p)) == 0
    return seed


SIM_CASES = [c for c in R.recorded_cases() if c[0] in R.SIM_JPEGS or c[0] in R.SYNTH_DITHER + R.RESTART_DITHER + R.PROGRESSIVE_DITHER]


@pytest.mark.parametrize("name,pt,opt", SIM_CASES, ids=[R.case_key(*c) for c in SIM_CASES])
def test_skewed_schedule_equals_row_major_equals_reference(name, pt, opt, sim, oracle):
    jpeg = R.any_jpeg(name)
    want = R.golden()[R.case_key(name, pt, opt)]
    orc, gray, oerr = oracle.decode_canvas(jpeg, 3, opt)
    assert orc == 1
    strip, log = want["draws"][0][3], [tuple(d) for d in want["draws"]]
    assert gray.shape[1] == log[0][2] and gray.shape[0] == strip * len(log)
    seed = seed_of(sim, jpeg)
    twin = run_sim(sim, gray, strip, pt, seed, 0)
    for waves in (1, 2, 8):
        assert np.array_equal(run_sim(sim, gray, strip, pt, seed, waves), twin), "schedule with %d wavefronts differs from row-major order" % waves
    pitch = twin.shape[1]
    got = R.digest(log, R.clip_strips(R.strips_from_packed(twin, pitch, gray.shape[0], strip), log))
    assert got["sha256"] == want["sha256"] and got["bytes"] == want["bytes"], "differs from the recorded reference bytes"
    if R.available():                                   # the live reference, where it was built
        rc, err, rlog, rstrips = R.ref_decode_dither(jpeg, pt, opt)
        assert rc == 1 and R.digest(rlog, R.clip_strips(rstrips, rlog)) == {k: want[k] for k in ("draws", "sha256", "bytes")}


def raw_patterns(w, h):
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    rng = np.random.RandomState(w * 131 + h)
    return {
        "white": np.full((h, w), 255, np.uint8),
        "checker": (((x + y) & 1) * 255).astype(np.uint8) + np.zeros((h, w), np.uint8),
        "ramp": ((x * 255 // max(w - 1, 1) + y * 3) % 256).astype(np.uint8) + np.zeros((h, w), np.uint8),
        "noise": rng.randint(0, 256, (h, w)).astype(np.uint8),
    }


@pytest.mark.parametrize("w", [1, 2, 7, 9, 63, 65])
@pytest.mark.parametrize("strip", [1, 2, 4, 8, 16])
def test_raw_arrays_row_major_twin_only(w, strip, sim):
    """No JPEG and no reference here (the reference only dithers what it decoded): the kernel's schedule against the ROW-MAJOR TWIN
    alone, on widths that are not whole bytes, every strip height and inputs that saturate -- with and without a seed."""
    h = 64 * 2 + strip * 3
    h -= h % strip
    seed = (np.arange(2184) * 37 % 251).astype(np.uint8)
    for pname, gray in raw_patterns(w, h).items():
        for pt in R.DITHER_TYPES:
            for sd in (None, seed):
                twin = run_sim(sim, gray, strip, pt, sd, 0)
                for waves in (1, 3):
                    assert np.array_equal(run_sim(sim, gray, strip, pt, sd, waves), twin), (pname, pt, waves, sd is not None)


def test_wide_canvas_beyond_the_reference_row(sim, oracle):
    """Padded width 4112 > 4096: the reference's error row overruns its buffer; the product's rule is the twin's."""
    jpeg = R.any_jpeg("d_gray_4112x72")
    orc, gray, _ = oracle.decode_canvas(jpeg, 3, 0)
    assert orc == 1 and gray.shape[1] == 4112
    seed = seed_of(sim, jpeg)
    for pt in R.DITHER_TYPES:
        twin = run_sim(sim, gray, 8, pt, seed, 0)
        assert np.array_equal(run_sim(sim, gray, 8, pt, seed, 8), twin)


CLASS_CASES = [c for c in R.recorded_cases() if c[0] in ("gray_333x217", "c420_333x217", "c422_333x217", "gray_64x64_rst3", "pgray_100x100", "d_gray_16x130", "demo")]


@pytest.mark.parametrize("name,pt,opt", CLASS_CASES, ids=[R.case_key(*c) for c in CLASS_CASES])
def test_class_cpu_build_draw_sequence_and_bytes(name, pt, opt, class_cpu):
    want = R.golden()[R.case_key(name, pt, opt)]
    rc, err, log, strips = R.ref_decode_dither(R.any_jpeg(name), pt, opt, lib_path=class_cpu, product=True)
    assert (rc, err) == (1, 0)
    assert R.digest(log, R.clip_strips(strips, log)) == {k: want[k] for k in ("draws", "sha256", "bytes")}


@pytest.mark.parametrize("pt", R.DITHER_TYPES)
def test_class_cpu_build_offsets_and_early_stop(pt, class_cpu):
    g = R.golden()
    jpeg = R.any_jpeg("c420_333x217")
    rc, err, log, strips = R.ref_decode_dither(jpeg, pt, 0, xy=(3, 5), lib_path=class_cpu, product=True)
    assert (rc, err) == (1, 0)
    assert R.digest(log, R.clip_strips(strips, log)) == g[R.case_key("c420_333x217", pt, 0) + ":xy3,5"]
    want = g[R.case_key("c420_333x217", pt, 2) + ":stop2"]
    rc, err, log, strips = R.ref_decode_dither(jpeg, pt, 2, stop_after=2, lib_path=class_cpu, product=True)
    assert dict(R.digest(log, R.clip_strips(strips, log)), rc=rc, err=err) == want


@pytest.mark.parametrize("pt", R.DITHER_TYPES)
def test_class_cpu_build_exif_thumbnail(pt, class_cpu):
    rc, err, log, strips = R.ref_decode_dither(R.exif_thumbnail_jpeg(), pt, R.JPEG_EXIF_THUMBNAIL, lib_path=class_cpu, product=True)
    assert (rc, err) == (1, 0)
    assert R.digest(log, R.clip_strips(strips, log)) == R.golden()["exifthumb:%d" % pt]


def check_refusals(lib_path):
    jpeg = R.any_jpeg("c420_333x217")
    INVALID, UNSUPPORTED = 1, 3
    for kw, code in ((dict(null_buffer=True), INVALID), (dict(framebuffer=True), UNSUPPORTED), (dict(crop=(16, 16, 64, 64)), UNSUPPORTED),
                     (dict(decode_instead=True), UNSUPPORTED)):
        rc, err, log, _ = R.ref_decode_dither(jpeg, R.ONE_BIT, 0, lib_path=lib_path, product=True, **kw)
        assert (rc, err, log) == (0, code, []), kw
    rc, err, log, _ = R.ref_decode_dither(jpeg, R.ONE_BIT, R.JPEG_USES_DMA, lib_path=lib_path, product=True)      # two error rows in the reference
    assert (rc, err, log) == (0, UNSUPPORTED, [])
    for pt in (0, 2, 3):                                # decodeDither with a pixel type that is not a dithered one
        rc, err, log, _ = R.ref_decode_dither(jpeg, pt, 0, lib_path=lib_path, product=True)
        assert (rc, err, log) == (0, INVALID, []), pt
    # a colour progressive file: refused as for EIGHT_BIT_GRAYSCALE
    rc, err, log, _ = R.ref_decode_dither(R.any_jpeg("p420_200x120"), R.ONE_BIT, 0, lib_path=lib_path, product=True)
    assert (rc, err, log) == (0, UNSUPPORTED, [])


def test_class_cpu_build_refusals(class_cpu):
    check_refusals(class_cpu)


def test_geometry_and_constants():
    import jpegdec_amd as J
    assert (J.FOUR_BIT_DITHERED, J.TWO_BIT_DITHERED, J.ONE_BIT_DITHERED) == (4, 5, 6)
    assert J.dither_geometry(333, 10, J.FOUR_BIT_DITHERED) == {"bits": 4, "pitch": 167, "bytes": 1670}
    assert J.dither_geometry(42, 3, J.TWO_BIT_DITHERED) == {"bits": 2, "pitch": 11, "bytes": 33}
    assert J.dither_geometry(42, 3, J.ONE_BIT_DITHERED) == {"bits": 1, "pitch": 6, "bytes": 18}
    with pytest.raises(J.JdaError):
        J.dither_geometry(42, 3, J.GRAY8)
    # the decode entry points keep refusing the dithered types
    from jpegdec_amd.binding import ImageInfo
    jpeg, info = R.any_jpeg("gray_333x217"), ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    for pt in R.DITHER_TYPES:
        with pytest.raises(J.JdaError):
            J.output_geometry(info, pt, 0)
