"""The libjpeg-exact decode on the CPU: the definition against Pillow, and the kernels against the definition.
(a) the numpy twin (tests/exact_util.py) = Pillow 's pixels, draft("L") and draft("YCbCr"), bit for bit, over the file grid of every layout
    and the 333 x 217 fixtures, every file asserted inside the comparison window and the set asserted to force both clamps;
(b) a file outside the window -- amplitude 1023, and 16-bit quantisers -- held to the twin alone;
(c) the kernels lane by lane (tests/hostsim/exact_sim.cpp: jda_exact_planes of all three load phases, jda_exact_colour over the
    runtime's plan, the LDS poisoned before every tile, every global access held to its allocation and alignment, the surface's stores
    counted) = the C row-major twin (exact_twin.h) = the numpy twin, for all three kinds of source, RGB8888 and gray, whole and clipped;
(d) the T.81 reader against the reference's truncated reads; (e) the plan and its refusals; (f) the same as a program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cases, coef_jpeg
from tests import exact_util as X
from tests import recode_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB8888, GRAY8 = 2, 3
FIXTURES = ("gray_333x217", "c444_333x217", "c420_333x217", "c422_333x217", "c440_200x120")


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "tests/hostsim/libjda_exactsim.so"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_exactsim.so"))
    lib.exactsim_run.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.exactsim_plan.argtypes = [C.c_int] * 10 + [C.c_void_p]
    return lib


def is_pillow(f, t):
    assert X.in_window(t), t["range"]
    assert np.array_equal(t["rgb"], X.pillow(f, "RGB"))
    assert np.array_equal(t["gray"], X.pillow(f, "L"))
    assert np.array_equal(t["ycc"], X.pillow(f, "YCbCr"))


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_twin_is_pillow(sampling):
    g = X.grid(sampling)
    assert len(g) >= 10
    kinds = set()
    for name, f in g:
        is_pillow(f, X.twin(f))
        kinds.add(name.split("_")[0])
    assert kinds >= ({"written", "dense60"} if sampling == "4:4:0" else {"baseline", "optimize", "progressive", "restart", "dense60"})
    lo, hi = min(X.twin(f)["range"][0] for _, f in g), max(X.twin(f)["range"][1] for _, f in g)
    assert lo < -128 and hi > 127                                   # both clamps are forced
    # the shapes the edges need: odd and even chroma extents on both axes, a one-sample chroma row and column, every w mod 4
    assert {w % 4 for w, h in X.SIZES} == {0, 1, 2, 3} and (1, 1) in X.SIZES and (2, 2) in X.SIZES


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_are_pillow(name):
    f = cases.jpeg_for(name)
    is_pillow(f, X.twin(f))


def test_dense_blocks_force_the_clamps():
    for sampling in coef_jpeg.LAYOUTS:
        f = X.written_file(33, 31, sampling, 0, amplitude=60)
        t = X.twin(f)
        is_pillow(f, t)
    f = X.written_file(40, 24, "4:2:0", 0, amplitude=120, seed=2)
    t = X.twin(f)
    assert t["range"][0] < -128 and t["range"][1] > 127 and t["planes"][0].min() == 0 and t["planes"][0].max() == 255
    is_pillow(f, t)


def test_outside_the_window_the_contract_is_the_twin():
    """amplitude 1023 in every position: libjpeg-turbo's SIMD IDCT saturates where the C table wraps, so Pillow is no witness here"""
    f = X.written_file(24, 16, "4:2:0", 0, amplitude=1023, seed=9)
    t = X.twin(f)
    assert not X.in_window(t) and (t["range"][0] < -512 or t["range"][1] > 511)
    assert X.range_limit(np.array([511, 512, -512, -513, 767, 1023, -1], np.int32)).tolist() == [255, 0, 0, 255, 0, 127, 127]


def run(sim, f, source, pt, clip=None, coefs=None):
    t = X.twin(f)
    h, w = t["gray"].shape
    bpp = 4 if pt == RGB8888 else 1
    pitch = (w * bpp + 15) & ~15
    raw = np.full(pitch * h + 16, 0x5A, np.uint8)
    a = (-raw.ctypes.data) & 15
    out = raw[a:a + pitch * h]
    twin_out = np.zeros((h, w * bpp), np.uint8)
    ncomp = len(t["planes"])
    want_planes = not (pt == GRAY8 and ncomp == 3)
    pbytes = sum(p.size for p in t["planes"])
    planes, tplanes = np.zeros(pbytes, np.uint8), np.zeros(pbytes, np.uint8)
    info = (C.c_int32 * 5)()
    cw, cr = clip if clip else (w, h)
    nb = 0 if coefs is None else coefs.shape[0]
    rc = sim.exactsim_run(f, len(f), None if coefs is None else coefs.ctypes.data, nb, source, pt, out.ctypes.data, pitch, cw, cr, twin_out.ctypes.data,
                          planes.ctypes.data if want_planes else None, tplanes.ctypes.data if want_planes else None, info)
    assert rc == 0, (rc, source, pt)
    assert info[0] > 0 and info[3] == 0 and info[4] == 0, list(info)
    assert (info[1], info[2]) == t["range"]
    want = X.rgba(t, pt == GRAY8)
    assert np.array_equal(twin_out, want), "the C twin is the numpy twin"
    cw, cr = min(cw, w), min(cr, h)
    got = out.reshape(h, pitch)
    assert np.array_equal(got[:cr, :cw * bpp], want[:cr, :cw * bpp]), ("the lanes", source, pt, clip)
    assert np.all(got[:, cw * bpp:] == 0x5A) and np.all(got[cr:] == 0x5A)
    if want_planes:
        flat = np.concatenate([p.reshape(-1) for p in t["planes"]])
        assert np.array_equal(tplanes, flat) and np.array_equal(planes, flat)


def sources_of(f):
    prog = R.frame_header(f)[1] == 0xC2
    return [(0, None), (1, None)] if prog else [(2, None), (0, X.natural_blocks(f)), (1, X.natural_blocks(f))]


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_lanes_are_the_twin(sim, sampling):
    extra = [("wrap", X.written_file(24, 16, sampling, 0, amplitude=1023, seed=9)), ("word", X.written_file(24, 16, sampling, 0, amplitude=60, seed=4, word=True))]
    for name, f in X.grid(sampling) + extra:
        for source, coefs in sources_of(f):
            for pt in (RGB8888, GRAY8):
                run(sim, f, source, pt, coefs=coefs)


@pytest.mark.parametrize("name", FIXTURES)
def test_lanes_on_the_fixtures(sim, name):
    run(sim, cases.jpeg_for(name), 2, RGB8888)


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_clipped_surfaces(sim, sampling):
    f = dict(X.grid(sampling))["%s_33x31_q90" % ("written" if sampling == "4:4:0" else "baseline")]
    for clip in ((32, 31), (33, 30), (0, 31), (33, 0), (34, 32), (1, 1), (5, 7)):
        for pt in (RGB8888, GRAY8):
            run(sim, f, 2, pt, clip=clip)


@pytest.mark.parametrize("name", ("c440_200x120", "c422_333x217", "gray_333x217"))
def test_whole_magnitudes_where_the_reference_truncates(sim, oracle, name):
    """a baseline file with truncation events (the reference's window runs dry inside a magnitude and it reads fewer bits): the exact road's
    reader takes T.81's whole magnitudes, so its pixels are Pillow's -- and the oracle's canvas of the same file is not"""
    import jpegdec_amd as J
    f = cases.jpeg_for(name)
    p = J.PreparedImage(f)
    assert p.truncation_events() > 0
    p.close()
    t = X.twin(f)
    is_pillow(f, t)
    run(sim, f, 2, RGB8888)                                          # (the baseline load phase's coefficients, through the lanes: the twin's pixels)
    h, w = t["gray"].shape
    gray = name.startswith("gray")
    orc, canvas, err = oracle.decode_canvas(f, J.GRAY8 if gray else J.RGB8888, 0)
    assert orc == 1
    bpp = 1 if gray else 4
    assert not np.array_equal(canvas[:h, :w * bpp], X.rgba(t, gray))


def test_plan(sim):
    out = (C.c_int64 * 12)()
    for (w, h), (sub, ncomp, hs, vs, per) in [((w, h), lay) for w, h in X.SIZES + ((333, 217),)
                                              for lay in ((0, 1, 1, 1, 64), (0x11, 3, 1, 1, 20), (0x21, 3, 2, 1, 16), (0x12, 3, 1, 2, 16), (0x22, 3, 2, 2, 10))]:
        assert sim.exactsim_plan(w, h, ncomp, sub, 0, RGB8888, 0, 0, 0, -1, out) == 0
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        py, pc = (mx * 8 * hs + 15) & ~15, (mx * 8 + 15) & ~15
        ysz, csz = (py * my * 8 * vs + 255) & ~255, (pc * my * 8 + 255) & ~255
        want = [hs, vs, py, pc if ncomp == 3 else 0, my * 8 * vs, my * 8 if ncomp == 3 else 0, -(-w // hs), -(-h // vs), ysz if ncomp == 3 else 0,
                ysz + csz if ncomp == 3 else 0, ysz + (2 * csz if ncomp == 3 else 0), my * -(-mx // per)]
        assert list(out) == want, (w, h, hex(sub))
        if ncomp == 3:                                              # a gray surface of a colour file: no chroma planes
            assert sim.exactsim_plan(w, h, ncomp, sub, 0, GRAY8, 1, 0, 0, -1, out) == 0 and out[10] == ysz and out[3] == 0
    # the 24-bit question: a dequantised value of a legal 8-bit file stays under 2^19, but a coefficient image's int16 coefficients do not --
    # the IDCT's multiplies are 32-bit, and only the dequantisation (int16 x uint16) takes the 24-bit multiplier
    assert 2047 * 255 < 1 << 19 and 32767 * 255 * 2 >= 1 << 23 and 32768 < 1 << 23 and 65535 < 1 << 23
    for pt in (0, 1, 4, 5, 6, -1):
        assert sim.exactsim_plan(33, 31, 3, 0x22, 0, pt, 0, 0, 0, -1, out) == 1
    assert sim.exactsim_plan(33, 31, 3, 0x22, 1, RGB8888, 0, 0, 0, -1, out) == 3      # an Adobe APP14 segment
    assert sim.exactsim_plan(33, 31, 4, 0x11, 0, RGB8888, 0, 0, 0, -1, out) == 3      # four components
    assert sim.exactsim_plan(0, 31, 3, 0x22, 0, RGB8888, 0, 0, 0, -1, out) == 1
    # a resident baseline image: every MCU validated by its pre-scan (3 x 2 of them here), and no progressive file's first scan
    assert sim.exactsim_plan(33, 31, 3, 0x22, 0, RGB8888, 0, 1, 0, 6, out) == 0
    assert sim.exactsim_plan(33, 31, 3, 0x22, 0, RGB8888, 0, 1, 0, 5, out) == 2
    assert sim.exactsim_plan(33, 31, 3, 0x22, 0, RGB8888, 0, 1, 0, 0, out) == 2
    assert sim.exactsim_plan(33, 31, 3, 0x22, 0, RGB8888, 0, 0, 0, 5, out) == 0       # (a coefficient image has no such count)
    assert sim.exactsim_plan(33, 31, 3, 0x22, 0, RGB8888, 0, 1, 1, 6, out) == 3
    assert sim.exactsim_plan(33, 31, 3, 0x22, 0, RGB8888, 0, 0, 1, -1, out) == 0      # (a progressive file as a coefficient image)


def test_refused_files(sim):
    """real files through the sources' own records: a baseline file whose pre-scan stops at a bad MCU (JDA_DECODE_ERROR, nothing walked), and
    a file with an Adobe APP14 segment as a baseline image and as a coefficient image (JDA_UNSUPPORTED_FEATURE): the surface stays untouched"""
    import jpegdec_amd as J
    bad, adobe = R.refused()["bad_mcu"][0], R.refused()["adobe"][0]
    for f, source, coefs, want in ((bad, 2, None, 2), (adobe, 2, None, 3), (adobe, 0, X.natural_blocks(adobe), 3), (adobe, 1, X.natural_blocks(adobe), 3)):
        info = J.parse(f)
        pitch = (info["width"] * 4 + 15) & ~15
        raw = np.full(pitch * info["height"] + 16, 0x5A, np.uint8)
        a = (-raw.ctypes.data) & 15
        nb = 0 if coefs is None else coefs.shape[0]
        rc = sim.exactsim_run(f, len(f), None if coefs is None else coefs.ctypes.data, nb, source, RGB8888, raw[a:].ctypes.data, pitch, info["width"], info["height"],
                              None, None, None, None)
        assert rc == want, (rc, source, want)
        assert np.all(raw == 0x5A)


def test_sanitizer_program(tmp_path):
    """the plan and the lanes over three files as a program of their own under ASan + UBSan (nothing is loaded into this process)"""
    subprocess.run(["make", "exactasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    picks = (("4:2:0", "progressive_75x53_q30"), ("4:2:2", "restart_64x48_q90"), ("gray", "baseline_161x17_q100"), ("4:4:0", "written_17x9_q30"))
    paths = []
    for k, (s, name) in enumerate(picks):
        paths.append(str(tmp_path / ("f%d.jpg" % k)))
        with open(paths[-1], "wb") as fh:
            fh.write(dict(X.grid(s))[name])
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "exact_asan")] + paths, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "exact_asan ok" in r.stdout, r.stdout[-4000:]


def test_constants_and_exports():
    import jpegdec_amd as J
    for name in ("exact_decode", "exact_planes", "decode_to_host_exact"):
        assert callable(getattr(J, name)), name
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    assert "int jda_exact_decode_surfaces(" in hdr and "int jda_exact_decode_planes(" in hdr and "int jda_decode_to_host_exact(" in hdr
    for kw in (dict(decoder="turbo"), dict(decoder="libjpeg", prescale=True, size=(8, 8)), dict(decoder="libjpeg", options=J.SCALE_QUARTER),
               dict(decoder="libjpeg", options=J.PROGRESSIVE_FULL), dict(decoder="libjpeg", options=J.LUMA_ONLY | 1)):
        with pytest.raises(ValueError):                             # (refused before torch or the GPU is touched)
            J.decode_to_tensors(None, [], **kw)
