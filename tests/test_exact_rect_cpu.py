"""The libjpeg-exact decode of a pixel rectangle on the CPU: the definition against Pillow's crop, the plan against an
independent read set, and the kernels' lanes against the definition.
(a) the numpy reference (tests/exact_rect_util.py: the whole-image twins, cropped, with libjpeg's narrow-plane rule) = Pillow's
    Image.open(f).crop(box), draft() in front for 1/2, 1/4, 1/8, every file asserted inside the comparison window;
(b) jda_exact_rect_plan = the smallest MCU rectangle holding the read set derived pixel by pixel from the upsampling formulas, for every
    rectangle of the set, with and without chroma, the narrow-plane rule at own widths 1, 2, 3, every refusal;
(c) the existing planes lanes over the rectangle's tile list into a poisoned scratch, then the new colour lanes (tests/hostsim/
    exact_rect_sim.cpp): every load inside its allocation and of a plane byte this rectangle's planes stage stored, every byte of the clip
    stored exactly once and none outside = the reference = the C row-major twin's crop, for dense, sparse and baseline sources;
(d) a rectangle equal to the image = the whole decode; (e) clipped surfaces; (f) the same as a program under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import coef_jpeg
from tests import exact_rect_util as Q
from tests import exact_scaled_util as S
from tests import exact_util as X
from tests import recode_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB8888, GRAY8 = 2, 3
SCALES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "tests/hostsim/libjda_exactrectsim.so"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_exactrectsim.so"))
    lib.exactrectsim_plan.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_void_p]
    lib.exactrectsim_run.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    return lib


def files_of(sampling):
    return [(Q.fixture(sampling), (333, 217))] + Q.small_files(sampling)


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_reference_is_pillows_crop(sampling):
    compared = 0
    for f, (w, h) in files_of(sampling):
        for s in SCALES:
            if not S.forcible(w, h, s):
                continue
            t = Q.reference(f, s)
            assert X.in_window(t), t["range"]
            sw, sh = S.scaled_size(w, h, s)
            assert t["gray"].shape == (sh, sw)
            # the whole image once (every rectangle of the set is a crop of it) ..
            assert np.array_equal(t["rgb"], Q.pillow_crop(f, s, (0, 0, sw, sh), "RGB")) and np.array_equal(t["gray"], Q.pillow_crop(f, s, (0, 0, sw, sh), "L"))
            # .. and Pillow's own crop() for a stride of the set
            for rect in Q.rect_set(sw, sh, sampling, s)[::23]:
                x, y, rw, rh = rect
                assert np.array_equal(Q.crop(f, s, rect).reshape(rh, rw, 4)[..., :3], Q.pillow_crop(f, s, rect, "RGB")), (s, rect)
                assert np.array_equal(Q.crop(f, s, rect, gray=True), Q.pillow_crop(f, s, rect, "L")), (s, rect)
                compared += 1
    assert compared >= 100


@pytest.mark.parametrize("sampling", ("4:2:0", "4:2:2"))
def test_narrow_planes_are_replicated_as_pillow_does(sampling):
    """own widths 1 and 2 at full size: the reference replicates (libjpeg's rule) and is Pillow; the full-size twin interpolates there"""
    differs = 0
    for w, h in ((2, 8), (3, 5), (4, 4), (4, 9)):
        for q in (30, 95):
            f = S.pillow_file(w, h, sampling, q)
            t = Q.reference(f, 1)
            assert Q.axis_kinds(w, h, sampling, 1)[0] == Q.REPLICATE
            assert np.array_equal(t["rgb"], X.pillow(f, "RGB"))
            differs += not np.array_equal(t["rgb"], X.twin(f)["rgb"])
    assert differs > 0
    assert Q.axis_kinds(5, 4, sampling, 1)[0] == Q.FANCY and Q.axis_kinds(6, 4, sampling, 1)[0] == Q.FANCY


def plan(sim, w, h, sampling, pt, s, rect):
    sub, ncomp = Q.SUB[sampling]
    out = (C.c_int32 * 4)(-1, -1, -1, -1)
    rc = sim.exactrectsim_plan(w, h, ncomp, sub, pt, s, (C.c_int32 * 4)(*rect), out)
    return rc, tuple(out)


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_plan_is_the_smallest_mcu_rectangle_of_the_read_set(sim, sampling):
    checked, grew = 0, 0
    for w, h in ((333, 217), (17, 9), (5, 7)):
        for s in SCALES:
            sw, sh = S.scaled_size(w, h, s)
            for rect in Q.rect_set(sw, sh, sampling, s):
                for pt in (RGB8888, GRAY8):
                    luma_only = pt == GRAY8
                    want = Q.mcu_rect(w, h, sampling, s, rect, luma_only)
                    assert plan(sim, w, h, sampling, pt, s, rect) == (0, want), (w, h, s, rect, pt)
                    checked += 1
                if sampling != "gray":
                    grew += Q.mcu_rect(w, h, sampling, s, rect, False) != Q.mcu_rect(w, h, sampling, s, rect, True)
    assert checked > 5000
    if sampling in ("4:2:0", "4:2:2", "4:4:0"):                         # (the fancy neighbour adds an MCU somewhere; without chroma it does not)
        assert grew > 0


@pytest.mark.parametrize("sampling", ("4:2:0", "4:2:2"))
def test_plan_narrow_plane_rule(sim, sampling):
    """own widths 1, 2 (replicated: no neighbour is read) and 3 (fancy) at full size, every rectangle of the image"""
    for w in (1, 2, 3, 4, 5, 6):
        h = 20
        cw = -(-w // 2)
        assert Q.axis_kinds(w, h, sampling, 1)[0] == (Q.REPLICATE if cw <= 2 else Q.FANCY)
        for x in range(w):
            for rw in range(1, w - x + 1):
                for y, rh in ((0, 1), (15, 1), (15, 2), (16, 1), (7, 9), (0, 20)):
                    rect = (x, y, rw, rh)
                    assert plan(sim, w, h, sampling, RGB8888, 1, rect) == (0, Q.mcu_rect(w, h, sampling, 1, rect)), (w, rect)
    # replicated both ways: row 15 of a 4:2:0 image 4 wide reads chroma row 7 alone, one MCU row; 6 wide (fancy) reads row 8 as well
    if sampling == "4:2:0":
        assert plan(sim, 4, 40, sampling, RGB8888, 1, (0, 15, 1, 1))[1] == (0, 0, 1, 1)
        assert plan(sim, 6, 40, sampling, RGB8888, 1, (0, 15, 1, 1))[1] == (0, 0, 1, 2)


def test_plan_refusals(sim):
    import jpegdec_amd as J
    for s in SCALES:
        sw, sh = S.scaled_size(333, 217, s)
        for rect in ((0, 0, 0, 5), (0, 0, 5, 0), (0, 0, -1, 5), (3, 3, 5, -2), (-1, 0, 5, 5), (0, -1, 5, 5), (sw, 0, 1, 1), (0, sh, 1, 1), (sw - 4, 0, 5, 1), (0, sh - 4, 1, 5),
                     (0, 0, sw + 1, sh), (2 ** 31 - 1, 0, 2, 1), (0, 2 ** 31 - 1, 1, 2)):
            for sampling in ("gray", "4:2:0"):
                assert plan(sim, 333, 217, sampling, RGB8888, s, rect)[0] == 1, (s, rect)
        assert plan(sim, 333, 217, "4:2:0", RGB8888, s, (sw - 1, sh - 1, 1, 1))[0] == 0
    assert plan(sim, 333, 217, "4:2:0", RGB8888, 3, (0, 0, 1, 1))[0] == 1          # a scale outside 1, 2, 4, 8
    assert plan(sim, 333, 217, "4:2:0", 0, 1, (0, 0, 1, 1))[0] == 1                # a pixel type the road lacks
    sub, ncomp = 0x11, 4
    assert sim.exactrectsim_plan(33, 31, ncomp, sub, RGB8888, 1, (C.c_int32 * 4)(0, 0, 1, 1), (C.c_int32 * 4)()) == 3
    # the public call, through a real file's header
    f = Q.fixture("4:2:0")
    assert J.exact_rect_mcus(f, (5, 6, 40, 30)) == Q.mcu_rect(333, 217, "4:2:0", 1, (5, 6, 40, 30))
    assert J.exact_rect_mcus(f, (5, 6, 40, 30), 1, J.GRAY8) == Q.mcu_rect(333, 217, "4:2:0", 1, (5, 6, 40, 30), True)
    assert J.exact_rect_mcus(f, (5, 6, 20, 10), 4) == Q.mcu_rect(333, 217, "4:2:0", 4, (5, 6, 20, 10))
    for bad in ((0, 0, 0, 0), (330, 0, 4, 1), (-1, 0, 2, 2)):
        with pytest.raises(J.JdaError) as e:
            J.exact_rect_mcus(f, bad)
        assert e.value.code == 1


def run(sim, f, source, pt, s, rects, clips=None, coefs=None, twin=False):
    """the rectangles through the lanes -> ([the clipped pixels of each], info); every status must be 0"""
    t = Q.reference(f, s)
    h, w = t["gray"].shape
    bpp = 4 if pt == RGB8888 else 1
    n = len(rects)
    sizes = []
    for k, (x, y, rw, rh) in enumerate(rects):
        cw, cr = (rw, rh) if clips is None else (max(0, min(rw, clips[k][0])), max(0, min(rh, clips[k][1])))
        sizes.append((cr, cw * bpp))
    out = np.full(sum(a * b for a, b in sizes) + 16, 0x77, np.uint8)
    twin_out = np.zeros((h, w * bpp), np.uint8)
    status = (C.c_int32 * n)(*([99] * n))
    info = (C.c_int32 * 2)()
    flat = (C.c_int32 * (4 * n))(*[v for r in rects for v in r])
    cl = None if clips is None else (C.c_int32 * (2 * n))(*[v for c in clips for v in c])
    nb = 0 if coefs is None else coefs.shape[0]
    rc = sim.exactrectsim_run(f, len(f), None if coefs is None else coefs.ctypes.data, nb, source, pt, s, n, flat, cl, out.ctypes.data,
                              twin_out.ctypes.data if twin else None, status, info)
    assert rc == 0, (rc, source, pt, s)
    bad = [(rects[k], status[k]) for k in range(n) if status[k] != 0]
    assert not bad, (source, pt, s, bad[:5], len(bad))
    got, at = [], 0
    for a, b in sizes:
        got.append(out[at:at + a * b].reshape(a, b))
        at += a * b
    assert np.all(out[at:] == 0x77)
    return got, list(info), twin_out


def sources_of(f):
    prog = R.frame_header(f)[1] == 0xC2
    return [(0, None), (1, None)] if prog else [(2, None), (0, X.natural_blocks(f)), (1, X.natural_blocks(f))]


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_lanes_are_the_reference(sim, sampling):
    """the whole rectangle set over the 333 x 217 file and the small ones, every scale, every kind of source (the baseline reader takes the
    whole set, the coefficient sources a stride of it), RGB8888 and gray"""
    ran = 0
    for f, (w, h) in files_of(sampling):
        narrow = Q.axis_kinds(w, h, sampling, 1)[0] == Q.REPLICATE
        for s in SCALES:
            sw, sh = S.scaled_size(w, h, s)
            rects = Q.rect_set(sw, sh, sampling, s)
            for j, (source, coefs) in enumerate(sources_of(f)):
                part = rects if source == sources_of(f)[0][0] else rects[j::5]
                for pt in (RGB8888, GRAY8):
                    some = part if pt == RGB8888 else (part[1::3] or part[:1])
                    if not some:
                        continue
                    got, info, twin_out = run(sim, f, source, pt, s, some, coefs=coefs, twin=source != 2)
                    for rect, g in zip(some, got):
                        assert np.array_equal(g, Q.crop(f, s, rect, pt == GRAY8)), (sampling, s, source, pt, rect)
                    if source != 2 and not (narrow and s == 1):          # the C row-major twin of the whole image, cropped
                        bpp = 4 if pt == RGB8888 else 1
                        assert np.array_equal(twin_out, X.rgba(Q.reference(f, s), pt == GRAY8))
                        x, y, rw, rh = some[0]
                        assert np.array_equal(got[0], twin_out[y:y + rh, x * bpp:(x + rw) * bpp])
                    ran += len(some)
    assert ran > 3000


@pytest.mark.parametrize("sampling", ("4:2:0", "4:2:2"))
def test_lanes_over_a_narrow_plane(sim, sampling):
    """a file 4 pixels wide: own width 2, replicated at full size -- every rectangle of it is Pillow's crop"""
    f = X.pillow_file(4, 24, sampling, 100, "baseline", "noise")
    assert len(f) >= 256
    assert X.in_window(Q.reference(f, 1)) and np.array_equal(Q.reference(f, 1)["rgb"], X.pillow(f, "RGB"))
    rects = [(x, y, rw, rh) for x in range(4) for rw in range(1, 5 - x) for y, rh in ((0, 24), (15, 1), (15, 2), (16, 3), (7, 10))]
    got, info, _ = run(sim, f, 2, RGB8888, 1, rects)
    for rect, g in zip(rects, got):
        assert np.array_equal(g, Q.crop(f, 1, rect)), rect
        assert np.array_equal(g.reshape(rect[3], rect[2], 4)[..., :3], Q.pillow_crop(f, 1, rect)), rect


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_a_rectangle_equal_to_the_image_is_the_whole_decode(sim, sampling):
    f = Q.fixture(sampling)
    hs, vs = coef_jpeg.LUMA_HV[sampling]
    mx, my = -(-333 // (8 * hs)), -(-217 // (8 * vs))
    for s in SCALES:
        sw, sh = S.scaled_size(333, 217, s)
        for pt in (RGB8888, GRAY8):
            got, info, _ = run(sim, f, 2, pt, s, [(0, 0, sw, sh)])
            assert np.array_equal(got[0], S.rgba(S.twin_scaled(f, s), pt == GRAY8))
            assert info[0] == my * -(-mx // Q.PER_TILE[sampling])         # every planes tile of the whole image
            assert info[1] == -(-sh // 32) * -(-(-(-sw // 4)) // 64)           # colour tile records: 64 quads x 32 rows each


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_clipped_surfaces(sim, sampling):
    f = Q.fixture(sampling)
    for s in (1, 4):
        rect = (7, 5, 70 // s + 3, 40 // s + 2)
        rw, rh = rect[2:]
        clips = [(rw - 1, rh), (rw, rh - 1), (0, rh), (rw, 0), (rw + 5, rh + 5), (1, 1), (4, 2), (5, rh), (rw - 4, 1), (rw - 3, 17)]
        for pt in (RGB8888, GRAY8):
            got, info, _ = run(sim, f, 2, pt, s, [rect] * len(clips), clips=clips)
            for clip, g in zip(clips, got):
                assert np.array_equal(g, Q.crop(f, s, rect, pt == GRAY8, clip)), (s, clip, pt)


def test_sanitizer_program(tmp_path):
    """the plan and the lanes as a program of their own under ASan + UBSan (nothing is loaded into this process)"""
    subprocess.run(["make", "exactrectasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    paths = []
    for k, sampling in enumerate(coef_jpeg.LAYOUTS):
        paths.append(str(tmp_path / ("f%d.jpg" % k)))
        with open(paths[-1], "wb") as fh:
            fh.write(Q.fixture(sampling) if k % 2 == 0 else [f for name, f, wh in S.grid(sampling) if wh == (75, 53)][-1])
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "exact_rect_asan")] + paths, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "exact_rect_asan ok" in r.stdout, r.stdout[-4000:]


def test_exports_and_argument_errors():
    import inspect
    import jpegdec_amd as J
    for name in ("exact_rect_mcus", "resize_reads", "exact_decode", "decode_to_host_exact"):
        assert callable(getattr(J, name)), name
    assert "rects" in inspect.signature(J.exact_decode).parameters and "rect" in inspect.signature(J.decode_to_host_exact).parameters
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    for fn in ("jda_exact_decode_surfaces_rect", "jda_exact_rect_mcus", "jda_decode_to_host_exact_rect", "jda_resize_reads"):
        assert "int %s(" % fn in hdr and hasattr(J.load_library(), fn), fn
    # the rectangle the taps read: the crop widened by the filter's support, clipped at the image
    x0, y0, x1, y1 = J.resize_reads((100, 80), (10, 10, 40, 40), (40, 40), J.binding.resize_filter("bilinear"))
    assert 9 <= x0 <= 10 and 9 <= y0 <= 10 and 50 <= x1 <= 51 and 50 <= y1 <= 51      # (at most the triangle's zero-weight neighbour)
    x0, y0, x1, y1 = J.resize_reads((100, 80), (10, 10, 40, 40), (20, 20), J.binding.resize_filter("bicubic"))
    assert 0 <= x0 < 10 and 0 <= y0 < 10 and 50 < x1 <= 100 and 50 < y1 <= 80
    assert J.resize_reads((100, 80), (0, 0, 100, 80), (10, 8), J.binding.resize_filter("lanczos")) == (0, 0, 100, 80)
    with pytest.raises(J.JdaError):
        J.resize_reads((100, 80), (90, 0, 20, 10), (4, 4))
    with pytest.raises(ValueError):                                     # draft= with crops= stays refused
        J.decode_to_tensors(None, [], decoder="libjpeg", draft=True, size=(8, 8), crops=[])
