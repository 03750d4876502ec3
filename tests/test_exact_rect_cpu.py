"""The libjpeg-exact decode of a pixel rectangle on the CPU: the definition against Pillow's crop, the plan against an
independent read set, and the kernels' lanes against the definition.
(a) the numpy reference (tests/exact_rect_util.py: the whole-image twins, cropped, with libjpeg's narrow-plane rule) = Pillow's
    Image.open(f).crop(box), draft() in front for 1/2, 1/4, 1/8, every file asserted inside the comparison window;
(b) jda_exact_rect_plan = the smallest MCU rectangle holding the read set derived pixel by pixel from the upsampling formulas, for every
    rectangle of the set, with and without chroma, the narrow-plane rule at own widths 1, 2, 3, every refusal;
(c) the existing planes lanes over the rectangle's tile list into a poisoned scratch, then the new colour lanes (tests/hostsim/
    exact_rect_sim.cpp): every load inside its allocation and of a plane byte this rectangle's planes stage stored, every byte of the clip
    stored exactly once and none outside = the reference = the C row-major twin's crop, for dense, sparse and baseline sources;
(d) a rectangle equal to the image = the whole decode; (e) clipped surfaces; (f) the same as a program under ASan + UBSan;
(g) the plan of a whole call (jda_exact_plan_build / _place) over a mixed batch of header numbers: the launch list in its order, the
    shared planes lists of a call without flags and rectangles, coverage, the blob's layout, calls with nothing to launch."""
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


# ---- the plan of a whole call (jda_exact_plan_build / _place of jda_exact_plan.h), from header numbers alone
MODES = ("gray", "4:4:4", "4:2:0", "4:2:2", "4:4:0")                   # JDA_MODE_*
MCU_PX = {"gray": (8, 8), "4:4:4": (8, 8), "4:2:0": (16, 16), "4:2:2": (16, 8), "4:4:0": (8, 16)}
DENSE, SPARSE, BASELINE, COLOUR, COLOUR_RGB, COLOUR4, COLOUR_RECT, COLOUR_RECT_RGB = range(8)      # jda_exact_kind
CS_GRAY, CS_YCBCR, CS_RGB, CS_CMYK = 0, 1, 2, 3                         # JDA_CS_*
COLOUR_MODELS = 1                                                       # JDA_EXACT_COLOUR_MODELS
STRIP = np.dtype([("image", "<u4"), ("mcu_y", "<u2"), ("mcu_x0", "<u2"), ("count", "u1"), ("first", "u1"), ("pad", "<u2"), ("ord", "<u4")])
DESC_BYTES, EX_BYTES, SRC_BYTES, RECT_BYTES = 104, 480, 72, 16


def plan_image(sampling, source, scale=1, colour=None, ncomp=None, pt=RGB8888, rect=(0, 0, 0, 0)):
    """an image one MCU wider than a tile and two MCU rows high, no multiple of the MCU either way (a full and a partial tile a row)"""
    mw, mh = MCU_PX[sampling]
    w, h = (Q.PER_TILE[sampling] + 1) * mw - 3, 2 * mh - 5
    sub, nc = Q.SUB[sampling]
    nc = ncomp or nc
    colour = colour if colour is not None else (CS_GRAY if nc == 1 else CS_YCBCR)
    sw, sh = (-(-w // scale), -(-h // scale)) if scale in SCALES else (w, h)
    if any(rect):
        sw, sh = rect[2], rect[3]
    return dict(sampling=sampling, source=source, scale=scale, colour=colour, ncomp=nc, w=w, h=h, rect=rect,
                hdr=[w, h, nc, sub, source, colour, pt, scale, *rect, sw, sh])


def mixed_batch():
    return [plan_image("gray", DENSE), plan_image("4:4:4", SPARSE, 2), plan_image("4:2:0", BASELINE), plan_image("4:2:2", DENSE, 8),
            plan_image("4:2:0", BASELINE, 3),                           # refused: no such scale
            plan_image("4:4:0", BASELINE), plan_image("4:2:0", DENSE, rect=(21, 3, 97, 20)), plan_image("4:4:4", SPARSE, 2, colour=CS_RGB),
            plan_image("4:4:4", DENSE, colour=CS_CMYK, ncomp=4), plan_image("4:2:0", SPARSE)]


def call_plan(sim, images, flags, with_rects):
    n = len(images)
    sim.exactrectsim_call_plan.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_int] + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    sim.exactrectsim_tiles_per_wg.argtypes = [C.c_int]
    hdr = np.array([im["hdr"] for im in images], np.int32).reshape(n, 14)
    status = np.full(max(n, 1), 99, np.int32)
    launches, n_launches = np.zeros((160, 5), np.int64), C.c_int32(-1)
    blob, layout, image = np.zeros(1 << 20, np.uint8), np.zeros(10, np.int64), np.zeros((max(n, 1), 10), np.int64)
    rc = sim.exactrectsim_call_plan(n, hdr.ctypes.data, flags, with_rects, status.ctypes.data, launches.ctypes.data, 160, C.byref(n_launches), blob.ctypes.data, blob.size,
                                    layout.ctypes.data, image.ctypes.data)
    keys = ("blob", "o_ex", "o_src", "o_rect", "o_scratch", "scratch", "colour_begin", "n_rec", "n_planned", "block")
    lay = dict(zip(keys, (int(v) for v in layout)))
    L = [tuple(int(v) for v in row) for row in launches[:n_launches.value]]
    return rc, list(status[:n]), L, blob[:lay["blob"]], lay, image[:n]


def tiles_of(blob, launch):
    kind, mode, scale, off, count = launch
    return blob[off:off + 16 * count].view(STRIP)


def padded(sim, im, mcus=None):
    """records an image adds to a planes / colour list of its layout: a tile a run of PER_TILE MCUs a row, padded to whole workgroups"""
    per, wg = Q.PER_TILE[im["sampling"]], sim.exactrectsim_tiles_per_wg(MODES.index(im["sampling"]))
    mw, mh = MCU_PX[im["sampling"]]
    x0, y0, x1, y1 = mcus or (0, 0, -(-im["w"] // mw), -(-im["h"] // mh))
    t = (y1 - y0) * -(-(x1 - x0) // per)
    return -(-t // wg) * wg, t


def test_call_plan_of_a_mixed_batch(sim):
    B = mixed_batch()
    n = len(B)
    rc, status, L, blob, lay, image = call_plan(sim, B, COLOUR_MODELS, 1)
    assert rc == 0 and status == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0] and lay["n_planned"] == 9 and lay["n_rec"] == 2 * n
    assert 15 <= sim.exactrectsim_tiles_per_wg(2) <= 16 and sim.exactrectsim_tiles_per_wg(0) == 15
    P = lambda i, mcus=None: padded(sim, B[i], mcus)[0]
    mcu6 = tuple(int(v) for v in image[6][4:8])
    assert mcu6 == plan(sim, B[6]["w"], B[6]["h"], "4:2:0", RGB8888, 1, B[6]["rect"])[1] == Q.mcu_rect(B[6]["w"], B[6]["h"], "4:2:0", 1, B[6]["rect"])
    k_gray = dict(B[8], sampling="gray")                               # component 3 of the four-component image: a gray image over its blocks
    rect_tiles = -(-(-(-20 // 32) * -(-(-(-97 // 4)) // 64)) // 4) * 4     # 64 quads x 32 rows a record, padded to the 4 of a workgroup
    # all planes launches by (layout, scale, source); then colour: own lists by (layout, scale, YCbCr | RGB), four-component by layout, rectangles
    want = [(DENSE, 0, 1, P(0) + padded(sim, k_gray)[0]), (DENSE, 1, 1, P(8)), (SPARSE, 1, 2, P(1) + P(7)),
            (DENSE, 2, 1, P(6, mcu6)), (SPARSE, 2, 1, P(9)), (BASELINE, 2, 1, P(2)), (DENSE, 3, 8, P(3)), (BASELINE, 4, 1, P(5)),
            (COLOUR, 0, 1, P(0)), (COLOUR, 1, 2, P(1)), (COLOUR_RGB, 1, 2, P(7)), (COLOUR, 2, 1, P(2) + P(9)), (COLOUR, 3, 8, P(3)), (COLOUR, 4, 1, P(5)),
            (COLOUR4, 1, 1, P(8)), (COLOUR_RECT, 2, 1, rect_tiles)]
    assert [(k, m, s, c) for k, m, s, off, c in L] == want
    assert lay["colour_begin"] == 8
    assert any(c % 4 for k, m, s, off, c in L)                          # (list lengths that are no multiple of a workgroup's 4 wavefronts)
    # coverage: every MCU of every planned image (a rectangle image: of its MCU rectangle) in the planes lists exactly once
    seen = {}
    for launch in L[:lay["colour_begin"]]:
        for t in tiles_of(blob, launch):
            for x in range(int(t["mcu_x0"]), int(t["mcu_x0"]) + int(t["count"])):
                key = (int(t["image"]), x, int(t["mcu_y"]))
                assert key not in seen, key
                seen[key] = launch[:3]
    want_mcus = set()
    for i, im in enumerate(B):
        if status[i]:
            continue
        mw, mh = MCU_PX[im["sampling"]]
        x0, y0, x1, y1 = mcu6 if i == 6 else (0, 0, -(-im["w"] // mw), -(-im["h"] // mh))
        want_mcus |= {(i, x, y) for x in range(x0, x1) for y in range(y0, y1)}
        assert all(seen[(i, x, y)] == (im["source"], MODES.index(im["sampling"]), im["scale"]) for x in range(x0, x1) for y in range(y0, y1))
    k_mcus = {(n + 8, x, y) for x in range(-(-B[8]["w"] // 8)) for y in range(-(-B[8]["h"] // 8))}      # record n + i, in the gray dense list
    assert set(seen) == want_mcus | k_mcus and all(seen[k] == (DENSE, 0, 1) for k in k_mcus)
    # jda_exact_tile_count (what the one call reports) = the records of the image that hold MCUs, of its MCU rectangle and whole
    held = {}
    for launch in L[:lay["colour_begin"]]:
        for t in tiles_of(blob, launch):
            held[int(t["image"])] = held.get(int(t["image"]), 0) + (int(t["count"]) != 0)
    for i, im in enumerate(B):
        if not status[i]:
            assert (int(image[i][8]), int(image[i][9])) == (held[i], padded(sim, im)[1]) and (held[i] == padded(sim, im)[1]) == (i != 6)
    # .. and every planned image's output in exactly one colour-stage list: a whole image's MCUs there exactly once, tile by tile
    owner, cseen = {}, set()
    for launch in L[lay["colour_begin"]:-1]:
        for t in tiles_of(blob, launch):
            if t["count"]:
                assert owner.setdefault(int(t["image"]), launch[:3]) == launch[:3]
            for x in range(int(t["mcu_x0"]), int(t["mcu_x0"]) + int(t["count"])):
                key = (int(t["image"]), x, int(t["mcu_y"]))
                assert key not in cseen, key
                cseen.add(key)
    assert cseen == {k for k in want_mcus if k[0] != 6}                 # (K's gray tiles and the rectangle's MCUs are in no whole-image colour list)
    assert owner == {i: ((COLOUR4 if i == 8 else COLOUR_RGB if i == 7 else COLOUR), MODES.index(B[i]["sampling"]), B[i]["scale"]) for i in (0, 1, 2, 3, 5, 7, 8, 9)}
    rt = [t for t in tiles_of(blob, L[-1]) if t["count"]]
    assert sorted((int(t["mcu_x0"]), int(t["mcu_y"])) for t in rt) == [(0, 0)] and all(int(t["image"]) == 6 for t in rt)
    # the rectangle's record, and the refused image's records left zero
    assert list(blob[lay["o_rect"] + 6 * RECT_BYTES:][:RECT_BYTES].view("<u4")) == [21, 3, 97, 20]
    assert not blob[4 * DESC_BYTES:5 * DESC_BYTES].any() and not blob[lay["o_ex"] + 4 * EX_BYTES:lay["o_ex"] + 5 * EX_BYTES].any()
    check_layout(L, blob, lay, image, n, True, False)


def check_layout(L, blob, lay, image, n, with_rects, shared):
    """16-aligned parts one behind the other inside the blob, the scratch at a multiple of 256 behind it, the planes disjoint and all of it"""
    nrec = lay["n_rec"]
    assert lay["o_ex"] % 16 == 0 and lay["o_src"] % 16 == 0 and lay["o_ex"] >= nrec * DESC_BYTES and lay["o_src"] >= lay["o_ex"] + nrec * EX_BYTES
    spans = sorted((off, off + 16 * c) for k, m, s, off, c in L if k <= BASELINE or not shared)      # (shared: the colour launches walk the planes lists)
    assert spans[0][0] >= lay["o_src"] + nrec * SRC_BYTES and spans[0][0] % 16 == 0
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0 and b0 % 16 == 0
    assert spans[-1][1] <= lay["o_rect"] and lay["o_rect"] + (n * RECT_BYTES if with_rects else 0) == lay["blob"] == blob.size
    assert lay["o_scratch"] % 256 == 0 and lay["blob"] <= lay["o_scratch"] < lay["blob"] + 256 and lay["block"] % 16 == 0
    at = 0
    for q in image:
        if q[0] < 0:
            continue
        assert q[1] == at and q[2] > 0 and q[2] % 256 == 0               # the planes one behind the other, each a multiple of 256
        at += int(q[2])
    assert at == lay["scratch"]
    for i, q in enumerate(image):                                       # the record's Y plane: where the plan says, inside the block
        if q[0] >= 0:
            assert int(blob[lay["o_ex"] + i * EX_BYTES:][:8].view("<u8")[0]) == lay["block"] + int(q[3]) and q[3] == lay["o_scratch"] + q[1]


def test_call_plan_shares_the_planes_lists_without_flags_and_rectangles(sim):
    B = [im for i, im in enumerate(mixed_batch()) if i not in (6, 7, 8)]
    n = len(B)
    rc, status, L, blob, lay, image = call_plan(sim, B, 0, 0)
    assert rc == 0 and status == [0, 0, 0, 0, 1, 0, 0] and lay["n_rec"] == n
    P = lambda i: padded(sim, B[i])[0]
    want = [(DENSE, 0, 1, P(0)), (SPARSE, 1, 2, P(1)), (SPARSE, 2, 1, P(6)), (BASELINE, 2, 1, P(2)), (DENSE, 3, 8, P(3)), (BASELINE, 4, 1, P(5)),
            (COLOUR, 0, 1, P(0)), (COLOUR, 1, 2, P(1)), (COLOUR, 2, 1, P(6) + P(2)), (COLOUR, 3, 8, P(3)), (COLOUR, 4, 1, P(5))]
    assert [(k, m, s, c) for k, m, s, off, c in L] == want and lay["colour_begin"] == 6
    planes = L[:6]
    for k, m, s, off, c in L[6:]:                                       # one colour launch a (layout, scale): from its dense list, over all three
        group = [p for p in planes if p[1:3] == (m, s)]
        assert off == min(p[3] for p in group) and c == sum(p[4] for p in group)
        assert [p[3] for p in group] == [off + 16 * sum(q[4] for q in group[:j]) for j in range(len(group))]      # (dense | sparse | baseline, back to back)
    assert max(off + 16 * c for k, m, s, off, c in planes) == lay["o_rect"] == lay["blob"]      # no list of the colour stage's own, no rectangle records
    check_layout(L, blob, lay, image, n, False, True)


def test_call_plan_with_nothing_to_launch(sim):
    rc, status, L, blob, lay, image = call_plan(sim, [], COLOUR_MODELS, 1)
    assert rc == 0 and L == [] and lay["blob"] == 0 and lay["n_planned"] == 0
    # every image refused: a scale that is none, a pixel type the road lacks, an RGB-coded file to a gray surface
    B = [plan_image("4:2:0", BASELINE, 3), plan_image("gray", DENSE, pt=0), plan_image("4:4:4", SPARSE, 2, colour=CS_RGB, pt=GRAY8)]
    rc, status, L, blob, lay, image = call_plan(sim, B, COLOUR_MODELS, 0)
    assert rc == 0 and status == [1, 1, 3] and L == [] and lay["n_planned"] == 0 and lay["scratch"] == 0 and lay["blob"] == 0


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
