"""The libjpeg-exact decode of a pixel rectangle on the GPU (jda_exact_decode_surfaces_rect, jda_decode_to_host_exact_rect,
decode_to_tensors(decoder="libjpeg", crops=)) against the numpy reference (tests/exact_rect_util.py), which
tests/test_exact_rect_cpu.py holds to Pillow's crop:
(a) per layout the whole rectangle set of the 333 x 217 file and of the small files at scales 1, 2, 4, 8 as entries of ONE call -- host-index,
    device-index, dense and sparse sources interleaved -- into guard-filled back-to-back surfaces: pixels = reference, the guard intact
    everywhere else, the launches counted per kernel instance (the planes launches present and ONE jda_exact_colour_rect), twice; RGB8888
    and gray; (b) whole images and rectangles mixed in one call; (c) RGB-coded files; (d) clipped surfaces; (e) the one call;
(f) refusals, and calls that launch nothing; (g) decode_to_tensors with crops= against Pillow's resize(box=); (h) a mixed batch -- every
    layout, source kind, colour model, three scales, a rectangle and a refused image -- in one call, each surface against its reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

import jpegdec_amd as J
from tests import coef_jpeg
from tests import exact_adobe_util as A
from tests import exact_rect_util as Q
from tests import exact_scaled_util as S
from tests import exact_util as X
from tests.test_gpu_exact import FILL, MODE, Sources

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUCCESS, INVALID_PARAMETER, DECODE_ERROR, UNSUPPORTED = 0, 1, 2, 3
LOAD = {"dense": 0, "sparse": 1, "host": 2, "device": 2}
COLOUR_LAYOUTS = ("4:4:4", "4:2:0", "4:2:2", "4:4:0")


def counts():
    c = J.kernel_launch_counts()
    out = {}
    for m in range(5):
        for f in range(3):
            out["planes", m, f, 1] = sum(v for k, v in c.items() if "jda_exact_planesILi%dELi%dE" % (m, f) in k)
            for s in (2, 4, 8):
                out["planes", m, f, s] = sum(v for k, v in c.items() if "jda_exact_planes_scaledILi%dELi%dELi%dE" % (m, f, s) in k)
        for name in ("colour", "colour_scaled", "colour_rgb", "colour_scaled_rgb", "colour4"):
            out[name, m] = sum(v for k, v in c.items() if "jda_exact_%sILi%dE" % (name, m) in k)
        for rgb in (0, 1):
            out["colour_rect", m, rgb] = sum(v for k, v in c.items() if "jda_exact_colour_rectILi%dELb%dE" % (m, rgb) in k)
    return out


def delta(before):
    after = counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def decode_into_guard(ctx, sources, rects, pixel_types, scales=None, clips=None, colour_models=False, shapes=None):
    """ONE jda_exact_decode_surfaces_rect call into back-to-back surfaces in a guard-filled allocation -> (statuses, [surface rows x pitch], the
    bytes between and behind the surfaces).  A surface holds its rectangle (shapes: the (w, h) of the entries whose rectangle is all zero);
    clips: (width_px, rows) each, default the surface's own"""
    dims = [(r[2], r[3]) if r is not None and any(r) and r[2] > 0 and r[3] > 0 else shapes[k] for k, r in enumerate(rects)]
    bpp = [4 if pt == J.RGB8888 else 1 for pt in pixel_types]
    pitch = [max(16, (w * b + 15) & ~15) for (w, h), b in zip(dims, bpp)]
    offs, total = [], 256
    for (w, h), p in zip(dims, pitch):
        offs.append(total)
        total += ((p * h + 255) & ~255) + 256
    base = ctx.malloc(total)
    try:
        ctx.memset(base, FILL, total)
        clips = clips or dims
        status = J.exact_decode(ctx, sources, [(base + o, p, cw, cr) for o, p, (cw, cr) in zip(offs, pitch, clips)], pixel_types, scales, colour_models, rects=rects)
        raw = ctx.to_host(base, total)
    finally:
        ctx.free(base)
    surfaces, rest = [], np.ones(total, dtype=bool)
    for o, p, (w, h) in zip(offs, pitch, dims):
        surfaces.append(raw[o:o + p * h].reshape(h, p))
        rest[o:o + p * h] = False
    return status, surfaces, raw[rest]


def check_surface(surface, want, what):
    h, wb = want.shape
    assert np.array_equal(surface[:h, :wb], want), (what, int(np.count_nonzero(surface[:h, :wb] != want)))
    assert np.all(surface[:h, wb:] == FILL) and np.all(surface[h:] == FILL), (what, "bytes outside the rectangle's pixels")


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_rectangle_set_in_one_call(gpu_ctx, sampling):
    files = [Q.fixture(sampling)] + [f for f, wh in Q.small_files(sampling)]
    sizes = [(333, 217)] + [wh for f, wh in Q.small_files(sampling)]
    S1 = Sources(gpu_ctx, files)
    try:
        assert {"host", "device", "dense", "sparse"} <= set(S1.kind)
        by_file = {i: [k for k, fo in enumerate(S1.file_of) if fo == i] for i in range(len(files))}
        items, file_of, kind, scales, rects = [], [], [], [], []
        for i, (w, h) in enumerate(sizes):
            for s in S.SCALES:
                sw, sh = S.scaled_size(w, h, s)
                for j, rect in enumerate(Q.rect_set(sw, sh, sampling, s)):
                    k = by_file[i][(j + s) % len(by_file[i])]
                    items.append(S1.items[k])
                    file_of.append(i)
                    kind.append(S1.kind[k])
                    scales.append(s)
                    rects.append(rect)
        n = len(items)
        assert n > 3000
        m = MODE[sampling]
        present = {(LOAD[kd], s) for kd, s in zip(kind, scales)}
        assert present == {(f, s) for f in range(3) for s in S.SCALES}
        want_launches = {("planes", m, f, s): 1 for f, s in present}
        want_launches[("colour_rect", m, 0)] = 1
        for gray in (False, True):
            pts = [J.GRAY8 if gray else J.RGB8888] * n
            wants = [Q.crop(files[i], s, r, gray) for i, s, r in zip(file_of, scales, rects)]
            for again in range(2):
                before = counts()
                status, surfaces, rest = decode_into_guard(gpu_ctx, items, rects, pts, scales)
                assert delta(before) == want_launches
                assert status == [SUCCESS] * n
                assert np.all(rest == FILL)
                for k in range(n):
                    check_surface(surfaces[k], wants[k], (sampling, kind[k], scales[k], rects[k], "gray" if gray else "rgba"))
    finally:
        S1.close()


@pytest.mark.parametrize("sampling", ("gray", "4:2:0", "4:2:2"))
def test_whole_images_and_rectangles_in_one_call(gpu_ctx, sampling):
    """an all-zero rectangle is that image whole, byte-equal to jda_exact_decode_surfaces_ex of it, through that call's colour kernels"""
    f = Q.fixture(sampling)
    S1 = Sources(gpu_ctx, [f])
    try:
        n = 8
        items = [S1.items[k % 4] for k in range(n)]
        scales = [1, 1, 2, 4, 8, 2, 1, 8]
        rects = [None, (5, 3, 100, 50), (0, 0, 0, 0), (9, 1, 30, 40), None, (1, 2, 3, 4), (3, 0, 330, 217), (0, 0, 0, 0)]
        shapes = [S.scaled_size(333, 217, s) for s in scales]
        m = MODE[sampling]
        for cm in (False, True):
            before = counts()
            status, surfaces, rest = decode_into_guard(gpu_ctx, items, rects, [J.RGB8888] * n, scales, colour_models=cm, shapes=shapes)
            d = delta(before)
            assert status == [SUCCESS] * n and np.all(rest == FILL)
            assert d[("colour_rect", m, 0)] == 1 and d[("colour", m)] == 1 and d[("colour_scaled", m)] == 2 and not any(k[0] in ("colour_rgb", "colour4") for k in d)
            whole = [k for k in range(n) if rects[k] is None or not any(rects[k])]
            from tests.test_gpu_exact_adobe import decode_into_guard as ex_call
            st2, sf2, rest2 = ex_call(gpu_ctx, [items[k] for k in whole], [shapes[k] for k in whole], [J.RGB8888] * len(whole), [scales[k] for k in whole], colour_models=True)
            assert st2 == [SUCCESS] * len(whole)
            for a, k in zip(sf2, whole):
                assert np.array_equal(a[:, :shapes[k][0] * 4], surfaces[k][:, :shapes[k][0] * 4]), k
                check_surface(surfaces[k], S.rgba(S.twin_scaled(f, scales[k])), ("whole", k))
            for k in range(n):
                if k not in whole:
                    check_surface(surfaces[k], Q.crop(f, scales[k], rects[k]), ("rect", k))
    finally:
        S1.close()


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_rgb_coded_files(gpu_ctx, sampling):
    """rectangles of RGB-coded files (JDA_EXACT_COLOUR_MODELS) beside YCbCr ones: a jda_exact_colour_rect launch each"""
    rgb3, ycc = A.pillow_rgb3(75, 53, sampling, 90, "ids"), A.pillow_rgb3(75, 53, sampling, 90, "none")
    assert A.model(rgb3) == A.RGB and A.model(ycc) == A.YCBCR
    Sr = Sources(gpu_ctx, [rgb3, ycc], only=("host", "dense", "sparse"))
    try:
        items, file_of, scales, rects = [], [], [], []
        for s in S.SCALES:
            sw, sh = S.scaled_size(75, 53, s)
            for j, rect in enumerate(Q.rect_set(sw, sh, sampling, s)[::7] + [(0, 0, sw, sh)]):
                k = (j + s) % len(Sr.items)
                items.append(Sr.items[k])
                file_of.append(Sr.file_of[k])
                scales.append(s)
                rects.append(rect)
        n = len(items)
        before = counts()
        status, surfaces, rest = decode_into_guard(gpu_ctx, items, rects, [J.RGB8888] * n, scales, colour_models=True)
        d = delta(before)
        m = MODE[sampling]
        assert d[("colour_rect", m, 0)] == 1 and d[("colour_rect", m, 1)] == 1 and all(k[0] in ("planes", "colour_rect") for k in d), d
        assert status == [SUCCESS] * n and np.all(rest == FILL)
        files = (rgb3, ycc)
        for k in range(n):
            x, y, w, h = rects[k]
            want = A.surface(A.twin3(files[file_of[k]], scales[k]))[y:y + h, 4 * x:4 * (x + w)]
            check_surface(surfaces[k], want, (sampling, file_of[k], scales[k], rects[k]))
    finally:
        Sr.close()


@pytest.mark.parametrize("sampling", ("gray", "4:2:0", "4:4:0"))
def test_clipped_surfaces(gpu_ctx, sampling):
    f = Q.fixture(sampling)
    S1 = Sources(gpu_ctx, [f], only=("host", "sparse"))
    try:
        for s in (1, 2, 8):
            rect = (7, 5, 70 // s + 3, 40 // s + 2)
            rw, rh = rect[2:]
            clips = [(rw - 1, rh), (rw, rh - 1), (0, rh), (rw, 0), (rw + 5, rh + 5), (1, 1), (4, 2), (5, rh), (rw - 4, 1), (rw - 3, 17)]
            n = len(clips)
            for pt in (J.RGB8888, J.GRAY8):
                status, surfaces, rest = decode_into_guard(gpu_ctx, [S1.items[k % 2] for k in range(n)], [rect] * n, [pt] * n, [s] * n, clips)
                assert status == [SUCCESS] * n and np.all(rest == FILL)
                for sf, clip in zip(surfaces, clips):
                    want = Q.crop(f, s, rect, pt == J.GRAY8, clip)
                    if want.size:
                        check_surface(sf, want, (s, clip, pt))
                    else:
                        assert np.all(sf == FILL), (s, clip, pt)
    finally:
        S1.close()


def test_decode_to_host_exact_rect(gpu_ctx):
    for sampling in coef_jpeg.LAYOUTS:
        f = Q.fixture(sampling)
        prog = [x for name, x, wh in S.grid(sampling) if wh[0] >= 40 and wh[1] >= 30 and name.startswith("progressive")]
        for s, rect in ((1, (33, 18, 50, 41)), (2, (3, 7, 21, 30)), (8, (1, 1, 9, 5))):
            for pt in (J.RGB8888, J.GRAY8):
                rc, got, tiles = J.decode_to_host_exact(gpu_ctx, f, pt, s, rect=rect)
                assert rc == 0, (sampling, s, pt)
                got = got.reshape(got.shape[0], -1)
                assert np.array_equal(got, Q.crop(f, s, rect, pt == J.GRAY8)), (sampling, s, pt)
                mx0, my0, mx1, my1 = J.exact_rect_mcus(f, rect, s, pt)
                assert (mx0, my0, mx1, my1) == Q.mcu_rect(333, 217, sampling, s, rect, pt == J.GRAY8)
                assert tiles[0] == (my1 - my0) * -(-(mx1 - mx0) // Q.PER_TILE[sampling]) and 0 < tiles[0] < tiles[1]
            if prog and s <= 2:                                         # a progressive file: a coefficient image behind the same call
                r2 = (rect[0] // 2, rect[1] // 2, 17, 11)
                rc, got, tiles = J.decode_to_host_exact(gpu_ctx, prog[0], J.RGB8888, s, rect=r2)
                assert rc == 0 and np.array_equal(got.reshape(11, -1), Q.crop(prog[0], s, r2)) and tiles[0] <= tiles[1]
    # a guard-filled host array with a pitch of its own: nothing outside w x h pixels is written
    f = Q.fixture("4:2:0")
    host = np.full((30, 200), FILL, np.uint8)
    tiles = (J.binding.C.c_int32 * 2)()
    rc = gpu_ctx.lib.jda_decode_to_host_exact_rect(gpu_ctx.handle, f, len(f), J.RGB8888, 1, 0, (J.binding.C.c_int32 * 4)(11, 13, 37, 25), host.ctypes.data_as(J.binding.C.c_void_p),
                                                   200, 25, tiles)
    assert rc == 0 and np.array_equal(host[:25, :148], Q.crop(f, 1, (11, 13, 37, 25))) and np.all(host[:, 148:] == FILL) and np.all(host[25:] == FILL)
    before = counts()
    for bad in ((330, 0, 4, 4), (0, 0, 4, 0), (-1, 0, 4, 4), (0, 215, 1, 3)):
        rc, got, tiles = J.decode_to_host_exact(gpu_ctx, f, rect=bad)
        assert rc == INVALID_PARAMETER and not got.any(), bad
    rc = gpu_ctx.lib.jda_decode_to_host_exact_rect(gpu_ctx.handle, f, len(f), J.RGB8888, 1, 0, (J.binding.C.c_int32 * 4)(0, 0, 40, 4), host.ctypes.data_as(J.binding.C.c_void_p), 159, 4, None)
    assert rc == INVALID_PARAMETER                                      # a pitch below the rectangle's bytes
    cmyk = A.grid4("4:2:0")[0][1]
    rc, got, tiles = J.decode_to_host_exact(gpu_ctx, cmyk, colour_models=True, rect=(0, 0, 1, 1))
    assert rc == UNSUPPORTED and not got.any()
    assert delta(before) == {}


def test_refusals_and_calls_that_launch_nothing(gpu_ctx):
    f = Q.fixture("4:2:0")
    S1 = Sources(gpu_ctx, [f], only=("host", "dense"))
    cmyk = A.grid4("4:2:0")[0][1]
    host4 = J.CoefImage.from_file(cmyk)
    dev4 = J.DeviceCoef(gpu_ctx, host4, J.COEF_AUTO)
    try:
        bad = [(333, 0, 1, 1), (0, 217, 1, 1), (330, 0, 4, 1), (0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, -3, 5), (0, 0, 334, 217), (100, 216, 2, 2)]
        n = len(bad)
        pitch, size = 1344, 1344 * 217 + 256
        base = gpu_ctx.malloc(size * (n + 1))
        try:
            gpu_ctx.memset(base, FILL, size * (n + 1))
            outs = [(base + size * k, pitch, 333, 217) for k in range(n + 1)]
            before = counts()
            items = [S1.items[k % 2] for k in range(n)]
            assert J.exact_decode(gpu_ctx, items, outs[:n], None, None, rects=bad) == [INVALID_PARAMETER] * n
            assert J.exact_decode(gpu_ctx, items[:4], outs[:4], None, [2, 4, 8, 8], rects=[(167, 0, 1, 1), (0, 55, 1, 1), (40, 0, 3, 1), (0, 0, 42, 29)]) == [INVALID_PARAMETER] * 4
            # a four-component source with a rectangle; whole (an all-zero rectangle) it is taken as ever
            assert J.exact_decode(gpu_ctx, [dev4], outs[:1], None, None, True, rects=[(0, 0, 4, 4)]) == [UNSUPPORTED]
            # everything the _ex call refuses stays refused: a scale, a pixel type, a misaligned surface
            assert J.exact_decode(gpu_ctx, items[:1], outs[:1], None, [3], rects=[(0, 0, 4, 4)]) == [INVALID_PARAMETER]
            assert J.exact_decode(gpu_ctx, items[:1], outs[:1], [J.RGB565_LE], None, rects=[(0, 0, 4, 4)]) == [INVALID_PARAMETER]
            assert J.exact_decode(gpu_ctx, items[:1], [(base + 4, pitch, 333, 217)], None, None, rects=[(0, 0, 4, 4)]) == [INVALID_PARAMETER]
            assert J.exact_decode(gpu_ctx, items[:1], [(base, 16, 333, 217)], None, None, rects=[(0, 0, 8, 4)]) == [INVALID_PARAMETER]      # a pitch below the rectangle's bytes
            assert J.exact_decode(gpu_ctx, [], [], None, None, rects=[]) == []
            lib = gpu_ctx.lib
            assert lib.jda_exact_decode_surfaces_rect(gpu_ctx.handle, 1, None, None, None, None, 0, None, None) == INVALID_PARAMETER
            assert lib.jda_exact_decode_surfaces_rect(gpu_ctx.handle, 1, None, None, None, None, 2, None, None) == INVALID_PARAMETER
            assert lib.jda_exact_decode_surfaces_rect(None, 1, None, None, None, None, 0, None, None) == 6
            assert delta(before) == {}
            assert np.all(gpu_ctx.to_host(base, size * (n + 1)) == FILL)
            # a pitch that holds the rectangle alone is enough; refused and decoded entries mix
            small = (base, 48, 333, 217)
            status = J.exact_decode(gpu_ctx, items[:3] + [dev4], [small, outs[1], outs[2], outs[3]], None, None, True,
                                    rects=[(321, 200, 12, 17), (333, 0, 1, 1), (0, 0, 0, 0), (0, 0, 0, 0)])
            assert status == [SUCCESS, INVALID_PARAMETER, SUCCESS, SUCCESS]
            raw = gpu_ctx.to_host(base, size * 4)
            assert np.array_equal(raw[:48 * 17].reshape(17, 48), Q.crop(f, 1, (321, 200, 12, 17))) and np.all(raw[48 * 17:size] == FILL)
            assert np.all(raw[size:2 * size] == FILL)
            assert np.array_equal(raw[2 * size:2 * size + pitch * 217].reshape(217, pitch)[:, :1332], X.rgba(X.twin(f)))
        finally:
            gpu_ctx.free(base)
    finally:
        dev4.close()
        host4.close()
        S1.close()


def test_mixed_batch_in_one_call(gpu_ctx):
    """the batch whose plan tests/test_exact_rect_cpu.py takes apart, as real files in ONE jda_exact_decode_surfaces_rect call with
    JDA_EXACT_COLOUR_MODELS: every layout, dense, sparse and baseline sources, scales 1, 2 and 8, a rectangle, an RGB-coded and a
    four-component file, and in the middle an image that is refused -- every surface its reference, the refused one's untouched"""
    mcu = {"gray": (8, 8), "4:4:4": (8, 8), "4:2:0": (16, 16), "4:2:2": (16, 8), "4:4:0": (8, 16)}
    size = lambda sampling: ((Q.PER_TILE[sampling] + 1) * mcu[sampling][0] - 3, 2 * mcu[sampling][1] - 5)      # a full and a partial tile a row, two MCU rows
    ycc = {sampling: X.written_file(*size(sampling), sampling, 90) for sampling in coef_jpeg.LAYOUTS}
    rgb3, cmyk = A.pillow_rgb3(*size("4:4:4"), "4:4:4", 90, "ids"), A.pillow_cmyk(*size("4:4:4"), "4:4:4", 90)
    assert A.model(rgb3) == A.RGB and A.model(cmyk) == A.CMYK
    rect = (21, 3, 97, 20)
    # (file, resident form, scale, rectangle or None, the reference's surface)
    batch = [(ycc["gray"], "dense", 1, None, X.rgba(X.twin(ycc["gray"]))),
             (ycc["4:4:4"], "sparse", 2, None, S.rgba(S.twin_scaled(ycc["4:4:4"], 2))),
             (ycc["4:2:0"], "host", 1, None, X.rgba(X.twin(ycc["4:2:0"]))),
             (ycc["4:2:2"], "dense", 8, None, S.rgba(S.twin_scaled(ycc["4:2:2"], 8))),
             (ycc["4:2:0"], "host", 3, None, None),                     # refused: no such scale
             (ycc["4:4:0"], "host", 1, None, X.rgba(X.twin(ycc["4:4:0"]))),
             (ycc["4:2:0"], "dense", 1, rect, Q.crop(ycc["4:2:0"], 1, rect)),
             (rgb3, "sparse", 2, None, A.surface(A.twin3(rgb3, 2))),
             (cmyk, "dense", 1, None, A.surface(A.twin4(cmyk))),
             (ycc["4:2:0"], "sparse", 1, None, X.rgba(X.twin(ycc["4:2:0"])))]
    for f, s in ((ycc["gray"], 1), (ycc["4:4:4"], 2), (ycc["4:2:0"], 1), (ycc["4:2:2"], 8), (ycc["4:4:0"], 1)):
        assert X.in_window(X.twin(f) if s == 1 else S.twin_scaled(f, s))
    assert A.in_window(A.twin3(rgb3, 2)) and A.in_window(A.twin4(cmyk))
    keep, items = [], []
    try:
        for f, form, s, r, want in batch:
            if form == "host":
                p = J.PreparedImage(f)
                d = J.DeviceImage(gpu_ctx, p)
            else:
                p = J.CoefImage.from_file(f) if f is cmyk else J.CoefImage(f, X.natural_blocks(f))
                d = J.DeviceCoef(gpu_ctx, p, J.COEF_SPARSE if form == "sparse" else J.COEF_DENSE)
                assert d.form == (J.COEF_SPARSE if form == "sparse" else J.COEF_DENSE)
            keep.append(p)
            items.append(d)
        n = len(batch)
        sizes = dict([(ycc[sampling], size(sampling)) for sampling in coef_jpeg.LAYOUTS] + [(rgb3, size("4:4:4")), (cmyk, size("4:4:4"))])
        shapes = [S.scaled_size(*sizes[f], s) if s in S.SCALES else sizes[f] for f, form, s, r, want in batch]
        rects = [r for f, form, s, r, want in batch]
        before = counts()
        status, surfaces, rest = decode_into_guard(gpu_ctx, items, rects, [J.RGB8888] * n, [s for f, form, s, r, want in batch], colour_models=True, shapes=shapes)
        d = delta(before)
        assert status == [SUCCESS] * 4 + [INVALID_PARAMETER] + [SUCCESS] * 5
        assert np.all(rest == FILL) and np.all(surfaces[4] == FILL)
        for k, (f, form, s, r, want) in enumerate(batch):
            if want is not None:
                check_surface(surfaces[k], want, (k, form, s, r))
        # one launch a list of the plan: the planes by (layout, scale, source), the colour stage's own lists, the four-component and the rectangle list
        assert d == {("planes", 0, 0, 1): 1, ("planes", 1, 0, 1): 1, ("planes", 1, 1, 2): 1, ("planes", 2, 0, 1): 1, ("planes", 2, 1, 1): 1, ("planes", 2, 2, 1): 1,
                     ("planes", 3, 0, 8): 1, ("planes", 4, 2, 1): 1, ("colour", 0): 1, ("colour_scaled", 1): 1, ("colour_scaled_rgb", 1): 1, ("colour", 2): 1,
                     ("colour_scaled", 3): 1, ("colour", 4): 1, ("colour4", 1): 1, ("colour_rect", 2, 0): 1}
    finally:
        for d_ in items:
            d_.close()
        for p in keep:
            p.close()


def test_decode_to_tensors_crops_are_pillows_resize_box(gpu_ctx):
    """decode_to_tensors(files, size=, crops=, decoder="libjpeg", resample="bicubic") equals Pillow's resize(size, BICUBIC, box=crop) bit for bit,
    and fewer planes-stage tiles run than for the whole files (a child: torch)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exact_rect_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "exact rect tensors ok" in r.stdout
