"""The colour models of the libjpeg-exact decode on the GPU (jda_exact_decode_surfaces_ex / _planes_ex, jda_decode_to_host_exact_ex with
JDA_EXACT_COLOUR_MODELS, decode_to_tensors(decoder="libjpeg", colour_models=True)) against the numpy twin
(tests/exact_adobe_util.py), which tests/test_exact_adobe_cpu.py holds to Pillow:
(a) per layout, the four-component file grid in ONE call into guard-filled back-to-back surfaces, every file to RGB8888 and to CMYK8888, CMYK
    and YCCK and both K samplings side by side: pixels = twin, the guard intact everywhere else, the launches counted per kernel instance, twice;
(b) clipped outputs; (c) the four component planes; (d) the one call, baseline and progressive; (e) RGB-coded and Adobe transform-1 files from
    host-index, device-index and coefficient sources at all four scales; (f) a mixed batch with refusals, calls that launch nothing, and what
    the calls without the flag and the other consumers of coefficient images still refuse; (g) decode_to_tensors over a mixed list."""
import os
import subprocess
import sys

import numpy as np
import pytest

import jpegdec_amd as J
from tests import exact_adobe_util as A
from tests import exact_scaled_util as S
from tests import exact_util as X
from tests import recode_util as R
from tests.test_gpu_exact import MODE, Sources

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A
SUCCESS, INVALID_PARAMETER, DECODE_ERROR, UNSUPPORTED = 0, 1, 2, 3
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
    return out


def delta(before):
    after = counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


class Coefs:
    """the coefficient images of jda_coef_prepare of a list of files, resident"""
    def __init__(self, ctx, files):
        self.hosts = [J.CoefImage.from_file(f) for f in files]
        self.items = [J.DeviceCoef(ctx, h, J.COEF_AUTO) for h in self.hosts]
        assert all(d.form == J.COEF_DENSE for d, h in zip(self.items, self.hosts) if h.info.ncomp == 4)      # (AUTO picks dense for four components)

    def close(self):
        for d in self.items:
            d.close()
        for h in self.hosts:
            h.close()


def decode_into_guard(ctx, sources, shapes, pixel_types, scales=None, clips=None, colour_models=True):
    """ONE call into back-to-back surfaces in a guard-filled allocation -> (statuses, [surface rows x pitch], the bytes between and behind)"""
    bpp = [1 if pt == J.GRAY8 else 4 for pt in pixel_types]
    pitch = [max(16, (w * b + 15) & ~15) for (w, h), b in zip(shapes, bpp)]
    offs, total = [], 256
    for (w, h), p in zip(shapes, pitch):
        offs.append(total)
        total += ((p * h + 255) & ~255) + 256
    base = ctx.malloc(total)
    try:
        ctx.memset(base, FILL, total)
        clips = clips or shapes
        status = J.exact_decode(ctx, sources, [(base + o, p, cw, cr) for o, p, (cw, cr) in zip(offs, pitch, clips)], pixel_types, scales, colour_models=colour_models)
        raw = ctx.to_host(base, total)
    finally:
        ctx.free(base)
    surfaces, rest = [], np.ones(total, dtype=bool)
    for o, p, (w, h) in zip(offs, pitch, shapes):
        surfaces.append(raw[o:o + p * h].reshape(h, p))
        rest[o:o + p * h] = False
    return status, surfaces, raw[rest]


def check_surface(surface, want, what):
    h, wb = want.shape
    assert np.array_equal(surface[:h, :wb], want), (what, int(np.count_nonzero(surface[:h, :wb] != want)))
    assert np.all(surface[:h, wb:] == FILL) and np.all(surface[h:] == FILL), (what, "bytes outside the visible pixels")


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_four_component_grid_in_one_call(gpu_ctx, sampling):
    names, files = zip(*A.grid4(sampling))
    twins = [A.twin4(f) for f in files]
    assert {A.model(f) for f in files} == {A.CMYK, A.YCCK}
    assert {A.header(f)["hv"][3] == A.header(f)["hv"][0] for f in files} == ({True} if sampling == "4:4:4" else {True, False})
    S4 = Coefs(gpu_ctx, files)
    try:
        n = len(files)
        items = S4.items * 2                                              # every file to RGB8888 and to CMYK8888, in one call
        pts = [J.RGB8888] * n + [J.CMYK8888] * n
        shapes = [t["rgb"].shape[1::-1] for t in twins] * 2
        m = MODE[sampling]
        for again in range(2):
            before = counts()
            status, surfaces, rest = decode_into_guard(gpu_ctx, items, shapes, pts)
            assert delta(before) == {("planes", m, 0, 1): 1, ("planes", 0, 0, 1): 1, ("colour4", m): 1}      # (K's tiles in the gray launch)
            assert status == [SUCCESS] * (2 * n) and np.all(rest == FILL)
            for k in range(2 * n):
                check_surface(surfaces[k], A.surface(twins[k % n], k >= n), (names[k % n], "cmyk" if k >= n else "rgb"))
    finally:
        S4.close()


@pytest.mark.parametrize("sampling", ("4:2:0", "4:4:0"))
def test_four_component_clips(gpu_ctx, sampling):
    name, f = [(nm, f) for nm, f in A.grid4(sampling) if "33x31" in nm][-1]
    t = A.twin4(f)
    clips = [(32, 31), (33, 30), (0, 31), (33, 0), (34, 32), (1, 1), (4, 2), (5, 31), (17, 16), (16, 17)]
    S4 = Coefs(gpu_ctx, [f] * len(clips))
    try:
        for pt in (J.RGB8888, J.CMYK8888):
            status, surfaces, rest = decode_into_guard(gpu_ctx, S4.items, [(33, 31)] * len(clips), [pt] * len(clips), clips=clips)
            assert status == [SUCCESS] * len(clips) and np.all(rest == FILL)
            for s, (cw, cr) in zip(surfaces, clips):
                cw, cr = min(cw, 33), min(cr, 31)
                assert np.array_equal(s[:cr, :cw * 4], A.surface(t, pt == J.CMYK8888)[:cr, :cw * 4]), (name, cw, cr, pt)
                assert np.all(s[:, cw * 4:] == FILL) and np.all(s[cr:] == FILL), (name, cw, cr, pt)
    finally:
        S4.close()


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_four_planes(gpu_ctx, sampling):
    """libjpeg's raw-data output: the samples un-inverted, each component at its own extent"""
    names, files = zip(*[(nm, f) for nm, f in A.grid4(sampling) if "45x53" in nm or "17x9" in nm or "3x3" in nm or "161x17" in nm])
    S4 = Coefs(gpu_ctx, files)
    try:
        specs, total = [], 256
        for f in files:
            four = []
            for p in A.twin4(f)["planes"]:
                h, w = p.shape
                four.append((total + 1, w + 3, w, h))                    # (any base, any pitch)
                total += (w + 3) * h + 64
            specs.append(four)
        base = gpu_ctx.malloc(total)
        try:
            gpu_ctx.memset(base, FILL, total)
            before = counts()
            status = J.exact_planes(gpu_ctx, S4.items, [[(base + o, p, w, h) for o, p, w, h in four] for four in specs], colour_models=True)
            assert delta(before) == {("planes", MODE[sampling], 0, 1): 1, ("planes", 0, 0, 1): 1}
            raw = gpu_ctx.to_host(base, total)
        finally:
            gpu_ctx.free(base)
        assert status == [SUCCESS] * len(files)
        rest = np.ones(total, dtype=bool)
        for k, f in enumerate(files):
            for c, plane in enumerate(A.twin4(f)["planes"]):
                o, p, w, h = specs[k][c]
                got = np.lib.stride_tricks.as_strided(raw[o:], shape=(h, w), strides=(p, 1))
                assert np.array_equal(got, plane), (names[k], c)
                for y in range(h):
                    rest[o + y * p:o + y * p + w] = False
        assert np.all(raw[rest] == FILL)
    finally:
        S4.close()


def test_the_one_call(gpu_ctx):
    for sampling in ("4:2:0", "4:2:2", "4:4:0"):
        g = [(nm, f) for nm, f in A.grid4(sampling) if "45x53" in nm or "75x53" in nm or "17x9" in nm]
        assert sampling == "4:4:0" or {A.header(f)["sof"] for nm, f in g} >= {0xC0, 0xC2}
        for nm, f in g:
            rc, got = J.decode_to_host_exact(gpu_ctx, f, colour_models=True)
            assert rc == 0 and np.array_equal(got[..., :3], A.pillow(f, "RGB")) and np.all(got[..., 3] == 255), (sampling, nm)
            rc, got = J.decode_to_host_exact(gpu_ctx, f, J.CMYK8888, colour_models=True)
            assert rc == 0 and np.array_equal(got, A.pillow(f)), (sampling, nm)
    before = counts()
    f = A.pillow_cmyk(45, 53, "4:2:0", 75, True)                          # (a progressive one: without the flag jda_progressive_prepare refuses it)
    for pt, scale, flag, want in ((J.GRAY8, 1, True, UNSUPPORTED), (J.RGB8888, 2, True, UNSUPPORTED), (J.RGB8888, 1, False, UNSUPPORTED), (J.CMYK8888, 1, False, INVALID_PARAMETER)):
        rc, got = J.decode_to_host_exact(gpu_ctx, f, pt, scale, colour_models=flag)
        assert rc == want and not got.any(), (pt, scale, flag)
    rgb3 = A.pillow_rgb3(45, 53, "4:2:0", 75, "ids")
    rc, got = J.decode_to_host_exact(gpu_ctx, rgb3, J.CMYK8888, colour_models=True)      # (a pixel type of four-component sources alone)
    assert rc == INVALID_PARAMETER and not got.any() and delta(before) == {}
    for variant in ("ids", "adobe0", "adobe1"):
        for prog in (False, True):
            f3 = A.pillow_rgb3(45, 53, "4:2:0", 75, variant, prog)
            for s in S.SCALES:
                rc, got = J.decode_to_host_exact(gpu_ctx, f3, J.RGB8888, s, colour_models=True)
                want = A.pillow(f3, "RGB") if s == 1 else S.pillow_scaled(f3, s)
                assert rc == 0 and np.array_equal(got[..., :3], want), (variant, prog, s)


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_three_component_files_at_all_scales(gpu_ctx, sampling):
    """RGB-coded and YCbCr files with and without the markers, from host-index, device-index, dense and sparse sources, scales mixed in ONE call"""
    names, files, models = zip(*A.grid3(sampling))
    assert set(models) == {A.RGB, A.YCBCR}
    Sr = Sources(gpu_ctx, files)
    try:
        assert {"host", "device", "dense", "sparse"} <= set(Sr.kind)
        n = len(Sr.items)
        m = MODE[sampling]
        for rot in range(4):                                              # (every source at every scale: every RGB instance is launched)
            scales = [S.SCALES[(k + rot) % 4] for k in range(n)]
            twins = [A.twin3(files[i], s) for i, s in zip(Sr.file_of, scales)]
            shapes = [t["rgb"].shape[1::-1] for t in twins]
            before = counts()
            status, surfaces, rest = decode_into_guard(gpu_ctx, Sr.items, shapes, [J.RGB8888] * n, scales)
            d = delta(before)
            assert status == [SUCCESS] * n and np.all(rest == FILL)
            for k in range(n):
                check_surface(surfaces[k], A.surface(twins[k]), (names[Sr.file_of[k]], Sr.kind[k], scales[k]))
            # one colour launch per (layout, scale, RGB-coded or not) present, each of its own kernel
            present = {(s, models[i] == A.RGB) for i, s in zip(Sr.file_of, scales)}
            assert d.get(("colour_rgb", m), 0) == ((1, True) in present) and d.get(("colour", m), 0) == ((1, False) in present)
            assert d.get(("colour_scaled_rgb", m), 0) == sum(1 for s in (2, 4, 8) if (s, True) in present)
            assert d.get(("colour_scaled", m), 0) == sum(1 for s in (2, 4, 8) if (s, False) in present)
            assert ("colour4", m) not in d
        # without the flag: an Adobe segment is refused as ever, and a file with 'R','G','B' ids is taken for YCbCr as ever
        status, surfaces, rest = decode_into_guard(gpu_ctx, Sr.items, [X.twin(files[i])["rgb"].shape[1::-1] for i in Sr.file_of], [J.RGB8888] * n, colour_models=False)
        for k, i in enumerate(Sr.file_of):
            if b"Adobe" in files[i]:
                assert status[k] == UNSUPPORTED and np.all(surfaces[k] == FILL)
            else:
                assert status[k] == SUCCESS
                check_surface(surfaces[k], X.rgba(X.twin(files[i])), (names[i], "no flag"))
        # gray output of an RGB-coded source is refused; of a YCbCr one with an Adobe segment it is the Y plane
        status, surfaces, rest = decode_into_guard(gpu_ctx, Sr.items, [X.twin(files[i])["rgb"].shape[1::-1] for i in Sr.file_of], [J.GRAY8] * n)
        for k, i in enumerate(Sr.file_of):
            if models[i] == A.RGB:
                assert status[k] == UNSUPPORTED and np.all(surfaces[k] == FILL)
            else:
                check_surface(surfaces[k], X.twin(files[i])["gray"], (names[i], "gray"))
    finally:
        Sr.close()


def test_narrow_rgb_coded_files(gpu_ctx):
    """a component of at most two samples across is replicated, not interpolated (jdsample.c): widths 3, 4 and 5 of every subsampled layout"""
    files = [A.pillow_rgb3(w, 7, s, 90, "ids") for s in ("4:2:0", "4:2:2") for w in (3, 4, 5)]
    Sr = Sources(gpu_ctx, files, only=("host", "dense"))
    try:
        twins = [A.twin3(files[i]) for i in Sr.file_of]
        status, surfaces, rest = decode_into_guard(gpu_ctx, Sr.items, [t["rgb"].shape[1::-1] for t in twins], [J.RGB8888] * len(Sr.items))
        assert status == [SUCCESS] * len(Sr.items) and np.all(rest == FILL)
        for k, i in enumerate(Sr.file_of):
            assert np.array_equal(twins[k]["rgb"], A.pillow(files[i], "RGB"))
            check_surface(surfaces[k], A.surface(twins[k]), (i, Sr.kind[k]))
    finally:
        Sr.close()


def test_refusals_and_a_mixed_batch(gpu_ctx):
    c4 = dict(A.grid4("4:2:0"))
    cmyk = [f for nm, f in c4.items() if "33x31" in nm][0]
    adobe = A.pillow_rgb3(33, 31, "4:2:0", 90, "adobe1")                  # Photoshop's: Adobe transform 1, YCbCr
    rgb3 = A.pillow_rgb3(33, 31, "4:2:0", 90, "adobe0")
    gray = dict(X.grid("gray"))["baseline_33x31_q90"]
    # the recode's refused Adobe file (JFIF + Adobe, 4:4:4, dense blocks under quantisers of 1): far outside the comparison window, where
    # libjpeg-turbo's SIMD IDCT saturates, so it is held to the twin alone, as every such file of the exact road is
    old = R.refused()["adobe"][0]
    t4, ta, tr, tg, to = A.twin4(cmyk), A.twin3(adobe), A.twin3(rgb3), X.twin(gray), A.twin3(old)
    assert np.array_equal(ta["rgb"], A.pillow(adobe, "RGB")) and A.in_window(ta) and not A.in_window(to) and A.model(old) == A.YCBCR
    S4 = Coefs(gpu_ctx, [cmyk, cmyk, cmyk, cmyk])
    Sr = Sources(gpu_ctx, [adobe, rgb3, old, gray], only=("device", "dense"))
    try:
        # four components: to RGB8888, to gray (refused), at 1/2 (refused), to RGB565 (no such type); then the Adobe, RGB-coded and gray files
        items = S4.items + Sr.items
        n = len(items)
        pts = [J.RGB8888, J.GRAY8, J.RGB8888, J.RGB565_LE] + [J.RGB8888] * len(Sr.items)
        scales = [1, 1, 2, 1] + [1] * len(Sr.items)
        tw = [ta, ta, tr, tr, to, to, tg, tg]
        shapes = [(33, 31)] * 4 + [t["rgb"].shape[1::-1] for t in tw]
        before = counts()
        status, surfaces, rest = decode_into_guard(gpu_ctx, items, shapes, pts, scales)
        assert status == [SUCCESS, UNSUPPORTED, UNSUPPORTED, INVALID_PARAMETER] + [SUCCESS] * len(Sr.items) and np.all(rest == FILL)
        check_surface(surfaces[0], A.surface(t4), "cmyk")
        for k in (1, 2, 3):
            assert np.all(surfaces[k] == FILL), k
        for k, want in enumerate([A.surface(ta)] * 2 + [A.surface(tr)] * 2 + [A.surface(to)] * 2 + [X.rgba(tg)] * 2):
            check_surface(surfaces[4 + k], want, ("mixed", k))
        assert delta(before) == {("planes", 2, 0, 1): 1, ("planes", 2, 2, 1): 1, ("planes", 1, 0, 1): 1, ("planes", 1, 2, 1): 1, ("planes", 0, 0, 1): 1, ("planes", 0, 2, 1): 1,
                                 ("colour4", 2): 1, ("colour", 2): 1, ("colour_rgb", 2): 1, ("colour", 1): 1, ("colour", 0): 1}
        # the flag absent: every one of them but the gray file is refused, as ever, and a call that refuses everything launches nothing
        before = counts()
        status, surfaces, rest = decode_into_guard(gpu_ctx, items[:10], shapes[:10], [J.RGB8888] * 10, colour_models=False)
        assert status == [UNSUPPORTED] * 10 and all(np.all(s == FILL) for s in surfaces) and np.all(rest == FILL)
        status, surfaces, rest = decode_into_guard(gpu_ctx, items[:4], shapes[:4], [J.GRAY8, J.GRAY8, J.RGB8888, J.RGB8888], [1, 1, 2, 4])
        assert status == [UNSUPPORTED] * 4 and all(np.all(s == FILL) for s in surfaces)
        status, surfaces, rest = decode_into_guard(gpu_ctx, items[:1], shapes[:1], [J.CMYK8888], colour_models=False)
        assert status == [INVALID_PARAMETER]
        status, surfaces, rest = decode_into_guard(gpu_ctx, Sr.items[:1], shapes[4:5], [J.CMYK8888])
        assert status == [INVALID_PARAMETER] and np.all(surfaces[0] == FILL)
        assert J.exact_planes(gpu_ctx, S4.items[:1], [[(0, 0, 0, 0)] * 3]) == [UNSUPPORTED]
        assert delta(before) == {}
        # the other consumers of coefficient images refuse a four-component one
        lib, C = gpu_ctx.lib, J.binding.C
        pitch = 48 * 4
        surf = gpu_ctx.malloc(pitch * 32)
        try:
            gpu_ctx.memset(surf, FILL, pitch * 32)
            out = (J.binding.Output * 1)(J.binding.Output(surf, pitch, 48, 32))
            one = (J.binding._P * 1)(S4.items[0].handle)
            pt, opt = (C.c_int32 * 1)(J.RGB8888), (C.c_int32 * 1)(0)
            assert lib.jda_coef_decode_surfaces(gpu_ctx.handle, 1, one, out, pt, opt) == UNSUPPORTED
            assert lib.jda_coef_decode_surfaces_rect(gpu_ctx.handle, 1, one, out, pt, opt, None) == UNSUPPORTED
            sizes, st = J.recode_images(gpu_ctx, S4.items[:1], [("baseline", None)], [surf], [pitch * 32])
            assert st == [UNSUPPORTED]
            assert np.all(gpu_ctx.to_host(surf, pitch * 32) == FILL)
        finally:
            gpu_ctx.free(surf)
        with pytest.raises(J.JdaError) as e:                              # dense only
            J.DeviceCoef(gpu_ctx, S4.hosts[0], J.COEF_SPARSE)
        assert e.value.code == UNSUPPORTED
    finally:
        Sr.close()
        S4.close()


def test_decode_to_tensors_with_colour_models_is_pillow(gpu_ctx):
    """a mixed list -- gray, YCbCr, Photoshop's transform 1, RGB-coded, CMYK, YCCK, baseline and progressive -- = convert("RGB").resize(BICUBIC) (a child: torch)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exact_adobe_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "exact adobe tensors ok" in r.stdout
