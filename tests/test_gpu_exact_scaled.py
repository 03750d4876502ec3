"""The libjpeg-exact decode at 1/2, 1/4 and 1/8 on the GPU (jda_exact_decode_surfaces_scaled / _planes_scaled,
jda_decode_to_host_exact_scaled, decode_to_tensors(decoder="libjpeg", draft=..)) against the numpy twin
(tests/exact_scaled_util.py), which tests/test_exact_scaled_cpu.py holds to Pillow's draft():
(a) the whole file grid of a layout x {host index, device index, dense, sparse} x scales {1, 2, 4, 8}, mixed, in ONE call into guard-filled
    back-to-back surfaces: pixels = twin, the guard intact everywhere else, the launches counted per kernel instance, twice; RGB8888 and gray;
    the scale-1 entries byte-equal to jda_exact_decode_surfaces; (b) clipped outputs; (c) the component planes; (d) the one call;
(e) files outside the comparison window, held to the twin alone; (f) a mixed batch with refused images, and calls that launch nothing;
(g) decode_to_tensors with draft=True against Pillow's draft -> convert -> resize."""
import os
import subprocess
import sys

import numpy as np
import pytest

import jpegdec_amd as J
from tests import coef_jpeg
from tests import exact_scaled_util as S
from tests import exact_util as X
from tests import recode_util as R
from tests.test_gpu_exact import FILL, MODE, Sources, check_surface

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUCCESS, INVALID_PARAMETER, DECODE_ERROR, UNSUPPORTED = 0, 1, 2, 3
LOAD = {"dense": 0, "sparse": 1, "host": 2, "device": 2}


def counts():
    c = J.kernel_launch_counts()
    out = {}
    for m in range(5):
        for f in range(3):                                          # the load phase: dense, sparse, a resident baseline image
            out["planes", m, f, 1] = sum(v for k, v in c.items() if "jda_exact_planesILi%dELi%dE" % (m, f) in k)
            for s in (2, 4, 8):
                out["planes", m, f, s] = sum(v for k, v in c.items() if "jda_exact_planes_scaledILi%dELi%dELi%dE" % (m, f, s) in k)
        out["colour", m, 1] = sum(v for k, v in c.items() if "jda_exact_colourILi%dE" % m in k)
        out["colour_scaled", m] = sum(v for k, v in c.items() if "jda_exact_colour_scaledILi%dE" % m in k)
    return out


def delta(before):
    after = counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def decode_into_guard(ctx, sources, shapes, pixel_types, scales, clips=None):
    """ONE jda_exact_decode_surfaces_scaled call into back-to-back surfaces in a guard-filled allocation -> (statuses, [surface rows x pitch],
    the bytes between and behind the surfaces).  shapes: the (w, h) of each surface; clips: (width_px, rows) each, default the surface's own"""
    bpp = [4 if pt == J.RGB8888 else 1 for pt in pixel_types]
    pitch = [max(16, (w * b + 15) & ~15) for (w, h), b in zip(shapes, bpp)]
    offs, total = [], 256
    for (w, h), p in zip(shapes, pitch):
        offs.append(total)
        total += ((p * h + 255) & ~255) + 256
    base = ctx.malloc(total)
    try:
        ctx.memset(base, FILL, total)
        clips = clips or shapes
        status = J.exact_decode(ctx, sources, [(base + o, p, cw, cr) for o, p, (cw, cr) in zip(offs, pitch, clips)], pixel_types, scales)
        raw = ctx.to_host(base, total)
    finally:
        ctx.free(base)
    surfaces, rest = [], np.ones(total, dtype=bool)
    for o, p, (w, h) in zip(offs, pitch, shapes):
        surfaces.append(raw[o:o + p * h].reshape(h, p))
        rest[o:o + p * h] = False
    return status, surfaces, raw[rest]


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_grid_in_one_call_at_mixed_scales(gpu_ctx, sampling):
    names, files, whs = zip(*S.grid(sampling))
    assert any(w > 500 for w, h in whs) and any(not S.forcible(w, h, 8) for w, h in whs)
    S1 = Sources(gpu_ctx, files)
    try:
        assert {"host", "device", "dense", "sparse"} <= set(S1.kind)
        # every resident source at every scale: the list interleaves the scales
        items, file_of, kind, scales = [], [], [], []
        for k, d in enumerate(S1.items):
            for j in range(4):
                items.append(d)
                file_of.append(S1.file_of[k])
                kind.append(S1.kind[k])
                scales.append(S.SCALES[(k + j) % 4])
        twins = [S.twin_scaled(files[i], s) for i, s in zip(file_of, scales)]
        shapes = [t["gray"].shape[::-1] for t in twins]
        m = MODE[sampling]
        present = {(LOAD[kd], s) for kd, s in zip(kind, scales)}
        assert present == {(f, s) for f in range(3) for s in S.SCALES}
        want_launches = {("planes", m, f, s): 1 for f, s in present}
        want_launches.update({("colour", m, 1): 1, ("colour_scaled", m): 3})
        full = None
        for gray in (False, True):
            pts = [J.GRAY8 if gray else J.RGB8888] * len(items)
            for again in range(2):
                before = counts()
                status, surfaces, rest = decode_into_guard(gpu_ctx, items, shapes, pts, scales)
                assert delta(before) == want_launches
                assert status == [SUCCESS] * len(items)
                assert np.all(rest == FILL)
                for k, i in enumerate(file_of):
                    check_surface(surfaces[k], S.rgba(twins[k], gray), (names[i], kind[k], scales[k], "gray" if gray else "rgba"))
            if not gray:
                full = [s for s, sc in zip(surfaces, scales) if sc == 1]
        # the scale-1 entries: the bytes jda_exact_decode_surfaces writes for the same sources
        ones = [k for k, sc in enumerate(scales) if sc == 1]
        from tests.test_gpu_exact import decode_into_guard as full_size
        status, surfaces, rest = full_size(gpu_ctx, [items[k] for k in ones], [shapes[k] for k in ones], [J.RGB8888] * len(ones))
        assert status == [SUCCESS] * len(ones) and len(full) == len(ones)
        for a, b in zip(full, surfaces):
            assert np.array_equal(a, b)
    finally:
        S1.close()


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_clipped_outputs(gpu_ctx, sampling):
    f = [f for name, f, wh in S.grid(sampling) if wh == (75, 53)][0]
    prog = R.frame_header(f)[1] == 0xC2
    S1 = Sources(gpu_ctx, [f] * 4, only=("dense", "sparse") if prog else ("host", "sparse"))
    try:
        n = len(S1.items)
        for s in (2, 4, 8):
            t = S.twin_scaled(f, s)
            h, w = t["gray"].shape
            clips = [(w - 1, h), (w, h - 1), (0, h), (w, 0), (w + 1, h + 1), (1, 1), (4, 2), (5, h)][:n]
            for pt in (J.RGB8888, J.GRAY8):
                status, surfaces, rest = decode_into_guard(gpu_ctx, S1.items, [(w, h)] * n, [pt] * n, [s] * n, clips)
                assert status == [SUCCESS] * n and np.all(rest == FILL)
                bpp = 4 if pt == J.RGB8888 else 1
                for sf, (cw, cr) in zip(surfaces, clips):
                    cw, cr = min(cw, w), min(cr, h)
                    want = S.rgba(t, pt == J.GRAY8)[:cr, :cw * bpp]
                    assert np.array_equal(sf[:cr, :cw * bpp], want), (cw, cr, pt, s)
                    assert np.all(sf[:, cw * bpp:] == FILL) and np.all(sf[cr:] == FILL), (cw, cr, pt, s)
    finally:
        S1.close()


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_planes(gpu_ctx, sampling):
    names, files, whs = zip(*S.grid(sampling)[::3])
    S1 = Sources(gpu_ctx, files, only=("device", "dense", "sparse"))
    try:
        n = len(S1.items)
        scales = [S.SCALES[1 + k % 3] for k in range(n)]
        twins = [S.twin_scaled(files[i], s) for i, s in zip(S1.file_of, scales)]
        specs, total = [], 256
        for t in twins:
            three = []
            for c in range(3):
                h, w = t["planes"][c].shape if c < len(t["planes"]) else (0, 0)
                pitch = w + 3                                       # (any base, any pitch)
                three.append((total + 1, pitch, w, h))
                total += pitch * h + 64
            specs.append(three)
        base = gpu_ctx.malloc(total)
        try:
            gpu_ctx.memset(base, FILL, total)
            before = counts()
            status = J.exact_planes(gpu_ctx, S1.items, [[(base + o, p, w, h) for o, p, w, h in three] for three in specs], scales)
            d = delta(before)
            assert d and all(k[0] == "planes" and k[3] in (2, 4, 8) and v == 1 for k, v in d.items()), d
            raw = gpu_ctx.to_host(base, total)
        finally:
            gpu_ctx.free(base)
        assert status == [SUCCESS] * n
        rest = np.ones(total, dtype=bool)
        for k, i in enumerate(S1.file_of):
            g = J.exact_scaled_geometry(files[i], scales[k])
            for c, plane in enumerate(twins[k]["planes"]):
                o, p, w, h = specs[k][c]
                assert g["components"][c] == (w, h)
                got = np.lib.stride_tricks.as_strided(raw[o:], shape=(h, w), strides=(p, 1))
                assert np.array_equal(got, plane), (names[i], S1.kind[k], scales[k], c)
                for y in range(h):
                    rest[o + y * p:o + y * p + w] = False
        assert np.all(raw[rest] == FILL)
    finally:
        S1.close()


def test_decode_to_host_exact_scaled(gpu_ctx):
    for sampling in coef_jpeg.LAYOUTS:
        for name, f, (w, h) in [x for x in S.grid(sampling) if x[2] in ((45, 53), (17, 9), (100, 37))][:4]:
            for s in (2, 4, 8):
                t = S.twin_scaled(f, s)
                assert X.in_window(t)
                rc, got = J.decode_to_host_exact(gpu_ctx, f, scale=s)
                assert rc == 0 and np.array_equal(got[..., :3], S.pillow_scaled(f, s, "RGB")) and np.all(got[..., 3] == 255), (sampling, name, s)
                rc, got = J.decode_to_host_exact(gpu_ctx, f, J.GRAY8, s)
                assert rc == 0 and np.array_equal(got, S.pillow_scaled(f, s, "L")), (sampling, name, s)
    before = counts()
    for bad in (0, 3, 16, -2):
        rc, got = J.decode_to_host_exact(gpu_ctx, f, scale=bad)
        assert rc == INVALID_PARAMETER and not got.any()
    rc, got = J.decode_to_host_exact(gpu_ctx, f, J.RGB565_LE, 2)
    assert rc == INVALID_PARAMETER and not got.any()
    # a pitch below the scaled width's bytes is refused; a bad MCU and an Adobe segment get their codes; nothing is launched or written
    w2, h2 = S.scaled_size(w, h, 2)
    host = np.full((h2, w2 * 4), FILL, np.uint8)
    for pt, pitch in ((J.RGB8888, w2 * 4 - 1), (J.GRAY8, w2 - 1)):
        assert gpu_ctx.lib.jda_decode_to_host_exact_scaled(gpu_ctx.handle, f, len(f), pt, 2, host.ctypes.data_as(J.binding.C.c_void_p), pitch, h2) == INVALID_PARAMETER
    refused = R.refused()
    for key, want in (("bad_mcu", DECODE_ERROR), ("adobe", UNSUPPORTED)):
        rc, got = J.decode_to_host_exact(gpu_ctx, refused[key][0], scale=4)
        assert rc == want and not got.any(), key
    assert np.all(host == FILL) and delta(before) == {}


@pytest.mark.parametrize("sampling", ("gray", "4:2:0", "4:4:0"))
def test_outside_the_window_the_twin_alone(gpu_ctx, sampling):
    """amplitude 1023 in every position under quantisers of 1, and 16-bit quantisers whose products leave 16 bits: the 32-bit multiplies wrap
    as the definition's do"""
    wrap = X.written_file(24, 16, sampling, 0, amplitude=1023, seed=9)
    word = X.written_file(24, 16, sampling, 0, amplitude=60, seed=4, word=True)
    outside = 0
    for f in (wrap, word):
        S1 = Sources(gpu_ctx, [f])
        try:
            for s in (2, 4, 8):
                t = S.twin_scaled(f, s)
                outside += not X.in_window(t)
                h, w = t["gray"].shape
                status, surfaces, rest = decode_into_guard(gpu_ctx, S1.items, [(w, h)] * 4, [J.RGB8888] * 4, [s] * 4)
                assert status == [SUCCESS] * 4 and np.all(rest == FILL)
                for sf, kd in zip(surfaces, S1.kind):
                    check_surface(sf, S.rgba(t), (kd, s))
        finally:
            S1.close()
    assert outside >= 3


def test_refusals_and_a_mixed_batch(gpu_ctx):
    g = {wh: f for name, f, wh in S.grid("4:2:0") if name.startswith("baseline")}
    f = g[(33, 31)] if (33, 31) in g else sorted(g.items())[-1][1]
    info = J.parse(f)
    w, h = info["width"], info["height"]
    S1 = Sources(gpu_ctx, [f], only=("host", "dense"))
    bad, adobe = R.refused()["bad_mcu"][0], R.refused()["adobe"][0]
    extra_host = [J.PreparedImage(bad), J.PreparedImage(adobe), J.CoefImage(adobe, X.natural_blocks(adobe))]
    extra = [J.DeviceImage(gpu_ctx, extra_host[0]), J.DeviceImage(gpu_ctx, extra_host[1]), J.DeviceCoef(gpu_ctx, extra_host[2], J.COEF_SPARSE)]
    try:
        items = S1.items * 3 + extra                                  # host, dense at three scale entries each, then the refused files
        n = len(items)
        pitch = (w * 4 + 15) & ~15
        size = pitch * h + 256
        base = gpu_ctx.malloc(size * n + 256)
        try:
            gpu_ctx.memset(base, FILL, size * n + 256)
            outs = [(base + size * k, pitch, w, h) for k in range(n)]
            before = counts()
            # every image refused: a scale outside {1, 2, 4, 8}, a pixel type the road lacks, a misaligned base, a pitch below the scaled width's bytes
            assert J.exact_decode(gpu_ctx, items[:4], outs[:4], None, [3, 0, 16, -1]) == [INVALID_PARAMETER] * 4
            w4 = -(-w // 4)
            for bad_pt, bad_out in ((J.RGB565_LE, outs[0]), (J.RGB8888, (base + 4, pitch, w, h)), (J.RGB8888, (base, (w4 * 4 - 1) & ~15, w, h)), (J.RGB8888, (0, pitch, w, h))):
                assert J.exact_decode(gpu_ctx, items[:1], [bad_out], [bad_pt], [4]) == [INVALID_PARAMETER]
            assert J.exact_decode(gpu_ctx, extra, outs[:3], None, [2, 4, 8]) == [DECODE_ERROR, UNSUPPORTED, UNSUPPORTED]
            assert J.exact_decode(gpu_ctx, [], [], None, []) == []
            lib = gpu_ctx.lib
            assert lib.jda_exact_decode_surfaces_scaled(gpu_ctx.handle, 1, None, None, None, None, None) == INVALID_PARAMETER
            assert lib.jda_exact_decode_surfaces_scaled(None, 1, None, None, None, None, None) == 6
            assert lib.jda_exact_decode_planes_scaled(gpu_ctx.handle, 1, None, None, None, None) == INVALID_PARAMETER
            assert delta(before) == {}
            assert np.all(gpu_ctx.to_host(base, size * n + 256) == FILL)
            # a surface whose pitch holds the scaled width only is taken at that scale (and refused at full size)
            small = [(base, (w4 * 4 + 15) & ~15, w, h)]
            assert J.exact_decode(gpu_ctx, items[:1], small, None, [1]) == [INVALID_PARAMETER]
            assert J.exact_decode(gpu_ctx, items[:1], small, None, [4]) == [SUCCESS]
            gpu_ctx.memset(base, FILL, size)
            # the mixed batch: scales == NULL entries and refused images beside decoded ones
            scales = [2, 2, 5, 8, 1, 4] + [2, 4, 8]
            pts = [J.RGB8888, J.RGB565_BE] + [J.RGB8888] * (n - 2)
            status = J.exact_decode(gpu_ctx, items, outs, pts, scales)
            assert status == [SUCCESS, INVALID_PARAMETER, INVALID_PARAMETER, SUCCESS, SUCCESS, SUCCESS, DECODE_ERROR, UNSUPPORTED, UNSUPPORTED]
            raw = gpu_ctx.to_host(base, size * n + 256)
            for k in range(n):
                sf = raw[size * k:size * k + pitch * h].reshape(h, pitch)
                if status[k] == SUCCESS:
                    check_surface(sf, S.rgba(S.twin_scaled(f, scales[k])), k)
                else:
                    assert np.all(sf == FILL), k
        finally:
            gpu_ctx.free(base)
    finally:
        for d in extra:
            d.close()
        for p in extra_host:
            p.close()
        S1.close()


def test_decode_to_tensors_draft_is_pillow(gpu_ctx):
    """decode_to_tensors(files, size=(32, 32), resample="bicubic", decoder="libjpeg", draft=True) equals Pillow's draft -> convert("RGB") ->
    resize((32, 32), BICUBIC) bit for bit (a child: torch)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exact_scaled_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "exact scaled tensors ok" in r.stdout
