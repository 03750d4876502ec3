"""The libjpeg-exact decode on the GPU (jda_exact_decode_surfaces / _planes, jda_decode_to_host_exact, decode_to_tensors(decoder="libjpeg");
DESIGN.md 5.17) against the numpy twin (tests/exact_util.py) and Pillow:
(a) the whole file grid of a layout in ONE call into guard-filled back-to-back surfaces -- per picture a baseline source with a host index,
    one with a device index, and a dense and a sparse coefficient image of the same coefficients side by side --: pixels = twin = Pillow,
    the guard intact everywhere else, a fixed number of launches, twice; the same into 8-bit gray surfaces (Pillow's draft("L"));
(b) clipped outputs; (c) the component planes; (d) jda_decode_to_host_exact; (e) a file outside the comparison window, held to the twin
    alone (the range-limit table's wrap); (f) a mixed batch with refused images, and calls that launch nothing; (g) decode_to_tensors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import jpegdec_amd as J
from tests import coef_jpeg
from tests import exact_util as X
from tests import recode_util as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
MODE = {"gray": 0, "4:4:4": 1, "4:2:0": 2, "4:2:2": 3, "4:4:0": 4}
SUCCESS, INVALID_PARAMETER, DECODE_ERROR, UNSUPPORTED = 0, 1, 2, 3


def counts():
    c = J.kernel_launch_counts()
    out = {}
    for m in range(5):
        for f in range(3):                                          # the load phase: dense, sparse, a resident baseline image
            out["planes", m, f] = sum(v for k, v in c.items() if "jda_exact_planesILi%dELi%dE" % (m, f) in k)
        out["colour", m] = sum(v for k, v in c.items() if "jda_exact_colourILi%dE" % m in k)
    return out


def delta(before):
    after = counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


class Sources:
    """every resident form of a list of files: a baseline file gives "host", "device", "dense", "sparse"; a progressive one the last two"""
    def __init__(self, ctx, files, only=None):
        self.items, self.file_of, self.kind, self.keep = [], [], [], []
        for i, f in enumerate(files):
            prog = R.frame_header(f)[1] == 0xC2
            for kind in (("dense", "sparse") if prog else ("host", "device", "dense", "sparse")):
                if only and kind not in only:
                    continue
                if kind in ("host", "device"):
                    p = J.PreparedImage(f, device_prescan=(kind == "device"))
                    d = J.DeviceImage(ctx, p)
                else:
                    p = J.CoefImage(f) if prog else J.CoefImage(f, X.natural_blocks(f))
                    d = J.DeviceCoef(ctx, p, J.COEF_SPARSE if kind == "sparse" else J.COEF_DENSE)
                    assert d.form == (J.COEF_SPARSE if kind == "sparse" else J.COEF_DENSE)
                self.keep.append(p)
                self.items.append(d)
                self.file_of.append(i)
                self.kind.append(kind)

    def close(self):
        for d in self.items:
            d.close()
        for p in self.keep:
            p.close()


def decode_into_guard(ctx, sources, shapes, pixel_types, clips=None):
    """ONE jda_exact_decode_surfaces call into back-to-back surfaces in a guard-filled allocation -> (statuses, [surface rows x pitch], the
    bytes between and behind the surfaces).  shapes: (w, h) each; clips: (width_px, rows) each, default the image's own"""
    n = len(sources)
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
        status = J.exact_decode(ctx, sources, [(base + o, p, cw, cr) for o, p, (cw, cr) in zip(offs, pitch, clips)], pixel_types)
        raw = ctx.to_host(base, total)
    finally:
        ctx.free(base)
    surfaces, rest = [], np.ones(total, dtype=bool)
    for o, p, (w, h) in zip(offs, pitch, shapes):
        surfaces.append(raw[o:o + p * h].reshape(h, p))
        rest[o:o + p * h] = False
    return status, surfaces, raw[rest]


def check_surface(surface, want, what):
    """the visible pixels are `want`, every other byte of the surface is the guard's"""
    h, wb = want.shape
    assert np.array_equal(surface[:h, :wb], want), (what, int(np.count_nonzero(surface[:h, :wb] != want)))
    assert np.all(surface[:h, wb:] == FILL) and np.all(surface[h:] == FILL), (what, "bytes outside the visible pixels")


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_grid_in_one_call(gpu_ctx, sampling):
    names, files = zip(*X.grid(sampling))
    twins = [X.twin(f) for f in files]
    for f, t in zip(files, twins):                                  # the third party, inside the comparison window
        assert X.in_window(t)
        assert np.array_equal(t["rgb"], X.pillow(f, "RGB")) and np.array_equal(t["gray"], X.pillow(f, "L"))
    assert any(t["range"][0] < -128 and t["range"][1] > 127 for t in twins)      # (both clamps are forced)
    S = Sources(gpu_ctx, files)
    try:
        assert {"host", "device", "dense", "sparse"} <= set(S.kind)
        shapes = [twins[i]["gray"].shape[::-1] for i in S.file_of]
        m = MODE[sampling]
        for gray in (False, True):
            pts = [J.GRAY8 if gray else J.RGB8888] * len(S.items)
            for again in range(2):
                before = counts()
                status, surfaces, rest = decode_into_guard(gpu_ctx, S.items, shapes, pts)
                assert delta(before) == {("planes", m, 0): 1, ("planes", m, 1): 1, ("planes", m, 2): 1, ("colour", m): 1}
                assert status == [SUCCESS] * len(S.items)
                assert np.all(rest == FILL)
                for k, i in enumerate(S.file_of):
                    check_surface(surfaces[k], X.rgba(twins[i], gray), (names[i], S.kind[k], "gray" if gray else "rgba"))
    finally:
        S.close()


@pytest.mark.parametrize("sampling", ("gray", "4:2:0", "4:2:2"))
def test_clipped_outputs(gpu_ctx, sampling):
    f = dict(X.grid(sampling))["baseline_33x31_q90"]
    t = X.twin(f)
    S = Sources(gpu_ctx, [f] * 4, only=("host", "sparse"))
    try:
        n = len(S.items)
        clips = [(32, 31), (33, 30), (0, 31), (33, 0), (34, 32), (1, 1), (4, 2), (5, 31)][:n]
        for pt in (J.RGB8888, J.GRAY8):
            status, surfaces, rest = decode_into_guard(gpu_ctx, S.items, [(33, 31)] * n, [pt] * n, clips)
            assert status == [SUCCESS] * n and np.all(rest == FILL)
            bpp = 4 if pt == J.RGB8888 else 1
            for s, (cw, cr) in zip(surfaces, clips):
                cw, cr = min(cw, 33), min(cr, 31)
                want = X.rgba(t, pt == J.GRAY8)[:cr, :cw * bpp]
                assert np.array_equal(s[:cr, :cw * bpp], want), (cw, cr, pt)
                assert np.all(s[:, cw * bpp:] == FILL) and np.all(s[cr:] == FILL), (cw, cr, pt)
    finally:
        S.close()


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_planes(gpu_ctx, sampling):
    names, files = zip(*X.grid(sampling))
    files = files[:8]
    S = Sources(gpu_ctx, files, only=("device", "dense", "sparse"))
    try:
        n = len(S.items)
        ext = [[p.shape for p in X.twin(files[i])["planes"]] for i in S.file_of]
        specs, total = [], 256
        for e in ext:
            three = []
            for c in range(3):
                h, w = e[c] if c < len(e) else (0, 0)
                pitch = w + 3                                       # (any base, any pitch)
                three.append((total + 1, pitch, w, h))
                total += pitch * h + 64
            specs.append(three)
        base = gpu_ctx.malloc(total)
        try:
            gpu_ctx.memset(base, FILL, total)
            before = counts()
            status = J.exact_planes(gpu_ctx, S.items, [[(base + o, p, w, h) for o, p, w, h in three] for three in specs])
            d = delta(before)
            if sampling == "4:4:0":                                   # (every file of this grid is a baseline one)
                assert d == {("planes", MODE[sampling], f): 1 for f in range(3)}
            assert ("colour", MODE[sampling]) not in d and d[("planes", MODE[sampling], 0)] == 1 and d[("planes", MODE[sampling], 1)] == 1
            raw = gpu_ctx.to_host(base, total)
        finally:
            gpu_ctx.free(base)
        assert status == [SUCCESS] * n
        rest = np.ones(total, dtype=bool)
        for k, i in enumerate(S.file_of):
            t = X.twin(files[i])
            for c, plane in enumerate(t["planes"]):
                o, p, w, h = specs[k][c]
                got = np.lib.stride_tricks.as_strided(raw[o:], shape=(h, w), strides=(p, 1))
                assert np.array_equal(got, plane), (names[i], S.kind[k], c)
                for y in range(h):
                    rest[o + y * p:o + y * p + w] = False
            if sampling in ("gray", "4:4:4"):                        # (.. where the planes are also Pillow's draft("L") / draft("YCbCr"))
                ycc = X.pillow(files[i], "YCbCr" if sampling == "4:4:4" else "L")
                assert np.array_equal(np.stack(t["planes"], -1) if sampling == "4:4:4" else t["planes"][0], ycc)
        assert np.all(raw[rest] == FILL)
    finally:
        S.close()


def test_decode_to_host_exact(gpu_ctx):
    for sampling in coef_jpeg.LAYOUTS:
        g = dict(X.grid(sampling))
        for name in [k for k in g if "45x53" in k or "17x9" in k]:
            t = X.twin(g[name])
            assert X.in_window(t)
            rc, got = J.decode_to_host_exact(gpu_ctx, g[name])
            assert rc == 0 and np.array_equal(got[..., :3], X.pillow(g[name], "RGB")) and np.all(got[..., 3] == 255), (sampling, name)
            rc, got = J.decode_to_host_exact(gpu_ctx, g[name], J.GRAY8)
            assert rc == 0 and np.array_equal(got, X.pillow(g[name], "L")), (sampling, name)
    rc, got = J.decode_to_host_exact(gpu_ctx, g[name], J.RGB565_LE)
    assert rc == INVALID_PARAMETER and not got.any()
    # a pitch below the width's bytes is refused, not truncated; a bad MCU and an Adobe segment get their codes; nothing is launched or written
    before = counts()
    f = g[name]
    w, h = X.twin(f)["gray"].shape[::-1]
    host = np.full((h, w * 4), FILL, np.uint8)
    for pt, pitch in ((J.RGB8888, w * 4 - 1), (J.GRAY8, w - 1), (J.RGB8888, 0)):
        assert gpu_ctx.lib.jda_decode_to_host_exact(gpu_ctx.handle, f, len(f), pt, host.ctypes.data_as(J.binding.C.c_void_p), pitch, h) == INVALID_PARAMETER
    refused = R.refused()
    for key, want in (("bad_mcu", DECODE_ERROR), ("adobe", UNSUPPORTED)):
        rc, got = J.decode_to_host_exact(gpu_ctx, refused[key][0])
        assert rc == want and not got.any(), key
    assert np.all(host == FILL) and delta(before) == {}


@pytest.mark.parametrize("sampling", ("gray", "4:2:0"))
def test_outside_the_window_the_twin_alone(gpu_ctx, sampling):
    """amplitude 1023 in every position under quantisers of 1: pre-limit results far outside -512 .. 511, where libjpeg-turbo's SIMD IDCT
    saturates and the C table -- the contract -- wraps; and 16-bit quantisers, whose products leave 16 bits"""
    wrap = X.written_file(24, 16, sampling, 0, amplitude=1023, seed=9)
    word = X.written_file(24, 16, sampling, 0, amplitude=60, seed=4, word=True)
    for f in (wrap, word):
        t = X.twin(f)
        assert not X.in_window(t)
        S = Sources(gpu_ctx, [f])
        try:
            status, surfaces, rest = decode_into_guard(gpu_ctx, S.items, [(24, 16)] * 4, [J.RGB8888] * 4)
            assert status == [SUCCESS] * 4 and np.all(rest == FILL)
            for s, kind in zip(surfaces, S.kind):
                check_surface(s, X.rgba(t), kind)
        finally:
            S.close()


def test_refusals_and_a_mixed_batch(gpu_ctx):
    g = dict(X.grid("4:2:0"))
    f, prog = g["baseline_33x31_q90"], g["progressive_33x31_q90"]
    t = X.twin(f)
    S = Sources(gpu_ctx, [f, prog], only=("host", "dense"))
    first_prepared = J.PreparedImage(prog)
    first_scan = J.DeviceImage(gpu_ctx, first_prepared)             # a resident image of a progressive file: its DC scan only
    bad, adobe = R.refused()["bad_mcu"][0], R.refused()["adobe"][0]
    extra_host = [J.PreparedImage(bad), J.PreparedImage(adobe), J.CoefImage(adobe, X.natural_blocks(adobe))]
    extra = [J.DeviceImage(gpu_ctx, extra_host[0]), J.DeviceImage(gpu_ctx, extra_host[1]), J.DeviceCoef(gpu_ctx, extra_host[2], J.COEF_SPARSE)]
    try:
        # (a baseline image whose pre-scan met a bad MCU; a file with an Adobe APP14 segment as a baseline image and as a coefficient image)
        items = S.items + extra + [first_scan]
        n = len(items)
        pitch = (33 * 4 + 15) & ~15
        size = pitch * 31 + 256
        base = gpu_ctx.malloc(size * n + 256)
        try:
            gpu_ctx.memset(base, FILL, size * n + 256)
            outs = [(base + size * k, pitch, 33, 31) for k in range(n)]
            before = counts()
            # a pixel type the road does not have, a misaligned base, a pitch too small, a NULL surface: the call launches nothing
            for bad_pt, bad_out in ((J.RGB565_LE, outs[0]), (J.RGB8888, (base + 4, pitch, 33, 31)), (J.RGB8888, (base, 64, 33, 31)), (J.RGB8888, (0, pitch, 33, 31))):
                assert J.exact_decode(gpu_ctx, items[:1], [bad_out], [bad_pt]) == [INVALID_PARAMETER]
            assert J.exact_decode(gpu_ctx, [first_scan], outs[:1]) == [UNSUPPORTED]
            assert J.exact_decode(gpu_ctx, extra, outs[:3]) == [DECODE_ERROR, UNSUPPORTED, UNSUPPORTED]
            assert J.exact_decode(gpu_ctx, [], []) == []
            lib = gpu_ctx.lib
            assert lib.jda_exact_decode_surfaces(gpu_ctx.handle, 1, None, None, None, None) == INVALID_PARAMETER
            assert lib.jda_exact_decode_surfaces(None, 1, None, None, None, None) == 6
            assert lib.jda_exact_decode_surfaces(gpu_ctx.handle, -1, None, None, None, None) == INVALID_PARAMETER
            both = (J.binding.RecodeSource * 1)(J.binding.RecodeSource(items[0].handle, items[1].handle))
            one_out = (J.binding.Output * 1)(J.binding.Output(*outs[0]))
            st = (J.binding.C.c_int32 * 1)()
            assert lib.jda_exact_decode_surfaces(gpu_ctx.handle, 1, both, one_out, None, st) == INVALID_PARAMETER
            assert delta(before) == {}
            assert np.all(gpu_ctx.to_host(base, size * n + 256) == FILL)
            # the mixed batch: the refused images get their codes, the others are decoded
            pts = [J.RGB8888, J.RGB565_BE] + [J.RGB8888] * (n - 2)
            status = J.exact_decode(gpu_ctx, items, outs, pts)
            assert status == [SUCCESS, INVALID_PARAMETER] + [SUCCESS] * (n - 6) + [DECODE_ERROR, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED]
            raw = gpu_ctx.to_host(base, size * n + 256)
            for k in range(n):
                s = raw[size * k:size * k + pitch * 31].reshape(31, pitch)
                if status[k] == SUCCESS:
                    check_surface(s, X.rgba(t), k)
                else:
                    assert np.all(s == FILL), k
        finally:
            gpu_ctx.free(base)
    finally:
        first_scan.close()
        first_prepared.close()
        for d in extra:
            d.close()
        for p in extra_host:
            p.close()
        S.close()


def test_decode_to_tensors_libjpeg_is_pillow(gpu_ctx):
    """decode_to_tensors(files, size=(32, 32), resample="bicubic", decoder="libjpeg") over a mixed baseline / progressive list equals
    Image.open(f).convert("RGB").resize((32, 32), Image.BICUBIC) bit for bit; decoder="reference" gives what the default gives (a child: torch)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exact_torch_child.py")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "exact tensors ok" in r.stdout
