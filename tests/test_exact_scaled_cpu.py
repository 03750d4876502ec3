"""The libjpeg-exact decode at 1/2, 1/4 and 1/8 on the CPU: the definition against Pillow's draft(), and the kernels
against the definition.
(a) the numpy twin (tests/exact_scaled_util.py) = Pillow after draft() -- convert("RGB"), draft("L"), draft("YCbCr") -- bit for bit over the
    file grid of every layout at every scale Pillow can be forced to, every file asserted inside the comparison window, every test asserting
    the IDCT sizes and the upsampling kind it exists for; the h2v1 rule (fancy only above an own width of 2) at its edge;
(b) the kernels lane by lane (tests/hostsim/exact_scaled_sim.cpp: jda_exact_planes_scaled of all three load phases, jda_exact_colour_scaled,
    the LDS poisoned, every access held to its allocation, every visible byte and every byte of the planes stored exactly once) = the C
    row-major twin (exact_scaled_twin.h) = the numpy twin, for all three kinds of source, RGB8888 and gray, whole and clipped;
(c) the DC-only load phase reads no byte of the scan; (d) files outside the window held to the twin alone; (e) geometry, Pillow's choice of
    scale, every refusal, decode_to_tensors' argument errors; (f) the same as a program under ASan + UBSan."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from tests import coef_jpeg
from tests import exact_scaled_util as S
from tests import exact_util as X
from tests import recode_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB8888, GRAY8 = 2, 3
SUB = {"gray": (0, 1), "4:4:4": (0x11, 3), "4:2:2": (0x21, 3), "4:4:0": (0x12, 3), "4:2:0": (0x22, 3)}
# what each layout exists for at scales 2, 4, 8: (IDCT sizes of Y and chroma, the upsampling kinds that may occur)
EXPECT = {
    "gray": {2: ([4], {S.UP_NONE}), 4: ([2], {S.UP_NONE}), 8: ([1], {S.UP_NONE})},
    "4:4:4": {2: ([4, 4, 4], {S.UP_NONE}), 4: ([2, 2, 2], {S.UP_NONE}), 8: ([1, 1, 1], {S.UP_NONE})},
    "4:2:0": {2: ([4, 8, 8], {S.UP_NONE}), 4: ([2, 4, 4], {S.UP_NONE}), 8: ([1, 2, 2], {S.UP_NONE})},
    "4:2:2": {2: ([4, 4, 4], {S.UP_H2V1_FANCY, S.UP_H2V1_REPLICATE}), 4: ([2, 2, 2], {S.UP_H2V1_FANCY, S.UP_H2V1_REPLICATE}), 8: ([1, 1, 1], {S.UP_H2V1_REPLICATE})},
    "4:4:0": {2: ([4, 4, 4], {S.UP_H1V2_FANCY}), 4: ([2, 2, 2], {S.UP_H1V2_FANCY}), 8: ([1, 1, 1], {S.UP_H1V2_REPLICATE})},
}


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "tests/hostsim/libjda_exactscaledsim.so"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_exactscaledsim.so"))
    lib.exactscaledsim_run.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
    lib.exactscaledsim_plan.argtypes = [C.c_int] * 8 + [C.c_void_p]
    lib.exactscaledsim_draft.argtypes = [C.c_int] * 4
    return lib


def is_pillow(f, s):
    t = S.twin_scaled(f, s)
    assert X.in_window(t), t["range"]
    assert np.array_equal(t["rgb"], S.pillow_scaled(f, s, "RGB"))
    assert np.array_equal(t["gray"], S.pillow_scaled(f, s, "L"))
    assert np.array_equal(t["ycc"], S.pillow_scaled(f, s, "YCbCr"))
    return t


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_twin_is_pillow_after_draft(sampling):
    files = S.files(sampling)
    assert len(files) == 2 * len(S.SIZES) + len(S.WIDE) + 1 and len(S.SIZES) == 17
    seen = {s: set() for s in (2, 4, 8)}
    compared = 0
    for name, f, (w, h) in files:
        for s in (2, 4, 8):
            if not S.forcible(w, h, s):                             # (Pillow cannot be made to: the twin alone, through the lanes below)
                continue
            t = is_pillow(f, s)
            assert t["sizes"] == EXPECT[sampling][s][0], (name, s)
            assert t["gray"].shape == (-(-h // s), -(-w // s))
            seen[s].add(t["up"])
            compared += 1
    assert compared >= 90
    for s in (2, 4, 8):
        assert seen[s] == EXPECT[sampling][s][1], (s, seen[s])
    if sampling != "4:4:0":                                             # (every kind of file Pillow writes)
        assert {name.split("_")[0] for name, f, wh in files} >= {"baseline", "progressive", "optimize"}
    # scale 1 of the new twin is the full-size twin
    f = files[12][1]
    assert np.array_equal(S.twin_scaled(f, 1)["rgb"], X.twin(f)["rgb"])


def test_h2v1_is_fancy_only_above_an_own_width_of_two():
    """4:2:2 at 1/2: the chroma's own width is ceil(W / 4) -- 2 at W = 8 (replicated), 3 at W = 9 and 12 (fancy); at 1/4 ceil(W / 8)"""
    for (w, h), s, cw, kind in (((8, 8), 2, 2, S.UP_H2V1_REPLICATE), ((9, 8), 2, 3, S.UP_H2V1_FANCY), ((12, 5), 2, 3, S.UP_H2V1_FANCY), ((5, 8), 2, 2, S.UP_H2V1_REPLICATE),
                                ((16, 8), 4, 2, S.UP_H2V1_REPLICATE), ((17, 8), 4, 3, S.UP_H2V1_FANCY), ((4, 4), 2, 1, S.UP_H2V1_REPLICATE)):
        for q in (30, 95):
            f = S.pillow_file(w, h, "4:2:2", q)
            t = is_pillow(f, s)
            assert t["planes"][1].shape[1] == cw and t["up"] == kind, (w, h, s)


def run(sim, f, source, pt, s, clip=None, coefs=None):
    t = S.twin_scaled(f, s)
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
    info = (C.c_int32 * 8)()
    cw, cr = clip if clip else (w, h)
    nb = 0 if coefs is None else coefs.shape[0]
    rc = sim.exactscaledsim_run(f, len(f), None if coefs is None else coefs.ctypes.data, nb, source, pt, s, out.ctypes.data, pitch, cw, cr, twin_out.ctypes.data,
                                planes.ctypes.data if want_planes else None, tplanes.ctypes.data if want_planes else None, info)
    assert rc == 0, (rc, source, pt, s)
    assert info[0] > 0 and info[3] == 0 and info[4] == 0 and info[6] == 0 and info[7] == 0, list(info)
    if want_planes or source != 2:                                      # (a gray surface of a colour baseline image: the chroma is never read)
        assert (info[1], info[2]) == t["range"]
    want = S.rgba(t, pt == GRAY8)
    assert np.array_equal(twin_out, want), "the C twin is the numpy twin"
    cw, cr = min(cw, w), min(cr, h)
    got = out.reshape(h, pitch)
    assert np.array_equal(got[:cr, :cw * bpp], want[:cr, :cw * bpp]), ("the lanes", source, pt, s, clip)
    assert np.all(got[:, cw * bpp:] == 0x5A) and np.all(got[cr:] == 0x5A)
    if want_planes:
        flat = np.concatenate([p.reshape(-1) for p in t["planes"]])
        assert np.array_equal(tplanes, flat) and np.array_equal(planes, flat)
    return list(info)


def sources_of(f):
    prog = R.frame_header(f)[1] == 0xC2
    return [(0, None), (1, None)] if prog else [(2, None), (0, X.natural_blocks(f)), (1, X.natural_blocks(f))]


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_lanes_are_the_twin(sim, sampling):
    """every file of the grid the front end takes -- the sizes smaller than the scale included, which only the twin can witness --, every
    source, both pixel types, all three scales"""
    g = S.grid(sampling)
    assert any(not S.forcible(w, h, 8) for name, f, (w, h) in g) and any(w > 500 for name, f, (w, h) in g)
    for k, (name, f, wh) in enumerate(g):
        for source, coefs in sources_of(f):
            for s in (2, 4, 8):
                run(sim, f, source, RGB8888 if (k + s) % 3 else GRAY8, s, coefs=coefs)
                if wh in S.WIDE or wh == (33, 31):
                    run(sim, f, source, GRAY8 if (k + s) % 3 else RGB8888, s, coefs=coefs)


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_clipped_surfaces(sim, sampling):
    f = [f for name, f, wh in S.grid(sampling) if wh == (75, 53)][0]
    for s in (2, 4, 8):
        w, h = S.scaled_size(75, 53, s)
        for clip in ((w - 1, h), (w, h - 1), (0, h), (w, 0), (w + 1, h + 1), (1, 1), (5, 3)):
            for pt in (RGB8888, GRAY8):
                run(sim, f, 2, pt, s, clip=clip)
    run(sim, f, 1, RGB8888, 4, clip=(7, 5), coefs=X.natural_blocks(f))


@pytest.mark.parametrize("sampling", coef_jpeg.LAYOUTS)
def test_dc_only_load_phase_reads_no_scan_byte(sim, sampling):
    """at 1/8 every component of gray, 4:4:4, 4:2:2 and 4:4:0 is one sample a block: the DC value comes from the index, and no load of the run
    falls into the scan; 4:2:0's chroma (2x2) walks, and so does every layout at 1/2 and 1/4"""
    f = [f for name, f, wh in S.grid(sampling) if wh == (345, 9)][0]
    assert R.frame_header(f)[1] != 0xC2
    for pt in (RGB8888, GRAY8):
        info = run(sim, f, 2, pt, 8)
        if sampling == "4:2:0" and pt == RGB8888:
            assert info[5] > 0
        else:                                                           # (a gray surface of a 4:2:0 file decodes no chroma: no walk either)
            assert info[5] == 0, (sampling, pt, info[5])
        assert run(sim, f, 2, pt, 4)[5] > 0 and run(sim, f, 2, pt, 2)[5] > 0


@pytest.mark.parametrize("sampling", ("gray", "4:2:0", "4:2:2"))
def test_outside_the_window_the_contract_is_the_twin(sim, sampling):
    """amplitude 1023 in every position, and 16-bit quantisers whose products leave 16 bits: Pillow is no witness, the lanes equal the twins"""
    wrap = X.written_file(24, 16, sampling, 0, amplitude=1023, seed=9)
    word = X.written_file(24, 16, sampling, 0, amplitude=60, seed=4, word=True)
    outside = 0
    for f in (wrap, word):
        for s in (2, 4, 8):
            outside += not X.in_window(S.twin_scaled(f, s))
            for source, coefs in sources_of(f):
                run(sim, f, source, RGB8888, s, coefs=coefs)
    assert outside >= 3


def test_plan_geometry(sim):
    import jpegdec_amd as J
    out = (C.c_int64 * 16)()
    for sampling in coef_jpeg.LAYOUTS:
        sub, ncomp = SUB[sampling]
        hs, vs = coef_jpeg.LUMA_HV[sampling]
        per = {"gray": 64, "4:4:4": 20, "4:2:2": 16, "4:4:0": 16, "4:2:0": 10}[sampling]
        for w, h in S.SIZES + S.WIDE + ((333, 217),):
            for s in (2, 4, 8):
                assert sim.exactscaledsim_plan(w, h, ncomp, sub, 0, RGB8888, 0, s, out) == 0
                ss = S.component_sizes(sampling, s)
                ext = S.own_extents(w, h, sampling, s)
                mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
                py, pc = (mx * hs * ss[0] + 15) & ~15, ((mx * ss[-1] + 15) & ~15) if ncomp == 3 else 0
                ysz, csz = (py * my * vs * ss[0] + 255) & ~255, (pc * my * ss[-1] + 255) & ~255
                want = [s, ss[0], ss[-1], -(-w // s), -(-h // s), ext[-1][1], ext[-1][0], S.upsampling_kind(w, h, sampling, s), py, pc, my * vs * ss[0],
                        my * ss[-1] if ncomp == 3 else 0, ysz if ncomp == 3 else 0, ysz + csz if ncomp == 3 else 0, ysz + (2 * csz if ncomp == 3 else 0), my * -(-mx // per)]
                assert list(out) == want, (sampling, w, h, s, list(out), want)
                # the public call, through a real file's header where the grid has one
        for name, f, (w, h) in S.files(sampling)[::5]:
            for s in S.SCALES:
                g = J.exact_scaled_geometry(f, s)
                assert (g["width"], g["height"]) == S.scaled_size(w, h, s)
                assert g["components"] == [e[::-1] for e in (S.own_extents(w, h, sampling, s) if s > 1 else X.own_extents(w, h, sampling))]
    # scale 1 of the scaled plan is the full-size plan
    assert sim.exactscaledsim_plan(33, 31, 3, 0x22, 0, RGB8888, 0, 1, out) == 0 and list(out)[:7] == [1, 8, 8, 33, 31, 17, 16]


def test_draft_scale_is_pillows_choice(sim):
    import jpegdec_amd as J
    from PIL import Image
    f = S.pillow_file(100, 37, "4:2:0", 30)
    for rw, rh in [(rw, rh) for rw in (1, 3, 5, 12, 13, 24, 25, 26, 49, 50, 51, 100, 101, 400) for rh in (1, 2, 4, 5, 9, 10, 18, 19, 36, 37, 38, 200)]:
        im = Image.open(io.BytesIO(f))
        im.draft("RGB", (rw, rh))
        want = im.decoderconfig[0] if im.decoderconfig else 1
        assert J.exact_draft_scale(f, (rw, rh)) == want == S.draft_scale(100, 37, rw, rh) == sim.exactscaledsim_draft(100, 37, rw, rh), (rw, rh)
        assert im.size == S.scaled_size(100, 37, want)
    for w, h in S.SIZES:
        for rw, rh in ((1, 1), (2, 3), (w, h), (max(1, w // 2), max(1, h // 2)), (max(1, w // 8), max(1, h // 4))):
            assert sim.exactscaledsim_draft(w, h, rw, rh) == S.draft_scale(w, h, rw, rh)
    assert J.exact_draft_scale(f, (0, 5)) == 1 and J.exact_draft_scale(f, (5, -1)) == 1


def test_refusals(sim):
    import jpegdec_amd as J
    out = (C.c_int64 * 16)()
    for scale in (0, 3, 5, 6, 7, 9, 16, -1, -2):
        assert sim.exactscaledsim_plan(33, 31, 3, 0x22, 0, RGB8888, 0, scale, out) == 1, scale
        with pytest.raises(J.JdaError):
            J.exact_scaled_geometry(S.pillow_file(24, 40, "4:2:0", 30), scale)
    four = J.binding.ImageInfo()
    four.width, four.height, four.ncomp, four.mcus_x, four.mcus_y = 33, 31, 4, 5, 4
    with pytest.raises(J.JdaError) as e:                                # (a header the decode calls refuse by its layout has no geometry either)
        J.exact_scaled_geometry(four, 2)
    assert e.value.code == 3
    for s in S.SCALES:                                                  # everything the full-size check refuses stays refused
        for pt in (0, 1, 4, 5, 6, -1):
            assert sim.exactscaledsim_plan(33, 31, 3, 0x22, 0, pt, 0, s, out) == 1
        assert sim.exactscaledsim_plan(33, 31, 3, 0x22, 1, RGB8888, 0, s, out) == 3      # an Adobe APP14 segment
        assert sim.exactscaledsim_plan(33, 31, 4, 0x11, 0, RGB8888, 0, s, out) == 3      # four components
        assert sim.exactscaledsim_plan(0, 31, 3, 0x22, 0, RGB8888, 0, s, out) == 1
    # real files through the sources' own records: a bad MCU, an Adobe segment -- the surface stays untouched
    bad, adobe = R.refused()["bad_mcu"][0], R.refused()["adobe"][0]
    for f, source, coefs, want in ((bad, 2, None, 2), (adobe, 2, None, 3), (adobe, 0, X.natural_blocks(adobe), 3), (adobe, 1, X.natural_blocks(adobe), 3)):
        info = J.parse(f)
        pitch = (info["width"] * 4 + 15) & ~15
        raw = np.full(pitch * info["height"] + 16, 0x5A, np.uint8)
        a = (-raw.ctypes.data) & 15
        nb = 0 if coefs is None else coefs.shape[0]
        for s in (2, 8):
            rc = sim.exactscaledsim_run(f, len(f), None if coefs is None else coefs.ctypes.data, nb, source, RGB8888, s, raw[a:].ctypes.data, pitch, info["width"],
                                        info["height"], None, None, None, None)
            assert rc == want, (rc, source, want)
        assert np.all(raw == 0x5A)


def test_sanitizer_program(tmp_path):
    """the plan and the lanes over five files as a program of their own under ASan + UBSan (nothing is loaded into this process)"""
    subprocess.run(["make", "exactscaledasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    picks = (("4:2:0", (75, 53)), ("4:2:2", (345, 9)), ("gray", (161, 17)), ("4:4:0", (17, 9)), ("4:4:4", (31, 65)), ("4:2:0", (5, 6)))
    paths = []
    for k, (s, wh) in enumerate(picks):
        paths.append(str(tmp_path / ("f%d.jpg" % k)))
        with open(paths[-1], "wb") as fh:
            fh.write([f for name, f, x in S.grid(s) if x == wh][-1])
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "exact_scaled_asan")] + paths, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "exact_scaled_asan ok" in r.stdout, r.stdout[-4000:]


def test_exports_and_argument_errors():
    import jpegdec_amd as J
    for name in ("exact_scaled_geometry", "exact_draft_scale", "exact_decode", "exact_planes", "decode_to_host_exact"):
        assert callable(getattr(J, name)), name
    import inspect
    assert "scales" in inspect.signature(J.exact_decode).parameters and "scales" in inspect.signature(J.exact_planes).parameters
    assert "scale" in inspect.signature(J.decode_to_host_exact).parameters and "draft" in inspect.signature(J.decode_to_tensors).parameters
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    for fn in ("jda_exact_scaled_geometry", "jda_exact_draft_scale", "jda_exact_decode_surfaces_scaled", "jda_exact_decode_planes_scaled", "jda_decode_to_host_exact_scaled"):
        assert "int %s(" % fn in hdr and hasattr(J.load_library(), fn), fn
    for kw in (dict(decoder="reference", draft=True, size=(8, 8)), dict(draft=True, size=(8, 8)), dict(decoder="libjpeg", draft=True),
               dict(decoder="libjpeg", draft=(4, 4)), dict(decoder="libjpeg", draft=True, size=(8, 8), crops=[]), dict(decoder="libjpeg", draft=(0, 4), size=(8, 8)),
               dict(decoder="libjpeg", draft=(4, 4, 4), size=(8, 8)),
               # .. and the reference road's scales stay refused with decoder="libjpeg", draft or not
               dict(decoder="libjpeg", prescale=True, size=(8, 8)), dict(decoder="libjpeg", prescale=True, size=(8, 8), draft=True),
               dict(decoder="libjpeg", options=J.SCALE_QUARTER), dict(decoder="libjpeg", options=J.SCALE_HALF, size=(8, 8), draft=True)):
        with pytest.raises(ValueError):                             # (refused before torch or the GPU is touched)
            J.decode_to_tensors(None, [], **kw)
