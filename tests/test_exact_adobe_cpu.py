"""The colour models of the libjpeg-exact decode (JDA_EXACT_COLOUR_MODELS) without a GPU:
(a) the numpy twin (tests/exact_adobe_util.py) = Pillow -- np.asarray(im) in mode CMYK and convert("RGB") -- over every accepted layout x
    {CMYK, YCCK, no Adobe segment} x sizes, every file inside the comparison window, both clamps of both conversions met; the
    three-component variants (Adobe transform 0 / 1, JFIF + Adobe, ids 'R','G','B', neither) at 1, 1/2, 1/4, 1/8;
(b) jda_exact_probe over every row of jdapimin.c's rule and over refused layouts;
(c) jda_coef_prepare's coefficients = the suite's own entropy decoder, sequential and progressive, restart markers, a scan per component;
(d) the kernels' lanes (tests/hostsim/exact_adobe_sim.cpp) = the C row-major twin = the numpy twin, whole and clipped, every access inside its
    allocation, every visible byte stored exactly once; jda_exact_check's answers as they were;
(e) the same as a program of its own under ASan + UBSan; (f) what still refuses a four-component image."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpegdec_amd as J
from tests import coef_jpeg
from tests import exact_adobe_util as A
from tests import exact_scaled_util as S
from tests import exact_util as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUCCESS, INVALID_PARAMETER, DECODE_ERROR, UNSUPPORTED = 0, 1, 2, 3
COLOUR_LAYOUTS = ("4:4:4", "4:2:0", "4:2:2", "4:4:0")


@pytest.fixture(scope="module")
def sim():
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_exactadobesim.so"))
    lib.exactadobesim_run.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.exactadobesim_plan.argtypes = [C.c_int] * 9 + [C.c_void_p]
    return lib


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_four_component_twin_is_pillow(sampling):
    files = A.grid4(sampling)
    models, k_samplings = set(), set()
    lo, hi, ylo, yhi = 255, 0, 0, 255
    for name, f in files:
        t = A.twin4(f)
        assert A.in_window(t), (name, t["range"])                       # (no file is left out: every one is inside the window)
        assert np.array_equal(t["cmyk"], A.pillow(f)), name
        assert np.array_equal(t["rgb"], A.pillow(f, "RGB")), name
        models.add(A.model(f))
        k_samplings.add(A.header(f)["hv"][3] == A.header(f)["hv"][0])
        lo, hi = min(lo, int(t["rgb"].min())), max(hi, int(t["rgb"].max()))
        if A.model(f) == A.YCCK:                                        # jdcolor.c's sums in front of their clamp
            y, cb, cr = (t["raw"][..., c].astype(np.int64) for c in range(3))
            r, b = y + ((91881 * (cr - 128) + 32768) >> 16), y + ((116130 * (cb - 128) + 32768) >> 16)
            ylo, yhi = min(ylo, int(r.min()), int(b.min())), max(yhi, int(r.max()), int(b.max()))
    assert models == {A.CMYK, A.YCCK}
    assert k_samplings == ({True} if sampling == "4:4:4" else {True, False})
    assert (lo, hi) == (0, 255) and ylo < 0 and yhi > 255               # both clamps of cmyk2rgb and of the YCCK conversion


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_three_component_variants_are_pillow(sampling):
    seen = set()
    for name, f, model in A.grid3(sampling):
        assert A.model(f) == model, name
        seen.add((name.split("_")[0], model))
        w, h = A.header(f)["width"], A.header(f)["height"]
        for s in S.SCALES:
            if s > 1 and not S.forcible(w, h, s):
                continue
            t = A.twin3(f, s)
            assert A.in_window(t), (name, s)
            want = A.pillow(f, "RGB") if s == 1 else S.pillow_scaled(f, s)
            assert np.array_equal(t["rgb"], want), (name, s)
        if model == A.RGB:                                              # .. and an RGB-coded file read as YCbCr gives other pixels
            assert not np.array_equal(X.twin(f)["rgb"], A.pillow(f, "RGB")), name
    assert seen == {("adobe0", A.RGB), ("adobe1", A.YCBCR), ("both", A.YCBCR), ("ids", A.RGB), ("none", A.YCBCR)}


def test_probe_over_the_rule_table():
    rows = []
    g = dict(X.grid("gray"))
    rows.append((g["baseline_33x31_q90"], A.GRAY, 1, 0))
    for variant, model in A.RGB3_MODEL.items():
        rows.append((A.pillow_rgb3(33, 31, "4:2:0", 90, variant), model, 3, 2))
    rows.append((dict(X.grid("4:2:2"))["baseline_33x31_q90"], A.YCBCR, 3, 3))          # JFIF alone
    rows.append((A.pillow_cmyk(33, 31, "4:2:0", 90, False, "cmyk"), A.CMYK, 4, 2))
    rows.append((A.pillow_cmyk(33, 31, "4:2:2", 90, True, "ycck"), A.YCCK, 4, 3))
    rows.append((A.pillow_cmyk(33, 31, "4:4:4", 90, False, "bare"), A.CMYK, 4, 1))
    rows.append((A.written4(33, 31, (1, 2), True, adobe=2), A.YCCK, 4, 4))
    f = A.pillow_cmyk(33, 31, "4:2:0", 90)
    i = f.index(b"Adobe")
    rows.append((f[:i + 11] + b"\x01" + f[i + 12:], A.YCCK, 4, 2))                       # (any transform but 0: YCCK)
    f3 = A.pillow_rgb3(33, 31, "4:4:4", 90, "adobe0")
    i = f3.index(b"Adobe")
    rows.append((f3[:i + 11] + b"\x02" + f3[i + 12:], A.YCBCR, 3, 1))                    # (three components, any transform but 0: YCbCr)
    for f, model, ncomp, layout in rows:
        p = J.exact_probe(f)
        h = A.header(f)
        assert (p["colour_model"], p["ncomp"], p["layout"], p["decodable"]) == (model, ncomp, layout, True), p
        assert (p["width"], p["height"], p["progressive"]) == (h["width"], h["height"], h["sof"] == 0xC2)
        assert (p["jfif"], p["adobe"], p["adobe_transform"], p["component_ids"]) == (h["jfif"], h["adobe"], h["transform"], h["ids"])
        assert p["k_sampling"] == ((h["hv"][3][0] << 4) | h["hv"][3][1] if ncomp == 4 else 0)
        assert A.model(f) == model
    # layouts the decode does not take: K at another sampling than 1x1 or component 0's, a chroma component that is not 1x1
    good = A.written4(33, 31, (2, 2), True)
    sof = good.index(b"\xff\xc0")
    for comp, hv in ((3, 0x21), (3, 0x12), (1, 0x21), (2, 0x12)):
        bad = bytearray(good)
        bad[sof + 11 + 3 * comp] = hv
        p = J.exact_probe(bytes(bad))
        assert p["ncomp"] == 4 and not p["decodable"], (comp, hv)
        assert J.load_library().jda_exact_probe(bytes(bad), len(bad), C.byref(J.binding.ExactFile())) == UNSUPPORTED
        with pytest.raises(J.JdaError) as e:
            J.CoefImage.from_file(bytes(bad))
        assert e.value.code == UNSUPPORTED
    with pytest.raises(J.JdaError):
        J.exact_probe(b"\xff\xd8" + b"\0" * 300)


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_coef_prepare_is_the_suites_decoder(sampling):
    kinds = set()
    for name, f in A.grid4(sampling):
        h = A.header(f)
        img = J.CoefImage.from_file(f)
        try:
            a, k = A.library_blocks(A.decode4(f))
            assert img.info.ncomp == 4 and np.array_equal(img.coefficients(), a), name
            k3 = img.component3()
            assert k3.info.ncomp == 1 and np.array_equal(k3.coefficients(), k), name
            # (dense only: no sparse form, and the calls of a file of one or three components refuse it)
            assert J.load_library().jda_coef_image_sparse_status(img.handle) == UNSUPPORTED and img.sparse_bytes() == 0
            with pytest.raises(J.JdaError):
                img.sparse()
        finally:
            img.close()
        kinds.add((h["sof"], f.count(b"\xff\xda") > 1 and h["sof"] != 0xC2, b"\xff\xdd" in f))
        for call in (J.CoefImage, J.PreparedImage):                     # jda_progressive_prepare, jda_prepare: their refusals stand
            with pytest.raises(J.JdaError):
                call(f)
    if sampling != "4:4:4":
        assert {(0xC0, False, False), (0xC0, True, False), (0xC0, False, True), (0xC1, True, False)} <= kinds, kinds
    if sampling in A.PILLOW_SUB:
        assert any(k[0] == 0xC2 for k in kinds)
    for name, f, model in A.grid3(sampling):
        img = J.CoefImage.from_file(f)
        assert img.component3() is None and np.array_equal(img.coefficients(), X.natural_blocks(f)), name
        if A.header(f)["sof"] == 0xC2:                                  # a progressive file: the image jda_progressive_prepare makes
            old = J.CoefImage(f)
            assert np.array_equal(old.coefficients(), img.coefficients()) and np.array_equal(old.quant()[0], img.quant()[0])
            old.close()
        img.close()


def _run(sim, f, pixel_type, scale=1, clip=None):
    """one file through the lanes -> (rc, surface rows, the C twin's pixels or None, planes bytes, info)"""
    h = A.header(f)
    w, hh = -(-h["width"] // scale), -(-h["height"] // scale)
    pitch = (w * 4 + 15) & ~15
    buf = np.full(pitch * hh + 16, 0x5A, np.uint8)
    off = (-buf.ctypes.data) % 16
    out = buf[off:off + pitch * hh]
    twin = np.zeros((hh, w * 4), np.uint8)
    planes = np.zeros(h["width"] * h["height"] * 4 + 64, np.uint8)
    info = (C.c_int32 * 8)()
    cw, ch = clip or (w, hh)
    rc = sim.exactadobesim_run(f, len(f), pixel_type, scale, out.ctypes.data, pitch, cw, ch, twin.ctypes.data, planes.ctypes.data, info)
    return rc, out.reshape(hh, pitch), (twin if info[7] else None), planes, list(info)


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_lanes_of_colour4(sim, sampling):
    for n, (name, f) in enumerate(A.grid4(sampling)):
        t = A.twin4(f)
        hgt, wid = t["rgb"].shape[:2]
        for pt in (J.RGB8888, J.CMYK8888):
            want = A.surface(t, pt == J.CMYK8888)
            for clip in (None, (max(wid - 3, 1), (hgt + 1) // 2)) if n % 3 == 0 or pt == J.RGB8888 else (None,):
                rc, got, ctwin, planes, info = _run(sim, f, pt, 1, clip)
                assert rc == 0 and info[0] > 0 and info[3] == 0 and info[4] == 0 and info[6] == 0, (name, pt, clip, rc, info)
                assert tuple(info[1:3]) == t["range"] and info[5] == A.model(f)
                cw, ch = clip or (wid, hgt)
                assert np.array_equal(got[:ch, :cw * 4], want[:ch, :cw * 4]) and np.array_equal(ctwin, want), (name, pt, clip)
                assert np.all(got[:, cw * 4:] == 0x5A) and np.all(got[ch:] == 0x5A), (name, pt, clip)
                flat = np.concatenate([p.ravel() for p in t["planes"]])
                assert np.array_equal(planes[:flat.size], flat), name


@pytest.mark.parametrize("sampling", COLOUR_LAYOUTS)
def test_lanes_of_the_rgb_instances(sim, sampling):
    for name, f, model in A.grid3(sampling):
        w, h = A.header(f)["width"], A.header(f)["height"]
        for s in S.SCALES:
            t = A.twin3(f, s)
            rc, got, ctwin, planes, info = _run(sim, f, J.RGB8888, s)
            assert rc == 0 and info[3] == 0 and info[4] == 0 and info[6] == 0 and info[5] == model, (name, s, rc, info)
            want = A.surface(t)
            assert np.array_equal(got[:, :want.shape[1]], want) and np.all(got[:, want.shape[1]:] == 0x5A), (name, s)
            assert s > 1 or np.array_equal(ctwin, want)
        if model == A.RGB:                                              # (component 0 of an RGB-coded file is red, not luma)
            assert _run(sim, f, J.GRAY8)[0] == UNSUPPORTED, name
    # a narrow RGB-coded file: jdsample.c replicates a component of at most two samples
    for w in (3, 4, 5):
        f = A.pillow_rgb3(w, 7, sampling, 90, "ids")
        t = A.twin3(f)
        assert np.array_equal(t["rgb"], A.pillow(f, "RGB")), w
        rc, got, ctwin, planes, info = _run(sim, f, J.RGB8888)
        assert rc == 0 and np.array_equal(got[:, :w * 4], A.surface(t)) and np.array_equal(ctwin, A.surface(t)), w


def test_the_plan(sim):
    out = (C.c_int64 * 16)()
    plan = lambda *a: sim.exactadobesim_plan(*a, out)                  # noqa: E731  (width, height, ncomp, subsample, k_hv, colour, pixel type, scale, baseline image)
    # the K plane: component 0's pitch and rows where it has its sampling, a chroma plane's otherwise; 256-byte alignment
    for sub, (hs, vs) in ((0x11, (1, 1)), (0x22, (2, 2)), (0x21, (2, 1)), (0x12, (1, 2))):
        for k_hv in {0x11, sub}:
            assert plan(333, 217, 4, sub, k_hv, A.CMYK, J.RGB8888, 1, 0) == SUCCESS
            v = list(out)
            full = k_hv == sub
            assert v[:2] == [hs, vs] and v[11] == int(full)
            assert v[12] == (v[2] if full else v[3]) and v[13] == (v[4] if full else v[5])
            assert v[14] == ((333 << 16) | 217 if full else (v[6] << 16) | v[7])
            assert v[10] % 256 == 0 and v[10] == v[9] + ((v[3] * v[5] + 255) & ~255) and v[15] == v[10] + ((v[12] * v[13] + 255) & ~255)
    assert plan(65535, 65535, 4, 0x11, 0x11, A.CMYK, J.RGB8888, 1, 0) == UNSUPPORTED          # (a plane of 2^32 bytes and more)
    for args, want in (((33, 31, 4, 0x22, 0x22, A.YCCK, J.CMYK8888, 1, 0), SUCCESS), ((33, 31, 4, 0x22, 0x22, A.YCCK, J.GRAY8, 1, 0), UNSUPPORTED),
                       ((33, 31, 4, 0x22, 0x22, A.YCCK, J.RGB565_LE, 1, 0), INVALID_PARAMETER), ((33, 31, 4, 0x22, 0x21, A.CMYK, J.RGB8888, 1, 0), UNSUPPORTED),
                       ((33, 31, 4, 0x22, 0x11, A.CMYK, J.RGB8888, 2, 0), UNSUPPORTED), ((33, 31, 4, 0x22, 0x11, A.CMYK, J.RGB8888, 1, 1), UNSUPPORTED),
                       ((33, 31, 4, 0x22, 0x11, A.YCBCR, J.RGB8888, 1, 0), UNSUPPORTED), ((33, 31, 3, 0x22, 0, A.RGB, J.RGB8888, 4, 0), SUCCESS),
                       ((33, 31, 3, 0x22, 0, A.RGB, J.GRAY8, 1, 0), UNSUPPORTED), ((33, 31, 3, 0x22, 0, A.RGB, J.CMYK8888, 1, 0), INVALID_PARAMETER),
                       ((33, 31, 3, 0x22, 0, A.YCBCR, J.GRAY8, 1, 1), SUCCESS), ((33, 31, 1, 0, 0, A.GRAY, J.RGB8888, 8, 0), SUCCESS),
                       ((33, 31, 3, 0x22, 0, A.CMYK, J.RGB8888, 1, 0), UNSUPPORTED), ((33, 31, 1, 0, 0, A.YCBCR, J.RGB8888, 1, 0), UNSUPPORTED)):
        assert plan(*args) == want, args
    # jda_exact_check, the old calls' check, answers as it did
    sim.exactadobesim_old_check.argtypes = [C.c_int] * 6
    for args, want in (((33, 31, 3, 0x22, 1, J.RGB8888), UNSUPPORTED), ((33, 31, 4, 0x22, 0, J.RGB8888), UNSUPPORTED), ((33, 31, 3, 0x22, 0, J.RGB8888), SUCCESS),
                       ((33, 31, 1, 0, 0, J.GRAY8), SUCCESS), ((33, 31, 3, 0x22, 0, J.CMYK8888), INVALID_PARAMETER), ((33, 31, 3, 0x22, 0, J.RGB565_LE), INVALID_PARAMETER)):
        assert sim.exactadobesim_old_check(*args) == want, args


def test_sanitizer_program(tmp_path):
    """the plan, the host scan decoder and the lanes as a program of their own under ASan + UBSan (nothing is loaded into this process)"""
    subprocess.run(["make", "exactadobeasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    files = []
    for sampling in COLOUR_LAYOUTS:
        g = A.grid4(sampling)
        files += [f for name, f in g if "45x53" in name or "3x3" in name or "17x9" in name or "161x17" in name]
    files += [f for name, f, m in A.grid3("4:2:0")][:4] + [f for name, f, m in A.grid3("4:2:2")][:3] + [A.pillow_rgb3(4, 7, "4:2:0", 90, "ids")]
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / ("f%d.jpg" % k)))
        with open(paths[-1], "wb") as fh:
            fh.write(f)
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "exact_adobe_asan")] + paths, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "exact_adobe_asan ok" in r.stdout, r.stdout[-4000:]


def test_exports_and_argument_errors():
    import inspect
    for name in ("exact_probe", "CMYK8888", "EXACT_COLOUR_MODELS", "CS_GRAY", "CS_YCBCR", "CS_RGB", "CS_CMYK", "CS_YCCK"):
        assert hasattr(J, name), name
    assert (J.CS_GRAY, J.CS_YCBCR, J.CS_RGB, J.CS_CMYK, J.CS_YCCK) == (A.GRAY, A.YCBCR, A.RGB, A.CMYK, A.YCCK)
    for fn in (J.exact_decode, J.exact_planes, J.decode_to_host_exact, J.decode_to_tensors):
        assert inspect.signature(fn).parameters["colour_models"].default is False, fn
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    for fn in ("jda_exact_probe", "jda_exact_decode_surfaces_ex", "jda_exact_decode_planes_ex", "jda_decode_to_host_exact_ex"):
        assert "int %s(" % fn in hdr and hasattr(J.load_library(), fn), fn
    for fn in ("jda_coef_prepare", "jda_coef_image_component3"):
        assert fn + "(" in hdr and hasattr(J.load_library(), fn), fn
    lib = J.load_library()
    assert lib.jda_exact_decode_surfaces_ex(None, 1, None, None, None, None, 2, None) == INVALID_PARAMETER      # (a flag the call does not have)
    assert lib.jda_exact_decode_surfaces_ex(None, 1, None, None, None, None, 1, None) == 6                      # JDA_ERROR_NO_DEVICE, as the other calls
    assert lib.jda_exact_decode_planes_ex(None, 1, None, None, None, 4, None) == INVALID_PARAMETER
    with pytest.raises(ValueError):                                     # (refused before torch or the GPU is touched)
        J.decode_to_tensors(None, [], colour_models=True)
    err = C.c_int32(0)
    assert not lib.jda_coef_prepare(b"\xff\xd8" + b"\0" * 300, 302, C.byref(err)) and err.value != 0
