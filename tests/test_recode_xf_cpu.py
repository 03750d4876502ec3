"""The lossless flip, rotate, transpose and MCU crop on the CPU (tests/hostsim/recode_xf_sim.cpp: the plan of jda_recode_images_ex and every
lane of jda_rc_extract_xf and jda_rc_from_coef_xf through the kernels' own code, every load and store held to its allocation, every byte of
the call's coefficients and block words stored exactly once), against the numpy twin of tests/recode_xf_util.py:

* the twin against the third party: Pillow's file of the numpy-turned picture (pictures constant per MCU cell, every operation, every EXIF
  orientation, all three forms), and Pillow's decode of the twin's file against the numpy-turned decode of the source;
* the stages lane by lane: coef and meta = the twin's of the twin-written file, for Pillow's and the written sources;
* whole files byte for byte: recode_ex(src, xform, form, ri) = recode(write_jpeg(twin(decode(src))), form, ri), the right side through
  tests/hostsim/recode_sim.cpp (the plain recode, held to Pillow by tests/test_recode_cpu.py);
* identities, every crop rectangle, the geometry call, every refusal, capacities and bounds;
* the plan and the lanes once more as a program of their own under ASan + UBSan."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from tests import coef_jpeg
from tests import recode_util as U
from tests import recode_xf_util as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A


class Info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "ncomp", "subsample", "bpp", "jpeg_type", "restart_interval", "orientation", "mcu_w", "mcu_h", "mcus_x",
                                         "mcus_y", "scan_offset", "blocks_per_mcu", "has_thumb", "thumb_w", "thumb_h", "thumb_offset", "scan_start", "scan_end", "approx")]


class Xform(C.Structure):
    _fields_ = [("op", C.c_int32), ("flags", C.c_int32), ("mcu_rect", C.c_int32 * 4)]


def xform_of(t):
    x = Xform()
    x.op, x.flags = t[0], t[1]
    for k in range(4):
        x.mcu_rect[k] = t[2 + k]
    return x


@pytest.fixture(scope="module")
def sims(built_checkers):
    xf = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_recodexfsim.so"))
    head = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    tail = [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p]
    xf.recodexfsim_files.argtypes = head + [C.POINTER(Xform)] + tail
    xf.recodexfsim_geometry.argtypes = [C.POINTER(Info), C.POINTER(Xform), C.POINTER(Info)]
    xf.recodexfsim_bound.argtypes = [C.POINTER(Info), C.POINTER(Xform), C.c_int, C.c_int, C.POINTER(C.c_int64)]
    plain = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_recodesim.so"))
    plain.recodesim_files.argtypes = head + tail
    return xf, plain


def run(sims, files, forms, ris, xforms=None, sparse=None, caps=None, use_plain=False):
    """-> dict(rc, files (None: not written), nbytes, status, coef (blocks, 64) int16, meta, bad, info); xforms: None (the plain simulator with
    use_plain, else a NULL pointer), or a tuple of recode_xf_util.xform a job"""
    n = len(files)
    caps = list(caps) if caps is not None else [1 << 20] * n
    offs = np.concatenate([[0], np.cumsum([(c + 63) & ~63 for c in caps])]).astype(np.int64)
    blob = np.full(int(offs[-1]) + 64, GUARD, dtype=np.uint8)
    base = blob.ctypes.data
    import jpegdec_amd as J
    nb_max = 1
    for f in files:
        d = J.parse(f)
        nb_max += max(d["mcus_x"] * d["mcus_y"] * d["blocks_per_mcu"], 0)
    coef, meta = np.full((nb_max, 64), 0x5A5A, np.int16), np.full(nb_max, 0x5A5A5A5A, np.uint32)
    bad, info = np.zeros(n, np.uint32), np.zeros(6, np.uint64)
    nbytes, status = (C.c_int64 * n)(), (C.c_int32 * n)(*([-1] * n))
    hdr_len = C.c_int64(0)
    head = (n, (C.c_char_p * n)(*files), (C.c_int32 * n)(*[len(f) for f in files]), (C.c_int32 * n)(*[U.FORM_ID[f] if isinstance(f, str) else f for f in forms]),
            (C.c_int32 * n)(*[-1 if r is None else r for r in ris]), None if sparse is None else (C.c_int32 * n)(*sparse))
    tail = ((C.c_void_p * n)(*[base + int(o) for o in offs[:n]]), (C.c_int64 * n)(*caps), nbytes, status, coef.ctypes.data, meta.ctypes.data, bad.ctypes.data,
            None, 0, C.byref(hdr_len), info.ctypes.data)
    if use_plain:
        assert xforms is None
        rc = sims[1].recodesim_files(*head, *tail)
    else:
        rc = sims[0].recodexfsim_files(*head, None if xforms is None else (Xform * n)(*[xform_of(t) for t in xforms]), *tail)
    out = []
    for i in range(n):
        lo, hi = int(offs[i]), int(offs[i + 1])
        written = status[i] == 0 and 0 < nbytes[i] <= caps[i]
        out.append(blob[lo:lo + nbytes[i]].tobytes() if written else None)
        assert (blob[lo + (nbytes[i] if written else 0):hi] == GUARD).all(), "a byte behind the file, or of a file that is not written"
    nb = int(info[0])
    assert (coef[nb:] == 0x5A5A).all() and (meta[nb:] == 0x5A5A5A5A).all()
    return dict(rc=rc, files=out, nbytes=list(nbytes), status=list(status), coef=coef[:nb], meta=meta[:nb], bad=bad, info=[int(v) for v in info])


def reference(sims, jobs, forms, ris):
    """recode(write_jpeg(twin(decode(src))), form, ri) of every job (src, op, rect, trim) through the PLAIN simulator; None where the twin refuses"""
    twins = [X.twin_file(src, op, rect, trim) for src, op, rect, trim in jobs]
    keep = [i for i, t in enumerate(twins) if t is not None]
    out = [None] * len(jobs)
    if keep:
        r = run(sims, [twins[i] for i in keep], [forms[i] for i in keep], [ris[i] for i in keep], use_plain=True)
        assert r["rc"] == 0 and r["status"] == [0] * len(keep), r["status"]
        for i, f in zip(keep, r["files"]):
            out[i] = f
    return out, twins


def check_jobs(sims, jobs, form="baseline", ri=0, arrays=True):
    """one _ex call over jobs (src, op, rect, trim): the files are the reference's, and (a baseline call) coef and meta the twin's of the twin-written files"""
    forms, ris = [form] * len(jobs), [ri] * len(jobs)
    want, twins = reference(sims, jobs, forms, ris)
    r = run(sims, [j[0] for j in jobs], forms, ris, [X.xform(op, rect, trim) for _, op, rect, trim in jobs])
    assert r["rc"] == 0 and not r["bad"].any()
    assert r["status"] == [0 if w is not None else U.UNSUPPORTED for w in want], r["status"]
    for k, (g, w) in enumerate(zip(r["files"], want)):
        assert g == w, ("job", k, jobs[k][1:])
    if arrays and any(t is not None for t in twins):
        cs, ms = zip(*[U.twin_of(t) for t in twins if t is not None])
        assert np.array_equal(r["coef"], np.concatenate(cs)), "coef"
        assert np.array_equal(r["meta"], np.concatenate(ms)), "meta"
    return r


# ---- 1. the twin against the third party ------------------------------------------------------------------------------------------
UNIFORM = dict(qtables=[[3] * 64, [5] * 64])       # (symmetric tables: Pillow's file of a transposed picture has the transposed file's DQT segments)


@pytest.mark.parametrize("sampling", ("gray", "4:4:4", "4:2:0", "4:2:2"))
def test_pillows_file_of_the_turned_picture(sims, sampling):
    """5 x 3 MCU cells, a colour a cell: the recode of Pillow's file under every operation is Pillow's file of the numpy-turned picture, in all three forms"""
    pytest.importorskip("PIL")
    pic = X.cell_picture(sampling)
    ops = [op for op in X.OPS if sampling != "4:2:2" or op not in X.TRANSPOSING]
    for form, extra in (("baseline", {}), ("optimize", dict(optimize=True)), ("progressive", dict(progressive=True))):
        for quality in ({}, UNIFORM):
            use = [op for op in ops if quality or op not in X.TRANSPOSING]      # (the standard tables are not symmetric)
            kw = dict(quality) if quality else dict(q=75)
            if sampling == "gray" and quality:
                kw = dict(qtables=UNIFORM["qtables"][:1])
            src = X.pillow_save(pic, sampling, **kw)
            assert len(src) >= 256
            ri = None if form == "progressive" else 0
            r = run(sims, [src] * len(use), [form] * len(use), [ri] * len(use), [X.xform(op) for op in use])
            assert r["rc"] == 0 and r["status"] == [0] * len(use), r["status"]
            for op, got in zip(use, r["files"]):
                want = X.pillow_save(X.pixel_turn(pic, op), sampling, **kw, **extra)
                U.is_pillow(got, want, form)


def test_exif_orientations_come_out_upright(sims):
    """a picture carrying each orientation 1..8 comes out as ImageOps.exif_transpose turns it, and without the tag"""
    pytest.importorskip("PIL")
    from PIL import ImageOps
    import jpegdec_amd as J
    for sampling in ("gray", "4:4:4", "4:2:0"):
        pic = X.cell_picture(sampling, seed=2)
        kw = dict(qtables=UNIFORM["qtables"][:1]) if sampling == "gray" else dict(UNIFORM)
        srcs = [X.pillow_save(pic, sampling, exif_orientation=o, **kw) for o in range(1, 9)]
        assert [J.parse(s)["orientation"] for s in srcs] == list(range(1, 9))
        r = run(sims, srcs, ["baseline"] * 8, [0] * 8, [X.xform("exif")] * 8)
        assert r["rc"] == 0 and r["status"] == [0] * 8
        for o, src, got in zip(range(1, 9), srcs, r["files"]):
            # (the upright PICTURE is exif_transpose's of the array: Pillow's own decode of the file plays no part)
            turned = np.asarray(ImageOps.exif_transpose(_with_orientation(pic, o)))
            assert np.array_equal(turned, X.pixel_turn(pic, X.EXIF_OP[o])), "the mapping of the orientation to the operation"
            U.is_pillow(got, X.pillow_save(turned, sampling, **kw), "baseline")
            assert J.parse(got)["orientation"] == 0 and b"Exif" not in got


def _with_orientation(pic, o):
    from PIL import Image
    im = Image.fromarray(pic)
    im.getexif()[274] = o
    return im


# ---- 2. the twin against pixels ---------------------------------------------------------------------------------------------------
def test_twin_against_pixels():
    """Pillow's decode of the twin's file against the numpy-turned Pillow decode of the source.  The limit is derived, not measured: jidctint
    is of IEEE-1180 class, peak error 1 on each side -> <= 2 for a gray sample, <= 6 for a colour channel behind YCbCr -> RGB.
    Measured maxima on these pictures (64 x 48 noise and smooth, quality 75): see DESIGN.md 5.15."""
    pytest.importorskip("PIL")
    from PIL import Image
    worst = {}
    for kind in ("noise", "smooth"):
        for sampling in ("gray", "4:4:4", "4:2:0", "4:2:2"):
            src = U.pillow_files(kind, 64, 48, sampling)["baseline"]
            a = np.asarray(Image.open(io.BytesIO(src))).astype(np.int64)
            for op in X.OPS:
                t = X.twin_file(src, op)
                if sampling == "4:2:2" and op in X.TRANSPOSING:
                    assert t is None
                    continue
                b = np.asarray(Image.open(io.BytesIO(t))).astype(np.int64)
                want = X.pixel_turn(a, op)
                assert b.shape == want.shape
                d = int(np.abs(b - want).max())
                key = ("gray" if sampling == "gray" else "colour", op)
                worst[key] = max(worst.get(key, 0), d)
                print(kind, sampling, op, d)
                assert d <= (2 if sampling == "gray" else 6), (kind, sampling, op, d)
    print(sorted(worst.items()))


# ---- 3. the stages lane by lane ---------------------------------------------------------------------------------------------------
def _pillow(kind, w, h, sampling, name="baseline"):
    return U.pillow_files(kind, w, h, sampling)[name]


def _ops_for(sampling):
    return [op for op in X.OPS if sampling != "4:2:2" or op not in X.TRANSPOSING]


def test_stages_small_shapes(sims):
    """one MCU of each layout, 1 x N and N x 1 MCUs: every operation of a layout in one call"""
    pytest.importorskip("PIL")
    shapes = [("noise", 8, 8, "gray"), ("noise", 8, 8, "4:4:4"), ("noise", 16, 8, "4:2:2"), ("noise", 16, 16, "4:2:0"),
              ("noise", 16 * 5, 16, "4:2:0"), ("noise", 16, 16 * 5, "4:2:0"), ("noise", 8 * 7, 8, "gray"), ("noise", 8, 8 * 7, "4:4:4"), ("noise", 16, 8 * 4, "4:2:2")]
    jobs = []
    for s in shapes:
        src = _pillow(*s)
        if len(src) < 256:
            src = _pillow(s[0], s[1], s[2], s[3], "restart")
        assert len(src) >= 256, s
        jobs += [(src, op, None, False) for op in _ops_for(s[3])]
    r = check_jobs(sims, jobs)
    assert r["info"][2:] == [0, 0, 1, 0]


def test_stages_workgroup_straddles_jobs_and_kinds(sims):
    """136 x 88 at 4:2:0 (324 blocks: a workgroup of 256 lanes straddles jobs), neighbours with different operations and source kinds"""
    pytest.importorskip("PIL")
    base, prog = _pillow("noise", 136, 88, "4:2:0"), _pillow("noise", 136, 88, "4:2:0", "progressive")
    jobs = [(base, "rot90", None, True), (prog, "flip_h", None, True), (base, "none", None, False), (prog, "transverse", None, True), (base, "flip_v", (1, 1, 5, 3), False),
            (prog, "rot270", (0, 2, 9, 4), True), (base, "transpose", None, False), (prog, "none", None, False), (base, "rot180", None, True)]
    r = check_jobs(sims, jobs)
    assert r["info"][2:] == [0, 0, 1, 1], "one launch of each _xf stage, none of the plain ones"
    for form in ("optimize", "progressive"):
        check_jobs(sims, jobs, form, None if form == "progressive" else 0, arrays=False)


@pytest.mark.parametrize("sampling", ("gray", "4:4:4", "4:2:2", "4:2:0"))
def test_stages_ragged_size_with_and_without_trim(sims, sampling):
    pytest.importorskip("PIL")
    src = _pillow("smooth" if sampling == "4:4:4" else "noise", 333, 217, sampling)
    jobs = [(src, op, None, trim) for op in X.OPS for trim in (False, True)]
    r = check_jobs(sims, jobs)
    refused = [op for (_, op, _, trim), st in zip(jobs, r["status"]) if st != 0 and not trim]
    assert refused == [op for op in X.OPS if X.MIRRORED[op] or (sampling == "4:2:2" and op in X.TRANSPOSING)], "without TRIM: jpegtran's -perfect"
    for (_, op, _, trim), f in zip(jobs, r["files"]):
        if f is not None and trim and X.MIRRORED[op]:
            d = U.decode_any(f)
            hs, vs = coef_jpeg.LUMA_HV[sampling]
            w, h = (d["height"], d["width"]) if op in X.TRANSPOSING else (d["width"], d["height"])
            assert (w == 333 // (8 * hs) * 8 * hs) == ("x" in X.MIRRORED[op]) and (h == 217 // (8 * vs) * 8 * vs) == ("y" in X.MIRRORED[op])


def test_stages_written_sources(sims):
    """coefficient 63, ZRL chains, category 10, custom tables, distinct asymmetric quantisers (a missing table transpose shows), 16-bit
    entries, ids 2 and 3 -- and a written progressive source through from_coef_xf"""
    names = [k for k in sorted(U.written_specs()) if k.startswith("huff_custom_")] + ["three_quantisers", "quant16", "ids_2_and_3"]
    jobs = []
    for k in names:
        src = U.written(k)
        jobs += [(src, op, None, True) for op in _ops_for(U.decode_any(src)["sampling"]) if op != "none"]
    prog = U.written_progressive()
    jobs += [(prog, op, None, True) for op in X.OPS]
    r = check_jobs(sims, jobs)
    assert r["info"][2:] == [0, 0, 1, 1]
    # the quantisers of a transposed job are the source's transposed: read back by the suite's own decoder
    src = U.written("three_quantisers")
    got = r["files"][[j[:2] for j in jobs].index((src, "transpose"))]
    a, b = U.decode_any(src), U.decode_any(got)
    assert b["quant_ids"] == a["quant_ids"]
    for i in a["quant"]:
        t = X.from_grid(X.to_grid(np.array(a["quant"][i]).reshape(1, 1, 64)).transpose(0, 1, 3, 2))[0, 0]
        assert list(b["quant"][i]) == list(t) and (i == 1 or list(t) != list(a["quant"][i]))
    for form in ("optimize", "progressive"):
        colour = [j for j in jobs if U.decode_any(j[0])["sampling"] != "gray"]
        check_jobs(sims, colour, form, None if form == "progressive" else 0, arrays=False)
        check_jobs(sims, [j for j in jobs if j not in colour], form, None if form == "progressive" else 0, arrays=False)


# ---- 4. whole files, byte for byte ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", U.FORMS)
def test_whole_files_every_operation_form_and_restart_target(sims, form):
    pytest.importorskip("PIL")
    srcs = [_pillow("noise", 136, 88, "4:2:0", "restart"), _pillow("smooth", 17, 9, "4:2:0"), U.written("huff_custom_gray"), U.written("three_quantisers"),
            _pillow("noise", 64, 48, "4:2:2"), U.written_progressive()]
    for ri in ((None,) if form == "progressive" else U.RESTART_TARGETS):
        for gray in (False, True):
            jobs = [(s, op, None, True) for s in srcs if (U.decode_any(s)["sampling"] == "gray") == gray for op in X.OPS]
            check_jobs(sims, jobs, form, ri, arrays=False)


def test_whole_files_from_restart_sources(sims):
    """sources with an interval of 1, of an MCU row and one that does not divide the MCU count: the target's own interval is the source's"""
    for form in ("baseline", "optimize"):
        for ri in U.RESTART_TARGETS:
            jobs = [(f, op, None, True) for f, _, _ in U.restart_sources() for op in ("flip_h", "rot90", "transverse")]
            r = check_jobs(sims, jobs, form, ri, arrays=False)
            for (src, *_), f in zip(jobs, r["files"]):
                assert U.decode_any(f)["restart_interval"] == (U.decode_any(src)["restart_interval"] if ri is None else ri)


# ---- 5. identities ----------------------------------------------------------------------------------------------------------------
def _chain(sims, src, ops, form="baseline"):
    for op in ops:
        r = run(sims, [src], ["baseline"], [0], [X.xform(op)])
        assert r["rc"] == 0 and r["status"] == [0], (op, r["status"])
        src = r["files"][0]
    if form != "baseline":
        src = run(sims, [src], [form], [None if form == "progressive" else 0], None)["files"][0]
    return src


def test_identities(sims):
    pytest.importorskip("PIL")
    for src in (_pillow("noise", 64, 48, "4:2:0"), _pillow("noise", 48, 64, "4:4:4"), U.written("three_quantisers"), U.written("huff_custom_gray")):
        for form in U.FORMS:
            ri = None if form == "progressive" else 0
            plain = run(sims, [src], [form], [ri], use_plain=True)
            assert plain["rc"] == 0 and plain["status"] == [0]
            none = run(sims, [src, src], [form] * 2, [ri] * 2, [X.xform("none")] * 2)
            assert none["files"] == plain["files"] * 2 and none["info"][2:] == [1, 0, 0, 0], "NONE: the plain stage, the plain bytes"
            null = run(sims, [src], [form], [ri], None)
            assert null["files"] == plain["files"] and null["info"][2:] == [1, 0, 0, 0]
        want = run(sims, [src], ["baseline"], [0], use_plain=True)["files"][0]
        for ops in (("flip_h", "flip_h"), ("flip_v", "flip_v"), ("transpose", "transpose"), ("rot90",) * 4, ("rot90", "rot270"), ("rot180", "rot180"), ("transverse", "transverse")):
            assert _chain(sims, src, ops) == want, ops
        assert _chain(sims, src, ("rot90",)) == _chain(sims, src, ("transpose", "flip_h"))
        assert _chain(sims, src, ("rot270",)) == _chain(sims, src, ("transpose", "flip_v"))
        assert _chain(sims, src, ("transverse",)) == _chain(sims, src, ("transpose", "rot180"))


# ---- 6. crop ----------------------------------------------------------------------------------------------------------------------
def _rects(cx, cy):
    return [(x, y, w, h) for x in range(cx) for w in range(1, cx - x + 1) for y in range(cy) for h in range(1, cy - y + 1)]


def _frame_size(f):
    fh = U.frame_header(f)
    return int.from_bytes(fh[7:9], "big"), int.from_bytes(fh[5:7], "big")


@pytest.mark.parametrize("sampling", ("gray", "4:4:4", "4:2:2", "4:2:0"))
def test_every_crop_rectangle(sims, sampling):
    """every rectangle of a 4 x 3-MCU image, alone and with ROT_90; the geometry call = the file's frame header"""
    hs, vs = coef_jpeg.LUMA_HV[sampling]
    src = coef_jpeg.write_jpeg(**U._small(sampling, {0: list(range(2, 66)), 1: list(range(70, 6, -1))}, seed=31, w=32 * hs, h=24 * vs))
    rects = _rects(4, 3)
    assert len(rects) == 60
    for op in ("none", "rot90"):
        jobs = [(src, op, r, False) for r in rects]
        r = check_jobs(sims, jobs)
        assert (r["status"] == [0] * 60) == (sampling != "4:2:2" or op == "none")
        _geometry_is_the_frame_header(sims, jobs, r["files"])


def _geometry_is_the_frame_header(sims, jobs, files):
    import jpegdec_amd as J
    for (src, op, rect, trim), f in zip(jobs, files):
        d = J.parse(src)
        assert d.pop("status") == 0
        out = Info()
        rc = sims[0].recodexfsim_geometry(C.byref(Info(**d)), C.byref(xform_of(X.xform(op, rect, trim))), C.byref(out))
        if f is None:
            assert rc == U.UNSUPPORTED
            continue
        g = J.parse(f)
        assert rc == 0 and (out.width, out.height, out.mcus_x, out.mcus_y) == (g["width"], g["height"], g["mcus_x"], g["mcus_y"]) and (out.width, out.height) == _frame_size(f)
        assert (out.subsample, out.ncomp, out.mcu_w, out.mcu_h, out.orientation) == (d["subsample"], d["ncomp"], d["mcu_w"], d["mcu_h"], 0)


def test_crop_at_a_ragged_size(sims):
    """the last column and row of a ragged image: the partial MCUs travel with their blocks where unmirrored, and are trimmed or refused where mirrored"""
    pytest.importorskip("PIL")
    for sampling in ("gray", "4:2:0", "4:2:2"):
        hs, vs = coef_jpeg.LUMA_HV[sampling]
        w, h = 8 * hs * 3 + 5, 8 * vs * 2 + 3
        src = coef_jpeg.write_jpeg(**U._small(sampling, {0: list(range(2, 66)), 1: [9] * 64}, seed=33, w=w, h=h))
        rects = [(3, 0, 1, 3), (0, 2, 4, 1), (3, 2, 1, 1), (2, 1, 2, 2), (0, 0, 4, 3), (0, 0, 3, 2)]
        jobs = [(src, op, r, trim) for r in rects for op in _ops_for(sampling) for trim in (False, True)]
        r = check_jobs(sims, jobs)
        _geometry_is_the_frame_header(sims, jobs, r["files"])
        by = {(j[1], j[2], j[3]): f for j, f in zip(jobs, r["files"])}
        assert _frame_size(by[("none", (3, 0, 1, 3), False)]) == (5, h)
        assert _frame_size(by[("none", (3, 2, 1, 1), False)]) == (5, 3)
        assert by[("flip_h", (3, 2, 1, 1), True)] is None, "trimmed to nothing"
        assert by[("flip_h", (2, 1, 2, 2), False)] is None and _frame_size(by[("flip_h", (2, 1, 2, 2), True)]) == (8 * hs, 8 * vs + 3)
        assert _frame_size(by[("rot180", (0, 0, 3, 2), False)]) == (24 * hs, 16 * vs), "an aligned region of a ragged image needs no TRIM"


# ---- 7. refusals and bounds -------------------------------------------------------------------------------------------------------
def test_refusals(sims):
    pytest.importorskip("PIL")
    good = U.written("three_quantisers")
    c422 = U.written("huff_custom_c422")
    # 4:2:2 with each transposing operation; the others run
    r = run(sims, [c422] * 8, ["baseline"] * 8, [0] * 8, [X.xform(op, None, True) for op in X.OPS])
    assert r["rc"] == 0 and r["status"] == [U.UNSUPPORTED if op in X.TRANSPOSING else 0 for op in X.OPS]
    # ragged mirrored axes without TRIM; trim to nothing
    ragged = _pillow("smooth", 17, 9, "4:2:0")
    ops = ["flip_h", "flip_v", "rot90", "rot270", "rot180", "transverse", "transpose", "none"]
    r = run(sims, [ragged] * 8, ["baseline"] * 8, [0] * 8, [X.xform(op) for op in ops])
    assert r["rc"] == 0 and r["status"] == [U.UNSUPPORTED] * 6 + [0, 0]
    r = run(sims, [ragged] * 8, ["baseline"] * 8, [0] * 8, [X.xform(op, None, True) for op in ops])
    # (17 x 9 at 4:2:0: 2 x 1 MCUs, both axes ragged: x trims to one MCU, y to nothing)
    assert r["status"] == [0, U.UNSUPPORTED, U.UNSUPPORTED, 0, U.UNSUPPORTED, U.UNSUPPORTED, 0, 0]
    # 4:4:0, Adobe, a bad MCU, range-rule blocks: each as without a transform, the rest of the call untouched
    ref = U.refused()
    names = sorted(ref)
    files = [good] + [ref[k][0] for k in names] + [good]
    for form in U.FORMS:
        ri = None if form == "progressive" else 0
        r = run(sims, files, [form] * len(files), [ri] * len(files), [X.xform("flip_v", None, True)] * len(files))      # (24 x 16: no block is trimmed away)
        assert r["rc"] == 0 and r["status"] == [0] + [ref[k][1] for k in names] + [0], (form, r["status"])
        assert [bool(b) for b in r["bad"]] == [False] + [k in ("ac_1024", "dc_1024", "dc_minus_1025") for k in names] + [False]
        assert all(g is None for g in r["files"][1:-1]) and r["nbytes"][1:-1] == [0] * len(names)
        assert r["files"][0] == r["files"][-1] == reference(sims, [(good, "flip_v", None, True)], [form], [ri])[0][0]
    # a bad-MCU source is refused whatever the region: the check stays on the whole source
    r = run(sims, [ref["bad_mcu"][0]], ["baseline"], [0], [X.xform("none", (0, 0, 1, 1))])
    assert r["rc"] == 0 and r["status"] == [U.DECODE_ERROR]
    # a sparse coefficient image
    prog = U.written_progressive()
    r = run(sims, [prog, good], ["baseline"] * 2, [0, 0], [X.xform("flip_h", None, True)] * 2, sparse=[1, 0])
    assert r["rc"] == 0 and r["status"] == [U.UNSUPPORTED, 0] and r["files"][0] is None


def test_call_level_argument_errors(sims):
    good = U.written("three_quantisers")          # 24 x 16 at 4:4:4: 3 x 2 MCUs
    ok = X.xform("flip_h")
    bad = [(9, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0), (1, -1, 0, 0, 0, 0), (0, 0, -1, 0, 1, 1), (0, 0, 0, -1, 1, 1), (0, 0, 0, 0, -1, 1), (0, 0, 0, 0, 1, -1),
           (0, 0, 3, 0, 1, 1), (0, 0, 0, 2, 1, 1), (0, 0, 1, 0, 3, 1), (0, 0, 0, 1, 1, 2), (0, 0, 0, 0, 0, 2), (0, 0, 0, 0, 2, 0), (0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0),
           (0, 0, 0, 0, 0x7FFFFFFF, 1), (0, 0, 2, 0, 0x7FFFFFFF, 1)]
    for t in bad:
        for xs in ([t, ok], [ok, t]):
            r = run(sims, [good] * 2, ["baseline"] * 2, [0] * 2, xs)
            assert r["rc"] == U.INVALID_PARAMETER and r["files"] == [None, None], t
    for t in ((0, 0, 0, 0, 3, 2), (0, 0, 2, 1, 1, 1), (8, 1, 0, 0, 0, 0)):
        assert run(sims, [good], ["baseline"], [0], [t])["rc"] == 0, t
    # .. and the call's other rules hold with transforms: forms mixed, a progressive target with an interval
    assert run(sims, [good] * 2, ["baseline", "progressive"], [0, None], [ok, ok])["rc"] == U.INVALID_PARAMETER
    assert run(sims, [good], ["progressive"], [4], [ok])["rc"] == U.INVALID_PARAMETER


@pytest.mark.parametrize("form", U.FORMS)
def test_capacity_a_byte_short_and_bounds(sims, form):
    import jpegdec_amd as J
    files = [U.written("three_quantisers"), U.written("quant16"), U.written("huff_custom_c420"), U.written("quant16_gray")]
    if form == "progressive":
        files = files[:3]
    n = len(files)
    xs = [X.xform("rot90", None, True), X.xform("flip_h", (0, 0, 1, 1)), X.xform("transverse", None, True), X.xform("rot270", None, True)][:n]
    ris = [None if form == "progressive" else 0] * n
    r = run(sims, files, [form] * n, ris, xs)
    assert r["rc"] == 0 and r["status"] == [0] * n
    caps = list(r["nbytes"])
    caps[1] -= 1
    again = run(sims, files, [form] * n, ris, xs, caps=caps)
    assert again["rc"] == 0 and again["status"] == [0, U.ERROR_MEMORY] + [0] * (n - 2) and again["nbytes"] == r["nbytes"], "the size it needs, and no byte of it"
    assert again["files"][0] == r["files"][0] and again["files"][1] is None and again["files"][2:] == r["files"][2:]
    for f, x, nb in zip(files, xs, r["nbytes"]):
        d = J.parse(f)
        assert d.pop("status") == 0
        for ri in ((None,) if form == "progressive" else (0, 1)):
            b = C.c_int64()
            assert sims[0].recodexfsim_bound(C.byref(Info(**d)), C.byref(xform_of(x)), U.FORM_ID[form], -1 if ri is None else ri, C.byref(b)) == 0
            got = run(sims, [f], [form], [ri], [x])
            assert got["status"] == [0] and 0 < got["nbytes"][0] <= b.value
    b = C.c_int64(7)
    d = J.parse(U.written("huff_custom_c422"))
    d.pop("status")
    assert sims[0].recodexfsim_bound(C.byref(Info(**d)), C.byref(xform_of(X.xform("transpose"))), 0, 0, C.byref(b)) == U.UNSUPPORTED and b.value == 0
    assert sims[0].recodexfsim_bound(C.byref(Info(**d)), C.byref(xform_of((9, 0, 0, 0, 0, 0))), 0, 0, C.byref(b)) == U.INVALID_PARAMETER
    assert sims[0].recodexfsim_bound(C.byref(Info(**d)), None, 0, 0, C.byref(b)) == 0 and b.value > 0


def test_sanitizers():
    """tests/hostsim/recode_xf_main.cpp: a program of its own (make recodexfasan), nothing preloaded"""
    subprocess.run(["make", "recodexfasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    golden = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "recode_xf_asan")] + [os.path.join(golden, n + ".jpg") for n in
                       ("c420_333x217", "c444_8x8_q30", "gray_64x64_rst3", "c422_333x217", "c444_384x192_q100_rst7", "p420_200x120", "pgray_100x100", "c420_16x16")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"recode_xf_asan ok" in r.stdout, r.stdout[-2000:]
