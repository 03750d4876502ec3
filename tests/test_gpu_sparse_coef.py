"""Progressive files at full size through the sparse coefficient form on the GPU: kernel jda_sparse_tiles (every layout's instantiation)
against the oracle, the edge sets of tests/sparse_cases.py in one call that mixes dense and sparse images against the row-major twin,
rectangles in both forms, a pipeline batch and a node batch submitted with SUBMIT_PROGRESSIVE_FULL, and decode_to_tensors(progressive="full").

Every comparison is bit-exact.  Expected pixels: the oracle's canvas of the baseline file (fixtures), of the re-encoded baseline (progressive
files: tests/prog_cases.py, tests/prog_scripts.py), or the twin tests/hostsim/coef_twin.h over the coefficients (sets no baseline stream
carries) -- never the dense kernel's output.  This file sorts before test_gpu_zz_kernel_coverage.py, which holds the process to every kernel
of the code object: (a) below launches all five jda_sparse_tiles instantiations."""
import ctypes as C
import os

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.binding import ImageInfo, Output
from tests import prog_cases as PC, prog_scripts as PS, sparse_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = J.PROGRESSIVE_FULL
FILL = 0x5A
MODES = ((J.RGB8888, 0), (J.RGB565_LE, 0), (J.RGB565_BE, 0), (J.GRAY8, 0), (J.RGB565_LE, J.LUMA_ONLY))      # those of test_gpu_progressive_full.py


def _info(jpeg):
    info = ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    return info


def _counts(before=None):
    now = {k: v for k, v in J.kernel_launch_counts().items() if "jda_sparse_tiles" in k or "jda_coef_tiles" in k}
    if before is None:
        return now
    return {k: v - before.get(k, 0) for k, v in now.items() if v > before.get(k, 0)}


def _decode(ctx, images, pts, opts=None, form=J.COEF_DENSE, rects=None, fill=0):
    """jda_coef_upload_ex per image + ONE jda_coef_decode_surfaces_rect into surfaces pre-filled with `fill`:
    ([(canvas, geometry)], [the form resident for each image: jda_dev_coef_form])"""
    n = len(images)
    opts = list(opts) if opts is not None else [0] * n
    forms = [form] * n if isinstance(form, int) else list(form)
    geos = [im.geometry(pt, opt) for im, pt, opt in zip(images, pts, opts)]
    pitch = [(g["canvas_w"] * g["bpp"] + 15) & ~15 for g in geos]
    offs, total = [], 0
    for g, p in zip(geos, pitch):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    lib, devs, base = ctx.lib, [], ctx.malloc(max(total, 256))
    try:
        ctx.from_host(base, np.full(max(total, 256), fill, np.uint8))
        for im, f in zip(images, forms):
            err = C.c_int32(0)
            d = lib.jda_coef_upload_ex(ctx.handle, im.handle, f, C.byref(err))
            assert d and err.value == 0, err.value
            devs.append(d)
            assert lib.jda_dev_coef_bytes(d) == 512 + (im.sparse_bytes() if lib.jda_dev_coef_form(d) == J.COEF_SPARSE else im.dense_bytes())
        resident = [lib.jda_dev_coef_form(d) for d in devs]
        outs = (Output * n)(*[Output(base + offs[i], pitch[i], geos[i]["canvas_w"], geos[i]["canvas_h"]) for i in range(n)])
        r = None
        if rects is not None:
            flat = []
            for im, rc in zip(images, rects):
                flat += list(rc) if rc is not None else [0, 0, im.info.mcus_x, im.info.mcus_y]
            r = (C.c_int32 * (4 * n))(*flat)
        ctx.check(lib.jda_coef_decode_surfaces_rect(ctx.handle, n, (C.c_void_p * n)(*devs), outs, (C.c_int32 * n)(*pts), (C.c_int32 * n)(*opts), r), "jda_coef_decode_surfaces_rect")
        res = [(ctx.to_host(base + offs[i], pitch[i] * g["canvas_h"]).reshape(g["canvas_h"], pitch[i])[:, :g["canvas_w"] * g["bpp"]].copy(), g) for i, g in enumerate(geos)]
        return res, resident
    finally:
        for d in devs:
            lib.jda_dev_coef_free(ctx.handle, d)
        ctx.free(base)


@pytest.fixture(scope="module")
def twin(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_coefsim.so"))
    lib.coefsim_decode.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]

    def decode(jpeg, coefs, pt, opt, g):
        pitch = (g["canvas_w"] * g["bpp"] + 15) & ~15
        buf = np.zeros(pitch * g["canvas_h"] + 16, np.uint8)
        off = (-buf.ctypes.data) & 15
        out = buf[off:off + pitch * g["canvas_h"]].reshape(g["canvas_h"], pitch)
        coefs = np.ascontiguousarray(coefs)
        assert lib.coefsim_decode(jpeg, len(jpeg), coefs.ctypes.data, coefs.shape[0], pt, opt, 1, out.ctypes.data, pitch, g["canvas_w"], g["canvas_h"], None) == 0
        return out[:, :g["canvas_w"] * g["bpp"]].copy()
    return decode


# ---- (a) every layout, every mode -----------------------------------------------------------------------------------------------------------
def test_sparse_decode_over_baseline_fixtures(gpu_ctx, oracle):
    names = PC.BASELINE_FIXTURES + PC.STRESS_FIXTURES
    made = [PC.fixture_coefs(n, oracle) for n in names]
    images = [J.CoefImage(jpeg, coefs) for jpeg, coefs in made]
    before = _counts()
    try:
        for pt, opt in MODES:
            res = J.coef_decode(gpu_ctx, images, [pt] * len(images), [opt] * len(images), form=J.COEF_SPARSE)
            for n, (jpeg, _), (got, g) in zip(names, made, res):
                orc, want, err = oracle.decode_canvas(jpeg, pt, opt)
                assert orc == 1 and got.shape == want.shape, (n, pt, opt)
                assert np.array_equal(got, want), (n, pt, opt, int(np.count_nonzero(got != want)))
    finally:
        for im in images:
            im.close()
    launched = _counts(before)
    assert not [k for k in launched if "jda_coef_tiles" in k], launched          # no dense launch in those calls
    assert len(launched) == 5, launched                                           # one instantiation per MCU layout ..
    assert all(v == len(MODES) for v in launched.values()), launched              # .. launched once per call


# ---- (b) the edge sets, dense and sparse images interleaved in ONE call -------------------------------------------------------------------------
def test_edge_sets_in_one_mixed_call(gpu_ctx, twin):
    sets = SC.edge_sets()
    assert "wrap_264" in [s[0] for s in sets]
    images = [J.CoefImage(jpeg, coefs) for _, jpeg, coefs, _, _ in sets]
    try:
        for flip in (0, 1):                                                       # every set in both forms, neighbours in different ones
            want_forms = [J.COEF_SPARSE if (k + flip) & 1 else J.COEF_DENSE for k in range(len(sets))]
            before = _counts()
            res, forms = _decode(gpu_ctx, images, [s[3] for s in sets], [s[4] for s in sets], form=want_forms)
            launched = _counts(before)
            assert forms == want_forms
            pairs = {(f, im.info.ncomp, im.info.subsample) for f, im in zip(forms, images)}
            assert sum(launched.values()) == len(pairs) <= 10, (launched, pairs)  # one launch per (form, layout) present
            for (label, jpeg, coefs, pt, opt), (got, g) in zip(sets, res):
                want = twin(jpeg, coefs, pt, opt, g)
                assert np.array_equal(got, want), (label, flip, int(np.count_nonzero(got != want)))
    finally:
        for im in images:
            im.close()


def test_auto_and_upload_refusals_on_the_device(gpu_ctx, oracle):
    """JDA_COEF_AUTO makes the form of fewer bytes resident (dense on a tie) -- a photograph-like file sparse, quality-100 noise dense -- and both
    decode to the same pixels as coef_decode's defaults; a form outside 0..2 and a null image are JDA_INVALID_PARAMETER; the Python door
    coef_decode(rects=) leaves zeros outside a rectangle"""
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.random.default_rng(7).integers(0, 256, size=(64, 64, 3), dtype=np.uint8)).save(b, "JPEG", quality=100, subsampling="4:4:4", progressive=True)
    images = [J.CoefImage(PC.files("c420_200x136_q50_rst")[0]), J.CoefImage(b.getvalue())]
    try:
        rule = [J.COEF_SPARSE if im.sparse_bytes() < im.dense_bytes() else J.COEF_DENSE for im in images]
        assert rule == [J.COEF_SPARSE, J.COEF_DENSE]
        res, forms = _decode(gpu_ctx, images, [J.RGB8888] * 2, form=J.COEF_AUTO)
        assert forms == rule
        base, events = PC.reencoded("c420_200x136_q50_rst")
        assert events == 0 and np.array_equal(res[0][0], oracle.decode_canvas(base, J.RGB8888, 0)[1])
        err = C.c_int32(0)
        for form in (-1, 3, 100):
            assert not gpu_ctx.lib.jda_coef_upload_ex(gpu_ctx.handle, images[0].handle, form, C.byref(err)) and err.value == 1
        assert not gpu_ctx.lib.jda_coef_upload_ex(gpu_ctx.handle, None, J.COEF_AUTO, C.byref(err)) and err.value == 1
        (got, g), = J.coef_decode(gpu_ctx, images[:1], [J.RGB8888], form=J.COEF_AUTO, rects=[(1, 1, 3, 2)])
        want = np.zeros_like(res[0][0])
        want[16:32, 16 * 4:48 * 4] = res[0][0][16:32, 16 * 4:48 * 4]
        assert np.array_equal(got, want)
    finally:
        for im in images:
            im.close()


# ---- (c) rectangles ------------------------------------------------------------------------------------------------------------------------------
def test_rectangles_in_both_forms(gpu_ctx, oracle):
    names = ["gray_1600x16", "c444_333x217", "c420_333x217", "c422_1100x24_rstrow", "c440_300x64_rst5"]                      # one image per layout
    for form in (J.COEF_DENSE, J.COEF_SPARSE):
        images, pts, rects, expect = [], [], [], []
        for n in names:
            jpeg, coefs = PC.fixture_coefs(n, oracle)
            I = _info(jpeg)
            mw, mh = I.mcu_w, I.mcu_h
            per = SC.MCUS_PER_TILE["gray" if I.ncomp == 1 else {0x11: "4:4:4", 0x21: "4:2:2", 0x12: "4:4:0", 0x22: "4:2:0"}[I.subsample]]
            pt = J.GRAY8 if I.ncomp == 1 else J.RGB8888
            orc, want, err = oracle.decode_canvas(jpeg, pt, 0)
            assert orc == 1
            bpp = 1 if I.ncomp == 1 else 4
            y1 = min(2, I.mcus_y)
            cases = [None,                                                        # the whole image
                     (1, 0, 2, 1),                                                # one MCU
                     (1, 0, min(I.mcus_x, 1 + per + 1), y1),                      # a width that is no whole number of tiles
                     (2, 1, 2, 1),                                                # empty
                     (I.mcus_x, I.mcus_y, I.mcus_x + 3, I.mcus_y + 3),            # out of range
                     (-3, -3, 2, 10 ** 6)]                                        # clamped on every side
            for r in cases:
                images.append((jpeg, coefs)); pts.append(pt); rects.append(r)
                e = np.full_like(want, FILL)
                x0, ya, x1, yb = (0, 0, I.mcus_x, I.mcus_y) if r is None else (max(r[0], 0), max(r[1], 0), min(max(r[2], 0), I.mcus_x), min(max(r[3], 0), I.mcus_y))
                if x1 > x0 and yb > ya:
                    e[ya * mh:yb * mh, x0 * mw * bpp:x1 * mw * bpp] = want[ya * mh:yb * mh, x0 * mw * bpp:x1 * mw * bpp]
                expect.append(e)
        ims = [J.CoefImage(j, c) for j, c in images]
        try:
            before = _counts()
            res, forms = _decode(gpu_ctx, ims, pts, form=form, rects=rects, fill=FILL)
            assert forms == [form] * len(ims)
            launched = _counts(before)
            assert len(launched) == 5 and all(v == 1 for v in launched.values()), launched
            assert all(("jda_sparse_tiles" in k) == (form == J.COEF_SPARSE) for k in launched), launched
            for k, ((got, g), e) in enumerate(zip(res, expect)):
                assert np.array_equal(got, e), (form, names[k // 6], rects[k], int(np.count_nonzero(got != e)))
        finally:
            for im in ims:
                im.close()


# ---- (d) the pipeline ------------------------------------------------------------------------------------------------------------------------------
def _pipeline_batch(oracle, twin):
    """[(file, pixel type, options, expected status, expected canvas or None = the surface stays as it was)]"""
    from tests import prog_jpeg
    pt = J.RGB8888
    batch = []
    for n in ("c420_200x136_q50_rst", "c444_333x217_q85"):                        # baseline files (the bit means nothing to them)
        tw = PC.files(n)[1]
        batch.append((tw, pt, FULL if n.startswith("c444") else 0, 0, oracle.decode_canvas(tw, pt, 0)[1]))
    for n in ("c420_200x136_q50_rst", "c444_333x217_q85", "c422_200x136_q50_rst", "c420_640x368_q85"):      # Pillow's progressive files with the bit
        base, events = PC.reencoded(n)
        assert events == 0
        batch.append((PC.files(n)[0], pt, FULL, 0, oracle.decode_canvas(base, pt, 0)[1]))
    base, events = PC.reencoded("gray_200x136_q85")
    assert events == 0
    batch.append((PC.files("gray_200x136_q85")[0], J.GRAY8, FULL, 0, oracle.decode_canvas(base, J.GRAY8, 0)[1]))
    pj = PC.files("c420_333x217_q98")[0]                                          # a progressive file without the bit: the 1/8 thumbnail of its first scan
    orc, thumb, err = oracle.decode_canvas(pj, pt, 0)
    assert orc == 1
    batch.append((pj, pt, 0, 0, thumb))
    base, events = PS.reencoded("fx_c420__deep_sa")                               # a written file, deep successive approximation
    assert events == 0
    batch.append((PS.files("fx_c420__deep_sa")[0], pt, FULL, 0, oracle.decode_canvas(base, pt, 0)[1]))
    # cut inside its second scan: what its scans carry, the scan the data end in read on with zero bits (tests/test_progressive_full_cpu.py:
    # test_a_file_cut_inside_a_scan_is_read_with_zero_bits) -- the host decoder's coefficients through the twin
    name = "c420_200x136_q50_rst"
    full, dec = PC.files(name)[0], PC.decoded(name)
    cut = full[:(dec["scan_ends"][0] + dec["scan_ends"][1]) // 2]
    ci = J.CoefImage(cut)
    carried = ci.coefficients()
    assert carried.any() and not np.array_equal(carried, prog_jpeg.to_library_order(dec))
    g = ci.geometry(pt, 0)
    ci.close()
    # (the twin takes geometry and quantisers from a baseline header: the re-encoded baseline of the whole file has the cut file's SOF geometry and DQT)
    batch.append((cut, pt, FULL, 0, ("twin", PC.reencoded(name)[0], carried, g)))
    batch.append((PS.malformed()["refinement_size_2"], pt, FULL, 2, None))        # one of the eight malformed scans: JDA_DECODE_ERROR, the surface untouched
    batch.append((PC.files("c444_200x136_q98_rst")[0], pt, FULL | J.SCALE_HALF, 3, None))      # a scale bit beside the bit
    return batch


def _surfaces(ctx, batch):
    geos = [J.output_geometry(_info(f), pt, opt if st != 3 else FULL) for f, pt, opt, st, _ in batch]
    pitch = [(g["canvas_w"] * g["bpp"] + 15) & ~15 for g in geos]
    offs, total = [], 0
    for g, p in zip(geos, pitch):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    return geos, pitch, offs, total


def _check_batch(ctx, base, batch, geos, pitch, offs, status, twin_fn):
    assert status == [b[3] for b in batch], status
    for k, (f, pt, opt, st, want) in enumerate(batch):
        g = geos[k]
        got = ctx.to_host(base + offs[k], pitch[k] * g["canvas_h"]).reshape(g["canvas_h"], pitch[k])[:, :g["canvas_w"] * g["bpp"]]
        if want is None:
            assert bool((got == FILL).all()), k                                  # nothing was written
            continue
        if isinstance(want, tuple):
            want = twin_fn(want[1], want[2], pt, 0, want[3])
        assert got.shape == want.shape and np.array_equal(got, want), (k, int(np.count_nonzero(got != want)))


def _forms_and_layouts(batch):
    pairs = set()
    for f, pt, opt, st, want in batch:
        I = _info(f)
        if st == 0 and I.jpeg_type == 1 and (opt & FULL):
            im = J.CoefImage(f)
            pairs.add((im.sparse_bytes() < im.dense_bytes(), I.ncomp, I.subsample))
            im.close()
    return pairs


def test_pipeline_with_the_flag(gpu_ctx, oracle, twin):
    batch = _pipeline_batch(oracle, twin)
    n = len(batch)
    geos, pitch, offs, total = _surfaces(gpu_ctx, batch)
    files, pts, opts = [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]
    n_full = sum(1 for f, pt, opt, st, w in batch if st == 0 and (opt & FULL) and _info(f).jpeg_type == 1)
    pairs = _forms_and_layouts(batch)
    assert n_full == 7 and 2 <= len(pairs) < n_full
    bases = [gpu_ctx.malloc(total) for _ in range(2)]
    try:
        outs = [[(b + offs[k], pitch[k], geos[k]["canvas_w"], geos[k]["canvas_h"]) for k in range(n)] for b in bases]
        # without the flag: every bit-carrying progressive file is refused, as ever; everything else decodes
        gpu_ctx.from_host(bases[0], np.full(total, FILL, np.uint8))
        pipe = J.Pipeline(gpu_ctx, max_images=n, depth=2)
        st0 = pipe.wait(pipe.submit(files, outs[0], pts, opts))
        h0 = pipe.stats["host_path_images"]
        pipe.close()
        assert st0 == [3 if (opt & FULL) and _info(f).jpeg_type == 1 else 0 for f, pt, opt, st, w in batch], st0
        # with it: two batches in flight at once
        for b in bases:
            gpu_ctx.from_host(b, np.full(total, FILL, np.uint8))
        pipe = J.Pipeline(gpu_ctx, max_images=n, depth=2)
        before = _counts()
        t0 = pipe.submit(files, outs[0], pts, opts, J.SUBMIT_PROGRESSIVE_FULL)
        t1 = pipe.submit(files, outs[1], pts, opts, J.SUBMIT_PROGRESSIVE_FULL)
        s0, s1 = pipe.wait(t0), pipe.wait(t1)
        launched = _counts(before)
        stats = pipe.stats
        pipe.close()
        for b, s in zip(bases, (s0, s1)):
            _check_batch(gpu_ctx, b, batch, geos, pitch, offs, s, twin)
        assert stats["images"] == 2 * n and stats["failed_images"] == 2 * 2
        assert stats["host_path_images"] == 2 * (h0 + n_full), (stats, h0)       # their entropy decode ran on the host
        assert 0 < sum(launched.values()) <= 2 * len(pairs), (launched, pairs)    # per batch: one launch per (form, layout) present, not per image
        assert any("jda_sparse_tiles" in k for k in launched)
        assert stats["h2d_bytes"] > 0
        # a pipeline destroyed with such a batch in flight
        pipe = J.Pipeline(gpu_ctx, max_images=n, depth=2)
        pipe.submit(files, outs[0], pts, opts, J.SUBMIT_PROGRESSIVE_FULL)
        pipe.close()
    finally:
        for b in bases:
            gpu_ctx.free(b)


# ---- (e) the node ----------------------------------------------------------------------------------------------------------------------------------
def test_node_passes_the_flag(gpu_ctx, oracle, twin):
    lib = gpu_ctx.lib
    P = C.c_void_p
    lib.jda_node_create.restype = P
    lib.jda_node_create.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P]
    lib.jda_node_destroy.restype = None
    lib.jda_node_destroy.argtypes = [P]
    lib.jda_node_submit_ex.argtypes = [P, C.c_int32, P, P, P, P, P, C.c_int32, P]
    lib.jda_node_wait.argtypes = [P, C.c_int32, P]
    batch = _pipeline_batch(oracle, twin)
    n = len(batch)
    geos, pitch, offs, total = _surfaces(gpu_ctx, batch)
    err = C.c_int32(0)
    node = lib.jda_node_create((C.c_int32 * 1)(gpu_ctx.device), 1, n, 2, 0, C.byref(err))
    assert node and err.value == 0
    base = gpu_ctx.malloc(total)
    try:
        gpu_ctx.from_host(base, np.full(total, FILL, np.uint8))
        files = [b[0] for b in batch]
        arr = (C.c_char_p * n)(*files)
        lens = (C.c_int32 * n)(*[len(f) for f in files])
        outs = (Output * n)(*[Output(base + offs[k], pitch[k], geos[k]["canvas_w"], geos[k]["canvas_h"]) for k in range(n)])
        pts = (C.c_int32 * n)(*[b[1] for b in batch])
        opts = (C.c_int32 * n)(*[b[2] for b in batch])
        t, st = C.c_int32(-1), (C.c_int32 * n)()
        assert lib.jda_node_submit_ex(node, n, arr, lens, outs, pts, opts, J.SUBMIT_PROGRESSIVE_FULL, C.byref(t)) == 0
        assert lib.jda_node_wait(node, t.value, st) == 0
        _check_batch(gpu_ctx, base, batch, geos, pitch, offs, list(st), twin)
    finally:
        lib.jda_node_destroy(node)
        gpu_ctx.free(base)


# ---- (f) decode_to_tensors(progressive="full") ------------------------------------------------------------------------------------------------------
def test_decode_to_tensors_progressive_full(gpu_ctx):
    """in a process of its own (tests/sparse_torch_child.py), as tests/test_gpu_resize.py runs its child: torch has to be imported before
    libjpegdec_amd.so is loaded"""
    import importlib.util
    import subprocess
    import sys
    assert importlib.util.find_spec("torch") is not None, "torch is part of this project's stack: decode_to_tensors cannot be checked without it"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sparse_torch_child.py")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "sparse_torch_child ok" in r.stdout, r.stdout[-4000:]
