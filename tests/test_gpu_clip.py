"""The output clip (jda_output::width_px x rows) on the GPU: every store path's clipped body against the ONE reference of
tests/clip_cases.py -- the guard byte everywhere except the oracle's canvas inside the clip, every byte of every allocation compared.
A plan holds the same resident image once per clip, each entry with a surface of its own inside one allocation filled with 0x5a:
wide (the canvas's pitch and more, two guard rows) or tight (the clipped row's pitch, one guard row), back to back, so a pixel stored at
or behind the clip lands in a neighbour's pixels or in the guard.  The decode kernel's lists, jda_quarter_tiles, jda_dc_thumbnail (its
packed gray path on and off), the two flat thumbnail kernels, jda_coef_tiles and jda_sparse_tiles, a clip with an MCU rectangle and with
a bad MCU, the one calls with fewer rows, the pipeline and the node with clipped surfaces, and the refusals.  Each test asserts the
launches of the kernels it is about (jda_kernel_launch_counts)."""
import collections
import ctypes as C
import re

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.binding import Output
from jpegdec_amd.synth import synth_jpeg
from tests import clip_cases as K
from tests import orient_util as U
from tests import prog_cases as PC
from tests import rect_cases as R
from tests.test_gpu_rect import Resident

pytestmark = pytest.mark.gpu

FILL = 0x5a          # what every device surface holds before a decode
GUARD = 0x33         # what a host array holds before a one call
FULL = J.PROGRESSIVE_FULL
TAIL = 1 << 16       # guard bytes behind the last surface of an allocation
KERNELS = ("jda_decode_tiles_persistent", "jda_quarter_tiles", "jda_dc_thumbnail", "jda_dc_thumbnail_flat", "jda_dc_thumbnail_flat420", "jda_coef_tiles",
           "jda_sparse_tiles")

# key: a resident file of the plan; clip: (width_px, rows); rect: an MCU rectangle or None; nok: MCUs in front of a bad one or None
Entry = collections.namedtuple("Entry", "key pt opt clip rect nok", defaults=(None, None))


def launches(before=None):
    """launches so far of each kernel of KERNELS, every instantiation counted (minus `before`)"""
    out = dict.fromkeys(KERNELS, 0)
    for name, n in J.kernel_launch_counts().items():
        for k in KERNELS:
            if re.search(k + r"(?![a-z_0-9])", name):
                out[k] += n
    return out if before is None else {k: out[k] - before[k] for k in KERNELS}


def expected_kernel(short, opt):
    if opt & J.SCALE_EIGHTH:
        return {"gray": "jda_dc_thumbnail_flat", "c420": "jda_dc_thumbnail_flat420"}.get(short, "jda_dc_thumbnail")
    return "jda_quarter_tiles" if opt & J.SCALE_QUARTER else "jda_decode_tiles_persistent"


def place(entries, geos, shape):
    """surfaces back to back: [(offset, pitch, surface rows)], the bytes of all of them"""
    places, total = [], 0
    for e, g in zip(entries, geos):
        pitch, srows = K.surface_shape(shape, e.clip[0], e.clip[1], g)
        places.append((total, pitch, srows))
        total += pitch * srows
    return places, total


def expected_allocation(oracle, res, entries, geos, places, total, zeros=False):
    exp = np.full(total + TAIL, FILL, np.uint8)
    for e, g, (off, pitch, srows) in zip(entries, geos, places):
        want = R.oracle_canvas(oracle, e.key, res.items[e.key][0], e.pt, e.opt, must_succeed=e.nok is None)
        assert want.shape == (g["ch"], g["cw"] * g["bpp"]), (e, want.shape)
        exp[off:off + pitch * srows] = K.expected_clipped(want, e.clip[0], e.clip[1], g["bpp"], pitch, srows, e.rect, e.nok, FILL, (g["mx"], g["my"]), zeros).reshape(-1)
    return exp


def compare(got, exp, entries, places):
    for i, (e, (off, pitch, srows)) in enumerate(zip(entries, places)):
        a, b = got[off:off + pitch * srows], exp[off:off + pitch * srows]
        assert np.array_equal(a, b), (i, e, pitch, srows, int(np.count_nonzero(a != b)), np.flatnonzero(a != b)[:8].tolist())
    assert np.array_equal(got, exp)                                     # (.. and the guard behind the last surface)


def run_plan(ctx, oracle, res, entries, shape):
    """ONE Batch over the entries (jda_batch_create; jda_batch_create_rect as soon as one of them has a rectangle), decoded twice: the whole
    allocation must be what expected_clipped says both times -> the plan's statistics"""
    geos = [K.file_geometry(res.items[e.key][0], e.pt, e.opt) for e in entries]
    places, total = place(entries, geos, shape)
    exp = expected_allocation(oracle, res, entries, geos, places, total)
    rects = None
    if any(e.rect is not None for e in entries):
        rects = [e.rect if e.rect is not None else (0, 0, g["mx"], g["my"]) for e, g in zip(entries, geos)]
    base = ctx.malloc(total + TAIL)
    try:
        ctx.memset(base, FILL, total + TAIL)
        outs = [(base + off, pitch, e.clip[0], e.clip[1]) for e, (off, pitch, srows) in zip(entries, places)]
        b = J.Batch(ctx, [res.items[e.key][1] for e in entries], outs, [e.pt for e in entries], [e.opt for e in entries], mcu_rects=rects)
        try:
            stats = dict(b.stats)
            for _ in range(2):
                b.decode()
                ctx.sync()
                compare(ctx.to_host(base, total + TAIL), exp, entries, places)
            assert b.status() == [0 if e.nok is None else 2 for e in entries]
        finally:
            b.close()
    finally:
        ctx.free(base)
    assert stats["output_bytes"] == sum(min(e.clip[0], g["cw"]) * min(e.clip[1], g["ch"]) * g["bpp"] for e, g in zip(entries, geos)), stats
    return stats


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("short,dri", R.IMAGES)
def test_every_clip_of_an_image_in_one_plan(short, dri, shape, gpu_ctx, oracle):
    """per mode ONE plan: the same DeviceImage once per clip of the list"""
    res = Resident(gpu_ctx)
    try:
        key = (short, dri)
        res.add(key, R.rect_jpeg(short, dri))
        for pt, opt in R.modes_of(short):
            before = launches()
            clips = K.clips_of(short, pt, opt)
            run_plan(gpu_ctx, oracle, res, [Entry(key, pt, opt, c) for c in clips], shape)
            ran = launches(before)
            want = expected_kernel(short, opt)
            assert ran[want] >= 2 and sum(ran.values()) == ran[want], (short, pt, opt, ran)        # two decodes, and no other kernel's
    finally:
        res.close()


@pytest.mark.parametrize("short", R.SHORTS)
def test_clips_with_rectangles(short, gpu_ctx, oracle):
    """a clip and an MCU rectangle together, both restart flavours and every mode in ONE jda_batch_create_rect plan per shape (1/8 entries,
    whole and cropped, go to jda_dc_thumbnail there); and the whole images at 1/8 under the same clips in a plan without rectangles: one
    record per image of a gray or 4:2:0 file for the flat kernels"""
    res = Resident(gpu_ctx)
    mx, my = R.LAYOUTS[short][3:5]
    try:
        for dri in (False, True):
            res.add((short, dri), R.rect_jpeg(short, dri))
        entries, whole = [], []
        for k, (pt, opt) in enumerate(R.modes_of(short)):
            key = (short, bool(k & 1))
            g = K.geometry(short, pt, opt)
            for rect in K.clip_rects(short) + [(0, 0, mx, my)]:
                entries += [Entry(key, pt, opt, c, rect) for c in K.rect_clips(g)]
            if opt & J.SCALE_EIGHTH:
                whole += [Entry(key, pt, opt, c) for c in K.rect_clips(g)]
        assert len(entries) == 12 * len(R.modes_of(short)) and len(whole) == 3 * sum(1 for m in R.modes_of(short) if m[1] & J.SCALE_EIGHTH) >= 6
        for shape in K.SHAPES:
            before = launches()
            run_plan(gpu_ctx, oracle, res, entries, shape)
            ran = launches(before)
            assert ran["jda_dc_thumbnail"] >= 2 and ran["jda_quarter_tiles"] >= 2 and ran["jda_decode_tiles_persistent"] >= 2, ran
            assert ran["jda_dc_thumbnail_flat"] == ran["jda_dc_thumbnail_flat420"] == 0, ran
            before = launches()
            st = run_plan(gpu_ctx, oracle, res, whole, shape)
            ran = launches(before)
            want = expected_kernel(short, J.SCALE_EIGHTH)
            assert ran[want] == 2 * st["n_launches"] == sum(ran.values()), (ran, st)
            if "flat" in want:
                assert st["n_launches"] == 1 and st["n_workgroups"] == len(whole), st           # one record, and one workgroup column, per image
    finally:
        res.close()


def test_clips_on_a_stream_with_a_bad_mcu(gpu_ctx, oracle):
    """a resident image with a bad MCU under a clip: JDA_DECODE_ERROR in the status, the MCUs in front of the bad one inside the clip, nothing else"""
    jpeg, nok = U.bad_mcu_jpeg()
    res = Resident(gpu_ctx)
    try:
        res.add("bad_mcu", jpeg)
        entries = []
        for pt, opt in R.MODES:
            entries += [Entry("bad_mcu", pt, opt, c, None, nok) for c in K.rect_clips(K.file_geometry(jpeg, pt, opt))]
        for shape in K.SHAPES:
            run_plan(gpu_ctx, oracle, res, entries, shape)
    finally:
        res.close()


def test_wide_gray_thumbnail_quads_at_the_clip(gpu_ctx, oracle):
    """288 x 3 gray MCUs: at 1/8 a row is four whole tiles and a half, 256 + 32 pixels.  jda_dc_thumbnail stores four whole tiles side by
    side as 256 packed pixels when the run starts at a multiple of four MCUs AND mcu_x0 + 256 <= out_w: clips on either side of that (256
    for a run from MCU 0, 260 for one from MCU 4), as whole images (the flat kernel), with the rectangle one MCU short on the right and
    with one that starts at MCU 4.  The same widths at 1/4 (jda_quarter_tiles' shared gray rows) and as RGB565 at 1/8."""
    jpeg = synth_jpeg(2304, 24, "gray", seed=5)
    res = Resident(gpu_ctx)
    try:
        p, d = res.add("gray_288", jpeg)
        assert (p.info.mcus_x, p.info.mcus_y) == (288, 3)
        widths = (0, 1, 255, 256, 257, 259, 260, 287, 288, 300)
        for pt, opt, rows, kernel in ((J.GRAY8, J.SCALE_EIGHTH, (1, 2, 3, 4), "jda_dc_thumbnail"), (J.GRAY8, J.SCALE_QUARTER, (1, 2, 5, 6), "jda_quarter_tiles"),
                                      (J.RGB565_LE, J.SCALE_EIGHTH, (1, 2, 3, 4), "jda_dc_thumbnail")):
            clips = [(w, rows[i % 4]) for i, w in enumerate(widths)]
            for rect in (None, (0, 0, 287, 3), (4, 0, 288, 3)):
                for shape in K.SHAPES:
                    before = launches()
                    st = run_plan(gpu_ctx, oracle, res, [Entry("gray_288", pt, opt, c, rect) for c in clips], shape)
                    ran = launches(before)
                    want = "jda_dc_thumbnail_flat" if rect is None and opt & J.SCALE_EIGHTH else kernel
                    assert ran[want] == 2 * st["n_launches"] == sum(ran.values()), (pt, opt, rect, shape, ran, st)
    finally:
        res.close()


def test_kernels_that_ran(gpu_ctx, oracle):
    """one plan with one clipping entry per kernel: each of the five is launched once per decode"""
    res = Resident(gpu_ctx)
    try:
        for short in ("c444", "c420", "gray"):
            res.add((short, False), R.rect_jpeg(short))
        entries = []
        for short, pt, opt in (("c444", J.RGB8888, 0), ("c420", J.RGB565_LE, J.SCALE_QUARTER), ("gray", J.GRAY8, J.SCALE_EIGHTH), ("c420", J.RGB8888, J.SCALE_EIGHTH),
                               ("c444", J.RGB565_BE, J.SCALE_EIGHTH)):
            g = K.geometry(short, pt, opt)
            entries.append(Entry((short, False), pt, opt, (g["tw"] + 1, g["mho"] + 1)))
        before = launches()
        st = run_plan(gpu_ctx, oracle, res, entries, "tight")
        ran = launches(before)
        assert st["n_launches"] == 5 and ran == dict(dict.fromkeys(KERNELS, 0), jda_decode_tiles_persistent=2, jda_quarter_tiles=2, jda_dc_thumbnail=2,
                                                      jda_dc_thumbnail_flat=2, jda_dc_thumbnail_flat420=2), (st, ran)
    finally:
        res.close()


COEF_PTS = (J.RGB8888, J.RGB565_LE, J.RGB565_BE, J.GRAY8)


@pytest.mark.parametrize("short", R.SHORTS)
def test_coefficient_kernels_clipped(short, gpu_ctx, oracle):
    """the image's own coefficients (as the reference's reader stores them) resident in both forms; ONE jda_coef_decode_surfaces_rect call per
    shape over form x pixel type x the full-size clip list -- the last clips of every list with the rectangles of the CPU file --, and
    one jda_coef_decode_surfaces call over the dense image's clips"""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    jpeg = R.rect_jpeg(short)
    n, coefs, _, _, _ = oracle.entropy(jpeg)
    im = J.CoefImage(jpeg, np.ascontiguousarray(coefs))
    key = (short, False)
    res = collections.namedtuple("Files", "items")({key: (jpeg,)})
    devs = {}
    try:
        for form in (J.COEF_DENSE, J.COEF_SPARSE):
            err = C.c_int32(0)
            devs[form] = lib.jda_coef_upload_ex(ctx.handle, im.handle, form, C.byref(err))
            assert devs[form] and err.value == 0 and lib.jda_dev_coef_form(devs[form]) == form
        entries, forms = [], []
        for form in devs:
            for pt in COEF_PTS:
                if short == "gray" and pt == J.RGB8888:
                    continue
                g = K.geometry(short, pt, 0)
                rects = [None] * 64 + [r for r in K.clip_rects(short) for _ in range(3)]
                clips = K.clips_of(short, pt, 0) + K.rect_clips(g) * 3
                assert len(clips) <= len(rects)
                entries += [Entry(key, pt, 0, c, rects[k - len(clips)]) for k, c in enumerate(clips)]
                forms += [form] * len(clips)
        assert sum(e.rect is not None for e in entries) == 9 * 2 * (3 if short == "gray" else 4)
        for shape in K.SHAPES:
            for plain in (False, True):
                ee = [e for e, f in zip(entries, forms) if e.rect is None and f == J.COEF_DENSE] if plain else entries
                ff = [J.COEF_DENSE] * len(ee) if plain else forms
                geos = [K.file_geometry(jpeg, e.pt, 0) for e in ee]
                places, total = place(ee, geos, shape)
                exp = expected_allocation(oracle, res, ee, geos, places, total)
                m = len(ee)
                base = ctx.malloc(total + TAIL)
                try:
                    ctx.memset(base, FILL, total + TAIL)
                    outs = (Output * m)(*[Output(base + off, pitch, e.clip[0], e.clip[1]) for e, (off, pitch, srows) in zip(ee, places)])
                    handles = (C.c_void_p * m)(*[devs[f] for f in ff])
                    pts, opts = (C.c_int32 * m)(*[e.pt for e in ee]), (C.c_int32 * m)(*[0] * m)
                    before = launches()
                    if plain:
                        rc = lib.jda_coef_decode_surfaces(ctx.handle, m, handles, outs, pts, opts)
                    else:
                        flat = [v for e, g in zip(ee, geos) for v in (e.rect if e.rect is not None else (0, 0, g["mx"], g["my"]))]
                        rc = lib.jda_coef_decode_surfaces_rect(ctx.handle, m, handles, outs, pts, opts, (C.c_int32 * (4 * m))(*flat))
                    assert rc == 0, (shape, plain, rc)
                    ran = launches(before)
                    assert ran == dict(dict.fromkeys(KERNELS, 0), jda_coef_tiles=1, jda_sparse_tiles=0 if plain else 1), ran
                    compare(ctx.to_host(base, total + TAIL), exp, ee, places)
                finally:
                    ctx.free(base)
    finally:
        for d in devs.values():
            lib.jda_dev_coef_free(ctx.handle, d)
        im.close()


def one_call(ctx, fn, jpeg, pt, opt, host, rows, rect=None):
    """jda_decode_to_host / _ex / _rect into host[:rows] (the array's row length is the pitch) -> (status, MCUs decoded or None)"""
    nok = C.c_int32(-1)
    p = host.ctypes.data_as(C.c_void_p)
    if fn == "plain":
        return ctx.lib.jda_decode_to_host(ctx.handle, jpeg, len(jpeg), pt, opt, p, host.shape[1], rows), None
    if fn == "ex":
        return ctx.lib.jda_decode_to_host_ex(ctx.handle, jpeg, len(jpeg), pt, opt, p, host.shape[1], rows, C.byref(nok)), nok.value
    rc = ctx.lib.jda_decode_to_host_rect(ctx.handle, jpeg, len(jpeg), pt, opt, (C.c_int32 * 4)(*rect), p, host.shape[1], rows, C.byref(nok), None)
    return rc, nok.value


def host_expected(want, g, rows, shape, rect=None, nok=None):
    """a guard-filled host array after a one call with `rows` rows: the canvas's first min(rows, ch) rows (zeros from a bad MCU on; with a
    rectangle only its MCU rows, zeros left and right of it), the guard in the pitch padding and in every row behind"""
    exp = np.full(shape, GUARD, np.uint8)
    rr = min(rows, g["ch"])
    src, r0, r1 = want, 0, rr
    if rect is not None or nok is not None:
        src = R.expected_surface(want, rect if rect is not None else (0, 0, g["mx"], g["my"]), R.geometry_of(want, g["mx"], g["my"]), nok, 0)
    if rect is not None:
        x0, y0, x1, y1 = R.clamp_rect(rect, g["mx"], g["my"])
        r0, r1 = min(rr, y0 * g["mho"]), min(rr, max(y0, y1) * g["mho"])
    exp[r0:r1, :want.shape[1]] = src[r0:r1]
    return exp


@pytest.mark.parametrize("short", R.SHORTS)
def test_one_calls_with_fewer_rows(short, gpu_ctx, oracle):
    """a host array of fewer rows than the canvas, a pitch of its own and guard rows behind: what fits arrives, nothing else is written"""
    jpeg, key = R.rect_jpeg(short, True), (short, True)
    for pt, opt in R.modes_of(short):
        want = R.oracle_canvas(oracle, key, jpeg, pt, opt)
        g = K.geometry(short, pt, opt)
        for k, rows in enumerate((0, 1, g["mho"], g["vh"], g["ch"] - 1)):
            for fn in ("plain", "ex", "rect"):
                rect = K.clip_rects(short)[k % 3] if fn == "rect" else None
                host = np.full((rows + 2, want.shape[1] + 24), GUARD, np.uint8)
                rc, nok = one_call(gpu_ctx, fn, jpeg, pt, opt, host, rows, rect)
                assert rc == 0 and nok in (None, g["mx"] * g["my"]), (short, pt, opt, rows, fn, rc, nok)
                exp = host_expected(want, g, rows, host.shape, rect)
                assert np.array_equal(host, exp), (short, pt, opt, rows, fn, rect, int(np.count_nonzero(host != exp)))


def test_one_calls_with_fewer_rows_bad_mcu_and_progressive(gpu_ctx, oracle):
    """the same for a stream with a bad MCU (JDA_DECODE_ERROR, zeros from the bad MCU on, inside the rows that fit) and for a progressive
    file with JDA_PROGRESSIVE_FULL (the coefficient kernel under a row clip)"""
    jpeg, nbad = U.bad_mcu_jpeg()
    for pt, opt in R.MODES:
        want = R.oracle_canvas(oracle, "bad_mcu", jpeg, pt, opt, must_succeed=False)
        g = K.file_geometry(jpeg, pt, opt)
        for rows in (0, 1, g["mho"], g["vh"], g["ch"] - 1):
            host = np.full((rows + 2, want.shape[1] + 24), GUARD, np.uint8)
            rc, nok = one_call(gpu_ctx, "ex", jpeg, pt, opt, host, rows)
            assert (rc, nok) == (2, nbad), (pt, opt, rows, rc, nok)
            exp = host_expected(want, g, rows, host.shape, None, nbad)
            assert np.array_equal(host, exp), (pt, opt, rows, int(np.count_nonzero(host != exp)))
    name = "c420_200x136_q50_rst"
    pj, (base, events) = PC.files(name)[0], PC.reencoded(name)
    assert events == 0
    for pt in COEF_PTS:
        want = R.oracle_canvas(oracle, ("reencoded", name), base, pt, 0)
        g = K.file_geometry(pj, pt, FULL)
        assert (g["ch"], g["cw"] * g["bpp"]) == want.shape and g["s"] == 0
        for rows in (0, 1, g["mho"], g["vh"], g["ch"] - 1):
            host = np.full((rows + 2, want.shape[1] + 24), GUARD, np.uint8)
            before = launches()
            rc, _ = one_call(gpu_ctx, "plain", pj, pt, FULL, host, rows)
            assert rc == 0 and launches(before)["jda_coef_tiles"] == 1, (pt, rows, rc)
            exp = host_expected(want, g, rows, host.shape)
            assert np.array_equal(host, exp), (pt, rows, int(np.count_nonzero(host != exp)))


def test_strips_call_on_a_stream_with_a_bad_mcu(gpu_ctx, oracle):
    """jda_decode_to_host_strips (RGB8888, strips of 4 MCUs, one copy back) on a stream with a bad MCU: JDA_DECODE_ERROR and the MCUs in
    front of the bad one; every strip in front of it holds the oracle's pixels, every byte behind it is zero"""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    jpeg, nbad = U.bad_mcu_jpeg()
    info = J.parse(jpeg)
    mx, my = info["mcus_x"], info["mcus_y"]
    _, canvas, _ = oracle.decode_canvas(jpeg, J.RGB8888, 0)
    canvas = U.zero_undecoded(canvas, info, nbad)
    mh, mwb = canvas.shape[0] // my, canvas.shape[1] // mx                  # (rows x bytes of an MCU)
    per, n_sx = 4, (mx + 3) // 4
    strip_bytes = per * mwb * mh
    exp = np.zeros(my * n_sx * strip_bytes, np.uint8)                      # (behind a row's last, narrower strip: zeros too)
    for y in range(my):
        for s in range(n_sx):
            px = canvas[y * mh:(y + 1) * mh, s * per * mwb:min(mx, (s + 1) * per) * mwb]
            o = (y * n_sx + s) * strip_bytes
            exp[o:o + px.size] = px.reshape(-1)
    host = np.full(exp.size + 64, GUARD, np.uint8)
    nok = C.c_int32(-1)
    P = C.c_void_p
    lib.jda_decode_to_host_strips.argtypes = [P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P, C.c_size_t, P, C.c_int32, P, P]
    rc = lib.jda_decode_to_host_strips(ctx.handle, jpeg, len(jpeg), J.RGB8888, 0, per, host.ctypes.data, exp.size, C.byref(nok), 1, None, None)
    assert (rc, nok.value) == (2, nbad)
    first = (nbad // mx) * n_sx + (nbad % mx) // per                        # the strip that holds the bad MCU
    assert first > 0 and exp[:first * strip_bytes].any()
    assert np.array_equal(host[:first * strip_bytes], exp[:first * strip_bytes]), "a strip in front of the bad MCU"
    assert np.array_equal(host[first * strip_bytes:(first + 1) * strip_bytes], exp[first * strip_bytes:(first + 1) * strip_bytes]), "the bad MCU's strip"
    assert not host[(first + 1) * strip_bytes:exp.size].any(), "a byte behind the bad MCU's strip"
    assert np.all(host[exp.size:] == GUARD)


def pipeline_entries(oracle):
    """[(Entry, file handed in, file whose oracle canvas is expected)]: two images per layout in mixed modes under different clips, a stream
    with a bad MCU under two clips, a progressive file at full size under a clip, and a clip of (0, 0)"""
    files, entries = {}, []
    for i, short in enumerate(R.SHORTS):
        modes = R.modes_of(short)
        for j in range(2):
            key = (short, bool((i + j) & 1))
            files[key] = (R.rect_jpeg(*key),) * 2
            pt, opt = modes[(2 * i + 5 * j + 1) % len(modes)]
            g = K.geometry(short, pt, opt)
            inner = [c for c in K.clips_of(short, pt, opt) if 0 < c[0] < g["cw"] and 0 < c[1] < g["ch"]]
            clip = K.rect_clips(g)[i % 3] if j == 0 else inner[(3 * i + 2) % len(inner)]
            entries.append(Entry(key, pt, opt, clip))
    bad, nbad = U.bad_mcu_jpeg()
    files["bad_mcu"] = (bad, bad)
    for (pt, opt), which in (((J.RGB8888, 0), 2), ((J.RGB565_BE, J.SCALE_HALF), 0), ((J.GRAY8, J.SCALE_EIGHTH), 0)):
        entries.append(Entry("bad_mcu", pt, opt, K.rect_clips(K.file_geometry(bad, pt, opt))[which], None, nbad))
    name = "c420_200x136_q50_rst"
    files["prog"] = (PC.files(name)[0], PC.reencoded(name)[0])
    g = K.file_geometry(files["prog"][0], J.RGB565_LE, FULL)
    entries.append(Entry("prog", J.RGB565_LE, FULL, (g["tw"] + 1, g["vh"] - 1)))
    entries.append(Entry(("c444", False), J.RGB8888, 0, (0, 0)))
    assert len({(e.key, e.pt, e.opt, e.clip) for e in entries}) == len(entries) == 15
    return files, entries


def pipeline_expected(oracle, files, entries):
    geos = [K.file_geometry(files[e.key][0], e.pt, e.opt) for e in entries]
    places, total = place(entries, geos, "tight")
    exp = np.full(total + TAIL, FILL, np.uint8)
    for e, g, (off, pitch, srows) in zip(entries, geos, places):
        want = R.oracle_canvas(oracle, ("expected", e.key), files[e.key][1], e.pt, e.opt & ~FULL, must_succeed=e.nok is None)
        assert want.shape == (g["ch"], g["cw"] * g["bpp"]), (e, want.shape)
        # a failed image through the pipeline: zeros from the bad MCU on, inside the clip only
        exp[off:off + pitch * srows] = K.expected_clipped(want, e.clip[0], e.clip[1], g["bpp"], pitch, srows, None, e.nok, FILL, (g["mx"], g["my"]), zeros=True).reshape(-1)
    return places, total, exp


def test_pipeline_and_node_batches_with_clipped_surfaces(gpu_ctx, oracle):
    """ONE jda_pipeline batch (depth 2) whose surfaces are one allocation, tight and back to back; then the same list through jda_node_* on
    the one device"""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    files, entries = pipeline_entries(oracle)
    places, total, exp = pipeline_expected(oracle, files, entries)
    n = len(entries)
    jpegs, pts, opts = [files[e.key][0] for e in entries], [e.pt for e in entries], [e.opt for e in entries]
    status = [0 if e.nok is None else 2 for e in entries]
    base = ctx.malloc(total + TAIL)
    try:
        outs = [(base + off, pitch, e.clip[0], e.clip[1]) for e, (off, pitch, srows) in zip(entries, places)]
        ctx.memset(base, FILL, total + TAIL)
        pipe = J.Pipeline(ctx, max_images=n, depth=2)
        try:
            st = pipe.wait(pipe.submit(jpegs, outs, pts, opts, J.SUBMIT_PROGRESSIVE_FULL))
            stats = pipe.stats
        finally:
            pipe.close()
        assert st == status, st
        compare(ctx.to_host(base, total + TAIL), exp, entries, places)
        assert stats["images"] == n and stats["failed_images"] == 3, stats
        assert stats["device_images"] + stats["host_path_images"] == n and stats["host_path_images"] >= 4, stats      # the bad stream's redos and the progressive file
        # the node
        P = C.c_void_p
        lib.jda_node_create.restype = P
        lib.jda_node_create.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P]
        lib.jda_node_destroy.restype = None
        lib.jda_node_destroy.argtypes = [P]
        lib.jda_node_submit_ex.argtypes = [P, C.c_int32, P, P, P, P, P, C.c_int32, P]
        lib.jda_node_wait.argtypes = [P, C.c_int32, P]
        err = C.c_int32(0)
        node = lib.jda_node_create((C.c_int32 * 1)(ctx.device), 1, n, 2, 0, C.byref(err))
        assert node and err.value == 0
        try:
            ctx.memset(base, FILL, total + TAIL)
            ctx.sync()
            t, got_st = C.c_int32(-1), (C.c_int32 * n)()
            assert lib.jda_node_submit_ex(node, n, (C.c_char_p * n)(*jpegs), (C.c_int32 * n)(*[len(f) for f in jpegs]), (Output * n)(*[Output(*o) for o in outs]),
                                          (C.c_int32 * n)(*pts), (C.c_int32 * n)(*opts), J.SUBMIT_PROGRESSIVE_FULL, C.byref(t)) == 0
            assert lib.jda_node_wait(node, t.value, got_st) == 0
            assert list(got_st) == status, list(got_st)
            compare(ctx.to_host(base, total + TAIL), exp, entries, places)
        finally:
            lib.jda_node_destroy(node)
    finally:
        ctx.free(base)


def test_refusals_launch_nothing(gpu_ctx, oracle):
    """a negative clip, a pitch below the clipped row, a pitch that is no multiple of 16 and misaligned pixels: JDA_INVALID_PARAMETER from the
    plan, the coefficient call and (per image) the pipeline; no kernel is launched and the surface keeps the guard.  A pitch below the
    canvas's row but not below the clipped row's is accepted and decodes."""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    jpeg, key = R.rect_jpeg("c420"), ("c420", False)
    g = K.geometry("c420", J.RGB8888, 0)
    assert g["cw"] * 4 == 1600
    res = Resident(ctx)
    n, coefs, _, _, _ = oracle.entropy(jpeg)
    im = J.CoefImage(jpeg, np.ascontiguousarray(coefs))
    err = C.c_int32(0)
    dco = lib.jda_coef_upload(ctx.handle, im.handle, C.byref(err))
    nbytes = 1664 * (g["ch"] + 2)
    base = ctx.malloc(nbytes)
    try:
        assert dco and err.value == 0
        p, d = res.add(key, jpeg)
        ctx.memset(base, FILL, nbytes)
        ctx.sync()
        # (pixels, pitch, width_px, rows)
        bad = [(base, 1632, -1, g["ch"]), (base, 1632, g["cw"], -1), (base, 1584, g["cw"], g["ch"]), (base, 1584, g["cw"] + 9, 1), (base, 1608, g["cw"], g["ch"]),
               (base, 392, 100, 5), (base + 8, 1632, g["cw"], g["ch"]), (base + 4, 1632, 0, 0)]
        before = J.kernel_launch_counts()
        for o in bad:
            with pytest.raises(J.JdaError) as e:
                J.Batch(ctx, [d], [o], [J.RGB8888], [0])
            assert e.value.code == 1, (o, e.value.code)
            with pytest.raises(J.JdaError) as e:
                J.Batch(ctx, [d], [o], [J.RGB8888], [0], mcu_rects=[(0, 0, 2, 1)])
            assert e.value.code == 1, (o, e.value.code)
            rc = lib.jda_coef_decode_surfaces(ctx.handle, 1, (C.c_void_p * 1)(dco), (Output * 1)(Output(*o)), (C.c_int32 * 1)(J.RGB8888), (C.c_int32 * 1)(0))
            assert rc == 1, (o, rc)
        pipe = J.Pipeline(ctx, max_images=len(bad), depth=2)
        try:
            st = pipe.wait(pipe.submit([jpeg] * len(bad), bad, [J.RGB8888] * len(bad), [0] * len(bad)))
        finally:
            pipe.close()
        assert st == [1] * len(bad), st
        assert J.kernel_launch_counts() == before
        assert (ctx.to_host(base, nbytes) == FILL).all()
        # accepted: the pitch holds the clipped row
        want = R.oracle_canvas(oracle, key, jpeg, J.RGB8888, 0)
        for w, rows, pitch in ((100, 5, 400), (g["cw"] + 9, g["ch"] + 9, 1600), (0, 0, 16), (397, 47, 1600)):
            ctx.memset(base, FILL, nbytes)
            b = J.Batch(ctx, [d], [(base, pitch, w, rows)], [J.RGB8888], [0])
            try:
                b.decode()
                ctx.sync()
            finally:
                b.close()
            srows = nbytes // pitch
            got = ctx.to_host(base, srows * pitch).reshape(srows, pitch)
            exp = K.expected_clipped(want, w, rows, 4, pitch, srows, guard=FILL)
            assert np.array_equal(got, exp), (w, rows, pitch, int(np.count_nonzero(got != exp)))
            assert (ctx.to_host(base, nbytes)[srows * pitch:] == FILL).all()
    finally:
        ctx.free(base)
        if dco:
            lib.jda_dev_coef_free(ctx.handle, dco)
        im.close()
        res.close()
