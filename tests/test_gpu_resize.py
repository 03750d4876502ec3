"""jda_resize_surfaces on the GPU: (a) random surfaces over the whole grid of tests/resize_util.py, the job at the tap cap among them, ONE
launch per pixel size, against the numpy twin, every byte outside the results still the fill; (b) jda_decode_to_host_resized against the twin
over the oracle's canvas cut to the visible size -- whole images, crops, scales, JDA_LUMA_ONLY, the crop-aware tile counts, a bad MCU, the
refusals; (c) a streamed pipeline batch resized where it lies in HBM, then packed; (d) decode_to_tensors(size=...) in a child process.
Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.binding import ImageInfo, Output
from tests import orient_util as U
from tests import resize_util as R
from tests.cases import jpeg_for
from tests.test_pack_cpu import CHW, U8, numpy_pack

pytestmark = pytest.mark.gpu

FILL = 0x5A
INVALID, DECODE_ERROR, UNSUPPORTED = 1, 2, 3
FILES = ("gray_333x217", "c420_333x217", "c444_333x217", "c422_333x217", "c440_200x120")


def resize_counts():
    return {k: v for k, v in J.kernel_launch_counts().items() if "jda_resize_tiles" in k}


def resize_launches():
    return sum(resize_counts().values())


@pytest.mark.parametrize("bpp", [1, 4])
def test_whole_grid_in_one_launch(bpp, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.RandomState(700 + bpp)
    cases = R.image_cases()
    assert R.CAP_CASE in cases
    srcs, dsts, rects, blobs, soff, doff = [], [], [], [], 0, 0
    for w, h, box, ow, oh in cases:
        spitch, dpitch = R.pitch_of(w, bpp, 1), R.pitch_of(ow, bpp, 2)
        s = rng.randint(0, 256, (h, spitch)).astype(np.uint8)                   # (the padding behind a row's pixels is random too)
        blobs.append(s)
        srcs.append((soff, spitch, w, h))
        dsts.append((doff, dpitch, ow, oh))
        rects.append(box)
        soff += (s.size + 255) & ~255
        doff += ((oh + 3) * dpitch + 255) & ~255                               # three guard rows behind every result
    dsrc, ddst = ctx.malloc(soff), ctx.malloc(doff)
    for s, (o, _, _, _) in zip(blobs, srcs):
        ctx.from_host(dsrc + o, s.reshape(-1))
    ctx.memset(ddst, FILL, doff)
    before = resize_launches()
    J.resize_surfaces(ctx, [(dsrc + o, p, w, h) for o, p, w, h in srcs], bpp, [(ddst + o, p, w, h) for o, p, w, h in dsts], rects)
    assert resize_launches() == before + 1, "one launch for the whole grid"
    got = ctx.to_host(ddst, doff)
    ctx.free(dsrc)
    ctx.free(ddst)
    untouched = np.ones(doff, bool)
    for (w, h, box, ow, oh), s, (o, dpitch, _, _) in zip(cases, blobs, dsts):
        want = R.resize(s[:, :w * bpp].reshape(h, w, bpp), ow, oh, box)
        d = got[o:o + oh * dpitch].reshape(oh, dpitch)
        assert np.array_equal(d[:, :ow * bpp].reshape(oh, ow, bpp), want), (w, h, box, ow, oh)
        mask = untouched[o:o + oh * dpitch].reshape(oh, dpitch)
        mask[:, :ow * bpp] = False
    assert np.all(got[untouched] == FILL), "a byte outside out_w * bpp x out_h of a result was written"


def test_beyond_the_cap_is_refused_and_launches_nothing(gpu_ctx):
    ctx = gpu_ctx
    w, h, box, ow, oh = R.BEYOND_CAP_CASE
    a, b = ctx.malloc(1 << 16), ctx.malloc(1 << 12)
    ctx.memset(b, FILL, 1 << 12)
    before = resize_launches()
    for bpp in (1, 4):
        s, d = (Output * 1)(Output(a, R.pitch_of(w, bpp), w, h)), (Output * 1)(Output(b, R.pitch_of(ow, bpp), ow, oh))
        assert ctx.lib.jda_resize_surfaces(ctx.handle, 1, s, bpp, None, d) == UNSUPPORTED
        s = (Output * 1)(Output(a, R.pitch_of(h, bpp), h, w))                    # .. and on the other axis
        d = (Output * 1)(Output(b, R.pitch_of(oh, bpp), oh, ow))
        assert ctx.lib.jda_resize_surfaces(ctx.handle, 1, s, bpp, None, d) == UNSUPPORTED
    s, d = (Output * 1)(Output(a, 64, 10, 20)), (Output * 1)(Output(b, 32, 5, 7))
    for what, rc in (("n < 0", ctx.lib.jda_resize_surfaces(ctx.handle, -1, s, 4, None, d)), ("pixel size 2", ctx.lib.jda_resize_surfaces(ctx.handle, 1, s, 2, None, d)),
                     ("null arrays", ctx.lib.jda_resize_surfaces(ctx.handle, 1, None, 4, None, None)),
                     ("dst is src", ctx.lib.jda_resize_surfaces(ctx.handle, 1, s, 4, None, (Output * 1)(Output(a, 32, 5, 7)))),
                     ("rectangle leaves", ctx.lib.jda_resize_surfaces(ctx.handle, 1, s, 4, (C.c_int32 * 4)(6, 0, 5, 5), d))):
        assert rc == INVALID, what
    assert ctx.lib.jda_resize_surfaces(ctx.handle, 0, None, 4, None, None) == 0                      # nothing to do, nothing launched
    assert resize_launches() == before and np.all(ctx.to_host(b, 1 << 12) == FILL), "a refused call launches nothing and writes nothing"
    assert ctx.lib.jda_resize_surfaces(ctx.handle, 1, s, 4, None, d) == 0 and resize_launches() == before + 1
    ctx.free(a)
    ctx.free(b)


def visible_pixels(oracle, jpeg, pt, options, zero_from=None):
    """the oracle's canvas cut to the visible size -> [out_h, out_w, bpp]"""
    info = ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    g = J.output_geometry(info, pt, options)
    rc, canvas, err = oracle.decode_canvas(jpeg, pt, options)
    if zero_from is None:
        assert rc == 1, err
    else:
        canvas = U.zero_undecoded(canvas, J.parse(jpeg), zero_from)
    bpp = g["bpp"]
    return np.ascontiguousarray(canvas[:g["out_h"], :g["out_w"] * bpp]).reshape(g["out_h"], g["out_w"], bpp)


def check_one_call(ctx, oracle, jpeg, pt, options, size, rect=None, want_rc=0, zero_from=None):
    vis = visible_pixels(oracle, jpeg, pt, options, zero_from)
    bpp = vis.shape[2]
    ow, oh = size
    host = np.full((oh + 2, ow * bpp + 24), FILL, np.uint8)                       # a pitch of its own, guard rows
    rc, got, g, tiles = J.decode_resized_to_host(ctx, jpeg, size, pt, options, rect, out=host)
    assert rc == want_rc, (rc, options, size, rect)
    assert np.array_equal(host[:oh, :ow * bpp].reshape(oh, ow, bpp), R.resize(vis, ow, oh, rect)), (pt, options, size, rect)
    assert np.all(host[:oh, ow * bpp:] == FILL) and np.all(host[oh:] == FILL), "only out_w * bpp x out_h bytes come back"
    return tiles, g


@pytest.mark.parametrize("name", FILES)
def test_one_call_equals_the_twin_over_the_oracle(name, gpu_ctx, oracle):
    ctx = gpu_ctx
    jpeg = jpeg_for(name)
    pt = J.GRAY8 if name.startswith("gray") else J.RGB8888
    w, h = (200, 120) if name.endswith("200x120") else (333, 217)
    tiles, _ = check_one_call(ctx, oracle, jpeg, pt, 0, (224, 224))
    assert tiles[0] == tiles[1] > 0                                               # the whole image: every tile
    assert check_one_call(ctx, oracle, jpeg, pt, 0, (7, 5))[0][0] == tiles[1]
    assert check_one_call(ctx, oracle, jpeg, pt, 0, (2 * w, 2 * h))[0][0] == tiles[1]
    mid = ((w - 40) // 2, (h - 30) // 2, 40, 30)
    for size in ((40, 30), (16, 11), (100, 75)):                                  # as it is, down, up
        t, _ = check_one_call(ctx, oracle, jpeg, pt, 0, size, mid)
        assert 0 < t[0] < t[1] == tiles[1], (t, size)                             # only the MCUs the taps read are decoded
    for x, y in ((0, 0), (w - 40, 0), (0, h - 30), (w - 40, h - 30)):             # each corner
        t, _ = check_one_call(ctx, oracle, jpeg, pt, 0, (24, 32), (x, y, 40, 30))
        assert 0 < t[0] < t[1]
    check_one_call(ctx, oracle, jpeg, pt, 0, (13, 1), (5, 7, 1, 1))               # a one-pixel box
    # JDA_SCALE_HALF: the rectangle is in the scaled image's pixels
    hw, hh = (w + 1) // 2, (h + 1) // 2
    check_one_call(ctx, oracle, jpeg, pt, J.SCALE_HALF, (64, 48))
    t, _ = check_one_call(ctx, oracle, jpeg, pt, J.SCALE_HALF, (31, 17), (hw - 40, hh - 30, 40, 30))
    assert 0 < t[0] < t[1]
    check_one_call(ctx, oracle, jpeg, pt, J.SCALE_EIGHTH, (9, 9))
    if pt == J.RGB8888:                                                           # JDA_LUMA_ONLY: one channel from a colour file
        check_one_call(ctx, oracle, jpeg, J.GRAY8, J.LUMA_ONLY, (50, 40))
        check_one_call(ctx, oracle, jpeg, J.GRAY8, J.LUMA_ONLY | J.SCALE_HALF, (20, 30), (3, 2, 60, 50))
        check_one_call(ctx, oracle, jpeg, J.GRAY8, 0, (33, 21))


def test_one_call_bad_mcu_and_refusals(gpu_ctx, oracle):
    ctx = gpu_ctx
    # a stream with a bad MCU: zeros from the bad MCU on BEFORE the resize, the whole result delivered, JDA_DECODE_ERROR
    bad, nok = U.bad_mcu_jpeg()
    for size, rect in (((224, 224), None), ((40, 30), (250, 150, 83, 67))):
        t, g = check_one_call(ctx, oracle, bad, J.RGB8888, 0, size, rect, want_rc=DECODE_ERROR, zero_from=nok)
        assert g["mcus_decoded"] == nok
    base, prog = jpeg_for("c420_333x217"), jpeg_for("p420_200x120")
    # a progressive file is its 1/8 thumbnail, as in jda_decode_to_host_ex
    check_one_call(ctx, oracle, prog, J.RGB8888, 0, (32, 20))
    before = resize_launches()
    host = np.full((40, 256), FILL, np.uint8)

    def call(jpeg=base, pt=J.RGB8888, opt=0, rect=None, size=(32, 24), pitch=256, rows=40, pixels=True):
        r = None if rect is None else (C.c_int32 * 4)(*rect)
        return ctx.lib.jda_decode_to_host_resized(ctx.handle, jpeg, len(jpeg), pt, opt, r, size[0], size[1], host.ctypes.data_as(C.c_void_p) if pixels else None,
                                                  pitch, rows, None, None)
    for what, rc, want in (
            ("RGB565", call(pt=J.RGB565_LE), INVALID), ("RGB565 big endian", call(pt=J.RGB565_BE), INVALID), ("dithered", call(pt=J.ONE_BIT_DITHERED), INVALID),
            ("no host pixels", call(pixels=False), INVALID), ("output width 0", call(size=(0, 24)), INVALID), ("output height -1", call(size=(32, -1)), INVALID),
            ("pitch too small", call(pitch=127), INVALID), ("too few rows", call(rows=23), INVALID),
            ("empty rectangle", call(rect=(0, 0, 0, 5)), INVALID), ("negative origin", call(rect=(0, -1, 5, 5)), INVALID),
            ("rectangle leaves the visible image", call(rect=(300, 0, 34, 10)), INVALID), ("rectangle leaves the scaled image", call(opt=J.SCALE_HALF, rect=(0, 0, 168, 10)), INVALID),
            ("every scan of a progressive file", call(jpeg=prog, opt=J.PROGRESSIVE_FULL), UNSUPPORTED), ("two scale bits", call(opt=J.SCALE_HALF | J.SCALE_QUARTER), UNSUPPORTED),
            ("beyond the tap cap", call(size=(4, 24)), UNSUPPORTED), ("beyond the tap cap, rows", call(size=(32, 2)), UNSUPPORTED)):
        assert rc == want, (what, rc)
    assert np.all(host == FILL) and resize_launches() == before, "a refused call writes nothing and launches nothing"
    assert call(opt=J.PROGRESSIVE_FULL) == 0 and resize_launches() == before + 1          # (a baseline file: the bit means nothing)
    assert ctx.lib.jda_decode_to_host_resized(None, base, len(base), J.RGB8888, 0, None, 32, 24, host.ctypes.data_as(C.c_void_p), 256, 40, None, None) == 6


def test_pipeline_batch_resized_where_it_lies_then_packed(gpu_ctx, oracle):
    ctx = gpu_ctx
    ow, oh = 48, 32
    for pt, names in ((J.RGB8888, FILES[1:]), (J.GRAY8, FILES)):                   # (a gray file has no RGB8888 output)
        files = [jpeg_for(n) for n in names]
        n = len(files)
        infos = []
        for f in files:
            info = ImageInfo()
            assert ctx.lib.jda_parse(f, len(f), C.byref(info)) == 0
            infos.append(info)
        geos = [J.output_geometry(i, pt, 0) for i in infos]
        bpp, channels = geos[0]["bpp"], 3 if pt == J.RGB8888 else 1
        pit = [(g["canvas_w"] * bpp + 15) & ~15 for g in geos]
        offs, total = [], 0
        for g, p in zip(geos, pit):
            offs.append(total)
            total += (p * g["canvas_h"] + 255) & ~255
        rpitch = R.pitch_of(ow, bpp, 1)
        roffs = [total + k * (oh + 1) * rpitch for k in range(n)]                  # the resized surfaces behind the canvases, a guard row each
        total += n * (oh + 1) * rpitch
        dense = ow * oh * channels
        doffs = [total + 1 + k * (dense + 1) for k in range(n)]
        total += n * (dense + 1) + 16
        base = ctx.malloc(total)
        ctx.memset(base, FILL, total)
        pipe = J.Pipeline(ctx, max_images=n, depth=2)
        st = pipe.wait(pipe.submit(files, [(base + offs[i], pit[i], geos[i]["canvas_w"], geos[i]["canvas_h"]) for i in range(n)], [pt] * n, [0] * n))
        assert list(st) == [0] * n, st
        crops = [None if i % 2 == 0 else (7, 5, geos[i]["out_w"] - 20, geos[i]["out_h"] - 11) for i in range(n)]
        rects = [(0, 0, geos[i]["out_w"], geos[i]["out_h"]) if c is None else c for i, c in enumerate(crops)]
        before = resize_launches()
        J.resize_surfaces(ctx, [(base + offs[i], pit[i], geos[i]["out_w"], geos[i]["out_h"]) for i in range(n)], bpp, [(base + r, rpitch, ow, oh) for r in roffs], rects)
        assert resize_launches() == before + 1
        J.pack_surfaces(ctx, [(base + r, rpitch, ow, oh) for r in roffs], bpp, [base + d for d in doffs], CHW, U8)
        got = ctx.to_host(base + roffs[0], total - roffs[0])
        pipe.close()
        ctx.free(base)
        for i, f in enumerate(files):
            want = R.resize(visible_pixels(oracle, f, pt, 0), ow, oh, crops[i])
            surf = got[roffs[i] - roffs[0]:roffs[i] - roffs[0] + (oh + 1) * rpitch].reshape(oh + 1, rpitch)
            assert np.array_equal(surf[:oh, :ow * bpp].reshape(oh, ow, bpp), want), names[i]
            assert np.all(surf[:oh, ow * bpp:] == FILL) and np.all(surf[oh:] == FILL), names[i]
            at = doffs[i] - roffs[0]
            packed = numpy_pack(np.ascontiguousarray(want.reshape(oh, ow * bpp)), bpp, (0, 0, ow, oh), CHW, U8, None)
            assert got[at - 1] == FILL and np.array_equal(got[at:at + dense], packed), names[i]


def test_decode_to_tensors_with_size(gpu_ctx):
    """decode_to_tensors(size=...) against twin, numpy pack and table (tests/resize_torch_child.py), in a process of its own, as
    tests/test_gpu_pack.py::test_decode_to_tensors runs its child: torch has to be imported before libjpegdec_amd.so is loaded"""
    import importlib.util
    import os
    import subprocess
    import sys
    if importlib.util.find_spec("torch") is None:
        pytest.skip("no torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "resize_torch_child.py")], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "resize_torch_child ok" in r.stdout, r.stdout[-4000:]
