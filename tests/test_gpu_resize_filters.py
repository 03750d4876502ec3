"""jda_resize_surfaces_ex on the GPU -- Pillow's BOX, BILINEAR, HAMMING, BICUBIC and LANCZOS -- against the numpy twin
(tests/resize_filter_util.py; tests/test_resize_filters_cpu.py holds the twin to Pillow), bit for bit: (a) per filter and pixel size the whole
grid, the job at the filter's tap cap and the pictures that force both clips in ONE launch over guard-filled destinations, by the signed
instances for BICUBIC and LANCZOS and the old ones for the others; (b) one step beyond each cap, refused, nothing launched; (c)
jda_decode_to_host_resized_ex over the oracle's canvas: whole image, a middle crop, a corner crop, the crop-aware tile counts; (d) a
pipeline batch resized with LANCZOS where it lies, then packed; (e) decode_to_tensors(resample=) in a child process and
thumbnails(resample=) against the numpy encode twin; (f) the old call = the new one with filter 0."""
import ctypes as C

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.binding import ImageInfo, Output
from tests import encode_util as E
from tests import resize_filter_util as F
from tests import resize_util as R
from tests.cases import jpeg_for
from tests.test_gpu_resize import FILES, FILL, INVALID, UNSUPPORTED, visible_pixels
from tests.test_pack_cpu import CHW, U8, numpy_pack

pytestmark = pytest.mark.gpu
IDS = [F.NAMES[f] for f in F.FILTERS]


def launches(signed):
    """launches of the two signed instances, or of the two old ones"""
    return sum(v for k, v in J.kernel_launch_counts().items() if "jda_resize_tiles" in k and ("jda_resize_tiles_signed" in k) == signed)


def both():
    return launches(True), launches(False)


def expect_one(before, f):
    assert both() == (before[0] + (f in F.SIGNED), before[1] + (f not in F.SIGNED)), "exactly one launch, of the filter's instance"


@pytest.mark.parametrize("bpp", [1, 4])
@pytest.mark.parametrize("f", F.FILTERS, ids=IDS)
def test_whole_grid_in_one_launch(f, bpp, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.RandomState(900 + 10 * f + bpp)
    jobs = []                                                                    # (w, h, box, ow, oh, source rows [h, pitch])
    for w, h, box, ow, oh in F.image_cases(f) + [F.cap_case(f)]:
        jobs.append((w, h, box, ow, oh, rng.randint(0, 256, (h, R.pitch_of(w, bpp, 1))).astype(np.uint8)))      # (the padding behind a row's pixels is random too)
    for _, img, ow, oh in F.clip_pictures(bpp):
        h, w = img.shape[:2]
        s = np.full((h, R.pitch_of(w, bpp, 1)), 0x33, np.uint8)
        s[:, :w * bpp] = img.reshape(h, w * bpp)
        jobs.append((w, h, (0, 0, w, h), ow, oh, s))
    srcs, dsts, soff, doff = [], [], 0, 0
    for w, h, box, ow, oh, s in jobs:
        dpitch = R.pitch_of(ow, bpp, 2)
        srcs.append((soff, s.shape[1], w, h))
        dsts.append((doff, dpitch, ow, oh))
        soff += (s.size + 255) & ~255
        doff += ((oh + 3) * dpitch + 255) & ~255                               # three guard rows behind every result
    dsrc, ddst = ctx.malloc(soff), ctx.malloc(doff)
    for job, (o, _, _, _) in zip(jobs, srcs):
        ctx.from_host(dsrc + o, job[5].reshape(-1))
    ctx.memset(ddst, FILL, doff)
    before = both()
    J.resize_surfaces(ctx, [(dsrc + o, p, w, h) for o, p, w, h in srcs], bpp, [(ddst + o, p, w, h) for o, p, w, h in dsts], [j[2] for j in jobs], filter=f)
    expect_one(before, f)
    got = ctx.to_host(ddst, doff)
    ctx.free(dsrc)
    ctx.free(ddst)
    untouched = np.ones(doff, bool)
    for (w, h, box, ow, oh, s), (o, dpitch, _, _) in zip(jobs, dsts):
        want = F.resize(s[:, :w * bpp].reshape(h, w, bpp), ow, oh, box, f)
        d = got[o:o + oh * dpitch].reshape(oh, dpitch)
        assert np.array_equal(d[:, :ow * bpp].reshape(oh, ow, bpp), want), (F.NAMES[f], w, h, box, ow, oh)
        untouched[o:o + oh * dpitch].reshape(oh, dpitch)[:, :ow * bpp] = False
    assert np.all(got[untouched] == FILL), "a byte outside out_w * bpp x out_h of a result was written"


def test_beyond_each_cap_is_refused_and_launches_nothing(gpu_ctx):
    ctx = gpu_ctx
    a, b = ctx.malloc(1 << 17), ctx.malloc(1 << 12)
    ctx.memset(b, FILL, 1 << 12)
    before = both()
    ex = ctx.lib.jda_resize_surfaces_ex
    for f in F.FILTERS:
        w, h, box, ow, oh = F.beyond_cap_case(f)
        for bpp in (1, 4):
            s, d = (Output * 1)(Output(a, R.pitch_of(w, bpp), w, h)), (Output * 1)(Output(b, R.pitch_of(ow, bpp), ow, oh))
            assert ex(ctx.handle, 1, s, bpp, None, d, f) == UNSUPPORTED, F.NAMES[f]
            s = (Output * 1)(Output(a, R.pitch_of(h, bpp), h, w))                # .. and on the other axis
            d = (Output * 1)(Output(b, R.pitch_of(oh, bpp), oh, ow))
            assert ex(ctx.handle, 1, s, bpp, None, d, f) == UNSUPPORTED, F.NAMES[f]
    s, d = (Output * 1)(Output(a, 64, 10, 20)), (Output * 1)(Output(b, 32, 5, 7))
    for what, rc in (("filter 5", ex(ctx.handle, 1, s, 4, None, d, 5)), ("filter -1", ex(ctx.handle, 1, s, 4, None, d, -1)), ("filter 5, nothing to do", ex(ctx.handle, 0, None, 4, None, None, 5)),
                     ("n < 0", ex(ctx.handle, -1, s, 4, None, d, 3)), ("pixel size 2", ex(ctx.handle, 1, s, 2, None, d, 3)), ("null arrays", ex(ctx.handle, 1, None, 4, None, None, 4)),
                     ("dst is src", ex(ctx.handle, 1, s, 4, None, (Output * 1)(Output(a, 32, 5, 7)), 4)),
                     ("rectangle leaves", ex(ctx.handle, 1, s, 4, (C.c_int32 * 4)(6, 0, 5, 5), d, 3))):
        assert rc == INVALID, what
    assert ex(ctx.handle, 0, None, 4, None, None, 4) == 0                          # nothing to do, nothing launched
    assert both() == before and np.all(ctx.to_host(b, 1 << 12) == FILL), "a refused call launches nothing and writes nothing"
    assert ex(ctx.handle, 1, s, 4, None, d, F.LANCZOS) == 0
    expect_one(before, F.LANCZOS)
    ctx.free(a)
    ctx.free(b)


def test_old_call_equals_filter_zero(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.RandomState(77)
    w, h, ow, oh, bpp = 217, 65, 64, 33, 4
    s = rng.randint(0, 256, (h, R.pitch_of(w, bpp))).astype(np.uint8)
    dpitch = R.pitch_of(ow, bpp)
    a, b = ctx.malloc(s.size), ctx.malloc(2 * oh * dpitch)
    ctx.from_host(a, s.reshape(-1))
    ctx.memset(b, FILL, 2 * oh * dpitch)
    S = (Output * 1)(Output(a, s.shape[1], w, h))
    before = both()
    assert ctx.lib.jda_resize_surfaces(ctx.handle, 1, S, bpp, None, (Output * 1)(Output(b, dpitch, ow, oh))) == 0
    assert ctx.lib.jda_resize_surfaces_ex(ctx.handle, 1, S, bpp, None, (Output * 1)(Output(b + oh * dpitch, dpitch, ow, oh)), 0) == 0
    assert both() == (before[0], before[1] + 2), "both launch the old instance"
    got = ctx.to_host(b, 2 * oh * dpitch).reshape(2, oh, dpitch)
    ctx.free(a)
    ctx.free(b)
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(got[0][:, :ow * bpp].reshape(oh, ow, bpp), R.resize(s[:, :w * bpp].reshape(h, w, bpp), ow, oh))


def check_one_call(ctx, vis, jpeg, pt, f, size, rect=None):
    bpp = vis.shape[2]
    ow, oh = size
    host = np.full((oh + 2, ow * bpp + 24), FILL, np.uint8)                       # a pitch of its own, guard rows
    before = both()
    rc, got, g, tiles = J.decode_resized_to_host(ctx, jpeg, size, pt, 0, rect, out=host, filter=f)
    assert rc == 0, (rc, F.NAMES[f], size, rect)
    expect_one(before, f)
    assert np.array_equal(host[:oh, :ow * bpp].reshape(oh, ow, bpp), F.resize(vis, ow, oh, rect, f)), (F.NAMES[f], size, rect)
    assert np.all(host[:oh, ow * bpp:] == FILL) and np.all(host[oh:] == FILL), "only out_w * bpp x out_h bytes come back"
    return tiles


@pytest.mark.parametrize("name", FILES)
def test_one_call_equals_the_twin_over_the_oracle(name, gpu_ctx, oracle):
    ctx = gpu_ctx
    jpeg = jpeg_for(name)
    pt = J.GRAY8 if name.startswith("gray") else J.RGB8888
    w, h = (200, 120) if name.endswith("200x120") else (333, 217)
    vis = visible_pixels(oracle, jpeg, pt, 0)
    for f in F.SIGNED:
        tiles = check_one_call(ctx, vis, jpeg, pt, f, (96, 64))
        assert tiles[0] == tiles[1] > 0                                           # the whole image: every tile
        mid = ((w - 40) // 2, (h - 30) // 2, 40, 30)
        for size in ((40, 30), (16, 11)):                                         # as it is, down: the taps leave the box, but not the MCUs around it
            t = check_one_call(ctx, vis, jpeg, pt, f, size, mid)
            assert 0 < t[0] < t[1] == tiles[1], (t, size)
        t = check_one_call(ctx, vis, jpeg, pt, f, (24, 32), (w - 40, h - 30, 40, 30))      # the corner: the taps are clipped at the image
        assert 0 < t[0] < t[1]
    before = both()
    host = np.full((40, 256), FILL, np.uint8)
    for what, flt, size, want in (("filter 5", 5, (32, 24), INVALID), ("filter -1", -1, (32, 24), INVALID), ("beyond BICUBIC's cap", F.BICUBIC, (32, h // 41), UNSUPPORTED),
                                  ("beyond LANCZOS' cap", F.LANCZOS, (w // 27, 24), UNSUPPORTED)):
        rc = ctx.lib.jda_decode_to_host_resized_ex(ctx.handle, jpeg, len(jpeg), pt, 0, None, size[0], size[1], flt, host.ctypes.data_as(C.c_void_p), 256, 40, None, None)
        assert rc == want, (what, rc)
    assert np.all(host == FILL) and both() == before, "a refused call writes nothing and launches nothing"


def test_pipeline_batch_resized_with_lanczos_where_it_lies_then_packed(gpu_ctx, oracle):
    ctx = gpu_ctx
    ow, oh = 48, 32
    names = FILES[1:] + ("c444_384x192_q100_rst7", "c420_256x256_q98")
    files = [jpeg_for(n) for n in names]
    n = len(files)
    assert n == 6
    infos = []
    for f in files:
        info = ImageInfo()
        assert ctx.lib.jda_parse(f, len(f), C.byref(info)) == 0
        infos.append(info)
    geos = [J.output_geometry(i, J.RGB8888, 0) for i in infos]
    bpp = 4
    pit = [(g["canvas_w"] * bpp + 15) & ~15 for g in geos]
    offs, total = [], 0
    for g, p in zip(geos, pit):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    rpitch = R.pitch_of(ow, bpp, 1)
    roffs = [total + k * (oh + 1) * rpitch for k in range(n)]                      # the resized surfaces behind the canvases, a guard row each
    total += n * (oh + 1) * rpitch
    dense = ow * oh * 3
    doffs = [total + 1 + k * (dense + 1) for k in range(n)]
    total += n * (dense + 1) + 16
    base = ctx.malloc(total)
    ctx.memset(base, FILL, total)
    pipe = J.Pipeline(ctx, max_images=n, depth=2)
    st = pipe.wait(pipe.submit(files, [(base + offs[i], pit[i], geos[i]["canvas_w"], geos[i]["canvas_h"]) for i in range(n)], [J.RGB8888] * n, [0] * n))
    assert list(st) == [0] * n, st
    crops = [None if i % 2 == 0 else (7, 5, geos[i]["out_w"] - 20, geos[i]["out_h"] - 11) for i in range(n)]
    rects = [(0, 0, geos[i]["out_w"], geos[i]["out_h"]) if c is None else c for i, c in enumerate(crops)]
    before = both()
    J.resize_surfaces(ctx, [(base + offs[i], pit[i], geos[i]["out_w"], geos[i]["out_h"]) for i in range(n)], bpp, [(base + r, rpitch, ow, oh) for r in roffs], rects,
                      filter=J.RESIZE_LANCZOS)
    expect_one(before, F.LANCZOS)
    J.pack_surfaces(ctx, [(base + r, rpitch, ow, oh) for r in roffs], bpp, [base + d for d in doffs], CHW, U8)
    got = ctx.to_host(base + roffs[0], total - roffs[0])
    pipe.close()
    ctx.free(base)
    for i, f in enumerate(files):
        want = F.resize(visible_pixels(oracle, f, J.RGB8888, 0), ow, oh, crops[i], F.LANCZOS)
        surf = got[roffs[i] - roffs[0]:roffs[i] - roffs[0] + (oh + 1) * rpitch].reshape(oh + 1, rpitch)
        assert np.array_equal(surf[:oh, :ow * bpp].reshape(oh, ow, bpp), want), names[i]
        assert np.all(surf[:oh, ow * bpp:] == FILL) and np.all(surf[oh:] == FILL), names[i]
        at = doffs[i] - roffs[0]
        packed = numpy_pack(np.ascontiguousarray(want.reshape(oh, ow * bpp)), bpp, (0, 0, ow, oh), CHW, U8, None)
        assert got[at - 1] == FILL and np.array_equal(got[at:at + dense], packed), names[i]


def test_thumbnails_with_resample(gpu_ctx, oracle):
    names = ("c420_333x217", "c444_333x217", "c440_200x120")
    files = [jpeg_for(nm) for nm in names]
    H, W = 48, 64
    crops = [(10, 20, 300, 150), (1, 2, 33, 47), (0, 0, 200, 120)]
    for resample, f in (("lanczos", F.LANCZOS), ("bicubic", F.BICUBIC)):
        before = both()
        out = J.thumbnails(gpu_ctx, files, (H, W), quality=80, sampling="4:2:0", prescale=False, resample=resample)
        expect_one(before, f)
        for jf, t in zip(files, out):
            assert t == E.file_bytes(F.resize(visible_pixels(oracle, jf, J.RGB8888, 0), W, H, None, f), "4:2:0", 80, 0), resample
        out = J.thumbnails(gpu_ctx, files, (H, W), quality=75, sampling="4:4:4", crops=crops, resample=resample)
        for jf, t, c in zip(files, out, crops):
            assert t == E.file_bytes(F.resize(visible_pixels(oracle, jf, J.RGB8888, 0), W, H, c, f), "4:4:4", 75, 0), resample
    assert J.thumbnails(gpu_ctx, files[:1], (H, W), prescale=False) == J.thumbnails(gpu_ctx, files[:1], (H, W), prescale=False, resample="bilinear")
    before = both()
    with pytest.raises(ValueError):
        J.thumbnails(gpu_ctx, files, (H, W), resample="nearest")
    assert both() == before


def test_decode_to_tensors_with_resample(gpu_ctx):
    """decode_to_tensors(size=(24, 24), resample=...) against the twin (tests/resize_filters_torch_child.py), in a process of its own, as
    tests/test_gpu_resize.py::test_decode_to_tensors_with_size runs its child: torch has to be imported before libjpegdec_amd.so is loaded"""
    import importlib.util
    import os
    import subprocess
    import sys
    if importlib.util.find_spec("torch") is None:
        pytest.skip("no torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "resize_filters_torch_child.py")], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "resize_filters_torch_child ok" in r.stdout, r.stdout[-4000:]
