"""Pillow's Image.thumbnail() on the GPU, bit for bit: (a) jda_reduce_surfaces over the CPU grid (tests/test_thumbnail_cpu.py) as ONE launch
per pixel size into one guard-filled allocation, twice, against the numpy twin (tests/thumbnail_util.py, held to Image.reduce on the CPU);
(b) jda_resize_surfaces_box over the float-box grid, one launch per pixel size and filter, against the twin (held to Image.resize there);
(c) jda_decode_to_host_thumbnail over Pillow-written files against Pillow's own thumbnail(), RGB8888 and gray, with the launches it
reports; (d) thumbnails(pillow=True) over a list of mixed sizes against the bytes Pillow saves -- baseline, optimize=True, progressive=True --,
a file already within the size among them, with the launch counts; (e) refusals, which launch nothing and write nothing."""
import io

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.binding import Output
from tests import resize_filter_util as F
from tests import thumbnail_util as T
from tests.test_gpu_resize import FILL, INVALID, UNSUPPORTED
from tests.test_thumbnail_cpu import CHAIN_FILES, CHAIN_REQUESTS, box_jobs, chain_decode, chain_file, reduce_cases, row_end_classes

pytestmark = pytest.mark.gpu
IDS = [F.NAMES[f] for f in F.FILTERS]


def launches(name):
    return sum(v for k, v in J.kernel_launch_counts().items() if name in k)


def pitch_of(w, bpp, extra=0):
    return ((w * bpp + 15) & ~15) + 16 * extra


@pytest.mark.parametrize("bpp", [1, 4])
def test_reduce_grid_in_one_launch(bpp, gpu_ctx):
    ctx = gpu_ctx
    assert row_end_classes() == (set(range(16)), set(range(4)))                  # every end of a row's last vector is in the launch
    rng = np.random.RandomState(500 + bpp)
    jobs = []                                                                    # (w, h, box, fx, fy, source rows [h, pitch], ow, oh)
    for k, (w, h, box, fx, fy) in enumerate(reduce_cases()):
        s = rng.randint(0, 256, (h, pitch_of(w, bpp, 1))).astype(np.uint8)       # (the padding behind a row's pixels is random too)
        if k % 5 == 0:
            s[:, :w * bpp] = 255 if k % 10 == 0 else ((np.add.outer(np.arange(h), np.arange(w * bpp) // bpp) & 1) * 255)
        bw, bh = (box[2] - box[0], box[3] - box[1]) if box else (w, h)
        jobs.append((w, h, box or (0, 0, w, h), fx, fy, s) + T.reduced_size(bw, bh, fx, fy))
    srcs, dsts, soff, doff = [], [], 0, 0
    for w, h, box, fx, fy, s, ow, oh in jobs:
        dpitch = pitch_of(ow, bpp, 2)
        srcs.append((soff, s.shape[1], w, h))
        dsts.append((doff, dpitch, ow, oh))
        soff += (s.size + 255) & ~255
        doff += ((oh + 3) * dpitch + 255) & ~255                               # three guard rows behind every result
    dsrc, ddst = ctx.malloc(soff), ctx.malloc(doff)
    for job, (o, _, _, _) in zip(jobs, srcs):
        ctx.from_host(dsrc + o, job[5].reshape(-1))
    for run in range(2):
        ctx.memset(ddst, FILL, doff)
        before = launches("jda_reduce_tiles")
        J.reduce_surfaces(ctx, [(dsrc + o, p, w, h) for o, p, w, h in srcs], bpp, [(j[3], j[4]) for j in jobs], [(ddst + o, p, w, h) for o, p, w, h in dsts], [j[2] for j in jobs])
        assert launches("jda_reduce_tiles") == before + 1, "one launch for the whole grid"
        got = ctx.to_host(ddst, doff)
        untouched = np.ones(doff, bool)
        for (w, h, box, fx, fy, s, ow, oh), (o, dpitch, _, _) in zip(jobs, dsts):
            want = T.reduce(s[:, :w * bpp].reshape(h, w, bpp), fx, fy, box)
            d = got[o:o + oh * dpitch].reshape(oh, dpitch)
            assert np.array_equal(d[:, :ow * bpp].reshape(oh, ow, bpp), want), (run, w, h, box, fx, fy)
            untouched[o:o + oh * dpitch].reshape(oh, dpitch)[:, :ow * bpp] = False
        assert np.all(got[untouched] == FILL), "a byte outside out_w * bpp x out_h of a result was written"
    ctx.free(dsrc)
    ctx.free(ddst)


@pytest.mark.parametrize("bpp", [1, 4])
@pytest.mark.parametrize("f", F.FILTERS, ids=IDS)
def test_float_box_grid_in_one_launch(f, bpp, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.RandomState(700 + 10 * f + bpp)
    jobs = []
    for w, h, b, ow, oh in box_jobs():
        fb = [T.f32(v) for v in b]
        if max(F.ksize_of(f, fb[0], fb[0] + T.f32(fb[2] - fb[0]), ow), F.ksize_of(f, fb[1], fb[1] + T.f32(fb[3] - fb[1]), oh)) > F.MAX_KSIZE:
            continue
        jobs.append((w, h, b, ow, oh, rng.randint(0, 256, (h, pitch_of(w, bpp, 1))).astype(np.uint8)))
    assert len(jobs) > 60
    srcs, dsts, soff, doff = [], [], 0, 0
    for w, h, b, ow, oh, s in jobs:
        dpitch = pitch_of(ow, bpp, 2)
        srcs.append((soff, s.shape[1], w, h))
        dsts.append((doff, dpitch, ow, oh))
        soff += (s.size + 255) & ~255
        doff += ((oh + 3) * dpitch + 255) & ~255
    dsrc, ddst = ctx.malloc(soff), ctx.malloc(doff)
    for job, (o, _, _, _) in zip(jobs, srcs):
        ctx.from_host(dsrc + o, job[5].reshape(-1))
    ctx.memset(ddst, FILL, doff)
    signed = f in F.SIGNED
    before = launches("jda_resize_tiles_signed"), launches("jda_resize_tiles")
    J.resize_surfaces_box(ctx, [(dsrc + o, p, w, h) for o, p, w, h in srcs], bpp, [(ddst + o, p, w, h) for o, p, w, h in dsts], [j[2] for j in jobs], f)
    assert (launches("jda_resize_tiles_signed"), launches("jda_resize_tiles")) == (before[0] + signed, before[1] + 1), "one launch, of the filter's instance"
    got = ctx.to_host(ddst, doff)
    ctx.free(dsrc)
    ctx.free(ddst)
    untouched = np.ones(doff, bool)
    for (w, h, b, ow, oh, s), (o, dpitch, _, _) in zip(jobs, dsts):
        want = T.resize_box(s[:, :w * bpp].reshape(h, w, bpp), ow, oh, b, f)
        d = got[o:o + oh * dpitch].reshape(oh, dpitch)
        assert np.array_equal(d[:, :ow * bpp].reshape(oh, ow, bpp), want), (F.NAMES[f], w, h, b, ow, oh)
        untouched[o:o + oh * dpitch].reshape(oh, dpitch)[:, :ow * bpp] = False
    assert np.all(got[untouched] == FILL), "a byte outside out_w * bpp x out_h of a result was written"


def pillow_filters():
    from PIL import Image
    return {F.BILINEAR: Image.BILINEAR, F.BOX: Image.BOX, F.HAMMING: Image.HAMMING, F.BICUBIC: Image.BICUBIC, F.LANCZOS: Image.LANCZOS}


def pillow_thumbnail(f, req, flt, gap):
    from PIL import Image
    im = Image.open(io.BytesIO(f))
    im.thumbnail(req, pillow_filters()[flt], reducing_gap=gap)
    return im


@pytest.mark.parametrize("sampling,w,h,kind", CHAIN_FILES, ids=["%s_%dx%d_%s" % c for c in CHAIN_FILES])
def test_decode_to_host_thumbnail_is_pillows(sampling, w, h, kind, gpu_ctx):
    f = chain_file(sampling, w, h, kind)
    gray = sampling == "gray"
    seen, refused = set(), 0
    for i, (req, gap) in enumerate(CHAIN_REQUESTS):
        for flt in F.FILTERS if i % 4 == 0 else (F.FILTERS[i % 5],):
            p = T.plan(w, h, req, flt, gap)
            before = launches("jda_reduce_tiles"), launches("jda_resize_tiles")
            rc, got, n = J.decode_to_host_thumbnail(gpu_ctx, f, req, flt, gap, J.GRAY8 if gray else J.RGB8888)
            after = launches("jda_reduce_tiles"), launches("jda_resize_tiles")
            if max(p["factors"]) > T.MAX_FACTOR:
                assert rc == UNSUPPORTED and got is None and after == before, (req, gap, flt, rc)
                refused += 1
                continue
            assert rc == 0, (sampling, w, h, req, gap, flt, rc)
            want = np.asarray(pillow_thumbnail(f, req, flt, gap))
            assert got.shape[:2] == want.shape[:2] == (p["out"][1], p["out"][0])
            if gray:
                assert np.array_equal(got, want), (req, gap, flt, p)
            else:
                assert np.array_equal(got[..., :3], want) and np.all(got[..., 3] == 255), (req, gap, flt, p)
            steps = (int(p["factors"] != (1, 1)), int(p["resize"]))
            assert n == steps and (after[0] - before[0], after[1] - before[1]) == steps, (req, gap, flt, n, steps)
            seen.add((p["scale"],) + steps)
    assert {s for s, r, z in seen} == {1, 2, 4, 8} and {r for s, r, z in seen} == {0, 1} and (1, 0, 0) in seen, seen
    assert refused == (2 if (w, h) == (257, 640) else 0)                         # (100, 4) of 257 x 640: 64 columns a cell, beyond the cap


@pytest.mark.parametrize("sampling,w,h", [("4:2:0", 1030, 64), ("4:4:4", 333, 217)])
def test_gray_of_a_colour_file_is_the_luma_plane_through_the_same_steps(sampling, w, h, gpu_ctx):
    """JDA_EIGHT_BIT_GRAYSCALE of a colour file: no single Pillow call makes it, so the reference is the twin chain (held to Pillow in
    tests/test_thumbnail_cpu.py) over the exact road's luma plane at the plan's scale"""
    f = chain_file(sampling, w, h, "baseline")
    seen = set()
    for i, (req, gap) in enumerate(CHAIN_REQUESTS):
        flt = F.FILTERS[(i + 2) % 5]
        want, p = T.thumbnail(chain_decode(f, True), w, h, req, flt, gap)
        rc, got, n = J.decode_to_host_thumbnail(gpu_ctx, f, req, flt, gap, J.GRAY8)
        assert rc == 0 and n == (int(p["factors"] != (1, 1)), int(p["resize"])), (req, gap, flt, rc, n)
        assert got.shape == want.shape and np.array_equal(got, want), (sampling, req, gap, flt, p)
        seen.add((p["scale"], n[0]))
    assert {s for s, r in seen} == {1, 2, 4, 8} and {r for s, r in seen} == {0, 1}, seen


def saved(im, sampling, quality, **kw):
    b = io.BytesIO()
    if im.mode == "L":
        im.save(b, "JPEG", quality=quality, **kw)
    else:
        im.save(b, "JPEG", quality=quality, subsampling={"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}[sampling], **kw)
    return b.getvalue()


def test_thumbnails_pillow_are_pillows_files(gpu_ctx):
    colour = [chain_file(*c) for c in CHAIN_FILES if c[0] != "gray"] + [chain_file("4:2:0", 100, 37, "baseline"), chain_file("4:4:4", 24, 40, "optimize")]
    gray = [chain_file("gray", 333, 217, "baseline"), chain_file("gray", 31, 65, "baseline")]
    for files, size, flt, gap, sampling, q in ((colour, (128, 128), "bicubic", 2.0, "4:2:0", 80), (colour, (40, 70), "lanczos", 3.0, "4:4:4", 92),
                                                (colour, (100, 100), "bilinear", None, "4:2:2", 75), (gray, (50, 70), "hamming", 2.0, "gray", 85)):
        fid = J.binding.resize_filter(flt)
        plans = [T.plan(J.parse(f)["width"], J.parse(f)["height"], size, fid, gap) for f in files]
        assert any(p["factors"] != (1, 1) for p in plans) or gap is None
        assert any(not p["resize"] for p in plans), "a file already within the size"
        assert len({p["out"] for p in plans}) >= 3 or len(files) == 2
        ims = [pillow_thumbnail(f, size, fid, gap) for f in files]
        for kw, args in ((dict(), dict()), (dict(optimize=True), dict(optimize=True)), (dict(progressive=True), dict(progressive=True))):
            before = launches("jda_reduce_tiles"), launches("jda_resize_tiles")
            out = J.thumbnails(gpu_ctx, files, size, quality=q, sampling=sampling, resample=flt, pillow=True, reducing_gap=gap, **args)
            after = launches("jda_reduce_tiles"), launches("jda_resize_tiles")
            assert (after[0] - before[0], after[1] - before[1]) == (int(any(p["factors"] != (1, 1) for p in plans)), int(any(p["resize"] for p in plans))), "one launch a step for the list"
            for k, (im, t) in enumerate(zip(ims, out)):
                assert t == saved(im, sampling, q, **kw), (size, flt, gap, sampling, kw, k, plans[k])
    # pillow=False is what it was: the same call with and without the new arguments at their defaults
    a = J.thumbnails(gpu_ctx, colour[:2], (48, 64), quality=80, prescale=False)
    assert a == J.thumbnails(gpu_ctx, colour[:2], (48, 64), quality=80, prescale=False, pillow=False, reducing_gap=2.0)
    assert J.thumbnails(gpu_ctx, colour[:1], (20, 30)) == J.thumbnails(gpu_ctx, colour[:1], (20, 30), prescale=True)
    with pytest.raises(ValueError):
        J.thumbnails(gpu_ctx, [colour[0], gray[0]], (64, 64), pillow=True)


def test_refusals_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    a, b = ctx.malloc(1 << 16), ctx.malloc(1 << 12)
    ctx.memset(b, FILL, 1 << 12)
    before = launches("jda_reduce_tiles"), launches("jda_resize_tiles")
    rd, rb = ctx.lib.jda_reduce_surfaces, ctx.lib.jda_resize_surfaces_box
    import ctypes as C
    s, d = (Output * 1)(Output(a, 64, 50, 40)), (Output * 1)(Output(b, 32, 25, 20))
    f22 = (C.c_int32 * 2)(2, 2)
    for what, rc, want in (("factor 33", rd(ctx.handle, 1, s, 1, (C.c_int32 * 2)(33, 2), None, d), UNSUPPORTED), ("factor 0", rd(ctx.handle, 1, s, 1, (C.c_int32 * 2)(2, 0), None, d), INVALID),
                           ("wrong size", rd(ctx.handle, 1, s, 1, f22, None, (Output * 1)(Output(b, 32, 24, 20))), INVALID),
                           ("box leaves", rd(ctx.handle, 1, s, 1, f22, (C.c_int32 * 4)(0, 0, 51, 40), d), INVALID), ("pixel size 2", rd(ctx.handle, 1, s, 2, f22, None, d), INVALID),
                           ("n < 0", rd(ctx.handle, -1, s, 1, f22, None, d), INVALID), ("null factors", rd(ctx.handle, 1, s, 1, None, None, d), INVALID),
                           ("dst in src", rd(ctx.handle, 1, s, 1, f22, None, (Output * 1)(Output(a + 64, 32, 25, 20))), INVALID),
                           ("box beyond", rb(ctx.handle, 1, s, 1, (C.c_float * 4)(0, 0, 50.5, 40), d, 0), INVALID), ("box empty", rb(ctx.handle, 1, s, 1, (C.c_float * 4)(5, 0, 5, 40), d, 0), INVALID),
                           ("box negative", rb(ctx.handle, 1, s, 1, (C.c_float * 4)(-0.5, 0, 20, 40), d, 3), INVALID), ("no boxes", rb(ctx.handle, 1, s, 1, None, d, 3), INVALID),
                           ("filter 5", rb(ctx.handle, 1, s, 1, (C.c_float * 4)(0, 0, 50, 40), d, 5), INVALID),
                           ("beyond the tap cap", rb(ctx.handle, 1, s, 1, (C.c_float * 4)(0, 0, 50, 40), (Output * 1)(Output(b, 16, 1, 1)), F.LANCZOS), UNSUPPORTED)):
        assert rc == want, what
    assert rd(ctx.handle, 0, None, 1, None, None, None) == 0 and rb(ctx.handle, 0, None, 1, None, None, 0) == 0      # nothing to do, nothing launched
    f = chain_file("4:2:0", 257, 640, "baseline")
    rc, got, n = J.decode_to_host_thumbnail(ctx, f, (100, 4), F.BICUBIC, 2.0)                                            # 64 columns a cell
    assert rc == UNSUPPORTED and got is None and n == (0, 0)
    rc, got, n = J.decode_to_host_thumbnail(ctx, f, (50, 50), F.BICUBIC, 0.5)
    assert rc == INVALID and got is None
    small = np.zeros((4, 16), np.uint8)
    assert ctx.lib.jda_decode_to_host_thumbnail(ctx.handle, f, len(f), 50, 50, 3, C.c_double(2.0), J.RGB8888, small.ctypes.data, 16, 4, None, None, None) == INVALID      # the host rows do not hold 20 x 50
    assert ctx.lib.jda_decode_to_host_thumbnail(ctx.handle, f, len(f), 50, 50, 3, C.c_double(2.0), J.RGB565_LE, small.ctypes.data, 16, 4, None, None, None) == INVALID
    assert (launches("jda_reduce_tiles"), launches("jda_resize_tiles")) == before and np.all(ctx.to_host(b, 1 << 12) == FILL), "a refused call launches nothing and writes nothing"
    assert rd(ctx.handle, 1, s, 1, f22, None, d) == 0 and launches("jda_reduce_tiles") == before[0] + 1
    ctx.free(a)
    ctx.free(b)
