"""jda_unpack_surfaces on the GPU: (a) the whole grid of tests/test_unpack_cpu.py -- every width, height, source offset, pitch -- as the jobs
of ONE launch per (format, element type, parameter set) into one allocation filled with 0xA5, against the numpy twin (tests/unpack_util.py),
the guard everywhere else, the sources unchanged; (b) every instance of the kernel; (c) a pipeline batch packed and unpacked again; (d) unpack
then each of the three encoders over the encoder's own grid, against the encoders' twins and Pillow; (e) jda_encode_dense_to_host; (f) decode
to a dense image and encode it again = jda_transcode_to_host; (g) refusals that launch nothing; (h) encode_tensors from torch tensors, in a
process of its own (tests/unpack_torch_child.py).  Everything is bit-exact."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.binding import ImageInfo, Output
from tests import encode_opt_util as O
from tests import encode_prog_util as P
from tests import encode_util as E
from tests import unpack_util as U
from tests.cases import jpeg_for
from tests.unpack_util import BGR, CHW, DTYPES, F16, F32, FORMATS, GUARD, HWC, U8

pytestmark = pytest.mark.gpu

INVALID, ERROR_MEMORY = 1, 5
PIPELINE_FILES = ("c420_1280x720", "c420_640x368_rstrow", "c444_384x192_q100_rst7", "c420_333x217", "c422_333x217")
LOOP_FILES = (("gray_333x217", "gray"), ("c444_333x217", "4:4:4"), ("c422_333x217", "4:2:2"), ("c420_333x217", "4:2:0"))
FORMS = ("baseline", "optimize", "progressive")


def unpack_counts():
    return {k: v for k, v in J.kernel_launch_counts().items() if "jda_unpack_tiles" in k}


def unpack_launches():
    return sum(unpack_counts().values())


def a16(v):
    return (v + 15) & ~15


@pytest.mark.parametrize("elem", [U8, F16, F32])
@pytest.mark.parametrize("bpp,flags", FORMATS)
def test_whole_grid_in_one_launch(bpp, flags, elem, gpu_ctx):
    ctx = gpu_ctx
    channels = 3 if bpp == 4 else 1
    for name, sb in U.param_sets(channels).items():
        if elem == U8 and name != "default":
            continue
        rng = np.random.RandomState(900 + 10 * flags + bpp + 100 * elem + len(name))
        jobs = U.grid_jobs(rng, bpp, flags, elem, sb)
        # one allocation: every job's source `offset` bytes behind a 16-byte boundary, its surface behind it, at least 32 guard bytes between all of them
        cursor = 0
        for j in jobs:
            j["src_at"] = a16(cursor) + 32 + j["offset"]
            j["dst_at"] = a16(j["src_at"] + j["src"].size) + 32
            cursor = j["dst_at"] + j["pitch"] * j["h"] + 32
        total = a16(cursor)
        host = np.full(total, GUARD, np.uint8)
        for j in jobs:
            host[j["src_at"]:j["src_at"] + j["src"].size] = j["src"]
        base = ctx.malloc(total)
        assert base % 16 == 0
        ctx.from_host(base, host)
        before = unpack_launches()
        J.unpack_surfaces(ctx, [base + j["src_at"] for j in jobs], [(base + j["dst_at"], j["pitch"], j["w"], j["h"]) for j in jobs], bpp, flags, elem, sb)
        assert unpack_launches() == before + 1, "one launch for the whole batch"
        got = ctx.to_host(base, total)
        ctx.free(base)
        for j in jobs:
            surf = got[j["dst_at"]:j["dst_at"] + j["pitch"] * j["h"]].reshape(j["h"], j["pitch"])
            rb = j["w"] * bpp
            assert np.array_equal(surf[:, :rb], j["want"]), (name, j["w"], j["h"], j["offset"], j["pitch"])
            host[j["dst_at"]:j["dst_at"] + j["pitch"] * j["h"]].reshape(j["h"], j["pitch"])[:, :rb] = j["want"]
        assert np.array_equal(got, host), "%s: a byte outside the rows was written (padding, guard or a source)" % name
        if elem == F32 and name in ("imagenet", "negative"):
            assert sum(j["fused_differs"] for j in jobs) >= 16


def test_every_unpack_instance_is_launched(gpu_ctx):
    """a small job through each (layout, element size) instance of the kernel; the code object has six"""
    ctx = gpu_ctx
    rng = np.random.RandomState(3)
    base = ctx.malloc(1 << 16)
    for bpp, flags in ((4, HWC), (4, CHW | BGR), (1, CHW)):
        for elem in (U8, F16, F32):
            channels, es = (3 if bpp == 4 else 1), np.dtype(DTYPES[elem]).itemsize
            sb = None if elem == U8 else U.param_sets(channels)["imagenet"]
            src = U.dense_bytes(U.random_image(rng, 17, 9, channels, elem, sb), flags)
            ctx.memset(base, GUARD, 1 << 16)
            ctx.from_host(base + es, src)
            J.unpack_surfaces(ctx, [base + es], [(base + 8192, 80, 17, 9)], bpp, flags, elem, sb)
            got = ctx.to_host(base + 8192, 80 * 9).reshape(9, 80)
            assert np.array_equal(got[:, :17 * bpp], U.numpy_unpack(src, 17, 9, bpp, flags, elem, sb)) and np.all(got[:, 17 * bpp:] == GUARD), (bpp, flags, elem)
    ctx.free(base)
    counts = unpack_counts()
    assert len(counts) == 6 and all(v > 0 for v in counts.values()), counts


def test_pipeline_batch_packed_and_unpacked_again(gpu_ctx):
    ctx = gpu_ctx
    files = [jpeg_for(n) for n in PIPELINE_FILES]
    infos = []
    for f in files:
        info = ImageInfo()
        assert ctx.lib.jda_parse(f, len(f), C.byref(info)) == 0
        infos.append(info)
    geos = [J.output_geometry(i, J.RGB8888, 0) for i in infos]
    n = len(files)
    pit = [a16(g["canvas_w"] * 4) for g in geos]
    offs, total = [], 0
    for g, p in zip(geos, pit):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    doffs = []
    for g in geos:                                      # the dense images back to back, a guard byte between them: none of them aligned
        doffs.append(total + 1)
        total += g["out_w"] * g["out_h"] * 3 + 1
    total = a16(total)
    upit = [a16(g["out_w"] * 4) + 16 for g in geos]
    uoffs = []
    for g, p in zip(geos, upit):
        uoffs.append(total)
        total += p * g["out_h"]
    base = ctx.malloc(total)
    ctx.memset(base, GUARD, total)
    pipe = J.Pipeline(ctx, max_images=n, depth=2)
    st = pipe.wait(pipe.submit(files, [(base + offs[i], pit[i], geos[i]["canvas_w"], geos[i]["canvas_h"]) for i in range(n)], [J.RGB8888] * n, [0] * n))
    pipe.close()
    assert list(st) == [0] * n, st
    for flags in (HWC, CHW | BGR):
        visible = [(base + offs[i], pit[i], geos[i]["out_w"], geos[i]["out_h"]) for i in range(n)]
        J.pack_surfaces(ctx, visible, 4, [base + d for d in doffs], flags, U8)
        before = unpack_launches()
        J.unpack_surfaces(ctx, [base + d for d in doffs], [(base + uoffs[i], upit[i], geos[i]["out_w"], geos[i]["out_h"]) for i in range(n)], 4, flags, U8)
        assert unpack_launches() == before + 1
        for i, g in enumerate(geos):
            w, h = g["out_w"], g["out_h"]
            canvas = ctx.to_host(base + offs[i], pit[i] * g["canvas_h"]).reshape(g["canvas_h"], pit[i])[:h, :w * 4].reshape(h, w, 4).copy()
            canvas[..., 3] = 0xFF
            back = ctx.to_host(base + uoffs[i], upit[i] * h).reshape(h, upit[i])
            assert np.array_equal(back[:, :w * 4].reshape(h, w, 4), canvas), (PIPELINE_FILES[i], flags)
            assert np.all(back[:, w * 4:] == GUARD), PIPELINE_FILES[i]
    ctx.free(base)


@functools.lru_cache(maxsize=None)
def grid_case(sampling, k):
    """size k of the encoder's grid as a dense image of a layout and element type that turn with k -> (dense bytes, w, h, bpp, flags, elem, the twin's pixels)"""
    w, h = E.SIZES[k]
    kind, q = O.GRID_PICTURES[k % len(O.GRID_PICTURES)]
    pic = E.picture(kind, w, h, sampling, seed=k)
    gray = sampling == "gray"
    bpp, channels = (1, 1) if gray else (4, 3)
    flags = CHW if gray else (HWC, CHW, HWC | BGR, CHW | BGR)[k % 4]
    elem = (U8, F32, U8, F16)[k % 4]
    img = pic[..., None] if gray else pic[..., :3]
    if elem != U8:
        img = (img.astype(np.float64) / 255.0).astype(DTYPES[elem])              # (float16 does not hold every v / 255: the twin says which byte comes back)
    src = U.dense_bytes(np.ascontiguousarray(img), flags)
    px = U.numpy_unpack(src, w, h, bpp, flags, elem)
    return src, w, h, bpp, flags, elem, (px if gray else px.reshape(h, w, 4)), q


def pillow_opens(f, w, h):
    from PIL import Image
    im = Image.open(io.BytesIO(f))
    im.load()
    assert im.size == (w, h)


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_unpack_then_each_encoder_over_the_encoders_grid(sampling, gpu_ctx):
    from tests.test_encode_cpu import body, pillow_file
    from tests.test_encode_opt_cpu import same_as_pillow
    from tests.test_encode_prog_cpu import from_sof2
    from tests.test_encode_prog_cpu import pillow_file as pillow_prog
    ctx = gpu_ctx
    cases = [grid_case(sampling, k) for k in range(len(E.SIZES))]
    bpp = cases[0][3]
    caps = [J.encode_bound_progressive(c[1], c[2], sampling) for c in cases]
    pitches = [a16(c[1] * bpp) for c in cases]
    at, total = [], 0
    for c, p, cap in zip(cases, pitches, caps):
        s_at = a16(total) + np.dtype(DTYPES[c[5]]).itemsize          # (one element off a 16-byte boundary)
        d_at = a16(s_at + c[0].size)
        f_at = d_at + p * c[2]
        at.append((s_at, d_at, f_at))
        total = f_at + cap
    base = ctx.malloc(a16(total))
    files = {form: [None] * len(cases) for form in FORMS}
    # one unpack launch per (layout, element type) of the grid, then one call of each encoder over all the surfaces
    for key in sorted(set((c[4], c[5]) for c in cases)):
        idx = [i for i, c in enumerate(cases) if (c[4], c[5]) == key]
        for i in idx:
            ctx.from_host(base + at[i][0], cases[i][0])
        J.unpack_surfaces(ctx, [base + at[i][0] for i in idx], [(base + at[i][1], pitches[i], cases[i][1], cases[i][2]) for i in idx], bpp, key[0], key[1])
    surfaces = [(base + at[i][1], pitches[i], c[1], c[2]) for i, c in enumerate(cases)]
    jobs = [(0, 0, c[1], c[2], sampling, c[7], 0) for c in cases]
    dsts = [base + a[2] for a in at]
    for form in FORMS:
        if form == "progressive":
            nbytes, st = J.encode_surfaces_progressive(ctx, surfaces, bpp, jobs, dsts, caps)
        else:
            nbytes, st = J.encode_surfaces(ctx, surfaces, bpp, jobs, dsts, caps, [J.ENCODE_OPTIMIZE] * len(cases) if form == "optimize" else None)
        assert st == [0] * len(cases), (form, st)
        files[form] = [ctx.to_host(dsts[i], nbytes[i]).tobytes() for i in range(len(cases))]
    ctx.free(base)
    for i, (src, w, h, _, flags, elem, px, q) in enumerate(cases):
        what = (sampling, w, h, flags, elem)
        assert files["baseline"][i] == E.file_bytes(px, sampling, q), what
        assert files["optimize"][i] == O.file_bytes_opt(px, sampling, q), what
        assert files["progressive"][i] == P.file_bytes_prog(px, sampling, q), what
        # .. and Pillow's save() of the same array (none of these shapes is skipped)
        assert body(files["baseline"][i]) == body(pillow_file(px, sampling, q, 0)), what
        same_as_pillow(files["optimize"][i], px, sampling, q, 0)
        assert from_sof2(files["progressive"][i]) == from_sof2(pillow_prog(px, sampling, q)), what
        for form in FORMS:
            pillow_opens(files[form][i], w, h)


def dense_call(ctx, a, w, h, channels, flags, elem, sb, sampling, quality, ri, form, capacity, buf):
    nbytes = C.c_int64(-1)
    sbp = None if sb is None else (C.c_float * (2 * channels))(*[float(v) for v in np.asarray(sb, np.float32).reshape(-1)])
    rc = ctx.lib.jda_encode_dense_to_host(ctx.handle, None if a is None else a.ctypes.data_as(C.c_void_p), w, h, channels, flags, elem, sbp, sampling, quality, ri, form,
                                          None if buf is None else buf.ctypes.data_as(C.c_void_p), capacity, C.byref(nbytes))
    return rc, nbytes.value


def test_encode_dense_to_host(gpu_ctx):
    ctx = gpu_ctx
    w, h = 33, 47
    pic = E.picture("noise", w, h, "4:2:0", seed=11)
    rgb = np.ascontiguousarray(pic[..., :3])
    px = pic.copy()
    px[..., 3] = 0xFF
    want = {"baseline": E.file_bytes(px, "4:2:0", 75), "optimize": O.file_bytes_opt(px, "4:2:0", 75), "progressive": P.file_bytes_prog(px, "4:2:0", 75)}
    mean, std = U.IMAGENET_MEAN, U.IMAGENET_STD
    table = J.normalise_table(mean, std, np.float32)
    normalised = np.stack([table[c][rgb[..., c]] for c in range(3)])                  # [3, h, w] float32: every byte comes back through denormalise_params
    for form in FORMS:
        rc, f, n = J.encode_dense_to_host(ctx, rgb, J.PACK_HWC, "4:2:0", 75, 0, form)
        assert rc == 0 and f == want[form] and n == len(f), form
        rc, f, n = J.encode_dense_to_host(ctx, normalised, J.PACK_CHW, "4:2:0", 75, 0, form, scale_bias=J.denormalise_params(mean, std))
        assert rc == 0 and f == want[form], form
        pillow_opens(f, w, h)
        # a capacity one byte short: the size it needs, the buffer untouched; and exactly enough
        buf = np.full(len(want[form]) + 8, GUARD, np.uint8)
        assert dense_call(ctx, rgb, w, h, 3, HWC, U8, None, 3, 75, 0, FORMS.index(form), len(want[form]) - 1, buf) == (ERROR_MEMORY, len(want[form])), form
        assert np.all(buf == GUARD), form
        assert dense_call(ctx, rgb, w, h, 3, HWC, U8, None, 3, 75, 0, FORMS.index(form), len(want[form]), buf) == (0, len(want[form])), form
        assert buf[:-8].tobytes() == want[form] and np.all(buf[-8:] == GUARD), form
    # BGR, a restart interval, gray in float16
    rc, f, n = J.encode_dense_to_host(ctx, np.ascontiguousarray(rgb[..., ::-1]), J.PACK_HWC | J.PACK_BGR, "4:4:4", 90, 3)
    assert rc == 0 and f == E.file_bytes(px, "4:4:4", 90, 3)
    g = E.picture("smooth", 40, 40, "gray")
    rc, f, n = J.encode_dense_to_host(ctx, (g.astype(np.float64) / 255.0).astype(np.float16), J.PACK_CHW, "4:2:0", 60)      # (gray takes the gray sampling)
    assert rc == 0 and f == E.file_bytes(U.numpy_unpack((g.astype(np.float64) / 255.0).astype(np.float16).reshape(-1).view(np.uint8), 40, 40, 1, CHW, F16), "gray", 60)
    # refusals
    before = unpack_launches()
    buf = np.full(1 << 16, GUARD, np.uint8)
    gray = np.ascontiguousarray(g)
    sb3 = np.array([255, 255, 255, 0, 0, 0], np.float32)
    for what, got in (
            ("a gray image with a colour sampling", dense_call(ctx, gray, 40, 40, 1, CHW, U8, None, 3, 75, 0, 0, buf.size, buf)),
            ("a colour image with the gray sampling", dense_call(ctx, rgb, w, h, 3, HWC, U8, None, 0, 75, 0, 0, buf.size, buf)),
            ("two channels", dense_call(ctx, rgb, w, h, 2, HWC, U8, None, 3, 75, 0, 0, buf.size, buf)),
            ("an unknown form", dense_call(ctx, rgb, w, h, 3, HWC, U8, None, 3, 75, 0, 3, buf.size, buf)),
            ("progressive with a restart interval", dense_call(ctx, rgb, w, h, 3, HWC, U8, None, 3, 75, 2, 2, buf.size, buf)),
            ("quality 0", dense_call(ctx, rgb, w, h, 3, HWC, U8, None, 3, 0, 0, 0, buf.size, buf)),
            ("scale_bias with U8", dense_call(ctx, rgb, w, h, 3, HWC, U8, sb3, 3, 75, 0, 0, buf.size, buf)),
            ("an unknown layout bit", dense_call(ctx, rgb, w, h, 3, 4, U8, None, 3, 75, 0, 0, buf.size, buf)),
            ("an unknown element type", dense_call(ctx, rgb, w, h, 3, HWC, 3, None, 3, 75, 0, 0, buf.size, buf)),
            ("no image", dense_call(ctx, None, w, h, 3, HWC, U8, None, 3, 75, 0, 0, buf.size, buf)),
            ("no buffer", dense_call(ctx, rgb, w, h, 3, HWC, U8, None, 3, 75, 0, 0, buf.size, None)),
            ("w == 0", dense_call(ctx, rgb, 0, h, 3, HWC, U8, None, 3, 75, 0, 0, buf.size, buf)),
            ("a negative capacity", dense_call(ctx, rgb, w, h, 3, HWC, U8, None, 3, 75, 0, 0, -1, buf)),
    ):
        assert got == (INVALID, 0), what
    assert np.all(buf == GUARD) and unpack_launches() == before, "a refused call writes nothing and launches nothing"
    assert ctx.lib.jda_encode_dense_to_host(None, None, 1, 1, 3, HWC, U8, None, 3, 75, 0, 0, None, 0, None) == 6          # JDA_ERROR_NO_DEVICE


@pytest.mark.parametrize("name,sampling", LOOP_FILES)
def test_decode_packed_then_encode_dense_is_transcode(name, sampling, gpu_ctx):
    """the loop closes: a file decoded to a dense image and that image encoded again = the file jda_transcode_to_host makes of it"""
    ctx = gpu_ctx
    jpeg = jpeg_for(name)
    for flags in ((HWC,) if sampling == "gray" else (HWC, CHW | BGR)):
        rc, dense, g = J.decode_packed_to_host(ctx, jpeg, 0, flags, U8)
        assert rc == 0 and (g["w"], g["h"]) == (333, 217)
        for form in FORMS:
            rc, want, n = J.transcode_to_host(ctx, jpeg, None, sampling, 80, optimize=form == "optimize", progressive=form == "progressive")
            assert rc == 0
            rc, got, n = J.encode_dense_to_host(ctx, dense, flags, sampling, 80, 0, form)
            assert rc == 0 and got == want, (name, flags, form)
            pillow_opens(got, 333, 217)


def test_unpack_surfaces_refusals_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    lib = ctx.lib
    a, b = ctx.malloc(1 << 16), ctx.malloc(1 << 16)
    ctx.memset(a, 7, 1 << 16)
    ctx.memset(b, GUARD, 1 << 16)
    good = (C.c_float * 6)(255, 255, 255, 0, 0, 0)

    def sbp(i, v, size=6):
        q = [255.0] * (size // 2) + [0.0] * (size // 2)
        q[i] = v
        return (C.c_float * size)(*q)

    def call(src=a + 3, dst=(b, 64, 10, 20), bpp=4, flags=HWC, elem=U8, sb=None, n=1, arrays=True):
        s = (C.c_void_p * 1)(src) if arrays else None
        d = (Output * 1)(Output(*dst)) if arrays else None
        return lib.jda_unpack_surfaces(ctx.handle, n, s, flags, elem, sb, d, bpp)
    before = unpack_launches()
    assert call(n=0) == 0 and call(n=0, arrays=False) == 0 and unpack_launches() == before                   # nothing to do, nothing launched
    for what, rc in (
            ("null dst pixels", call(dst=(0, 64, 10, 20))), ("null src", call(src=0)), ("null arrays", call(arrays=False)), ("n < 0", call(n=-1)),
            ("pixel size 2", call(bpp=2)), ("pixel size 3", call(bpp=3)), ("unknown layout bit", call(flags=4)), ("unknown element type", call(elem=3)),
            ("unknown layout with n == 0", call(flags=4, n=0)), ("pixel size 2 with n == 0", call(bpp=2, n=0)),
            ("BGR with one channel", call(bpp=1, dst=(b, 16, 10, 20), flags=BGR)), ("scale_bias with U8", call(sb=good)),
            ("infinite scale", call(elem=F32, src=a, sb=sbp(1, float("inf")))), ("NaN bias", call(elem=F16, src=a, sb=sbp(4, float("nan")))),
            ("misaligned F16 src", call(elem=F16, src=a + 1)), ("misaligned F32 src", call(elem=F32, src=a + 2)),
            ("misaligned dst", call(dst=(b + 4, 64, 10, 20))), ("pitch too small", call(dst=(b, 32, 10, 20))), ("pitch not a multiple of 16", call(dst=(b, 72, 10, 20))),
            ("w == 0", call(dst=(b, 64, 0, 20))), ("h < 0", call(dst=(b, 64, 10, -5))),
            ("dst is src", call(src=b)), ("src begins inside dst's rows", call(src=b + 64 * 19 + 8)), ("dst begins inside src", call(src=b - 100)),
            ("source over JDA_PACK_MAX_BYTES", call(dst=(b, 65536 * 4, 65536, 16384))),
    ):
        assert rc == INVALID, what
    assert unpack_launches() == before and np.all(ctx.to_host(b, 1 << 16) == GUARD), "a refused call launches nothing and writes nothing"
    assert call() == 0 and unpack_launches() == before + 1
    got = ctx.to_host(b, 64 * 20).reshape(20, 64)
    assert np.all(got[:, :40].reshape(20, 10, 4) == [7, 7, 7, 255]) and np.all(got[:, 40:] == GUARD)
    assert call(src=b + 64 * 19 + 40) == 0 and unpack_launches() == before + 2                               # side by side is fine
    assert lib.jda_unpack_surfaces(None, 1, None, HWC, U8, None, None, 4) == 6                               # JDA_ERROR_NO_DEVICE
    ctx.free(a)
    ctx.free(b)


def test_encode_tensors(gpu_ctx):
    """encode_tensors against the encoders' twins (tests/unpack_torch_child.py), in a process of its own: torch has to be imported BEFORE
    libjpegdec_amd.so is loaded where torch brings a HIP runtime of its own, and this process loaded the library long ago"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "unpack_torch_child.py")], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "unpack_torch_child ok" in r.stdout, r.stdout[-4000:]
