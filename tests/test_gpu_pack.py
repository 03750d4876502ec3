"""jda_pack_surfaces on the GPU: (a) random surfaces over the size x rectangle x destination-offset grid of tests/test_pack_cpu.py, all jobs of
a (source, layout, element type) combination in one launch, against the numpy expressions, guard bytes included; (b) jda_decode_to_host_packed
against the oracle's canvas cut and permuted by numpy; (c) a streamed pipeline batch packed where it lies in HBM; (d) decode_to_tensors into
torch tensors; (e) refusals that launch nothing.  Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.binding import ImageInfo, Output
from tests import orient_util as U
from tests.cases import jpeg_for
from tests.test_pack_cpu import BGR, CHW, DTYPES, F16, F32, FORMATS, GUARD, HEIGHTS, HWC, INVALID, ORIGINS, U8, U8_OFFSETS, WIDTHS, numpy_pack

pytestmark = pytest.mark.gpu

SCALES = (0, J.SCALE_HALF, J.SCALE_QUARTER, J.SCALE_EIGHTH)
ONE_CALL_FILES = ("gray_333x217", "c420_333x217", "c444_333x217", "c422_333x217", "c440_200x120")
PIPELINE_FILES = ("c420_1280x720", "c420_640x368_rstrow", "c444_384x192_q100_rst7", "c444_256x256_q100_opt", "c420_333x217", "c420_512x256_q98_rstrow", "c422_333x217")


def pack_counts():
    return {k: v for k, v in J.kernel_launch_counts().items() if "jda_pack_tiles" in k}


def pack_launches():
    return sum(pack_counts().values())


def random_table(rng, channels, elem):
    """random bit patterns of the element type, as bytes [channels * 256 * es]"""
    return None if elem == U8 else rng.randint(0, 256, channels * 256 * np.dtype(DTYPES[elem]).itemsize).astype(np.uint8)


def upload(ctx, data):
    ptr = ctx.malloc(max(int(data.size), 16))
    ctx.from_host(ptr, data)
    return ptr


@pytest.mark.parametrize("elem", [U8, F16, F32])
@pytest.mark.parametrize("bpp,flags", FORMATS)
def test_every_size_rectangle_and_offset_in_one_launch(bpp, flags, elem, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.RandomState(500 + 10 * flags + bpp + 100 * elem)
    channels = 3 if bpp == 4 else 1
    es = np.dtype(DTYPES[elem]).itemsize
    # one random surface (alpha bytes and padding random) that every rectangle of the launch is cut from; a pitch wider than its rows
    width, rows = max(WIDTHS) + 7 + 2, max(HEIGHTS) + 5 + 1
    pitch = ((width * bpp + 15) & ~15) + 16
    surface = rng.randint(0, 256, (rows, pitch)).astype(np.uint8)
    table = random_table(rng, channels, elem)
    offsets = U8_OFFSETS if elem == U8 else tuple(sorted(set(es * k % 16 for k in (0, 1, 2, 3, 5, 15))))
    jobs, cursor = [], 0
    for k, (w, h) in enumerate((w, h) for w in WIDTHS for h in HEIGHTS):
        # bytes: every origin with every offset; through a table: every origin and every offset in turn
        pairs = [(o, f) for o in ORIGINS for f in offsets] if elem == U8 else [(ORIGINS[(k + i) % len(ORIGINS)], offsets[(k + i) % len(offsets)]) for i in range(len(ORIGINS))]
        for (x, y), off in pairs:
            nbytes = w * h * channels * es
            start = ((cursor + 15) & ~15) + 32 + off                 # `off` bytes behind a 16-byte boundary, >= 32 guard bytes in front
            jobs.append((x, y, w, h, start, nbytes))
            cursor = start + nbytes + 32
    total = (cursor + 15) & ~15
    dsrc, ddst = upload(ctx, surface.reshape(-1)), ctx.malloc(total)
    dtab = None if table is None else upload(ctx, table)
    ctx.memset(ddst, GUARD, total)
    assert ddst % 16 == 0 and (dtab is None or dtab % 16 == 0)
    before = pack_launches()
    J.pack_surfaces(ctx, [(dsrc, pitch, width, rows)] * len(jobs), bpp, [ddst + j[4] for j in jobs], flags, elem, dtab, rects=[j[:4] for j in jobs])
    assert pack_launches() == before + 1, "one launch for the whole batch"
    got = ctx.to_host(ddst, total)
    assert np.array_equal(ctx.to_host(dsrc, surface.size), surface.reshape(-1)), "the source is left as it is"
    ctx.free(dsrc)
    ctx.free(ddst)
    if dtab is not None:
        ctx.free(dtab)
    guard = np.ones(total, bool)
    for (x, y, w, h, start, nbytes) in jobs:
        assert np.array_equal(got[start:start + nbytes], numpy_pack(surface, bpp, (x, y, w, h), flags, elem, table)), (w, h, x, y, start % 16)
        guard[start:start + nbytes] = False
    assert np.all(got[guard] == GUARD), "a byte outside every destination was written"


def test_every_pack_instance_is_launched(gpu_ctx):
    """a small job through each (layout, element size) instance of the kernel; the code object has six"""
    ctx = gpu_ctx
    rng = np.random.RandomState(3)
    surface = rng.randint(0, 256, (9, 80)).astype(np.uint8)
    dsrc, ddst = upload(ctx, surface.reshape(-1)), ctx.malloc(4096)
    for bpp, flags in ((4, HWC), (4, CHW), (1, CHW)):
        for elem in (U8, F16, F32):
            channels, es = (3 if bpp == 4 else 1), np.dtype(DTYPES[elem]).itemsize
            table = random_table(rng, channels, elem)
            dtab = None if table is None else upload(ctx, table)
            J.pack_surfaces(ctx, [(dsrc, 80, 17, 9)], bpp, [ddst + es], flags, elem, dtab)
            got = ctx.to_host(ddst + es, 17 * 9 * channels * es)
            assert np.array_equal(got, numpy_pack(surface, bpp, (0, 0, 17, 9), flags, elem, table)), (bpp, flags, elem)
            if dtab is not None:
                ctx.free(dtab)
    ctx.free(dsrc)
    ctx.free(ddst)
    counts = pack_counts()
    assert len(counts) == 6 and all(v > 0 for v in counts.values()), counts


def expected_packed(oracle, jpeg, options, flags, elem, table, zero_from=None):
    """the oracle's canvas (RGB8888, or GRAY8 for a gray file / JDA_LUMA_ONLY), its visible rectangle packed by numpy -> (bytes, w, h, channels)"""
    info = ImageInfo()
    assert J.load_library().jda_parse(jpeg, len(jpeg), C.byref(info)) == 0
    gray = info.ncomp == 1 or bool(options & J.LUMA_ONLY)
    pt = J.GRAY8 if gray else J.RGB8888
    g = J.output_geometry(info, pt, options)
    rc, canvas, err = oracle.decode_canvas(jpeg, pt, options)
    if zero_from is None:
        assert rc == 1, err
    else:
        canvas = U.zero_undecoded(canvas, J.parse(jpeg), zero_from)
    tab = None if table is None else np.ascontiguousarray(table).view(np.uint8).reshape(-1)
    return numpy_pack(np.ascontiguousarray(canvas), g["bpp"], (0, 0, g["out_w"], g["out_h"]), flags, elem, tab), g["out_w"], g["out_h"], 1 if gray else 3


def check_one_call(ctx, oracle, jpeg, options, flags, elem, table=None):
    want, w, h, channels = expected_packed(oracle, jpeg, options, flags, elem, table)
    rc, got, g = J.decode_packed_to_host(ctx, jpeg, options, flags, elem, table)
    assert rc == 0, (rc, options, flags, elem)
    assert (g["w"], g["h"], g["channels"]) == (w, h, channels)
    assert got.shape == ((channels, h, w) if flags & CHW else (h, w, channels)) and got.dtype == DTYPES[elem]
    assert np.array_equal(got.reshape(-1).view(np.uint8), want), (options, flags, elem)


@pytest.mark.parametrize("name", ONE_CALL_FILES)
def test_one_call_equals_the_oracle_packed_by_numpy(name, gpu_ctx, oracle):
    jpeg = jpeg_for(name)
    gray = name.startswith("gray")
    mean, std = ((0.5,), (0.25,)) if gray else ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    for opt in SCALES:
        for flags in ((HWC, CHW) if gray else (HWC, CHW, HWC | BGR, CHW | BGR)):
            check_one_call(gpu_ctx, oracle, jpeg, opt, flags, U8)
        check_one_call(gpu_ctx, oracle, jpeg, opt, CHW, F32, J.normalise_table(mean, std, np.float32))
        check_one_call(gpu_ctx, oracle, jpeg, opt, HWC, F16, J.normalise_table(mean, std, np.float16))
    if not gray:                                        # JDA_LUMA_ONLY: one channel from a colour file
        check_one_call(gpu_ctx, oracle, jpeg, J.LUMA_ONLY, CHW, U8)
        check_one_call(gpu_ctx, oracle, jpeg, J.LUMA_ONLY | J.SCALE_HALF, HWC, F32, J.normalise_table((0.5,), (0.5,)))


def test_one_call_bad_mcu_progressive_thumbnail_and_refusals(gpu_ctx, oracle):
    ctx = gpu_ctx
    # a stream with a bad MCU: zeros from the bad MCU on BEFORE the pack, the whole result delivered, JDA_DECODE_ERROR
    bad, nok = U.bad_mcu_jpeg()
    table = J.normalise_table((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    for flags, elem, tab in ((HWC, U8, None), (CHW | BGR, U8, None), (CHW, F32, table)):
        rc, got, g = J.decode_packed_to_host(ctx, bad, 0, flags, elem, tab)
        assert rc == 2 and g["mcus_decoded"] == nok                                        # JDA_DECODE_ERROR
        want, w, h, channels = expected_packed(oracle, bad, 0, flags, elem, tab, zero_from=nok)
        assert (g["w"], g["h"]) == (333, 217) and np.array_equal(got.reshape(-1).view(np.uint8), want), (flags, elem)
    rc, got, g = J.decode_packed_to_host(ctx, bad, 0, HWC, U8)
    assert got.any() and not got[217 - 16:, 333 - 16:].any()                               # the end of the image was never reached
    # a progressive file is its 1/8 thumbnail; with JDA_SCALE_HALF its 1/2 ... as jda_decode_to_host_ex
    for name in ("p420_200x120", "p444_333x217", "pgray_100x100"):
        for flags in (HWC, CHW):
            check_one_call(ctx, oracle, jpeg_for(name), 0, flags, U8)
            check_one_call(ctx, oracle, jpeg_for(name), J.SCALE_EIGHTH, flags, U8)
            check_one_call(ctx, oracle, jpeg_for(name), J.SCALE_HALF, flags, U8)
    # refusals: the codes of jda_decode_to_host_ex / jda_output_geometry, and the bit that only three entry points take
    prog, base = jpeg_for("p420_200x120"), jpeg_for("c420_333x217")
    before = pack_launches()
    assert J.decode_packed_to_host(ctx, prog, J.PROGRESSIVE_FULL)[0] == 3                  # JDA_UNSUPPORTED_FEATURE
    assert J.decode_packed_to_host(ctx, prog, J.SCALE_QUARTER)[0] == 3                     # 1/4 of a progressive file: as jda_output_geometry refuses it
    assert J.decode_packed_to_host(ctx, base, J.SCALE_HALF | J.SCALE_QUARTER)[0] == 3      # two scale bits
    assert J.decode_packed_to_host(ctx, base, 0, 4)[0] == INVALID                          # unknown layout bit
    assert J.decode_packed_to_host(ctx, base, 0, HWC, 3)[0] == INVALID                     # unknown element type
    assert J.decode_packed_to_host(ctx, base, 0, HWC, F32)[0] == INVALID                   # no table
    assert J.decode_packed_to_host(ctx, base, 0, HWC, U8, table)[0] == INVALID             # a table with bytes
    assert J.decode_packed_to_host(ctx, jpeg_for("gray_333x217"), 0, BGR)[0] == INVALID    # BGR of one channel
    host = np.full(333 * 217 * 3 + 8, GUARD, np.uint8)
    call = ctx.lib.jda_decode_to_host_packed
    assert call(ctx.handle, base, len(base), 0, HWC, U8, None, host.ctypes.data_as(C.c_void_p), 333 * 217 * 3 - 1, None, None, None) == INVALID      # too small
    assert call(ctx.handle, base, len(base), 0, HWC, U8, None, None, 1 << 20, None, None, None) == INVALID
    assert np.all(host == GUARD) and pack_launches() == before, "a refused call writes nothing and launches nothing"
    assert J.decode_packed_to_host(ctx, base, J.PROGRESSIVE_FULL)[0] == 0                  # (a baseline file: the bit means nothing)
    # exactly the dense bytes are written
    assert call(ctx.handle, base, len(base), 0, HWC, U8, None, host.ctypes.data_as(C.c_void_p), host.size, None, None, None) == 0
    assert np.array_equal(host[:-8], expected_packed(oracle, base, 0, HWC, U8, None)[0]) and np.all(host[-8:] == GUARD)


def test_pipeline_batch_then_pack_its_resident_outputs(gpu_ctx, oracle):
    ctx = gpu_ctx
    files = [jpeg_for(n) for n in PIPELINE_FILES]
    infos = []
    for f in files:
        info = ImageInfo()
        assert ctx.lib.jda_parse(f, len(f), C.byref(info)) == 0
        infos.append(info)
    geos = [J.output_geometry(i, J.RGB8888, 0) for i in infos]
    pit = [(g["canvas_w"] * 4 + 15) & ~15 for g in geos]
    offs, total = [], 0
    for g, p in zip(geos, pit):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    dense = [g["out_w"] * g["out_h"] * 3 for g in geos]
    doffs = []
    for d in dense:                                     # the dense images back to back, a guard byte between them: none of them aligned
        doffs.append(total + 1)
        total += d + 1
    total += 16
    base = ctx.malloc(total)
    ctx.memset(base, GUARD, total)
    pipe = J.Pipeline(ctx, max_images=len(files), depth=2)
    st = pipe.wait(pipe.submit(files, [(base + offs[i], pit[i], geos[i]["canvas_w"], geos[i]["canvas_h"]) for i in range(len(files))], [J.RGB8888] * len(files), [0] * len(files)))
    assert list(st) == [0] * len(files), st
    for flags in (CHW, HWC | BGR):
        before = pack_launches()
        # after the wait: the VISIBLE rectangles of the resident canvases, one launch
        J.pack_surfaces(ctx, [(base + offs[i], pit[i], geos[i]["out_w"], geos[i]["out_h"]) for i in range(len(files))], 4, [base + d for d in doffs], flags, U8)
        assert pack_launches() == before + 1
        got = ctx.to_host(base + doffs[0] - 1, total - doffs[0] + 1)
        at = 0
        for i, f in enumerate(files):
            assert got[at] == GUARD, PIPELINE_FILES[i]
            assert np.array_equal(got[at + 1:at + 1 + dense[i]], expected_packed(oracle, f, 0, flags, U8, None)[0]), (PIPELINE_FILES[i], flags)
            at += 1 + dense[i]
        assert np.all(got[at:] == GUARD)
    pipe.close()
    ctx.free(base)


def test_decode_to_tensors(gpu_ctx):
    """decode_to_tensors against the oracle (tests/pack_torch_child.py), in a process of its own: torch has to be imported BEFORE
    libjpegdec_amd.so is loaded where torch brings a HIP runtime of its own (one process, one runtime -- jpegdec_amd/tensors.py), and this
    process loaded the library long ago"""
    import importlib.util
    import os
    import subprocess
    import sys
    if importlib.util.find_spec("torch") is None:
        pytest.skip("no torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "pack_torch_child.py")], cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "pack_torch_child ok" in r.stdout, r.stdout[-4000:]


def test_pack_surfaces_refusals_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    lib = ctx.lib
    a, b, t = ctx.malloc(1 << 16), ctx.malloc(1 << 16), ctx.malloc(3 * 256 * 4)

    def call(src=(a, 64, 10, 20), dst=b + 3, bpp=4, rect=None, flags=HWC, elem=U8, table=None, n=1, arrays=True):
        s = (Output * 1)(Output(*src)) if arrays else None
        d = (C.c_void_p * 1)(dst) if arrays else None
        r = None if rect is None else (C.c_int32 * 4)(*rect)
        return lib.jda_pack_surfaces(ctx.handle, n, s, bpp, r, flags, elem, table, d)
    before = pack_launches()
    assert call() == 0 and pack_launches() == before + 1
    assert call(n=0) == 0 and call(n=0, arrays=False) == 0 and pack_launches() == before + 1            # nothing to do, nothing launched
    for what, rc in (
            ("null src pixels", call(src=(0, 64, 10, 20))), ("null dst", call(dst=0)), ("null arrays", call(arrays=False)), ("n < 0", call(n=-1)),
            ("misaligned src", call(src=(a + 4, 64, 10, 20))), ("misaligned F16 dst", call(elem=F16, table=t, dst=b + 1)),
            ("misaligned F32 dst", call(elem=F32, table=t, dst=b + 2)), ("misaligned table", call(elem=F32, table=t + 4, dst=b)),
            ("pitch too small", call(src=(a, 32, 10, 20))), ("pitch not a multiple of 16", call(src=(a, 72, 10, 20))),
            ("empty surface", call(src=(a, 64, 0, 20))), ("empty rectangle", call(rect=(0, 0, 0, 5))), ("negative origin", call(rect=(-1, 0, 5, 5))),
            ("rectangle leaves on the right", call(rect=(6, 0, 5, 5))), ("rectangle leaves at the bottom", call(rect=(0, 16, 5, 5))),
            ("pixel size 2", call(bpp=2)), ("pixel size 3", call(bpp=3)), ("unknown layout bit", call(flags=4)), ("unknown element type", call(elem=3)),
            ("unknown layout with n == 0", call(flags=4, n=0)), ("pixel size 2 with n == 0", call(bpp=2, n=0)),
            ("table with U8", call(table=t)), ("no table with F16", call(elem=F16, dst=b)), ("no table with F32", call(elem=F32, dst=b)),
            ("BGR on a gray source", call(bpp=1, src=(a, 16, 10, 20), flags=BGR)),
            ("dst is src", call(dst=a)), ("dst begins inside src", call(dst=a + 64 * 19 + 8)), ("src begins inside dst", call(src=(b + 16, 64, 10, 20), dst=b + 3)),
            ("dst overlaps the table", call(elem=F32, table=t, dst=t + 1024)),
            ("destination over JDA_PACK_MAX_BYTES", call(src=(a, 65536 * 4, 65536, 16384))),
    ):
        assert rc == INVALID, what
    assert pack_launches() == before + 1, "a refused call launches nothing"
    assert call(dst=a + 64 * 19 + 40) == 0 and pack_launches() == before + 2                            # side by side is fine
    assert lib.jda_pack_surfaces(None, 1, None, 4, None, HWC, U8, None, None) == 6                      # JDA_ERROR_NO_DEVICE
    for p in (a, b, t):
        ctx.free(p)
