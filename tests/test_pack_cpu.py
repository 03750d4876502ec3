"""jda_pack_surfaces without a GPU.

* the row-major twin (tests/hostsim/pack_twin.h) = the numpy expressions: canvas[y:y+h, x:x+w, :3], [..., ::-1], .transpose(2, 0, 1), table[c][v];
* the kernel's schedule, lane by lane through the kernel's own code (tests/hostsim/pack_sim.cpp over jda_device_core.h), against the twin:
  every size, rectangle origin, destination offset, layout, channel order, element type and source of the grid, alpha bytes that are random,
  guard bytes in front of and behind every destination; the simulator also holds every access to the kernel's promises (aligned loads inside
  the rectangle's rows, stores aligned to their width, narrow stores only at the ends of a run, every byte once, LDS read where written);
* every refusal of jda_pack_surfaces, through the same checks the runtime runs (jpegdec_amd/csrc/jda_pack_plan.h);
* jda_pack_bytes, normalise_table against its formula, the constants and exports."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5
HWC, CHW, BGR = 0, 1, 2
U8, F16, F32 = 0, 1, 2
DTYPES = {U8: np.uint8, F16: np.float16, F32: np.float32}
INVALID = 1
WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 63, 64, 65, 333)
HEIGHTS = (1, 2, 9, 217)
ORIGINS = tuple((x, y) for x in (0, 1, 3, 7) for y in (0, 5))
U8_OFFSETS = (0, 1, 2, 3, 5, 15)
# (source bytes per pixel, layout flags): both layouts, BGR, the gray source
FORMATS = ((4, HWC), (4, CHW), (4, HWC | BGR), (4, CHW | BGR), (1, HWC), (1, CHW))


class Output(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("pitch_bytes", C.c_int32), ("width_px", C.c_int32), ("rows", C.c_int32)]


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_packsim.so"))
    lib.packsim_rowmajor.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p, C.c_void_p]
    lib.packsim_lanes.argtypes = [C.c_void_p] + [C.c_int] * 10 + [C.c_void_p, C.c_void_p]
    lib.packsim_check.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    return lib


def aligned(nbytes, align=16, offset=0):
    """nbytes of uint8 whose first byte lies `offset` bytes behind an address that is a multiple of `align`"""
    raw = np.zeros(nbytes + 2 * align + offset, np.uint8)
    off = (-raw.ctypes.data) % align + offset
    return raw[off:off + nbytes]


def make_table(rng, channels, elem):
    """random BIT PATTERNS of the element type (NaNs among them: a lookup moves bits), 16-byte aligned"""
    if elem == U8:
        return None
    es = np.dtype(DTYPES[elem]).itemsize
    t = aligned(channels * 256 * es)
    t[:] = rng.randint(0, 256, t.size)
    return t


def numpy_pack(surface, bpp, rect, flags, elem, table):
    """surface: [rows, pitch] uint8 -> the dense result as bytes, by the issue's numpy expressions"""
    x, y, w, h = rect
    if bpp == 4:
        img = surface[:, : (surface.shape[1] // 4) * 4].reshape(surface.shape[0], -1, 4)[y:y + h, x:x + w, :3]
        if flags & BGR:
            img = img[..., ::-1]
    else:
        img = surface[y:y + h, x:x + w, None]
    if elem != U8:
        es = np.dtype(DTYPES[elem]).itemsize
        tab = table.reshape(img.shape[2], 256, es)                    # (as raw bytes: bit-exact whatever the pattern means)
        img = np.stack([tab[c][img[..., c]] for c in range(img.shape[2])], axis=2)      # [h, w, C, es]
        if flags & CHW:
            img = img.transpose(2, 0, 1, 3)
    elif flags & CHW:
        img = img.transpose(2, 0, 1)
    return np.ascontiguousarray(img).reshape(-1)


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def surface_for(rng, bpp, x, y, w, h, extra_px=2, extra_rows=1, extra_pitch=0):
    width, rows = x + w + extra_px, y + h + extra_rows
    pitch = ((width * bpp + 15) & ~15) + extra_pitch
    s = aligned(pitch * rows)
    s[:] = rng.randint(0, 256, s.size)                                 # (alpha bytes and padding are random, not 0xFF)
    return s.reshape(rows, pitch), width, rows, pitch


def dest_for(nbytes, offset):
    """a dense destination `offset` bytes behind a 16-byte boundary with 32 guard bytes on either side"""
    buf = aligned(nbytes + 64, 16, (offset - 32) % 16)
    buf[:] = GUARD
    return buf, buf[32:32 + nbytes]


@pytest.mark.parametrize("elem", [U8, F16, F32])
@pytest.mark.parametrize("bpp,flags", FORMATS)
def test_row_major_twin_equals_numpy(bpp, flags, elem, sim):
    rng = np.random.RandomState(1000 + 10 * flags + bpp + 100 * elem)
    channels = 3 if bpp == 4 else 1
    table = make_table(rng, channels, elem)
    es = np.dtype(DTYPES[elem]).itemsize
    for w, h, x, y in ((1, 1, 0, 0), (2, 3, 1, 0), (17, 5, 3, 5), (64, 9, 7, 5), (333, 2, 0, 5), (65, 17, 1, 1)):
        surf, width, rows, pitch = surface_for(rng, bpp, x, y, w, h, extra_pitch=16)
        buf, dst = dest_for(w * h * channels * es, 0)
        assert sim.packsim_rowmajor(p(surf), pitch, bpp, x, y, w, h, flags, elem, p(table), p(dst)) == 0
        assert np.array_equal(dst, numpy_pack(surf, bpp, (x, y, w, h), flags, elem, table)), (w, h, x, y)
        assert np.all(buf[:32] == GUARD) and np.all(buf[32 + dst.size:] == GUARD)


@pytest.mark.parametrize("elem", [U8, F16, F32])
@pytest.mark.parametrize("bpp,flags", FORMATS)
def test_lane_schedule_equals_row_major_twin(bpp, flags, elem, sim):
    rng = np.random.RandomState(7 + 10 * flags + bpp + 100 * elem)
    channels = 3 if bpp == 4 else 1
    es = np.dtype(DTYPES[elem]).itemsize
    table = make_table(rng, channels, elem)
    offsets = U8_OFFSETS if elem == U8 else tuple(es * k for k in (0, 1, 2, 3, 5, 15) if es * k < 16) + (16 - es,)
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            # every origin and every offset is met at every width and height in turn (the full product is 8 x 6 times the work and
            # exercises no other code: the origin only moves the loads, the offset only the stores)
            for (x, y), off in ((ORIGINS[(k + i) % len(ORIGINS)], offsets[(k + i) % len(offsets)]) for i in range(max(len(ORIGINS), len(offsets)))):
                surf, width, rows, pitch = surface_for(rng, bpp, x, y, w, h, extra_px=(k % 3), extra_rows=(k % 2), extra_pitch=16 * (k % 2))
                nbytes = w * h * channels * es
                buf, dst = dest_for(nbytes, off)
                assert dst.ctypes.data % 16 == off
                rc = sim.packsim_lanes(p(surf), pitch, width, rows, bpp, x, y, w, h, flags, elem, p(table), p(dst))
                assert rc == 0, "the schedule broke a promise (%d) at %dx%d+%d+%d, destination offset %d" % (rc, w, h, x, y, off)
                twin = np.empty(nbytes, np.uint8)
                assert sim.packsim_rowmajor(p(surf), pitch, bpp, x, y, w, h, flags, elem, p(table), p(twin)) == 0
                assert np.array_equal(dst, twin), "differs from the row-major twin at %dx%d+%d+%d, destination offset %d" % (w, h, x, y, off)
                assert np.all(buf[:32] == GUARD) and np.all(buf[32 + nbytes:] == GUARD), "guard bytes at %dx%d offset %d" % (w, h, off)
            k += 1


@pytest.mark.parametrize("bpp,flags", FORMATS)
def test_lane_schedule_every_origin_and_offset(bpp, flags, sim):
    """the full product of rectangle origins and destination offsets, U8, at the widths around a vector and one that spans tiles"""
    rng = np.random.RandomState(99 + flags + bpp)
    channels = 3 if bpp == 4 else 1
    for w, h in ((1, 1), (5, 2), (16, 9), (17, 2), (333, 9), (65, 217)):
        for x, y in ORIGINS:
            surf, width, rows, pitch = surface_for(rng, bpp, x, y, w, h)
            twin = np.empty(w * h * channels, np.uint8)
            assert sim.packsim_rowmajor(p(surf), pitch, bpp, x, y, w, h, flags, U8, None, p(twin)) == 0
            for off in U8_OFFSETS:
                buf, dst = dest_for(twin.size, off)
                rc = sim.packsim_lanes(p(surf), pitch, width, rows, bpp, x, y, w, h, flags, U8, None, p(dst))
                assert rc == 0, (rc, w, h, x, y, off)
                assert np.array_equal(dst, twin) and np.all(buf[:32] == GUARD) and np.all(buf[32 + twin.size:] == GUARD), (w, h, x, y, off)


def test_whole_surface_rectangle_and_tile_counts(sim):
    """rects == NULL is all of width_px x rows; the launch has ceil((run + 15) / 4096) tiles a job, one job after the other"""
    a = aligned(1 << 16)
    d = aligned(1 << 18)
    src = (Output * 2)(Output(a.ctypes.data, 64, 10, 20), Output(a.ctypes.data + 4096, 1024, 256, 30))
    dst = (C.c_void_p * 2)(d.ctypes.data + 1, d.ctypes.data + 1 + 600)
    tiles = C.c_uint32(0)
    assert sim.packsim_check(2, src, 4, None, HWC, U8, None, dst, C.byref(tiles)) == 0
    assert tiles.value == 1 + (256 * 30 * 3 + 15 + 4095) // 4096
    assert sim.packsim_check(2, src, 4, None, CHW, U8, None, dst, C.byref(tiles)) == 0
    assert tiles.value == 1 + (256 * 30 + 15 + 4095) // 4096


def test_every_refusal(sim):
    a, b, t = aligned(1 << 16), aligned(1 << 16), aligned(3 * 256 * 4)
    A, Bp, T = a.ctypes.data, b.ctypes.data, t.ctypes.data

    def call(src=(A, 64, 10, 20), dst=Bp + 3, bpp=4, rect=None, flags=HWC, elem=U8, table=None, n=1, arrays=True):
        s = (Output * 1)(Output(*src)) if arrays else None
        d = (C.c_void_p * 1)(dst) if arrays else None
        r = None if rect is None else (C.c_int32 * 4)(*rect)
        return sim.packsim_check(n, s, bpp, r, flags, elem, table, d, None)
    assert call() == 0 and call(rect=(1, 2, 9, 18)) == 0 and call(elem=F32, table=T, dst=Bp + 4) == 0 and call(elem=F16, table=T, dst=Bp + 2, flags=CHW | BGR) == 0
    assert call(bpp=1, src=(A, 16, 10, 20)) == 0 and call(bpp=1, src=(A, 16, 10, 20), flags=CHW) == 0
    for what, rc in (
            ("null src pixels", call(src=(0, 64, 10, 20))), ("null dst", call(dst=0)), ("null arrays", call(arrays=False)), ("n < 0", call(n=-1)),
            ("misaligned src", call(src=(A + 4, 64, 10, 20))), ("misaligned F16 dst", call(elem=F16, table=T, dst=Bp + 1)),
            ("misaligned F32 dst", call(elem=F32, table=T, dst=Bp + 2)), ("misaligned table", call(elem=F32, table=T + 4, dst=Bp)),
            ("pitch too small", call(src=(A, 32, 10, 20))), ("pitch not a multiple of 16", call(src=(A, 72, 10, 20))),
            ("gray pitch too small", call(bpp=1, src=(A, 16, 20, 20))),
            ("empty surface", call(src=(A, 64, 0, 20))), ("empty rectangle", call(rect=(0, 0, 0, 5))), ("empty rectangle (rows)", call(rect=(0, 0, 5, 0))),
            ("negative origin", call(rect=(-1, 0, 5, 5))), ("rectangle leaves on the right", call(rect=(6, 0, 5, 5))),
            ("rectangle leaves at the bottom", call(rect=(0, 16, 5, 5))), ("negative size", call(rect=(0, 0, -3, 5))),
            ("pixel size 2", call(bpp=2)), ("pixel size 3", call(bpp=3)), ("pixel size 0", call(bpp=0)),
            ("unknown layout bit", call(flags=4)), ("unknown layout bits", call(flags=CHW | 8)), ("negative layout", call(flags=-1)),
            ("unknown element type", call(elem=3)), ("negative element type", call(elem=-1)),
            ("table with U8", call(table=T)), ("no table with F16", call(elem=F16, dst=Bp)), ("no table with F32", call(elem=F32, dst=Bp)),
            ("BGR on a gray source", call(bpp=1, src=(A, 16, 10, 20), flags=BGR)), ("BGR | CHW on a gray source", call(bpp=1, src=(A, 16, 10, 20), flags=BGR | CHW)),
            ("dst is src", call(dst=A)), ("dst begins inside src", call(dst=A + 64 * 19 + 8)), ("src begins inside dst", call(src=(Bp + 16, 64, 10, 20), dst=Bp + 3)),
            ("dst overlaps the table", call(elem=F32, table=T, dst=T + 1024)), ("dst ends inside src", call(dst=A - 100)),
    ):
        assert rc == INVALID, what
    assert call(dst=A + 64 * 19 + 40) == 0                       # right behind the last pixel that is read: side by side is fine
    # two destinations that overlap each other, and a destination over the OTHER job's source
    src = (Output * 2)(Output(A, 64, 10, 20), Output(A + 4096, 64, 10, 20))
    for dsts, want in (((Bp, Bp + 600), 0), ((Bp, Bp + 599), INVALID), ((Bp + 7, Bp + 7), INVALID), ((Bp, A + 4096 + 64), INVALID), ((Bp + 1000, Bp + 1), 0)):
        assert sim.packsim_check(2, src, 4, None, HWC, U8, None, (C.c_void_p * 2)(*dsts), None) == want, dsts
    # a dense destination larger than JDA_PACK_MAX_BYTES (0x7fff0000): the pointers are never followed
    big = (Output * 1)(Output(A, 65536 * 4, 65536, 16384))
    far = (C.c_void_p * 1)(1 << 44)
    assert sim.packsim_check(1, big, 4, None, HWC, U8, None, far, None) == INVALID            # 3 GiB
    assert sim.packsim_check(1, big, 4, (C.c_int32 * 4)(0, 0, 65536, 10922), HWC, U8, None, far, None) == 0          # just under the limit
    assert sim.packsim_check(1, big, 4, (C.c_int32 * 4)(0, 0, 65536, 10923), HWC, U8, None, far, None) == INVALID
    assert sim.packsim_check(1, big, 4, (C.c_int32 * 4)(0, 0, 65536, 8192), CHW, F16, T, far, None) == INVALID       # 3 x 2^29 x 2 bytes


def test_entry_points_without_a_device(product_lib):
    """jda_pack_bytes; and the GPU entry points fail loudly without a context"""
    lib = product_lib
    assert lib.jda_pack_bytes(333, 217, 3, U8) == 333 * 217 * 3 and lib.jda_pack_bytes(333, 217, 3, F16) == 333 * 217 * 6
    assert lib.jda_pack_bytes(5, 7, 1, F32) == 140 and lib.jda_pack_bytes(65536, 65536, 3, F32) == 3 * 4 * (1 << 32)
    assert lib.jda_pack_bytes(0, 7, 1, U8) == 0 and lib.jda_pack_bytes(5, -1, 1, U8) == 0 and lib.jda_pack_bytes(5, 7, 0, U8) == 0 and lib.jda_pack_bytes(5, 7, 3, 3) == 0
    assert lib.jda_pack_surfaces(None, 0, None, 4, None, HWC, U8, None, None) == 6                      # JDA_ERROR_NO_DEVICE
    assert lib.jda_decode_to_host_packed(None, b"x", 1, 0, HWC, U8, None, None, 0, None, None, None) == 6


def test_normalise_table_against_its_formula():
    import jpegdec_amd as J
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for dt in (np.float32, np.float16):
        t = J.normalise_table(mean, std, dt)
        assert t.shape == (3, 256) and t.dtype == dt and t.flags["C_CONTIGUOUS"]
        for c in range(3):
            want = ((np.arange(256, dtype=np.float64) / 255.0 - mean[c]) / std[c]).astype(dt)
            assert np.array_equal(t[c].view(np.uint16 if dt == np.float16 else np.uint32), want.view(np.uint16 if dt == np.float16 else np.uint32)), (dt, c)
    g = J.normalise_table([0.5], [0.25])
    assert g.shape == (1, 256) and g.dtype == np.float32 and g[0, 0] == -2.0 and g[0, 255] == 2.0
    assert np.array_equal(J.normalise_table(0.0, 1.0, "float32")[0], (np.arange(256) / 255.0).astype(np.float32))
    with pytest.raises(ValueError):
        J.normalise_table((0.5, 0.5), (1.0,))
    with pytest.raises(ValueError):
        J.normalise_table((0.5,), (1.0,), np.int32)


def test_constants_and_exports():
    import jpegdec_amd as J
    assert (J.PACK_HWC, J.PACK_CHW, J.PACK_BGR) == (HWC, CHW, BGR) and (J.PACK_U8, J.PACK_F16, J.PACK_F32) == (U8, F16, F32)
    for name in ("pack_surfaces", "decode_packed_to_host", "decode_to_tensors", "normalise_table"):
        assert callable(getattr(J, name))
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    assert "JDA_PACK_HWC = 0, JDA_PACK_CHW = 1, JDA_PACK_BGR = 2" in hdr and "JDA_PACK_U8 = 0, JDA_PACK_F16 = 1, JDA_PACK_F32 = 2" in hdr
    assert "#define JDA_PACK_MAX_BYTES 0x7fff0000u" in hdr
