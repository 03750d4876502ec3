"""jda_resize_surfaces without a GPU.  Every comparison is exact equality of bytes.

* the numpy twin (tests/resize_util.py) = Pillow's Image.resize(BILINEAR, box) for L and RGBX over the grid (skipped where Pillow is absent);
* the row-major C twin (tests/hostsim/resize_twin.h) = the numpy twin;
* the host's tap tables (jpegdec_amd/csrc/jda_resize_plan.h) = the twin's integers, entry for entry, for every axis case of the grid and
  the ratios the documents quote -- where a fused multiply-add would show;
* the kernel's two passes, lane by lane through the kernel's own code over the plan's tiles (tests/hostsim/resize_sim.cpp over
  jda_device_core.h), against the twin, for both pixel sizes: guard-filled destinations with extra pitch and extra rows, random source
  padding; the simulator also holds every access to the kernel's promises; the job at the tap cap, whose tiles are one row high;
* every refusal of jda_resize_surfaces through the same plan header, one step beyond the tap cap and beyond the table cap among them;
* the constants and exports, and the argument errors of decode_to_tensors that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import resize_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5
INVALID, UNSUPPORTED = 1, 3
EXTRA_AXES = ((4096, 0, 4096, 224), (500, 0, 500, 224), (375, 0, 375, 224), (333, 0, 333, 7), (217, 0, 217, 5), (640, 0, 640, 224), (33, 0, 33, 224),
              (160, 0, 160, 2), (217, 13, 203, 224), (333, 7, 329, 100))


class Output(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("pitch_bytes", C.c_int32), ("width_px", C.c_int32), ("rows", C.c_int32)]


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_resizesim.so"))
    lib.resizesim_rowmajor.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p] + [C.c_int] * 3
    lib.resizesim_taps.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int]
    lib.resizesim_lanes.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p] + [C.c_int] * 3 + [C.POINTER(C.c_uint32)]
    lib.resizesim_check.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(C.c_int32), C.POINTER(Output), C.c_void_p, C.POINTER(C.c_uint32)]
    return lib


def aligned(nbytes, align=16):
    raw = np.zeros(nbytes + 2 * align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def make_surface(rng, w, h, bpp, extra_pitch=1):
    """[h, pitch] uint8, 16-byte aligned, every byte random -- the padding behind a row's pixels too"""
    pitch = R.pitch_of(w, bpp, extra_pitch)
    s = aligned(h * pitch).reshape(h, pitch)
    s[:] = rng.randint(0, 256, s.shape)
    return s


def pixels_of(surface, w, bpp):
    return surface[:, :w * bpp].reshape(surface.shape[0], w, bpp)


@pytest.fixture(scope="module")
def cases():
    """the grid's images, made once: (w, h, box, ow, oh, bpp, surface, the numpy twin's result)"""
    rng = np.random.RandomState(20261018)
    out = []
    for w, h, box, ow, oh in R.image_cases():
        for bpp in (1, 4):
            s = make_surface(rng, w, h, bpp)
            out.append((w, h, box, ow, oh, bpp, s, R.resize(pixels_of(s, w, bpp), ow, oh, box)))
    return out


def test_twin_equals_pillow(cases):
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: the twin cannot be held to it here")
    extra = [(1024, 700, None, 7, 5), (640, 480, None, 224, 224), (33, 17, None, 224, 224), (4096, 16, None, 64, 16)]
    rng = np.random.RandomState(5)
    todo = [(w, h, box, ow, oh, bpp, pixels_of(s, w, bpp), want) for w, h, box, ow, oh, bpp, s, want in cases]
    for w, h, box, ow, oh in extra:
        for bpp in (1, 4):
            a = rng.randint(0, 256, (h, w, bpp), dtype=np.uint8)
            todo.append((w, h, box, ow, oh, bpp, a, R.resize(a, ow, oh, box)))
    for w, h, box, ow, oh, bpp, a, twin in todo:
        im = Image.frombytes("L" if bpp == 1 else "RGBX", (w, h), np.ascontiguousarray(a).tobytes())
        b = None if box is None else (box[0], box[1], box[0] + box[2], box[1] + box[3])
        pil = np.asarray(im.resize((ow, oh), Image.BILINEAR, box=b)).reshape(oh, ow, bpp)
        assert np.array_equal(twin, pil), (w, h, box, ow, oh, bpp)


def test_c_twin_equals_numpy_twin(sim, cases):
    for w, h, box, ow, oh, bpp, s, want in cases:
        dpitch = R.pitch_of(ow, bpp)
        d = aligned(oh * dpitch).reshape(oh, dpitch)
        assert sim.resizesim_rowmajor(s.ctypes.data, s.shape[1], w, h, bpp, *box, d.ctypes.data, dpitch, ow, oh) == 0
        assert np.array_equal(pixels_of(d, ow, bpp), want), (w, h, box, ow, oh, bpp)


def test_host_taps_equal_the_twin_entry_for_entry(sim):
    for in_size, in0, in1, out_size in tuple(R.axis_cases()) + EXTRA_AXES:
        bounds, k = R.axis_taps(in_size, in0, in1, out_size)
        tab = np.full(out_size * (2 + k.shape[1]) + 8, -7, np.int32)
        ksize = sim.resizesim_taps(in_size, in0, in1, out_size, tab.ctypes.data, tab.size - 8)
        assert ksize == k.shape[1], (in_size, in0, in1, out_size, ksize)
        assert np.array_equal(tab[:2 * out_size].reshape(out_size, 2), bounds), (in_size, in0, in1, out_size)
        assert np.array_equal(tab[2 * out_size:-8].reshape(out_size, ksize), k), (in_size, in0, in1, out_size)
        assert np.all(tab[-8:] == -7)
        # what the kernel's arithmetic leans on: no negative coefficient, 23 bits at most, rising bounds
        assert k.min() >= 0 and k.max() <= 1 << 22
        assert np.all(np.diff(bounds[:, 0]) >= 0) and np.all(np.diff(bounds.sum(axis=1)) >= 0) and np.all(bounds[:, 1] >= 1)
    for in_size, in0, in1, out_size in R.BEYOND_CAP_AXES:
        assert sim.resizesim_taps(in_size, in0, in1, out_size, None, 0) == -UNSUPPORTED


def run_lanes(sim, s, w, h, bpp, box, ow, oh, extra_pitch=2, extra_rows=3):
    dpitch = R.pitch_of(ow, bpp, extra_pitch)
    d = aligned((oh + extra_rows) * dpitch).reshape(oh + extra_rows, dpitch)
    d[:] = GUARD
    info = (C.c_uint32 * 5)()
    rc = sim.resizesim_lanes(s.ctypes.data, s.shape[1], w, h, bpp, *box, d.ctypes.data, dpitch, ow, oh, info)
    return rc, d, list(info)


def test_simulator_equals_the_twin_and_keeps_the_promises(sim, cases):
    for w, h, box, ow, oh, bpp, s, want in cases:
        rc, d, info = run_lanes(sim, s, w, h, bpp, box, ow, oh)
        assert rc == 0, (w, h, box, ow, oh, bpp, rc)
        assert np.array_equal(pixels_of(d[:oh], ow, bpp), want), (w, h, box, ow, oh, bpp)
        assert np.all(d[:oh, ow * bpp:] == GUARD) and np.all(d[oh:] == GUARD), (w, h, box, ow, oh, bpp)
        assert info[2] <= 192 * 256
        if (w, h, box, ow, oh) == R.CAP_CASE:
            assert info[1] == 1 and info[4] == R.MAX_KSIZE and info[0] == 6, info      # one row a tile at the cap


def test_simulator_on_wide_and_tall_tiles(sim):
    """more than one tile across and down, a partial last tile and a partial last vector on both, 2.2 : 1 and 18 : 1 (tiles of fewer rows)"""
    rng = np.random.RandomState(9)
    for w, h, box, ow, oh, bpp in ((500, 375, (0, 0, 500, 375), 224, 224, 4), (1100, 90, (3, 1, 1090, 88), 483, 37, 1), (70, 2310, (0, 0, 70, 2310), 67, 125, 4),
                                   (31, 9, (0, 0, 31, 9), 301, 35, 1)):
        s = make_surface(rng, w, h, bpp)
        rc, d, info = run_lanes(sim, s, w, h, bpp, box, ow, oh)
        assert rc == 0, (w, h, ow, oh, bpp, rc)
        assert np.array_equal(pixels_of(d[:oh], ow, bpp), R.resize(pixels_of(s, w, bpp), ow, oh, box)), (w, h, ow, oh, bpp)
        assert np.all(d[:oh, ow * bpp:] == GUARD) and np.all(d[oh:] == GUARD)
        assert info[0] > 1


def check(sim, src, dst, bpp=4, rects=None, tables_at=None):
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    d = (Output * max(n, 1))(*[Output(*o) for o in dst])
    r = None if rects is None else (C.c_int32 * (4 * n))(*[v for q in rects for v in q])
    info = (C.c_uint32 * 3)()
    return sim.resizesim_check(n, s, bpp, r, d, tables_at, info), list(info)


def test_refusals(sim):
    A, B, T = 0x10000000, 0x20000000, 0x30000000          # (host addresses that are never followed)
    src, dst = (A, 1344, 333, 217), (B, 896, 224, 224)
    assert check(sim, [src], [dst])[0] == 0
    assert check(sim, [src], [dst], tables_at=T)[0] == 0
    assert check(sim, [src, src], [dst, (B + 0x100000, 896, 224, 224)], rects=[(0, 0, 333, 217), (5, 6, 40, 30)])[0] == 0
    bad = [
        ([(0, 1344, 333, 217)], [dst], 4, None),                              # null pointers
        ([src], [(0, 896, 224, 224)], 4, None),
        ([(A + 4, 1344, 333, 217)], [dst], 4, None),                          # misaligned pixels
        ([src], [(B + 8, 896, 224, 224)], 4, None),
        ([(A, 1340, 333, 217)], [dst], 4, None),                              # a pitch that is no multiple of 16
        ([src], [(B, 900, 224, 224)], 4, None),
        ([(A, 1328, 333, 217)], [dst], 4, None),                              # .. or too small
        ([src], [(B, 880, 224, 224)], 4, None),
        ([src], [dst], 4, [(0, 0, 0, 10)]),                                   # an empty rectangle
        ([src], [dst], 4, [(0, 0, 10, 0)]),
        ([src], [dst], 4, [(-1, 0, 10, 10)]),                                 # one that leaves the surface
        ([src], [dst], 4, [(0, -1, 10, 10)]),
        ([src], [dst], 4, [(300, 0, 34, 10)]),
        ([src], [dst], 4, [(0, 200, 10, 18)]),
        ([src], [(B, 896, 0, 224)], 4, None),                                 # an output size that is not positive
        ([src], [(B, 896, 224, -1)], 4, None),
        ([(A, 1344, 0, 217)], [dst], 4, None),
        ([src], [dst], 2, None),                                              # a pixel size other than 1 or 4
        ([src], [dst], 3, None),
        ([src], [(A + 1344 * 100, 896, 224, 224)], 4, None),                  # a destination inside the source
        ([src, src], [dst, (B + 896 * 223, 896, 224, 224)], 4, None),         # two destinations that share their last / first row
    ]
    for s, d, bpp, rects in bad:
        assert check(sim, s, d, bpp, rects)[0] == INVALID, (s, d, bpp, rects)
    assert check(sim, [], [], 4)[0] == INVALID                               # (n == 0 is the entry point's: it succeeds before the plan)
    # a destination over the tables; tables that are not aligned
    assert check(sim, [src], [dst], tables_at=B + 896 * 10)[0] == INVALID
    assert check(sim, [src], [dst], tables_at=T + 4)[0] == INVALID
    # two sources may overlap, and a destination may lie right behind a source's last byte that is read
    assert check(sim, [src, src], [dst, (B + 896 * 224, 896, 224, 224)])[0] == 0
    # the tap cap: 80 : 1 on either axis is taken, one source row or column more is not; every upscale is
    assert check(sim, [(A, 176, 160, 160)], [(B, 16, 2, 2)], 1)[0] == 0
    assert check(sim, [(A, 176, 161, 160)], [(B, 16, 2, 2)], 1)[0] == UNSUPPORTED
    assert check(sim, [(A, 176, 160, 161)], [(B, 16, 2, 2)], 1)[0] == UNSUPPORTED
    for in_size, in0, in1, out_size in R.BEYOND_CAP_AXES:
        pitch = (in_size + 15) & ~15
        assert check(sim, [(A, pitch, in_size, 40)], [(B, 16, out_size, 7)], 1, [(in0, 0, in1 - in0, 40)])[0] == UNSUPPORTED
        assert check(sim, [(A, 48, 40, in_size)], [(B, 16, 7, out_size)], 1, [(0, in0, 40, in1 - in0)])[0] == UNSUPPORTED
    assert check(sim, [(A, 16 * 640, 64 * 40, 64 * 30)], [(B, 160, 40, 30)], 4)[0] == 0         # 64 : 1
    assert check(sim, [(A, 16, 1, 1)], [(B, 1 << 16, 1 << 14, 1 << 10)], 4)[0] == 0
    # the table cap: (2 + 161) * 4 bytes an output column at 80 : 1 -- 102,926 columns fit 64 MiB with the one output row's table, one more does not
    per = (2 + R.MAX_KSIZE) * 4
    fit = (R.MAX_TABLE_BYTES - (2 + 3) * 4) // per
    rc, info = check(sim, [(A, 80 * fit, 80 * fit, 1)], [(B, (fit + 15) & ~15, fit, 1)], 1)
    assert rc == 0 and info[2] == fit * per + 20 <= R.MAX_TABLE_BYTES
    assert check(sim, [(A, 80 * (fit + 1) + 16, 80 * (fit + 1), 1)], [(B, (fit + 16) & ~15, fit + 1, 1)], 1)[0] == UNSUPPORTED
    # .. and jobs with equal axes share their tables: a thousand of them cost what one does
    many_src = [(A + k * 0x100000, 1344, 333, 217) for k in range(1000)]
    many_dst = [(0x60000000 + k * 0x100000, 896, 224, 224) for k in range(1000)]
    rc1, one = check(sim, many_src[:1], many_dst[:1])
    rcn, many = check(sim, many_src, many_dst)
    assert rc1 == 0 and rcn == 0 and many[2] == one[2] and many[0] == 1000 * one[0]


def test_exports_and_constants(product_lib):
    import jpegdec_amd as J
    for name in ("jda_resize_surfaces", "jda_decode_to_host_resized"):
        assert hasattr(product_lib, name), name
    assert J.RESIZE_MAX_KSIZE == R.MAX_KSIZE == 161 and J.RESIZE_MAX_TABLE_BYTES == R.MAX_TABLE_BYTES == 64 << 20
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    assert "#define JDA_RESIZE_MAX_KSIZE 161" in hdr and "#define JDA_RESIZE_MAX_TABLE_BYTES (64u << 20)" in hdr
    assert callable(J.resize_surfaces) and callable(J.decode_resized_to_host)
    # without a context nothing is decoded: the no-device answer, as every entry point gives it
    assert product_lib.jda_resize_surfaces(None, 0, None, 4, None, None) == 6
    assert product_lib.jda_decode_to_host_resized(None, b"x", 1, 0, 0, None, 1, 1, None, 0, 0, None, None) == 6


def test_decode_to_tensors_argument_errors():
    """refused before torch or a GPU is looked at"""
    import jpegdec_amd as J
    f = [b"\xff\xd8"]
    for kw in (dict(crops=[(0, 0, 1, 1)]), dict(prescale=True), dict(size=(0, 4)), dict(size=(4, -1)), dict(size=(4,)), dict(size=(4, 4), crops=[(0, 0, 1, 1)], prescale=True),
               dict(size=(4, 4), crops=[]), dict(size=(4, 4), crops=[(0, 0, 1)]), dict(size=(4, 4), prescale=True, options=J.SCALE_HALF), dict(layout="NCHW")):
        with pytest.raises(ValueError):
            J.decode_to_tensors(None, f, **kw)
