"""jda_resize_surfaces_ex -- Pillow's BOX, BILINEAR, HAMMING, BICUBIC and LANCZOS -- without a GPU.  Every comparison is exact equality.

* the numpy twin (tests/resize_filter_util.py) = Pillow's Image.resize(F, box) for L and RGBX over the grid, the jobs at each filter's tap
  cap, and pictures of 0 and 255 that force both clips in both passes (skipped where Pillow is absent); the twin's sums before the clip
  show that every signed filter did leave 0 .. 255 * 2^22 on both sides in each pass;
* the host's tap tables (jpegdec_amd/csrc/jda_resize_plan.h) = the twin's integers, entry for entry and per filter, no axis trips the
  guard, and BILINEAR's tables through the new entry are the old function's;
* the two passes lane by lane through the kernel's own code -- the signed instances for BICUBIC and LANCZOS -- over the plan's tiles
  (tests/hostsim/resize_filters_sim.cpp) = the twin, with every access held to the promises of DESIGN.md 5.12;
* wide and tall tiles, tiles of fewer than 16 rows, the jobs at the caps; every refusal; the read rectangle that decides which MCUs
  jda_decode_to_host_resized_ex decodes; the Python argument errors; and the same code as a program of its own under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import resize_filter_util as F
from tests import resize_util as R
from tests.test_resize_cpu import GUARD, INVALID, UNSUPPORTED, Output, aligned, make_surface, pixels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA_AXES = ((4096, 0, 4096, 224), (500, 0, 500, 224), (375, 0, 375, 224), (333, 0, 333, 7), (33, 0, 33, 224), (217, 13, 203, 224), (1, 0, 1, 5))
ONE = 1 << 22
# the largest tile rows with which cnt + (th - 1) * scale source rows fit the 192 of the LDS budget, at each filter's cap of 161 taps: the
# output rows lie 160, 80, 80, 40 and 26.7 source rows apart, so only LANCZOS fits two (161 + 27 = 188)
CAP_TH = {F.BOX: 1, F.BILINEAR: 1, F.HAMMING: 1, F.BICUBIC: 1, F.LANCZOS: 2}


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_resizefilterssim.so"))
    lib.resizefsim_taps.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int]
    lib.resizefsim_taps_old.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int]
    lib.resizefsim_guard.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.resizefsim_lanes.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p] + [C.c_int] * 3 + [C.POINTER(C.c_uint32)]
    lib.resizefsim_check.argtypes = [C.c_int, C.c_int, C.POINTER(Output), C.c_int, C.POINTER(C.c_int32), C.POINTER(Output), C.c_void_p, C.POINTER(C.c_uint32)]
    return lib


def surface_of(img):
    """[h, w, bpp] uint8 -> an aligned surface [h, pitch] with the pixels in front of a padding of 0x33"""
    h, w, bpp = img.shape
    s = aligned(h * R.pitch_of(w, bpp, 1)).reshape(h, -1)
    s[:] = 0x33
    s[:, :w * bpp] = img.reshape(h, w * bpp)
    return s


@pytest.fixture(scope="module")
def cases():
    """per filter the grid's images, the job at the filter's cap and the clip-forcing pictures, made once:
    (w, h, box, ow, oh, bpp, surface, the numpy twin's result, the twin's sums before the clip or None)"""
    rng = np.random.RandomState(20261019)
    out = {}
    for f in F.FILTERS:
        todo = []
        for w, h, box, ow, oh in F.image_cases(f) + [F.cap_case(f)]:
            for bpp in (1, 4):
                s = make_surface(rng, w, h, bpp)
                todo.append((w, h, box, ow, oh, bpp, s, F.resize(pixels_of(s, w, bpp), ow, oh, box, f), None))
        for bpp in (1, 4):
            for _, img, ow, oh in F.clip_pictures(bpp):
                h, w = img.shape[:2]
                sums = []
                want = F.resize(img, ow, oh, None, f, sums)
                todo.append((w, h, (0, 0, w, h), ow, oh, bpp, surface_of(img), want, sums))
        out[f] = todo
    return out


def test_twin_equals_pillow_and_both_clips_are_forced(cases):
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: the twin cannot be held to it here")
    pil_filter = {F.BILINEAR: Image.BILINEAR, F.BOX: Image.BOX, F.HAMMING: Image.HAMMING, F.BICUBIC: Image.BICUBIC, F.LANCZOS: Image.LANCZOS}
    for f in F.FILTERS:
        for w, h, box, ow, oh, bpp, s, twin, _ in cases[f]:
            im = Image.frombytes("L" if bpp == 1 else "RGBX", (w, h), np.ascontiguousarray(pixels_of(s, w, bpp)).tobytes())
            pil = np.asarray(im.resize((ow, oh), pil_filter[f], box=(box[0], box[1], box[0] + box[2], box[1] + box[3]))).reshape(oh, ow, bpp)
            assert np.array_equal(twin, pil), (F.NAMES[f], w, h, box, ow, oh, bpp)


def test_signed_filters_leave_the_range_on_both_sides_in_each_pass(cases):
    """without this the arithmetic shift and the two-sided clip of the signed instances would not really be tested: from the twin's sums
    (the rounding term taken off) every signed filter has a sum below 0 and one above 255 * 2^22 in the horizontal and in the vertical pass"""
    for f in F.SIGNED:
        for bpp in (1, 4):
            sums = [c[8] for c in cases[f] if c[8] is not None and c[5] == bpp]
            assert sums
            for p in (0, 1):
                assert min(s[p][0] for s in sums) - (ONE >> 1) < 0, (F.NAMES[f], bpp, p)
                assert max(s[p][1] for s in sums) - (ONE >> 1) > 255 * ONE, (F.NAMES[f], bpp, p)
    for f in (F.BILINEAR, F.BOX, F.HAMMING):                                     # (.. and the others never do below)
        assert all(s[p][0] >= 0 for c in cases[f] if c[8] is not None for s in (c[8],) for p in (0, 1))


def test_hamming_window_constants_are_floats():
    """Pillow writes 0.54f + 0.46f * cos(x): a tap in a few hundred differs by one from what the doubles 0.54 and 0.46 give, and on this
    row -- found by search -- the result does; the twin must side with Pillow"""
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed")
    assert F.HAMMING_A != 0.54 and F.HAMMING_B != 0.46 and abs(F.HAMMING_A - 0.54) < 1e-7
    rng = np.random.RandomState(11)
    for w, ow in ((333, 217), (500, 224), (777, 100)):
        a = rng.randint(0, 256, (64, w, 1), dtype=np.uint8)
        pil = np.asarray(Image.frombytes("L", (w, 64), a.tobytes()).resize((ow, 64), Image.HAMMING)).reshape(64, ow, 1)
        assert np.array_equal(F.resize(a, ow, 64, None, F.HAMMING), pil)


def host_taps(sim, f, axis, slack=8):
    in_size, in0, in1, out_size = axis
    ks = F.ksize_of(f, in0, in1, out_size)
    tab = np.full(out_size * (2 + ks) + slack, -7, np.int32)
    return sim.resizefsim_taps(f, in_size, in0, in1, out_size, tab.ctypes.data, tab.size - slack), tab


@pytest.mark.parametrize("f", F.FILTERS, ids=[F.NAMES[f] for f in F.FILTERS])
def test_host_taps_equal_the_twin_entry_for_entry(sim, f):
    cap_axes = ((480, 0, 480, F.CAP_ROWS[f]), (33, 0, 33, 17))
    for axis in tuple(F.axis_cases(f)) + tuple(a for a in EXTRA_AXES if F.within_cap(f, a)) + cap_axes:
        in_size, in0, in1, out_size = axis
        bounds, k = F.axis_taps(f, *axis)
        ksize, tab = host_taps(sim, f, axis)
        assert ksize == k.shape[1] > 0, (axis, ksize)                            # (a negative answer would be a refusal: no axis trips the guard)
        assert np.array_equal(tab[:2 * out_size].reshape(out_size, 2), bounds), axis
        assert np.array_equal(tab[2 * out_size:-8].reshape(out_size, ksize), k), axis
        assert np.all(tab[-8:] == -7)
        # what the kernels' arithmetic leans on (the host's guard checks the same): the taps' size, the 32-bit sums, rising bounds
        k64 = k.astype(np.int64)
        pos, neg = np.where(k64 > 0, k64, 0).sum(axis=1), np.where(k64 < 0, k64, 0).sum(axis=1)
        assert np.abs(k64).max() < 1 << 23 and 255 * pos.max() + (ONE >> 1) < 1 << 31 and 255 * neg.min() + (ONE >> 1) > -(1 << 31)
        if f not in F.SIGNED:
            assert k.min() >= 0 and k.max() <= ONE
        assert np.all(np.diff(bounds[:, 0]) >= 0) and np.all(np.diff(bounds.sum(axis=1)) >= 0) and np.all(bounds[:, 1] >= 1)
        if in1 - in0 <= out_size:
            assert ksize == F.UPSCALE_TAPS[f]
        if f == F.BILINEAR:                                                      # the new entry makes exactly the tables of the old one
            old = np.full(tab.size, -7, np.int32)
            assert sim.resizefsim_taps_old(in_size, in0, in1, out_size, old.ctypes.data, old.size - 8) == ksize and np.array_equal(old, tab)
            rb, rk = R.axis_taps(*axis)
            assert np.array_equal(rb, bounds) and np.array_equal(rk, k)
    assert ksize_at_cap(f) == F.MAX_KSIZE
    for axis in tuple(F.beyond_cap_axes(f)) + ((F.BEYOND_ROWS[f], 0, F.BEYOND_ROWS[f], F.CAP_ROWS[f]),):
        assert sim.resizefsim_taps(f, *axis, None, 0) == -UNSUPPORTED, axis
    for bad in (-1, 5, 100):
        assert sim.resizefsim_taps(bad, 10, 0, 10, 5, None, 0) == -INVALID


def ksize_at_cap(f):
    return F.ksize_of(f, 0, 480, F.CAP_ROWS[f])


def run_lanes(sim, f, s, w, h, bpp, box, ow, oh, extra_pitch=2, extra_rows=3):
    dpitch = R.pitch_of(ow, bpp, extra_pitch)
    d = aligned((oh + extra_rows) * dpitch).reshape(oh + extra_rows, dpitch)
    d[:] = GUARD
    info = (C.c_uint32 * 6)()
    rc = sim.resizefsim_lanes(f, s.ctypes.data, s.shape[1], w, h, bpp, *box, d.ctypes.data, dpitch, ow, oh, info)
    return rc, d, list(info)


@pytest.mark.parametrize("f", F.FILTERS, ids=[F.NAMES[f] for f in F.FILTERS])
def test_simulator_equals_the_twin_and_keeps_the_promises(sim, cases, f):
    for w, h, box, ow, oh, bpp, s, want, _ in cases[f]:
        rc, d, info = run_lanes(sim, f, s, w, h, bpp, box, ow, oh)
        assert rc == 0, (w, h, box, ow, oh, bpp, rc)
        assert np.array_equal(pixels_of(d[:oh], ow, bpp), want), (w, h, box, ow, oh, bpp)
        assert np.all(d[:oh, ow * bpp:] == GUARD) and np.all(d[oh:] == GUARD), (w, h, box, ow, oh, bpp)
        assert info[2] <= 192 * 256 and info[5] == (1 if f in F.SIGNED else 0)
        if (w, h, box, ow, oh) == F.cap_case(f):                                 # the job at the cap
            assert info[4] == F.MAX_KSIZE and info[1] == CAP_TH[f] and info[0] == F.CAP_ROWS[f] // CAP_TH[f], info


@pytest.mark.parametrize("f", F.SIGNED, ids=[F.NAMES[f] for f in F.SIGNED])
def test_simulator_on_wide_and_tall_tiles(sim, f):
    """one job wider than a 64-dword tile and taller than a 16-row tile, with a partial last tile and a partial last vector on both; and a
    ratio at which a tile has fewer than 16 rows (217 -> 5 rows: th from the plan)"""
    rng = np.random.RandomState(90 + f)
    for w, h, box, ow, oh, bpp in ((500, 375, (0, 0, 500, 375), 224, 224, 4), (1100, 90, (3, 1, 1090, 88), 483, 37, 1), (31, 40, (0, 0, 31, 40), 301, 35, 1)):
        s = make_surface(rng, w, h, bpp)
        rc, d, info = run_lanes(sim, f, s, w, h, bpp, box, ow, oh)
        assert rc == 0, (w, h, ow, oh, bpp, rc)
        assert np.array_equal(pixels_of(d[:oh], ow, bpp), F.resize(pixels_of(s, w, bpp), ow, oh, box, f)), (w, h, ow, oh, bpp)
        assert np.all(d[:oh, ow * bpp:] == GUARD) and np.all(d[oh:] == GUARD)
        assert info[0] >= 2 * 3 and info[1] == 16, info                          # more than one tile across and down, whole tiles of 16 rows
    for bpp in (1, 4):
        s = make_surface(rng, 70, 217, bpp)
        rc, d, info = run_lanes(sim, f, s, 70, 217, bpp, (0, 0, 70, 217), 67, 5)
        # 43.4 : 1 is beyond BICUBIC's 40 : 1 and LANCZOS' 26.6 : 1
        assert rc == UNSUPPORTED
        oh = 9 if f == F.BICUBIC else 12                                         # 24.1 : 1 and 18.1 : 1: 2 x 2 (3) x the ratio + 1 source rows an output row
        rc, d, info = run_lanes(sim, f, s, 70, 217, bpp, (0, 0, 70, 217), 67, oh)
        vb, _ = F.axis_taps(f, 217, 0, 217, oh)
        th = max(t for t in range(1, oh + 1) if all(vb[min(o + t, oh) - 1].sum() - vb[o, 0] <= 192 for o in range(0, oh, t)))
        assert rc == 0 and 1 < info[1] == th < 16, (info, th)
        assert np.array_equal(pixels_of(d[:oh], 67, bpp), F.resize(pixels_of(s, 70, bpp), 67, oh, None, f))


def check(sim, f, src, dst, bpp=4, rects=None, tables_at=None):
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    d = (Output * max(n, 1))(*[Output(*o) for o in dst])
    r = None if rects is None else (C.c_int32 * (4 * n))(*[v for q in rects for v in q])
    info = (C.c_uint32 * 7)()
    return sim.resizefsim_check(f, n, s, bpp, r, d, tables_at, info), list(info)


def test_refusals(sim):
    A, B, T = 0x10000000, 0x20000000, 0x30000000          # (host addresses that are never followed)
    src, dst = (A, 1344, 333, 217), (B, 896, 224, 224)
    for f in (-1, 5, 6, 1 << 20):                                                 # a filter id that is none
        assert check(sim, f, [src], [dst])[0] == INVALID
    bad = [
        ([(0, 1344, 333, 217)], [dst], 4, None), ([src], [(0, 896, 224, 224)], 4, None),                       # null pointers
        ([(A + 4, 1344, 333, 217)], [dst], 4, None), ([src], [(B + 8, 896, 224, 224)], 4, None),               # misaligned pixels
        ([(A, 1340, 333, 217)], [dst], 4, None), ([src], [(B, 900, 224, 224)], 4, None),                       # a pitch that is no multiple of 16
        ([(A, 1328, 333, 217)], [dst], 4, None), ([src], [(B, 880, 224, 224)], 4, None),                       # .. or too small
        ([src], [dst], 4, [(0, 0, 0, 10)]), ([src], [dst], 4, [(0, 0, 10, 0)]),                                # an empty rectangle
        ([src], [dst], 4, [(-1, 0, 10, 10)]), ([src], [dst], 4, [(0, -1, 10, 10)]),                            # one that leaves the surface
        ([src], [dst], 4, [(300, 0, 34, 10)]), ([src], [dst], 4, [(0, 200, 10, 18)]),
        ([src], [(B, 896, 0, 224)], 4, None), ([src], [(B, 896, 224, -1)], 4, None), ([(A, 1344, 0, 217)], [dst], 4, None),      # sizes that are not positive
        ([src], [dst], 2, None), ([src], [dst], 3, None),                                                      # a pixel size other than 1 or 4
        ([src], [(A + 1344 * 100, 896, 224, 224)], 4, None),                                                   # a destination inside the source
        ([src, src], [dst, (B + 896 * 223, 896, 224, 224)], 4, None),                                          # two destinations that share a row
    ]
    for f in F.FILTERS:
        assert check(sim, f, [src], [dst])[0] == 0 and check(sim, f, [src], [dst], tables_at=T)[0] == 0
        for s, d, bpp, rects in bad:
            assert check(sim, f, s, d, bpp, rects)[0] == INVALID, (F.NAMES[f], s, d, bpp, rects)
        assert check(sim, f, [], [], 4)[0] == INVALID
        assert check(sim, f, [src], [dst], tables_at=B + 896 * 10)[0] == INVALID and check(sim, f, [src], [dst], tables_at=T + 4)[0] == INVALID
        # the tap cap of the filter on either axis: taken, and one step beyond it refused; every upscale is taken
        rows, brows, out = 480, F.BEYOND_ROWS[f], F.CAP_ROWS[f]
        assert check(sim, f, [(A, 48, 33, rows)], [(B, 32, 17, out)], 1)[0] == 0
        assert check(sim, f, [(A, 48, 33, brows)], [(B, 32, 17, out)], 1)[0] == UNSUPPORTED
        assert check(sim, f, [(A, 496, rows, 33)], [(B, 32, out, 17)], 1)[0] == 0
        assert check(sim, f, [(A, 496, brows, 33)], [(B, 32, out, 17)], 1)[0] == UNSUPPORTED
        assert check(sim, f, [(A, 16, 1, 1)], [(B, 1 << 16, 1 << 14, 1 << 10)], 4)[0] == 0
        # the table cap: (2 + 161) * 4 bytes an output column at the filter's cap ratio
        ratio = rows // out if rows % out == 0 else None
        if ratio:
            per = (2 + F.MAX_KSIZE) * 4
            fit = (R.MAX_TABLE_BYTES - (2 + F.UPSCALE_TAPS[f]) * 4) // per
            rc, info = check(sim, f, [(A, ratio * fit + 16 - (ratio * fit) % 16, ratio * fit, 1)], [(B, (fit + 15) & ~15, fit, 1)], 1)
            assert rc == 0 and info[2] == fit * per + (2 + F.UPSCALE_TAPS[f]) * 4 <= R.MAX_TABLE_BYTES
            n1 = ratio * (fit + 1)
            assert check(sim, f, [(A, n1 + 16 - n1 % 16, n1, 1)], [(B, (fit + 16) & ~15, fit + 1, 1)], 1)[0] == UNSUPPORTED


def test_guard_on_hand_made_tables(sim):
    """jda_resize_axis_guard through the test hook: tables of one output coordinate and three taps"""
    def guard(f, *k):
        tab = np.array((0, 3) + k, np.int32)
        return sim.resizefsim_guard(f, tab.ctypes.data, 1, 3)
    for f in F.FILTERS:
        assert guard(f, ONE, 0, 0) == 0 and guard(f, ONE // 2, ONE // 4, ONE // 4) == 0
    for f in (F.BOX, F.HAMMING):                                                 # a negative tap in a table for the unsigned instances
        assert guard(f, ONE + 1, -1, 0) == UNSUPPORTED
    for f in F.SIGNED:
        assert guard(f, ONE + 1000, -1000, 0) == 0
        assert guard(f, (1 << 23) - 1, -(1 << 23) + 1, 0) == 0                     # the largest taps: 255 * (2^23 - 1) + 2^21 < 2^31
        assert guard(f, 1 << 23, -ONE, 0) == UNSUPPORTED and guard(f, 0, -(1 << 23), 3 * ONE) == UNSUPPORTED      # a tap of 24 bits
        fits = ((1 << 31) - (ONE >> 1) - 1) // 255                                 # 255 * fits + 2^21 < 2^31 <= 255 * (fits + 1) + 2^21
        assert guard(f, fits // 2, fits - fits // 2, -ONE) == 0 and guard(f, fits // 2, fits - fits // 2 + 1, -ONE) == UNSUPPORTED
        fitn = ((1 << 31) + (ONE >> 1) - 1) // 255                                 # 255 * -fitn + 2^21 > -2^31 >= 255 * -(fitn + 1) + 2^21
        assert guard(f, -(fitn // 2), -(fitn - fitn // 2), ONE) == 0 and guard(f, -(fitn // 2), -(fitn - fitn // 2) - 1, ONE) == UNSUPPORTED


def test_read_rectangle_of_a_crop_per_filter(sim):
    """what jda_decode_to_host_resized_ex turns into its MCU rectangle: for a crop in the middle of a 333 x 217 image the plan's read rectangle
    is the twin's [min(0), min(last) + cnt(last)) on both axes -- wider with the filter's support, and never clipped at the box"""
    A, B = 0x10000000, 0x20000000
    crop = (140, 90, 60, 45)
    seen = {}
    for f in F.FILTERS:
        for ow, oh in ((16, 11), (60, 45), (100, 75)):
            rc, info = check(sim, f, [(A, 1344, 333, 217)], [(B, R.pitch_of(ow, 4), ow, oh)], 4, [crop])
            x0, x1 = F.read_range(f, 333, crop[0], crop[0] + crop[2], ow)
            y0, y1 = F.read_range(f, 217, crop[1], crop[1] + crop[3], oh)
            assert rc == 0 and info[3:7] == [x0, y0, x1, y1], (F.NAMES[f], ow, oh, info)
            assert 0 <= x0 <= crop[0] and crop[0] + crop[2] <= x1 <= 333 and 0 <= y0 <= crop[1] and crop[1] + crop[3] <= y1 <= 217
            seen[f, ow] = (x0, y0, x1, y1)
    # 60 -> 16 is 3.75 : 1, the first centre lies at 141.875 and the last at 198.125: LANCZOS reads 3 x 3.75 on each side of them, the triangle
    # 3.75, BOX 1.875 -- which is the box itself
    assert (seen[F.LANCZOS, 16][0], seen[F.LANCZOS, 16][2]) == (131, 209) and (seen[F.BICUBIC, 16][0], seen[F.BICUBIC, 16][2]) == (134, 206)
    assert (seen[F.BILINEAR, 16][0], seen[F.BILINEAR, 16][2]) == (138, 202) and (seen[F.BOX, 16][0], seen[F.BOX, 16][2]) == (140, 200)


def test_exports_and_constants(product_lib):
    import jpegdec_amd as J
    for name in ("jda_resize_surfaces_ex", "jda_decode_to_host_resized_ex"):
        assert hasattr(product_lib, name), name
    assert (J.RESIZE_BILINEAR, J.RESIZE_BOX, J.RESIZE_HAMMING, J.RESIZE_BICUBIC, J.RESIZE_LANCZOS) == F.FILTERS == (0, 1, 2, 3, 4)
    assert {v: k for k, v in J.RESIZE_FILTERS.items()} == F.NAMES
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    assert "JDA_RESIZE_BILINEAR = 0, JDA_RESIZE_BOX = 1, JDA_RESIZE_HAMMING = 2, JDA_RESIZE_BICUBIC = 3, JDA_RESIZE_LANCZOS = 4" in hdr
    # without a context nothing is decoded: the no-device answer, as every entry point gives it
    assert product_lib.jda_resize_surfaces_ex(None, 0, None, 4, None, None, 3) == 6
    assert product_lib.jda_decode_to_host_resized_ex(None, b"x", 1, 0, 0, None, 1, 1, 4, None, 0, 0, None, None) == 6


def test_python_argument_errors():
    """refused before torch or a GPU is looked at"""
    import jpegdec_amd as J
    f = [b"\xff\xd8"]
    for fid, name in F.NAMES.items():
        assert J.resize_filter(name) == J.resize_filter(name.upper()) == fid and J.resize_filter(fid) == fid
    for bad in ("nearest", "cubic", "", 5, -1, 2.0, None, True):
        with pytest.raises(ValueError):
            J.resize_filter(bad)
        if bad is not None:
            with pytest.raises(ValueError):
                J.decode_to_tensors(None, f, size=(4, 4), resample=bad)
        with pytest.raises(ValueError):
            J.thumbnails(None, f, (4, 4), resample=bad)
    for kw in (dict(resample="bicubic"), dict(resample=0), dict(resample="nearest")):      # resample goes with size=, as crops does
        with pytest.raises(ValueError):
            J.decode_to_tensors(None, f, **kw)


def test_plan_and_lanes_under_sanitizers():
    """tests/hostsim/resize_filters_main.cpp: a program of its own (make resizefiltersasan), nothing preloaded"""
    subprocess.run(["make", "resizefiltersasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "resize_filters_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"resize_filters_asan ok" in r.stdout, r.stdout[-2000:]
