"""Pillow's Image.thumbnail() without a GPU: reduce, float-box resize, the plan and the whole chain.  Every comparison is exact equality.

* the numpy reduce (tests/thumbnail_util.py) = Image.reduce((fx, fy), box) for "L" and "RGB" over the grid, and the grid holds cells where
  the plain rounded mean differs: the multiplier is part of the definition;
* the reduce kernel's two phases, lane by lane through the kernel's own code over the plan's tiles (tests/hostsim/reduce_sim.cpp over
  jda_device_core.h) = the twin, both pixel sizes, guard-filled destinations; the simulator also holds every access to the kernel's promises;
* the host's tap tables of fractional boxes = the twin's, entry for entry; the twin = Image.resize(size, F, box = a float box); a box kept in
  double differs somewhere (the float32 rule is forced); whole boxes through the new entry give the old entry's tables;
* the plan (jda_thumbnail_plan) = the Python restatement = Pillow: im.size after thumbnail(), after the draft() it performs, the factors;
* the chain over Pillow-written files, the decode taken from the exact road's twins = Image.thumbnail, all five filters;
* every refusal; the exports; the sanitizer program."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import jpegdec_amd as J
from tests import exact_scaled_util as S
from tests import exact_util as X
from tests import resize_filter_util as F
from tests import thumbnail_util as T
from tests.test_resize_cpu import GUARD, INVALID, UNSUPPORTED, Output, aligned, make_surface, pixels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = tuple((fx, fy) for fx in range(1, 9) for fy in range(1, 9)) + ((16, 16), (32, 32), (1, 32), (32, 1), (5, 11))


class Steps(C.Structure):
    _fields_ = J.binding.ThumbnailSteps._fields_


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "tests/hostsim/libjda_reducesim.so"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_reducesim.so"))
    lib.reducesim_geometry.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int32)] * 2
    lib.reducesim_lanes.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_int32), C.c_void_p] + [C.c_int] * 3 + [C.POINTER(C.c_uint32)]
    lib.reducesim_check.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(Output), C.POINTER(C.c_uint32)]
    lib.reducesim_taps_box.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_int]
    lib.reducesim_resize_plan.argtypes = [C.POINTER(Output), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(Output), C.c_int, C.c_void_p, C.c_int,
                                          C.POINTER(C.c_int32)]
    lib.reducesim_resize_check_box.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(C.c_float), C.POINTER(Output), C.c_int]
    lib.reducesim_thumbnail_plan.argtypes = [C.c_int] * 5 + [C.c_double, C.POINTER(Steps)]
    return lib


def reduce_cases():
    """(w, h, box or None, fx, fy): per factor pair sizes one below, at and one above a multiple of the factors, a box with an origin and
    partial cells, and the fixed cases: widths and heights of 1, a 1 x 1 output, destination widths that end 0, 1, 2, 3 pixels (0 .. 15 gray
    bytes) into a 16-byte group -- row_end_classes counts them --, widths that cross a tile edge (64 RGB8888 pixels, 256 gray ones)"""
    out = []
    for i, (fx, fy) in enumerate(FACTORS):
        mx, my = max(1, min(70 // fx, 3 + i % 4)), max(1, min(70 // fy, 2 + i % 3))
        for dx, dy in ((-1, 1), (0, 0), (1, -1)):
            w, h = max(1, fx * mx + dx), max(1, fy * my + dy)
            out.append((w, h, None, fx, fy))
        w, h = min(70, fx * mx + 5), min(70, fy * my + 4)
        out.append((w, h, (2 + i % 3, 1 + i % 2, w - (i % 2), h - 1), fx, fy))
    out += [(1, 1, None, 1, 1), (1, 1, None, 8, 3), (1, 37, None, 2, 5), (41, 1, None, 3, 2), (7, 5, None, 8, 8), (70, 70, (69, 69, 70, 70), 4, 4)]
    out += [(n, 3, None, 1, 1) for n in (17, 18, 19, 20, 33, 47)]
    # a row's last vector: every count of gray bytes 0 .. 15 (so every mix of dword and byte stores behind it) as a copy, through whole
    # cells of a factor and through a partial last cell
    out += [(n, 3, None, 1, 1) for n in range(25, 33)] + [(2 * n, 4, None, 2, 2) for n in range(25, 33)]
    out += [(3 * n + 1, 5, (1, 1, 3 * n, 5), 3, 2) for n in range(16, 32)]           # (out_w = n: 3 n - 1 columns, the last cell two wide)
    out += [(2 * n + 1, 5, (1, 0, 2 * n + 1, 5), 2, 2) for n in (5, 6, 7, 21)]
    out += [(130, 20, None, 2, 3), (131, 18, (1, 1, 131, 18), 2, 1), (520, 6, (3, 0, 519, 6), 2, 2), (257, 4, None, 1, 1), (70, 70, None, 1, 1)]      # past a tile edge
    return out


def row_end_classes():
    """the destination widths of reduce_cases() modulo 16 (bytes of a gray row behind its last whole vector) and modulo 4 (RGB8888 pixels)"""
    ows = [T.reduced_size(*((b[2] - b[0], b[3] - b[1]) if b else (w, h)), fx, fy)[0] for w, h, b, fx, fy in reduce_cases()]
    return {ow % 16 for ow in ows}, {ow % 4 for ow in ows}


def content(rng, kind, w, h, c):
    if kind == "random":
        return rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    if kind == "white":
        return np.full((h, w, c), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.repeat(((((xx + yy) & 1) * 255).astype(np.uint8))[:, :, None], c, axis=2))


def test_reduce_twin_is_pillows_reduce():
    from PIL import Image
    rng = np.random.RandomState(20261021)
    cells = differ = 0
    for k, (w, h, box, fx, fy) in enumerate(reduce_cases()):
        for mode, c in (("L", 1), ("RGB", 3)):
            for kind in ("random", "white", "checker")[:3 if k % 4 == 0 else 1]:
                a = content(rng, kind, w, h, c)
                im = Image.fromarray(a[:, :, 0] if c == 1 else a, mode)
                want = np.asarray(im.reduce((fx, fy), box=box)).reshape(-1, *T.reduced_size(*((box[2] - box[0], box[3] - box[1]) if box else (w, h)), fx, fy)[:1], c)
                got = T.reduce(a, fx, fy, box)
                assert got.shape == want.shape and np.array_equal(got, want), (w, h, box, fx, fy, mode, kind)
                if kind == "white":
                    assert np.all(got == 255)
                cells += got.size
                differ += int(np.count_nonzero(got != T.rounded_mean(a, fx, fy, box)))
    assert cells > 20000 and differ > 200, (cells, differ)                           # the rounded mean is another function


def run_lanes(sim, s, w, h, bpp, fx, fy, box, extra_pitch=1, extra_rows=2):
    bw, bh = (box[2] - box[0], box[3] - box[1]) if box else (w, h)
    ow, oh = T.reduced_size(bw, bh, fx, fy)
    dpitch = (ow * bpp + 15 & ~15) + 16 * extra_pitch
    d = aligned((oh + extra_rows) * dpitch).reshape(oh + extra_rows, dpitch)
    d[:] = GUARD
    info = (C.c_uint32 * 5)()
    b = None if box is None else (C.c_int32 * 4)(*box)
    rc = sim.reducesim_lanes(s.ctypes.data, s.shape[1], w, h, bpp, fx, fy, b, d.ctypes.data, dpitch, ow, oh, info)
    return rc, d, ow, oh, list(info)


def test_lanes_are_the_twin(sim):
    rng = np.random.RandomState(7)
    tiles_x = set()
    for k, (w, h, box, fx, fy) in enumerate(reduce_cases()):
        for bpp in (1, 4):
            s = make_surface(rng, w, h, bpp)
            if k % 5 == 0:
                s[:, :w * bpp] = content(rng, "white" if k % 10 == 0 else "checker", w, h, bpp).reshape(h, -1)
            rc, d, ow, oh, info = run_lanes(sim, s, w, h, bpp, fx, fy, box)
            assert rc == 0, (w, h, box, fx, fy, bpp, rc)
            want = T.reduce(pixels_of(s, w, bpp), fx, fy, box)
            assert np.array_equal(pixels_of(d[:oh], ow, bpp), want), (w, h, box, fx, fy, bpp)
            assert np.all(d[:oh, ow * bpp:] == GUARD) and np.all(d[oh:] == GUARD)
            if bpp == 4 and k % 10 == 0:
                assert np.all(want[..., 3] == 255)                                   # A = 0xFF in, A = 0xFF out
            bw, bh = (box[2] - box[0], box[3] - box[1]) if box else (w, h)
            assert info[4] <= (-(-(bw * bpp + 3) // 4) + 1) * bh                      # every source dword at most once
            tiles_x.add(-(-ow * bpp // 256))
    assert tiles_x >= {1, 2} and max(tiles_x) >= 3                                    # one tile across, two, more
    assert row_end_classes() == (set(range(16)), set(range(4)))                      # every end of a row's last vector, both pixel sizes
    # the tile rows the LDS budget allows: 16 up to fx = 3, one at the cap
    for fx, th in ((1, 16), (2, 16), (3, 16), (4, 15), (8, 7), (16, 3), (32, 1)):
        s = make_surface(rng, 40 * fx, 40, 1)
        rc, d, ow, oh, info = run_lanes(sim, s, 40 * fx, 40, 1, fx, 1, None)
        assert rc == 0 and info[1] == th and info[2] <= 32768, (fx, info)


BOXES = ((0, 0, 333 / 2, 217 / 4), (0, 0, 333 / 8, 217 / 8), (0.25, 1.75, 61.3, 40.1), (3, 2, 50, 40), (7.1, 0.9, 20.7, 13.2), (0, 0, 70, 45), (10.3, 20.6, 10.9, 44.4))
SIZES_OUT = ((40, 26), (7, 5), (83, 67), (1, 1), (70, 45))


def box_jobs():
    """(w, h, box, ow, oh) on a 70 x 45 or a 167 x 109 source"""
    out = []
    for i, b in enumerate(BOXES):
        w, h = (167, 109) if b[2] > 70 or b[3] > 45 else (70, 45)
        for ow, oh in SIZES_OUT[i % 2::2] + SIZES_OUT[:1]:
            out.append((w, h, b, ow, oh))
    rng = np.random.RandomState(3)
    for _ in range(60):
        x0, y0 = rng.uniform(0, 60), rng.uniform(0, 38)
        out.append((70, 45, (x0, y0, rng.uniform(x0 + 0.7, 70), rng.uniform(y0 + 0.7, 45)), int(rng.randint(1, 50)), int(rng.randint(1, 40))))
    return out


def host_taps(sim, f, in_size, in0, in1, out_size):
    tab = np.full(out_size * (2 + F.MAX_KSIZE) + 8, -7, np.int32)
    ks = sim.reducesim_taps_box(f, in_size, in0, in1, out_size, tab.ctypes.data, tab.size - 8)
    if ks < 0:
        return ks, None, None
    assert np.all(tab[out_size * (2 + ks):] == -7)
    return ks, tab[:2 * out_size].reshape(out_size, 2), tab[2 * out_size:out_size * (2 + ks)].reshape(out_size, ks)


@pytest.mark.parametrize("f", F.FILTERS, ids=[F.NAMES[f] for f in F.FILTERS])
def test_float_box_taps_are_the_twins(sim, f):
    n = 0
    for w, h, b, ow, oh in box_jobs():
        for in_size, in0, in1, out in ((w, b[0], b[2], ow), (h, b[1], b[3], oh)):
            if F.ksize_of(f, T.f32(in0), T.f32(in0) + T.f32(T.f32(in1) - T.f32(in0)), out) > F.MAX_KSIZE:
                assert host_taps(sim, f, in_size, in0, in1, out)[0] == -UNSUPPORTED
                continue
            bounds, k = T.box_axis(f, in_size, in0, in1, out)
            ks, hb, hk = host_taps(sim, f, in_size, in0, in1, out)
            assert ks == k.shape[1] and np.array_equal(hb, bounds) and np.array_equal(hk, k), (f, in_size, in0, in1, out)
            n += 1
    assert n > 100


def test_resize_box_twin_is_pillows_resize_and_float32_is_forced():
    from PIL import Image
    pf = {F.BILINEAR: Image.BILINEAR, F.BOX: Image.BOX, F.HAMMING: Image.HAMMING, F.BICUBIC: Image.BICUBIC, F.LANCZOS: Image.LANCZOS}
    rng = np.random.RandomState(11)
    src = {(70, 45): rng.randint(0, 256, (45, 70, 3)).astype(np.uint8), (167, 109): rng.randint(0, 256, (109, 167, 3)).astype(np.uint8)}
    double_differs = n = 0
    for i, (w, h, b, ow, oh) in enumerate(box_jobs()):
        for f in F.FILTERS:
            a = src[(w, h)] if (i + f) % 2 else np.ascontiguousarray(src[(w, h)][:, :, 0])
            want = np.asarray(Image.fromarray(a).resize((ow, oh), pf[f], box=b))
            assert np.array_equal(T.resize_box(a, ow, oh, b, f), want), (w, h, b, ow, oh, f)
            double_differs += not np.array_equal(T.resize_box(a, ow, oh, b, f, double_box=True), want)
            n += 1
    assert n >= 400 and double_differs >= 1, (n, double_differs)


def test_whole_boxes_through_the_new_entry_give_the_old_tables(sim):
    for f in F.FILTERS:
        for w, h, rect, ow, oh in ((70, 45, (0, 0, 70, 45), 33, 21), (70, 45, (9, 6, 50, 31), 83, 67), (333, 217, (0, 0, 333, 217), 64, 48), (31, 9, (3, 1, 20, 7), 5, 2)):
            S_, D_ = Output(0x10000000, (w + 15) & ~15, w, h), Output(0x20000000, (ow + 15) & ~15, ow, oh)
            cap = (ow + oh) * (2 + F.MAX_KSIZE)
            old, new = np.full(cap, -7, np.int32), np.full(cap, -7, np.int32)
            io, inw = (C.c_int32 * 7)(), (C.c_int32 * 7)()
            fb = (C.c_float * 4)(rect[0], rect[1], rect[0] + rect[2], rect[1] + rect[3])
            assert sim.reducesim_resize_plan(C.byref(S_), 1, (C.c_int32 * 4)(*rect), None, C.byref(D_), f, old.ctypes.data, cap, io) == 0
            assert sim.reducesim_resize_plan(C.byref(S_), 1, None, fb, C.byref(D_), f, new.ctypes.data, cap, inw) == 0
            assert list(io) == list(inw) and io[0] > 0 and np.array_equal(old, new), (f, w, h, rect)


PLAN_SOURCES = tuple((w, h) for w in range(1, 41) for h in range(1, 41)) + ((333, 217), (4096, 4096), (16384, 512), (17, 1700))
PLAN_REQUESTS = ((1, 1), (3, 5), (8, 8), (10, 7), (13, 40), (40, 40), (64, 64), (128, 128), (100, 1000), (5000, 3))
GAPS = (None, 1.0, 2.0, 3.0)


def c_plan(sim, w, h, req, f, gap):
    t = Steps()
    rc = sim.reducesim_thumbnail_plan(w, h, req[0], req[1], f, gap or 0.0, C.byref(t))
    return rc, dict(out=(t.out_w, t.out_h), scale=t.scale, draft=(t.draft_w, t.draft_h), factors=(t.fx, t.fy), reduce_box=tuple(t.reduce_box),
                    reduced=(t.reduced_w, t.reduced_h), resize=bool(t.resize), box=tuple(t.box))


def test_plan_is_the_restatement(sim):
    """the C plan = tests/thumbnail_util.plan, field for field, over every source x request x gap x filter; its refusals are the > 100 : 1
    case, a factor beyond the cap and a resize beyond the tap cap, and nothing else"""
    seen = dict(noop=0, tie=0, floor1=0, reduce=0, tall=0, cap=0, fractional=0)
    for w, h in PLAN_SOURCES:
        for req in PLAN_REQUESTS:
            for gap in GAPS:
                for f in (F.BICUBIC, F.BOX) if (w + h) % 7 else F.FILTERS:
                    p = T.plan(w, h, req, f, gap)
                    rc, c = c_plan(sim, w, h, req, f, gap)
                    for key in ("out", "scale", "draft", "factors", "reduce_box", "reduced", "resize"):
                        assert c[key] == p[key], (w, h, req, gap, f, key, c, p)
                    assert c["box"] == tuple(T.f32(v) for v in p["box"]), (w, h, req, gap, f)
                    over = max(p["factors"]) > T.MAX_FACTOR
                    ks = p["resize"] and not over and not p["tall"] and max(F.ksize_of(f, c["box"][0], c["box"][0] + T.f32(c["box"][2] - c["box"][0]), p["out"][0]),
                                                                              F.ksize_of(f, c["box"][1], c["box"][1] + T.f32(c["box"][3] - c["box"][1]), p["out"][1])) > F.MAX_KSIZE
                    assert rc == (UNSUPPORTED if p["tall"] or over or ks else 0), (w, h, req, gap, f, rc, p)
                    seen["noop"] += p["out"] == (w, h) and not p["resize"] and req[0] >= w and req[1] >= h
                    seen["tie"] += p["tie"]
                    seen["floor1"] += 1 in p["out"] and p["resize"]
                    seen["reduce"] += p["factors"] != (1, 1)
                    seen["tall"] += p["tall"]
                    seen["cap"] += over
                    seen["fractional"] += any(v != int(v) for v in p["box"])
    assert all(seen[k] > 0 for k in ("noop", "tie", "floor1", "reduce", "tall", "cap", "fractional")), seen
    # a tie of the aspect rule goes to the floor: 3 x 2 asked into (2, 2) is 1.5 wide per 1 high -- |1.5 - 2 / 1| == |1.5 - 1 / 1|
    assert T.plan(6, 4, (5, 1), F.BICUBIC)["out"] == (1, 1) and c_plan(sim, 6, 4, (5, 1), F.BICUBIC, 2.0)[1]["out"] == (1, 1)
    assert T.plan(10, 4, (9, 3), F.BICUBIC)["out"] == (7, 3) and c_plan(sim, 10, 4, (9, 3), F.BICUBIC, 2.0)[1]["out"] == (7, 3)
    # the argument errors
    t = Steps()
    for args in ((0, 5, 3, 3, 0, 2.0), (5, -1, 3, 3, 0, 2.0), (5, 5, 0, 3, 0, 2.0), (5, 5, 3, 0, 0, 2.0), (5, 5, 3, 3, 5, 2.0), (5, 5, 3, 3, -1, 2.0), (5, 5, 3, 3, 0, 0.5),
                 (5, 5, 3, 3, 0, -2.0), (5, 5, 3, 3, 0, float("nan"))):
        assert sim.reducesim_thumbnail_plan(*args, C.byref(t)) == INVALID, args
    assert sim.reducesim_thumbnail_plan(1600, 1700, 20, 20, 3, 2.0, None) == INVALID
    assert c_plan(sim, 16, 1700, (5, 50), F.BILINEAR, None)[0] == UNSUPPORTED and c_plan(sim, 17, 1700, (5, 50), F.BILINEAR, None)[0] == 0


def test_plan_is_pillow():
    """im.size after thumbnail(), the scale of the draft() it performs (so im.size after it), and the factors and the box its resize()
    hands to Image.reduce, from Pillow itself on black files of every source size"""
    from PIL import Image
    pf = {F.BILINEAR: Image.BILINEAR, F.BOX: Image.BOX, F.HAMMING: Image.HAMMING, F.BICUBIC: Image.BICUBIC, F.LANCZOS: Image.LANCZOS}
    checked = reduces = ties = 0
    for w, h in PLAN_SOURCES:
        small = w <= 40 and h <= 40
        b = io.BytesIO()
        Image.new("L", (w, h)).save(b, "JPEG")
        for req in PLAN_REQUESTS[(w + h) % 2::2] if small else PLAN_REQUESTS:
            for gap in GAPS if not small else GAPS[(w * h) % 2::2]:
                # (a large source without a gap is resized at full size, and the plan has no step a filter could change: one filter, BOX)
                for f in ((F.BICUBIC, F.BOX, F.LANCZOS, F.BILINEAR, F.HAMMING)[(w + 2 * h) % 5],) if small else (F.BICUBIC, F.BOX, F.LANCZOS) if gap is not None else (F.BOX,):
                    p = T.plan(w, h, req, f, gap)
                    if p["tall"]:                                                     # (the other order of passes)
                        continue
                    im = Image.open(io.BytesIO(b.getvalue()))
                    seen = {}

                    def spy(factor, box=None, _im=im):
                        seen.update(factors=tuple(factor), reduce_box=tuple(box), draft=_im.size)
                        return Image.Image.reduce(_im, factor, box)

                    im.reduce = spy                                                   # (Image.resize calls self.reduce)
                    im.thumbnail(req, pf[f], reducing_gap=gap)
                    assert im.size == p["out"], (w, h, req, gap, f, im.size, p)
                    scale = im.decoderconfig[0] if im.decoderconfig else 1
                    assert scale == p["scale"] and (-(-w // scale), -(-h // scale)) == p["draft"], (w, h, req, gap, f, scale, p)
                    assert seen.get("factors", (1, 1)) == p["factors"], (w, h, req, gap, f, seen, p)
                    if seen:
                        assert seen["reduce_box"] == p["reduce_box"] and seen["draft"] == p["draft"], (w, h, req, gap, f, seen, p)
                        reduces += 1
                    checked += 1
                    ties += p["tie"]
    assert checked > 3000 and reduces > 200 and ties > 20, (checked, reduces, ties)


CHAIN_FILES = (("4:4:4", 333, 217, "baseline"), ("4:2:2", 257, 640, "baseline"), ("4:2:0", 1030, 64, "baseline"), ("gray", 333, 217, "baseline"), ("4:2:0", 257, 640, "progressive"))
CHAIN_REQUESTS = (((300, 300), 2.0), ((100, 100), 2.0), ((40, 40), 2.0), ((20, 20), 2.0), ((10, 10), 2.0), ((100, 100), 1.0), ((50, 50), 1.0), ((25, 25), 1.0),
                  ((10, 10), 3.0), ((64, 64), None), ((33, 200), 2.0), ((2000, 2000), 2.0), ((130, 16), 2.0), ((100, 4), 2.0), ((60, 3), 2.0))


def chain_file(sampling, w, h, kind):
    return S.pillow_file(w, h, sampling, 95, kind)


def chain_decode(f, gray):
    def decode(s):
        t = S.twin_scaled(f, s)
        assert X.in_window(t), t["range"]
        return t["gray"] if gray else t["rgb"]
    return decode


@pytest.mark.parametrize("sampling,w,h,kind", CHAIN_FILES, ids=["%s_%dx%d_%s" % c for c in CHAIN_FILES])
def test_chain_is_pillows_thumbnail(sampling, w, h, kind):
    from PIL import Image
    pf = {F.BILINEAR: Image.BILINEAR, F.BOX: Image.BOX, F.HAMMING: Image.HAMMING, F.BICUBIC: Image.BICUBIC, F.LANCZOS: Image.LANCZOS}
    f = chain_file(sampling, w, h, kind)
    seen = set()
    for req, gap in CHAIN_REQUESTS:
        for flt in F.FILTERS:
            got, p = T.thumbnail(chain_decode(f, sampling == "gray"), w, h, req, flt, gap)
            im = Image.open(io.BytesIO(f))
            im.thumbnail(req, pf[flt], reducing_gap=gap)
            assert im.size == p["out"] and np.array_equal(got, np.asarray(im)), (sampling, w, h, req, gap, flt, p)
            seen.add((p["scale"], p["factors"] != (1, 1), p["resize"]))
    assert {s for s, r, z in seen} == {1, 2, 4, 8} and {r for s, r, z in seen} == {False, True} and (1, False, False) in seen, seen


def test_refusals(sim):
    S_, D_ = Output(0x10000000, 64, 50, 40), Output(0x20000000, 32, 25, 20)
    f22, whole = (C.c_int32 * 2)(2, 2), None

    def check(src=S_, bpp=1, factors=f22, boxes=whole, dst=D_, n=1):
        return sim.reducesim_check(n, C.byref(src), bpp, factors, boxes, C.byref(dst), None)

    assert check() == 0
    assert check(n=0) == INVALID and check(bpp=2) == INVALID and check(bpp=3) == INVALID and check(factors=None) == INVALID
    for fx, fy, rc in ((0, 2, INVALID), (2, -1, INVALID), (33, 2, UNSUPPORTED), (2, 33, UNSUPPORTED)):
        assert check(factors=(C.c_int32 * 2)(fx, fy)) == rc, (fx, fy)
    assert check(factors=(C.c_int32 * 2)(32, 32), dst=Output(0x20000000, 16, 2, 2)) == 0
    for dw, dh in ((24, 20), (26, 20), (25, 19), (25, 21)):                          # a destination that is not the reduced size
        assert check(dst=Output(0x20000000, 32, dw, dh)) == INVALID
    for box in ((0, 0, 51, 40), (0, 0, 50, 41), (-1, 0, 49, 40), (10, 10, 10, 20), (10, 10, 20, 5)):
        assert check(boxes=(C.c_int32 * 4)(*box)) == INVALID, box
    assert check(boxes=(C.c_int32 * 4)(1, 0, 50, 39), dst=Output(0x20000000, 32, 25, 20)) == 0
    assert check(src=Output(0x10000008, 64, 50, 40)) == INVALID and check(src=Output(0x10000000, 56, 50, 40)) == INVALID       # alignment, pitch
    assert check(src=Output(0x10000000, 48, 50, 40)) == INVALID and check(dst=Output(0x20000000, 16, 25, 20)) == INVALID       # a pitch below the row
    assert check(dst=Output(0x10000000 + 64 * 39, 32, 25, 20)) == INVALID                                                      # a destination inside the source
    assert check(src=Output(None, 64, 50, 40)) == INVALID and check(src=Output(0x10000000, 64, 0, 40)) == INVALID
    ow, oh = C.c_int32(7), C.c_int32(7)
    assert sim.reducesim_geometry(50, 40, 3, 7, C.byref(ow), C.byref(oh)) == 0 and (ow.value, oh.value) == (17, 6)
    assert sim.reducesim_geometry(0, 40, 3, 7, C.byref(ow), C.byref(oh)) == INVALID and (ow.value, oh.value) == (0, 0)
    assert sim.reducesim_geometry(50, 40, 33, 7, C.byref(ow), C.byref(oh)) == UNSUPPORTED
    # jda_resize_surfaces_box: Pillow's conditions on the box
    def box_check(box, filt=0, src=S_, dst=D_):
        return sim.reducesim_resize_check_box(1, C.byref(src), 1, None if box is None else (C.c_float * 4)(*box), C.byref(dst), filt)
    assert box_check((0, 0, 49.5, 39.75)) == 0 and box_check((0, 0, 50, 40)) == 0 and box_check((0.5, 0.5, 0.6, 0.6)) == 0
    for box in ((0, 0, 50.5, 40), (0, 0, 50, 40.01), (-0.1, 0, 50, 40), (0, -1e-6, 50, 40), (10, 0, 10, 40), (20, 0, 10, 40), (0, 30, 50, 30), (float("nan"), 0, 50, 40),
                (0, 0, float("nan"), 40), None):
        assert box_check(box) == INVALID, box
    assert box_check((0, 0, 50, 40), filt=5) == INVALID and box_check((0, 0, 50, 40), filt=F.LANCZOS, dst=Output(0x20000000, 16, 1, 1)) == UNSUPPORTED
    # the Python calls refuse before the GPU is touched
    with pytest.raises(ValueError):
        J.thumbnails(None, [b""], (8, 8), pillow=True, crops=[(0, 0, 4, 4)])
    with pytest.raises(ValueError):
        J.thumbnails(None, [b""], (8, 8), pillow=True, prescale=True)
    for gap in (0.5, -1, "2", True, float("nan")):
        with pytest.raises(ValueError):
            J.thumbnails(None, [b""], (8, 8), pillow=True, reducing_gap=gap)
    for gap in (None, 0, 0.0, 1, 2.5):                                               # (0 is None everywhere: thumbnail_plan, the one call, thumbnails)
        assert J.thumbnails(None, [], (8, 8), pillow=True, reducing_gap=gap) == []
    with pytest.raises(ValueError, match=r"\(W, H\)"):
        J.thumbnails(None, [b""], (8, 0), pillow=True)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        J.thumbnails(None, [b""], (8, 0))
    with pytest.raises(J.JdaError):
        J.thumbnail_plan(16, 1700, (5, 50), J.binding.RESIZE_BILINEAR, None)
    with pytest.raises(J.JdaError):
        J.reduce_geometry(10, 10, 33, 1)


def test_exports_and_the_plan_through_the_library(sim):
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    for fn in ("jda_reduce_surfaces", "jda_reduce_geometry", "jda_resize_surfaces_box", "jda_thumbnail_plan", "jda_decode_to_host_thumbnail"):
        assert "int %s(" % fn in hdr and hasattr(J.load_library(), fn), fn
    assert "#define JDA_REDUCE_MAX_FACTOR 32" in hdr and J.REDUCE_MAX_FACTOR == T.MAX_FACTOR == 32
    assert C.sizeof(J.binding.ThumbnailSteps) == 14 * 4 + 4 * 4
    assert J.reduce_geometry(333, 217, 2, 4) == (167, 55)
    for w, h, req, f, gap in ((333, 217, (40, 40), F.BICUBIC, 2.0), (4096, 4096, (224, 224), F.LANCZOS, 2.0), (1280, 720, (128, 128), F.BILINEAR, 3.0), (30, 20, (64, 64), F.BOX, None)):
        p = T.plan(w, h, req, f, gap)
        p["box"] = tuple(T.f32(v) for v in p["box"])
        del p["tall"], p["tie"]
        assert J.thumbnail_plan(w, h, req, f, gap) == p == c_plan(sim, w, h, req, f, gap)[1]
    # host calls that need no context refuse without one
    lib = J.load_library()
    assert lib.jda_reduce_surfaces(None, 1, None, 4, None, None, None) == 6 and lib.jda_resize_surfaces_box(None, 1, None, 4, None, None, 0) == 6      # JDA_ERROR_NO_DEVICE
    assert lib.jda_decode_to_host_thumbnail(None, b"", 0, 8, 8, 0, 2.0, J.RGB8888, None, 0, 0, None, None, None) == 6


def test_table_order_helper_makes_the_twins_file_pillows():
    """thumbnails(pillow=True) hands out Pillow's file from the first byte: jda_encode_surfaces' contract is the bytes behind the SOS header
    (tests/test_encode_cpu.py), and the four table segments of a standard-table colour file stand in another order than libjpeg's"""
    from PIL import Image
    from jpegdec_amd.tensors import _libjpeg_table_order as order
    from tests import encode_util as E
    rng = np.random.RandomState(4)
    moved = 0
    for sampling, ri in (("4:2:0", 0), ("4:2:2", 0), ("4:4:4", 0), ("gray", 0), ("4:2:0", 3)):
        px = rng.randint(0, 256, (37, 53) if sampling == "gray" else (37, 53, 3)).astype(np.uint8)
        b = io.BytesIO()
        kw = {} if sampling == "gray" else dict(subsampling=E.PILLOW_SUBSAMPLING[sampling])
        if ri:
            kw["restart_marker_blocks"] = ri
        Image.fromarray(px).save(b, "JPEG", quality=77, **kw)
        twin = E.file_bytes(px if sampling == "gray" else np.concatenate([px, np.full(px.shape[:2] + (1,), 255, np.uint8)], -1), sampling, 77, ri)
        assert order(twin) == b.getvalue() and order(b.getvalue()) == b.getvalue(), (sampling, ri)
        moved += order(twin) != twin
        for kw2 in (dict(optimize=True), dict(progressive=True)):                   # (their tables already stand in libjpeg's order)
            b2 = io.BytesIO()
            Image.fromarray(px).save(b2, "JPEG", quality=77, **kw, **kw2)
            assert order(b2.getvalue()) == b2.getvalue()
    assert moved == 4
    for junk in (b"", b"\xff\xd8", b"\xff\xd8\xff\xc4", b"\xff\xd8\xff\xc4\x00\x03\x00" + b"\x00" * 9, bytes(range(256))):
        assert order(junk) == junk or len(order(junk)) == len(junk)


def test_sanitizer_program():
    """tests/hostsim/thumb_main.cpp: a program of its own (make thumbasan), nothing preloaded"""
    subprocess.run(["make", "thumbasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "thumb_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"thumb_asan ok" in r.stdout, r.stdout[-2000:]
