"""jda_unpack_surfaces without a GPU.

* the row-major twin (tests/hostsim/unpack_twin.h) = the numpy twin (tests/unpack_util.py);
* uint8: numpy_unpack(numpy_pack(s)) gives s with A = 0xFF and numpy_pack(numpy_unpack(t)) gives t (numpy_pack of tests/test_pack_cpu.py);
* the kernel's schedule, lane by lane through the kernel's own code (tests/hostsim/unpack_sim.cpp over jda_device_core.h), against the twin:
  every width, height and source offset of the grid, pitches with and without 16 spare bytes, every layout, channel order and element
  type, every parameter set, 0xA5 guards in the row padding and around surfaces and sources; the simulator also holds every access to the
  kernel's promises (aligned dword loads that hold a byte of the image, stores aligned to their width, narrow stores only in the last
  vector of a row, every byte of every row once, nothing else);
* the float images hold NaNs of both kinds, +-inf, +-0, subnormals of both types, every k + 0.5, values above 3e38 and -- float32 -- values at
  which a fused multiply-add gives another byte than the product and the sum rounded one after the other: the twin counts them, at least 16
  under each parameter set with a bias (with bias 0 the two are the same number; of the 65,536 float16 values an exhaustive search finds none
  under these parameter sets, so that set is float32's);
* every refusal of jda_unpack_surfaces, through the same checks the runtime runs (jpegdec_amd/csrc/jda_unpack_plan.h);
* denormalise_params against its formula, the sanitizer program, the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import unpack_util as U
from tests.test_pack_cpu import aligned, numpy_pack
from tests.unpack_util import BGR, CHW, DTYPES, F16, F32, FORMATS, GUARD, HWC, U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


class Output(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("pitch_bytes", C.c_int32), ("width_px", C.c_int32), ("rows", C.c_int32)]


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_unpacksim.so"))
    lanes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.unpacksim_rowmajor.argtypes = lanes
    lib.unpacksim_lanes.argtypes = lanes
    lib.unpacksim_check.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.POINTER(Output), C.c_int, C.POINTER(C.c_uint32)]
    return lib


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def params_ptr(scale_bias):
    return None if scale_bias is None else np.ascontiguousarray(scale_bias, np.float32).reshape(-1)


def guarded(nbytes, offset):
    """nbytes `offset` bytes behind a 16-byte boundary with at least 32 guard bytes on either side -> (whole buffer, the bytes)"""
    lead = 32 + offset
    buf = aligned(lead + nbytes + 48)
    buf[:] = GUARD
    return buf, buf[lead:lead + nbytes]


def surface(h, pitch):
    buf, s = guarded(h * pitch, 0)
    return buf, s.reshape(h, pitch)


def check_surface(buf, surf, want, what):
    h, rb = want.shape
    assert np.array_equal(surf[:, :rb], want), "differs from the twin: %s" % (what,)
    assert np.all(surf[:, rb:] == GUARD), "row padding written: %s" % (what,)
    assert np.all(buf[:32] == GUARD) and np.all(buf[32 + surf.size:] == GUARD), "guard bytes around the surface: %s" % (what,)


@pytest.mark.parametrize("elem", [U8, F16, F32])
@pytest.mark.parametrize("bpp,flags", FORMATS)
def test_row_major_twin_equals_numpy(bpp, flags, elem, sim):
    rng = np.random.RandomState(2000 + 10 * flags + bpp + 100 * elem)
    channels = 3 if bpp == 4 else 1
    for name, sb in U.param_sets(channels).items():
        if elem == U8 and name != "default":
            continue
        for k, (w, h) in enumerate(((1, 1), (2, 3), (17, 5), (64, 9), (333, 2), (65, 17))):
            src = U.dense_bytes(U.random_image(rng, w, h, channels, elem, sb, k), flags)
            pitch = ((w * bpp + 15) & ~15) + 16
            buf, surf = surface(h, pitch)
            sbp = params_ptr(sb)
            assert sim.unpacksim_rowmajor(p(src), w, h, flags, elem, p(sbp), p(surf), pitch, bpp) == 0
            check_surface(buf, surf, U.numpy_unpack(src, w, h, bpp, flags, elem, sb), (name, w, h))


@pytest.mark.parametrize("bpp,flags", FORMATS)
def test_u8_round_trips_with_numpy_pack(bpp, flags):
    rng = np.random.RandomState(31 + flags + bpp)
    channels = 3 if bpp == 4 else 1
    for w, h in ((1, 1), (5, 2), (17, 9), (333, 3)):
        pitch = (w * bpp + 15) & ~15
        s = rng.randint(0, 256, (h, pitch)).astype(np.uint8)
        dense = numpy_pack(s, bpp, (0, 0, w, h), flags, U8, None)
        back = U.numpy_unpack(dense, w, h, bpp, flags, U8)
        want = s[:, :w * bpp].copy()
        if bpp == 4:
            want[:, 3::4] = 0xFF
        assert np.array_equal(back, want), (w, h)
        t = rng.randint(0, 256, w * h * channels).astype(np.uint8)
        surf = np.full((h, pitch), GUARD, np.uint8)
        surf[:, :w * bpp] = U.numpy_unpack(t, w, h, bpp, flags, U8)
        assert np.array_equal(numpy_pack(surf, bpp, (0, 0, w, h), flags, U8, None), t), (w, h)


@pytest.mark.parametrize("elem", [U8, F16, F32])
@pytest.mark.parametrize("bpp,flags", FORMATS)
def test_lane_schedule_equals_the_twin(bpp, flags, elem, sim):
    channels = 3 if bpp == 4 else 1
    for name, sb in U.param_sets(channels).items():
        if elem == U8 and name != "default":
            continue
        rng = np.random.RandomState(7 + 10 * flags + bpp + 100 * elem + len(name))
        jobs = U.grid_jobs(rng, bpp, flags, elem, sb)
        assert len(jobs) == len(U.WIDTHS) * len(U.HEIGHTS) * len(U.OFFSETS)
        differs = 0
        for j in jobs:
            w, h, pitch = j["w"], j["h"], j["pitch"]
            sbuf, src = guarded(j["src"].size, j["offset"])
            src[:] = j["src"]
            assert src.ctypes.data % 16 == j["offset"] % 16
            buf, surf = surface(h, pitch)
            sbp = params_ptr(sb)
            rc = sim.unpacksim_lanes(p(src), w, h, flags, elem, p(sbp), p(surf), pitch, bpp)
            what = (name, w, h, j["offset"], pitch)
            assert rc == 0, "the schedule broke a promise (%d): %s" % (rc, what)
            check_surface(buf, surf, j["want"], what)
            assert np.array_equal(src, j["src"]) and np.all(sbuf[:32 + j["offset"]] == GUARD) and np.all(sbuf[32 + j["offset"] + src.size:] == GUARD), what
            differs += j["fused_differs"]
        if elem == F32 and name in ("imagenet", "negative"):
            assert differs >= 16, "%s: only %d elements tell a fused multiply-add from two roundings" % (name, differs)


def test_float_images_hold_the_special_values():
    """the pool of every channel: NaNs of both kinds, infinities, zeros, subnormals, the ties, values above 3e38 and the contraction set"""
    for name, sb in U.param_sets(3).items():
        s, b = U._sb(sb, 3)
        for c in range(3):
            f32 = U.float_pool(F32, s[c], b[c]).view(np.float32)
            bits = f32.view(np.uint32)
            assert 0x7fc00000 in bits and 0x7f800001 in bits and 0xffa00000 in bits                      # quiet and signalling
            assert np.any(np.isposinf(f32)) and np.any(np.isneginf(f32)) and 0 in bits and 0x80000000 in bits
            assert np.any((np.abs(f32) > 0) & (np.abs(f32) < np.finfo(np.float32).tiny))                 # float32 subnormals
            assert np.any(f32 > 3e38) and np.any(f32 < -3e38)
            assert all(np.float32(k + 0.5) in f32 for k in range(-1, 256))
            f16 = U.float_pool(F16, s[c], b[c]).view(np.float16)
            h = f16.view(np.uint16)
            assert 0x7e00 in h and 0x7c01 in h and 0x7c00 in h and 0xfc00 in h and 0 in h and 0x8000 in h and 0x0001 in h and 0x03ff in h
            assert all(np.float16(k + 0.5) in f16 for k in range(-1, 256))
            if name in ("imagenet", "negative"):
                assert len(U.contraction_values(s[c], b[c], F32)) >= 16
    # subnormals under a large scale become bytes: they are kept, not flushed
    tiny = np.array([2.0 ** -127], np.float32)                                                         # (a float32 subnormal: the least normal is 2^-126)
    assert list(U.numpy_unpack(np.array([2.0 ** -24], np.float16).view(np.uint8), 1, 1, 1, CHW, F16, [[2.0 ** 30], [0.0]])[0]) == [64]
    assert list(U.numpy_unpack(tiny.view(np.uint8), 1, 1, 1, CHW, F32, [[2.0 ** 127], [0.0]])[0]) == [1]


def test_tile_counts(sim):
    """ceil(ceil(w * bpp / 16) * h / 256) tiles a job, one job after the other"""
    a, d = aligned(1 << 16), aligned(1 << 20)
    src = (C.c_void_p * 2)(a.ctypes.data + 1, a.ctypes.data + 1 + 600)
    dst = (Output * 2)(Output(d.ctypes.data, 64, 10, 20), Output(d.ctypes.data + 4096, 1024, 256, 30))
    tiles = C.c_uint32(0)
    assert sim.unpacksim_check(2, src, HWC, U8, None, dst, 4, C.byref(tiles)) == 0
    assert tiles.value == 1 + (64 * 30 + 255) // 256
    assert sim.unpacksim_check(2, src, CHW, U8, None, dst, 1, C.byref(tiles)) == 0
    assert tiles.value == 1 + (16 * 30 + 255) // 256


def test_every_refusal(sim):
    a, b = aligned(1 << 16), aligned(1 << 16)
    A, Bp = a.ctypes.data, b.ctypes.data
    good = np.array([255, 255, 255, 0, 0, 0], np.float32)

    def call(src=A + 3, dst=(Bp, 64, 10, 20), bpp=4, flags=HWC, elem=U8, sb=None, n=1, arrays=True):
        s = (C.c_void_p * 1)(src) if arrays else None
        d = (Output * 1)(Output(*dst)) if arrays else None
        return sim.unpacksim_check(n, s, flags, elem, p(sb), d, bpp, None)

    def bad(i, v, size=6):
        q = good[:size].copy()
        q[i] = v
        return q
    assert call() == 0 and call(elem=F32, src=A + 4, sb=good) == 0 and call(elem=F16, src=A + 2, flags=CHW | BGR) == 0 and call(elem=F32, src=A) == 0
    assert call(bpp=1, dst=(Bp, 16, 10, 20)) == 0 and call(bpp=1, dst=(Bp, 16, 10, 20), flags=CHW, elem=F16, src=A + 6, sb=good[:2]) == 0
    for what, rc in (
            ("null dst pixels", call(dst=(0, 64, 10, 20))), ("null src", call(src=0)), ("null arrays", call(arrays=False)), ("n < 0", call(n=-1)),
            ("pixel size 2", call(bpp=2)), ("pixel size 3", call(bpp=3)), ("pixel size 0", call(bpp=0)),
            ("unknown layout bit", call(flags=4)), ("unknown layout bits", call(flags=CHW | 8)), ("negative layout", call(flags=-1)),
            ("unknown element type", call(elem=3)), ("negative element type", call(elem=-1)),
            ("BGR with one channel", call(bpp=1, dst=(Bp, 16, 10, 20), flags=BGR)), ("BGR | CHW with one channel", call(bpp=1, dst=(Bp, 16, 10, 20), flags=BGR | CHW)),
            ("scale_bias with U8", call(sb=good)),
            ("infinite scale", call(elem=F32, src=A, sb=bad(1, np.inf))), ("NaN scale", call(elem=F32, src=A, sb=bad(0, np.nan))),
            ("infinite bias", call(elem=F16, src=A, sb=bad(5, -np.inf))), ("NaN bias", call(elem=F32, src=A, sb=bad(3, np.nan))),
            ("NaN gray bias", call(bpp=1, dst=(Bp, 16, 10, 20), elem=F32, src=A, sb=bad(1, np.nan, 2))),
            ("misaligned F16 src", call(elem=F16, src=A + 1)), ("misaligned F32 src", call(elem=F32, src=A + 2)),
            ("misaligned dst", call(dst=(Bp + 4, 64, 10, 20))), ("pitch too small", call(dst=(Bp, 32, 10, 20))),
            ("pitch not a multiple of 16", call(dst=(Bp, 72, 10, 20))), ("gray pitch too small", call(bpp=1, dst=(Bp, 16, 20, 20))),
            ("w == 0", call(dst=(Bp, 64, 0, 20))), ("h == 0", call(dst=(Bp, 64, 10, 0))), ("w < 0", call(dst=(Bp, 64, -1, 20))), ("h < 0", call(dst=(Bp, 64, 10, -5))),
            ("dst is src", call(src=Bp)), ("src begins inside dst's rows", call(src=Bp + 64 * 19 + 8)), ("dst begins inside src", call(src=Bp - 100)),
            ("src in the first row", call(src=Bp + 39)),
    ):
        assert rc == INVALID, what
    # side by side is fine: right behind the last row's last pixel, and inside the padding of a row, which is never written
    assert call(src=Bp + 64 * 19 + 40) == 0
    assert call(src=Bp + 44, dst=(Bp, 4096, 10, 20), flags=CHW, bpp=1) == 0 and call(src=Bp + 40, dst=(Bp, 64, 10, 1)) == 0
    # two destinations: one behind the other, overlapping, the same, side by side in one canvas (rows interleaved), and over the OTHER job's source
    srcs = (C.c_void_p * 2)(A, A + 4096)
    for dsts, want in ((((Bp, 64, 10, 20), (Bp + 64 * 20, 64, 10, 20)), 0), (((Bp, 64, 10, 20), (Bp + 64 * 19, 64, 10, 20)), INVALID),
                       (((Bp, 64, 10, 20), (Bp, 64, 10, 20)), INVALID), (((Bp, 128, 10, 20), (Bp + 48, 128, 10, 20)), 0),
                       (((Bp, 128, 10, 20), (Bp + 32, 128, 10, 20)), INVALID), (((Bp, 64, 10, 20), (A + 4096 + 64, 64, 10, 20)), INVALID),
                       (((Bp + 8192, 64, 10, 20), (Bp, 64, 10, 20)), 0)):
        d = (Output * 2)(*[Output(*q) for q in dsts])
        assert sim.unpacksim_check(2, srcs, HWC, U8, None, d, 4, None) == want, dsts
    # a dense source larger than JDA_PACK_MAX_BYTES (0x7fff0000): the pointers are never followed
    far = (C.c_void_p * 1)(1 << 44)

    def big(w, h, bpp=4, flags=HWC, elem=U8):
        return sim.unpacksim_check(1, far, flags, elem, None, (Output * 1)(Output(1 << 45, w * bpp, w, h)), bpp, None)
    assert big(65536, 16384) == INVALID and big(65536, 10922) == 0 and big(65536, 10923) == INVALID
    assert big(65536, 8192, flags=CHW, elem=F16) == INVALID and big(65536, 32767, bpp=1) == 0 and big(65536, 32768, bpp=1) == INVALID


def test_entry_points_without_a_device(product_lib):
    lib = product_lib
    assert lib.jda_unpack_surfaces(None, 0, None, HWC, U8, None, None, 4) == 6                       # JDA_ERROR_NO_DEVICE
    assert lib.jda_encode_dense_to_host(None, None, 1, 1, 3, HWC, U8, None, 3, 75, 0, 0, None, 0, None) == 6


def test_denormalise_params_against_its_formula():
    import jpegdec_amd as J
    sb = J.denormalise_params(U.IMAGENET_MEAN, U.IMAGENET_STD)
    assert sb.shape == (2, 3) and sb.dtype == np.float32 and sb.flags["C_CONTIGUOUS"]
    for c in range(3):
        assert sb[0, c] == np.float32(255.0 * U.IMAGENET_STD[c]) and sb[1, c] == np.float32(255.0 * U.IMAGENET_MEAN[c])
    assert np.array_equal(sb, U.denormalise(U.IMAGENET_MEAN, U.IMAGENET_STD))
    g = J.denormalise_params(0.5, 0.25)
    assert g.shape == (2, 1) and g[0, 0] == 63.75 and g[1, 0] == 127.5
    assert np.array_equal(J.denormalise_params(0.0, 1.0), [[255.0], [0.0]])
    # the inverse of normalise_table: every byte comes back
    for dt, elem in ((np.float32, F32), (np.float16, F16)):
        t = J.normalise_table(U.IMAGENET_MEAN, U.IMAGENET_STD, dt)
        img = np.ascontiguousarray(t.T).reshape(256, 1, 3)                 # pixel v = (table[0][v], table[1][v], table[2][v])
        back = U.numpy_unpack(img.reshape(-1).view(np.uint8), 1, 256, 4, HWC, elem, sb).reshape(256, 4)
        assert np.array_equal(back[:, :3], np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)), dt
    with pytest.raises(ValueError):
        J.denormalise_params((0.5, 0.5), (1.0,))


def test_sanitizer_program():
    """the plan and the lanes over a reduced grid as a program of their own under ASan + UBSan (nothing is loaded into this process)"""
    subprocess.run(["make", "unpackasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "unpack_asan")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "unpack_asan ok" in r.stdout, r.stdout[-4000:]


def test_constants_and_exports():
    import jpegdec_amd as J
    for name in ("unpack_surfaces", "encode_dense_to_host", "encode_tensors", "denormalise_params"):
        assert callable(getattr(J, name)), name
    hdr = open(os.path.join(ROOT, "include", "jpegdec_amd.h")).read()
    assert "int jda_unpack_surfaces(" in hdr and "int jda_encode_dense_to_host(" in hdr
    lib = J.load_library()
    assert lib.jda_unpack_surfaces and lib.jda_encode_dense_to_host
