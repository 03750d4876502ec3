"""The device-only helper branches of jda_device_core.h: one numpy definition per helper, and the inputs the tests hold them to.

tests/devprims/libjda_devprims.so runs every helper's host side (devprims_host_*) and device side (devprims_device_*) through one call
expression.  A definition here is written from what the helper's comment and the instruction's name promise -- uint64 / int64
arithmetic, masks, explicit sign extension -- not from the host branch.  The pixel formulas are restated from jdcolor.c (SCALEBITS 16,
tests/exact_util.colour) and from the reference's constants and 10-bit wrap, as oracle/jpegdec_oracle.c states them.

The generators return (a, b, c) uint32 arrays of one length; the tests assert that the edge cases named in their docstrings are there."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

from tests import exact_util as X
from tests import unpack_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBRARY = os.path.join(ROOT, "tests", "devprims", "libjda_devprims.so")
ASAN_PROGRAM = os.path.join(ROOT, "tests", "devprims", "devprims_asan")
M32 = np.uint64(0xFFFFFFFF)
U32, U64, I64 = np.uint32, np.uint64, np.int64
SEED = 20261021

VAL_OPS = ("alignbyte", "alignbit", "perm", "dup8", "dup16", "pack16", "pk_add16", "pk_sub16", "pk_add16_bhi", "pk_add16_alo", "pk_add16_ahi",
           "pk_sext10_at5", "pk_limit10", "sat_pk_u8", "pk_clamp255", "pk_ashr2", "mad24", "umul24", "mulc_fast", "mulc_full", "rs_mul_u",
           "rs_mul_s", "udot4", "udot4_acc", "shr_upto32", "extend_top", "add_byte0", "bfe", "lag_add", "unpack_half", "unpack_byte",
           "rs_clip_u", "rs_clip_s")
WAVE_OPS = ("excl_sum", "class_rank0", "class_rank1", "class_rank2", "class_rank3", "lane_pull", "wave_any_branch")
LDS_OPS = ("bytes_apart", "load_u16", "coef_store")
CUBE_OPS = ("ex_rgba", "pixel_rgba", "pixel_565_le", "pixel_565_be", "pair_rgba_px0", "pair_rgba_px1", "pair_565_le", "pair_565_be",
            "pair2_rgba_px0", "pair2_rgba_px1", "half_rgba_px0", "half_rgba_px1", "half_565_le", "half_565_be", "rgb_pixel_rgba",
            "rgb_pixel_565_le", "rgb_pixel_565_be")
WAVE_OUTSIDE, WR_STOP = 0x0BADF00D, 0xDEADBEEF
WIN_BYTES, WIN_DWORDS, WR_MAXSTEPS = 256, 64, 2048
CUBE = 1 << 24

# the function or macro of jda_device_core.h / jda_internal.h that encloses a fork -> the ops of the library that run both its sides
FORK_OPS = {
    "jda_alignbyte": ("val:alignbyte",), "jda_perm": ("val:perm", "val:dup8", "val:dup16", "val:pack16"), "jda_pk_add16": ("val:pk_add16",),
    "jda_pk_sub16": ("val:pk_sub16",), "jda_pk_add16_bhi": ("val:pk_add16_bhi",), "jda_pk_add16_alo": ("val:pk_add16_alo",),
    "jda_pk_add16_ahi": ("val:pk_add16_ahi",), "jda_lds_bytes_apart": ("lds:bytes_apart",), "jda_mad24": ("val:mad24",),
    "jda_pk_sext10_at5": ("val:pk_sext10_at5",), "jda_pk_limit10": ("val:pk_limit10",), "jda_sat_pk_u8": ("val:sat_pk_u8",),
    "jda_umul24": ("val:umul24", "val:rs_mul_u"), "jda_udot4": ("val:udot4",), "jda_udot4_acc": ("val:udot4_acc",),
    "jda_wave_excl_sum": ("wave:excl_sum",), "jda_wave_class_rank": ("wave:class_rank0", "wave:class_rank1", "wave:class_rank2", "wave:class_rank3"),
    "jda_add_byte0": ("val:add_byte0",), "jda_bfe": ("val:bfe",),
    "jda_alignbit": ("val:alignbit",), "jda_wr_init": ("wr",), "jda_wr_peek": ("wr",), "JDA_LDS_A32": ("lds:load_u16", "lds:coef_store"),
    "jda_wave_any": ("wave:wave_any_branch",), "jda_mulc": ("val:mulc_fast", "val:mulc_full"), "jda_lag_add": ("val:lag_add",),
    "jda_lane_pull": ("wave:lane_pull",), "jda_pk_clamp255": ("val:pk_clamp255",), "jda_pk_ashr2": ("val:pk_ashr2",),
    "jda_unpack_half": ("val:unpack_half",), "jda_rs_mul": ("val:rs_mul_s",),
}
# .. and the forks that have no value to compare
FORK_EXEMPT = {
    "JDA_OPAQUE": "JDA_OPAQUE / JDA_STORE_ORDER are empty asm statements that only hide a value from, or order stores for, the compiler",
    "jda_atomic_inc_u32": "a global atomic: its value is the order lanes arrive in, which the emulator fixes by stepping them",
    "jda_atomic_or_u32": "a global atomic OR: the same word as the plain OR once every lane is through",
    "jda_lds_or_u32": "the LDS atomic OR: the same word as the plain OR once every lane is through",
    "jda_store_u32x4": "the 16-byte store: four dwords either way, no arithmetic",
    "jda_p1_lists": "emulator-only scaffolding: the host side builds the all[] arrays and skips the overrun stores the wavefront's order makes harmless",
    "jda_decode_block_win": "an address kept in one register the compiler cannot see through: the same sixteen stores",
    "jda_p3_row_class": "an address kept in one register the compiler cannot see through: the same loads and stores",
    "JDA_GLOBAL": "an address-space qualifier (jda_internal.h): no value",
}


# ---- the library ---------------------------------------------------------------------------------------------------------------
def build(*targets):
    subprocess.run(["make", *(targets or ("devprims",))], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def load():
    build("devprims")
    lib = C.CDLL(LIBRARY)
    P = C.c_void_p
    for side in ("host", "device"):
        res = None if side == "host" else C.c_int
        for name, args in (("val", [C.c_int, P, P, P, P, C.c_int]), ("wave", [C.c_int, P, P, P, C.c_int]), ("wr", [P, P, P, P, C.c_int, C.c_int]),
                           ("lds", [C.c_int, P, P, P, P, C.c_int]), ("cube", [C.c_int, P, C.c_uint32, C.c_int])):
            f = getattr(lib, "devprims_%s_%s" % (side, name))
            f.argtypes, f.restype = args, res
    lib.devprims_ops.argtypes, lib.devprims_ops.restype = [C.c_int], C.c_int
    return lib


def _u32(a):
    return np.ascontiguousarray(a, dtype=U32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_val(lib, op, a, b, c):
    a, b, c = _u32(a), _u32(b), _u32(c)
    out = np.full(a.size, 0xA5A5A5A5, U32)
    lib.devprims_host_val(VAL_OPS.index(op), _p(a), _p(b), _p(c), _p(out), a.size)
    return out


def host_wave(lib, op, a, b):
    a, b = _u32(a), _u32(b)
    out = np.full(2 * a.size, 0xA5A5A5A5, U32)
    lib.devprims_host_wave(WAVE_OPS.index(op), _p(a), _p(b), _p(out), a.size)
    return out.reshape(-1, 2)


def host_wr(lib, win, start, steps):
    win, start, steps = _u32(win), _u32(start), np.ascontiguousarray(steps, dtype=np.uint8)
    out = np.full(steps.shape, 0xA5A5A5A5, U32)
    lib.devprims_host_wr(_p(win), _p(start), _p(steps), _p(out), steps.shape[0], steps.shape[1])
    return out


def host_lds(lib, op, win, a, b):
    win, a, b = _u32(win), _u32(a), _u32(b)
    out = np.full(a.size, 0xA5A5A5A5, U32)
    lib.devprims_host_lds(LDS_OPS.index(op), _p(win), _p(a), _p(b), _p(out), a.size)
    return out


def host_cube(lib, op, first, n):
    out = np.full(n, 0xA5A5A5A5, U32)
    lib.devprims_host_cube(CUBE_OPS.index(op), _p(out), first, n)
    return out


def checksum(out):
    """devprims_main.cpp's: the sum of out[i] * (i + 1) modulo 2^64"""
    o = np.asarray(out, U32).reshape(-1).astype(U64)
    with np.errstate(over="ignore"):
        return int((o * np.arange(1, o.size + 1, dtype=U64)).sum(dtype=U64))


def first_difference(name, want, got, *inputs):
    """None, or the op, the first differing element's inputs and both results"""
    want, got = np.asarray(want).reshape(-1), np.asarray(got).reshape(-1)
    if want.shape == got.shape and np.array_equal(want, got):
        return None
    if want.shape != got.shape:
        return "%s: %d results for %d" % (name, got.size, want.size)
    i = int(np.flatnonzero(want != got)[0])
    ins = ", ".join("0x%08x" % int(np.asarray(v).reshape(-1)[i * np.asarray(v).size // want.size]) for v in inputs)
    return "%s: element %d of %d (%d differ), inputs (%s): definition 0x%08x, got 0x%08x" % (name, i, want.size, int(np.count_nonzero(want != got)), ins, int(want[i]), int(got[i]))


# ---- definitions: family 1 ---------------------------------------------------------------------------------------------------------
def _sext(x, bits):
    """the low `bits` bits of x as a signed number (int64)"""
    x = np.asarray(x).astype(U64) & U64((1 << bits) - 1)
    return np.where(x >> U64(bits - 1) != 0, x.astype(I64) - I64(1 << bits), x.astype(I64))


def _halves(x):
    x = np.asarray(x, U32).astype(U64)
    return x & U64(0xFFFF), x >> U64(16)


def _join(lo, hi):
    return ((np.asarray(lo).astype(I64) & I64(0xFFFF)) | ((np.asarray(hi).astype(I64) & I64(0xFFFF)) << I64(16))).astype(U32)


def _wrap32(x):
    return (np.asarray(x).astype(I64) & I64(0xFFFFFFFF)).astype(U32)


def _pool(hi, lo):
    return (np.asarray(hi, U32).astype(U64) << U64(32)) | np.asarray(lo, U32).astype(U64)


def _perm(hi, lo, sel):
    """v_perm_b32: byte i of the result is chosen by byte i of sel from the pool {hi, lo}: 0..7 a byte, 8..11 the replicated sign of
    lo's low half, lo's high half, hi's low half, hi's high half, 12 -> 0x00, 13 and above -> 0xff"""
    pool, sel, r = _pool(hi, lo), np.asarray(sel, U32).astype(U64), np.zeros(np.shape(sel), U64)
    for i in range(4):
        k = (sel >> U64(8 * i)) & U64(0xFF)
        byte = (pool >> (U64(8) * np.minimum(k, U64(7)))) & U64(0xFF)
        sign = ((pool >> (U64(16) * (np.clip(k, U64(8), U64(11)) - U64(8)) + U64(15))) & U64(1)) * U64(0xFF)
        b = np.where(k < 8, byte, np.where(k < 12, sign, np.where(k == 12, U64(0), U64(0xFF))))
        r |= b << U64(8 * i)
    return r.astype(U32)


def _clamp255(x):
    return np.clip(x, 0, 255)


def _bytes(x):
    x = np.asarray(x, U32).astype(U64)
    return [(x >> U64(8 * i)) & U64(0xFF) for i in range(4)]


def _f32(bits):
    return np.asarray(bits, U32).view(np.float32)


def define_val(op, a, b, c):
    a, b, c = (np.asarray(v, U32) for v in (a, b, c))
    A, B, Cc = a.astype(U64), b.astype(U64), c.astype(U64)
    al, ah = _halves(a)
    bl, bh = _halves(b)
    if op == "alignbyte":                                   # v_alignbyte_b32: ({hi, lo} >> 8 * (shift & 3)), low 32 bits
        return ((_pool(a, b) >> (U64(8) * (Cc & U64(3)))) & M32).astype(U32)
    if op == "alignbit":                                    # v_alignbit_b32: ({hi, lo} >> (shift & 31)), low 32 bits
        return ((_pool(a, b) >> (Cc & U64(31))) & M32).astype(U32)
    if op == "perm":
        return _perm(a, b, c)
    if op == "dup8":
        return ((A & U64(0xFF)) * U64(0x01010101)).astype(U32)
    if op == "dup16":
        return _join(al, al)
    if op == "pack16":
        return _join(al, bl)
    if op == "pk_add16":
        return _join(al + bl, ah + bh)
    if op == "pk_sub16":
        return _join(al.astype(I64) - bl.astype(I64), ah.astype(I64) - bh.astype(I64))
    if op == "pk_add16_bhi":
        return _join(al + bh, ah + bh)
    if op == "pk_add16_alo":
        return _join(al + bl, al + bh)
    if op == "pk_add16_ahi":
        return _join(ah + bl, ah + bh)
    if op == "pk_sext10_at5":
        return _join(_sext(al >> U64(5), 10), _sext(ah >> U64(5), 10))
    if op == "pk_limit10":                                  # the three packed steps of the comment, each modulo / saturating at 2^16
        def lane(h):
            x = (h * U64(2) + U64(0x8000)) & U64(0xFFFF)
            x = np.where(x > 24576, x - U64(24576), U64(0))
            return np.minimum(x * U64(4), U64(0xFFFF))
        return _join(lane(al), lane(ah))
    if op == "sat_pk_u8":
        return (_clamp255(_sext(al, 16)) | (_clamp255(_sext(ah, 16)) << I64(8))).astype(U32)
    if op == "pk_clamp255":
        return _join(_clamp255(_sext(al, 16)), _clamp255(_sext(ah, 16)))
    if op == "pk_ashr2":
        return _join(_sext(al, 16) >> I64(2), _sext(ah, 16) >> I64(2))
    if op == "mad24":                                       # v_mad_i32_i24
        return _wrap32(_sext(a, 24) * _sext(b, 24) + _sext(c, 32))
    if op in ("umul24", "rs_mul_u"):                        # v_mul_u32_u24
        return (((A & U64(0xFFFFFF)) * (B & U64(0xFFFFFF))) & M32).astype(U32)
    if op in ("mulc_fast", "rs_mul_s"):                     # v_mul_i32_i24
        return _wrap32(_sext(a, 24) * _sext(b, 24))
    if op == "mulc_full":                                   # v_mul_lo_u32
        return _wrap32(_sext(a, 32) * _sext(b, 32))
    if op in ("udot4", "udot4_acc"):
        s = sum(x * y for x, y in zip(_bytes(a), _bytes(b)))
        return ((s + (Cc if op == "udot4_acc" else U64(0))) & M32).astype(U32)
    if op == "shr_upto32":                                  # the hardware's shift: n mod 32 (n == 32 gives x)
        return (A >> (B & U64(31))).astype(U32)
    if op == "extend_top":                                  # EXTEND of the top s bits of t, s = 1 .. 31
        assert 1 <= int(b.min()) and int(b.max()) < 32
        v = (A >> (U64(32) - B)).astype(I64)
        return _wrap32(np.where(A >> U64(31) != 0, v, v - ((I64(1) << B.astype(I64)) - I64(1))))
    if op == "add_byte0":
        return ((A + (B & U64(0xFF))) & M32).astype(U32)
    if op == "bfe":                                         # v_bfe_u32: offset & 31, width & 31
        return ((A >> (B & U64(31))) & ((U64(1) << (Cc & U64(31))) - U64(1))).astype(U32)
    if op == "lag_add":                                     # n added to each of the six 5-bit fields of the low 30 bits, modulo 2^32
        return ((A + sum(B << U64(5 * k) for k in range(6))) & M32).astype(U32)
    if op == "unpack_half":                                 # the float16's value in float32; a NaN comes out quiet
        h = a.astype(np.uint16).view(np.float16)
        bits = h.astype(np.float32).view(U32).copy()
        bits[np.isnan(h)] |= U32(0x00400000)
        return bits
    if op == "unpack_byte":                                 # two roundings (tests/unpack_util.numpy_unpack)
        with np.errstate(all="ignore"):
            return U._bytes_of(np.rint(_f32(a) * _f32(b) + _f32(c))).astype(U32)
    if op == "rs_clip_u":
        return np.minimum(((A + U64(1 << 21)) & M32) >> U64(22), U64(255)).astype(U32)
    if op == "rs_clip_s":                                   # clip8(t >> 22), t = acc + 2^21 as a 32-bit two's-complement sum
        return _clamp255(_sext(A + U64(1 << 21), 32) >> I64(22)).astype(U32)
    raise KeyError(op)


# ---- inputs: family 1 --------------------------------------------------------------------------------------------------------------
def _rng(tag):
    return np.random.RandomState((SEED + sum(map(ord, tag))) & 0x7FFFFFFF)


def _words(rng, n):
    return ((rng.randint(0, 1 << 16, n).astype(U64) << U64(16)) | rng.randint(0, 1 << 16, n).astype(U64)).astype(U32)


def packed_one():
    """every 16-bit value in each half: x low and ~x high, the halves swapped, 65,536 random words"""
    x = np.arange(1 << 16, dtype=U64)
    nx = x ^ U64(0xFFFF)
    return np.concatenate([(x | (nx << U64(16))), (nx | (x << U64(16))), _words(_rng("one"), 1 << 16).astype(U64)]).astype(U32)


PAIR_EDGES = (0, 1, 2, 0x7F, 0x80, 0xFF, 0x100, 0x7FFF, 0x8000, 0x8001, 0xFFFE, 0xFFFF)


def packed_two():
    """all pairs of the 12-value edge set per half, crossed over both halves (12^4 = 20,736 words), + 65,536 random pairs"""
    q = np.array(list(itertools.product(PAIR_EDGES, repeat=4)), dtype=U64)
    a, b = q[:, 0] | (q[:, 1] << U64(16)), q[:, 2] | (q[:, 3] << U64(16))
    rng = _rng("two")
    return np.concatenate([a.astype(U32), _words(rng, 1 << 16)]), np.concatenate([b.astype(U32), _words(rng, 1 << 16)])


# every selector constant of a jda_perm call in the tree (all of them are in jda_device_core.h), collected by hand, in the header's order;
# tests/test_devprims_cpu.py reads the header and fails on a constant that is not here
PERM_SELECTORS = (
    0x00000000, 0x01000100, 0x05040100,                                     # jda_dup8, jda_dup16, jda_pack16
    0x05070301,                                                             # jda_idct_row: the range-limited bytes of a row
    0x07060302, 0x0d040100, 0x0d050100, 0x02030001, 0x0c010c00, 0x0c030c02,      # jda_pack_hi16, the RGB8888 / RGB565 pairs, the luma pairs
    0x06040200,                                                             # jda_pair_sums' neighbour: four sums >> 2 as bytes
    0x05010400, 0x0d050302,                                                 # jda_rgba_pair_half
    0x00010203, 0x01000302,                                                 # jda_bswap32, the orient kernel's pixel reversal
    0x07030602,                                                             # the orient kernel's transposition
    0x06000102, 0x05060001, 0x04050600, 0x04020100, 0x05040201, 0x06050402,      # the pack kernel: three channels out of RGBA, by phase, BGR and RGB
    0x0d000102, 0x0d020100, 0x0d030405, 0x0d050403, 0x0d020304, 0x0d040302, 0x0d010203, 0x0d030201,      # the unpack kernel: RGB(A) from dense bytes
) + tuple(0x0c0c0400 + p * 0x0101 for p in range(4)) + tuple(0x0d040100 + (p << 16) for p in range(4))      # .. and its planar gather, p = 0 .. 3
# the computed selectors of jda_be64_from_words / jda_load_be64 (an alignbyte of these pairs by ~pos) are made in perm_inputs
PERM_SELECTOR_PARTS = (0x00000102, 0x03040506, 0x08070605, 0x04030201)


def perm_inputs():
    """each of the 256 selector byte values in each of the four positions (the other three random), over 16 random pools each; the tree's
    selector constants and the selectors jda_load_be64 / jda_be64_from_words make, over 64 pools; 65,536 random selectors"""
    rng = _rng("perm")
    sel = []
    for pos in range(4):
        for v in range(256):
            s = _words(rng, 16) & ~U32(0xFF << (8 * pos)) | U32(v << (8 * pos))
            sel.append(s)
    h0, l0, h1, l1 = PERM_SELECTOR_PARTS
    made = [(((h << 32) | l) >> (8 * k)) & 0xFFFFFFFF for h, l in ((h0, l0), (h1, l1)) for k in range(4)]
    sel.append(np.repeat(np.array(PERM_SELECTORS + tuple(made), dtype=U32), 64))
    sel.append(_words(rng, 1 << 16))
    sel = np.concatenate(sel)
    return _words(rng, sel.size), _words(rng, sel.size), sel


def shift_inputs(op):
    rng = _rng(op)
    if op == "alignbyte":                                   # shift 0 .. 7 (the instruction masks to 0 .. 3) and random words
        c = np.concatenate([np.repeat(np.arange(8, dtype=U32), 256), _words(rng, 2048)])
    elif op == "alignbit":                                  # shift 0 .. 63
        c = np.concatenate([np.repeat(np.arange(64, dtype=U32), 128), _words(rng, 2048)])
    else:
        raise KeyError(op)
    return _words(rng, c.size), _words(rng, c.size), c


def bfe_inputs():
    """every (off, width) with off + width <= 32 and width <= 31, and width 32 at every offset, over 32 words each (all ones among them)"""
    rng = _rng("bfe")
    ow = [(o, w) for w in range(32) for o in range(33 - w) if o < 32] + [(o, 32) for o in range(32)]
    ow = np.array(ow, dtype=U32)
    v = _words(rng, len(ow) * 32).reshape(len(ow), 32)
    v[:, 0], v[:, 1] = 0xFFFFFFFF, 0x80000001
    return v.reshape(-1), np.repeat(ow[:, 0], 32), np.repeat(ow[:, 1], 32)


MUL_EDGES = (0, 1, -1, (1 << 23) - 1, -((1 << 23) - 1), -(1 << 23), 1 << 23, (1 << 24) - 1)


def mul_inputs():
    """operands at 0, +-1, +-(2^23 - 1), -2^23, 2^23, 2^24 - 1 (all pairs), random inside 24 signed bits, random full words, and a
    small operand against a full word; c: random full words"""
    rng = _rng("mul")
    e = np.array(list(itertools.product(MUL_EDGES, repeat=2)), dtype=I64)
    n = 1 << 15
    in24 = lambda: (rng.randint(-(1 << 23), 1 << 23, n).astype(I64))
    a = np.concatenate([e[:, 0], in24(), _words(rng, n).astype(I64), rng.randint(0, 256, n).astype(I64)])
    b = np.concatenate([e[:, 1], in24(), _words(rng, n).astype(I64), _words(rng, n).astype(I64)])
    return _wrap32(a), _wrap32(b), _words(rng, a.size)


def udot4_inputs():
    """random words, and all bytes 0xff with accumulators that make the sum wrap"""
    rng = _rng("udot4")
    n = 1 << 14
    a, b, c = _words(rng, n), _words(rng, n), _words(rng, n)
    a[:8] = b[:8] = 0xFFFFFFFF
    c[:8] = np.array([0xFFFFFFFF, 0xFFFC07FC, 0xFFFC07FB, 0xFFFC07FD, 0, 1, 0x80000000, 0xFFFFFFFE], dtype=U32)      # (4 * 255^2 = 0x3F804)
    return a, b, c


def shr_inputs(op):
    rng = _rng(op)
    n = np.repeat(np.arange(1, 32, dtype=U32) if op == "extend_top" else np.array(list(range(34)) + [63, 64, 0xFFFFFFE0], dtype=U32), 256)
    t = _words(rng, n.size)
    t[::4] |= 0x80000000
    t[1::4] &= 0x7FFFFFFF
    return t, n, np.zeros(n.size, U32)


def add_byte0_inputs():
    rng = _rng("add_byte0")
    n = 1 << 14
    a, b = _words(rng, n), _words(rng, n)
    a[:4], b[:4] = [0xFFFFFFFF, 0xFFFFFF01, 0, 0xFFFFFFFF], [0xFFFFFFFF, 0x123456FF, 0xFFFFFF00, 0x00000001]
    return a, b, np.zeros(n, U32)


def lag_inputs():
    """n = 0 .. 3 over random U and over U with every 5-bit field at 0 and at 31 (all 64 combinations, random top bits)"""
    rng = _rng("lag")
    combos = np.array([sum((31 if (m >> k) & 1 else 0) << (5 * k) for k in range(6)) for m in range(64)], dtype=U32)
    U_ = np.concatenate([combos, combos | U32(0xC0000000), combos | U32(0x40000000), _words(rng, 4096)])
    return np.tile(U_, 4), np.repeat(np.arange(4, dtype=U32), U_.size), np.zeros(4 * U_.size, U32)


def half_inputs():
    a = np.arange(1 << 16, dtype=U32)
    return a, np.zeros(a.size, U32), np.zeros(a.size, U32)


def unpack_byte_inputs():
    """the value pool of tests/unpack_util.py (ties, both NaN kinds, infinities, subnormals, the contraction set) of both element types
    under the scale and bias pairs of its parameter sets; returns (x, s, b) as float32 bits and the number of elements at which ONE
    rounding (a fused multiply-add) gives another byte"""
    xs, ss, bs = [], [], []
    pairs = {(255.0, 0.0)}
    for sb in U.param_sets(3).values():
        if sb is not None:
            pairs |= {(float(sb[0][k]), float(sb[1][k])) for k in range(3)}
    for s, b in sorted(pairs):
        s32, b32 = np.float32(s), np.float32(b)
        with np.errstate(all="ignore"):
            pool = np.concatenate([U.float_pool(U.F32, s32, b32).astype(U32), U.float_pool(U.F16, s32, b32).astype(np.uint16).view(np.float16).astype(np.float32).view(U32)])
        xs.append(pool)
        ss.append(np.full(pool.size, s32, np.float32).view(U32))
        bs.append(np.full(pool.size, b32, np.float32).view(U32))
    x, s, b = np.concatenate(xs), np.concatenate(ss), np.concatenate(bs)
    with np.errstate(all="ignore"):
        two = U._bytes_of(np.rint(_f32(x) * _f32(s) + _f32(b)))
        one = U._bytes_of(np.rint((_f32(x).astype(np.float64) * _f32(s).astype(np.float64) + _f32(b).astype(np.float64)).astype(np.float32)))
    return x, s, b, int(np.count_nonzero(two != one))


def rs_clip_inputs():
    """a stride through the 32-bit range, every value within +-2 of a multiple of 2^22, and +-2 around both clamp ends of both forms"""
    stride = np.arange(0, 1 << 32, 65521, dtype=U64)
    near = (np.arange(0, 1 << 32, 1 << 22, dtype=I64)[:, None] + np.arange(-2, 3, dtype=I64)[None, :]).reshape(-1)
    ends = [-(1 << 21), (255 << 22) - (1 << 21), (256 << 22) - (1 << 21), (1 << 30) - 1 - (1 << 21), (1 << 31) - 1, -(1 << 31), (1 << 31) - (1 << 21), 0]
    ends = (np.array(ends, dtype=I64)[:, None] + np.arange(-2, 3, dtype=I64)[None, :]).reshape(-1)
    a = np.concatenate([stride.astype(I64), near, ends])
    a = _wrap32(a)
    return a, np.zeros(a.size, U32), np.zeros(a.size, U32)


def val_inputs(op):
    z = lambda a: (a, np.zeros(a.size, U32), np.zeros(a.size, U32))
    if op in ("pk_sext10_at5", "pk_limit10", "sat_pk_u8", "pk_clamp255", "pk_ashr2", "dup8", "dup16"):
        return z(packed_one())
    if op in ("pk_add16", "pk_sub16", "pk_add16_bhi", "pk_add16_alo", "pk_add16_ahi", "pack16"):
        a, b = packed_two()
        return a, b, np.zeros(a.size, U32)
    if op == "perm":
        return perm_inputs()
    if op in ("alignbyte", "alignbit"):
        return shift_inputs(op)
    if op == "bfe":
        return bfe_inputs()
    if op in ("mad24", "umul24", "mulc_fast", "mulc_full", "rs_mul_u", "rs_mul_s"):
        return mul_inputs()
    if op in ("udot4", "udot4_acc"):
        return udot4_inputs()
    if op in ("shr_upto32", "extend_top"):
        return shr_inputs(op)
    if op == "add_byte0":
        return add_byte0_inputs()
    if op == "lag_add":
        return lag_inputs()
    if op == "unpack_half":
        return half_inputs()
    if op == "unpack_byte":
        return unpack_byte_inputs()[:3]
    if op in ("rs_clip_u", "rs_clip_s"):
        return rs_clip_inputs()
    raise KeyError(op)


# ---- family 2: wave helpers ------------------------------------------------------------------------------------------------------
def wave_inputs(op):
    """[groups, 64] operands a, b"""
    rng = _rng("wave" + op)
    rows_a, rows_b = [], []

    def add(a, b=None):
        rows_a.append(np.asarray(a, dtype=U64).astype(U32))
        rows_b.append(np.zeros(64, U32) if b is None else np.asarray(b, dtype=U64).astype(U32))
    one_hot = np.eye(64, dtype=U64)
    if op == "excl_sum":                                    # all 0, all 1, one lane set (each of the 64), values up to 2^32 - 1 (sums wrap), random
        add(np.zeros(64)), add(np.ones(64)), add(np.full(64, 0xFFFFFFFF))
        for l in range(64):
            add(one_hot[l]), add(one_hot[l] * 0xFFFFFFFF)
        for _ in range(32):
            add(_words(rng, 64)), add(rng.randint(0, 9, 64) | (rng.randint(0, 9, 64) << 16))
    elif op.startswith("class_rank"):                       # all equal (each class), none (class 4), one lane of the class, random
        for cls in range(5):
            add(np.full(64, cls))
        for l in range(64):
            add(4 - one_hot[l] * (4 - int(op[-1])))
        for _ in range(32):
            add(rng.randint(0, 5, 64))
    elif op == "lane_pull":                                 # a random permutation, all lanes pulling one lane, sources >= 64 (wrap modulo 64)
        for _ in range(8):
            add(_words(rng, 64), rng.permutation(64))
        for l in (0, 1, 31, 32, 63):
            add(_words(rng, 64), np.full(64, l))
        for _ in range(8):
            add(_words(rng, 64), rng.permutation(64) + 64 * rng.randint(1, 1 << 20, 64))
        add(_words(rng, 64), _words(rng, 64) & U32(0x3FFFFFFF))
    elif op == "wave_any_branch":                           # b: who goes in; a: who says yes
        for inside in (np.zeros(64), np.ones(64), np.arange(64) % 2, np.arange(64) < 32, np.arange(64) >= 32):
            for yes in (np.zeros(64), np.ones(64), inside, 1 - np.asarray(inside, dtype=U64)):
                add(yes, inside)
        for l in range(64):
            add(one_hot[l], 1 - one_hot[l])                 # the only yes stays outside: the lanes inside must see a no
            add(one_hot[l], one_hot[l] + one_hot[(l + 7) % 64])
        for _ in range(32):
            add(rng.randint(0, 4, 64) == 0, rng.randint(0, 2, 64))
    else:
        raise KeyError(op)
    return np.stack(rows_a), np.stack(rows_b)


def define_wave(op, a, b, host=False):
    """[groups, 64, 2]: what every lane reports.  host: jda_wave_any's host side is by design the lane's own answer (the emulator steps
    the lanes one after another), so the host loop reports that"""
    A, B = a.astype(U64), b.astype(U64)
    out = np.zeros(a.shape + (2,), U64)
    if op == "excl_sum":
        cs = np.cumsum(A, axis=1)
        out[..., 0], out[..., 1] = (cs - A) & M32, (cs[:, -1:] & M32)
    elif op.startswith("class_rank"):
        m = (a == int(op[-1])).astype(U64)
        cs = np.cumsum(m, axis=1)
        out[..., 0], out[..., 1] = cs - m, cs[:, -1:]
    elif op == "lane_pull":
        out[..., 0] = np.take_along_axis(A, (B & U64(63)).astype(np.intp), axis=1)
    elif op == "wave_any_branch":
        inside, yes = b != 0, a != 0
        if host:
            out[..., 0], out[..., 1] = np.where(inside, yes, WAVE_OUTSIDE), inside
        else:
            out[..., 0] = np.where(inside, (inside & yes).any(axis=1, keepdims=True), WAVE_OUTSIDE)
            out[..., 1] = inside.any(axis=1, keepdims=True)
    else:
        raise KeyError(op)
    return out.astype(U32).reshape(-1, 2)


# ---- family 3: LDS helpers -------------------------------------------------------------------------------------------------------
def window():
    """64 random dwords, as they lie in LDS"""
    return _words(_rng("window"), WIN_DWORDS)


def window_peeks(win):
    """peek[q]: the 32 bits of the window's bit string from bit q on (a dword's top bit first), q = 0 .. 2016"""
    bits = np.unpackbits(np.asarray(win, U32).astype(">u4").view(np.uint8)).astype(U64)
    weights = U64(1) << np.arange(31, -1, -1, dtype=U64)
    return (np.lib.stride_tricks.sliding_window_view(bits, 32) * weights).sum(axis=1).astype(U32)


def wr_walks():
    """start [n] (pos << 3 | off: every pos 0..15 x off 0..7), steps [n, WR_MAXSTEPS] of 1 .. 16 bits: three random walks a start, and from
    sixteen of the starts a walk of constant step k, k = 1 .. 16"""
    rng = _rng("walks")
    start, steps = [], []
    for pos in range(16):
        for off in range(8):
            for _ in range(3):
                start.append(pos << 3 | off)
                steps.append(rng.randint(1, 17, WR_MAXSTEPS))
    for k in range(1, 17):
        start.append(((k * 5) % 16) << 3 | (k % 8) if k > 1 else 0)
        steps.append(np.full(WR_MAXSTEPS, k))
    return np.array(start, dtype=U32), np.array(steps, dtype=np.uint8)


def define_wr(win, start, steps):
    """peek for peek: the walk peeks, consumes its step, and ends at the last position from which a peek stays inside the window"""
    peeks = window_peeks(win)
    q = (start >> 3).astype(I64)[:, None] * 8 + (start & 7).astype(I64)[:, None] + np.concatenate([np.zeros((len(start), 1), I64), np.cumsum(steps.astype(I64), axis=1)[:, :-1]], axis=1)
    ok = q <= 8 * WIN_BYTES - 32
    return np.where(ok, peeks[np.minimum(q, 8 * WIN_BYTES - 32)], U32(WR_STOP)).astype(U32)


def lds_inputs(op):
    rng = _rng("lds" + op)
    if op == "bytes_apart":                                 # step and delta 0 .. 127 each (the library reduces them so): every byte of the window is read
        a, b = np.tile(np.arange(128, dtype=U32), 128), np.repeat(np.arange(128, dtype=U32), 128)
    elif op == "load_u16":                                  # every even offset
        a, b = np.tile(np.arange(0, 255, 2, dtype=U32), 2)[:256], np.zeros(256, U32)
    elif op == "coef_store":                                # a group's 64 lanes: distinct even offsets in byte 0 of t, random bits above it
        groups = 32
        a = np.stack([rng.permutation(128)[:64] * 2 for _ in range(groups)]).astype(U32) | (_words(rng, groups * 64).reshape(groups, 64) & U32(0xFFFFFF00))
        a[0] &= U32(0xFF)
        a, b = a.reshape(-1), _words(rng, groups * 64)
    else:
        raise KeyError(op)
    return a, b


def define_lds(op, win, a, b):
    wb = np.asarray(win, U32).astype("<u4").view(np.uint8).astype(U32)
    if op == "bytes_apart":
        return wb[a] | (wb[a + b] << U32(8))
    if op == "load_u16":
        return wb[a] | (wb[a + 1] << U32(8))
    if op == "coef_store":
        out = []
        for ga, gb in zip(a.reshape(-1, 64), b.reshape(-1, 64)):
            w = wb.astype(np.uint8).copy()
            o = (ga & 0xFE).astype(np.intp)
            assert len(set(o.tolist())) == 64
            w[o], w[o + 1] = gb & 0xFF, (gb >> 8) & 0xFF
            out.append(w.view("<u4").astype(U32))
        return np.concatenate(out)
    raise KeyError(op)


# ---- family 4: the pixel cube ------------------------------------------------------------------------------------------------------
def _rgba(r, g, b):
    return (_clamp255(r) | (_clamp255(g) << 8) | (_clamp255(b) << 16) | I64(0xFF000000)).astype(U32)


def _wrap10(x):
    """the reference's usRangeTable index: x & 0x3ff as a 10-bit two's-complement number, then clamped"""
    return _clamp255(_sext(x, 10))


def _p565(r, g, b, big):
    """one RGB565 pixel of three 8-bit channels; big: the two bytes swapped"""
    v = ((r >> 3) << 11) | ((g >> 2) << 5) | (b >> 3)
    return np.where(big, ((v & 0xFF) << 8) | (v >> 8), v)


def _ref_channels(ys, cb, cr, shift):
    """jpeg.inl:3158-3161 (oracle put_pixel): (k * (c - 128) + iY) >> shift for iY = luma << shift (full size: Y << 12; half size: the
    2x2 sum << 10), int64"""
    cb, cr = cb - 128, cr - 128
    return (5742 * cr + ys) >> shift, (-1409 * cb - 2925 * cr + ys) >> shift, (7258 * cb + ys) >> shift


def define_cube(op, first, n):
    i = np.arange(first, first + n, dtype=I64)
    y, cb, cr = (i >> 16) & 255, (i >> 8) & 255, i & 255
    y1 = 255 - y
    if op == "ex_rgba":
        c = X.colour(y, cb, cr).astype(I64)
        return _rgba(c[..., 0], c[..., 1], c[..., 2])
    kind = op.split("_")[0]
    big = op.endswith("_be")
    if kind in ("pixel", "rgb"):                            # one pixel at full size: iY = Y << 12
        r, g, b = _ref_channels(y << 12, cb, cr, 12)
        return _rgba(r, g, b) if op.endswith("_rgba") else _p565(_wrap10(r), _wrap10(g), _wrap10(b), big).astype(U32)
    if kind in ("pair", "pair2"):
        swap = kind == "pair2"                              # the second pixel's chroma samples: its own (Cr, Cb), or the first's
        r0, g0, b0 = _ref_channels(y << 12, cb, cr, 12)
        r1, g1, b1 = _ref_channels(y1 << 12, cr if swap else cb, cb if swap else cr, 12)
        if "rgba" in op:
            return _rgba(r0, g0, b0) if op.endswith("px0") else _rgba(r1, g1, b1)
        p0, p1 = _p565(_wrap10(r0), _wrap10(g0), _wrap10(b0), big), _p565(_wrap10(r1), _wrap10(g1), _wrap10(b1), big)
        return (p0 | (p1 << 16)).astype(U32)
    if kind == "half":                                      # jpeg.inl:3577-3626: luma = the 2x2 sum << 10, chroma the sample at its place
        s0 = 4 * y + (cr & 3)
        s1 = 1023 - s0
        r0, g0, b0 = _ref_channels(s0 << 10, cb, cr, 12)
        r1, g1, b1 = _ref_channels(s1 << 10, cr, cb, 12)
        if "rgba" in op:
            return _rgba(r0, g0, b0) if op.endswith("px0") else _rgba(r1, g1, b1)
        p0, p1 = _p565(_wrap10(r0), _wrap10(g0), _wrap10(b0), big), _p565(_wrap10(r1), _wrap10(g1), _wrap10(b1), big)
        return (p0 | (p1 << 16)).astype(U32)
    raise KeyError(op)
