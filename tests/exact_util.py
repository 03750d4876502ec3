"""The libjpeg-exact decode (jda_exact_decode_surfaces) stated once more in numpy, and the files its tests decode.

The definition is libjpeg's: T.81's quantised coefficients times the RAW DQT entries, jidctint.c's 8x8 islow IDCT in 32-bit integers
(CONST_BITS 13, PASS1_BITS 2, the wrapping range-limit table), "fancy" chroma upsampling over the component's own extent with the edge
sample replicated, jdcolor.c's 16-bit colour constants.  twin() is held to Pillow (libjpeg-turbo) bit for bit by tests/test_exact_cpu.py
wherever every pre-limit row result of the file lies in [-512, 511] (WINDOW): libjpeg-turbo's SIMD IDCT saturates where the C table wraps,
so outside that window the contract is the twin alone.  The twin reports the extremes it saw, and every comparison with Pillow asserts them.

Coefficients come from the suite's own entropy decoders (coef_jpeg.decode_coefs / prog_jpeg.decode_coefs through recode_util.decode_any),
which share no code with the library."""
import functools
import io

import numpy as np

from jpegdec_amd.synth import _ZIGZAG
from tests import coef_jpeg
from tests import encode_util as E
from tests import recode_util as R

WINDOW = (-512, 511)
I32 = np.int32
_C = {k: I32(v) for k, v in dict(c0_298=2446, c0_390=3196, c0_541=4433, c0_765=6270, c0_899=7373, c1_175=9633, c1_501=12299, c1_847=15137,
                                 c1_961=16069, c2_053=16819, c2_562=20995, c3_072=25172).items()}


def _descale(x, n):
    return (x + I32(1 << (n - 1))) >> I32(n)


def _pass(d, shift):
    """one pass of jidctint.c's jpeg_idct_islow over the LAST axis of d (.., 8), int32 with wrap-around"""
    c = _C
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * c["c0_541"]
    t2 = z1 - z3 * c["c1_847"]
    t3 = z1 + z2 * c["c0_765"]
    t0, t1 = (d[..., 0] + d[..., 4]) << I32(13), (d[..., 0] - d[..., 4]) << I32(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * c["c1_175"]
    t0, t1, t2, t3 = t0 * c["c0_298"], t1 * c["c2_053"], t2 * c["c3_072"], t3 * c["c1_501"]
    z1, z2, z3, z4 = -z1 * c["c0_899"], -z2 * c["c2_562"], -z3 * c["c1_961"] + z5, -z4 * c["c0_390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)
    return _descale(out, shift)


def range_limit(x):
    """libjpeg's sample_range_limit table behind the IDCT (the index is x & 1023): clamp(x + 128) for x in -512 .. 511, wrapping outside"""
    i = x & I32(1023)
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.uint8)


def idct_islow(blocks):
    """(.., 8, 8) dequantised coefficients (int32, natural order) -> ((.., 8, 8) uint8 samples, min and max of the pre-limit row results)"""
    with np.errstate(over="ignore"):
        ws = _pass(np.asarray(blocks, dtype=I32).swapaxes(-1, -2), 11).swapaxes(-1, -2)      # columns first
        x = _pass(ws, 18)                                                                     # then rows
    return range_limit(x), (int(x.min()), int(x.max())) if x.size else (0, 0)


def own_extents(w, h, sampling):
    hs, vs = coef_jpeg.LUMA_HV[sampling]
    return [(h, w)] + ([] if sampling == "gray" else [((h + vs - 1) // vs, (w + hs - 1) // hs)] * 2)


def planes_of(dec):
    """dec: decode_any's dict -> ([Y, Cb, Cr] uint8 at their OWN extents, (min, max) of the pre-limit row results over the whole MCU grid)"""
    out, lo, hi = [], 0, 0
    for c, (arr, (rows, cols)) in enumerate(zip(dec["coefs"], own_extents(dec["width"], dec["height"], dec["sampling"]))):
        qz = np.asarray(dec["quant"][dec["quant_ids"][c]], dtype=np.int64)
        nat = np.zeros(arr.shape, dtype=np.int64)
        nat[..., _ZIGZAG] = np.asarray(arr, dtype=np.int64) * qz
        nat = ((nat + (1 << 31)) % (1 << 32) - (1 << 31)).astype(I32)
        pix, (a, b) = idct_islow(nat.reshape(arr.shape[0], arr.shape[1], 8, 8))
        lo, hi = min(lo, a), max(hi, b)
        out.append(np.ascontiguousarray(pix.transpose(0, 2, 1, 3).reshape(arr.shape[0] * 8, arr.shape[1] * 8)[:rows, :cols]))
    return out, (lo, hi)


def _h2(t, b_even, b_odd, shift):
    """out[2i] = (3 t[i] + t[i-1] + b_even) >> shift, out[2i+1] = (3 t[i] + t[i+1] + b_odd) >> shift, the edge sample replicated"""
    p = np.pad(t, ((0, 0), (1, 1)), mode="edge")
    out = np.empty((t.shape[0], 2 * t.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * p[:, 1:-1] + p[:, :-2] + b_even) >> shift
    out[:, 1::2] = (3 * p[:, 1:-1] + p[:, 2:] + b_odd) >> shift
    return out


def upsample(s, hs, vs, w, h):
    """libjpeg's fancy upsampling of one chroma plane at its own extent to w x h"""
    s = s.astype(np.int64)
    if hs == 1 and vs == 1:
        return s[:h, :w].astype(np.uint8)
    if vs == 1:
        return _h2(s, 1, 2, 2)[:h, :w].astype(np.uint8)
    p = np.pad(s, ((1, 1), (0, 0)), mode="edge")
    up, dn = 3 * p[1:-1] + p[:-2], 3 * p[1:-1] + p[2:]                # the output rows 2j (nearer the row above) and 2j + 1
    out = np.empty((2 * s.shape[0], s.shape[1] * hs), dtype=np.int64)
    if hs == 1:
        out[0::2], out[1::2] = (up + 1) >> 2, (dn + 2) >> 2
    else:
        out[0::2], out[1::2] = _h2(up, 8, 7, 4), _h2(dn, 8, 7, 4)
    return out[:h, :w].astype(np.uint8)


def colour(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def twin_dec(dec):
    """dict(planes, ycc (H x W x 3, or H x W for gray), rgb (H x W x 3), gray (H x W: the Y plane), range (min, max))"""
    planes, rng = planes_of(dec)
    w, h = dec["width"], dec["height"]
    hs, vs = coef_jpeg.LUMA_HV[dec["sampling"]]
    if len(planes) == 1:
        return dict(planes=planes, ycc=planes[0], rgb=np.repeat(planes[0][..., None], 3, axis=-1), gray=planes[0], range=rng)
    cb, cr = upsample(planes[1], hs, vs, w, h), upsample(planes[2], hs, vs, w, h)
    return dict(planes=planes, ycc=np.stack([planes[0], cb, cr], axis=-1), rgb=colour(planes[0], cb, cr), gray=planes[0], range=rng)


@functools.lru_cache(maxsize=None)
def twin(jpeg):
    return twin_dec(R.decode_any(jpeg))


def natural_blocks(jpeg):
    """(blocks, 64) int16 in natural order, the blocks in the order of the interleaved scan: a coefficient image's own form"""
    zz = R.flat_zigzag(R.decode_any(jpeg))[0]
    nat = np.zeros(zz.shape, dtype=np.int16)
    nat[:, _ZIGZAG] = zz
    return nat


def in_window(t):
    return WINDOW[0] <= t["range"][0] and t["range"][1] <= WINDOW[1]


def rgba(t, gray=False):
    """the surface jda_exact_decode_surfaces writes: RGB8888 (A = 0xFF) as H x 4W bytes, or the Y plane"""
    if gray:
        return t["gray"]
    return np.concatenate([t["rgb"], np.full(t["rgb"].shape[:2] + (1,), 255, np.uint8)], axis=-1).reshape(t["rgb"].shape[0], -1)


def pillow(jpeg, mode="RGB"):
    """Pillow's decode: "RGB" (convert), "L" / "YCbCr" through draft() -- the Y plane / the upsampled planes without colour conversion"""
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    if mode == "RGB":
        return np.asarray(im.convert("RGB"))
    im.draft(mode, im.size)
    assert im.mode == mode or (mode == "YCbCr" and im.mode == "L")
    return np.asarray(im)


# ---- files ------------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (2, 2), (8, 33), (17, 9), (33, 31), (45, 53), (75, 53), (64, 48), (161, 17))
KINDS = ("baseline", "optimize", "progressive", "restart")


@functools.lru_cache(maxsize=None)
def pillow_file(w, h, sampling, q, kind, picture="noise"):
    return R.pillow_files(picture, w, h, sampling, q)[kind]


@functools.lru_cache(maxsize=None)
def written_file(w, h, sampling, q, amplitude=0, seed=5, word=False):
    """a baseline file from coef_jpeg.write_jpeg: a picture's coefficients (amplitude 0), or dense random blocks of +-amplitude in all 64
    positions under quantisers of 1, so that the amplitude is the dequantised one -- or, word=True, under word_quant()"""
    if amplitude == 0:
        img = E.picture("noise", w, h, sampling)
        if sampling != "4:4:0":
            return coef_jpeg.write_jpeg(w, h, sampling, E.coefficients(img, sampling, q), E.quant_tables(q, sampling))
        # (the encoder's twin has no 4:4:0: the planes here, chroma averaged over row pairs, every plane edge-padded to the MCU grid)
        shapes = coef_jpeg.geometry(w, h, sampling)[2]
        y, cb, cr = E.ycc(img)
        planes = [y] + [(lambda p: (p[0::2] + p[1::2] + 1) >> 1)(np.pad(p, ((0, h & 1), (0, 0)), mode="edge")) for p in (cb, cr)]
        lum, chrom = E.quant_natural(q)
        coefs = []
        for c, (p, (rows, cols)) in enumerate(zip(planes, shapes)):
            blocks = E._pad(p, rows * 8, cols * 8).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)
            coefs.append(E.quantise(E.fdct(blocks), (lum if c == 0 else chrom).reshape(8, 8)).reshape(rows, cols, 64)[..., E._ZZ])
        return coef_jpeg.write_jpeg(w, h, sampling, coefs, E.quant_tables(q, "4:2:0"))
    rng = np.random.default_rng(seed)
    coefs = coef_jpeg.zero_coefs(w, h, sampling)
    for c in coefs:
        c[...] = rng.integers(-amplitude, amplitude + 1, size=c.shape)
    qt = word_quant() if word else {0: [1] * 64, 1: [1] * 64}
    if sampling == "gray":
        qt = {0: qt[0]}
    return coef_jpeg.write_jpeg(w, h, sampling, coefs, qt)


def word_quant():
    """16-bit quantisers: a DQT segment of precision 1, products that leave 16 bits"""
    return {0: [600] * 64, 1: [700] * 64}


def grid(sampling):
    """the files of one layout the GPU decodes in one call, and the CPU tests hold to Pillow: [(name, jpeg)]"""
    out = []
    for i, (w, h) in enumerate(SIZES):
        q = (30, 90, 100)[i % 3]
        if sampling == "4:4:0":
            out.append(("written_%dx%d_q%d" % (w, h, q), written_file(w, h, sampling, q)))
            continue
        kind = KINDS[i % 4]
        f = pillow_file(w, h, sampling, q, kind)
        if len(f) < 256:                                                # (the front end refuses smaller files, as the reference does)
            f = pillow_file(w, h, sampling, 100, "progressive" if kind == "progressive" else "baseline", "noise")
        if len(f) >= 256:
            out.append(("%s_%dx%d_q%d" % (kind, w, h, q), f))
        if kind != "progressive":
            p = pillow_file(w, h, sampling, q, "progressive")
            if len(p) >= 256:
                out.append(("progressive_%dx%d_q%d" % (w, h, q), p))
    out.append(("dense60", written_file(33, 31, sampling, 0, amplitude=60)))
    return out
