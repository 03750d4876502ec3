"""The libjpeg-exact decode at 1/2, 1/4 and 1/8 (jda_exact_decode_surfaces_scaled) stated in numpy, and the files its tests
decode.  It is libjpeg's scaled decode as Pillow's Image.draft() drives it:

  scale s in {1, 2, 4, 8}, min = 8 / s, the output ceil(W / s) x ceil(H / s);
  per component (jdmaster.c) an IDCT size ss: from min, doubled while ss < 8 and hmax min % (h_c ss 2) == 0 and vmax min % (v_c ss 2) == 0
  -- min for luma, 2 min for the chroma of 4:2:0 (which then needs no upsampling), min for every other chroma;
  jidctred.c's 4x4, 2x2 and 1x1 IDCTs (CONST_BITS 13, PASS1_BITS 2, 32-bit integers that wrap), jidctint.c's 8x8 where ss is 8;
  jdsample.c: fancy upsampling only while min > 1, h2v1 fancy only where the component's own width is > 2, else replication;
  dequantisation, range limit and colour conversion as at full size (tests/exact_util.py, whose functions this file imports).

The comparison window carries over: twin_scaled() is held to Pillow wherever every pre-limit result of the file lies in -512 .. 511."""
import functools
import io

import numpy as np

from jpegdec_amd.synth import _ZIGZAG
from tests import coef_jpeg
from tests import encode_util as E
from tests import exact_util as X
from tests import recode_util as R

I32 = np.int32
SCALES = (1, 2, 4, 8)
UP_NONE, UP_H2V1_FANCY, UP_H2V1_REPLICATE, UP_H1V2_FANCY, UP_H1V2_REPLICATE = 0, 1, 2, 3, 4


def component_sizes(sampling, s):
    """[ss of Y, (Cb, Cr)]: the IDCT size of each component at scale s"""
    mn = 8 // s
    hmax, vmax = coef_jpeg.LUMA_HV[sampling]
    out = []
    for h_c, v_c in [(hmax, vmax)] + ([] if sampling == "gray" else [(1, 1)] * 2):
        ss = mn
        while ss < 8 and (hmax * mn) % (h_c * ss * 2) == 0 and (vmax * mn) % (v_c * ss * 2) == 0:
            ss *= 2
        out.append(ss)
    return out


def scaled_size(w, h, s):
    return -(-w // s), -(-h // s)


def own_extents(w, h, sampling, s):
    """(rows, cols) of each component's own extent at scale s"""
    hmax, vmax = coef_jpeg.LUMA_HV[sampling]
    out = []
    for c, ss in enumerate(component_sizes(sampling, s)):
        h_c, v_c = (hmax, vmax) if c == 0 else (1, 1)
        out.append((-(-h * v_c * ss // (vmax * 8)), -(-w * h_c * ss // (hmax * 8))))
    return out


def upsampling_kind(w, h, sampling, s):
    """what jdsample.c does to the chroma planes at scale s < 1 (UP_*)"""
    if sampling in ("gray", "4:4:4", "4:2:0") or s == 1:
        assert s > 1 or sampling in ("gray", "4:4:4")
        return UP_NONE
    fancy = 8 // s > 1
    if sampling == "4:2:2":
        return UP_H2V1_FANCY if fancy and own_extents(w, h, sampling, s)[1][1] > 2 else UP_H2V1_REPLICATE
    return UP_H1V2_FANCY if fancy else UP_H1V2_REPLICATE


def _descale(x, n):
    return (x + I32(1 << (n - 1))) >> I32(n)


def _pass4(d, shift):
    """one pass of jidctred.c's jpeg_idct_4x4 over the LAST axis of d (.., 8) -> (.., 4); d[..., 4] is not read"""
    t0 = d[..., 0] << I32(14)
    t2 = d[..., 2] * I32(15137) - d[..., 6] * I32(6270)
    t10, t12 = t0 + t2, t0 - t2
    a = -d[..., 7] * I32(1730) + d[..., 5] * I32(11893) - d[..., 3] * I32(17799) + d[..., 1] * I32(8697)
    c = -d[..., 7] * I32(4176) - d[..., 5] * I32(4926) + d[..., 3] * I32(7373) + d[..., 1] * I32(20995)
    return _descale(np.stack([t10 + c, t12 + a, t12 - a, t10 - c], axis=-1), shift)


def _pass2(d, shift):
    """one pass of jpeg_idct_2x2: frequencies 0, 1, 3, 5, 7 only"""
    t10 = d[..., 0] << I32(15)
    t0 = -d[..., 7] * I32(5906) + d[..., 5] * I32(6967) - d[..., 3] * I32(10426) + d[..., 1] * I32(29692)
    return _descale(np.stack([t10 + t0, t10 - t0], axis=-1), shift)


def idct_scaled(blocks, ss):
    """(.., 8, 8) dequantised coefficients (int32, natural order) -> ((.., ss, ss) uint8 samples, (min, max) of the pre-limit results)"""
    if ss == 8:
        return X.idct_islow(blocks)
    b = np.asarray(blocks, dtype=I32)
    with np.errstate(over="ignore"):
        if ss == 4:
            x = _pass4(_pass4(b.swapaxes(-1, -2), 12).swapaxes(-1, -2), 19)
        elif ss == 2:
            x = _pass2(_pass2(b.swapaxes(-1, -2), 13).swapaxes(-1, -2), 20)
        else:
            x = _descale(b[..., :1, :1], 3)
    return X.range_limit(x), (int(x.min()), int(x.max())) if x.size else (0, 0)


def planes_of(dec, s):
    """dec: decode_any's dict -> ([Y, Cb, Cr] uint8 at their own scaled extents, (min, max) of the pre-limit results over the MCU grid)"""
    out, lo, hi = [], 0, 0
    sizes = component_sizes(dec["sampling"], s)
    for c, (arr, (rows, cols)) in enumerate(zip(dec["coefs"], own_extents(dec["width"], dec["height"], dec["sampling"], s))):
        ss = sizes[c]
        qz = np.asarray(dec["quant"][dec["quant_ids"][c]], dtype=np.int64)
        nat = np.zeros(arr.shape, dtype=np.int64)
        nat[..., _ZIGZAG] = np.asarray(arr, dtype=np.int64) * qz
        nat = ((nat + (1 << 31)) % (1 << 32) - (1 << 31)).astype(I32)
        pix, (a, b) = idct_scaled(nat.reshape(arr.shape[0], arr.shape[1], 8, 8), ss)
        lo, hi = min(lo, a), max(hi, b)
        out.append(np.ascontiguousarray(pix.transpose(0, 2, 1, 3).reshape(arr.shape[0] * ss, arr.shape[1] * ss)[:rows, :cols]))
    return out, (lo, hi)


def upsample(p, kind, w, h):
    """one chroma plane at its own scaled extent -> h x w"""
    if kind == UP_NONE:
        return p[:h, :w]
    if kind == UP_H2V1_FANCY:
        return X.upsample(p, 2, 1, w, h)
    if kind == UP_H1V2_FANCY:
        return X.upsample(p, 1, 2, w, h)
    return np.repeat(p, 2, axis=1 if kind == UP_H2V1_REPLICATE else 0)[:h, :w]


def twin_scaled_dec(dec, s):
    """as exact_util.twin_dec, at scale s, plus sizes (the IDCT size per component) and up (the UP_* kind)"""
    if s == 1:
        t = dict(X.twin_dec(dec))
        t.update(sizes=component_sizes(dec["sampling"], 1), up=None, scale=1)
        return t
    planes, rng = planes_of(dec, s)
    w, h = scaled_size(dec["width"], dec["height"], s)
    sizes = component_sizes(dec["sampling"], s)
    assert planes[0].shape == (h, w)
    if len(planes) == 1:
        return dict(planes=planes, ycc=planes[0], rgb=np.repeat(planes[0][..., None], 3, axis=-1), gray=planes[0], range=rng, sizes=sizes, up=UP_NONE, scale=s)
    kind = upsampling_kind(dec["width"], dec["height"], dec["sampling"], s)
    cb, cr = upsample(planes[1], kind, w, h), upsample(planes[2], kind, w, h)
    return dict(planes=planes, ycc=np.stack([planes[0], cb, cr], axis=-1), rgb=X.colour(planes[0], cb, cr), gray=planes[0], range=rng, sizes=sizes, up=kind, scale=s)


@functools.lru_cache(maxsize=None)
def twin_scaled(jpeg, s):
    return twin_scaled_dec(R.decode_any(jpeg), s)


def draft_scale(w, h, rw, rh):
    """Pillow's choice: the largest of 8, 4, 2, 1 that does not exceed min(W // rw, H // rh)"""
    k = min(w // rw, h // rh)
    return 8 if k >= 8 else 4 if k >= 4 else 2 if k >= 2 else 1


def forcible(w, h, s):
    """Pillow can be made to decode a w x h file at scale s"""
    return w >= s and h >= s


def pillow_scaled(jpeg, s, mode="RGB"):
    """Pillow's decode at scale s through draft(): "RGB" (draft, then convert), "L" (the Y plane), "YCbCr" (the upsampled planes)"""
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    w, h = im.size
    assert forcible(w, h, s)
    im.draft("RGB" if mode == "RGB" and im.mode != "L" else ("L" if im.mode == "L" else mode), (max(1, w // s), max(1, h // s)))
    assert im.decoderconfig[0] == s, (im.decoderconfig, s)
    assert im.size == scaled_size(w, h, s)
    if mode == "RGB":
        return np.asarray(im.convert("RGB"))
    assert im.mode == mode or (mode == "YCbCr" and im.mode == "L")
    return np.asarray(im)


# ---- files ------------------------------------------------------------------------------------------------------------------------
SIZES = X.SIZES + ((3, 3), (4, 4), (5, 6), (9, 9), (16, 16), (24, 40), (31, 65), (100, 37))
WIDE = ((345, 9), (530, 9))                                             # more than one tile a row in every layout at every scale
QUALITIES = (30, 95)


@functools.lru_cache(maxsize=None)
def pillow_file(w, h, sampling, q, kind="baseline"):
    """Pillow's file of encode_util.picture("noise", ..), written in one piece however wide it is"""
    from PIL import Image, ImageFile
    img = E.picture("noise", w, h, sampling)
    im = Image.fromarray(img) if sampling == "gray" else Image.fromarray(np.ascontiguousarray(img[..., :3]))
    kw = {} if sampling == "gray" else dict(subsampling=E.PILLOW_SUBSAMPLING[sampling])
    kw.update(dict(optimize=True) if kind == "optimize" else dict(progressive=True) if kind == "progressive" else {})
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 1 << 22)
    try:
        b = io.BytesIO()
        im.save(b, "JPEG", quality=q, **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def files(sampling):
    """[(name, jpeg, (w, h))]: 17 sizes x 2 qualities, the two wide sizes and a file of dense blocks of one layout; 4:4:0 from the suite's own writer"""
    out = []
    for i, (w, h) in enumerate(SIZES + WIDE):
        for q in QUALITIES if (w, h) not in WIDE else (QUALITIES[i % 2],):
            if sampling == "4:4:0":
                out.append(("written_%dx%d_q%d" % (w, h, q), X.written_file(w, h, sampling, q), (w, h)))
            else:
                kind = ("baseline", "progressive", "optimize")[(i + q) % 3] if (w, h) not in WIDE else ("baseline", "optimize")[i % 2]
                out.append(("%s_%dx%d_q%d" % (kind, w, h, q), pillow_file(w, h, sampling, q, kind), (w, h)))
    out.append(("dense60", X.written_file(33, 31, sampling, 0, amplitude=60), (33, 31)))     # (dense blocks: both clamps of the range limit)
    return out


def grid(sampling):
    """the files of files() the front end takes (it refuses files under 256 bytes, as the reference does)"""
    return [(name, f, wh) for name, f, wh in files(sampling) if len(f) >= 256]


def rgba(t, gray=False):
    return X.rgba(t, gray)
