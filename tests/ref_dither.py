"""The unmodified reference's decodeDither, driven through ctypes (test helper).

oracle/_ref/libjpegdec_ref_scalar.so is the whole reference class compiled with default visibility.  The class is one JPEGIMAGE
with no virtual functions (reference src/JPEGDEC.h:249-287), so a zeroed buffer of ref_sizeof_state() bytes serves as `this` for
its exported member functions.  The draw callback records the six JPEGDRAW fields and copies iHeight rows of
(iWidth * iBpp + 7) / 8 bytes from pPixels: what a display driver would be given.

Also here: the cases the dither tests share, and the digest both the live reference and the product's output are reduced to."""
import ctypes as C
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SCALAR = os.path.join(ROOT, "oracle", "_ref", "libjpegdec_ref_scalar.so")
REF_SSE2 = os.path.join(ROOT, "oracle", "_ref", "libjpegdec_ref_sse2.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dither", "dither_golden.json")

FOUR_BIT, TWO_BIT, ONE_BIT = 4, 5, 6
DITHER_TYPES = (FOUR_BIT, TWO_BIT, ONE_BIT)
BITS = {FOUR_BIT: 4, TWO_BIT: 2, ONE_BIT: 1}
SCALES = (0, 2, 4, 8)

# mangled names as `nm -D` lists them
_SYM = {
    "openFLASH": "_ZN7JPEGDEC9openFLASHEPKhiPFiP13jpeg_draw_tagE",
    "setPixelType": "_ZN7JPEGDEC12setPixelTypeEi",
    "setUserPointer": "_ZN7JPEGDEC14setUserPointerEPv",
    "setFramebuffer": "_ZN7JPEGDEC14setFramebufferEPv",
    "setCropArea": "_ZN7JPEGDEC11setCropAreaEiiii",
    "decodeDitherXY": "_ZN7JPEGDEC12decodeDitherEiiPhi",
    "decodeDither": "_ZN7JPEGDEC12decodeDitherEPhi",
    "getLastError": "_ZN7JPEGDEC12getLastErrorEv",
    "close": "_ZN7JPEGDEC5closeEv",
}


class JPEGDRAW(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("iWidth", C.c_int), ("iHeight", C.c_int), ("iWidthUsed", C.c_int), ("iBpp", C.c_int),
                ("pPixels", C.c_void_p), ("pUser", C.c_void_p)]


DRAW_CB = C.CFUNCTYPE(C.c_int, C.POINTER(JPEGDRAW))


def available(path=REF_SCALAR):
    return os.path.exists(path)


def recorder(log, strips, stop_after=None, user_seen=None):
    """A draw callback that appends (x, y, iWidth, iHeight, iWidthUsed, iBpp) to log and the strip's packed rows to strips."""
    def cb(p):
        d = p.contents
        log.append((d.x, d.y, d.iWidth, d.iHeight, d.iWidthUsed, d.iBpp))
        n = ((d.iWidth * d.iBpp + 7) // 8) * max(d.iHeight, 0)
        strips.append(C.string_at(d.pPixels, n) if n else b"")
        if user_seen is not None:
            user_seen.append(d.pUser)
        return 0 if (stop_after is not None and len(log) >= stop_after) else 1
    return DRAW_CB(cb)


def digest(log, strips):
    h = hashlib.sha256()
    for s in strips:
        h.update(s)
    return {"draws": [list(d) for d in log], "sha256": h.hexdigest(), "bytes": sum(len(s) for s in strips)}


def ref_decode_dither(jpeg, pixel_type, options=0, xy=None, stop_after=None, lib_path=REF_SCALAR, crop=None, product=False,
                      framebuffer=False, null_buffer=False, decode_instead=False):
    """-> (rc, last error, draw log, strips) of decodeDither: the reference's (lib_path: a build of it under oracle/_ref), or -- product --
    the drop-in class's, from a library that holds it (the product library, or the class's CPU build): the same exported member
    functions, on an object made by the class's own constructor."""
    lib = C.CDLL(lib_path)
    fn = {k: getattr(lib, v) for k, v in _SYM.items()}
    for f in fn.values():
        f.restype = C.c_int
    fn["openFLASH"].argtypes = [C.c_void_p, C.c_char_p, C.c_int, DRAW_CB]
    fn["setPixelType"].argtypes = [C.c_void_p, C.c_int]
    fn["setCropArea"].argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    fn["decodeDitherXY"].argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    fn["decodeDither"].argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    fn["getLastError"].argtypes = [C.c_void_p]
    fn["close"].argtypes = [C.c_void_p]
    fn["close"].restype = None
    fn["setPixelType"].restype = None
    fn["setCropArea"].restype = None
    fn["setFramebuffer"].argtypes = [C.c_void_p, C.c_void_p]
    fn["setFramebuffer"].restype = None
    if product:
        this = C.create_string_buffer(256)
        ctor, dtor = lib._ZN7JPEGDECC1Ev, lib._ZN7JPEGDECD1Ev
        ctor.argtypes = dtor.argtypes = [C.c_void_p]
        ctor.restype = dtor.restype = None
        ctor(this)
        decode = lib._ZN7JPEGDEC6decodeEiii
        decode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        decode.restype = C.c_int
    else:
        lib.ref_sizeof_state.restype = C.c_int
        this = C.create_string_buffer(int(lib.ref_sizeof_state()) + 64)
    log, strips = [], []
    cb = recorder(log, strips, stop_after)
    src = C.create_string_buffer(bytes(jpeg), len(jpeg) + 64)
    if not fn["openFLASH"](this, C.cast(src, C.c_char_p), len(jpeg), cb):
        err = int(fn["getLastError"](this))
        if product:
            dtor(this)
        return 0, err, log, strips
    fn["setPixelType"](this, pixel_type)
    if crop is not None:
        fn["setCropArea"](this, *crop)
    # room for one MCU row of the padded canvas at full size (16 rows x (width + 15)), and slack
    w = int.from_bytes(_sof_dims(jpeg)[1], "big")
    buf = C.create_string_buffer((w + 32) * 16 + 4096)
    fb = C.create_string_buffer(64)
    if framebuffer:
        fn["setFramebuffer"](this, fb)
    target = None if null_buffer else buf
    if decode_instead:                                  # (product only: the reference dereferences a null dither buffer here)
        assert product
        rc = decode(this, 0, 0, options)
    elif xy is None:
        rc = fn["decodeDither"](this, target, options)
    else:
        rc = fn["decodeDitherXY"](this, xy[0], xy[1], target, options)
    err = int(fn["getLastError"](this))
    fn["close"](this)
    if product:
        dtor(this)
    return int(rc), err, log, strips


def _sof_dims(jpeg):
    """(height bytes, width bytes) of the first SOF0 / SOF1 / SOF2 marker."""
    i = 2
    while i + 9 < len(jpeg):
        if jpeg[i] != 0xFF:
            i += 1
            continue
        m = jpeg[i + 1]
        if m in (0xC0, 0xC1, 0xC2):
            return jpeg[i + 5:i + 7], jpeg[i + 7:i + 9]
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7 or m == 0xFF:
            i += 2 if m != 0xFF else 1
            continue
        i += 2 + int.from_bytes(jpeg[i + 2:i + 4], "big")
    raise ValueError("no SOF marker")


def strips_from_packed(packed, pitch, canvas_h, strip_rows):
    """A canvas of packed rows (numpy uint8, canvas_h x >= pitch) cut into the MCU-row strips a draw callback is handed."""
    out = []
    for y in range(0, canvas_h, strip_rows):
        out.append(np.ascontiguousarray(packed[y:y + strip_rows, :pitch]).tobytes())
    return out


def clip_strips(strips, log):
    """The rows a callback may read: iHeight of them (the last strip of an image is trimmed)."""
    out = []
    for s, d in zip(strips, log):
        pitch = (d[2] * d[5] + 7) // 8
        out.append(s[: pitch * d[3]])
    return out


def case_key(name, pixel_type, options):
    return "%s:%d:%d" % (name, pixel_type, options)


# ---- the cases (names of tests/cases.py, the reference's own fixtures under tests/golden/ref, canvases made for this under tests/golden/dither)
SYNTH_DITHER = ("gray_333x217", "c444_333x217", "c422_333x217", "c440_200x120", "c420_333x217")
RESTART_DITHER = ("gray_64x64_rst3", "c420_640x368_rstrow", "c440_300x64_rst5")
PROGRESSIVE_DITHER = ("pgray_100x100",)
PROGRESSIVE_SCALES = (0, 2, 8)             # (1/4 of a progressive file is refused, as for every pixel type: DESIGN.md 3)
REF_FIXTURE_MODES = {                      # fixture -> (pixel type, options) recorded
    "squirrel_dither": ((ONE_BIT, 0), (FOUR_BIT, 0), (TWO_BIT, 2), (ONE_BIT, 4), (FOUR_BIT, 8)),
    "demo": tuple((pt, o) for pt in DITHER_TYPES for o in SCALES),
    "perf": tuple((pt, o) for pt in DITHER_TYPES for o in SCALES),
    "croptest": tuple((pt, o) for pt in DITHER_TYPES for o in SCALES),
    "tulips": ((ONE_BIT, 0), (TWO_BIT, 2), (FOUR_BIT, 4)),
}
# canvases the host simulator is held to, full size: padded widths 8, 16, 64, 72, 336, 4096; heights that are and are not multiples of 64
SIM_JPEGS = {
    "d_gray_8x8": dict(width=8, height=8, subsampling="gray", seed=71),
    "d_gray_16x130": dict(width=16, height=130, subsampling="gray", seed=72),
    "d_gray_64x64": dict(width=64, height=64, subsampling="gray", seed=73),
    "d_gray_72x128": dict(width=72, height=128, subsampling="gray", seed=74),
    "d_c420_330x200": dict(width=330, height=200, subsampling="4:2:0", seed=77),
    "d_gray_4096x80": dict(width=4096, height=80, subsampling="gray", seed=75),
    "d_c420_4090x144": dict(width=4090, height=144, subsampling="4:2:0", seed=76),
}
NO_REFERENCE_JPEGS = {                     # padded width above the reference's 4096-pixel error row: the product against its twin only
    "d_gray_4112x72": dict(width=4112, height=72, subsampling="gray", seed=78),
}
DITHER_DIR = os.path.join(ROOT, "tests", "golden", "dither")


def dither_jpeg(name):
    return open(os.path.join(DITHER_DIR, name + ".jpg"), "rb").read()


def any_jpeg(name):
    if name in SIM_JPEGS or name in NO_REFERENCE_JPEGS:
        return dither_jpeg(name)
    if name in REF_FIXTURE_MODES:
        from tests.ref_fixtures import ref_jpeg
        return ref_jpeg(name)
    from tests.cases import jpeg_for
    return jpeg_for(name)


JPEG_EXIF_THUMBNAIL, JPEG_USES_DMA = 32, 128


def exif_thumbnail_jpeg():
    """A colour image with its own (optimised) Huffman tables that carries a gray thumbnail with other tables: decodeDither with
    JPEG_EXIF_THUMBNAIL dithers the thumbnail on an error row that starts from BOTH files' DHT contents."""
    from tests.cases import jpeg_for
    from tests.exif_util import with_exif_thumbnail
    return with_exif_thumbnail(jpeg_for("c444_256x256_q100_opt"), dither_jpeg("d_gray_72x128"), 72, 128)


def recorded_cases():
    """(name, pixel type, options) of every case with a recorded digest."""
    out = []
    for n in SYNTH_DITHER + RESTART_DITHER:
        out += [(n, pt, o) for pt in DITHER_TYPES for o in SCALES]
    for n in PROGRESSIVE_DITHER:
        out += [(n, pt, o) for pt in DITHER_TYPES for o in PROGRESSIVE_SCALES]
    for n, modes in REF_FIXTURE_MODES.items():
        out += [(n, pt, o) for pt, o in modes]
    for n in SIM_JPEGS:
        out += [(n, pt, 0) for pt in DITHER_TYPES]
    return out


_golden = None


def golden():
    global _golden
    if _golden is None:
        import json
        _golden = json.load(open(GOLDEN))
    return _golden
