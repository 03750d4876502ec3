"""Helpers of the orientation tests (JPEG_AUTO_ROTATE): the table of include/jpegdec_amd.h as numpy expressions, files that carry an
EXIF orientation, and the drop-in class's decode() driven through ctypes with a recording draw callback."""
import ctypes as C
import struct

import numpy as np

from tests.ref_dither import DRAW_CB, JPEGDRAW  # noqa: F401  (the JPEGDRAW layout)

AUTO_ROTATE = 1
ORIENTATIONS = tuple(range(9))
SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 130, 333)

# dst = f(a), a = the source as (H, W, bytes per pixel)
NUMPY = {
    0: lambda a: a,
    1: lambda a: a,
    2: lambda a: a[:, ::-1],
    3: lambda a: a[::-1, ::-1],
    4: lambda a: a[::-1],
    5: lambda a: a.swapaxes(0, 1),
    6: lambda a: np.rot90(a, -1),
    7: lambda a: a[::-1, ::-1].swapaxes(0, 1),
    8: lambda a: np.rot90(a, 1),
}
# Pillow's Image.transpose methods, as exif_transpose picks them (FLIP_LEFT_RIGHT .. ROTATE_90)
PILLOW = {2: 0, 3: 3, 4: 1, 5: 5, 6: 4, 7: 6, 8: 2}


def oriented(rows, width, bpp, o):
    """rows: (H, >= width * bpp) uint8 -> the oriented visible rectangle as (H', W' * bpp); o outside 2..8: as it is."""
    h = rows.shape[0]
    a = np.ascontiguousarray(rows[:, :width * bpp]).reshape(h, width, bpp)
    t = np.ascontiguousarray(NUMPY.get(o, NUMPY[0])(a))
    return t.reshape(t.shape[0], t.shape[1] * bpp)


def with_orientation(jpeg: bytes, o: int, big_endian: bool = False) -> bytes:
    """The file with an APP1 in front that holds one IFD with the single tag 274 (orientation, SHORT) = o."""
    e = ">" if big_endian else "<"
    tiff = (b"MM" if big_endian else b"II") + struct.pack(e + "HI", 42, 8)
    tiff += struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", 274, 3, 1, o, 0) + struct.pack(e + "I", 0)
    app1 = b"Exif\x00\x00" + tiff
    assert jpeg[:2] == b"\xff\xd8"
    return b"\xff\xd8\xff\xe1" + struct.pack(">H", len(app1) + 2) + app1 + jpeg[2:]


_bad = {}


def bad_mcu_jpeg(name="c420_333x217"):
    """A copy of the file with a few scan bytes changed so that the pre-scan meets a bad MCU in the middle of the image while the stream
    still has data (a stream that runs out of data is outside the contract) -> (jpeg, MCUs in front of the bad one)."""
    if name not in _bad:
        import jpegdec_amd as J
        from tests.cases import jpeg_for
        base = jpeg_for(name)
        sos = base.index(b"\xff\xda")
        rng = np.random.default_rng(11)
        while name not in _bad:
            b = bytearray(base)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(sos + 14, len(b) - 2))] = int(rng.integers(0, 256))
            try:
                p = J.PreparedImage(bytes(b))
            except J.JdaError:
                continue
            idx, nok = p.block_index()
            ran_out = (int(idx[-1]) >> 7) + ((int(idx[-1]) & 127) + 7) // 8 > len(p.scan())
            if not ran_out and p.n_mcus // 4 < nok < p.n_mcus * 3 // 4:
                _bad[name] = (bytes(b), nok)
            p.close()
    return _bad[name]


def zero_undecoded(canvas, info, mcus_decoded):
    """The product's canvas of a stream with a bad MCU: the MCUs from the bad one on are zeros (canvas: the oracle's, MCU-padded)."""
    out = canvas.copy()
    mx, my = info["mcus_x"], info["mcus_y"]
    mw, mh = out.shape[1] // mx, out.shape[0] // my      # (bytes x rows of an MCU)
    for m in range(mcus_decoded, mx * my):
        out[(m // mx) * mh:(m // mx + 1) * mh, (m % mx) * mw:(m % mx + 1) * mw] = 0
    return out


_SYM = {
    "ctor": "_ZN7JPEGDECC1Ev", "dtor": "_ZN7JPEGDECD1Ev",
    "openFLASH": "_ZN7JPEGDEC9openFLASHEPKhiPFiP13jpeg_draw_tagE",
    "setPixelType": "_ZN7JPEGDEC12setPixelTypeEi", "setFramebuffer": "_ZN7JPEGDEC14setFramebufferEPv",
    "setCropArea": "_ZN7JPEGDEC11setCropAreaEiiii", "setMaxOutputSize": "_ZN7JPEGDEC16setMaxOutputSizeEi",
    "decode": "_ZN7JPEGDEC6decodeEiii", "getLastError": "_ZN7JPEGDEC12getLastErrorEv", "close": "_ZN7JPEGDEC5closeEv",
    "getWidth": "_ZN7JPEGDEC8getWidthEv", "getHeight": "_ZN7JPEGDEC9getHeightEv", "getOrientation": "_ZN7JPEGDEC14getOrientationEv",
}


def class_decode(lib_path, jpeg, pixel_type, options, px_bytes, framebuffer=None, xy=(0, 0), stop_after=None, crop=None, max_mcus=None):
    """JPEGDEC::decode of the drop-in class in lib_path (the product library or the class's CPU build).  px_bytes: bytes of a pixel in the
    strips (jda_output_geometry).  framebuffer: None (callback mode) or a writable uint8 array.  -> dict(rc, err, log, strips, getters)."""
    lib = C.CDLL(lib_path)
    fn = {k: getattr(lib, v) for k, v in _SYM.items()}
    for f in fn.values():
        f.restype = C.c_int
    for k in ("ctor", "dtor", "close", "setPixelType", "setFramebuffer", "setCropArea", "setMaxOutputSize"):
        fn[k].restype = None
    for k in ("ctor", "dtor", "close", "getLastError", "getWidth", "getHeight", "getOrientation"):
        fn[k].argtypes = [C.c_void_p]
    fn["openFLASH"].argtypes = [C.c_void_p, C.c_char_p, C.c_int, DRAW_CB]
    fn["setPixelType"].argtypes = fn["setMaxOutputSize"].argtypes = [C.c_void_p, C.c_int]
    fn["setFramebuffer"].argtypes = [C.c_void_p, C.c_void_p]
    fn["setCropArea"].argtypes = [C.c_void_p] + [C.c_int] * 4
    fn["decode"].argtypes = [C.c_void_p] + [C.c_int] * 3
    log, strips = [], []

    def cb(p):
        d = p.contents
        log.append((d.x, d.y, d.iWidth, d.iHeight, d.iWidthUsed, d.iBpp))
        n = d.iWidth * px_bytes * max(d.iHeight, 0)
        strips.append(C.string_at(d.pPixels, n) if n > 0 else b"")
        return 0 if (stop_after is not None and len(log) >= stop_after) else 1
    keep = DRAW_CB(cb)
    this = C.create_string_buffer(256)
    fn["ctor"](this)
    src = C.create_string_buffer(bytes(jpeg), len(jpeg) + 64)
    out = dict(rc=0, log=log, strips=strips)
    if fn["openFLASH"](this, C.cast(src, C.c_char_p), len(jpeg), keep):
        fn["setPixelType"](this, pixel_type)
        if max_mcus is not None:
            fn["setMaxOutputSize"](this, max_mcus)
        if crop is not None:
            fn["setCropArea"](this, *crop)
        if framebuffer is not None:
            fn["setFramebuffer"](this, framebuffer.ctypes.data_as(C.c_void_p))
        out["rc"] = int(fn["decode"](this, xy[0], xy[1], options))
        out["getters"] = (int(fn["getWidth"](this)), int(fn["getHeight"](this)), int(fn["getOrientation"](this)))
    out["err"] = int(fn["getLastError"](this))
    fn["close"](this)
    fn["dtor"](this)
    return out


def strips_of(pixels, strip_rows):
    """An oriented image (H' x W' * bpp) cut into the strips the class hands to a draw callback."""
    return [np.ascontiguousarray(pixels[y:y + strip_rows]).tobytes() for y in range(0, pixels.shape[0], strip_rows)]
