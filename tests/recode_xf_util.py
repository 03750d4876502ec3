"""The numpy twin of the lossless flip, rotate, transpose and MCU crop (jda_recode_images_ex), shared by
tests/test_recode_xf_cpu.py (the stages lane by lane on the CPU) and tests/test_gpu_recode_xf.py.

Per component the coefficients are a grid C[by, bx, v, u] over the whole MCU grid (v: vertical frequency, u: horizontal):
    FLIP_H      C[:, ::-1] * (-1)^u            FLIP_V      C[::-1] * (-1)^v            TRANSPOSE   C.transpose(1, 0, 3, 2)
    ROT_90      TRANSPOSE then FLIP_H          ROT_270     TRANSPOSE then FLIP_V       ROT_180     FLIP_H then FLIP_V
    TRANSVERSE  TRANSPOSE then ROT_180
The transposing operations swap width and height and transpose every quantiser; the crop ({x, y, w, h} in source MCUs) comes first; a
mirrored source axis must be a whole number of MCUs, or is trimmed to one.  twin() works on what the suite's own decoders give
(coef_jpeg.decode_coefs / prog_jpeg.decode_coefs) and returns coef_jpeg.write_jpeg's arguments: it shares no code with the library.
The reference of a whole file is recode(write_jpeg(twin(decode(src)))): the plain recode (held to Pillow by
tests/test_recode_cpu.py) of the twin-written file."""
import functools
import io

import numpy as np

from jpegdec_amd.synth import _ZIGZAG
from tests import coef_jpeg
from tests import recode_util as U

OPS = ("none", "flip_h", "flip_v", "transpose", "transverse", "rot90", "rot180", "rot270")
OP_ID = {"none": 0, "flip_h": 1, "flip_v": 2, "transpose": 3, "transverse": 4, "rot90": 5, "rot180": 6, "rot270": 7, "exif": 8}
TRANSPOSING = ("transpose", "transverse", "rot90", "rot270")
MIRRORED = {"none": "", "flip_h": "x", "flip_v": "y", "transpose": "", "transverse": "xy", "rot90": "y", "rot180": "xy", "rot270": "x"}      # SOURCE axes
EXIF_OP = {0: "none", 1: "none", 2: "flip_h", 3: "rot180", 4: "flip_v", 5: "transpose", 6: "rot90", 7: "transverse", 8: "rot270"}
TRIM = 1
_ZZ = np.array(_ZIGZAG)


class Refused(Exception):
    """the job gets JDA_UNSUPPORTED_FEATURE"""


def _flip_h(c):
    return c[:, ::-1] * np.where(np.arange(8) % 2, -1, 1)[None, None, None, :]


def _flip_v(c):
    return c[::-1] * np.where(np.arange(8) % 2, -1, 1)[None, None, :, None]


def _transpose(c):
    return c.transpose(1, 0, 3, 2)


_STEPS = {"none": (), "flip_h": (_flip_h,), "flip_v": (_flip_v,), "transpose": (_transpose,), "rot90": (_transpose, _flip_h), "rot270": (_transpose, _flip_v),
          "rot180": (_flip_h, _flip_v), "transverse": (_transpose, _flip_h, _flip_v)}


def to_grid(zz):
    """(rows, columns, 64) zig-zag -> C[by, bx, v, u]"""
    nat = np.zeros_like(zz)
    nat[..., _ZZ] = zz
    return nat.reshape(zz.shape[0], zz.shape[1], 8, 8)


def from_grid(c):
    return np.ascontiguousarray(c).reshape(c.shape[0], c.shape[1], 64)[..., _ZZ]


def pixel_turn(a, op):
    """the picture the operation makes of picture a (numpy, rows first)"""
    for step in _STEPS[op]:
        a = a[:, ::-1] if step is _flip_h else a[::-1] if step is _flip_v else a.swapaxes(0, 1)
    return np.ascontiguousarray(a)


def shape_of(width, height, sampling, op, rect=None, trim=False):
    """((x, y, w, h) the region in MCUs that is kept, (width, height) of the target) -- or Refused"""
    cx, cy, _, (hs, vs) = coef_jpeg.geometry(width, height, sampling)
    mw, mh = 8 * hs, 8 * vs
    x, y, w, h = rect if rect is not None and any(rect) else (0, 0, cx, cy)
    assert w > 0 and h > 0 and x + w <= cx and y + h <= cy
    pw, ph = min(w * mw, width - x * mw), min(h * mh, height - y * mh)
    if op in TRANSPOSING and hs != vs:
        raise Refused("4:2:2 would become 4:4:0")
    if "x" in MIRRORED[op] and pw % mw:
        if not trim or w == 1:
            raise Refused("a ragged mirrored axis")
        w, pw = w - 1, (w - 1) * mw
    if "y" in MIRRORED[op] and ph % mh:
        if not trim or h == 1:
            raise Refused("a ragged mirrored axis")
        h, ph = h - 1, (h - 1) * mh
    return (x, y, w, h), ((ph, pw) if op in TRANSPOSING else (pw, ph))


def twin(dec, op, rect=None, trim=False):
    """write_jpeg's arguments for the file the operation makes of a decoded file (dict of decode_coefs) -- or Refused"""
    sampling = dec["sampling"]
    (x, y, w, h), (tw, th) = shape_of(dec["width"], dec["height"], sampling, op, rect, trim)
    hs, vs = coef_jpeg.LUMA_HV[sampling]
    coefs = []
    for c, zz in enumerate(dec["coefs"]):
        fh, fv = (hs, vs) if c == 0 else (1, 1)
        g = to_grid(np.asarray(zz))[y * fv:(y + h) * fv, x * fh:(x + w) * fh]
        for step in _STEPS[op]:
            g = step(g)
        coefs.append(from_grid(g).astype(np.int64))
    quant = {}
    for i, q in dec["quant"].items():
        q = np.asarray(list(q))
        quant[i] = [int(v) for v in (from_grid(_transpose(to_grid(q.reshape(1, 1, 64))))[0, 0] if op in TRANSPOSING else q)]
    return dict(width=tw, height=th, sampling=sampling, coefs=coefs, quant=quant, quant_ids=list(dec["quant_ids"]), restart_interval=dec.get("restart_interval", 0))


@functools.lru_cache(maxsize=None)
def twin_file(src, op, rect=None, trim=False):
    """write_jpeg(twin(decode(src))): a baseline file under the Annex K tables with the source's restart interval -- or None where the job is refused"""
    try:
        return coef_jpeg.write_jpeg(**twin(U.decode_any(src), op, rect, trim))
    except Refused:
        return None


def xform(op="none", rect=None, trim=False):
    """(op id, flags, x, y, w, h): a jda_recode_xform's six words"""
    return (OP_ID[op] if isinstance(op, str) else op, TRIM if trim else 0) + tuple(rect if rect is not None else (0, 0, 0, 0))


# ---- pictures constant per MCU cell: their files carry DC values only, so Pillow's file of the turned picture is the turned file -----------
def cell_picture(sampling, cells_x=5, cells_y=3, seed=1):
    """(H, W) or (H, W, 3) uint8, one random colour an MCU cell"""
    hs, vs = coef_jpeg.LUMA_HV[sampling]
    rng = np.random.default_rng(seed)
    cells = rng.integers(16, 240, (cells_y, cells_x) if sampling == "gray" else (cells_y, cells_x, 3)).astype(np.uint8)
    return np.repeat(np.repeat(cells, 8 * vs, axis=0), 8 * hs, axis=1)


def pillow_save(a, sampling, q=75, exif_orientation=None, **extra):
    from PIL import Image
    from tests import encode_util as E
    im = Image.fromarray(np.ascontiguousarray(a))
    kw = {} if sampling == "gray" else dict(subsampling=E.PILLOW_SUBSAMPLING[sampling])
    if exif_orientation is not None:
        ex = Image.Exif()
        ex[274] = exif_orientation
        kw["exif"] = ex.tobytes()
    b = io.BytesIO()
    im.save(b, "JPEG", quality=q, **kw, **extra)
    return b.getvalue()


def strip_app1(jpeg):
    """the file without its APP1 segments (Pillow writes the EXIF block there; a recode carries no APPn segment over)"""
    out, i = bytearray(jpeg[:2]), 2
    while jpeg[i + 1] != 0xDA:
        n = 2 + int.from_bytes(jpeg[i + 2:i + 4], "big")
        if jpeg[i + 1] != 0xE1:
            out += jpeg[i:i + n]
        i += n
    return bytes(out + jpeg[i:])
