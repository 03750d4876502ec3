"""The colour models of the libjpeg-exact decode (JDA_EXACT_COLOUR_MODELS) stated once more in numpy, and the files its
tests decode: Adobe APP14 files, RGB-coded three-component files, CMYK and YCCK.

The rules are libjpeg's and Pillow's, each restated here and held to Pillow itself by tests/test_exact_adobe_cpu.py:
  model()      jdapimin.c's default_decompress_parms: which colour model a header gets
  twin4()      a four-component file: every component through exact_util's islow IDCT with its own raw quantiser, fancy upsampling over its
               own extent, then CMYK (Pillow's "CMYK;I": every byte inverted) or YCCK (jdcolor.c's YCbCr -> RGB on components 0..2, libjpeg
               emits 255 - R, G, B and passes K; inverted again by Pillow) and Pillow's convert("RGB") (Convert.c's cmyk2rgb)
  twin3()      a three-component file: exact_util's / exact_scaled_util's twin, the upsampled planes taken as R, G, B where the model says so
Coefficients come from decode4(), an entropy decoder of this suite for any component count and sampling (sequential scans here, progressive
ones through prog_jpeg's scan decoder); it shares no code with the library."""
import functools
import io

import numpy as np

from jpegdec_amd.synth import _ZIGZAG
from tests import coef_jpeg
from tests import encode_util as E
from tests import exact_scaled_util as S
from tests import exact_util as X
from tests import prog_jpeg

GRAY, YCBCR, RGB, CMYK, YCCK = 0, 1, 2, 3, 4
LAYOUT_OF = {(1, 1): 1, (2, 2): 2, (2, 1): 3, (1, 2): 4}              # jda_exact_probe's layout of components 0..2
SAMPLING_OF = {(1, 1): "4:4:4", (2, 2): "4:2:0", (2, 1): "4:2:2", (1, 2): "4:4:0"}


# ---- the header -------------------------------------------------------------------------------------------------------------------
def header(jpeg):
    """dict(ncomp, ids, hv [(h, v)], tq, sof, jfif, adobe, transform, width, height) of the segments in front of the first scan"""
    out = dict(jfif=False, adobe=False, transform=-1)
    for m, off, ln, ent in prog_jpeg._segments(bytes(jpeg)):
        seg = jpeg[off:off + ln]
        if m == 0xE0 and ln >= 14 and seg[:5] == b"JFIF\0":
            out["jfif"] = True
        elif m == 0xEE and ln >= 12 and seg[:5] == b"Adobe":
            out["adobe"], out["transform"] = True, seg[11]
        elif m in (0xC0, 0xC1, 0xC2):
            nc = seg[5]
            out.update(sof=m, height=(seg[1] << 8) | seg[2], width=(seg[3] << 8) | seg[4], ncomp=nc, ids=[seg[6 + 3 * k] for k in range(nc)],
                       hv=[(seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15) for k in range(nc)], tq=[seg[8 + 3 * k] for k in range(nc)])
        elif m == 0xDA:
            break
    return out


def model(jpeg):
    """jdapimin.c: the colour model libjpeg gives the file"""
    h = header(jpeg)
    if h["ncomp"] == 1:
        return GRAY
    if h["ncomp"] == 3:
        if h["jfif"]:
            return YCBCR
        if h["adobe"]:
            return RGB if h["transform"] == 0 else YCBCR
        return RGB if h["ids"] == [0x52, 0x47, 0x42] else YCBCR
    assert h["ncomp"] == 4
    return (CMYK if h["transform"] == 0 else YCCK) if h["adobe"] else CMYK


# ---- the entropy decoder ----------------------------------------------------------------------------------------------------------
def decode4(jpeg):
    """-> dict(width, height, hv, coefs [(block rows, block columns, 64) zig-zag over the MCU-padded grid of each component], quant [the 64
    zig-zag entries latched for each component at the first scan that names it], sof).  Sequential files: any sampling, interleaved scans
    or one a component, restart intervals.  Progressive ones go through prog_jpeg._scan, which wants every component but the first at 1x1."""
    jpeg = bytes(jpeg)
    quant, huff_raw, dri, H = {}, {}, 0, None
    coefs = latched = None
    for m, off, ln, ent in prog_jpeg._segments(jpeg):
        seg = jpeg[off:off + ln]
        if m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                quant[tq] = [(seg[j + 1 + 2 * k] << 8) | seg[j + 2 + 2 * k] for k in range(64)] if pq else list(seg[j + 1:j + 65])
                j += 129 if pq else 65
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                bits = list(seg[j + 1:j + 17])
                huff_raw[(seg[j] >> 4, seg[j] & 15)] = prog_jpeg._lookup(bits, list(seg[j + 17:j + 17 + sum(bits)]))
                j += 17 + sum(bits)
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m in (0xC0, 0xC1, 0xC2):
            H = header(jpeg)
            hmax, vmax = max(h for h, v in H["hv"]), max(v for h, v in H["hv"])
            cx, cy = -(-H["width"] // (8 * hmax)), -(-H["height"] // (8 * vmax))
            coefs = [np.zeros((cy * v, cx * h, 64), dtype=np.int64) for h, v in H["hv"]]
            own = [(-(-(-(-H["height"] * v // vmax)) // 8), -(-(-(-H["width"] * h // hmax)) // 8)) for h, v in H["hv"]]
            latched = [None] * H["ncomp"]
        elif m == 0xDA:
            members = [(H["ids"].index(seg[1 + 2 * k]), seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(seg[0])]
            for c, _, _ in members:
                if latched[c] is None:
                    latched[c] = list(quant[H["tq"][c]])
            if H["sof"] == 0xC2:
                assert all(hv == (1, 1) for hv in H["hv"][1:])
                frame = (H["width"], H["height"], [(i, 0, 0) for i in H["ids"]])
                prog_jpeg._scan(jpeg, seg, ent, frame, (cx, cy, hmax, vmax), own, coefs, huff_raw, dri)
            else:
                _sequential_scan(jpeg[ent[0]:ent[1]], members, H, (cx, cy), own, coefs, huff_raw, dri)
    return dict(width=H["width"], height=H["height"], hv=H["hv"], coefs=coefs, quant=latched, sof=H["sof"])


def _sequential_scan(raw, members, H, grid, own, coefs, huff, dri):
    cx, cy = grid
    pieces, a, j = [], 0, 0
    while j + 1 < len(raw):
        if raw[j] == 0xFF and 0xD0 <= raw[j + 1] <= 0xD7:
            pieces.append(raw[a:j])
            a = j = j + 2
        else:
            j += 2 if raw[j] == 0xFF else 1
    pieces.append(raw[a:])
    if len(members) > 1:
        units = [[(c, my * H["hv"][c][1] + y, mx * H["hv"][c][0] + x) for c, _, _ in members for y in range(H["hv"][c][1]) for x in range(H["hv"][c][0])]
                 for my in range(cy) for mx in range(cx)]
    else:
        c0 = members[0][0]
        units = [[(c0, by, bx)] for by in range(own[c0][0]) for bx in range(own[c0][1])]
    tabs = {c: (td, ta) for c, td, ta in members}
    pred = {c: 0 for c in tabs}
    bits, piece = prog_jpeg._Bits(pieces[0]), 0

    def symbol(key):
        sym, ln = huff[key]
        p = bits.peek16()
        assert ln[p], "invalid code"
        bits.p += ln[p]
        return sym[p]

    for u, unit in enumerate(units):
        if dri and u and u % dri == 0:
            piece += 1
            bits = prog_jpeg._Bits(pieces[piece])
            pred = {c: 0 for c in tabs}
        for c, by, bx in unit:
            blk = coefs[c][by, bx]
            s = symbol((0, tabs[c][0]))
            pred[c] += prog_jpeg._extend(bits.get(s), s)
            blk[0] = pred[c]
            k = 1
            while k < 64:
                rs = symbol((1, tabs[c][1]))
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r != 15:
                        break
                    k += 16
                    continue
                k += r
                assert k <= 63
                blk[k] = prog_jpeg._extend(bits.get(s), s)
                k += 1


def library_blocks(dec):
    """decode4's coefficients as a four-component coefficient image holds them: (components 0..2 as int16 (blocks, 64) in natural order, the
    blocks MCU-interleaved; component 3 the same way, row-major over its own grid)"""
    def nat(a):
        out = np.zeros(a.shape, dtype=np.int64)
        out[..., _ZIGZAG] = a
        return (out.reshape(-1, 64) & 0xFFFF).astype(np.uint16).view(np.int16)
    (hs, vs) = dec["hv"][0]
    cy, cx = dec["coefs"][1].shape[:2]
    per = hs * vs + 2
    mcu = np.zeros((cy, cx, per, 64), dtype=np.int64)
    mcu[:, :, :hs * vs] = dec["coefs"][0].reshape(cy, vs, cx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(cy, cx, hs * vs, 64)
    mcu[:, :, hs * vs] = dec["coefs"][1]
    mcu[:, :, hs * vs + 1] = dec["coefs"][2]
    return nat(mcu), (nat(dec["coefs"][3]) if len(dec["coefs"]) == 4 else None)


# ---- the twins --------------------------------------------------------------------------------------------------------------------
def upsample(p, hs, vs, w, h):
    """exact_util.upsample with jdsample.c's other rule: the fancy h2v1 / h2v2 upsamplers are taken only for a component MORE than two samples
    wide (downsampled_width > 2); a narrower one is replicated, both ways"""
    if hs == 2 and p.shape[1] <= 2:
        return np.repeat(np.repeat(p, 2, axis=1), vs, axis=0)[:h, :w]
    return X.upsample(p, hs, vs, w, h)


def muldiv255(a, b):
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def cmyk2rgb(cmyk):
    """Pillow's convert("RGB") of mode-"CMYK" bytes (Convert.c)"""
    c = cmyk.astype(np.int64)
    nk = 255 - c[..., 3:4]
    return np.clip(nk - muldiv255(c[..., :3], nk), 0, 255).astype(np.uint8)


def twin4_dec(dec, ycck):
    """dict(planes [four, own extents], cmyk (H x W x 4: Pillow's mode-"CMYK" bytes), rgb (H x W x 3), range, raw (H x W x 4: the upsampled
    samples as libjpeg has them in front of the colour stage))"""
    w, h = dec["width"], dec["height"]
    hmax, vmax = dec["hv"][0]
    planes, up, lo, hi = [], [], 0, 0
    for arr, qz, (ch, cv) in zip(dec["coefs"], dec["quant"], dec["hv"]):
        nat = np.zeros(arr.shape, dtype=np.int64)
        nat[..., _ZIGZAG] = np.asarray(arr, dtype=np.int64) * np.asarray(qz, dtype=np.int64)
        nat = ((nat + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32)
        pix, (a, b) = X.idct_islow(nat.reshape(arr.shape[0], arr.shape[1], 8, 8))
        lo, hi = min(lo, a), max(hi, b)
        rows, cols = -(-h * cv // vmax), -(-w * ch // hmax)
        p = np.ascontiguousarray(pix.transpose(0, 2, 1, 3).reshape(arr.shape[0] * 8, arr.shape[1] * 8)[:rows, :cols])
        planes.append(p)
        up.append(upsample(p, hmax // ch, vmax // cv, w, h))
    raw = np.stack(up, axis=-1)
    if ycck:
        cmyk = np.concatenate([X.colour(up[0], up[1], up[2]), (255 - up[3])[..., None]], axis=-1)
    else:
        cmyk = 255 - raw
    return dict(planes=planes, raw=raw, cmyk=cmyk.astype(np.uint8), rgb=cmyk2rgb(cmyk), range=(lo, hi))


@functools.lru_cache(maxsize=None)
def twin4(jpeg):
    return twin4_dec(decode4(jpeg), model(jpeg) == YCCK)


@functools.lru_cache(maxsize=None)
def twin3(jpeg, scale=1):
    """a one- or three-component file at 1 / scale: exact_util's / exact_scaled_util's twin, its rgb the upsampled planes themselves where
    the file is RGB-coded"""
    t = dict(X.twin(jpeg) if scale == 1 else S.twin_scaled(jpeg, scale))
    if model(jpeg) == RGB:
        if scale == 1:                                                   # (the narrow-component rule, which exact_util's twin does not state)
            hs, vs = header(jpeg)["hv"][0]
            h, w = t["planes"][0].shape
            t["ycc"] = np.stack([t["planes"][0]] + [upsample(p, hs, vs, w, h) for p in t["planes"][1:]], axis=-1)
        t["rgb"] = np.ascontiguousarray(t["ycc"])
    return t


def in_window(t):
    return X.WINDOW[0] <= t["range"][0] and t["range"][1] <= X.WINDOW[1]


def surface(t, cmyk=False):
    """the surface the _ex calls write: RGB8888 (A = 0xFF) or CMYK8888 as H x 4W bytes"""
    if cmyk:
        return t["cmyk"].reshape(t["cmyk"].shape[0], -1)
    rgb = t["rgb"]
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=-1).reshape(rgb.shape[0], -1)


def pillow(jpeg, mode=None):
    """Pillow's own bytes (mode "CMYK" for a four-component file), or its convert("RGB")"""
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    return np.asarray(im.convert(mode) if mode else im)


# ---- files ------------------------------------------------------------------------------------------------------------------------
ADOBE = lambda transform: coef_jpeg._seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([transform]))      # noqa: E731
PILLOW_SUB = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def _cut(jpeg, marker):
    """the file without its first segment of that marker"""
    for m, off, ln, ent in prog_jpeg._segments(bytes(jpeg)):
        if m == marker:
            return jpeg[:off - 4] + jpeg[off + ln:]
    raise AssertionError("no such segment")


def _pad(jpeg, to=300):
    """a COM segment behind SOI brings a small file up to the size the front end takes"""
    return jpeg if len(jpeg) >= to else jpeg[:2] + coef_jpeg._seg(0xFE, b"\0" * (to - len(jpeg))) + jpeg[2:]


def _picture4(w, h, seed=3):
    """noise over a ramp, every channel reaching 0 and 255 somewhere: both clamps of the conversions are met"""
    rng = np.random.default_rng(seed + 7 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), 255 - (xx * 255) // max(w - 1, 1), ((xx + yy) * 255) // max(w + h - 2, 1)], axis=-1)
    a = np.clip(base + rng.integers(-40, 41, size=base.shape), 0, 255).astype(np.uint8)
    a[0, 0] = (0, 0, 0, 0)
    a[-1, -1] = (255, 255, 255, 255)
    return a


@functools.lru_cache(maxsize=None)
def pillow_cmyk(w, h, sampling, q, progressive=False, variant="cmyk"):
    """Pillow's own CMYK file (Adobe transform 0, K at 1x1), or the same bytes read another way: variant "ycck" -- the transform byte 2 --,
    "bare" -- the APP14 segment cut out (CMYK again)"""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(_picture4(w, h), "CMYK").save(b, "JPEG", quality=q, subsampling=PILLOW_SUB[sampling], progressive=progressive)
    f = b.getvalue()
    i = f.index(b"Adobe")
    assert f[i + 11] == 0
    if variant == "ycck":
        f = f[:i + 11] + b"\x02" + f[i + 12:]
    elif variant == "bare":
        f = _cut(f, 0xEE)
    else:
        assert variant == "cmyk"
    return _pad(f)


@functools.lru_cache(maxsize=None)
def pillow_rgb3(w, h, sampling, q, variant, progressive=False):
    """a Pillow RGB file (JFIF, YCbCr) with other markers: "adobe0" -- APP0 replaced by an Adobe transform-0 segment (RGB-coded) --, "adobe1" --
    by a transform-1 one (YCbCr, Photoshop's) --, "both" -- JFIF and Adobe transform 0: JFIF wins, YCbCr --, "ids" -- neither marker and the
    component ids 'R', 'G', 'B' in SOF and SOS (RGB-coded) --, "none" -- neither marker, the ids as they were (YCbCr)"""
    from PIL import Image
    if sampling == "4:4:0":                                              # (Pillow writes no 4:4:0: the suite's own baseline writer, the same surgery)
        assert not progressive
        f = X.written_file(w, h, sampling, q)
    else:
        img = E.picture("noise", w, h, sampling)
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img[..., :3])).save(b, "JPEG", quality=q, subsampling=PILLOW_SUB[sampling], progressive=progressive)
        f = b.getvalue()
    assert f[2:4] == b"\xff\xe0" and f[6:11] == b"JFIF\0"
    app0 = 4 + ((f[4] << 8) | f[5])
    if variant == "both":
        f = f[:app0] + ADOBE(0) + f[app0:]
    elif variant in ("adobe0", "adobe1"):
        f = f[:2] + ADOBE(int(variant[-1])) + f[app0:]
    else:
        f = f[:2] + f[app0:]
        if variant == "ids":
            out = bytearray(f)
            for m, off, ln, ent in prog_jpeg._segments(f):
                if m in (0xC0, 0xC2):
                    for k in range(3):
                        assert out[off + 6 + 3 * k] == k + 1
                        out[off + 6 + 3 * k] = b"RGB"[k]
                elif m == 0xDA:
                    for k in range(out[off]):
                        out[off + 1 + 2 * k] = b"RGB"[out[off + 1 + 2 * k] - 1]
            f = bytes(out)
        else:
            assert variant == "none"
    return _pad(f)


RGB3_MODEL = {"adobe0": RGB, "adobe1": YCBCR, "both": YCBCR, "ids": RGB, "none": YCBCR}


@functools.lru_cache(maxsize=None)
def written4(w, h, hv0, k_full, q=90, adobe=0, restart_interval=0, per_component=False, sof1=False, seed=11):
    """a four-component sequential file from a picture's coefficients, written with coef_jpeg's bit writer and tables: component 0 at hv0,
    components 1 and 2 at 1x1, component 3 at hv0 (k_full) or 1x1 -- the layouts Pillow cannot write; adobe: the transform byte (0 CMYK,
    2 YCCK), None: no APP14 segment; one interleaved scan, or a scan per component; an optional restart interval (in MCUs of the
    interleaved scan; in blocks of a component's own scan)"""
    hs, vs = hv0
    hvs = [hv0, (1, 1), (1, 1), hv0 if k_full else (1, 1)]
    cx, cy = -(-w // (8 * hs)), -(-h // (8 * vs))
    pic = _picture4(w, h, seed).astype(np.int64)
    lum, chrom = E.quant_natural(q)
    huff = coef_jpeg.annex_k()[2]
    dc_t = {th: coef_jpeg._codes(*huff[(0, th)]) for th in (0, 1)}
    ac_t = {th: coef_jpeg._codes(*huff[(1, th)]) for th in (0, 1)}
    coefs = []
    for c, (ch, cv) in enumerate(hvs):
        p = pic[..., c]
        fy, fx = vs // cv, hs // ch                                       # box-average down to the component's own extent
        p = np.pad(p, ((0, (-p.shape[0]) % fy), (0, (-p.shape[1]) % fx)), mode="edge")
        p = (p.reshape(p.shape[0] // fy, fy, p.shape[1] // fx, fx).sum(axis=(1, 3)) + fy * fx // 2) // (fy * fx)
        rows, cols = cy * cv, cx * ch
        blocks = E._pad(p, rows * 8, cols * 8).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)
        coefs.append(E.quantise(E.fdct(blocks), (lum if c in (0, 3) else chrom).reshape(8, 8)).reshape(rows, cols, 64)[..., E._ZZ])
    own = [(-(-(-(-h * cv // vs)) // 8), -(-(-(-w * ch // hs)) // 8)) for ch, cv in hvs]
    tabs = [(0, 0), (1, 1), (1, 1), (0, 0)]

    def scan(members):
        bw = coef_jpeg._BitWriter()
        if len(members) > 1:
            units = [[(c, my * hvs[c][1] + y, mx * hvs[c][0] + x) for c in members for y in range(hvs[c][1]) for x in range(hvs[c][0])]
                     for my in range(cy) for mx in range(cx)]
        else:
            units = [[(members[0], by, bx)] for by in range(own[members[0]][0]) for bx in range(own[members[0]][1])]
        pred, rst = {c: 0 for c in members}, 0
        for u, unit in enumerate(units):
            if restart_interval and u and u % restart_interval == 0:
                bw.flush()
                bw.out += bytes([0xFF, 0xD0 + (rst & 7)])
                rst += 1
                pred = {c: 0 for c in members}
            for c, by, bx in unit:
                zz = coefs[c][by, bx]
                td, ta = tabs[c]
                s, b = coef_jpeg._mag(int(zz[0]) - pred[c])
                pred[c] = int(zz[0])
                bw.put(*dc_t[td][s])
                if s:
                    bw.put(b, s)
                k = 1
                for i in [i for i in range(1, 64) if zz[i]]:
                    run = i - k
                    while run > 15:
                        bw.put(*ac_t[ta][0xF0])
                        run -= 16
                    s, b = coef_jpeg._mag(zz[i])
                    bw.put(*ac_t[ta][(run << 4) | s])
                    bw.put(b, s)
                    k = i + 1
                if k < 64:
                    bw.put(*ac_t[ta][0x00])
        bw.flush()
        sos = coef_jpeg._seg(0xDA, bytes([len(members)]) + b"".join(bytes([b"CMYK"[c], (tabs[c][0] << 4) | tabs[c][1]]) for c in members) + bytes([0, 63, 0]))
        return sos + bytes(bw.out)

    qt = E.quant_tables(q, "4:2:0")
    hdr = bytearray(b"\xff\xd8")
    if adobe is not None:
        hdr += ADOBE(adobe)
    for t in sorted(qt):
        hdr += coef_jpeg._seg(0xDB, bytes([t]) + bytes(int(x) for x in qt[t]))
    hdr += coef_jpeg._seg(0xC1 if sof1 else 0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([4]) +
                          b"".join(bytes([b"CMYK"[c], (hvs[c][0] << 4) | hvs[c][1], 0 if c in (0, 3) else 1]) for c in range(4)))
    for (tc, th) in sorted(huff):
        bits, vals = huff[(tc, th)]
        hdr += coef_jpeg._seg(0xC4, bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals))
    if restart_interval:
        hdr += coef_jpeg._seg(0xDD, restart_interval.to_bytes(2, "big"))
    body = b"".join(scan([c]) for c in range(4)) if per_component else scan([0, 1, 2, 3])
    return _pad(bytes(hdr) + body + b"\xff\xd9")


# (component 0's factors, component 3 at them?): Pillow's own three (K at 1x1 under 1x1, 2x1, 2x2) come from pillow_cmyk; the writer adds
# K at component 0's factors and the 1x2 layouts
WRITTEN_LAYOUTS = (((2, 2), True), ((2, 1), True), ((1, 2), True), ((1, 2), False))
SIZES = X.SIZES
EDGE_SIZES = ((3, 3), (4, 5), (5, 7), (17, 1), (9, 17), (333, 217))       # quad and MCU edges the grid lacks: widths 3, 4, 5, one past an MCU, odd heights


def grid4(sampling):
    """the four-component files of one layout of components 0..2, [(name, jpeg)]: CMYK, YCCK and no-Adobe, K at 1x1 and at component 0's
    factors, baseline and progressive, over SIZES and EDGE_SIZES"""
    hv0 = coef_jpeg.LUMA_HV[sampling]
    out = []
    for i, (w, h) in enumerate(SIZES + EDGE_SIZES):
        q = (90, 75, 95)[i % 3]
        variant = ("cmyk", "ycck", "bare")[i % 3]
        if sampling in PILLOW_SUB:
            out.append(("pillow_%s_%dx%d_q%d%s" % (variant, w, h, q, "_prog" if i % 2 else ""), pillow_cmyk(w, h, sampling, q, bool(i % 2), variant)))
        if sampling != "4:4:4":
            adobe = (2, 0, None)[i % 3]
            for k_full in ((True, False) if sampling == "4:4:0" else (True,)):
                if i % 2 == 0 or sampling == "4:4:0":
                    out.append(("written_%s_k%d_%dx%d_q%d" % ({0: "cmyk", 2: "ycck", None: "bare"}[adobe], k_full, w, h, q),
                                written4(w, h, hv0, k_full, q, adobe, restart_interval=(3 if i % 4 == 0 else 0), per_component=(i % 4 == 2), sof1=(i % 8 == 6))))
    return out


def grid3(sampling):
    """the three-component files of one layout: every marker variant, baseline and progressive, [(name, jpeg, model)]"""
    out = []
    for i, (w, h) in enumerate(((33, 31), (45, 53), (17, 9), (64, 48), (8, 33))):
        for j, variant in enumerate(("adobe0", "adobe1", "both", "ids", "none")):
            if (i + j) % 2 == 0 or variant in ("adobe0", "ids"):
                prog = (i + j) % 3 == 0 and sampling != "4:4:0"
                out.append(("%s_%dx%d%s" % (variant, w, h, "_prog" if prog else ""), pillow_rgb3(w, h, sampling, (90, 75)[i % 2], variant, prog), RGB3_MODEL[variant]))
    return out
