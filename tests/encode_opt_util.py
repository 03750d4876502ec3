"""JDA_ENCODE_OPTIMIZE stated in Python (rule 9): libjpeg's optimize_coding, checked against Pillow's optimize=True in
tests/test_encode_opt_cpu.py.  It shares no code with the product: the table algorithm is a port of jchuff.c's jpeg_gen_optimal_table,
the symbols are counted from the coefficients of tests/encode_util.py, and the file is tests/coef_jpeg.write_jpeg's with these tables.

  optimal_table(freq)                      (bits[16], vals, the longest code before the lengths were limited)
  histograms(w, h, sampling, coefs, ri)    {(class, table): 256 counts}: class 0 DC, 1 AC; table 0 luma, 1 Cb and Cr together
  hist544(hists)                           the same in the index layout of the product's word tables: AC at t * 256 + rs, DC at 512 + t * 16 + s
  tables(hists)                            {(class, table): (bits, vals)}
  file_bytes_opt(img, sampling, q, ri)     the whole file (return_layout: as encode_util.file_bytes)"""
import numpy as np

from tests import coef_jpeg
from tests import encode_util as E

HUFF_DWORDS = 544
OPT_MAX_BLOCKS = 15_625_000
START = 1000000000                      # libjpeg's searches start from here: no count may pass it


def optimal_table(freq):
    """jpeg_gen_optimal_table: freq = up to 256 counts.  The pseudo-symbol 256 (count 1) is added; the two least frequent symbols are merged,
    a tie going to the LARGER index (<= in both searches); code sizes from the others[] chains; lengths above 16 folded back; one code taken
    from the longest length in use; the symbols listed by length, then by value."""
    f = np.zeros(257, dtype=np.int64)
    f[:len(freq)] = np.asarray(freq, dtype=np.int64)
    assert f.max() <= START
    f[256] = 1
    codesize, others = [0] * 257, [-1] * 257
    while True:
        live = np.flatnonzero((f > 0) & (f <= START))
        if len(live) < 2:
            break
        c1 = int(live[np.flatnonzero(f[live] == f[live].min())[-1]])
        rest = live[live != c1]
        c2 = int(rest[np.flatnonzero(f[rest] == f[rest].min())[-1]])
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    longest = max(codesize)
    assert longest <= 32, "libjpeg gives up here (JERR_HUFF_CLEN_OVERFLOW)"
    bits = [0] * 33
    for s in codesize:
        if s:
            bits[s] += 1
    i = 32
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for ln in range(1, 33) for s in range(256) if codesize[s] == ln]
    return bits[1:17], vals, longest


def block_symbols(zz, pred):
    """(DC category, [AC symbols]) of one block's 64 zig-zag coefficients"""
    cat = abs(int(zz[0]) - pred).bit_length()
    syms, k = [], 1
    nz = np.flatnonzero(zz[1:]) + 1
    for i in nz.tolist():
        run = i - k
        syms += [0xF0] * (run >> 4)
        syms.append(((run & 15) << 4) | abs(int(zz[i])).bit_length())
        k = i + 1
    if k < 64:
        syms.append(0x00)
    return cat, syms


def histograms(w, h, sampling, coefs, ri=0):
    """every block of the scan, dummy blocks included (encode_util.coefficients gives them their DC), the predictors reset at every interval"""
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(w, h, sampling)
    nc = len(shapes)
    hist = {(cls, t): np.zeros(256, dtype=np.int64) for cls in (0, 1) for t in range(1 if nc == 1 else 2)}
    pred = [0] * nc
    for m in range(cx * cy):
        my, mx = divmod(m, cx)
        if ri and m and m % ri == 0:
            pred = [0] * nc
        order = [(0, my * vs + v, mx * hs + hh) for v in range(vs) for hh in range(hs)] + [(c, my, mx) for c in range(1, nc)]
        for c, by, bx in order:
            zz = coefs[c][by, bx]
            cat, syms = block_symbols(zz, pred[c])
            pred[c] = int(zz[0])
            t = 0 if c == 0 else 1
            hist[(0, t)][cat] += 1
            np.add.at(hist[(1, t)], syms, 1)
    return hist


def hist544(hists):
    out = np.zeros(HUFF_DWORDS, dtype=np.uint32)
    for (cls, t), f in hists.items():
        if cls:
            out[t * 256:t * 256 + 256] = f
        else:
            out[512 + t * 16:512 + t * 16 + 16] = f[:16]
    return out


def tables(hists):
    return {key: optimal_table(f)[:2] for key, f in hists.items()}


def reorder_dht(jpeg):
    """coef_jpeg.write_jpeg lists the DHT segments DC 0, DC 1, AC 0, AC 1; libjpeg writes an optimised scan's tables component by component:
    DC 0, AC 0, DC 1, AC 1.  The same segments in that order."""
    i, segs = 2, []
    while True:
        assert jpeg[i] == 0xFF
        ln = int.from_bytes(jpeg[i + 2:i + 4], "big")
        segs.append(jpeg[i:i + 2 + ln])
        i += 2 + ln
        if segs[-1][1] == 0xDA:
            break
    at = [k for k, s in enumerate(segs) if s[1] == 0xC4]
    assert at == list(range(at[0], at[0] + len(at)))
    dht = sorted((segs[k] for k in at), key=lambda s: (s[4] & 15, s[4] >> 4))
    return jpeg[:2] + b"".join(segs[:at[0]] + dht + segs[at[-1] + 1:]) + jpeg[i:]


def dht_segments(jpeg):
    """[(Tc << 4 | Th, bits, vals)] in the file's order"""
    i, out = 2, []
    while jpeg[i + 1] != 0xDA:
        ln = int.from_bytes(jpeg[i + 2:i + 4], "big")
        if jpeg[i + 1] == 0xC4:
            seg, j = jpeg[i + 4:i + 2 + ln], 0
            while j < len(seg):
                n = sum(seg[j + 1:j + 17])
                out.append((seg[j], list(seg[j + 1:j + 17]), list(seg[j + 17:j + 17 + n])))
                j += 17 + n
        i += 2 + ln
    return out


def file_bytes_opt(img, sampling, quality, restart_interval=0, return_layout=False):
    img = np.asarray(img)
    h, w = img.shape[:2]
    coefs = E.coefficients(img, sampling, quality)
    huff = tables(histograms(w, h, sampling, coefs, restart_interval))
    out = coef_jpeg.write_jpeg(w, h, sampling, coefs, E.quant_tables(quality, sampling), huff=huff, restart_interval=restart_interval, pad_to=0,
                               return_layout=return_layout)
    return (reorder_dht(out[0]), out[1]) if return_layout else reorder_dht(out)


# ---- the jobs of the tests: (img, sampling, quality, restart interval, flag), one pixel size ("gray" | "colour") a call ---------------------------
GRID_PICTURES = (("noise", 75), ("smooth", 30), ("pixels", 100), ("blocks", 100))
PILLOW_PICTURES = GRID_PICTURES + (("flat", 50), ("noise", 100), ("noise", 1))
PILLOW_INTERVALS = (0, 1, 3)
_TWINS = {}


def twin(img, sampling, q, ri, flag):
    """(file, layout) of the optimised twin (flag 1) or the standard one (0), computed once a case"""
    key = (img.shape, img.tobytes(), sampling, q, ri, flag)
    if key not in _TWINS:
        _TWINS[key] = (file_bytes_opt if flag else E.file_bytes)(img, sampling, q, ri, return_layout=True)
    return _TWINS[key]


def grid_cases(sampling):
    """encode_util.SIZES x GRID_PICTURES, the interval choices of encode_util.restart_intervals dealt round; every third job standard"""
    out = []
    for w, h in E.SIZES:
        for kind, q in GRID_PICTURES:
            ris = E.restart_intervals(w, h, sampling)
            out.append((E.picture(kind, w, h, sampling), sampling, q, ris[len(out) % len(ris)], 0 if len(out) % 3 == 2 else 1))
    return out


def edge_cases(sampling_class):
    """The smallest shapes at which gather and the second lengths pass can go wrong: 1 x 1 jobs between larger ones (a job's blocks begin and
    end inside a wavefront), optimised and standard jobs alternating, a job over four workgroups (gray 264 x 240: 990 blocks into one
    histogram), 257 flat blocks (blocks 255 | 256), dummy luma blocks (17 x 9, 25 x 16 in 4:2:0 and 4:2:2), zero runs of 15 .. 62, the top
    categories ("pixels" and "blocks" at quality 100), flat 1 x 1 (tables of one symbol, codes of one bit), an interval every MCU."""
    one = lambda kind, s, seed=0: E.picture(kind, 1, 1, s, seed)
    if sampling_class == "gray":
        g = "gray"
        return [(one("flat", g), g, 75, 0, 1), (E.picture("noise", 264, 240, g, 11), g, 75, 0, 1), (one("noise", g, 1), g, 75, 0, 0),
                (E.picture("flat", 2056, 8, g), g, 75, 0, 1), (one("noise", g, 2), g, 75, 1, 1), (E.zrl_picture(), g, E.ZRL_QUALITY, 0, 1),
                (E.picture("noise", 17, 9, g, 3), g, 75, 1, 0), (E.picture("pixels", 25, 16, g), g, 100, 1, 1), (one("flat", g), g, 1, 0, 0),
                (E.picture("noise", 264, 240, g, 11), g, 75, 1, 1), (E.picture("noise", 40, 40, g, 4), g, 100, 0, 0), (one("flat", g), g, 100, 0, 1)]
    a, b, c = "4:2:0", "4:2:2", "4:4:4"
    return [(one("flat", a), a, 75, 0, 1), (E.picture("noise", 17, 9, a, 1), a, 75, 0, 1), (one("noise", c, 1), c, 75, 0, 0),
            (E.picture("noise", 25, 16, a, 2), a, 75, 1, 1), (E.picture("noise", 17, 9, b, 3), b, 75, 1, 1), (one("flat", b), b, 50, 0, 1),
            (E.picture("noise", 25, 16, b, 4), b, 75, 0, 0), (E.picture("pixels", 33, 47, a), a, 100, 0, 1), (one("noise", a, 2), a, 75, 1, 0),
            (E.picture("blocks", 33, 47, a), a, 100, 1, 1), (E.picture("noise", 129, 65, c, 5), c, 75, 0, 1), (one("flat", c), c, 100, 0, 1),
            (E.picture("smooth", 25, 16, b), b, 30, 3, 1), (E.picture("noise", 129, 65, c, 5), c, 75, 0, 0), (E.picture("noise", 17, 9, a, 1), a, 75, 1, 1)]


def batch(sampling_class):
    """the grid of every sampling of the pixel size, then the edges"""
    samplings = ("gray",) if sampling_class == "gray" else ("4:4:4", "4:2:2", "4:2:0")
    return [c for s in samplings for c in grid_cases(s)] + edge_cases(sampling_class)
