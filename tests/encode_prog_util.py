"""jda_encode_surfaces_progressive stated in Python (rules 10 to 14): libjpeg's default scan script (jcparam.c's
jpeg_simple_progression) and jcphuff.c's four passes, one unit after the other, with optimal tables per scan.  Checked against Pillow's
Image.save(progressive=True) in tests/test_encode_prog_cpu.py.  It shares no code with the product: the coefficients are
tests/encode_util.py's, the table algorithm tests/encode_opt_util.py's port of jpeg_gen_optimal_table.  Unlike tests/prog_write.py it
knows the two rules only an ENCODER needs to be libjpeg's: a run of end-of-band blocks is flushed at 0x7FFF blocks and as soon as more
than 937 correction bits are buffered.

  script(sampling)                          [(components, Ss, Se, Ah, Al)] in file order
  file_bytes_prog(img, sampling, quality)   the whole file (return_layout: (file, layout))
  write_prog(w, h, sampling, coefs, q)      the same from chosen coefficients

layout = a dict per scan: comps, ss, se, ah, al, n_units,
  cls    per unit: breaker | joins << 1 | bits handed to the run << 8 | last newly nonzero position << 16 (refinement AC scans; 0 for DC)
  run    per unit: 0, or IN_RUN | distance to the run's first unit << 10 | offset in the run's buffered bits, or -- a run's first unit --
         IN_RUN | HEAD | units of the run << 10 | buffered bits
  runs   [(first unit, units, buffered bits, why)]: why = "breaker" | "limit" (0x7FFF) | "bits" (the 937 rule) | "end" (of the scan)
  len    per unit: its bits in the scan -- a run's symbol, extra bits and buffered bits belong to the run's FIRST unit, behind its own
  end    the running sum of len: the bit behind a unit's bits
  hist   {(class, table id): 256 counts}, tables {(class, table id): (bits, vals)}, zrl, no_zrl (refinement blocks with a newly nonzero coefficient
         and a zero run above 15 behind the last of them), header (bytes from the scan's first DHT, or SOS, to the end of SOS), data (stuffed),
         unstuffed_bytes
"""
import numpy as np

from jpegdec_amd.synth import _codes
from tests import coef_jpeg
from tests import encode_util as E
from tests.encode_opt_util import optimal_table
from tests.prog_write import own_extent

BREAKER, JOINS, IN_RUN, HEAD = 1, 2, 0x80000000, 0x40000000
MAX_RUN, MAX_BE = 0x7FFF, 937
ALL = (0, 1, 2)


def script(sampling):
    if sampling == "gray":
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    return [(ALL, 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
            (ALL, 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def _unit_blocks(sc, w, h, sampling, coefs):
    """(component per unit, (n_units, 64) coefficients) in the scan's order"""
    comps = sc[0]
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(w, h, sampling)
    if len(comps) > 1 or (sampling == "gray" and sc[1] == 0):
        cs, rows = [], []
        for my in range(cy):
            for mx in range(cx):
                for c in comps:
                    ch, cv = (hs, vs) if c == 0 else (1, 1)
                    for y in range(cv):
                        for x in range(ch):
                            cs.append(c)
                            rows.append(coefs[c][my * cv + y, mx * ch + x])
        return cs, np.asarray(rows, dtype=np.int64).reshape(len(rows), 64)
    c = comps[0]
    r, k = own_extent(w, h, sampling, c)
    return [c] * (r * k), np.asarray(coefs[c][:r, :k], dtype=np.int64).reshape(r * k, 64)


def _scan(sc, comp_of, blocks):
    """tokens [(owner unit, table key or None, symbol, extra value, extra bits)] and the unit records"""
    comps, ss, se, ah, al = sc
    n = len(blocks)
    toks, runs = [], []
    cls, run = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    info = dict(zrl=0, no_zrl=0)
    if ss == 0:
        pred = {c: 0 for c in comps}
        for u in range(n):
            c, dc = comp_of[u], int(blocks[u, 0])
            if ah:
                toks.append((u, None, 0, (dc >> al) & 1, 1))
                continue
            v = dc >> al
            d, pred[c] = v - pred[c], v
            s = abs(d).bit_length()
            toks.append((u, (0, 0 if c == 0 else 1), s, (d if d >= 0 else d - 1) & ((1 << s) - 1), s))
        return toks, cls, run, runs, info
    key = (1, 0 if comps[0] == 0 else 1)
    T = np.abs(blocks[:, ss:se + 1]) >> al
    neg = blocks[:, ss:se + 1] < 0
    busy = T.any(axis=1)
    st = dict(first=0, n=0, be=[], offs=[])

    def flush(why):
        if not st["n"]:
            return
        a, ln = st["first"], st["n"]
        cat = ln.bit_length() - 1
        toks.append((a, key, cat << 4, ln - (1 << cat), cat))
        toks.extend((a, None, 0, b, 1) for b in st["be"])
        run[a] = IN_RUN | HEAD | (ln << 10) | len(st["be"])
        for i, off in enumerate(st["offs"][1:], 1):
            run[a + i] = IN_RUN | (i << 10) | off
        runs.append((a, ln, len(st["be"]), why))
        st["n"], st["be"], st["offs"] = 0, [], []

    def join(u, bits):
        if not st["n"]:
            st["first"] = u
        st["offs"].append(len(st["be"]))
        st["n"] += 1
        st["be"] += bits
        if st["n"] == MAX_RUN:
            flush("limit")
        elif len(st["be"]) > MAX_BE:
            flush("bits")

    for u in range(n):
        if not busy[u]:                                     # nothing in the band: no symbol, no correction bit
            cls[u] = JOINS
            join(u, [])
            continue
        t, ng = T[u].tolist(), neg[u].tolist()
        r = 0
        if not ah:
            cls[u] = BREAKER | (JOINS if t[-1] == 0 else 0)
            flush("breaker")
            for i, x in enumerate(t):
                if x == 0:
                    r += 1
                    continue
                while r > 15:
                    toks.append((u, key, 0xF0, 0, 0))
                    info["zrl"] += 1
                    r -= 16
                s = x.bit_length()
                toks.append((u, key, (r << 4) | s, ((1 << s) - 1 - x) if ng[i] else x, s))
                r = 0
            if r:
                join(u, [])
            continue
        eob = max([i for i, x in enumerate(t) if x == 1], default=-1)
        br = []
        for i, x in enumerate(t):
            if x == 0:
                r += 1
                continue
            while r > 15 and i <= eob:
                flush("breaker")
                toks.append((u, key, 0xF0, 0, 0))
                info["zrl"] += 1
                r -= 16
                toks.extend((u, None, 0, b, 1) for b in br)
                br = []
            if x > 1:
                br.append(x & 1)
                continue
            flush("breaker")
            toks.append((u, key, (r << 4) | 1, 0 if ng[i] else 1, 1))
            toks.extend((u, None, 0, b, 1) for b in br)
            r, br = 0, []
        info["no_zrl"] += r > 15 and eob >= 0
        cls[u] = (BREAKER if eob >= 0 else 0) | (JOINS if eob < se - ss else 0) | (len(br) << 8) | ((eob + ss if eob >= 0 else 0) << 16)
        if r or br:
            join(u, br)
    flush("end")
    assert all(p[0] <= q[0] for p, q in zip(toks, toks[1:]))   # a run's bits lie behind its first unit's own and in front of the next unit's
    return toks, cls, run, runs, info


def _stuff(raw):
    return raw.replace(b"\xff", b"\xff\x00")


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def write_prog(w, h, sampling, coefs, quality, return_layout=False):
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(w, h, sampling)
    nc = len(shapes)
    quant = E.quant_tables(quality, sampling)
    out = bytearray(b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"))
    for t in sorted(quant):
        out += _seg(0xDB, bytes([t]) + bytes(quant[t]))
    comp = [(1, (hs << 4) | vs, 0)] + [(2 + i, 0x11, 1) for i in range(nc - 1)]
    out += _seg(0xC2, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc]) + b"".join(bytes(c) for c in comp))
    layout = []
    for sc in script(sampling):
        comps, ss, se, ah, al = sc
        comp_of, blocks = _unit_blocks(sc, w, h, sampling, coefs)
        toks, cls, run, runs, info = _scan(sc, comp_of, blocks)
        hist = {}
        for _, key, sym, _, _ in toks:
            if key is not None:
                hist.setdefault(key, np.zeros(256, dtype=np.int64))[sym] += 1
        tables = {key: optimal_table(f)[:2] for key, f in sorted(hist.items())}
        header = bytearray()
        for (tc, th), (bits, vals) in sorted(tables.items()):
            header += _seg(0xC4, bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals))
        sel = []
        for c in comps:
            td = (0 if c == 0 else 1) if (ss == 0 and ah == 0) else 0
            ta = (0 if c == 0 else 1) if ss else 0
            sel.append(bytes([comp[c][0], (td << 4) | ta]))
        header += _seg(0xDA, bytes([len(comps)]) + b"".join(sel) + bytes([ss, se, (ah << 4) | al]))
        codes = {key: _codes(*tab) for key, tab in tables.items()}
        lens = np.zeros(len(blocks), dtype=np.int64)
        acc, nbits = 0, 0
        for owner, key, sym, val, nb in toks:
            if key is not None:
                code, ln = codes[key][sym]
                acc, nbits = (acc << ln) | code, nbits + ln
                lens[owner] += ln
            acc, nbits = (acc << nb) | (val & ((1 << nb) - 1)), nbits + nb
            lens[owner] += nb
        pad = -nbits % 8
        acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
        raw = acc.to_bytes(nbits // 8, "big")
        data = _stuff(raw)
        out += header + data
        layout.append(dict(comps=comps, ss=ss, se=se, ah=ah, al=al, n_units=len(blocks), cls=cls, run=run, runs=runs, len=lens, end=np.cumsum(lens),
                           hist=hist, tables=tables, header=bytes(header), data=data, unstuffed=raw, unstuffed_bytes=len(raw), **info))
    out += b"\xff\xd9"
    return (bytes(out), layout) if return_layout else bytes(out)


_TWINS = {}


def file_bytes_prog(img, sampling, quality, return_layout=False):
    img = np.asarray(img)
    key = (img.shape, img.tobytes(), sampling, quality)
    if key not in _TWINS:
        h, w = img.shape[:2]
        _TWINS[key] = write_prog(w, h, sampling, E.coefficients(img, sampling, quality), quality, return_layout=True)
    return _TWINS[key] if return_layout else _TWINS[key][0]


def hist_words(layout_scan):
    """a scan's histogram in the product's layout: 256 bins, an AC scan's symbol rs at [rs], the first DC scan's category s of table t at [t * 16 + s]"""
    out = np.zeros(256, dtype=np.uint32)
    for (cls, t), f in layout_scan["hist"].items():
        if cls:
            out[:] = f
        else:
            out[t * 16:t * 16 + 16] = f[:16]
    return out


# ---- the pictures of the tests --------------------------------------------------------------------------------------------------------
def repeated_block(sampling):
    """160 x 16, twenty times two the first 8 x 8 draw of default_rng(5): at quality 100 no AC coefficient of it is newly nonzero in either
    refinement scan, so every block hands about 60 correction bits to one run -- which the 937 rule cuts"""
    blk = np.random.default_rng(5).integers(0, 256, (8, 8), np.uint8)
    g = np.tile(blk, (2, 20))
    return np.ascontiguousarray(g) if sampling == "gray" else np.ascontiguousarray(np.repeat(g[..., None], 4, -1))


def last_nonzero_picture():
    """gray 24 x 8: a checkerboard of pixels (zig-zag position 63 is its strongest term) between two flat blocks"""
    yy, xx = np.mgrid[0:8, 0:24]
    g = np.where((xx >= 8) & (xx < 16), ((xx + yy) & 1) * 255, 128)
    return np.ascontiguousarray(g.astype(np.uint8))


def edge_cases(sampling_class):
    """(img, sampling, quality) of one pixel size: what each is listed for is asserted from the twin's layout in tests/test_encode_prog_cpu.py"""
    one = lambda kind, s, seed=0: E.picture(kind, 1, 1, s, seed)
    if sampling_class == "gray":
        g = "gray"
        return [(one("flat", g), g, 75), (repeated_block(g), g, 100), (one("noise", g, 1), g, 75), (E.zrl_picture(), g, E.ZRL_QUALITY),
                (last_nonzero_picture(), g, 100), (E.picture("flat", 2056, 8, g), g, 75), (one("noise", g, 2), g, 100),
                (E.picture("flat", 264, 240, g), g, 75), (E.picture("noise", 17, 9, g, 3), g, 75), (E.picture("smooth", 264, 16, g), g, 90),
                (one("flat", g), g, 1), (E.zrl_picture(), g, 50)]
    a, b, c = "4:2:0", "4:2:2", "4:4:4"
    return [(one("flat", a), a, 75), (repeated_block(c), c, 100), (one("noise", c, 1), c, 75), (E.picture("noise", 17, 9, a, 1), a, 75),
            (E.picture("noise", 25, 16, b, 2), b, 100), (one("flat", b), b, 50), (E.picture("noise", 33, 47, a, 3), a, 90),
            (E.picture("noise", 17, 9, b, 3), b, 75), (one("noise", a, 2), a, 75), (E.picture("smooth", 129, 65, c), c, 75),
            (E.picture("flat", 2056, 8, c), c, 75), (E.picture("noise", 25, 16, a, 4), a, 30), (E.picture("noise", 33, 47, b, 5), b, 100), (one("flat", c), c, 100)]


FLAT_LIMIT = ("flat", 1456, 1456, "gray", 75)              # 33,124 blocks: an end-of-band run of 0x7FFF and the remainder in every AC scan


def grid_cases(sampling):
    from tests.encode_opt_util import GRID_PICTURES
    return [(E.picture(kind, w, h, sampling), sampling, q) for w, h in E.SIZES for kind, q in GRID_PICTURES]


def batch(sampling_class):
    samplings = ("gray",) if sampling_class == "gray" else ("4:4:4", "4:2:2", "4:2:0")
    return [c for s in samplings for c in grid_cases(s)] + edge_cases(sampling_class)
