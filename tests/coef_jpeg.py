"""Baseline JPEGs written straight from chosen quantised coefficients, and a small independent decoder for them.

The synthetic inputs elsewhere in the suite are encodes of smooth pictures: small coefficients, the common Huffman symbols,
predictors that never drift.  This module writes the stream from the coefficients themselves, so that a test can put any
value at any zig-zag position of any block, under any quantiser (8- or 16-bit), any Huffman table and any restart interval.

  write_jpeg()      the writer (baseline, one interleaved scan, optional DRI)
  decode_coefs()    a pure-Python entropy decoder (baseline + RSTn) that gives back the coefficient arrays and the symbol
                    histogram of every table: it shares no code with the writer's bit packing, nor with the project
  float_decode()    a float64 decode (dequantise, exact 8x8 IDCT, level shift, YCbCr -> RGB, nearest-neighbour chroma)
  huff_from_hist()  a length-limited Huffman table (JPEG Annex K.2) from a symbol histogram

Coefficient arrays are per component, shaped (block rows, block columns, 64) in zig-zag order over the whole MCU grid
(padding blocks included); entry 0 of a block is its DC VALUE (the writer codes the differences).  Values are Python-int
ranges: a DC value may leave int16 (the predictor drift cases), a difference may not leave category 11.
"""
import numpy as np

from jpegdec_amd.synth import _ZIGZAG, _annex_k_tables, _codes

LUMA_HV = {"gray": (1, 1), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:4:0": (1, 2), "4:2:0": (2, 2)}
LAYOUTS = ("gray", "4:4:4", "4:2:2", "4:4:0", "4:2:0")
SHORT = {"gray": "gray", "4:4:4": "c444", "4:2:2": "c422", "4:4:0": "c440", "4:2:0": "c420"}
AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]      # the 162 symbols of a baseline AC table


def geometry(width, height, sampling):
    """(MCU columns, MCU rows, [(block rows, block columns) per component], (h, v) of luma)"""
    hs, vs = LUMA_HV[sampling]
    cx, cy = (width + 8 * hs - 1) // (8 * hs), (height + 8 * vs - 1) // (8 * vs)
    shapes = [(cy * vs, cx * hs)] + ([] if sampling == "gray" else [(cy, cx), (cy, cx)])
    return cx, cy, shapes, (hs, vs)


def zero_coefs(width, height, sampling):
    return [np.zeros((r, c, 64), dtype=np.int64) for r, c in geometry(width, height, sampling)[2]]


def annex_k():
    """(luma quantiser, chroma quantiser (quality 50, zig-zag), {(class, id): (bits, vals)})"""
    return _annex_k_tables()


def huff_from_hist(hist, max_len=16):
    """Huffman table (bits[16], vals) for {symbol: count > 0}, code lengths limited to max_len, the all-ones code left unused:
    the procedure of JPEG Annex K.2 (a reserved symbol of count 1 takes the all-ones code and is dropped at the end)."""
    freq = {s: int(c) for s, c in hist.items() if c > 0}
    freq[256] = 1
    syms = sorted(freq)
    f = {s: freq[s] for s in syms}
    size = {s: 0 for s in syms}
    other = {s: None for s in syms}
    live = dict(f)
    while len(live) > 1:
        v1 = min(live, key=lambda s: (live[s], -s))
        v2 = min((s for s in live if s != v1), key=lambda s: (live[s], -s))
        live[v1] += live.pop(v2)
        while True:
            size[v1] += 1
            if other[v1] is None:
                break
            v1 = other[v1]
        other[v1] = v2
        while True:
            size[v2] += 1
            if other[v2] is None:
                break
            v2 = other[v2]
    bits = [0] * 40
    for s in syms:
        bits[size[s]] += 1
    i = len(bits) - 1
    while i > max_len:                     # K.2 adjust_BITS, to max_len
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
    bits[i] -= 1                           # the reserved symbol's code
    order = sorted((s for s in syms if s != 256), key=lambda s: (size[s], s))
    return bits[1:17], order


def _mag(v):
    a = abs(int(v))
    s = a.bit_length()
    return s, (int(v) if v >= 0 else int(v) + (1 << s) - 1)


class _BitWriter:
    """MSB-first bit packer with byte stuffing; `bits` counts the bits of the FILTERED scan (no stuffing, no markers)"""
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.bits = 0

    def put(self, code, ln):
        self.acc = (self.acc << ln) | (code & ((1 << ln) - 1))
        self.n += ln
        self.bits += ln
        if self.n >= 64:
            self._drain()

    def _drain(self):
        k = self.n >> 3
        if k:
            self.n -= 8 * k
            self.out += (self.acc >> self.n).to_bytes(k, "big").replace(b"\xff", b"\xff\x00")
            self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n & 7:
            self.put((1 << (8 - (self.n & 7))) - 1, 8 - (self.n & 7))
        self._drain()


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def write_jpeg(width, height, sampling, coefs, quant, quant_ids=None, huff=None, table_ids=None, restart_interval=0,
               ac_pairs=None, pad_to=300, return_layout=False):
    """coefs: per component (block rows, block columns, 64) zig-zag arrays over the MCU grid (zero_coefs' shapes).
    quant: {table id: 64 zig-zag entries}; a table with an entry above 255 is written at 16-bit precision.
    quant_ids: quantiser per component (default luma 0, chroma 1, or 0 where only table 0 is given).
    huff: {(class, id): (bits, vals)} (default Annex K); table_ids: (DC, AC) table per component.
    ac_pairs: {(component, block row, block column): [(run, value), ...]} -- that block's AC symbols exactly as given, no EOB
    added (the syntax of runs past position 63).  pad_to: a COM segment brings smaller files up to this size (the reference
    refuses files under 256 bytes).
    return_layout: also return the scan's layout, (jpeg, layout): layout["blocks"] lists every block in stream order as
    (component, block row, block column, DC symbol, AC symbols), a symbol = (position of its first bit in the FILTERED scan,
    code length, magnitude bits or -1 for EOB); layout["restarts"] the filtered bit position of every restart interval's start;
    layout["scan_bits"] the filtered scan's length in bits (whole bytes)."""
    cx, cy, shapes, (hs, vs) = geometry(width, height, sampling)
    nc = len(shapes)
    assert len(coefs) == nc and all(c.shape == (r, w, 64) for c, (r, w) in zip(coefs, shapes))
    if quant_ids is None:
        quant_ids = [0] + [1 if 1 in quant else 0] * (nc - 1)
    if huff is None:
        huff = annex_k()[2]
    if table_ids is None:
        table_ids = [(0, 0)] + [(1, 1)] * (nc - 1)
    dc_t = {th: _codes(*huff[(0, th)]) for (tc, th) in huff if tc == 0}
    ac_t = {th: _codes(*huff[(1, th)]) for (tc, th) in huff if tc == 1}
    ac_pairs = ac_pairs or {}
    bw = _BitWriter()
    blocks, restarts = [], []

    def block(c, by, bx, pred):
        td, ta = table_ids[c]
        zz = coefs[c][by, bx]
        dc = int(zz[0])
        s, b = _mag(dc - pred)
        assert s <= 11, ("DC difference out of range", c, by, bx, dc - pred)
        syms = []
        dc_sym = (bw.bits, dc_t[td][s][1], s)
        bw.put(*dc_t[td][s])
        if s:
            bw.put(b, s)

        def ac(rs, s, b):
            code, ln = ac_t[ta][rs]
            syms.append((bw.bits, ln, s if rs else -1))
            bw.put(code, ln)
            if s:
                bw.put(b, s)

        if (c, by, bx) in ac_pairs:
            for run, v in ac_pairs[(c, by, bx)]:
                s, b = _mag(v)
                ac((run << 4) | s, s, b)
        else:
            nz = [i for i in range(1, 64) if zz[i]]
            run, k = 0, 1
            for i in nz:
                run = i - k
                while run > 15:
                    ac(0xF0, 0, 0)
                    run -= 16
                s, b = _mag(zz[i])
                assert 1 <= s <= 10, ("AC value out of range", c, by, bx, i, int(zz[i]))
                ac((run << 4) | s, s, b)
                k = i + 1
            if not nz or nz[-1] < 63:
                ac(0x00, 0, 0)
        if return_layout:
            blocks.append((c, by, bx, dc_sym, syms))
        return dc

    pred = [0] * nc
    rst = 0
    for m in range(cx * cy):
        my, mx = divmod(m, cx)
        if restart_interval and m and m % restart_interval == 0:
            bw.flush()
            bw.out += bytes([0xFF, 0xD0 + (rst & 7)])
            rst += 1
            pred = [0] * nc
            restarts.append(bw.bits)
        for v in range(vs):
            for h in range(hs):
                pred[0] = block(0, my * vs + v, mx * hs + h, pred[0])
        for c in range(1, nc):
            pred[c] = block(c, my, mx, pred[c])
    bw.flush()

    hdr = bytearray(b"\xff\xd8")
    hdr += _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in sorted(quant):
        q = [int(x) for x in quant[t]]
        assert len(q) == 64 and all(1 <= x <= 65535 for x in q)
        if max(q) > 255:
            hdr += _seg(0xDB, bytes([0x10 | t]) + b"".join(x.to_bytes(2, "big") for x in q))
        else:
            hdr += _seg(0xDB, bytes([t]) + bytes(q))
    comp = [(1, (hs << 4) | vs, quant_ids[0])] + [(2 + i, 0x11, quant_ids[1 + i]) for i in range(nc - 1)]
    hdr += _seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc]) +
                b"".join(bytes(c) for c in comp))
    used = {(0, td) for td, _ in table_ids} | {(1, ta) for _, ta in table_ids}
    for (tc, th) in sorted(used):
        bits, vals = huff[(tc, th)]
        hdr += _seg(0xC4, bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals))
    if restart_interval:
        hdr += _seg(0xDD, restart_interval.to_bytes(2, "big"))
    body = bytes(bw.out) + b"\xff\xd9"
    short = pad_to - (len(hdr) + 14 + 2 * nc + len(body))
    if short > 0:
        hdr += _seg(0xFE, b"\x00" * max(short, 1))
    hdr += _seg(0xDA, bytes([nc]) + b"".join(bytes([c[0], (td << 4) | ta]) for c, (td, ta) in zip(comp, table_ids)) + bytes([0, 63, 0]))
    if return_layout:
        return bytes(hdr) + body, dict(blocks=blocks, restarts=restarts, scan_bits=bw.bits,
                                       round_last=bool(restart_interval) and (cx * cy) % restart_interval == 0)
    return bytes(hdr) + body


def reader_entries(layout):
    """The block index the reference's bit reader implies (the serial host pre-scan writes it): for every block,
    (byte, bit offset, truncated) of the reader at the block's first AC symbol -- behind the refill at the top of the AC loop --
    and the closing entry (byte, offset) where the last block leaves it.  The reader holds 64 bits from its byte on and moves
    its byte on (off >> 3 bytes) only when more than 47 bits of them are used: at a block's start, in front of a DC magnitude
    the DC table's lookup does not hold (code + magnitude longer than six bits), at the top of the AC loop and behind every AC
    symbol but EOB.  A magnitude read is truncated where it reaches past the 64 bits (the bits it misses read as zeros).  A
    restart interval starts on the next byte boundary (the byte is not moved); so does the closing entry where the last interval
    is whole."""
    pos = off = 0
    out = []
    restarts = set(layout["restarts"])

    def check(pos, off):
        return (pos + (off >> 3), off & 7) if off > 47 else (pos, off)

    for c, by, bx, (p, ln, s), syms in layout["blocks"]:
        if p in restarts:
            assert (8 * pos + off + 7) // 8 * 8 == p
            off = p - 8 * pos
        assert 8 * pos + off == p
        pos, off = check(pos, off)
        if s and ln + s <= 6:
            off += ln + s
        else:
            off += ln
            if s:
                pos, off = check(pos, off)
                off += s
        pos, off = check(pos, off)
        entry = [pos, off, False]
        for q, ln, s in syms:
            assert 8 * pos + off == q
            off += ln
            if s < 0:
                break
            if s and off + s > 64:
                entry[2] = True
            off += s
            pos, off = check(pos, off)
        out.append(tuple(entry))
    if layout.get("round_last"):              # (the interval count runs out behind the last MCU as well)
        off = (off + 7) & ~7
    return out, (pos, off)


# ---- the independent decoder ---------------------------------------------------------------------------------------
class DecodeError(Exception):
    pass


def _parse(jpeg):
    assert jpeg[:2] == b"\xff\xd8"
    i, q, huff, dri, frame, scan = 2, {}, {}, 0, None, None
    while i < len(jpeg):
        assert jpeg[i] == 0xFF
        m = jpeg[i + 1]
        ln = (jpeg[i + 2] << 8) | jpeg[i + 3]
        seg = jpeg[i + 4:i + 2 + ln]
        if m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                if pq:
                    q[tq] = [(seg[j + 1 + 2 * k] << 8) | seg[j + 2 + 2 * k] for k in range(64)]
                    j += 129
                else:
                    q[tq] = list(seg[j + 1:j + 65])
                    j += 65
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                tc, th = seg[j] >> 4, seg[j] & 15
                bits = list(seg[j + 1:j + 17])
                n = sum(bits)
                huff[(tc, th)] = (bits, list(seg[j + 17:j + 17 + n]))
                j += 17 + n
        elif m == 0xC0:
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            frame = (w, h, [(seg[6 + 3 * k], seg[7 + 3 * k], seg[8 + 3 * k]) for k in range(nc)])
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            nc = seg[0]
            scan = [(seg[1 + 2 * k], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(nc)]
            return q, huff, dri, frame, scan, i + 2 + ln
        i += 2 + ln
    raise DecodeError("no SOS")


def decode_coefs(jpeg):
    """-> dict(width, height, sampling, coefs (as zero_coefs), quant {id: zig-zag list}, quant_ids, table_ids,
    hist {(class, id): {symbol: count}}, restart_interval).  Raises DecodeError on what a baseline decoder must refuse."""
    q, huff, dri, frame, scan, p = _parse(jpeg)
    w, h, comps = frame
    hv = comps[0][1]
    sampling = "gray" if len(comps) == 1 else {v: k for k, v in LUMA_HV.items() if k != "gray"}[(hv >> 4, hv & 15)]
    cx, cy, shapes, (hs, vs) = geometry(w, h, sampling)
    # the entropy-coded bytes, stuffing removed, restart markers as None
    data, j = [], p
    while j < len(jpeg):
        b = jpeg[j]
        if b == 0xFF:
            n = jpeg[j + 1]
            if n == 0:
                data.append(0xFF)
                j += 2
                continue
            if 0xD0 <= n <= 0xD7:
                data.append(("RST", n - 0xD0))
                j += 2
                continue
            break
        data.append(b)
        j += 1
    decs = {}
    for key, (bits, vals) in huff.items():
        d, code, k = {}, 0, 0
        for ln in range(1, 17):
            for _ in range(bits[ln - 1]):
                d[(ln, code)] = vals[k]
                code += 1
                k += 1
            code <<= 1
        decs[key] = d
    hist = {key: {} for key in huff}
    st = {"i": 0, "acc": 0, "n": 0}

    def bit():
        if st["n"] == 0:
            if st["i"] >= len(data) or not isinstance(data[st["i"]], int):
                raise DecodeError("out of data")
            st["acc"], st["n"] = data[st["i"]], 8
            st["i"] += 1
        st["n"] -= 1
        return (st["acc"] >> st["n"]) & 1

    def sym(key):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | bit()
            s = decs[key].get((ln, code))
            if s is not None:
                hist[key][s] = hist[key].get(s, 0) + 1
                return s
        raise DecodeError("bad code")

    def receive(s):
        v = 0
        for _ in range(s):
            v = (v << 1) | bit()
        return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v

    coefs = [np.zeros((r, c, 64), dtype=np.int64) for r, c in shapes]
    ids = {cid: k for k, (cid, _, _) in enumerate(comps)}
    tabs = [None] * len(comps)
    for cid, td, ta in scan:
        tabs[ids[cid]] = (td, ta)
    pred = [0] * len(comps)

    def block(c, by, bx):
        td, ta = tabs[c]
        s = sym((0, td))
        pred[c] += receive(s)
        out = coefs[c][by, bx]
        out[0] = pred[c]
        k = 1
        while k < 64:
            rs = sym((1, ta))
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r != 15:
                    break
                k += 16
                continue
            k += r
            if k > 63:
                raise DecodeError("run past coefficient 63")
            out[k] = receive(s)
            k += 1

    for m in range(cx * cy):
        my, mx = divmod(m, cx)
        if dri and m and m % dri == 0:
            st["n"] = 0
            if st["i"] >= len(data) or isinstance(data[st["i"]], int):
                raise DecodeError("restart marker missing")
            st["i"] += 1
            pred = [0] * len(comps)
        for v in range(vs):
            for hh in range(hs):
                block(0, my * vs + v, mx * hs + hh)
        for c in range(1, len(comps)):
            block(c, my, mx)
    return dict(width=w, height=h, sampling=sampling, coefs=coefs, quant=q, quant_ids=[c[2] for c in comps],
                table_ids=tabs, hist=hist, huff=huff, restart_interval=dri)


# ---- the float64 reference -------------------------------------------------------------------------------------------
_K = np.arange(8)
_IDCT = (np.cos((2 * _K[:, None] + 1) * _K[None, :] * np.pi / 16) * np.where(_K[None, :] == 0, np.sqrt(1 / 8), 0.5))   # x = C @ X @ C.T


def float_planes(dec):
    """float64 samples of every component (level-shifted, NOT clamped), at the component's own resolution over the MCU grid"""
    planes = []
    for c, arr in enumerate(dec["coefs"]):
        qz = np.asarray(dec["quant"][dec["quant_ids"][c]], dtype=np.float64)
        nat = np.zeros(arr.shape, dtype=np.float64)
        nat[..., _ZIGZAG] = arr * qz
        blk = nat.reshape(arr.shape[0], arr.shape[1], 8, 8)
        pix = np.einsum("ij,abjk,lk->abil", _IDCT, blk, _IDCT) + 128.0
        planes.append(pix.transpose(0, 2, 1, 3).reshape(arr.shape[0] * 8, arr.shape[1] * 8))
    return planes


def float_decode(dec):
    """float64 RGB (or gray) image, H x W (x 3), rounded and clamped to 0..255: chroma upsampled by nearest neighbour."""
    planes = float_planes(dec)
    w, h = dec["width"], dec["height"]
    hs, vs = LUMA_HV[dec["sampling"]]
    y = np.clip(planes[0], 0, 255)[:h, :w]
    if len(planes) == 1:
        return np.clip(np.rint(y), 0, 255).astype(np.uint8)
    cb, cr = (np.clip(p, 0, 255).repeat(vs, 0).repeat(hs, 1)[:h, :w] - 128.0 for p in planes[1:])
    rgb = np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)
