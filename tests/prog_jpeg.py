"""A pure-Python decoder of progressive (SOF2) JPEGs down to their quantised coefficients (ITU-T T.81 Annex G).

It shares no code with the library: the file is cut into segments first, every scan's entropy-coded bytes are cut at their
restart markers and unstuffed as a whole, and the bits are read from the unstuffed bytes of one restart interval at a time.  The result has the
shape of tests/coef_jpeg.decode_coefs: per component a (block rows, block columns, 64) array in ZIG-ZAG order over the whole MCU
grid, entry 0 the DC value -- so that coef_jpeg.write_jpeg can re-encode it as a baseline file with the same quantisers.

  decode_coefs(jpeg)   -> dict(width, height, sampling, coefs, quant, quant_ids, quant_latched, restart_interval, n_scans, scan_ends)
                          quant: the DQT contents at the end of the file; quant_latched[c]: component c's table as it stood at the
                          first scan that names c (None: never named, or no table then)
                          scan_ends[k]: the file offset just behind scan k's entropy-coded bytes (where a file may be cut)
"""
import numpy as np

from tests.coef_jpeg import LUMA_HV, DecodeError, geometry


def _segments(jpeg):
    """[(marker, payload offset, payload length, entropy (offset, end) for SOS)] up to EOI or the end of the data"""
    assert jpeg[:2] == b"\xff\xd8"
    out, i, n = [], 2, len(jpeg)
    while i + 4 <= n:
        if jpeg[i] != 0xFF:
            raise DecodeError("marker expected at %d" % i)
        m = jpeg[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xD9:
            break
        ln = (jpeg[i + 2] << 8) | jpeg[i + 3]
        if m == 0xDA:
            j = i + 2 + ln
            while j < n:                                   # the entropy-coded segment ends at the next marker that is not RSTn
                if jpeg[j] == 0xFF and j + 1 < n and jpeg[j + 1] != 0 and not 0xD0 <= jpeg[j + 1] <= 0xD7 and jpeg[j + 1] != 0xFF:
                    break
                j += 1
            out.append((m, i + 4, ln - 2, (i + 2 + ln, j)))
            i = j
            continue
        out.append((m, i + 4, ln - 2, None))
        i += 2 + ln
    return out


class _Bits:
    """the bits of one restart interval, most significant first; zeros behind the end"""
    def __init__(self, raw):
        self.d = raw.replace(b"\xff\x00", b"\xff")
        self.p = 0

    def peek16(self):
        b = self.p >> 3
        return (int.from_bytes(self.d[b:b + 3].ljust(3, b"\0"), "big") >> (8 - (self.p & 7))) & 0xFFFF

    def get(self, k):                                      # k <= 16
        if k == 0:
            return 0
        b = self.p >> 3
        v = (int.from_bytes(self.d[b:b + 4].ljust(4, b"\0"), "big") >> (32 - (self.p & 7) - k)) & ((1 << k) - 1)
        self.p += k
        return v


def _lookup(bits, vals):
    """16-bit prefix -> (symbol, length) as two lists; length 0 = no code starts like this"""
    sym, ln = [0] * 65536, [0] * 65536
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            if code >= (1 << length):
                raise DecodeError("over-subscribed Huffman table")
            lo = code << (16 - length)
            span = 1 << (16 - length)
            sym[lo:lo + span] = [vals[k]] * span
            ln[lo:lo + span] = [length] * span
            code += 1
            k += 1
        code <<= 1
    return sym, ln


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def decode_coefs(jpeg):
    jpeg = bytes(jpeg)
    segs = _segments(jpeg)
    quant, huff, dri, frame = {}, {}, 0, None
    coefs = None
    scan_ends = []
    for m, off, ln, ent in segs:
        seg = jpeg[off:off + ln]
        if m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                if pq:
                    quant[tq] = [(seg[j + 1 + 2 * k] << 8) | seg[j + 2 + 2 * k] for k in range(64)]
                    j += 129
                else:
                    quant[tq] = list(seg[j + 1:j + 65])
                    j += 65
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                tc, th = seg[j] >> 4, seg[j] & 15
                bits = list(seg[j + 1:j + 17])
                n = sum(bits)
                huff[(tc, th)] = _lookup(bits, list(seg[j + 17:j + 17 + n]))
                j += 17 + n
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xC0:
            raise DecodeError("a baseline file")
        elif m == 0xC2:
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            comps = [(seg[6 + 3 * k], seg[7 + 3 * k], seg[8 + 3 * k]) for k in range(nc)]
            hv = comps[0][1]
            sampling = "gray" if nc == 1 else {v: k for k, v in LUMA_HV.items() if k != "gray"}[(hv >> 4, hv & 15)]
            cx, cy, shapes, (hs, vs) = geometry(w, h, sampling)
            coefs = [np.zeros((r, c, 64), dtype=np.int64) for r, c in shapes]
            frame = (w, h, comps)
            latched = [None] * nc
            # a component's own extent in blocks (A.1.1): what a non-interleaved scan visits
            own = []
            for k in range(nc):
                ch, cv = (hs, vs) if k == 0 else (1, 1)
                wc, hc = -(-w * ch // hs), -(-h * cv // vs)
                own.append((-(-hc // 8), -(-wc // 8)))
        elif m == 0xDA:
            if frame is None:
                raise DecodeError("SOS before SOF")
            for k in range(seg[0]):                        # a component's quantiser is the one in force at the first scan that names it
                for c, comp in enumerate(frame[2]):
                    if comp[0] == seg[1 + 2 * k] and latched[c] is None:
                        latched[c] = list(quant[comp[2]]) if comp[2] in quant else None
            _scan(jpeg, seg, ent, frame, (cx, cy, hs, vs), own, coefs, huff, dri)
            scan_ends.append(ent[1])
    if not scan_ends:
        raise DecodeError("no scan")
    w, h, comps = frame
    return dict(width=w, height=h, sampling=sampling, coefs=coefs, quant=quant, quant_ids=[c[2] for c in comps],
                quant_latched=latched, restart_interval=dri, n_scans=len(scan_ends), scan_ends=scan_ends)


def _scan(jpeg, seg, ent, frame, grid, own, coefs, huff, dri):
    w, h, comps = frame
    cx, cy, hs, vs = grid
    ns = seg[0]
    ids = {cid: k for k, (cid, _, _) in enumerate(comps)}
    members = []
    for k in range(ns):
        if seg[1 + 2 * k] not in ids:
            raise DecodeError("unknown component")
        members.append((ids[seg[1 + 2 * k]], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15))
    ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
    if ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns != 1) or al > 13 or (ah and al != ah - 1):
        raise DecodeError("band")
    if any(a[0] >= b[0] for a, b in zip(members, members[1:])):
        raise DecodeError("components out of frame order, or one named twice (B.2.3)")
    # restart intervals: cut the entropy-coded bytes at the RSTn markers
    raw = jpeg[ent[0]:ent[1]]
    pieces, a, j = [], 0, 0
    while j + 1 < len(raw):
        if raw[j] == 0xFF and 0xD0 <= raw[j + 1] <= 0xD7:
            pieces.append(raw[a:j])
            a = j + 2
            j += 2
        else:
            j += 2 if raw[j] == 0xFF else 1
    pieces.append(raw[a:])
    # the units of the scan, in order: (component, block row, block column) lists
    if ns > 1:
        def unit(u):
            my, mx = divmod(u, cx)
            out = []
            for c, _, _ in members:
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                out += [(c, my * cv + y, mx * ch + x) for y in range(cv) for x in range(ch)]
            return out
        n_units = cx * cy
    else:
        c0 = members[0][0]
        rows, cols = own[c0]

        def unit(u):
            return [(c0, u // cols, u % cols)]
        n_units = rows * cols
    tabs = {c: (td, ta) for c, td, ta in members}
    state = {"eobrun": 0}
    pred = {c: 0 for c, _, _ in members}
    bits = None

    def symbol(key):
        if key not in huff:
            raise DecodeError("undefined table")
        sym, ln = huff[key]
        p = bits.peek16()
        if ln[p] == 0:
            raise DecodeError("invalid code")
        bits.p += ln[p]
        return sym[p]

    def dc_first(blk, c):
        s = symbol((0, tabs[c][0]))
        if s > 16:
            raise DecodeError("DC category")
        pred[c] += _extend(bits.get(s), s)
        blk[0] = pred[c] << al

    def dc_refine(blk, c):
        if bits.get(1):
            blk[0] |= 1 << al

    def ac_first(blk, c):
        if state["eobrun"]:
            state["eobrun"] -= 1
            return
        k = ss
        while k <= se:
            rs = symbol((1, tabs[c][1]))
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r < 15:                                 # EOBn: this band of this block and of (1 << r) + extra - 1 more is zero
                    state["eobrun"] = (1 << r) + bits.get(r) - 1
                    return
                k += 16
                continue
            k += r
            if k > se:
                raise DecodeError("run past the band")
            blk[k] = _extend(bits.get(s), s) << al
            k += 1

    def correct(blk, k):                                   # one correction bit of an already-nonzero coefficient
        if bits.get(1) and not (abs(int(blk[k])) >> al) & 1:
            blk[k] += (1 << al) if blk[k] > 0 else -(1 << al)

    def ac_refine(blk, c):
        k = ss
        if state["eobrun"] == 0:
            while k <= se:
                rs = symbol((1, tabs[c][1]))
                r, s = rs >> 4, rs & 15
                new = 0
                if s == 1:
                    new = (1 << al) if bits.get(1) else -(1 << al)
                elif s != 0:
                    raise DecodeError("refinement magnitude")
                elif r < 15:
                    state["eobrun"] = (1 << r) + bits.get(r)
                    break
                # skip r zero-history coefficients; the nonzero ones met on the way take a correction bit each
                while k <= se:
                    if blk[k] != 0:
                        correct(blk, k)
                    else:
                        if r == 0:
                            break
                        r -= 1
                    k += 1
                if new:
                    if k > se:
                        raise DecodeError("run past the band")
                    blk[k] = new
                k += 1
        if state["eobrun"]:
            while k <= se:
                if blk[k] != 0:
                    correct(blk, k)
                k += 1
            state["eobrun"] -= 1

    step = dc_first if (ss == 0 and ah == 0) else dc_refine if ss == 0 else ac_first if ah == 0 else ac_refine
    piece = 0
    bits = _Bits(pieces[0])
    for u in range(n_units):
        if dri and u and u % dri == 0:
            piece += 1
            bits = _Bits(pieces[piece] if piece < len(pieces) else b"")
            state["eobrun"] = 0
            for c in pred:
                pred[c] = 0
        for c, by, bx in unit(u):
            step(coefs[c][by, bx], c)


def to_library_order(dec):
    """the coefficients as the library lays them out: int16 (modulo 2^16), one row of 64 per block in NATURAL order, blocks in
    MCU-interleaved scan order (luma blocks of an MCU in raster order, then Cb, Cr)"""
    from jpegdec_amd.synth import _ZIGZAG
    cx, cy, shapes, (hs, vs) = geometry(dec["width"], dec["height"], dec["sampling"])
    nc = len(shapes)
    per = hs * vs + (nc - 1)
    out = np.zeros((cy, cx, per, 64), dtype=np.int64)
    y = dec["coefs"][0].reshape(cy, vs, cx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(cy, cx, hs * vs, 64)
    out[:, :, :hs * vs, :][..., _ZIGZAG] = y
    for c in range(1, nc):
        out[:, :, hs * vs + c - 1, :][..., _ZIGZAG] = dec["coefs"][c]
    return (out.reshape(-1, 64) & 0xFFFF).astype(np.uint16).view(np.int16)
