"""A pure-Python writer of progressive (SOF2) JPEGs from chosen quantised coefficients and a chosen scan script (T.81 Annex G).

Pillow writes one script (libjpeg's default); this module writes any: DC scans interleaved or one per component, any band split,
any successive-approximation depth, Huffman table ids 0-3 with fixed or per-scan optimal tables at any length limit, and DRI, DQT
and DHT segments in front of any scan.  It shares the bit packer, the segment helper, the geometry and the table construction with
tests/coef_jpeg; the Annex G passes are written here from G.1.2 (the refinement pass buffers its correction bits and emits them
behind the next symbol, as libjpeg's encoder does; that is the only order a decoder can read them in).

  scan(components, Ss, Se, Ah, Al, **options)   one record of a script; a plain (components, Ss, Se, Ah, Al[, options]) tuple works too
      td, ta     {component: table id} of the DC / AC tables (default 0 for luma, 1 for chroma)
      huff       "default" (one fixed table per class that holds every legal symbol), "opt" (from this scan's own symbols) or an
                 int: "opt" with that length limit
      tables     {(class, id): (bits, vals)}: this scan's tables given outright (they must hold its symbols)
      define     {(class, id): (bits, vals)}: further tables to put in front of the scan
      pack       True: every table in front of this scan goes into ONE DHT segment
      dri        a DRI segment in front of the scan (0 switches restarts off)
      dqt        {table id: 64 zigzag entries}: a DQT in front of the scan; an entry above 255 makes it 16-bit
  write_progressive(...) -> bytes, or (bytes, log) with return_log: log[k] describes scan k's symbols (see _new_log)
  effective(...)        the coefficients a decoder must find after the script's scans (zero where nothing was sent)

Unit order: an interleaved scan (two or more components) walks the frame's MCU grid, h x v blocks per component; a scan of one
component walks that component's own ceil(w_c / 8) x ceil(h_c / 8) blocks in raster order (A.2.2), restart intervals counted in
those units.
"""
import functools

import numpy as np

from jpegdec_amd.synth import _codes
from tests.coef_jpeg import LUMA_HV, _BitWriter, _seg, geometry, huff_from_hist

NOT_SENT = 99


def scan(components, ss, se, ah, al, **options):
    return dict(options, comps=tuple(components), ss=ss, se=se, ah=ah, al=al)


def _norm(rec):
    if isinstance(rec, dict):
        return dict(rec)
    return scan(*rec[:5], **(rec[5] if len(rec) > 5 else {}))


@functools.lru_cache(maxsize=None)
def default_tables():
    """{class: (bits, vals)}: Annex K's luminance DC table (categories 0-11; a scan with a larger difference asks for "opt"), and an AC
    table over all 256 run/size bytes with short codes for the common symbols (what Annex K does for baseline; a progressive scan also
    needs the EOBn symbols and sizes above 10)"""
    from tests.coef_jpeg import annex_k
    hist = {}
    for r in range(16):
        for s in range(16):
            hist[(r << 4) | s] = max(1, 4096 >> r) if s == 0 else max(1, 16384 >> (s + (r + 1) // 2))
    hist[0xF0] = 64
    dc = annex_k()[2][(0, 0)]
    return {0: (list(dc[0]), list(dc[1])), 1: huff_from_hist(hist)}


def own_extent(width, height, sampling, c):
    """(block rows, block columns) of component c's own extent (A.1.1)"""
    hs, vs = LUMA_HV[sampling]
    ch, cv = (hs, vs) if c == 0 else (1, 1)
    wc, hc = -(-width * ch // hs), -(-height * cv // vs)
    return -(-hc // 8), -(-wc // 8)


def _new_log(sc):
    return dict(comps=sc["comps"], ss=sc["ss"], se=sc["se"], ah=sc["ah"], al=sc["al"], n_units=0, hist={},
                zrl=0,                     # ZRL symbols (0xF0)
                max_eob_cat=-1,            # the largest EOBn category emitted
                max_eobrun=0,
                eob_with_bits=0,           # EOB runs that carried correction bits (refinement)
                eob_cross_rows=0,          # EOB runs that span more than one row of units
                eob_by_restart=0,          # EOB runs ended by a restart
                eob_by_limit=0,            # EOB runs ended at 32767
                new_after_history=0,       # newly-nonzero coefficients whose run passed nonzero-history coefficients (refinement)
                restarts=0, max_code_len={}, dht_segments=[])


def _scan_tokens(sc, L, geo, dri, log):
    """the scan as tokens: (0, class, table id, symbol), (1, value, bit count), (2,) a restart"""
    cx, cy, hs, vs, own = geo
    comps, ss, se, ah, al = sc["comps"], sc["ss"], sc["se"], sc["ah"], sc["al"]
    toks = []
    if len(comps) > 1:
        units_x, n_units = cx, cx * cy

        def unit(u):
            my, mx = divmod(u, cx)
            out = []
            for c in comps:
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                out += [(c, my * cv + y, mx * ch + x) for y in range(cv) for x in range(ch)]
            return out
    else:
        rows, units_x = own[comps[0]]
        n_units = rows * units_x

        def unit(u):
            return [(comps[0], u // units_x, u % units_x)]
    log["n_units"] = n_units
    pred = {c: 0 for c in comps}
    eob = dict(run=0, be=[], first=0, last=0)
    ta = sc["ta"].get(comps[0], 0)

    def flush_eob(why=None):
        if eob["run"]:
            n = eob["run"].bit_length() - 1
            toks.append((0, 1, ta, n << 4))
            if n:
                toks.append((1, eob["run"] - (1 << n), n))
            log["max_eob_cat"] = max(log["max_eob_cat"], n)
            log["max_eobrun"] = max(log["max_eobrun"], eob["run"])
            log["eob_with_bits"] += bool(eob["be"])
            log["eob_cross_rows"] += eob["first"] // units_x != eob["last"] // units_x
            if why:
                log[why] += 1
            toks.extend((1, b, 1) for b in eob["be"])
            eob["run"], eob["be"] = 0, []

    def end_of_band(u, bits):
        if eob["run"] == 0:
            eob["first"] = u
        eob["run"] += 1
        eob["last"] = u
        eob["be"] += bits
        if eob["run"] == 0x7FFF:
            flush_eob("eob_by_limit")

    def dc_first(blk, c, u):
        v = blk[0] >> al                                   # the point transform: an arithmetic shift (G.1.2.1)
        d = v - pred[c]
        pred[c] = v
        s = abs(d).bit_length()
        toks.append((0, 0, sc["td"].get(c, 0), s))
        if s:
            toks.append((1, d if d >= 0 else d + (1 << s) - 1, s))

    def dc_refine(blk, c, u):
        toks.append((1, (blk[0] >> al) & 1, 1))

    def ac_first(blk, c, u):
        r = 0
        for k in range(ss, se + 1):
            t = abs(blk[k]) >> al                          # AC: the magnitude shifted, the sign kept (G.1.2.2)
            if t == 0:
                r += 1
                continue
            flush_eob()
            while r > 15:
                toks.append((0, 1, ta, 0xF0))
                log["zrl"] += 1
                r -= 16
            s = t.bit_length()
            toks.append((0, 1, ta, (r << 4) | s))
            toks.append((1, t if blk[k] > 0 else (1 << s) - 1 - t, s))
            r = 0
        if r:
            end_of_band(u, [])

    def ac_refine(blk, c, u):
        mag = [abs(blk[k]) >> al for k in range(ss, se + 1)]
        last_new = max([i for i, t in enumerate(mag) if t == 1], default=-1)
        r, br = 0, []                                      # br: correction bits waiting for the next symbol
        for i, t in enumerate(mag):
            if t == 0:
                r += 1
                continue
            while r > 15 and i <= last_new:                # ZRL only where another newly-nonzero coefficient follows
                flush_eob()
                toks.append((0, 1, ta, 0xF0))
                log["zrl"] += 1
                r -= 16
                toks.extend((1, b, 1) for b in br)
                br = []
            if t > 1:
                br.append(t & 1)
                continue
            flush_eob()
            toks.append((0, 1, ta, (r << 4) | 1))
            toks.append((1, 1 if blk[ss + i] > 0 else 0, 1))
            log["new_after_history"] += bool(br) and r > 0
            toks.extend((1, b, 1) for b in br)
            r, br = 0, []
        if r or br:
            end_of_band(u, br)

    step = dc_first if (ss == 0 and ah == 0) else dc_refine if ss == 0 else ac_first if ah == 0 else ac_refine
    for u in range(n_units):
        if dri and u and u % dri == 0:
            flush_eob("eob_by_restart")
            toks.append((2,))
            log["restarts"] += 1
            for c in pred:
                pred[c] = 0
        for c, by, bx in unit(u):
            step(L[c][by][bx], c, u)
    flush_eob()
    return toks


def _dqt(t, values):
    q = [int(x) for x in values]
    assert len(q) == 64 and all(1 <= x <= 65535 for x in q)
    if max(q) > 255:
        return _seg(0xDB, bytes([0x10 | t]) + b"".join(x.to_bytes(2, "big") for x in q))
    return _seg(0xDB, bytes([t]) + bytes(q))


def write_progressive(width, height, sampling, coefs, quant, quant_ids=None, script=(), restart_interval=0, header_quant=None,
                      pad_to=300, malform=None, return_log=False, eoi=True):
    """coefs: per component (block rows, block columns, 64) zigzag arrays over the MCU grid; quant: {id: 64 zigzag entries};
    header_quant: the ids whose DQT stands in the header (default all of quant; the others must come by a scan's dqt=), or {id: entries}
    to put other contents there than quant's;
    restart_interval: the header's DRI.  malform: {scan index: {"tokens": fn(tokens) -> tokens, "sos": fn(payload) -> payload}},
    applied to the scan's symbols before the tables are made and to the SOS payload: the error cases' byte surgery."""
    cx, cy, shapes, (hs, vs) = geometry(width, height, sampling)
    nc = len(shapes)
    assert len(coefs) == nc and all(c.shape == (r, w, 64) for c, (r, w) in zip(coefs, shapes))
    if quant_ids is None:
        quant_ids = [0] + [1 if 1 in quant else 0] * (nc - 1)
    geo = (cx, cy, hs, vs, [own_extent(width, height, sampling, c) for c in range(nc)])
    L = [np.asarray(a).tolist() for a in coefs]
    malform = malform or {}
    out = bytearray(b"\xff\xd8")
    out += _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    pad_at = len(out)
    for t in (sorted(quant) if header_quant is None else header_quant):
        out += _dqt(t, header_quant[t] if isinstance(header_quant, dict) else quant[t])
    comp = [(1, (hs << 4) | vs, quant_ids[0])] + [(2 + i, 0x11, quant_ids[1 + i]) for i in range(nc - 1)]
    out += _seg(0xC2, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc]) + b"".join(bytes(c) for c in comp))
    dri = restart_interval
    if dri:
        out += _seg(0xDD, dri.to_bytes(2, "big"))
    in_force, logs = {}, []
    for index, rec in enumerate(script):
        sc = _norm(rec)
        for key in ("td", "ta"):
            ids = sc.get(key)
            sc[key] = {c: (0 if c == 0 else 1) for c in sc["comps"]} if ids is None else dict(ids)
        log = _new_log(sc)
        if "dri" in sc:
            dri = sc["dri"]
            out += _seg(0xDD, dri.to_bytes(2, "big"))
        for t, values in sorted(sc.get("dqt", {}).items()):
            out += _dqt(t, values)
        toks = _scan_tokens(sc, L, geo, dri, log)
        if "tokens" in malform.get(index, {}):
            toks = malform[index]["tokens"](toks)
        hist = {}
        for tk in toks:
            if tk[0] == 0:
                h = hist.setdefault((tk[1], tk[2]), {})
                h[tk[3]] = h.get(tk[3], 0) + 1
        log["hist"] = hist
        how = sc.get("huff", "default")
        tables = dict(sc.get("define", {}))
        for key in sorted(hist):
            if key in sc.get("tables", {}):
                tab = sc["tables"][key]
            else:
                tab = default_tables()[key[0]] if how == "default" else huff_from_hist(hist[key], max_len=16 if how == "opt" else how)
            tab = (tuple(tab[0]), tuple(tab[1]))
            if in_force.get(key) != tab or key in tables:
                tables[key] = tab
        parts = []
        for (tc, th), (bits, vals) in sorted(tables.items()):
            in_force[(tc, th)] = (tuple(bits), tuple(vals))
            parts.append(bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals))
        if parts and sc.get("pack"):
            out += _seg(0xC4, b"".join(parts))
            log["dht_segments"].append(len(parts))
        else:
            for p in parts:
                out += _seg(0xC4, p)
                log["dht_segments"].append(1)
        sos = bytes([len(sc["comps"])]) + b"".join(bytes([comp[c][0], (sc["td"][c] << 4) | sc["ta"][c]]) for c in sc["comps"]) + \
            bytes([sc["ss"], sc["se"], (sc["ah"] << 4) | sc["al"]])
        if "sos" in malform.get(index, {}):
            sos = malform[index]["sos"](sos)
        out += _seg(0xDA, sos)
        codes = {key: _codes(*in_force[key]) for key in hist}
        bw = _BitWriter()
        rst = 0
        for tk in toks:
            if tk[0] == 0:
                code, ln = codes[(tk[1], tk[2])][tk[3]]
                log["max_code_len"][(tk[1], tk[2])] = max(log["max_code_len"].get((tk[1], tk[2]), 0), ln)
                bw.put(code, ln)
            elif tk[0] == 1:
                bw.put(tk[1], tk[2])
            else:
                bw.flush()
                bw.out += bytes([0xFF, 0xD0 + (rst & 7)])
                rst += 1
        bw.flush()
        out += bw.out
        log["end"] = len(out)                              # the file offset just behind the scan (where a file may be cut)
        logs.append(log)
    if eoi:
        out += b"\xff\xd9"
    if len(out) < pad_to:
        pad = _seg(0xFE, b"\x00" * max(pad_to - len(out) - 4, 1))
        out[pad_at:pad_at] = pad
        for log in logs:
            log["end"] += len(pad)
    return (bytes(out), logs) if return_log else bytes(out)


def effective(width, height, sampling, coefs, script):
    """what the script's scans carry: per coefficient the value truncated to the lowest bit sent (DC: arithmetic shift; AC: the
    magnitude shifted), zero where no scan reached -- bands never sent, and the AC terms of the padding blocks that a scan of one
    component does not visit.  Assumes a legal progression (every refinement follows its predecessor)."""
    cx, cy, shapes, (hs, vs) = geometry(width, height, sampling)
    low = [np.full(a.shape, NOT_SENT, dtype=np.int64) for a in coefs]
    for rec in script:
        sc = _norm(rec)
        for c in sc["comps"]:
            r, w = shapes[c] if len(sc["comps"]) > 1 else own_extent(width, height, sampling, c)
            low[c][:r, :w, sc["ss"]:sc["se"] + 1] = sc["al"]
    out = []
    for a, lo in zip(coefs, low):
        a = np.asarray(a, dtype=np.int64)
        sh = np.where(lo == NOT_SENT, 0, lo)
        v = np.sign(a) * ((np.abs(a) >> sh) << sh)
        v[..., 0] = (a[..., 0] >> sh[..., 0]) << sh[..., 0]
        out.append(np.where(lo == NOT_SENT, 0, v))
    return out
