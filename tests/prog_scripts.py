"""Scan scripts and coefficient sets for the progressive files that tests/prog_write.py writes (tests/prog_cases.py holds Pillow's).

A case is (coefficient set, script); its file, the writer's symbol log, the effective coefficients (what the script sends) and the
baseline twin written from those come from case(name).  NEW lists every case; PATHS names the property some cases exist for, with
the function that measures it from the writer's log -- the tests assert those, so a change to a generator cannot silently stop
exercising the path.  Everything is generated at test time.

Scripts (colour; the gray forms drop the chroma scans):
  seq           DC interleaved, one full-band AC scan per component, no successive approximation
  split_dc      DC one scan per component; AC in bands 1-1, 2-5, 6-20, 21-63, chroma before luma; optimal tables
  split_dc_lateq    .. the chroma DQT absent from the header, in front of Cb's first scan (legal: the latch picks it up)
  split_dc_swapq    .. the header's chroma DQT is all 255, the real one stands in front of Cb's first scan: a latch at the FIRST scan of the
                    file (instead of the component's first) would keep the wrong one
  split_dc_requant  .. table 0 redefined (all 255) behind Y's first scan: Y keeps what was latched
  deep_sa       DC at Al = 3 and three refinements; AC first pass at Al = 3 in bands 1-8 and 9-63, refined 3->2, 2->1, 1->0
  pair          Y-only DC scan, then Cb+Cr interleaved DC, then AC (luma with one refinement)
  missing_band  luma 6-63 never sent, Cr without any AC
  dri_moves     DRI 3 in the header, then 1, 0 (off), 7 and 5 in front of later scans; interleaved and one-component scans
  tables        all four ids of both classes defined, three DC and four AC ids used, AC id 0 redefined between two scans that use
                it, several tables in one DHT, a skewed table with 16-bit codes, a 16-bit DQT
  long_eob      gray, more than 16384 (and more than 32767) blocks in one EOB run, first pass and refinement
"""
import functools

import numpy as np

from tests import coef_jpeg, prog_write as PW
from tests.coef_jpeg import LAYOUTS, SHORT
from tests.prog_write import scan

# ---- scripts -------------------------------------------------------------------------------------------------------------
def _seq(nc, quant):
    allc = tuple(range(nc))
    return [scan(allc, 0, 0, 0, 0)] + [scan((c,), 1, 63, 0, 0) for c in allc], {}


SPLIT_BANDS = ((1, 1), (2, 5), (6, 20), (21, 63))


def _split_dc(nc, quant, variant=None):
    order = (1, 2, 0) if nc == 3 else (0,)
    s = [scan((c,), 0, 0, 0, 0, huff="opt") for c in range(nc)]
    s += [scan((c,), a, b, 0, 0, huff="opt") for a, b in SPLIT_BANDS for c in order]
    kw = {}
    if variant == "lateq":
        assert nc == 3
        kw["header_quant"] = [0]
        s[1]["dqt"] = {1: quant[1]}
    elif variant == "swapq":
        assert nc == 3
        kw["header_quant"] = {0: quant[0], 1: [255] * 64}
        s[1]["dqt"] = {1: quant[1]}
    elif variant == "requant":
        s[1]["dqt"] = {0: [255] * 64}
    return s, kw


DEEP_BANDS = ((1, 8), (9, 63))


def _deep_sa(nc, quant):
    allc = tuple(range(nc))
    s = [scan(allc, 0, 0, 0, 3)] + [scan((c,), a, b, 0, 3, huff="opt") for c in allc for a, b in DEEP_BANDS]
    for al in (2, 1, 0):
        s += [scan(allc, 0, 0, al + 1, al)] + [scan((c,), a, b, al + 1, al, huff="opt") for c in allc for a, b in DEEP_BANDS]
    return s, {}


def _pair(nc, quant):
    assert nc == 3
    return [scan((0,), 0, 0, 0, 0), scan((1, 2), 0, 0, 0, 0), scan((0,), 1, 63, 0, 1), scan((2,), 1, 63, 0, 0), scan((1,), 1, 63, 0, 0),
            scan((0,), 1, 63, 1, 0)], {}


def _missing_band(nc, quant):
    allc = tuple(range(nc))
    return [scan(allc, 0, 0, 0, 0), scan((0,), 1, 5, 0, 0)] + ([scan((1,), 1, 63, 0, 0)] if nc == 3 else []), {}


def _dri_moves(nc, quant):
    allc = tuple(range(nc))
    s = [scan(allc, 0, 0, 0, 1), scan((0,), 1, 63, 0, 1, dri=1)]
    if nc == 3:
        s += [scan((1,), 1, 63, 0, 0, dri=0), scan((2,), 1, 63, 0, 0, dri=7), scan(allc, 0, 0, 1, 0), scan((0,), 1, 63, 1, 0, dri=5)]
    else:
        s += [scan(allc, 0, 0, 1, 0, dri=0), scan((0,), 1, 63, 1, 0, dri=7)]
    return s, dict(restart_interval=3)


def _fib_table(hist):
    """a table for the symbols of `hist` under Fibonacci weights, the rarest first, filled up with unused symbols that weigh more than
    any used one: an unlimited Huffman code would be as deep as the table has symbols, so the limit of 16 binds; the first filling
    that gives one of the scan's own symbols a 16-bit code"""
    from jpegdec_amd.synth import _codes
    spare = [s for s in range(255, 0, -1) if s not in hist]
    for fill in range(64):
        a, b, w = 1, 1, {}
        for s in sorted(hist, key=lambda s: (hist[s], s)) + spare[:fill]:
            w[s] = a
            a, b = b, a + b
        table = coef_jpeg.huff_from_hist(w, max_len=16)
        if max(_codes(*table)[s][1] for s in hist) == 16:
            return table
    raise AssertionError("no 16-bit code for a used symbol")


def _tables(nc, quant):
    allc = tuple(range(nc))
    decoy = PW.default_tables()
    if nc == 3:
        s = [scan(allc, 0, 0, 0, 0, td={0: 3, 1: 1, 2: 2}, huff="opt", pack=True, define={(0, 0): decoy[0], (1, 3): decoy[1]}),
             scan((0,), 1, 10, 0, 0, ta={0: 0}, huff="opt"), scan((1,), 1, 5, 0, 0, ta={1: 1}, huff=9),
             scan((0,), 11, 63, 0, 0, ta={0: 0}, huff="opt"), scan((1,), 6, 63, 0, 0, ta={1: 2}, huff="opt"),
             scan((2,), 1, 63, 0, 0, ta={2: 3}, huff="skew")]
    else:
        s = [scan(allc, 0, 0, 0, 0, td={0: 3}, huff="opt", pack=True, define={(0, 0): decoy[0], (0, 1): decoy[0], (0, 2): decoy[0], (1, 3): decoy[1]}),
             scan((0,), 1, 3, 0, 0, ta={0: 0}, huff="opt"), scan((0,), 4, 6, 0, 0, ta={0: 1}, huff=9),
             scan((0,), 7, 10, 0, 0, ta={0: 0}, huff="opt"), scan((0,), 11, 20, 0, 0, ta={0: 2}, huff="opt"),
             scan((0,), 21, 63, 0, 0, ta={0: 3}, huff="skew")]
    return s, {}


SCRIPTS = {"seq": _seq, "split_dc": _split_dc, "split_dc_lateq": functools.partial(_split_dc, variant="lateq"),
           "split_dc_requant": functools.partial(_split_dc, variant="requant"), "split_dc_swapq": functools.partial(_split_dc, variant="swapq"), "deep_sa": _deep_sa, "pair": _pair,
           "missing_band": _missing_band, "dri_moves": _dri_moves, "tables": _tables}
# the first scan is the interleaved DC scan of every component under tables the reference accepts: without JPEG_PROGRESSIVE_FULL such a file
# gives the 1/8 thumbnail.  (tables is such a scan too, under DC table ids the reference refuses; split_dc* and pair start with Y alone.)
FIRST_SCAN_ALL_DC = ("seq", "deep_sa", "dri_moves", "missing_band")


# ---- coefficient sets ------------------------------------------------------------------------------------------------------
# (baseline fixture, width, height): the top-left blocks of the fixture's coefficients, at sizes that leave the last block column and
# row of luma partly or wholly outside the picture (a scan of one component does not visit the wholly-outside ones)
FIXTURE_SETS = {"gray": ("gray_64x64_rst3", 61, 43), "4:4:4": ("c444_333x217", 83, 41), "4:2:2": ("c422_1100x24_rstrow", 83, 21),
                "4:4:0": ("c440_300x64_rst5", 83, 35), "4:2:0": ("c420_333x217", 83, 41)}
K_SETS = (["k_fastbound_dc_%s_%s" % (e, SHORT[l]) for e in ("hi", "lo") for l in LAYOUTS] + ["k_q4reach_%s_phase" % SHORT[l] for l in LAYOUTS] +
          ["k_dcdrift_%s_%s_y_q200" % (SHORT[l], v) for l in LAYOUTS for v in ("32767", "-32768")])
RND_SIZE = {"gray": (61, 43), "4:4:4": (45, 37), "4:2:2": (75, 37), "4:4:0": (45, 53), "4:2:0": (75, 53)}


def _fixture_set(sampling):
    from tests.cases import jpeg_for
    src, w, h = FIXTURE_SETS[sampling]
    dec = coef_jpeg.decode_coefs(jpeg_for(src))
    assert dec["sampling"] == sampling
    shapes = coef_jpeg.geometry(w, h, sampling)[2]
    coefs = [np.array(a[:r, :c]) for a, (r, c) in zip(dec["coefs"], shapes)]
    return dict(width=w, height=h, sampling=sampling, coefs=coefs, quant=dec["quant"], quant_ids=dec["quant_ids"])


def _random_set(sampling):
    """sparse blocks made for the refinement passes of deep_sa (first pass at Al = 3, bands 1-8 and 9-63): in band 9-63 a few coefficients
    of magnitude 8 or more (nonzero from the first pass on: they take a correction bit in every refinement), and further apart than 16
    zero-history positions coefficients of magnitude 4-7, 2-3 and 1, which become nonzero in the refinements 3->2, 2->1 and 1->0: ZRLs
    with correction bits on the way, new +-1s behind runs that pass nonzero history.  Blocks with history only, and empty blocks, make
    EOB runs that carry correction bits.  Signs and low bits are random."""
    w, h = RND_SIZE[sampling]
    rng = np.random.default_rng(7000 + LAYOUTS.index(sampling))
    coefs = coef_jpeg.zero_coefs(w, h, sampling)

    def mag(lo, hi):
        return int(rng.integers(lo, hi + 1)) * (1 if rng.integers(0, 2) else -1)

    for ci, arr in enumerate(coefs):
        flat = arr.reshape(-1, 64)
        dc = 0
        for i in range(flat.shape[0]):
            dc = max(-1000, min(1000, dc + int(rng.integers(-90, 91))))
            flat[i, 0] = dc
            kind = int(rng.integers(0, 8))
            if kind <= 1:
                continue                                   # DC only
            if kind <= 3:                                  # history only
                for k in rng.choice(np.arange(1, 64), size=int(rng.integers(1, 5)), replace=False):
                    flat[i, k] = mag(8, 120)
                continue
            if kind == 4:                                  # sparse, anything
                for k in rng.choice(np.arange(1, 64), size=int(rng.integers(1, 7)), replace=False):
                    flat[i, k] = mag(1, 40)
                continue
            j = int(rng.integers(0, 3))
            for k in (10 + j, 19 + j, 33 + j):
                flat[i, k] = mag(8, 200)
            flat[i, 41 + j] = mag(4, 7)                    # 29 zero-history positions in front of it
            flat[i, 62] = mag(2, 3)                        # 20 more
            if kind >= 6:
                flat[i, 61 - 2 * j] = mag(1, 1)
                flat[i, 2 + j] = mag(8, 60)
                flat[i, 8] = mag(1, 7)
    return dict(width=w, height=h, sampling=sampling, coefs=coefs, quant={0: coef_jpeg.annex_k()[0].tolist(), 1: coef_jpeg.annex_k()[1].tolist()},
                quant_ids=[0] + [1] * (len(coefs) - 1))


def _k_set(name):
    from tests.cases import coef_spec
    spec = coef_spec(name)
    nc = len(spec["coefs"])
    return dict(width=spec["width"], height=spec["height"], sampling=spec["sampling"], coefs=spec["coefs"], quant=spec["quant"],
                quant_ids=spec.get("quant_ids") or [0] + [1 if 1 in spec["quant"] else 0] * (nc - 1))


def _with_word_quant(cs):
    """the set under a luma quantiser whose upper half is above 255: a 16-bit DQT (Pq = 1)"""
    q = {t: list(v) for t, v in cs["quant"].items()}
    q[0] = [int(x) if k < 32 else 256 + 8 * k + int(x) for k, x in enumerate(q[0])]
    return dict(cs, quant=q)


LONG_EOB = {"long_eob_16512": (1032, 1024), "long_eob_32896": (2056, 1024)}


def _long_eob_set(w, h):
    """gray, everything zero but the DC of a few blocks and, in the LAST block, AC terms 3 (value 2: sent as 1 at Al = 1, a correction
    bit in the refinement) and 5 (value 1: newly nonzero in the refinement)"""
    coefs = coef_jpeg.zero_coefs(w, h, "gray")
    coefs[0][0, 0, 0] = 40
    coefs[0][-1, -1, 0] = -30
    coefs[0][-1, -1, 3] = 2
    coefs[0][-1, -1, 5] = -1
    return dict(width=w, height=h, sampling="gray", coefs=coefs, quant={0: [16] * 64}, quant_ids=[0])


LONG_EOB_SCRIPT = [scan((0,), 0, 0, 0, 0), scan((0,), 1, 63, 0, 1, huff="opt"), scan((0,), 1, 63, 1, 0, huff="opt")]


@functools.lru_cache(maxsize=None)
def coef_set(name):
    if name.startswith("fx_"):
        return _fixture_set({SHORT[l]: l for l in LAYOUTS}[name[3:]])
    if name.startswith("rnd_"):
        return _random_set({SHORT[l]: l for l in LAYOUTS}[name[4:]])
    if name.startswith("fxflat_"):
        # libjpeg smooths a component whose low AC terms never came (jdcoefct.c, decompress_smooth_data: they are estimated from the
        # neighbours' DC differences).  With Cr's DC constant the estimate is zero, and Pillow decodes the file to the baseline twin's pixels
        cs = _fixture_set({SHORT[l]: l for l in LAYOUTS}[name[7:]])
        coefs = [np.array(a) for a in cs["coefs"]]
        coefs[2][..., 0] = 12
        return dict(cs, coefs=coefs)
    if name.startswith("w16fx_"):
        return _with_word_quant(_fixture_set({SHORT[l]: l for l in LAYOUTS}[name[6:]]))
    return _k_set(name)


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _cases():
    S = [SHORT[l] for l in LAYOUTS]
    colour = [s for s in S if s != "gray"]
    new = {}

    def add(cs, script):
        new["%s__%s" % (cs, script)] = (cs, script)

    for s in S:
        add("fx_" + s, "seq")
        add("fx_" + s, "split_dc")
        add("fx_" + s, "deep_sa")
        add("rnd_" + s, "deep_sa")
        add(("fx_" if s == "gray" else "fxflat_") + s, "missing_band")
        add("fx_" + s, "dri_moves")
        add("rnd_" + s, "dri_moves")
        add("w16fx_" + s, "tables")
    add("rnd_c420", "split_dc")
    for s in ("c444", "c440", "c420"):
        add("fx_" + s, "split_dc_lateq")
    for s in ("gray", "c422"):
        add("fx_" + s, "split_dc_requant")
    for s in ("c444", "c422"):
        add("fx_" + s, "split_dc_swapq")
    for s in colour:
        add("fx_" + s, "pair")
    add("rnd_c420", "pair")
    for k in K_SETS:
        add(k, "seq")
        add(k, "deep_sa")
    return new


NEW = _cases()
NAMES = sorted(NEW)
LONG_NAMES = sorted(LONG_EOB)
ONE_PER_LAYOUT = ["rnd_gray__deep_sa", "fx_c444__split_dc_lateq", "fx_c422__pair", "fx_c440__deep_sa", "rnd_c420__dri_moves"]

# Pillow (libjpeg) is the third party that decodes every written file to the pixels of the baseline file written from the same effective
# coefficients.  Exempt: only DC-edge sets, whose samples libjpeg's range limiting may treat differently in the two files' decoders
# (the progressive decoder's block smoothing is off when every band was sent; kept as a list so that a test can bound it)
PILLOW_EXEMPT = ()
PILLOW_EXEMPT_ALLOWED = tuple(n for n in NAMES if n.startswith(("k_fastbound_dc_", "k_dcdrift_"))) + tuple(LONG_NAMES)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(jpeg, log, set, script, kwargs, effective, twin): twin = coef_jpeg.write_jpeg of the effective coefficients, None where a
    baseline file cannot carry them (a DC difference above category 11 or an AC value above category 10)"""
    if name in LONG_EOB:
        cs, (script, kw) = _long_eob_set(*LONG_EOB[name]), (LONG_EOB_SCRIPT, {})
    else:
        cs = coef_set(NEW[name][0])
        script, kw = SCRIPTS[NEW[name][1]](len(cs["coefs"]), cs["quant"])
    script = _resolve_skew(cs, script, kw)
    jpeg, log = PW.write_progressive(cs["width"], cs["height"], cs["sampling"], cs["coefs"], cs["quant"], cs["quant_ids"], script,
                                     return_log=True, **kw)
    eff = PW.effective(cs["width"], cs["height"], cs["sampling"], cs["coefs"], script)
    try:
        twin = coef_jpeg.write_jpeg(cs["width"], cs["height"], cs["sampling"], eff, {t: cs["quant"][t] for t in sorted(set(cs["quant_ids"]))},
                                    quant_ids=cs["quant_ids"])
    except (AssertionError, KeyError):
        twin = None
    return dict(jpeg=jpeg, log=log, set=cs, script=script, kwargs=kw, effective=eff, twin=twin)


# ---- the same accessors as tests/prog_cases.py, over Pillow's cases and the written ones ------------------------------------------------
def files(name):
    """(progressive file, baseline twin)"""
    from tests import prog_cases as PC
    if name in PC.CASES:
        return PC.files(name)
    c = case(name)
    return c["jpeg"], c["twin"]


@functools.lru_cache(maxsize=None)
def decoded(name):
    from tests import prog_cases as PC, prog_jpeg
    if name in PC.CASES:
        return PC.decoded(name)
    dec = prog_jpeg.decode_coefs(case(name)["jpeg"])
    # the quantisers a decoder applies are the latched ones (a table may be redefined behind a component's first scan)
    quant = {}
    for c, t in enumerate(dec["quant_ids"]):
        q = dec["quant_latched"][c] or dec["quant"][t]
        assert quant.setdefault(t, q) == q, "two components latched different contents of table %d" % t
    return dict(dec, quant=quant)


@functools.lru_cache(maxsize=None)
def reencoded(name):
    from tests import prog_cases as PC
    return PC.reencoded(name) if name in PC.CASES else PC.reencode_coefs(decoded(name))


def _resolve_skew(cs, script, kw):
    """huff="skew": the scan's own symbols under Fibonacci weights (a first write gives the histogram)"""
    if not any(sc.get("huff") == "skew" for sc in script):
        return script
    first = [dict(sc, huff="opt") if sc.get("huff") == "skew" else sc for sc in script]
    log = PW.write_progressive(cs["width"], cs["height"], cs["sampling"], cs["coefs"], cs["quant"], cs["quant_ids"], first, return_log=True, **kw)[1]
    out = []
    for sc, lg in zip(script, log):
        if sc.get("huff") == "skew":
            sc = dict(sc, huff="opt", tables={key: _fib_table(h) for key, h in lg["hist"].items()})
        out.append(sc)
    return out


def malformed():
    """{name: file}: files a decoder must refuse (JDA_DECODE_ERROR), all made from fx_c420 by the writer's malform hook"""
    cs = coef_set("fx_c420")
    nc = 3

    def write(script, malform=None, **kw):
        return PW.write_progressive(cs["width"], cs["height"], cs["sampling"], cs["coefs"], cs["quant"], cs["quant_ids"], script, malform=malform, **kw)

    def first_symbol(pred, change):
        def fn(toks):
            for i, tk in enumerate(toks):
                if tk[0] == 0 and tk[1] == 1 and pred(tk[3]):
                    sym, nbits = change(tk[3])
                    out = list(toks)
                    out[i] = (0, 1, tk[2], sym)
                    if nbits is not None:
                        out[i + 1] = (1, 0, nbits)
                    return out
            raise AssertionError("no such symbol in the scan")
        return fn

    deep = _deep_sa(nc, cs["quant"])[0]
    k_ref = [i for i, sc in enumerate(deep) if sc["ss"] == 1 and sc["ah"] == 3][0]           # the first refinement of Y's band 1-8
    k_first = [i for i, sc in enumerate(deep) if sc["ss"] == 1 and sc["ah"] == 0][0]
    seq = _seq(nc, cs["quant"])[0]
    pair = _pair(nc, cs["quant"])[0]

    def sos_tables(k, td, ta):                             # component k of the scan names tables td, ta
        def fn(p):
            p = bytearray(p)
            p[2 + 2 * k] = (td << 4) | ta
            return bytes(p)
        return fn

    def sos_ids(*ids):
        def fn(p):
            p = bytearray(p)
            for k, v in enumerate(ids):
                p[1 + 2 * k] = v
            return bytes(p)
        return fn

    return {
        "refinement_size_2": write(deep[:k_ref + 1], {k_ref: {"tokens": first_symbol(lambda s: s & 15 == 1, lambda s: (s + 1, 2))}}),
        "first_pass_run_past_se": write(deep[:k_first + 1], {k_first: {"tokens": first_symbol(lambda s: s & 15, lambda s: (0xF0 | (s & 15), None))}}),
        "refinement_run_past_se": write(deep[:k_ref + 1], {k_ref: {"tokens": first_symbol(lambda s: s & 15 == 1, lambda s: (0xF1, None))}}),
        "al_14": write([scan((0, 1, 2), 0, 0, 0, 14)]),
        "undefined_dc_table": write(seq, {0: {"sos": sos_tables(1, 2, 1)}}),
        "undefined_ac_table": write(seq, {1: {"sos": sos_tables(0, 0, 3)}}),
        "out_of_frame_order": write(pair, {1: {"sos": sos_ids(3, 2)}}),
        "component_twice": write(pair, {1: {"sos": sos_ids(2, 2)}}),
    }


def wrap_case():
    """(file, coefficients) of an AC first pass whose value << Al leaves int16: 5000 << 3 and -20000 << 1 (coefficient level only)"""
    cs = _long_eob_set(24, 16)
    coefs = [np.array(cs["coefs"][0])]
    coefs[0][0, 1, 4] = 40000
    coefs[0][1, 2, 9] = -40000
    coefs[0][1, 0, 7] = 32767
    script = [scan((0,), 0, 0, 0, 0), scan((0,), 1, 5, 0, 3, huff="opt"), scan((0,), 6, 63, 0, 1, huff="opt")]
    return PW.write_progressive(24, 16, "gray", coefs, cs["quant"], [0], script), PW.effective(24, 16, "gray", coefs, script)


# ---- the paths the cases exist for: name -> (case, measure(log) -> value, predicate) ----------------------------------------------------
def _refine(log):
    return [lg for lg in log if lg["ss"] > 0 and lg["ah"] > 0]


PATHS = {
    "zrl_in_refinement": ("rnd_c420__deep_sa", lambda log: sum(lg["zrl"] for lg in _refine(log)), lambda v: v > 0),
    "new_after_history": ("rnd_c420__deep_sa", lambda log: sum(lg["new_after_history"] for lg in _refine(log)), lambda v: v > 0),
    "refinement_eob_runs_with_bits": ("rnd_c420__deep_sa", lambda log: sum(lg["eob_with_bits"] for lg in _refine(log)), lambda v: v > 0),
    "zrl_in_refinement_440": ("rnd_c440__deep_sa", lambda log: sum(lg["zrl"] for lg in _refine(log)), lambda v: v > 0),
    "eob_runs_cross_rows": ("fx_c420__deep_sa", lambda log: sum(lg["eob_cross_rows"] for lg in log), lambda v: v > 0),
    "eob_runs_ended_by_restart": ("rnd_c420__dri_moves", lambda log: sum(lg["eob_by_restart"] for lg in log), lambda v: v > 0),
    "eob_category_14_first_pass": ("long_eob_16512", lambda log: log[1]["max_eob_cat"], lambda v: v == 14),
    "eob_category_14_refinement": ("long_eob_16512", lambda log: log[2]["max_eob_cat"], lambda v: v == 14),
    "eob_run_split_at_32767": ("long_eob_32896", lambda log: (log[1]["eob_by_limit"], log[2]["eob_by_limit"], log[1]["max_eobrun"]), lambda v: v == (1, 1, 32767)),
    "sixteen_bit_code_used": ("w16fx_c420__tables", lambda log: max(max(lg["max_code_len"].values()) for lg in log), lambda v: v == 16),
    "sixteen_bit_code_used_gray": ("w16fx_gray__tables", lambda log: max(max(lg["max_code_len"].values()) for lg in log), lambda v: v == 16),
    "tables_per_dht_segment": ("w16fx_c420__tables", lambda log: max(max(lg["dht_segments"], default=0) for lg in log), lambda v: v >= 2),
    "restart_interval_in_blocks": ("fx_c420__dri_moves", lambda log: [(lg["n_units"], lg["restarts"]) for lg in log], lambda v: v[1][0] != v[0][0] and v[1][1] == v[1][0] - 1 and v[-1][1] == (v[-1][0] - 1) // 5),
}
