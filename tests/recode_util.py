"""Cases and comparators of the lossless recode (jda_recode_images), shared by tests/test_recode_cpu.py (the stages lane by
lane on the CPU) and tests/test_gpu_recode.py.

Pillow is the third party for every direction: its baseline, optimize=True, progressive=True and restart_marker_blocks= files of one
picture carry the same coefficients and the same bytes in front of SOF, so recoding any of them to another form must give Pillow's file of
that form -- held under the comparators the encoder's tests use (the DHT segments and everything behind the SOS header for a baseline or
optimised file, SOF2 to EOI for a progressive one), and the bytes in front of SOF must be the source's.
One deliberate weakening: for a BASELINE target the four DHT segments are compared as a set, not in the file's order.  They are the Annex K
tables in both files, but the encoder's baseline header lists them DC 0, DC 1, AC 0, AC 1 (every baseline file it writes does, and those
bytes may not change) where Pillow lists them component by component.  An optimised target's DHT segments are compared in file order; the
frame header, the whole scan and the bytes in front of SOF are compared exactly in every form.

Written sources (tests/coef_jpeg.write_jpeg, tests/prog_write.py) put chosen coefficients under chosen tables: the recoded file is read
back by the suite's own decoders (coef_jpeg.decode_coefs / prog_jpeg.decode_coefs, which share no code with the library) and must give the
source's coefficients, coefficient for coefficient, and its quantisers, component for component.

A file under 256 bytes is no source: the front end refuses it, as the reference does."""
import functools
import io

import numpy as np

from jpegdec_amd.synth import _ZIGZAG
from tests import cases, coef_jpeg, prog_jpeg, prog_write
from tests import encode_opt_util as O
from tests import encode_util as E

FORMS = ("baseline", "optimize", "progressive")
FORM_ID = {"baseline": 0, "optimize": 1, "progressive": 2}
SUCCESS, INVALID_PARAMETER, DECODE_ERROR, UNSUPPORTED, ERROR_MEMORY = 0, 1, 2, 3, 5
PILLOW_RESTART = 3                                    # restart_marker_blocks of the fourth Pillow file


# ---- Pillow sources ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pillow_files(kind, w, h, sampling, q=75):
    """{"baseline", "optimize", "progressive", "restart"}: Pillow's four files of encode_util.picture(kind, w, h, sampling)"""
    from PIL import Image
    img = E.picture(kind, w, h, sampling)
    im = Image.fromarray(img) if sampling == "gray" else Image.fromarray(np.ascontiguousarray(img[..., :3]))
    kw = {} if sampling == "gray" else dict(subsampling=E.PILLOW_SUBSAMPLING[sampling])
    out = {}
    for name, extra in (("baseline", {}), ("optimize", dict(optimize=True)), ("progressive", dict(progressive=True)), ("restart", dict(restart_marker_blocks=PILLOW_RESTART))):
        b = io.BytesIO()
        im.save(b, "JPEG", quality=q, **kw, **extra)
        out[name] = b.getvalue()
    return out


# (picture, w, h, sampling): a one-MCU image of every layout, the 333 x 217 of the fixtures, and 136 x 88 at 4:2:0 -- 324 blocks, so that a
# workgroup of 256 lanes straddles two jobs wherever it stands in a call
PILLOW_SHAPES = (("noise", 8, 8, "gray"), ("noise", 8, 8, "4:4:4"), ("noise", 16, 8, "4:2:2"), ("noise", 16, 16, "4:2:0"), ("smooth", 17, 9, "4:2:0"),
                 ("noise", 136, 88, "4:2:0"), ("noise", 333, 217, "gray"), ("smooth", 333, 217, "4:4:4"), ("noise", 333, 217, "4:2:2"), ("noise", 333, 217, "4:2:0"))


def pillow_jobs(colour, sources=("baseline", "optimize", "progressive", "restart")):
    """[(source file, the Pillow files of its picture)] of the gray (colour False) or the colour shapes: every Pillow file the front end takes"""
    out = []
    for shape in PILLOW_SHAPES:
        if (shape[3] != "gray") != colour:
            continue
        files = pillow_files(*shape)
        out += [(files[s], files) for s in sources if len(files[s]) >= 256]
    return out


def want_of(files, form, restart_interval):
    """Pillow's file a recode to (form, restart_interval) must give, or None where Pillow wrote none with that interval"""
    if form == "progressive":
        return files["progressive"]
    if form == "optimize":
        return files["optimize"] if restart_interval == 0 else None
    return files["baseline"] if restart_interval == 0 else files["restart"] if restart_interval == PILLOW_RESTART else None


def _segments_to_sof(jpeg):
    i = 2
    while jpeg[i + 1] not in (0xC0, 0xC2):
        assert jpeg[i] == 0xFF
        i += 2 + int.from_bytes(jpeg[i + 2:i + 4], "big")
    return i


def front(jpeg):
    """the bytes in front of the frame header"""
    return jpeg[:_segments_to_sof(jpeg)]


def frame_header(jpeg):
    i = _segments_to_sof(jpeg)
    return jpeg[i:i + 2 + int.from_bytes(jpeg[i + 2:i + 4], "big")]


def body(jpeg):
    return jpeg[coef_jpeg._parse(jpeg)[5]:]


def from_sof2(f):
    return f[f.index(b"\xff\xc2"):]


def is_pillow(got, want, form, source=None):
    """got is Pillow's file `want` under the comparator of its form; with source: the bytes in front of SOF are the source's"""
    assert got[:2] == b"\xff\xd8" and got[-2:] == b"\xff\xd9"
    if form == "progressive":
        assert from_sof2(got) == from_sof2(want), "SOF2 to EOI"
    else:
        if form == "optimize":
            assert O.dht_segments(got) == O.dht_segments(want), "the DHT segments, in the file's order"
        else:       # (the Annex K tables: the encoder lists them DC 0, DC 1, AC 0, AC 1, Pillow component by component -- the same four tables)
            assert sorted(O.dht_segments(got)) == sorted(O.dht_segments(want)), "the DHT segments"
        assert body(got) == body(want), "the bytes behind the SOS header"
        assert frame_header(got) == frame_header(want), "the frame header"
    assert front(got) == front(want if source is None else source), "the bytes in front of SOF"


# ---- coefficients -----------------------------------------------------------------------------------------------------------------
def decode_any(jpeg):
    """coef_jpeg.decode_coefs of a baseline file, prog_jpeg.decode_coefs of a progressive one: dict(coefs, quant, quant_ids, ...)"""
    sof = jpeg[_segments_to_sof(jpeg) + 1]
    return prog_jpeg.decode_coefs(jpeg) if sof == 0xC2 else coef_jpeg.decode_coefs(jpeg)


def same_coefficients(src, out):
    """the recoded file carries the source's coefficients, coefficient for coefficient, and its quantisers, component for component"""
    a, b = decode_any(src), decode_any(out)
    assert (a["width"], a["height"], a["sampling"]) == (b["width"], b["height"], b["sampling"])
    prog = frame_header(out)[1] == 0xC2 and frame_header(src)[1] != 0xC2
    for c, (x, y) in enumerate(zip(a["coefs"], b["coefs"])):
        if prog:
            # A progressive file's AC scans hold one component each, and such a scan visits the component's OWN extent (T.81 A.2.2): the AC
            # coefficients of the MCU grid's padding blocks have no place in the format (jpegtran drops them too).  The DC scan is interleaved
            # and keeps every block's.  A written source fills the padding blocks; a picture's are (DC, zeros), so Pillow's files lose nothing.
            rows, cols = prog_write.own_extent(a["width"], a["height"], a["sampling"], c)
            x = x.copy()
            x[rows:, :, 1:] = 0
            x[:, cols:, 1:] = 0
        assert np.array_equal(x, y), ("coefficients of component", c, int(np.count_nonzero(x != y)))
    for c, (i, k) in enumerate(zip(a["quant_ids"], b["quant_ids"])):
        assert i == k and list(a["quant"][i]) == list(b["quant"][k]), ("quantiser of component", c)


def flat_zigzag(dec):
    """(blocks, 64) int64 in zig-zag order, the blocks in the order of the interleaved scan: what the stage leaves in `coef`"""
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(dec["width"], dec["height"], dec["sampling"])
    nc = len(shapes)
    out = np.zeros((cy, cx, hs * vs + nc - 1, 64), dtype=np.int64)
    out[:, :, :hs * vs] = dec["coefs"][0].reshape(cy, vs, cx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(cy, cx, hs * vs, 64)
    for c in range(1, nc):
        out[:, :, hs * vs + c - 1] = dec["coefs"][c]
    return out.reshape(-1, 64), hs * vs, nc


@functools.lru_cache(maxsize=None)
def _annex_k_lengths():
    huff = coef_jpeg.annex_k()[2]
    out = []
    for t in (0, 1):
        bits, vals = huff[(1, t)]
        ln, k = {}, 0
        for n in range(1, 17):
            for _ in range(bits[n - 1]):
                ln[vals[k]] = n
                k += 1
        out.append(ln)
    return out


def twin_meta(dec):
    """the block words the stage leaves beside the coefficients: (AC code bits under the Annex K table of the block's class << 16) | DC"""
    flat, nl, nc = flat_zigzag(dec)
    per = nl + nc - 1
    lengths = _annex_k_lengths()
    meta = np.zeros(flat.shape[0], dtype=np.uint32)
    for b, zz in enumerate(flat):
        ln = lengths[0 if b % per < nl else 1]
        bits, run = 0, 0
        for v in zz[1:]:
            if v == 0:
                run += 1
                continue
            s = int(abs(int(v))).bit_length()
            bits += (run >> 4) * ln[0xF0] + ln[((run & 15) << 4) | s] + s
            run = 0
        if run:
            bits += ln[0x00]
        meta[b] = (bits << 16) | (int(zz[0]) & 0xFFFF)
    return flat, meta


@functools.lru_cache(maxsize=None)
def twin_of(jpeg):
    """twin_meta(decode_any(jpeg)), once a file: the pure-Python decoders take their time"""
    return twin_meta(decode_any(jpeg))


# ---- written sources --------------------------------------------------------------------------------------------------------------
def _in_range(spec, ri=0):
    """a copy of a coefficient case of tests/cases.py with its DC values at both ends of the recode's range and in between (-1024, 1023, 0, 5,
    ..: differences of 2047, category 11), the rest as it is: every AC symbol of a baseline table (category 10 included), ZRL chains, blocks full
    to coefficient 63"""
    d = dict(spec)
    d["coefs"] = [c.copy() for c in spec["coefs"]]
    ramp = np.array([-1024, 1023, 0, 5, -1024, -3, 1023, 1023, 512], dtype=np.int64)
    for c, arr in enumerate(d["coefs"]):
        flat = arr.reshape(-1, 64)
        flat[:, 0] = ramp[(np.arange(flat.shape[0]) + c) % len(ramp)]
    if ri:
        d["restart_interval"] = ri
    return d


def _small(sampling, quant, quant_ids=None, seed=3, w=24, h=16):
    rng = np.random.default_rng(seed)
    coefs = coef_jpeg.zero_coefs(w, h, sampling)
    for arr in coefs:
        arr[...] = rng.integers(-40, 41, arr.shape) * (rng.random(arr.shape) < 0.3)
        arr[..., 0] = rng.integers(-1024, 1024, arr.shape[:2])
    d = dict(width=w, height=h, sampling=sampling, coefs=coefs, quant=quant)
    if quant_ids is not None:
        d["quant_ids"] = quant_ids
    return d


@functools.lru_cache(maxsize=None)
def written_specs():
    """{name: write_jpeg's arguments}"""
    out = {}
    for lay in E.SAMPLINGS:
        s = coef_jpeg.SHORT[lay]
        out["huff_custom_" + s] = _in_range(cases.coef_spec("k_huff_custom_" + s))       # 16-bit codes, custom tables under ids 0 and 1
    out["huff_annexk_c420"] = _in_range(cases.coef_spec("k_huff_annexk_c420"))
    q3 = {0: list(range(1, 65)), 1: [7] * 64, 2: list(range(64, 0, -1))}
    out["three_quantisers"] = _small("4:4:4", q3, [0, 1, 2])
    out["ids_2_and_3"] = _small("4:2:0", {2: [3] * 64, 3: [9] * 64}, [2, 3, 3], seed=4)
    out["one_table_for_all"] = _small("4:2:2", {0: [5] * 64}, [0, 0, 0], seed=5)
    out["quant16"] = _small("4:2:0", {0: [300 + i for i in range(64)], 1: [2] * 64}, seed=6)
    out["quant16_gray"] = _small("gray", {0: [1000] * 63 + [255]}, seed=7)
    return out


@functools.lru_cache(maxsize=None)
def written(name):
    return coef_jpeg.write_jpeg(**written_specs()[name])


def restart_sources():
    """[(file, its MCU count, MCUs in a row)]: k_huff_annexk at 4:2:0 with intervals of 1, of an MCU row, and one that does not divide the MCU count"""
    spec = _in_range(cases.coef_spec("k_huff_annexk_c420"))
    cx, cy = coef_jpeg.geometry(spec["width"], spec["height"], spec["sampling"])[:2]
    assert (cx * cy) % 7 != 0
    return [(coef_jpeg.write_jpeg(**dict(spec, restart_interval=ri)), cx * cy, cx) for ri in (1, cx, 7)]


RESTART_TARGETS = (None, 0, 5)                        # the source's own, none, another


@functools.lru_cache(maxsize=None)
def written_progressive():
    """a progressive source from chosen coefficients under a script of its own (tests/prog_write.py): spectral selection only, three quantisers"""
    d = _small("4:4:4", {0: list(range(1, 65)), 1: [7] * 64, 2: [300] * 64}, [0, 1, 2], seed=9, w=40, h=24)
    script = [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]
    return prog_write.write_progressive(d["width"], d["height"], d["sampling"], d["coefs"], d["quant"], d["quant_ids"], script=script)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _with_symbol_11():
    hist = {s: 1 for s in coef_jpeg.AC_SYMBOLS}
    hist[0x0B] = 1
    huff = dict(coef_jpeg.annex_k()[2])
    huff[(1, 0)] = coef_jpeg.huff_from_hist(hist)
    return huff


@functools.lru_cache(maxsize=None)
def refused():
    """{name: (file, the status its job must get)}: a block outside the range, a layout the encoder lacks, an Adobe segment, a bad MCU"""
    from tests import orient_util
    out = {}
    d = _small("4:2:0", {0: [1] * 64, 1: [1] * 64}, seed=21)
    d["huff"] = _with_symbol_11()
    d["ac_pairs"] = {(0, 1, 2): [(0, 1024), (0, 0)]}                      # (the symbols as given: the value, then EOB)
    out["ac_1024"] = (coef_jpeg.write_jpeg(**d), UNSUPPORTED)
    d = _small("4:2:0", {0: [1] * 64, 1: [1] * 64}, seed=22)
    d["coefs"][0][...] = 0
    d["coefs"][0][0, 1, 0] = 1024
    out["dc_1024"] = (coef_jpeg.write_jpeg(**d), UNSUPPORTED)
    d = _small("4:2:0", {0: [1] * 64, 1: [1] * 64}, seed=23)
    d["coefs"][1][...] = 0
    d["coefs"][1][0, 0, 0] = -1025
    out["dc_minus_1025"] = (coef_jpeg.write_jpeg(**d), UNSUPPORTED)
    out["c440"] = (coef_jpeg.write_jpeg(**_small("4:4:0", {0: [2] * 64, 1: [3] * 64}, seed=24)), UNSUPPORTED)
    base = written("three_quantisers")
    at = 2 + 2 + int.from_bytes(base[4:6], "big")                              # behind APP0
    out["adobe"] = (base[:at] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + base[at:], UNSUPPORTED)
    out["bad_mcu"] = (orient_util.bad_mcu_jpeg()[0], DECODE_ERROR)
    return out
