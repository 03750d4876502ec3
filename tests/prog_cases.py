"""Inputs and expected pixels of the JPEG_PROGRESSIVE_FULL tests (CPU and GPU files share them).

A case is a smooth synthetic picture saved by Pillow twice -- progressive=True (libjpeg's default script: 10 scans with successive
approximation, 6 for gray) and as its baseline twin (same pixels, quality, sampling).  The expected pixels of the progressive file
come from a chain that never touches the library's scan decoder:

    tests/prog_jpeg.decode_coefs (pure Python)  ->  tests/coef_jpeg.write_jpeg (a baseline file, same DQT)  ->  the oracle

which gives the whole MCU-padded canvas.  The chain stands on one condition: the re-encoded baseline has no truncation event
(an artefact of the baseline bit reader that means nothing for a progressive file).  reencode() tries Huffman
tables -- Annex K, then tables made from the file's own symbol histogram at several length limits (a code of at most 7 bits
cannot be truncated: 47 + 7 + 10 <= 64) -- and returns the first file with zero events and the count; the tests ASSERT the count.
"""
import functools
import io

import numpy as np

from tests import coef_jpeg, prog_jpeg

PROGRESSIVE_FULL = 256

# name: (width, height, sampling, quality, seed, Pillow restart keyword or None)
CASES = {
    "gray_200x136_q85": (200, 136, "gray", 85, 101, None),
    "gray_17x9_q98": (17, 9, "gray", 98, 102, None),
    "gray_333x217_q50_rst": (333, 217, "gray", 50, 103, ("restart_marker_blocks", 5)),
    "c444_333x217_q85": (333, 217, "4:4:4", 85, 104, None),
    "c444_200x136_q98_rst": (200, 136, "4:4:4", 98, 105, ("restart_marker_rows", 1)),
    "c444_17x9_q50": (17, 9, "4:4:4", 50, 106, None),
    "c422_333x217_q85": (333, 217, "4:2:2", 85, 107, None),
    "c422_200x136_q50_rst": (200, 136, "4:2:2", 50, 108, ("restart_marker_blocks", 3)),
    "c422_17x9_q98": (17, 9, "4:2:2", 98, 109, None),
    "c420_640x368_q85": (640, 368, "4:2:0", 85, 110, None),
    "c420_333x217_q98": (333, 217, "4:2:0", 98, 111, None),
    "c420_200x136_q50_rst": (200, 136, "4:2:0", 50, 112, ("restart_marker_rows", 1)),
    "c420_17x9_q85_rst": (17, 9, "4:2:0", 85, 113, ("restart_marker_blocks", 1)),
}
SMALL = ("gray_17x9_q98", "c444_17x9_q50", "c422_17x9_q98", "c420_17x9_q85_rst")


def picture(width, height, seed, gray):
    """a smooth picture with a little noise: low-frequency coefficients everywhere, a few high ones"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    f = rng.uniform(5.0, 40.0, size=6)
    a = np.stack([128 + 100 * np.sin(x / f[0] + y / f[1]), 128 + 90 * np.cos(x / f[2] - y / f[3]),
                  128 + 80 * np.sin(x / f[4]) * np.cos(y / f[5])], axis=-1) + rng.normal(0, 3.0, (height, width, 3))
    from PIL import Image
    im = Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))
    return im.convert("L") if gray else im


def _save(im, sampling, quality, restart, progressive):
    kw = dict(quality=quality, progressive=progressive)
    if sampling != "gray":
        kw["subsampling"] = sampling
    if restart:
        kw[restart[0]] = restart[1]
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def files(name):
    """(progressive file, baseline twin)"""
    w, h, sampling, quality, seed, restart = CASES[name]
    im = picture(w, h, seed, sampling == "gray")
    return _save(im, sampling, quality, restart, True), _save(im, sampling, quality, restart, False)


@functools.lru_cache(maxsize=None)
def decoded(name):
    return prog_jpeg.decode_coefs(files(name)[0])


def truncation_events(jpeg):
    import jpegdec_amd as J
    p = J.PreparedImage(jpeg, flags=J.PREPARE_SERIAL_PRESCAN)
    try:
        return p.truncation_events()
    finally:
        p.close()


def reencode_coefs(dec):
    """coefficients (prog_jpeg / coef_jpeg dict) -> (baseline JPEG with the same quantisers, its truncation events)"""
    w, h, sampling = dec["width"], dec["height"], dec["sampling"]
    nc = len(dec["coefs"])
    quant = {t: dec["quant"][t] for t in sorted(set(dec["quant_ids"]))}
    first = coef_jpeg.write_jpeg(w, h, sampling, dec["coefs"], quant, quant_ids=dec["quant_ids"])
    best = (first, truncation_events(first))
    if best[1] == 0:
        return best
    hist = coef_jpeg.decode_coefs(first)["hist"]
    for max_len in (16, 12, 10, 9, 8, 7):
        try:
            huff = {key: coef_jpeg.huff_from_hist(hh, max_len=max_len) for key, hh in hist.items() if hh}
            jpeg = coef_jpeg.write_jpeg(w, h, sampling, dec["coefs"], quant, quant_ids=dec["quant_ids"], huff=huff,
                                        table_ids=[(0, 0)] + [(1, 1)] * (nc - 1))
        except Exception:
            continue                                       # (a length limit the alphabet does not fit)
        ev = truncation_events(jpeg)
        if ev < best[1]:
            best = (jpeg, ev)
        if ev == 0:
            break
    return best


@functools.lru_cache(maxsize=None)
def reencoded(name):
    return reencode_coefs(decoded(name))


def cut_after_scan(jpeg, dec, k):
    """the file cut right behind scan k's entropy-coded bytes (no EOI)"""
    return jpeg[:dec["scan_ends"][k]]


# ---- baseline fixtures fed to the coefficient kernel through jda_coef_image_from_coefficients ---------------------------------
# every layout, 8- and 16-bit quantisers, restart intervals, many DC-only blocks; the coefficient-level stress JPEGs (COEF_CASES) that
# have no truncation event: DC values at the int16 edges, the 24-bit-multiply bound's edges, the 1/4 kernel's reach, restart windows
LAYOUT_SHORT = ("gray", "c444", "c422", "c440", "c420")
BASELINE_FIXTURES = ["gray_1600x16", "gray_64x64_rst3", "c444_333x217", "c444_600x16", "c420_333x217", "c420_640x368_rstrow", "c420_250x250_q10",
                     "c422_1100x24_rstrow", "c440_300x64_rst5",
                     "w16_gray_200x120_x400", "w16_c444_136x88_x3000", "w16_c420_333x217_x400", "w16_c422_200x72_x3000", "w16_c440_120x96_x400"]
STRESS_FIXTURES = (["k_fastbound_dc_%s_%s" % (e, l) for e in ("hi", "lo") for l in LAYOUT_SHORT] + ["k_q4reach_%s_phase" % l for l in LAYOUT_SHORT] +
                   ["k_window_%s_dri" % l for l in LAYOUT_SHORT] + ["k_dcdrift_%s_%s_y_q200" % (l, v) for l in LAYOUT_SHORT for v in ("32767", "-32768")])
# the 16-bit-quantiser files whose streams DO have truncation events (uniform noise under huge quantisers): their coefficients are taken as
# the reference's reader stores them (the oracle's JPEGDecodeMCU restatement) -- what decode_coefs gives wherever there is no event
TRUNCATED_OK = ("w16_gray_200x120_x400", "w16_c420_333x217_x400")


def fixture_jpeg(name):
    from tests.cases import coef_jpeg_for, jpeg_for
    return coef_jpeg_for(name) if name.startswith("k_") else jpeg_for(name)


def fixture_coefs(name, oracle):
    """(jpeg, coefficients in the library's order) of a baseline fixture; asserts what the docstrings above promise"""
    jpeg = fixture_jpeg(name)
    events = truncation_events(jpeg)
    n, ocoefs, oflags, _, _ = oracle.entropy(jpeg)
    if name in TRUNCATED_OK:
        return jpeg, np.ascontiguousarray(ocoefs)
    assert events == 0, "%s has %d truncation events" % (name, events)
    coefs = prog_jpeg.to_library_order(coef_jpeg.decode_coefs(jpeg))
    assert n == len(coefs) and np.array_equal(ocoefs, coefs), name
    return jpeg, coefs
