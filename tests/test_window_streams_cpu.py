"""The scan-window stress streams (k_window_*, k_q4reach_* in tests/cases.py) without a GPU.

A tile stages bytes [win_lo, hi) of the filtered scan in its wavefront's LDS window (jda_tile_setup_from); a tile whose win_need
is over the layout's WIN_BYTES takes the general reader, which reads past the staged bytes from HBM.  The corpus puts tiles at
exactly W - 16, W, W + 16 and W + 32 of both layouts' windows, tight (no spare byte behind the +8+12 reach) and loose, at the end
of the scan (hi clamped), at a row's partial tile, behind a restart, with a truncated magnitude read in the last block; and blocks
that fill the 1/4 kernel's five dwords at every bit phase and at the scan's end.  First the corpus is held to what it claims,
from the product's own block index, then the wave emulator runs every case at the real window sizes, over LDS poisoned with three
different bytes, and must give the oracle's pixels each time."""
import ctypes as C
import math

import numpy as np
import pytest

import jpegdec_amd as J
from tests import coef_jpeg as cj
from tests.cases import (COEF_CASES, Q4REACH_VARIANTS, WINDOW_KINDS, _NBLK, _window_plan, coef_jpeg_for, coef_spec,
                         lds_layout)

MODE = {"gray": 0, "4:4:4": 1, "4:2:0": 2, "4:2:2": 3, "4:4:0": 4}              # JDA_MODE_*
SAMPLING = {v: k for k, v in cj.SHORT.items()}
WINDOW = sorted(k for k in COEF_CASES if k.startswith("k_window_"))
Q4REACH = sorted(k for k in COEF_CASES if k.startswith("k_q4reach_"))
SCAN_PAD = 32                                                                   # JDA_SCAN_PAD


def _layout_of(name):
    return SAMPLING[name.split("_")[2]]


def _kind_of(name):
    return name.split("_", 3)[3]


def hw_layout(hostsim, sampling, big):
    out = (C.c_uint32 * 4)()
    assert hostsim.hostsim_lds_layout(MODE[sampling], big, out) == 0
    return tuple(out)


def window_tiles(jpeg, flags=0):
    """(block index, scan_len, MCU columns, MCU rows) of the prepared image"""
    p = J.PreparedImage(jpeg, flags=flags)
    try:
        idx, nok = p.block_index()
        idx = np.asarray(idx, dtype=np.int64)
        scan_len = len(p.scan())
        mx, my = p.info.mcus_x, p.info.mcus_y
    finally:
        p.close()
    return idx, scan_len, mx, my


def tiles_from(idx, scan_len, mx, my, sampling):
    """every tile's MCUs, win_lo, hi before and after the clamp, win_need, spare and blocks, as jda_tile_setup_from and the host's
    routing count (jda_upload_batch) work them out"""
    mcus = lds_layout(sampling, 0)[0]
    nb = _NBLK[sampling]
    cap = (scan_len + SCAN_PAD) & ~15
    out = []
    for y in range(my):
        for x in range(0, mx, mcus):
            cnt = min(mcus, mx - x)
            b0 = (y * mx + x) * nb
            b1 = b0 + cnt * nb
            lo = (int(idx[b0]) >> 7) & ~15
            end = int(idx[b1]) >> 7
            hi_raw = (end + 8 + 12 + 15) & ~15
            hi = min(hi_raw, cap)
            out.append(dict(count=cnt, lo=lo, first=int(idx[b0]) >> 7, hi_raw=hi_raw, hi=hi, need=hi - lo, spare=hi - (end + 20),
                            b0=b0, b1=b1, clamped=hi_raw > cap))
    return out


def routing(tiles, scan_len, mx, my, sampling):
    """(host index: large layout?, device pre-scan's average rule: large layout?) -- jda_big_window"""
    mcus, _, ws, _ = lds_layout(sampling, 0)
    over = sum(t["hi_raw"] - t["lo"] > ws for t in tiles)
    avg = scan_len * mcus // (mx * my)
    return over * 100 > len(tiles), avg + avg // 2 + 48 > ws


def test_families_present():
    for lay in cj.LAYOUTS:
        s = cj.SHORT[lay]
        for kind in WINDOW_KINDS:
            assert "k_window_%s_%s" % (s, kind) in COEF_CASES
        for v in Q4REACH_VARIANTS:
            assert "k_q4reach_%s_%s" % (s, v) in COEF_CASES
    assert 40 <= len(WINDOW) + len(Q4REACH) <= 100


@pytest.mark.parametrize("sampling", cj.LAYOUTS)
def test_lds_layout_is_the_kernels(sampling, hostsim):
    """the corpus' restatement of jda_lds_layout is what the kernels' header compiles to (MCUS, WAVES, WIN_BYTES, WIN_OFF), and
    the two layouts' windows and workgroup sizes differ as the routing assertions need"""
    for big in (0, 1):
        assert lds_layout(sampling, big) == hw_layout(hostsim, sampling, big), (sampling, big)
    (m0, w0, ws, _), (m1, w1, wl, _) = (lds_layout(sampling, b) for b in (0, 1))
    assert m0 == m1 and w1 == w0 - 1 and wl > ws + 64


@pytest.mark.parametrize("name", WINDOW)
def test_window_corpus_is_what_it_claims(name):
    """from the product's block index: every intended edge tile is there with its win_lo phase, win_need and spare; the layout the
    host index and the average rule choose; the truncated reads where they were put.  The serial pre-scan's index is the reference
    reader's model of the written layout, entry for entry; the default (canonical entries) names the same bytes at every tile edge"""
    sampling, kind = _layout_of(name), _kind_of(name)
    jpeg = coef_jpeg_for(name)
    plan = _window_plan(sampling, kind)
    _, _, ws, _ = lds_layout(sampling, 0)
    _, _, wl, _ = lds_layout(sampling, 1)
    idx, scan_len, mx, my = window_tiles(jpeg, J.PREPARE_SERIAL_PRESCAN)
    _, layout = cj.write_jpeg(**coef_spec(name), return_layout=True)
    model, closing = cj.reader_entries(layout)
    assert [((int(v) >> 7), int(v) & 63, bool(int(v) & 64)) for v in idx[:-1]] == model
    assert ((int(idx[-1]) >> 7), int(idx[-1]) & 127) == closing
    tiles = tiles_from(idx, scan_len, mx, my, sampling)
    assert len(tiles) == plan["T"]
    canon, _, _, _ = window_tiles(jpeg)
    tiles_c = tiles_from(canon, scan_len, mx, my, sampling)
    for i, (t, tc) in enumerate(zip(tiles, tiles_c)):
        assert (t["lo"], t["hi"]) == (tc["lo"], tc["hi"]), (name, i)
    needs = set()
    for i, (need, fit, ph, opt) in plan["spec"].items():
        t = tiles[i]
        assert t["first"] % 16 == ph, (name, i)
        assert t["need"] == need, (name, i, t, need)
        if fit == "clamp":
            assert t["clamped"] and i == len(tiles) - 1 and scan_len % 16 == (14 if opt == "last14" else 15), (name, t, scan_len)
        else:
            assert t["spare"] == (0 if fit == "tight" else 15) and not t["clamped"], (name, i, t)
        if opt == "partial":
            assert t["count"] < plan["mcus"], (name, i)
        flagged = [b for b in range(t["b0"], t["b1"]) if int(idx[b]) & 64]
        assert flagged == ([t["b1"] - 1] if opt == "trunc" else []), (name, i, flagged)
        needs.add((need, fit))
    n_trunc = sum(1 for v in idx[:-1] if int(v) & 64)
    assert n_trunc == sum(1 for e in plan["spec"].values() if e[3] == "trunc")
    host_big, avg_big = routing(tiles, scan_len, mx, my, sampling)
    over_small = [i for i, t in enumerate(tiles) if t["hi_raw"] - t["lo"] > ws]
    if kind.startswith("small"):
        # one tile over the small window among >= 100: the host keeps the small layout (that tile reads HBM); the average rule
        # sends the same file to the large one
        assert len(over_small) == 1 and tiles[over_small[0]]["need"] == ws + 32 and len(tiles) >= 100
        assert (host_big, avg_big) == (False, True), name
        assert {(ws - 16, "tight"), (ws - 16, "loose"), (ws, "tight"), (ws, "loose")} <= needs
    elif kind == "large":
        assert (host_big, avg_big) == (True, True), name
        assert {(n, f) for n in (wl - 16, wl, wl + 16, wl + 32) for f in ("tight", "loose")} <= needs
        assert {(n, f) for n in (ws + 16, ws + 32) for f in ("tight", "loose")} <= needs
        assert max(t["need"] for t in tiles) >= 4096
    else:
        d = cj.decode_coefs(jpeg)
        assert d["restart_interval"] == plan["mcus"] and plan["spec"]
        restarts = set(layout["restarts"])
        for i in sorted(plan["spec"])[:-1]:
            # the tile behind the edge tile starts a restart interval (its first block's DC symbol at the interval's first bit)
            assert layout["blocks"][tiles[i]["b1"]][3][0] in restarts, (name, i)
    _, ws_waves, _, _ = lds_layout(sampling, 0)
    _, wl_waves, _, _ = lds_layout(sampling, 1)
    if kind != "dri":
        assert math.ceil(len(tiles) / ws_waves) != math.ceil(len(tiles) / wl_waves)


@pytest.mark.parametrize("name", Q4REACH)
def test_q4reach_corpus_is_what_it_claims(name):
    """every (0, 10) symbol has a 16-bit code: blocks of four take 104 bits; 'phase' puts their first AC bit at all 32 bits of a
    dword (from the product's index), and EOB-only blocks in front of such blocks; 'endK' ends the scan with one, scan_len = K mod 4"""
    jpeg = coef_jpeg_for(name)
    _, layout = cj.write_jpeg(**coef_spec(name), return_layout=True)
    p = J.PreparedImage(jpeg)
    try:
        idx, _ = p.block_index()
        scan_len = len(p.scan())
    finally:
        p.close()
    bits = [(int(v) >> 7) * 8 + (int(v) & 63) for v in idx[:-1]]
    full = []
    for i, (c, by, bx, dc, syms) in enumerate(layout["blocks"]):
        if len(syms) >= 4 and all(ln == 16 and s == 10 for _, ln, s in syms[:4]):
            assert syms[0][0] == bits[i] and syms[4][0] - syms[0][0] == 104
            full.append(i)
    assert full
    blocks = layout["blocks"]
    if name.endswith("_phase"):
        assert {(bits[i] - 1) & 31 for i in full} == set(range(32))
        assert sum(1 for i in full if i and len(blocks[i - 1][4]) == 1 and blocks[i - 1][4][0][2] == -1) >= 8
    else:
        k = int(name[-1])
        assert full[-1] == len(blocks) - 1 and scan_len % 4 == k and len(blocks[-2][4]) == 1
        assert (bits[-1] >> 3) + 20 > scan_len                   # (its bytes reach into the scan's last five dwords)


def _decode(hostsim, oracle, jpeg, pt, opt):
    rc, want, err = oracle.decode_canvas(jpeg, pt, opt)
    assert rc == 1, err
    got = np.full_like(want, 0x33)
    inf, cx, cy, mw, mh, bpp, sh = oracle.canvas_geometry(jpeg, pt, opt)
    hrc = hostsim.hostsim_decode(jpeg, len(jpeg), pt, opt, got.ctypes.data_as(C.c_void_p), got.shape[1], cx * mw, cy * mh)
    return hrc, got, want


@pytest.mark.parametrize("name", WINDOW + Q4REACH)
def test_emulator_at_the_real_windows(name, hostsim, oracle):
    """the wave emulator at each layout's own WIN_BYTES (hostsim_lds_layout), the wavefront's LDS poisoned with 0x00, 0xFF and 0xA5
    before every tile: full size, 1/2 and 1/4, a plain and a general pixel type, P1 whole and in chunks -- the oracle's pixels"""
    jpeg = coef_jpeg_for(name)
    sampling = _layout_of(name)
    plain = J.GRAY8 if sampling == "gray" else J.RGB8888
    try:
        for big in (0, 1):
            hostsim.hostsim_set_window(hw_layout(hostsim, sampling, big)[2])
            for poison in (0x00, 0xFF, 0xA5):
                hostsim.hostsim_set_poison(poison)
                for pt, opt in ((plain, 0), (J.RGB565_BE, J.SCALE_HALF), (J.RGB565_BE, 0)):
                    hrc, got, want = _decode(hostsim, oracle, jpeg, pt, opt)
                    assert hrc == 0 and np.array_equal(got, want), (name, big, poison, pt, opt, int(np.count_nonzero(got != want)))
            for pt, opt in ((plain, J.SCALE_QUARTER), (J.RGB565_LE, J.SCALE_QUARTER), (plain, J.SCALE_HALF | J.LUMA_ONLY)):
                hrc, got, want = _decode(hostsim, oracle, jpeg, pt, opt)
                assert hrc == 0 and np.array_equal(got, want), (name, big, pt, opt)
            hostsim.hostsim_set_chunked(1)
            try:
                for poison in (0x00, 0xFF):
                    hostsim.hostsim_set_poison(poison)
                    hrc, got, want = _decode(hostsim, oracle, jpeg, plain, 0)
                    assert hrc == 0 and np.array_equal(got, want), (name, big, "chunked", poison)
            finally:
                hostsim.hostsim_set_chunked(0)
    finally:
        hostsim.hostsim_set_poison(0xA5)
        hostsim.hostsim_set_window(1024)
