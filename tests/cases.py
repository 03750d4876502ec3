"""Shared test inputs: small deterministic synthetic JPEGs covering the shapes the path supports."""
import functools
import os

from jpegdec_amd.synth import synth_jpeg

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> kwargs for synth_jpeg
SYNTH_CASES = {
    "c420_333x217": dict(width=333, height=217, subsampling="4:2:0", seed=11),
    "c444_333x217": dict(width=333, height=217, subsampling="4:4:4", seed=12),
    "gray_333x217": dict(width=333, height=217, subsampling="gray", seed=13),
    "c420_640x368_rstrow": dict(width=640, height=368, subsampling="4:2:0", seed=14, restart_rows=1),
    "c420_256x256_q98": dict(width=256, height=256, subsampling="4:2:0", seed=15, quality=98),
    "c444_256x256_q100_opt": dict(width=256, height=256, subsampling="4:4:4", seed=16, quality=100, optimize=True),
    "gray_64x64_rst3": dict(width=64, height=64, subsampling="gray", seed=17, restart_blocks=3),
    "c420_1100x48": dict(width=1100, height=48, subsampling="4:2:0", seed=18),       # > 32 MCUs per row: 3 tiles
    "gray_1100x24": dict(width=1100, height=24, subsampling="gray", seed=19),        # 138 MCUs per row: one partial tile
    "gray_1600x16": dict(width=1600, height=16, subsampling="gray", seed=23),        # a full 192-MCU gray tile + remainder
    "c444_600x16": dict(width=600, height=16, subsampling="4:4:4", seed=24),         # a full 64-MCU 4:4:4 tile + remainder
    "c444_384x192_q100_rst7": dict(width=384, height=192, subsampling="4:4:4", seed=36, quality=100, restart_blocks=7),  # truncated reads + restarts
    "c420_512x256_q98_rstrow": dict(width=512, height=256, subsampling="4:2:0", seed=31, quality=98, restart_rows=1),
    "c420_16x16": dict(width=16, height=16, subsampling="4:2:0", seed=20),           # single MCU
    "c444_8x8_q30": dict(width=8, height=8, subsampling="4:4:4", seed=21, quality=30),
    "c420_1280x720": dict(width=1280, height=720, subsampling="4:2:0", seed=1234),   # BASELINE config 2 shape
    # 4:2:2 (h2v1, Pillow) and 4:4:0 (h1v2, our own encoder: Pillow cannot write it)
    "c422_333x217": dict(width=333, height=217, subsampling="4:2:2", seed=41),
    "c422_1100x24_rstrow": dict(width=1100, height=24, subsampling="4:2:2", seed=42, restart_rows=1),   # 69 MCUs per row: 5 tiles
    "c440_200x120": dict(width=200, height=120, subsampling="4:4:0", seed=43, quality=90),
    "c440_300x64_rst5": dict(width=300, height=64, subsampling="4:4:0", seed=44, restart_blocks=5),
    "c420_250x250_q10": dict(width=250, height=250, subsampling="4:2:0", seed=22, quality=10),  # many DC-only blocks
    # word-precision DQT (jpeg.inl:1742-1750): quantisers x 400 / x 3000 over uniform noise -> max |coef| x max |q'| >= 2^21, the
    # 32-bit-multiply kernels (jda_image_fast_mul == 0: asserted by tests/test_frontend.py::test_word_precision_dqt_cases)
    "w16_gray_200x120_x400": dict(width=200, height=120, subsampling="gray", seed=61, quality=90, noise=True, dqt16=400),
    "w16_c444_136x88_x3000": dict(width=136, height=88, subsampling="4:4:4", seed=62, quality=90, noise=True, dqt16=3000),
    "w16_c420_333x217_x400": dict(width=333, height=217, subsampling="4:2:0", seed=63, quality=90, noise=True, dqt16=400),
    "w16_c422_200x72_x3000": dict(width=200, height=72, subsampling="4:2:2", seed=64, quality=90, noise=True, dqt16=3000),
    "w16_c440_120x96_x400": dict(width=120, height=96, subsampling="4:4:0", seed=65, quality=90, noise=True, dqt16=400),
}
WORD_DQT_CASES = sorted(k for k in SYNTH_CASES if k.startswith("w16_"))

# progressive files (decoded from their first, DC-only scan as a 1/8 thumbnail, jpeg.inl:4964-4966)
PROGRESSIVE_CASES = {
    "p420_200x120": dict(width=200, height=120, subsampling="4:2:0", seed=51, progressive=True),
    "p444_333x217": dict(width=333, height=217, subsampling="4:4:4", seed=52, progressive=True),
    "p422_640x368": dict(width=640, height=368, subsampling="4:2:2", seed=53, progressive=True),
    "pgray_100x100": dict(width=100, height=100, subsampling="gray", seed=54, progressive=True),
    "p420_1280x720_q95": dict(width=1280, height=720, subsampling="4:2:0", seed=55, quality=95, progressive=True),
}
SYNTH_ALL = dict(SYNTH_CASES, **PROGRESSIVE_CASES)

PIXEL_TYPES = (0, 1, 2, 3)                 # RGB565_LE, RGB565_BE, RGB8888, GRAY8
OPTIONS = (0, 2, 4, 8, 64, 64 | 2)         # full, 1/2, 1/4, 1/8, luma-only, luma-only 1/2


@functools.lru_cache(maxsize=None)
def jpeg_for(name: str) -> bytes:
    path = os.path.join(GOLDEN_DIR, name + ".jpg")
    if os.path.exists(path):               # committed fixture wins (keeps tests independent of Pillow's version)
        return open(path, "rb").read()
    return synth_jpeg(**SYNTH_ALL[name])


def all_modes(name):
    for pt in PIXEL_TYPES:
        for opt in OPTIONS:
            if "c440" in name and pt == 2 and (opt & 4):
                continue       # JPEGPutMCU12, 1/4 scale, RGB8888 writes through the address of a local (jpeg.inl:4620): UB in the reference
            yield pt, opt


def progressive_modes(name):
    """pixel type x options a progressive file can be decoded with: everything except what the reference itself cannot do
    -- a colour file to 8-bit gray (it crashes: JPEGDecodeMCU_P(MCU_SKIP) stores far outside the object) and
    JPEG_SCALE_QUARTER (uninitialised sample bytes in its output); see DESIGN.md 3."""
    gray = name.startswith("pgray")
    for pt in PIXEL_TYPES:
        for opt in OPTIONS:
            if (opt & 4) and not (opt & 2):
                continue
            if not gray and (pt == 3 or (opt & 64)):
                continue
            if gray and pt == 2:
                continue       # gray JPEG + RGB8888: the reference emits 565 with iBpp = 32
            yield pt, opt


# ---- coefficient-level stress streams (tests/coef_jpeg.py): inputs chosen per quantised coefficient --------------------
# Each builder returns the write_jpeg keyword arguments; COEF_CASES maps a name to (builder, its arguments).  Families:
#   k_classes_*   the IDCT work lists (jda_p1_lists): per tile every (n1 & 7, n2 & 7) of the class-1 / class-2 counts, every
#                 column mask with rows 4-7 empty and not, tiles all DC-only / all class 0 / all class 2
#   k_single_*    one coefficient at each of the 64 positions, +-1 / +-511 / +-1023, flat 8-bit quantisers of 1 and 255: the
#                 24-bit-multiply kernels driven into the 10-bit wrap of the range limit
#   k_fastbound_* the two sides of the 24-bit multiply bound max|coef| x max|q'| < 2^21 (prescaled q')
#   k_huff_*      every AC symbol of both AC tables, Annex K and a custom table with codes of every length 1..16
#   k_dcdrift_*   DC predictors driven to 32767 / 32768 / -32768 / -32769, and swung past int16 over and
#                 over in streams long enough for the parallel host pre-scans (*_par*)
#   k_edge_*      extreme coefficients in the blocks the image does not cover, ragged sizes
import numpy as _np

from tests import coef_jpeg as _cj

_TILE_MCUS = {"gray": 64, "4:4:4": 20, "4:2:2": 16, "4:4:0": 16, "4:2:0": 10}    # jda_lds_layout<MODE>::MCUS
_MCU_PX = {"gray": (8, 8), "4:4:4": (8, 8), "4:2:2": (16, 8), "4:4:0": (8, 16), "4:2:0": (16, 16)}


def _blocks_in_mcu_order(coefs, sampling, cx, cy):
    """[(component, block row, block column)] in stream order"""
    hs, vs = _cj.LUMA_HV[sampling]
    out = []
    for m in range(cx * cy):
        my, mx = divmod(m, cx)
        out += [(0, my * vs + v, mx * hs + h) for v in range(vs) for h in range(hs)]
        out += [(c, my, mx) for c in range(1, len(coefs))]
    return out


def _mask_block(rng, mask, rows47, variant):
    """zig-zag block whose AC coefficients sit in exactly the columns of `mask`, rows 4-7 used or not"""
    nat = _np.zeros(64, dtype=_np.int64)
    cols = [c for c in range(8) if mask >> c & 1]
    for i, c in enumerate(cols):
        if rows47 and i == 0:
            r = 4 + variant % 4                                      # (a quarter of them: the only coefficient of its column in row 4)
        else:
            r = (1 + (variant + i) % 3) if c == 0 else (variant + i) % 4
        v = int(rng.integers(1, 16))
        nat[r * 8 + c] = v if rng.integers(0, 2) else -v
    zz = nat[_cj._ZIGZAG]
    zz[0] = 0 if (rows47 and len(cols) == 1) else int(rng.integers(-20, 21))
    return zz


def _k_classes(sampling):
    rng = _np.random.default_rng(101)
    per = _TILE_MCUS[sampling]
    mw, mh = _MCU_PX[sampling]
    nb = per * {"gray": 1, "4:4:4": 3, "4:2:2": 4, "4:4:0": 4, "4:2:0": 6}[sampling]
    queues = {0: [(m, r) for m in (1, 2, 3) for r in (0, 1)],
              1: [(m, r) for m in range(4, 16) for r in (0, 1)],
              2: [(m, r) for m in range(16, 256) for r in (0, 1)]}
    pos = {0: 0, 1: 0, 2: 0}
    plans = []
    for t in range(64):
        a, b = t & 7, t >> 3
        n1, n2 = a + 8 * ((t >> 2) & 1), b + 8 * (t & 3)
        rest = nb - n1 - n2
        plans.append([0] * (rest // 2) + [1] * n1 + [2] * n2 + [3] * (rest - rest // 2))
    plans += [[3] * nb, [0] * nb, [2] * nb]
    width, height = per * mw, len(plans) * mh
    coefs = _cj.zero_coefs(width, height, sampling)
    cx, cy = per, len(plans)
    order = _blocks_in_mcu_order(coefs, sampling, cx, cy)
    for t, plan in enumerate(plans):
        plan = list(plan)
        rng.shuffle(plan)
        for k, cls in enumerate(plan):
            c, by, bx = order[t * nb + k]
            if cls == 3:
                coefs[c][by, bx, 0] = int(rng.integers(-20, 21))
                continue
            q = queues[cls]
            mask, rows47 = q[pos[cls] % len(q)]
            coefs[c][by, bx] = _mask_block(rng, mask, rows47, pos[cls] // len(q))
            pos[cls] += 1
    return dict(width=width, height=height, sampling=sampling, coefs=coefs,
                quant={0: [4] * 64, 1: [6] * 64})


_SINGLE_VALUES = (1, -1, 511, -511, 1023, -1023)


def _k_single(sampling, q):
    width = height = 160
    coefs = _cj.zero_coefs(width, height, sampling)
    seq = [(p, v) for p in range(64) for v in _SINGLE_VALUES]
    for c, arr in enumerate(coefs):
        flat = arr.reshape(-1, 64)
        for i in range(flat.shape[0]):
            p, v = seq[(i + 128 * c) % len(seq)]
            flat[i, p] = v
    return dict(width=width, height=height, sampling=sampling, coefs=coefs, quant={0: [q] * 64, 1: [q] * 64})


# the prescaled quantiser q'[n] = (q[n] * aan[n]) >> 12 (jpeg.inl:1789-1811); these q give q' = 16513 / 16514 at rows 1, 3, 5, 7 of
# column 7 (checked against the front end's tables by tests/test_coef_streams_cpu.py)
FASTBOUND_Q = {"lo": (10788, 12726, 19043, 54240), "hi": (10788, 12727, 19044, 54244)}


def _k_fastbound(sampling, side, term):
    """term 'ac': category-7 coefficients (+-127) against q' = 16513 (worst = 127 x 16513 = 2^21 - 1) or, on the 'hi' side, q' = 16514;
    four of them in one column, signed so that the odd part's z10 + z12 = (c5 - c3) + (c1 - c7) is the largest operand it can be.
    term 'dc': |DC| x q0' with q0' = 4 x q0: 3942 x 4 x 133 = 2^21 - 8 (an odd worst is out of the DC term's reach), or
    16384 x 4 x 32 = 2^21 exactly (out of the AC term's reach)."""
    width, height = 48, 32
    coefs = _cj.zero_coefs(width, height, sampling)
    zz = {n: i for i, n in enumerate(_cj._ZIGZAG)}
    if term == "ac":
        qz = [1] * 64
        for r, q in zip((1, 3, 5, 7), FASTBOUND_Q[side]):
            qz[zz[r * 8 + 7]] = q
        for arr in coefs:
            flat = arr.reshape(-1, 64)
            for i in range(flat.shape[0]):
                sg = 1 if i % 2 == 0 else -1
                for r, s in zip((1, 3, 5, 7), (1, -1, 1, -1)):
                    flat[i, zz[r * 8 + 7]] = sg * s * 127
                flat[i, zz[7]] = 3                                    # (and something in the rows' direction too)
        quant = {0: qz, 1: qz}
    else:
        q0, dc = (133, 3942) if side == "lo" else (32, 16384)
        qz = [q0] + [2] * 63
        order = _blocks_in_mcu_order(coefs, sampling, *_cj.geometry(width, height, sampling)[:2])
        for comp in range(len(coefs)):
            # in stream order: ramp in steps the DC category allows, hold +-dc, turn: the peak in several blocks of every component
            v, i = 0, 0
            for c, by, bx in order:
                if c != comp:
                    continue
                tgt = dc if (i // 24) % 2 == 0 else -dc
                v = v + max(-2047, min(2047, tgt - v))
                coefs[c][by, bx, 0] = v
                if i % 5 == 1:
                    coefs[c][by, bx, 1] = 7
                i += 1
        quant = {0: qz, 1: qz}
    return dict(width=width, height=height, sampling=sampling, coefs=coefs, quant=quant)


def _huff_blocks(first_dc=0):
    """zig-zag blocks that use every AC symbol once at least, and the corner cases of the AC syntax"""
    blocks = []
    for r in range(16):
        for s in range(1, 11):
            zz = _np.zeros(64, dtype=_np.int64)
            zz[1 + r] = (1 << (s - 1)) + ((r * 7) % (1 << (s - 1)) if s > 1 else 0)
            if (r + s) & 1:
                zz[1 + r] = -zz[1 + r]
            zz[1 + r + 1 + (s % 3)] = 1                               # (a second symbol behind it)
            blocks.append(zz)
    zz = _np.zeros(64, dtype=_np.int64); zz[17] = 2; blocks.append(zz)                  # ZRL, then run 0
    zz = _np.zeros(64, dtype=_np.int64); zz[63] = 5; blocks.append(zz)                  # ZRL x 3, run 14, coefficient 63, no EOB
    zz = _np.zeros(64, dtype=_np.int64); zz[1] = 1; zz[63] = -300; blocks.append(zz)    # ZRL x 3 in the middle of a block, then 63
    zz = _np.zeros(64, dtype=_np.int64); zz[0] = 1500; blocks.append(zz)                # DC category 11, EOB right after DC
    zz = _np.zeros(64, dtype=_np.int64); zz[0] = -300; blocks.append(zz)                # DC category 11 down
    zz = _np.zeros(64, dtype=_np.int64); zz[0] = 1700; zz[63] = 1; blocks.append(zz)
    zz = _np.zeros(64, dtype=_np.int64); blocks.append(zz)
    return blocks


# Two AC tables whose code lengths together are every length 1..16, most codes 16 bits long.  (One table of 162 codes cannot
# have every length: lengths 1..15 once each leave room for one 16-bit code.)  A code longer than 10 bits must start 111111 --
# the long half of the LUT, jpeg.inl:2232-2233 -- so the short codes fill 63/64 of the code space first.
CUSTOM_AC_BITS = ([1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, 0, 0, 152],
                  [0, 3, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, 1, 149])


def custom_ac_table(which):
    order = list(_cj.AC_SYMBOLS)
    _np.random.default_rng(7 + which).shuffle(order)
    return list(CUSTOM_AC_BITS[which]), order


def _k_huff(sampling, custom):
    blocks = _huff_blocks()
    nc = 1 if sampling == "gray" else 3
    hs, vs = _cj.LUMA_HV[sampling]
    mcus = len(blocks) + 2
    cx = 12
    cy = (mcus + cx - 1) // cx
    width, height = cx * 8 * hs, cy * 8 * vs
    coefs = _cj.zero_coefs(width, height, sampling)
    for c, arr in enumerate(coefs):
        flat = arr.reshape(-1, 64)
        for i in range(flat.shape[0]):
            flat[i] = blocks[(i + 17 * c) % len(blocks)]
    huff = dict(_cj.annex_k()[2])
    if custom:
        huff[(1, 0)] = custom_ac_table(0)
        huff[(1, 1)] = custom_ac_table(1)
    return dict(width=width, height=height, sampling=sampling, coefs=coefs, quant={0: [1] * 64, 1: [2] * 64}, huff=huff)


def _k_huff_cross(sampling):
    """a run that crosses position 63 (legal syntax, a corrupt block): ZRL x 3, run 11 to coefficient 60, then run 15 (to 76)"""
    d = _k_huff(sampling, False)
    d["ac_pairs"] = {(0, 0, 3): [(15, 0), (15, 0), (15, 0), (11, 3), (15, 1)]}
    return d


def _k_dcdrift(sampling, target, comp, q0, dri):
    """the DC value of component `comp` ramps (+-2047 a block) to `target` in the LAST block of that component in MCU k - 1, then
    back; dri: a restart interval of k MCUs resets the predictor before the component's next block"""
    hs, vs = _cj.LUMA_HV[sampling]
    per_mcu = hs * vs if comp == 0 else 1
    steps = (abs(target) + 2046) // 2047
    k = (steps + per_mcu - 1) // per_mcu + 1
    cx = 2 * k + 2
    width, height = cx * 8 * hs, 8 * vs
    coefs = _cj.zero_coefs(width, height, sampling)
    order = [b for b in _blocks_in_mcu_order(coefs, sampling, cx, 1) if b[0] == comp]
    peak = k * per_mcu - 1
    vals = [0] * len(order)
    sg = 1 if target > 0 else -1
    for i in range(peak + 1):
        vals[peak - i] = target - sg * 2047 * i if abs(target) > 2047 * i else 0
    for i in range(peak + 1, len(order)):
        vals[i] = 0 if dri else (target - sg * 2047 * (i - peak) if abs(target) > 2047 * (i - peak) else 0)
    for (c, by, bx), v in zip(order, vals):
        coefs[c][by, bx, 0] = v
    if q0 == 1:
        c, by, bx = order[peak]
        coefs[c][by, bx, 2] = 3                                       # (the peak block not DC-only)
    qs = {0: [q0 if comp == 0 else 3] + [3] * 63, 1: [q0 if comp != 0 else 5] + [5] * 63}
    return dict(width=width, height=height, sampling=sampling, coefs=coefs, quant=qs if sampling != "gray" else {0: qs[0]},
                restart_interval=k if dri else 0)


def _k_dcdrift_par(dri):
    """a 1024x256 4:2:0 stream long enough for the parallel host pre-scans (interval workers with a DRI, scan chunks without):
    luma and Cb predictors swing between +-40000 (+-2047 a block), past int16 again and again; with dri, one MCU row an
    interval and the swing restarts from 0 in each"""
    rng = _np.random.default_rng(211)
    width, height = 1024, 256
    coefs = _cj.zero_coefs(width, height, "4:2:0")
    cx, cy = _cj.geometry(width, height, "4:2:0")[:2]
    order = _blocks_in_mcu_order(coefs, "4:2:0", cx, cy)
    per_mcu = 6
    amp = {0: 40000, 1: 35000}
    v, step = [0, 0, 0], [2047, 2047, 0]
    for i, (c, by, bx) in enumerate(order):
        if dri and i % (dri * per_mcu) == 0:
            v, step = [0, 0, 0], [2047, 2047, 0]
        if c in amp:
            if abs(v[c] + step[c]) > amp[c]:
                step[c] = -step[c]
            v[c] += step[c]
        coefs[c][by, bx, 0] = v[c]
        coefs[c][by, bx, 1:9] = rng.integers(-3, 4, size=8)
    return dict(width=width, height=height, sampling="4:2:0", coefs=coefs, quant={0: [2] * 64, 1: [3] * 64},
                restart_interval=dri)


def _k_edge(sampling, w, h):
    rng = _np.random.default_rng(w * 1000 + h)
    coefs = _cj.zero_coefs(w, h, sampling)
    hs, vs = _cj.LUMA_HV[sampling]
    for c, arr in enumerate(coefs):
        cw, ch = (w, h) if c == 0 else ((w + hs - 1) // hs, (h + vs - 1) // vs)
        for by in range(arr.shape[0]):
            for bx in range(arr.shape[1]):
                inside = (bx + 1) * 8 <= cw and (by + 1) * 8 <= ch
                if inside:
                    arr[by, bx, :6] = rng.integers(-12, 13, size=6)
                else:                                                # a block the image does not (wholly) cover: extremes
                    arr[by, bx, 0] = 2000 if (bx + by) & 1 else -2000
                    arr[by, bx, [1, 2, 9, 20, 35, 63]] = _np.where(rng.integers(0, 2, size=6) == 1, 1023, -1023)
    # DC differences stay inside category 11: walk the DC values in stream order and clamp the steps
    order = _blocks_in_mcu_order(coefs, sampling, *_cj.geometry(w, h, sampling)[:2])
    pred = [0] * len(coefs)
    for c, by, bx in order:
        v = int(coefs[c][by, bx, 0])
        v = max(pred[c] - 2047, min(pred[c] + 2047, v))
        coefs[c][by, bx, 0] = v
        pred[c] = v
    return dict(width=w, height=h, sampling=sampling, coefs=coefs, quant={0: [16] * 64, 1: [16] * 64})


# ---- scan-window edges (k_window_*) and the 1/4 kernel's five-dword reach (k_q4reach_*) --------------------------------------------
# A tile stages bytes [win_lo, hi) of the filtered scan in its wavefront's LDS window (jda_tile_setup_from): win_lo = byte(entry of its
# first block) & ~15, hi = (byte(entry of the first block behind it) + 8 + 12 + 15) & ~15, clamped to (scan_len + 32) & ~15;
# win_need = hi - win_lo against the layout's WIN_BYTES.  The builders below write tiles whose win_need is chosen to the byte: every
# DC difference is 0 (a 2-bit code), a block's AC bits are a sum of Annex K symbol lengths, and the last block of each tile is searched
# for with the reference reader's model (tests/coef_jpeg.py reader_entries) until the next tile's first entry lands where it should --
# with a bit offset below 8, so that the serial pre-scan's entry and the canonical (bit >> 3, bit & 7) of the parallel and the device
# pre-scans name the same byte.
_LT_BYTES, _COEF_STRIDE, _LDS_BYTES = 10528, 136, 160 * 1024          # JDA_LT_BYTES, JDA_COEF_STRIDE, the LDS of a CU
_NBLK = {"gray": 1, "4:4:4": 3, "4:2:2": 4, "4:4:0": 4, "4:2:0": 6}


def lds_layout(sampling, big):
    """jda_lds_layout<MODE, BIG> restated: (MCUS, WAVES, WIN_BYTES, WIN_OFF) -- tests pin it to the compiled header"""
    nblk = _NBLK[sampling]
    mcus = 20 if sampling == "4:4:4" else 64 // nblk
    blocks = mcus * nblk
    win_off = (blocks * _COEF_STRIDE + 64 + 32 + 15) // 16 * 16
    free = _LDS_BYTES - _LT_BYTES - 16
    waves = min(16, free // (win_off + blocks * 16 + 16)) - big
    return mcus, waves, min(2048, free // waves // 16 * 16 - win_off), win_off


def _sym_costs(huff_t):
    """{(run, size): bits} of an AC table's symbols (code + magnitude), EOB as (0, 0)"""
    from jpegdec_amd.synth import _codes
    return {(rs >> 4, rs & 15): ln + (rs & 15) for rs, (code, ln) in _codes(*huff_t).items()}


@functools.lru_cache(maxsize=None)
def _fill_table(table_key):
    """fewest run-0 symbols whose bits sum to b, for every b up to 1700: dp[b] = (count, size of one of them).  Only symbols of 17 bits
    at most (code + magnitude): the reference's 64-bit reader cannot truncate their magnitude reads (it holds 17 bits more than 47)"""
    costs = _sym_costs(_cj.annex_k()[2][(1, table_key)])
    sizes = [(costs[(0, sz)], sz) for sz in range(1, 11) if costs[(0, sz)] <= 17]
    dp = [(0, 0)] + [(10 ** 9, 0)] * 1700
    for b in range(1, 1701):
        for c, sz in sizes:
            if c <= b and dp[b - c][0] + 1 < dp[b][0]:
                dp[b] = (dp[b - c][0] + 1, sz)
    return dp, costs[(0, 0)], costs


@functools.lru_cache(maxsize=None)
def _block_sizes(table_key, bits, tail=()):
    """magnitude sizes of run-0 symbols that, with the symbols of `tail` ((run, size) pairs) and EOB, take exactly `bits` AC bits;
    None if no such block (at most 62 coefficients before EOB)"""
    dp, eob, costs = _fill_table(table_key)
    b = bits - eob - sum(costs[t] for t in tail)
    if b < 0 or b > 1700 or dp[b][0] + sum(1 + r for r, _ in tail) > 62:
        return None
    out = []
    while b:
        out.append(dp[b][1])
        b -= costs[(0, dp[b][1])]
    return tuple(out)


def _reader_step(pos, off, syms, restart=False):
    """the reference reader over one block whose DC difference is 0 (reader_entries, in (byte, offset) form): syms = [(bits of the
    code, magnitude size or -1 for EOB)] -> (pos, off behind it, its entry, a truncated read)"""
    if restart:
        off = (off + 7) & ~7
    if off > 47:
        pos, off = pos + (off >> 3), off & 7
    off += 2
    if off > 47:
        pos, off = pos + (off >> 3), off & 7
    entry, trunc = (pos, off), False
    for ln, sz in syms:
        off += ln
        if sz < 0:
            break
        if sz and off + sz > 64:
            trunc = True
        off += sz
        if off > 47:
            pos, off = pos + (off >> 3), off & 7
    return pos, off, entry, trunc


@functools.lru_cache(maxsize=None)
def _symbols(sampling, t, sizes, tail):
    """(pairs, [(code bits, magnitude size)] + EOB) of a block of run-0 symbols of these sizes, then `tail`"""
    from jpegdec_amd.synth import _codes
    lens = {(rs >> 4, rs & 15): ln for rs, (code, ln) in _codes(*_cj.annex_k()[2][(1, t)]).items()}
    pairs = tuple((0, sz) for sz in sizes) + tuple(tail)
    return pairs, tuple((lens[p], p[1]) for p in pairs) + ((lens[(0, 0)], -1),)


class _WindowStream:
    """blocks in stream order, planned with the reader model; tiles are added one after the other"""

    def __init__(self, sampling, rng):
        self.sampling, self.rng = sampling, rng
        self.pos = self.off = 0
        self.restart = False                   # the next block starts a restart interval
        self.blocks = []                       # per block: [(run, value)] of its AC symbols (EOB implied)
        self.entries = []                      # the model's entry of every block (byte, offset, truncated)

    def table(self, i):
        nb, nl = _NBLK[self.sampling], _NBLK[self.sampling] - (2 if self.sampling != "gray" else 0)
        return 0 if i % nb < nl else 1

    def symbols(self, t, sizes, tail):
        return _symbols(self.sampling, t, sizes, tail)

    def value(self, sz):
        v = int(self.rng.integers(1 << (sz - 1), 1 << sz))
        return v if self.rng.integers(0, 2) else -v

    def add(self, pairs):
        t = self.table(len(self.blocks))
        _, syms = self.symbols(t, tuple(p[1] for p in pairs if p[0] == 0), tuple(p for p in pairs if p[0] != 0))
        self.pos, self.off, entry, trunc = _reader_step(self.pos, self.off, syms, self.restart)
        self.restart = False
        self.entries.append((entry[0], entry[1], trunc))
        self.blocks.append([(r, self.value(sz)) for r, sz in pairs])

    def next_entry(self, restart=False):
        """the entry a block behind the last one would get (its DC difference 0)"""
        return _reader_step(self.pos, self.off, [], restart)[2]

    def tile(self, nb, target, restart_next=False, trunc_last=False, last=False):
        """nb blocks; target(pos, off) of the next tile's first entry (or, last=True, of the closing entry) -> bool.  The blocks share
        the bits in front of the last one; the last one is searched for"""
        saved = (self.pos, self.off, len(self.blocks), self.restart)
        for attempt in range(64):
            if self._tile(nb, target, restart_next, trunc_last, last, 64 + 8 * attempt):
                self.restart = restart_next
                return
            self.pos, self.off, _, self.restart = saved    # (the byte the reader can reach next depends on where it last moved: again,
            del self.blocks[saved[2]:]                     # with the blocks in front of the last two a little shorter)
            del self.entries[saved[2]:]
        raise AssertionError("no block reaches the tile's target")

    def _tile(self, nb, target, restart_next, trunc_last, last, slack):
        want = target.bits
        start = 8 * self.pos + self.off
        per = max(4, (want - start - 2 * nb - slack) // nb)
        for i in range(nb - 2):
            t = self.table(len(self.blocks))
            b = per + int(self.rng.integers(-per // 8, per // 8 + 1))
            sizes = None
            while sizes is None:
                sizes = _block_sizes(t, b)
                b += 1
            self.add([(0, sz) for sz in sizes])
        # the last two blocks: the reader's refills follow the symbols, not only their bits -- the one in front of the last is
        # varied as well
        t2, t = self.table(len(self.blocks)), self.table(len(self.blocks) + 1)
        tail = ((1, 10),) if trunc_last else ()
        mid = max(8, (want - (8 * self.pos + self.off) - 8 - (26 if trunc_last else 0)) // 2)
        for d2 in range(0, 48):
            b2 = mid + (d2 // 2 if d2 % 2 == 0 else -(d2 // 2) - 1)
            sizes2 = _block_sizes(t2, b2)
            if sizes2 is None:
                continue
            pairs2, syms2 = self.symbols(t2, sizes2, ())
            pos2, off2, _, _ = _reader_step(self.pos, self.off, syms2)
            base = want - (8 * pos2 + off2) - 4
            for d in range(0, 160):
                b = base + (d // 2 if d % 2 == 0 else -(d // 2) - 1)
                sizes = _block_sizes(t, b, tail)
                if sizes is None:
                    continue
                pairs, syms = self.symbols(t, sizes, tail)
                pos, off, entry, trunc = _reader_step(pos2, off2, syms)
                if trunc_last and not trunc:
                    continue
                if last:
                    ok = target(pos, off)
                else:
                    ok = target(*_reader_step(pos, off, [], restart_next)[2])
                if ok:
                    self.add(pairs2)
                    self.add(pairs)
                    return True
        return False


def _at(x, phase_only=False):
    """target: the next entry at byte x -- or, phase_only, at a byte of x's phase mod 16 within 64 bytes of x --, offset < 8 (the
    serial and the canonical entry agree)"""
    if phase_only:
        f = lambda pos, off: pos % 16 == x % 16 and abs(pos - x) <= 64 and off < 8
    else:
        f = lambda pos, off: pos == x and off < 8
    f.bits = 8 * x + 3
    return f


def _window_plan(sampling, kind):
    """(tiles per row, rows, partial MCUs of a row's last tile, restart interval) and the tile specs:
    {slot: (win_need, 'tight' | 'loose', start phase, options)}, the fillers' byte range"""
    mcus, ws_waves, ws, _ = lds_layout(sampling, 0)
    _, wl_waves, wl, _ = lds_layout(sampling, 1)
    if kind == "dri":
        full, rows, part, dri = 4, 3, 0, mcus
    else:
        # T tiles: ceil(T / waves) differs between the two layouts (112 for 16 / 15 wavefronts, 105 for 15 / 14)
        full, rows = (7, 14) if ws_waves == 16 else (6, 15)
        part, dri = mcus // 2, 0
    per_row = full + (1 if part else 0)
    T = per_row * rows
    partial = [r * per_row + full for r in range(rows)] if part else []
    edges = []
    if kind in ("small_tight", "small_loose"):
        edges.append((ws + 32, kind[6:], 0, ""))                                  # the one tile over the small window
        edges += [(n, f, ph, "") for n in (ws - 16, ws) for f in ("tight", "loose") for ph in (0, 15)]
        edges += [(ws, "tight", 15, "trunc")]
        fill, W = (ws * 3 // 4, ws - 48), ws
    elif kind == "large":
        edges += [(n, f, ph, "") for n in (wl - 16, wl, wl + 16, wl + 32) for f in ("tight", "loose") for ph in (0, 15)]
        edges += [(n, f, ph, "") for n in (ws + 16, ws + 32) for f in ("tight", "loose") for ph in (0, 15)]
        edges += [(wl, "tight", 0, "trunc")]
        fill, W = (ws + 64, wl - 64), wl
    else:
        edges += [(n, "tight", 0, "") for n in (wl + 32, wl + 16, ws + 32, ws + 16)]
        fill, W = (ws // 2, ws - 64), wl
    spec = {}
    # a partial tile at W (a row's last tile, count < MCUS) and the last tile, clamped at the end of the scan
    odd_partial = [i for i in partial if i % 2 == 1 and i < T - 2]
    if odd_partial:
        spec[odd_partial[0]] = (W, "tight", 0, "partial")
    # (the host's routing count takes hi before the clamp: a last tile clamped to W is over W -- in a "small" image it is clamped to W - 16)
    spec[T - 1] = (W - 16 if kind.startswith("small") else W, "clamp", 0, "last15" if kind in ("small_loose", "dri") else "last14")
    slot = 1
    for e in edges:
        while slot in spec or slot >= T - 2:
            slot += 2
            assert slot < T, (sampling, kind)
        spec[slot] = e
        slot += 2
    return dict(full=full, rows=rows, part=part, dri=dri, T=T, spec=spec, fill=fill, mcus=mcus, big4k=kind == "large")


def _k_window(sampling, kind):
    rng = _np.random.default_rng(sum(map(ord, sampling + kind)))
    P = _window_plan(sampling, kind)
    nblk = _NBLK[sampling]
    mw, mh = _MCU_PX[sampling]
    mcus_x = P["full"] * P["mcus"] + P["part"]
    width, height = mcus_x * mw - 3, P["rows"] * mh - 5                        # (ragged: the last MCU column and row are cut)
    st = _WindowStream(sampling, rng)
    per_row = P["full"] + (1 if P["part"] else 0)
    spec = P["spec"]
    win_lo = 0
    for i in range(P["T"]):
        count = P["part"] if P["part"] and i % per_row == P["full"] else P["mcus"]
        nb = count * nblk
        if i == P["T"] - 1:
            # the last tile: hi clamped at (scan_len + 32) & ~15 = win_lo + W -- scan_len = 14 or 15 mod 16, the closing entry's byte
            # close enough to the end that the +8+12 reach passes the clamp
            need, _, _, opt = spec[i]
            cls = 14 if opt == "last14" else 15
            scan_len = win_lo + need - 32 + cls

            def target(pos, off, scan_len=scan_len, cls=cls):
                return (8 * pos + off + 7) // 8 == scan_len and pos >= scan_len - (1 if cls == 14 else 2)
            target.bits = 8 * scan_len - 4
            st.tile(nb, target, last=True)
            continue
        if i in spec:
            need, fit, _, opt = spec[i]
            assert i + 1 not in spec
            x = win_lo + need - (20 if fit == "tight" else 35)            # tight: hi = byte + 20, no spare byte; loose: 15 spare
        else:
            a, b = P["fill"]
            size = 4200 if (P["big4k"] and i == 2) else int(rng.integers(a, b))
            nxt = spec.get(i + 1)
            ph = nxt[2] if nxt is not None else int(rng.integers(0, 16))
            x = st.pos + size
            x += (ph - x) % 16
        tgt = _at(x, phase_only=i not in spec)
        st.tile(nb, tgt, restart_next=bool(P["dri"]), trunc_last=i in spec and spec[i][3] == "trunc")
        win_lo = st.next_entry(bool(P["dri"]))[0] & ~15
    coefs = _cj.zero_coefs(width, height, sampling)
    cx, cy = _cj.geometry(width, height, sampling)[:2]
    order = _blocks_in_mcu_order(coefs, sampling, cx, cy)
    assert len(order) == len(st.blocks)
    for (c, by, bx), pairs in zip(order, st.blocks):
        k = 1
        for r, v in pairs:
            k += r
            coefs[c][by, bx, k] = v
            k += 1
    return dict(width=width, height=height, sampling=sampling, coefs=coefs, quant={0: [2] * 64, 1: [2] * 64},
                restart_interval=P["dri"])


def _k_q4reach(sampling, variant):
    """the 1/4 kernel's five dwords (jda_q4_load): one AC table (Annex K's luma table for both: every S = 10 symbol has a 16-bit
    code).  'phase': blocks whose first four AC symbols are (0, 10) -- 4 x 26 = 104 bits, the most four symbols take -- with the first
    AC bit at every bit of its dword; blocks that end with EOB on the first trip in front of such blocks.  'endK': such a block, behind
    an EOB-only block, is the scan's last, its first AC bit late in its dword, scan_len = K mod 4."""
    rng = _np.random.default_rng(sum(map(ord, sampling + variant)))
    nblk = _NBLK[sampling]
    M, E = ((0, 10),) * 4, ()
    lens = _symbols(sampling, 0, (), ())[1][-1][0]               # (EOB's code length)
    seq, cur = [], 0                                             # blocks' AC pairs; bit position of the next block's start

    def add(pairs):
        nonlocal cur
        seq.append(pairs)
        _, syms = _symbols(sampling, 0, tuple(p[1] for p in pairs), ())
        cur += 2 + sum(ln + max(sz, 0) for ln, sz in syms)

    def filler_to(phase, extra=0):                               # a filler block: the block behind `extra` bits of others starts its AC at `phase`
        b = 10 + ((phase - cur - 2 - extra - 2 - 10) % 32)
        add(tuple((0, sz) for sz in _block_sizes(0, b)))
    if variant == "phase":
        n = {1: 88, 3: 90, 4: 96, 6: 90}[nblk]
        for ph in range(32):
            filler_to(ph)
            add(M)
        for ph in range(24, 32):
            filler_to(ph, extra=2 + lens)
            add(E)
            add(M)
        while len(seq) < n:
            add(tuple((0, sz) for sz in _block_sizes(0, int(rng.integers(10, 60)))))
    else:
        k = int(variant[3:])
        n = {1: 16, 3: 18, 4: 16, 6: 18}[nblk]
        while len(seq) < n - 3:
            add(tuple((0, sz) for sz in _block_sizes(0, int(rng.integers(10, 60)))))
        best = None
        for b in range(10, 42):                                  # (of the bit phases with scan_len = K mod 4, the latest)
            p_m = cur + 2 + b + 2 + lens + 2                         # the last block's first AC bit
            if ((p_m + 104 + lens + 7) // 8) % 4 == k and (best is None or ((p_m - 1) & 31) > best[0]):
                best = ((p_m - 1) & 31, b)
        add(tuple((0, sz) for sz in _block_sizes(0, best[1])))
        add(E)
        add(M)
    cx = {1: 8, 3: 6, 4: 4, 6: 3}[nblk]
    mcus = len(seq) // nblk
    assert mcus * nblk == len(seq) and mcus % cx == 0, (sampling, variant, len(seq))
    mw, mh = _MCU_PX[sampling]
    width, height = cx * mw, mcus // cx * mh
    coefs = _cj.zero_coefs(width, height, sampling)
    order = _blocks_in_mcu_order(coefs, sampling, cx, mcus // cx)
    for (c, by, bx), pairs in zip(order, seq):
        for i, (r, sz) in enumerate(pairs):
            v = int(rng.integers(1 << (sz - 1), 1 << sz))
            coefs[c][by, bx, 1 + i] = v if rng.integers(0, 2) else -v
    huff = dict(_cj.annex_k()[2])
    huff[(1, 1)] = huff[(1, 0)]
    return dict(width=width, height=height, sampling=sampling, coefs=coefs, quant={0: [1] * 64, 1: [1] * 64}, huff=huff)


WINDOW_KINDS = ("small_tight", "small_loose", "large", "dri")
Q4REACH_VARIANTS = ("phase", "end0", "end1", "end2", "end3")


def _coef_cases():
    cases = {}
    for lay in _cj.LAYOUTS:
        s = _cj.SHORT[lay]
        cases["k_classes_" + s] = (_k_classes, (lay,))
        for q in (1, 255):
            cases["k_single_q%d_%s" % (q, s)] = (_k_single, (lay, q))
        for term in ("ac", "dc"):
            for side in ("lo", "hi"):
                cases["k_fastbound_%s_%s_%s" % (term, side, s)] = (_k_fastbound, (lay, side, term))
        cases["k_huff_annexk_" + s] = (_k_huff, (lay, False))
        cases["k_huff_custom_" + s] = (_k_huff, (lay, True))
        for target in (32767, 32768, -32768, -32769):
            for comp in ((0,) if lay == "gray" else (0, 1)):
                for q0 in ((1, 200) if lay in ("gray", "4:2:0") else (200,)):
                    for dri in (0, 1):
                        cases["k_dcdrift_%s_%d_%s_q%d%s" % (s, target, "y" if comp == 0 else "cb", q0, "_dri" if dri else "")] = (
                            _k_dcdrift, (lay, target, comp, q0, dri))
        mw, mh = _MCU_PX[lay]
        per = _TILE_MCUS[lay]
        for w, h in ((1, 1), (7, 9), (17, 15), ((per - 1) * mw - 3, mh + 5), ((per + 1) * mw - 5, 2 * mh - 1)):
            cases["k_edge_%s_%dx%d" % (s, w, h)] = (_k_edge, (lay, w, h))
    for lay in _cj.LAYOUTS:
        for kind in WINDOW_KINDS:
            cases["k_window_%s_%s" % (_cj.SHORT[lay], kind)] = (_k_window, (lay, kind))
        for v in Q4REACH_VARIANTS:
            cases["k_q4reach_%s_%s" % (_cj.SHORT[lay], v)] = (_k_q4reach, (lay, v))
    cases["k_dcdrift_c420_40000_ycb_q2_par"] = (_k_dcdrift_par, (0,))
    cases["k_dcdrift_c420_40000_ycb_q2_par_dri64"] = (_k_dcdrift_par, (64,))
    cases["k_huff_cross_c420"] = (_k_huff_cross, ("4:2:0",))
    cases["k_huff_cross_gray"] = (_k_huff_cross, ("gray",))
    return cases


COEF_CASES = _coef_cases()
COEF_CORRUPT = sorted(k for k in COEF_CASES if k.startswith("k_huff_cross_"))     # legal syntax, a run past position 63


@functools.lru_cache(maxsize=None)
def coef_spec(name):
    fn, args = COEF_CASES[name]
    return fn(*args)


@functools.lru_cache(maxsize=None)
def coef_jpeg_for(name):
    if name in RUNONLY_CASES:
        return _cj.write_jpeg(**runonly_spec(RUNONLY_CASES[name]))
    return _cj.write_jpeg(**coef_spec(name))


# AC symbols with a run of 1 .. 14 and NO magnitude bits (0x10, 0x20, 0x30): no encoder writes one, but a table may hold one, and the
# reference skips the run and stores nothing (jpeg.inl:2246, "if (.. && usHuff)"); libjpeg -- and tests/coef_jpeg.decode_coefs -- end the
# block there, so these files are no members of COEF_CASES and its round trips.  They take the places of 0x51, 0x61 and 0x71 in the
# Annex K tables: codes of 7 and 8 bits, so that the 32 stream bits behind such a symbol, shifted left by its length, are not zero in
# their low half -- which is what a kernel that takes the symbol's "value" from them stores (jda_q4_block did, on the GPU alone).
RUNONLY_CASES = {"x_runonly_gray": "gray", "x_runonly_c420": "4:2:0"}
RUNONLY_SYMBOLS = ((0x51, 0x10), (0x61, 0x20), (0x71, 0x30))
RUNONLY_BLOCKS = ([(1, 0), (0, 0)], [(3, 0), (0, 0)], [(2, 0), (0, 9), (0, 0)], [(1, 0), (1, 0), (0, 0)], [(0, -7), (1, 0), (0, 0)], [(2, 0), (0, 0)])


def runonly_spec(sampling):
    """every other block one of RUNONLY_BLOCKS (the symbols as given: a run without a value lands on zig-zag positions 2, 3 and 4 --
    coefficients 8, 9 and beyond of the 1/4-scale decode --, before and after a real coefficient), the rest one small coefficient"""
    hs, vs = _cj.LUMA_HV[sampling]
    cx, cy = 6, 2
    width, height = cx * 8 * hs, cy * 8 * vs
    coefs = _cj.zero_coefs(width, height, sampling)
    huff = dict(_cj.annex_k()[2])
    for th in (0, 1):
        bits, vals = huff[(1, th)]
        vals = list(vals)
        for old, new in RUNONLY_SYMBOLS:
            vals[vals.index(old)] = new
        huff[(1, th)] = (list(bits), vals)
    rng = _np.random.default_rng(5)
    pairs, k = {}, 0
    for c, arr in enumerate(coefs):
        flat = arr.reshape(-1, 64)
        for i in range(flat.shape[0]):
            flat[i, 0] = int(rng.integers(-60, 60))
            flat[i, 1 + (i % 5)] = int(rng.integers(-40, 40)) or 3
        for by in range(arr.shape[0]):
            for bx in range(arr.shape[1]):
                if (by + bx + c) % 2 == 0:
                    pairs[(c, by, bx)] = RUNONLY_BLOCKS[k % len(RUNONLY_BLOCKS)]
                    k += 1
    return dict(width=width, height=height, sampling=sampling, coefs=coefs, quant={0: [3] * 64, 1: [5] * 64}, huff=huff, ac_pairs=pairs)

