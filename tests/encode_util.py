"""The baseline encoder of jda_encode_surfaces stated in numpy: libjpeg's rules, checked against Pillow in
tests/test_encode_cpu.py.  It shares no code with the product: quantisers, colour, padding and downsampling, the islow FDCT and
the quantisation are written out here; entropy coding and the file are tests/coef_jpeg.write_jpeg's.

  quant_tables(q)                      {0: luma, 1: chroma} in zig-zag order (libjpeg's jpeg_set_quality)
  coefficients(img, sampling, q)      per component (block rows, block columns, 64) zig-zag arrays over the MCU grid, dummy blocks included
  file_bytes(img, sampling, q, ri)    the whole file

and the pictures of the test grid, LONG_JOBS among them: the jobs that take the scan stage past one element a lane.

img: H x W x 3 or 4 (R, G, B[, A]) uint8 for the colour samplings, H x W uint8 for "gray"."""
import functools

import numpy as np

from jpegdec_amd.synth import _ZIGZAG
from tests import coef_jpeg

SAMPLINGS = ("gray", "4:4:4", "4:2:2", "4:2:0")
SAMPLING_ID = {"gray": 0, "4:4:4": 1, "4:2:2": 2, "4:2:0": 3}          # jda_encode_job.sampling
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}

_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
_ZZ = np.asarray(_ZIGZAG)                                              # zig-zag position -> natural index


def quant_natural(q):
    """(luma, chroma) in natural order"""
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(t, dtype=np.int64) * s + 50) // 100, 1, 255) for t in (_LUMA, _CHROMA))


def quant_tables(q, sampling="4:2:0"):
    lum, chrom = quant_natural(q)
    out = {0: [int(v) for v in lum[_ZZ]]}
    if sampling != "gray":
        out[1] = [int(v) for v in chrom[_ZZ]]
    return out


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    """replicate the last column to `cols` columns and the last row to `rows` rows"""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def component_planes(img, sampling):
    """per component the sample plane over its blocks of the MCU grid (what lies under a dummy block is padding, and unused)"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(w, h, sampling)
    if sampling == "gray":
        assert img.ndim == 2
        return [_pad(img.astype(np.int64), shapes[0][0] * 8, shapes[0][1] * 8)]
    y, cb, cr = ycc(img)
    out = [_pad(y, shapes[0][0] * 8, shapes[0][1] * 8)]
    for p in (cb, cr):
        cw, ch = -(-w // hs), -(-h // vs)
        wb = -(-cw // 8)
        full = _pad(p, -(-h // vs) * vs, wb * 8 * hs)              # right: to the component's real blocks; down: to a multiple of v_max / v_c only
        if hs == 2 and vs == 2:
            bias = 1 + (np.arange(full.shape[1] // 2) & 1)
            ds = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + bias) >> 2
        elif hs == 2:
            bias = np.arange(full.shape[1] // 2) & 1
            ds = (full[:, 0::2] + full[:, 1::2] + bias) >> 1
        else:
            ds = full
        assert ds.shape[0] == ch
        out.append(_pad(ds, shapes[1][0] * 8, shapes[1][1] * 8))   # the downsampled plane goes down to the MCU grid's block rows
    return out


_C = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069, c2053=16819,
          c2562=20995, c3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """one pass of jfdctint.c over the LAST axis of d (.., 8)"""
    k = _C
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 13 - 2 if first else 13 + 2
    if first:
        out[..., 0] = (t10 + t11) << 2
        out[..., 4] = (t10 - t11) << 2
    else:
        out[..., 0] = _descale(t10 + t11, 2)
        out[..., 4] = _descale(t10 - t11, 2)
    z1 = (t12 + t13) * k["c0541"]
    out[..., 2] = _descale(z1 + t13 * k["c0765"], n)
    out[..., 6] = _descale(z1 - t12 * k["c1847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * k["c1175"]
    t4, t5, t6, t7 = t4 * k["c0298"], t5 * k["c2053"], t6 * k["c3072"], t7 * k["c1501"]
    z1, z2, z3, z4 = -z1 * k["c0899"], -z2 * k["c2562"], -z3 * k["c1961"] + z5, -z4 * k["c0390"] + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def fdct(blocks):
    """(.., 8, 8) samples -> (.., 8, 8) DCT x 8"""
    d = _pass(blocks.astype(np.int64) - 128, True)                  # rows
    return _pass(d.swapaxes(-1, -2), False).swapaxes(-1, -2)        # columns


def quantise(c, q):
    d = q.astype(np.int64) << 3
    r = (np.abs(c) + (d >> 1)) // d
    return np.where(c < 0, -r, r)


def coefficients(img, sampling, quality):
    img = np.asarray(img)
    h, w = img.shape[:2]
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(w, h, sampling)
    lum, chrom = quant_natural(quality)
    out = []
    for c, plane in enumerate(component_planes(img, sampling)):
        rows, cols = shapes[c]
        blocks = plane.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)
        qz = quantise(fdct(blocks), (lum if c == 0 else chrom).reshape(8, 8)).reshape(rows, cols, 64)[..., _ZZ]
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        wb, hb = -(-(-(-w * ch // hs)) // 8), -(-(-(-h * cv // vs)) // 8)
        if wb < cols or hb < rows:                                  # dummy blocks, in the MCU's block order: DC of the block before, no AC
            for my in range(cy):
                for mx in range(cx):
                    prev = None
                    for v in range(cv):
                        for hh in range(ch):
                            by, bx = my * cv + v, mx * ch + hh
                            if bx >= wb or by >= hb:
                                assert prev is not None
                                qz[by, bx] = 0
                                qz[by, bx, 0] = prev
                            prev = qz[by, bx, 0]
        out.append(qz)
    return out


def file_bytes(img, sampling, quality, restart_interval=0, return_layout=False):
    img = np.asarray(img)
    h, w = img.shape[:2]
    return coef_jpeg.write_jpeg(w, h, sampling, coefficients(img, sampling, quality), quant_tables(quality, sampling),
                                restart_interval=restart_interval, pad_to=0, return_layout=return_layout)


# ---- pictures of the test grid -------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (8, 24), (17, 9), (25, 16), (33, 47), (40, 40), (64, 7), (7, 64), (129, 65))          # (w, h)
SECOND_TILE_WIDTH = {"gray": 528, "4:4:4": 360, "4:2:2": 272, "4:2:0": 184}


def picture(kind, w, h, sampling, seed=0):
    """'noise' | 'smooth' | 'pixels' (a pixel checkerboard) | 'blocks' (an 8x8-block checkerboard) | 'flat' (every sample 200): H x W (gray)
    or H x W x 4 uint8"""
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.RandomState(seed * 7919 + w * 131 + h)
    if kind == "noise":
        a = rng.randint(0, 256, size=(h, w, 4))
    elif kind == "smooth":
        a = np.stack([(xx * 3 + yy * 2 + seed) % 256, (128 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.int64), (yy * 5 + xx) % 256, xx * 0 + 255], -1)
    elif kind == "pixels":
        a = np.repeat((((xx + yy) & 1) * 255)[..., None], 4, -1)
    elif kind == "blocks":
        a = np.repeat(((((xx >> 3) + (yy >> 3)) & 1) * 255)[..., None], 4, -1)
    elif kind == "flat":
        a = np.full((h, w, 4), 200)
    else:
        raise ValueError(kind)
    a = a.astype(np.uint8)
    return np.ascontiguousarray(a[..., 1]) if sampling == "gray" else np.ascontiguousarray(a)


def restart_intervals(w, h, sampling):
    """0, 1, 3, the MCUs of a row, all MCUs, all + 1"""
    cx, cy = coef_jpeg.geometry(w, h, sampling)[:2]
    return sorted({0, 1, 3, cx, cx * cy, cx * cy + 1})


# ---- long jobs: a lane of the scan stage sums a run of per = ceil(n / 256) elements -- a job's blocks, then its 64-byte chunks ----------
SCAN_LANES, CHUNK = 256, 64
# (kind, w, h, sampling, quality, restart interval, seed) -> what the job is in the list for (long_job_facts: asserted from the twin)
LONG_JOBS = (
    (("noise", 264, 240, "gray", 75, 1, 11), {"starts": 4}),           # 990 blocks, per 4, an interval a block
    (("noise", 264, 240, "gray", 75, 2, 12), {"starts": 2}),
    (("noise", 264, 240, "gray", 75, 3, 13), {"starts": 2}),
    (("noise", 256, 128, "4:4:4", 75, 1, 14), {"starts": 2}),          # 1536 blocks, per 6, an interval every 3
    (("noise", 368, 184, "4:2:2", 75, 1, 15), {"starts": 2}),          # 2116 blocks, per 9, every 4
    (("noise", 352, 352, "4:2:0", 75, 1, 16), {"starts": 2}),          # 2904 blocks, per 12, every 6
    (("noise", 160, 160, "4:4:4", 100, 0, 17), {"chunk_per": 3}),      # 1200 blocks, per 5; a file of about 105 KB: the chunks' scan
    (("flat", 2056, 8, "gray", 1, 0, 0), {"in_a_dword": 5, "shared": ((63, 64), (255, 256))}),      # 257 blocks of 6 bits behind the first
    (("flat", 2056, 8, "gray", 75, 0, 0), {"in_a_dword": 5, "shared": ((63, 64), (255, 256))}),
    (("flat", 264, 240, "gray", 1, 0, 0), {"in_a_dword": 5, "shared": ((63, 64), (255, 256))}),     # 990
    (("flat", 264, 240, "gray", 75, 0, 0), {"in_a_dword": 5, "shared": ((63, 64), (255, 256))}),
)


def long_job_case(job):
    kind, w, h, sampling, q, ri, seed = job
    return picture(kind, w, h, sampling, seed), sampling, q, ri


@functools.lru_cache(maxsize=None)
def long_job_twin(job):
    """(the twin's file, its layout)"""
    return file_bytes(*long_job_case(job), return_layout=True)


def long_job_facts(job):
    """From the TWIN's layout alone: starts = the most interval starts in one lane's run of blocks; chunk_per = the run of a lane of the
    chunks' scan (the header's chunks left out: they only add); in_a_dword = the most blocks with a bit in one dword of the unstuffed scan;
    shared = the pairs of neighbouring blocks (a, a + 1), a + 1 a multiple of 64, that have bits in one dword."""
    kind, w, h, sampling, q, ri, seed = job
    jpeg, lay = long_job_twin(job)
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(w, h, sampling)
    n = len(lay["blocks"])
    bpm = n // (cx * cy)
    per, period = -(-n // SCAN_LANES), ri * bpm
    first = np.zeros(n, dtype=np.int64)
    first[0] = 1
    if period:
        first[::period] = 1
    starts = max(int(first[i:i + per].sum()) for i in range(0, n, per))
    assert lay["scan_bits"] % 8 == 0
    chunk_per = -(-(-(-(lay["scan_bits"] // 8) // CHUNK)) // SCAN_LANES)
    p0 = np.asarray([blk[3][0] for blk in lay["blocks"]], dtype=np.int64)
    p1 = np.asarray([blk[4][-1][0] + blk[4][-1][1] + max(blk[4][-1][2], 0) if blk[4] else blk[3][0] + blk[3][1] + blk[3][2] for blk in lay["blocks"]], dtype=np.int64)
    d0, d1 = p0 >> 5, (p1 - 1) >> 5                                    # a block's first and last dword
    count = np.zeros(int(d1[-1]) + 2, dtype=np.int64)
    np.add.at(count, d0, 1)
    np.add.at(count, d1 + 1, -1)
    shared = tuple((a, a + 1) for a in range(63, n - 1, 64) if d1[a] == d0[a + 1])
    return dict(blocks=n, per=per, period=period, starts=starts, chunk_per=chunk_per, in_a_dword=int(np.cumsum(count).max()), shared=shared)


def long_job_holds(job, why):
    """whether the job, by its twin, is what LONG_JOBS lists it for"""
    f = long_job_facts(job)
    return all(set(v) <= set(f[k]) if k == "shared" else f[k] >= v for k, v in why.items())


def long_batch(sampling_class):
    """'gray' | 'colour' -> (cases, per case its LONG_JOBS entry or None): the LONG_JOBS of one pixel size with a 1 x 1 job in front of,
    between and behind them -- a job's blocks and chunks begin in the middle of a wavefront, and the bisections over the jobs run over
    large block0 / chunk0"""
    jobs = [(job, why) for job, why in LONG_JOBS if (job[3] == "gray") == (sampling_class == "gray")]
    cases, whys = [], []
    for k, (job, why) in enumerate(jobs):
        cases += [(picture("noise", 1, 1, job[3], seed=k), job[3], 75, k % 2), long_job_case(job)]
        whys += [None, (job, why)]
    cases.append((picture("noise", 1, 1, jobs[-1][0][3], seed=99), jobs[-1][0][3], 75, 0))
    whys.append(None)
    return cases, whys


# ---- zero runs of 16 and more: a ZRL symbol for every 16 zeros in front of a coefficient ------------------------------------------------------
ZRL_RUNS = (15, 16, 31, 32, 47, 48, 62)                                # the zeros in front of a block's only AC coefficient
ZRL_QUALITY = 20


def zrl_picture(amplitude=100):
    """gray, a block for every run of ZRL_RUNS: 128 + amplitude x the DCT basis function at zig-zag position run + 1 -- at ZRL_QUALITY the
    only AC coefficient the twin keeps (the test asserts it from the twin's symbols)"""
    yy, xx = np.mgrid[0:8, 0:8]
    blocks = []
    for run in ZRL_RUNS:
        v, u = divmod(int(_ZZ[run + 1]), 8)
        blocks.append(128 + amplitude * np.cos((2 * xx + 1) * u * np.pi / 16) * np.cos((2 * yy + 1) * v * np.pi / 16))
    return np.ascontiguousarray(np.clip(np.rint(np.concatenate(blocks, axis=1)), 0, 255).astype(np.uint8))
