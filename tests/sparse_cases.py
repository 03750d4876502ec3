"""Coefficient sets at the edges of the sparse load phase (jda_sparse_tiles), shared by tests/test_sparse_coef_cpu.py and
tests/test_gpu_sparse_coef.py.  Every set is (label, header JPEG, coefficients in the library's order, pixel type, options): the header file
is written by coef_jpeg.write_jpeg with zero coefficients (geometry and quantisers only), the coefficients are made here with numpy and
go in through jda_coef_image_from_coefficients.  All small: the smallest shapes at which the phase can go wrong."""
import functools

import numpy as np

from tests import coef_jpeg

RGB8888, RGB565_LE, GRAY8, LUMA_ONLY = 2, 0, 3, 64      # (jpegdec_amd.RGB8888 ..: this module imports nothing of the product)
NBLK = {"gray": 1, "4:4:4": 3, "4:2:2": 4, "4:4:0": 4, "4:2:0": 6}
MCUS_PER_TILE = {"gray": 64, "4:4:4": 20, "4:2:2": 16, "4:4:0": 16, "4:2:0": 10}
# lengths of the entry ranges of the twelve tiles (MCU rows) of the "ranges" image, and where each range starts modulo four entries (16 bytes)
RANGE_LENGTHS = [63, 64, 65, 255, 256, 257, 1, 1, 2, 5, 4, 3]
RANGE_STARTS_MOD4 = [0, 3, 3, 0, 3, 3, 0, 1, 2, 0, 1, 1]


@functools.lru_cache(maxsize=None)
def header(width, height, sampling):
    quant = {0: [2] * 64} if sampling == "gray" else {0: [2] * 64, 1: [3] * 64}
    return coef_jpeg.write_jpeg(width, height, sampling, coef_jpeg.zero_coefs(width, height, sampling), quant)


def n_blocks(width, height, sampling):
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(width, height, sampling)
    return cx * cy * NBLK[sampling]


def _random(rng, nb, density):
    """nb blocks with about `density` of the 64 positions nonzero, values in -40..40"""
    c = rng.integers(-40, 41, size=(nb, 64)).astype(np.int16)
    c[rng.random((nb, 64)) >= density] = 0
    return c


@functools.lru_cache(maxsize=None)
def edge_sets():
    rng = np.random.default_rng(20240)
    sets = []

    def add(label, w, h, sampling, coefs, pt=None, opt=0):
        assert coefs.shape == (n_blocks(w, h, sampling), 64) and coefs.dtype == np.int16
        sets.append((label, header(w, h, sampling), np.ascontiguousarray(coefs), (GRAY8 if sampling == "gray" else RGB8888) if pt is None else pt, opt))

    # every block of the tile empty, DC 0 included: no entry in the range
    add("empty_gray", 512, 8, "gray", np.zeros((64, 64), np.int16))
    add("empty_c420", 32, 32, "4:2:0", np.zeros((24, 64), np.int16))
    # an image whose only entries lie in its LAST tile: every range in front of it is empty and starts at 0
    c = np.zeros((128, 64), np.int16)
    c[100, 5] = 7
    add("empty_then_one", 512, 16, "gray", c)
    # all 64 coefficients of a block nonzero beside empty blocks
    c = np.zeros((64, 64), np.int16)
    c[::2] = rng.integers(1, 30, size=(32, 64)).astype(np.int16) * rng.choice(np.array([-1, 1], np.int16), size=(32, 64))
    add("full_beside_empty", 512, 8, "gray", c)
    # a gray 64-block tile with 64 entries in every block: 4,096 entries, the longest range; a second tile behind it
    c = np.zeros((128, 64), np.int16)
    c[:64] = rng.integers(1, 20, size=(64, 64)).astype(np.int16) * rng.choice(np.array([-1, 1], np.int16), size=(64, 64))
    c[64:] = _random(rng, 64, 0.1)
    add("gray_full_tile", 512, 16, "gray", c)
    # entry ranges of 63 .. 257 entries, and ranges that start 1, 2 and 3 entries past a 16-byte boundary: one tile an MCU row
    c = np.zeros((64 * len(RANGE_LENGTHS), 64), np.int16)
    for t, ln in enumerate(RANGE_LENGTHS):
        flat = c[64 * t:64 * (t + 1)].reshape(-1)
        pos = np.sort(rng.choice(4096, size=ln, replace=False))
        flat[pos] = rng.integers(1, 30, size=ln).astype(np.int16)
    add("ranges", 512, 8 * len(RANGE_LENGTHS), "gray", c)
    # the values at the ends of the 16 bits, in the DC place and in AC places
    c = np.zeros((8, 64), np.int16)
    c[0, 0], c[1, 0], c[2, 0] = -32768, -1, 1
    c[3, 1], c[4, 63], c[5, 8] = -32768, -1, 1
    c[6, [0, 7, 56]] = [-1, -32768, 1]
    c[7, [1, 2, 9]] = [1, -1, -32768]
    add("values", 64, 8, "gray", c)
    # 33 x 33 blocks: the tile of MCU row 31 covers blocks 1023 .. 1055, so the ten block bits wrap inside a tile
    add("wrap_264", 264, 264, "gray", _random(rng, 33 * 33, 0.08))
    # a last (and only) tile of one MCU in each layout
    for sampling, (w, h) in (("gray", (8, 8)), ("4:2:0", (16, 16)), ("4:2:2", (16, 8)), ("4:4:0", (8, 16)), ("4:4:4", (8, 8))):
        add("one_mcu_" + coef_jpeg.SHORT[sampling], w, h, sampling, _random(rng, NBLK[sampling], 0.3))
    # a tile that is not full and one more MCU behind a full one, in each colour layout
    for sampling, (w, h) in (("4:2:0", (16 * 11, 32)), ("4:2:2", (16 * 17, 16)), ("4:4:0", (8 * 17, 32)), ("4:4:4", (8 * 21, 16))):
        add("rows_" + coef_jpeg.SHORT[sampling], w, h, sampling, _random(rng, n_blocks(w, h, sampling), 0.12))
    # JDA_LUMA_ONLY on a colour image
    add("luma_only_c420", 48, 32, "4:2:0", _random(rng, n_blocks(48, 32, "4:2:0"), 0.2), RGB565_LE, LUMA_ONLY)
    return sets
