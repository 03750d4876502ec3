"""The decode kernel's pool: a launch that fills the GPU with tiles of one table generation keeps its last quads (groups of as many
tiles as the workgroup has wavefronts) out of the static split, and the workgroups that have drawn their own run claim them a quad at a
time from a counter in global memory (jda_pool_resolve in jda_kernels.hip).

jda_internal_set_decode_pool(4, 250) caps the launches at four workgroups and puts a quarter of the quads into the pool, so that a
1280x720 image (360 tiles of 4:2:0 = 23 quads: runs of 4 or 5 own quads, a pool of 5, so one or two chunks per workgroup and the failing
claim of each) runs what the 64-image batch runs on 256 CUs.  Every case is compared with the oracle byte for byte, and
jda_internal_decode_pool_last says what the last launch did: the pool's quads, claims made == pool + workgroups, failing claims ==
workgroups, and that the launch left its counters zeroed (else it returns an error)."""
import ctypes as C

import numpy as np
import pytest

import jpegdec_amd as J
from jpegdec_amd.synth import synth_jpeg
from tests.cases import jpeg_for

pytestmark = pytest.mark.gpu

GRID, PERMILLE = 4, 250
CHUNKS = 32                      # JDA_POOL_CHUNKS: quads a workgroup can take from the pool


def expected_pool(n_quads, grid=GRID, permille=PERMILLE):
    """launch_persistent's rule under a forced cap"""
    if n_quads < grid:
        return 0
    return max(0, min(n_quads * permille // 1000, CHUNKS // 2 * grid, n_quads - 3 * grid))


def pool_last(lib):
    out = (C.c_int32 * 4)()
    lib.jda_internal_decode_pool_last.argtypes = [C.POINTER(C.c_int32)]
    assert lib.jda_internal_decode_pool_last(out) == 0, "the last launch did not leave its counters zeroed"
    return list(out)


@pytest.fixture
def forced_pool(gpu_ctx):
    lib = gpu_ctx.lib
    lib.jda_internal_set_decode_pool.argtypes = [C.c_int32, C.c_int32]
    assert lib.jda_internal_set_decode_pool(GRID, PERMILLE) == 0
    yield lib
    assert lib.jda_internal_set_decode_pool(0, 0) == 0


_files, _canvases = {}, {}


def file_of(key):
    """key: a name of tests/cases.py or (width, height, subsampling, seed, quality, noise)"""
    if key not in _files:
        _files[key] = jpeg_for(key) if isinstance(key, str) else synth_jpeg(key[0], key[1], key[2], seed=key[3], quality=key[4], noise=key[5])
    return _files[key]


def canvas_of(oracle, key, pt, opt):
    if (key, pt, opt) not in _canvases:
        rc, want, err = oracle.decode_canvas(file_of(key), pt, opt)
        assert rc == 1, (key, pt, opt, err)
        want.setflags(write=False)
        _canvases[(key, pt, opt)] = want
    return _canvases[(key, pt, opt)]


class Plan:
    """one Batch over resident images, each with a zeroed surface of its own"""

    def __init__(self, ctx, keys, pt, opt, flags=0):
        self.ctx, self.keys, self.pt, self.opt = ctx, keys, pt, opt
        self.prep = [J.PreparedImage(file_of(k), flags=flags) for k in keys]
        self.dev = [J.DeviceImage(ctx, p) for p in self.prep]
        self.geo = [p.geometry(pt, opt) for p in self.prep]
        self.pitch = [(g["canvas_w"] * g["bpp"] + 15) & ~15 for g in self.geo]
        self.surf = [ctx.malloc(p * g["canvas_h"]) for p, g in zip(self.pitch, self.geo)]
        for s, p, g in zip(self.surf, self.pitch, self.geo):
            ctx.memset(s, 0, p * g["canvas_h"])
        self.batch = J.Batch(ctx, self.dev, [(s, p, g["canvas_w"], g["canvas_h"]) for s, p, g in zip(self.surf, self.pitch, self.geo)],
                             [pt] * len(keys), [opt] * len(keys))
        self.n_quads = self.batch.stats["n_workgroups"]          # (one launch list: its quads)
        assert self.batch.stats["n_launches"] == 1

    def check(self, oracle):
        for k, s, p, g in zip(self.keys, self.surf, self.pitch, self.geo):
            got = self.ctx.to_host(s, p * g["canvas_h"]).reshape(g["canvas_h"], p)[:, : g["canvas_w"] * g["bpp"]]
            want = canvas_of(oracle, k, self.pt, self.opt)
            assert got.shape == want.shape and np.array_equal(got, want), (k, self.pt, self.opt, int(np.count_nonzero(got != want)))

    def close(self):
        self.batch.close()
        for s in self.surf:
            self.ctx.free(s)
        for d in self.dev:
            d.close()
        for p in self.prep:
            p.close()


def run_pooled(ctx, lib, oracle, keys, pt, opt, flags=0, n_quads=None):
    """decode, compare, and hold the launch to its pool -> (n_quads, n_pool)"""
    plan = Plan(ctx, keys, pt, opt, flags)
    try:
        if n_quads is not None:
            assert plan.n_quads == n_quads, plan.batch.stats
        plan.batch.decode()
        ctx.sync()
        n_pool, claims, failing, slot = pool_last(lib)
        plan.check(oracle)
        assert n_pool == expected_pool(plan.n_quads) and n_pool > 0, (plan.n_quads, n_pool)
        assert (claims, failing) == (n_pool + GRID, GRID) and slot >= 0, (n_pool, claims, failing, slot)
        return plan.n_quads, n_pool
    finally:
        plan.close()


C420, C444, GRAY = "c420_1280x720", (1280, 720, "4:4:4", 41, 85, False), (1280, 720, "gray", 42, 85, False)


@pytest.mark.parametrize("pt", [J.RGB8888, J.RGB565_LE, J.GRAY8])
def test_720p_420_plain_kernels(pt, gpu_ctx, oracle, forced_pool):
    """360 tiles = 23 quads on four workgroups: own runs of 5, 5, 4, 4 quads and a pool of 5"""
    assert run_pooled(gpu_ctx, forced_pool, oracle, [C420], pt, 0, n_quads=23) == (23, 5)


@pytest.mark.parametrize("key,pt", [(C444, J.RGB8888), (C444, J.RGB565_LE), (C444, J.GRAY8), (GRAY, J.GRAY8), (GRAY, J.RGB565_LE)])
def test_720p_444_and_gray(key, pt, gpu_ctx, oracle, forced_pool):
    """4:4:4: 8 tiles of 20 MCUs a row x 90 rows = 45 quads of 16; gray: 3 tiles of 64 blocks a row x 90 rows = 270 tiles = 18 quads of 15
    (the gray workgroup has 15 wavefronts)"""
    run_pooled(gpu_ctx, forced_pool, oracle, [key], pt, 0, n_quads=45 if key is C444 else 18)


@pytest.mark.parametrize("pt,opt", [(J.RGB565_BE, 0), (J.RGB8888, J.SCALE_HALF)])
def test_general_kernel_and_half_scale(pt, opt, gpu_ctx, oracle, forced_pool):
    run_pooled(gpu_ctx, forced_pool, oracle, [C420], pt, opt, n_quads=23)


def test_p1_in_chunks(gpu_ctx, oracle, forced_pool):
    """continuation entries on every image: the CONT kernel"""
    before = sum(n for k, n in J.kernel_launch_counts().items() if "jda_decode_tiles_persistentILi2ELi1ELi1ELi1EE" in k)
    run_pooled(gpu_ctx, forced_pool, oracle, [C420], J.RGB8888, 0, flags=J.PREPARE_CONT_ALWAYS, n_quads=23)
    assert sum(n for k, n in J.kernel_launch_counts().items() if "jda_decode_tiles_persistentILi2ELi1ELi1ELi1EE" in k) == before + 1


def test_large_window(gpu_ctx, oracle, forced_pool):
    """uniform noise whose tiles' scan slices need the large window: 15 wavefronts, a quad is 15 tiles; 2 tiles a row x 240 rows = 32 quads,
    runs of 6 own quads and a pool of 8"""
    assert run_pooled(gpu_ctx, forced_pool, oracle, [(320, 3840, "4:2:0", 71, 75, True)], J.RGB8888, 0, n_quads=32) == (32, 8)


def test_pool_spans_image_boundaries(gpu_ctx, oracle, forced_pool):
    """four images with equal tables, 23 + 23 + 23 + 12 quads (a list runs the pool when its images average 16 quads and more): the pool of
    20 holds the last image and eight quads of the third"""
    keys = [C420, (1280, 720, "4:2:0", 43, 85, False), (1280, 720, "4:2:0", 44, 85, False), (1280, 368, "4:2:0", 45, 85, False)]
    assert run_pooled(gpu_ctx, forced_pool, oracle, keys, J.RGB8888, 0, n_quads=81) == (81, 20)


def test_small_images_run_the_static_split(gpu_ctx, oracle, forced_pool):
    """equal tables, but 2 quads an image: a pool tile would start cold nearly every time, so the list keeps the static split"""
    plan = Plan(gpu_ctx, [(320, 240, "4:2:0", 47, 85, False)] * 12, J.RGB8888, 0)
    try:
        assert plan.n_quads == 24
        plan.batch.decode()
        gpu_ctx.sync()
        assert pool_last(forced_pool) == [0, 0, 0, -1]
        plan.check(oracle)
    finally:
        plan.close()


def test_two_table_generations_run_the_static_split(gpu_ctx, oracle, forced_pool):
    """images with different quantisers: two generations in one list, no pool"""
    plan = Plan(gpu_ctx, [C420, (1280, 720, "4:2:0", 46, 50, False)], J.RGB8888, 0)
    try:
        plan.batch.decode()
        gpu_ctx.sync()
        assert pool_last(forced_pool) == [0, 0, 0, -1]
        plan.check(oracle)
    finally:
        plan.close()


def test_three_decodes_back_to_back(gpu_ctx, oracle, forced_pool):
    """no synchronisation between the launches: each finds the counters as the one before left them -- zeroed"""
    plans = [Plan(gpu_ctx, [C420], pt, 0) for pt in (J.RGB8888, J.RGB8888, J.RGB565_LE)]
    try:
        for p in plans:
            p.batch.decode()
        gpu_ctx.sync()
        n_pool, claims, failing, slot = pool_last(forced_pool)
        for p in plans:
            p.check(oracle)
        assert (n_pool, claims, failing) == (5, 5 + GRID, GRID)
    finally:
        for p in plans:
            p.close()


def test_defaults_give_a_small_image_no_pool(gpu_ctx, oracle):
    lib = gpu_ctx.lib
    lib.jda_internal_set_decode_pool.argtypes = [C.c_int32, C.c_int32]
    assert lib.jda_internal_set_decode_pool(0, 0) == 0
    plan = Plan(gpu_ctx, [C420], J.RGB8888, 0)
    try:
        plan.batch.decode()
        gpu_ctx.sync()
        assert pool_last(lib) == [0, 0, 0, -1]
        plan.check(oracle)
    finally:
        plan.close()
