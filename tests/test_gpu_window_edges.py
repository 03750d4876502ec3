"""The scan-window stress streams (k_window_*, k_q4reach_*: tests/cases.py, checked without a GPU by
tests/test_window_streams_cpu.py) on the GPU, where the bytes behind a wavefront's staged slice are not poison but what the
wavefront's window held before -- a previous tile's scan bytes, partly overwritten by its column list.  Every image must be
bit-exact with the oracle: in the layout its index routes it to (asserted from the launch plan's workgroup count), behind a
dense slice in the same wavefront, in P1's chunked mode, through the 1/4 kernel's clamped five-dword loads, and in a pipeline
batch whose average rule puts the "small" images in the small layout, where their one over-window tile reads HBM."""
import math

import numpy as np
import pytest

import jpegdec_amd as J
from tests.cases import COEF_CASES, all_modes, coef_jpeg_for, jpeg_for, lds_layout
from tests.test_window_streams_cpu import SAMPLING, routing, tiles_from, window_tiles

pytestmark = pytest.mark.gpu

WINDOW = sorted(k for k in COEF_CASES if k.startswith("k_window_"))
Q4REACH = sorted(k for k in COEF_CASES if k.startswith("k_q4reach_"))


def _plain(name):
    return J.GRAY8 if "_gray_" in name else J.RGB8888


def _batch(ctx, dimgs, pts, opts):
    """one resident batch over the images -> (stats, [host canvas of every image], status)"""
    outs, geo = [], []
    for d, pt, opt in zip(dimgs, pts, opts):
        g = J.output_geometry(d.info, pt, opt)
        pitch = (g["canvas_w"] * g["bpp"] + 15) & ~15
        ptr = ctx.malloc(pitch * g["canvas_h"])
        ctx.memset(ptr, 0x5a, pitch * g["canvas_h"])
        outs.append((ptr, pitch, g["canvas_w"], g["canvas_h"]))
        geo.append((g, pitch))
    try:
        b = J.Batch(ctx, dimgs, outs, pts, opts)
        try:
            b.decode()
            ctx.sync()
            st, stats = b.status(), dict(b.stats)
        finally:
            b.close()
        canv = [ctx.to_host(o[0], p * g["canvas_h"]).reshape(g["canvas_h"], p)[:, : g["canvas_w"] * g["bpp"]].copy()
                for o, (g, p) in zip(outs, geo)]
    finally:
        for o in outs:
            ctx.free(o[0])
    return stats, canv, st


def _expect_big(jpeg, sampling, on_device):
    idx, scan_len, mx, my = window_tiles(jpeg)
    tiles = tiles_from(idx, scan_len, mx, my, sampling)
    host_big, avg_big = routing(tiles, scan_len, mx, my, sampling)
    return (avg_big if on_device else host_big), len(tiles)


@pytest.mark.parametrize("short", ["gray", "c444", "c422", "c440", "c420"])
def test_routing_and_bits(short, gpu_ctx, oracle):
    """every window case as a resident batch of its own, host index and device pre-scan, at the plain pixel type (the plain kernel
    where the layout has one) and at RGB565-BE half size (the general kernel): the layout the index's rule picks is the launch's
    (workgroups = ceil(tiles / wavefronts of that layout)), both layouts are reached by both kernels, and the pixels are the oracle's"""
    sampling = SAMPLING[short]
    reached = set()
    for name in [k for k in WINDOW if k.startswith("k_window_%s_" % short)]:
        jpeg = coef_jpeg_for(name)
        for device_prescan in (False, True):
            prep = J.PreparedImage(jpeg, device_prescan=device_prescan)
            dimg = J.DeviceImage(gpu_ctx, prep)
            try:
                big, n_tiles = _expect_big(jpeg, sampling, dimg.prescan_on_device)
                for kernel, pt, opt in (("plain", _plain(name), 0), ("general", J.RGB565_BE, J.SCALE_HALF)):
                    stats, (got,), st = _batch(gpu_ctx, [dimg], [pt], [opt])
                    waves = lds_layout(sampling, 1 if big else 0)[1]
                    assert stats["n_workgroups"] == math.ceil(n_tiles / waves), (name, device_prescan, kernel, big, stats)
                    orc, want, err = oracle.decode_canvas(jpeg, pt, opt)
                    assert orc == 1 and st == [0], (name, err, st)
                    assert np.array_equal(got, want), (name, device_prescan, kernel, int(np.count_nonzero(got != want)))
                    reached.add((kernel, big))
            finally:
                dimg.close()
                prep.close()
    assert reached == {(k, b) for k in ("plain", "general") for b in (False, True)}, (short, reached)


@pytest.mark.parametrize("mixed", [False, True])
def test_stale_window_bytes(mixed, gpu_ctx, oracle):
    """~200 images in one resident batch, each layout's densest large-window case alternating with its tight edge cases: the wavefront
    that stages an edge tile is, as often as not, one that has just held a dense slice.  One RGB8888 plan, one of mixed formats"""
    names = []
    for short in ("gray", "c444", "c422", "c440", "c420"):
        names += ["k_window_%s_large" % short, "k_window_%s_small_tight" % short, "k_window_%s_large" % short, "k_window_%s_dri" % short]
    names = names * 10
    preps = {n: J.PreparedImage(coef_jpeg_for(n)) for n in set(names)}
    dimgs = {n: J.DeviceImage(gpu_ctx, p) for n, p in preps.items()}
    try:
        if mixed:
            modes = [(J.RGB8888, 0), (J.RGB565_BE, J.SCALE_HALF), (J.RGB565_LE, 0), (J.RGB8888, J.SCALE_HALF)]
            pts = [modes[i % 4][0] if "_gray_" not in n or modes[i % 4][0] != J.RGB8888 else J.GRAY8 for i, n in enumerate(names)]
            opts = [modes[i % 4][1] for i in range(len(names))]
        else:
            pts, opts = [_plain(n) for n in names], [0] * len(names)
        stats, canv, st = _batch(gpu_ctx, [dimgs[n] for n in names], pts, opts)
        assert st == [0] * len(names)
        want = {}
        for n, pt, opt, got in zip(names, pts, opts, canv):
            if (n, pt, opt) not in want:
                orc, want[(n, pt, opt)], err = oracle.decode_canvas(coef_jpeg_for(n), pt, opt)
                assert orc == 1, (n, err)
            assert np.array_equal(got, want[(n, pt, opt)]), (n, pt, opt, int(np.count_nonzero(got != want[(n, pt, opt)])))
    finally:
        for d in dimgs.values():
            d.close()
        for p in preps.values():
            p.close()


def test_p1_in_chunks_at_the_edge(gpu_ctx, oracle):
    """4:2:0 and 4:4:4 window cases with continuation entries on every image (JDA_PREPARE_CONT_ALWAYS) at RGB8888: the CONT kernels,
    in the small layout ("small" images) and the large one; a tile over the window falls back to whole blocks"""
    for name in [k for k in WINDOW if k.startswith(("k_window_c420_", "k_window_c444_"))]:
        jpeg = coef_jpeg_for(name)
        p = J.PreparedImage(jpeg, flags=J.PREPARE_CONT_ALWAYS)
        try:
            assert len(p.block_cont()[1]) > 0, name
            st, got, g = J.decode_resident(gpu_ctx, p, J.RGB8888, 0)
            orc, want, err = oracle.decode_canvas(jpeg, J.RGB8888, 0)
            assert st == 0 and orc == 1, (name, st, err)
            assert np.array_equal(got, want), (name, int(np.count_nonzero(got != want)))
        finally:
            p.close()


def test_q4_reach(gpu_ctx, oracle):
    """k_q4reach_* at 1/4 in every pixel type, through decode_to_host and through one pipeline batch (which launches the decode before
    the device pre-scan's verdict: the loads are clamped)"""
    from tests.test_gpu_pipeline import _check, _surfaces
    for name in Q4REACH:
        jpeg = coef_jpeg_for(name)
        for pt, opt in all_modes(name):
            if not (opt & J.SCALE_QUARTER):
                continue
            orc, want, err = oracle.decode_canvas(jpeg, pt, opt)
            rc, got, g = J.decode_to_host(gpu_ctx, jpeg, pt, opt)
            assert rc == 0 and orc == 1, (name, pt, opt, rc, err)
            assert np.array_equal(got, want), (name, pt, opt, int(np.count_nonzero(got != want)))
    jp = [coef_jpeg_for(n) for n in Q4REACH]
    pts = [(J.RGB565_LE, J.RGB565_BE, J.GRAY8)[i % 3] for i in range(len(Q4REACH))]
    opts = [J.SCALE_QUARTER] * len(Q4REACH)
    pipe = J.Pipeline(gpu_ctx, max_images=len(jp), depth=2, host_threads=4)
    try:
        outs, metas = _surfaces(gpu_ctx, jp, pts, opts)
        st = pipe.wait(pipe.submit(jp, outs, pts, opts))
        _check(gpu_ctx, oracle, jp, pts, opts, outs, metas, st, Q4REACH)
        for o in outs:
            gpu_ctx.free(o[0])
        assert pipe.stats["failed_images"] == 0, pipe.stats
    finally:
        pipe.close()


def test_pipeline_with_normal_files(gpu_ctx, oracle):
    """the window family with normal files in one pipeline batch: its index comes from the device pre-scan, and the average rule
    puts the "small" images in the small layout, where their one over-window tile takes the general reader"""
    from tests.test_gpu_pipeline import _check, _surfaces
    normal = ["c420_333x217", "c444_333x217", "gray_333x217", "c422_333x217", "c440_200x120"]
    names = normal + WINDOW
    jp = [jpeg_for(n) for n in normal] + [coef_jpeg_for(n) for n in WINDOW]
    pts = [_plain(n) if "gray" not in n else J.GRAY8 for n in names]
    opts = [(0, J.SCALE_HALF)[i % 2] for i in range(len(names))]
    pipe = J.Pipeline(gpu_ctx, max_images=len(names), depth=2, host_threads=4)
    try:
        outs, metas = _surfaces(gpu_ctx, jp, pts, opts)
        st = pipe.wait(pipe.submit(jp, outs, pts, opts))
        _check(gpu_ctx, oracle, jp, pts, opts, outs, metas, st, names)
        for o in outs:
            gpu_ctx.free(o[0])
        s = pipe.stats
        assert s["images"] == len(names) and s["failed_images"] == 0, s
    finally:
        pipe.close()


def test_window_cases_match_real_reference_when_present(gpu_ctx, ref_scalar):
    """one case per layout and family against oracle/_ref itself, in four modes"""
    names = [k for k in WINDOW if k.endswith(("_small_tight", "_dri"))] + [k for k in Q4REACH if k.endswith(("_phase", "_end1"))]
    for name in names:
        jpeg = coef_jpeg_for(name)
        for pt, opt in ((J.RGB565_LE, 0), (J.RGB565_BE, J.SCALE_HALF), (J.GRAY8, J.SCALE_QUARTER), (J.RGB565_LE, J.SCALE_QUARTER)):
            rc, got, g = J.decode_to_host(gpu_ctx, jpeg, pt, opt)
            r = ref_scalar.decode_cb(jpeg, pt, opt)
            assert rc == 0 and r["rc"] == 1, (name, pt, opt)
            want = r["canvas"][: g["out_h"], : g["canvas_w"] * g["bpp"]]
            assert np.array_equal(got[: g["out_h"]], want), (name, pt, opt)
