"""jda_encode_surfaces on the GPU, against the numpy twin (tests/encode_util.py; tests/test_encode_cpu.py holds the twin to Pillow): (a) the
whole grid, ONE call per (sampling, restart interval), the jobs as rectangles at unaligned places inside larger guard-filled surfaces, the
files back to back in one guard-filled allocation; (b) fitting and too-small capacities in one call; (c) the product's own decode of every
file; (d) jda_transcode_to_host against the twin over the oracle's canvas, cut and resized by tests/resize_util.py; (e) thumbnails() over a
list of mixed sizes and samplings; (f) the refusals, which launch nothing; (g) every encode kernel in the launch counts; (h) the long jobs
of tests/encode_util.LONG_JOBS -- runs of many blocks and chunks a lane of the scan stage, several interval starts in a run, dwords of the
unstuffed scan that wavefronts and workgroups share -- and the inputs of the named edges of tests/test_encode_cpu.py.  All bit-exact."""
import functools

import numpy as np
import pytest

import jpegdec_amd as J
from tests import coef_jpeg
from tests import encode_prog_util as P
from tests import encode_util as E
from tests import orient_util as U
from tests import resize_util as R
from tests.cases import jpeg_for
from tests.test_encode_cpu import ALL_EDGES, ZRL_WANT, edge_cases, twin_layout, zrl_symbols
from tests.test_gpu_resize import visible_pixels

pytestmark = pytest.mark.gpu

FILL = 0x5A
INVALID, DECODE_ERROR, MEMORY = 1, 2, 5
KERNELS = ("jda_encode_blocks", "jda_encode_lengths", "jda_encode_scan", "jda_encode_emit", "jda_encode_count", "jda_encode_write")
GRID_PICTURES = (("noise", 75), ("smooth", 30), ("pixels", 100), ("blocks", 100))
FILES = {"gray": "gray_333x217", "4:4:4": "c444_333x217", "4:2:2": "c422_333x217", "4:2:0": "c420_333x217"}


def encode_counts():
    c = J.kernel_launch_counts()
    return {k: sum(v for name, v in c.items() if k in name) for k in KERNELS}


@functools.lru_cache(maxsize=None)
def twin(kind, w, h, sampling, q, ri, seed=0):
    return E.file_bytes(E.picture(kind, w, h, sampling, seed), sampling, q, ri)


def interval(w, h, sampling, k):
    """choice k of: none, 1, 3, the MCUs of a row, all MCUs, all + 1"""
    cx, cy = coef_jpeg.geometry(w, h, sampling)[:2]
    return (0, 1, 3, cx, cx * cy, cx * cy + 1)[k]


def encode_batch(ctx, cases, caps=None, slack=5):
    """cases: [(img, sampling, q, ri)] of one pixel size.  Rectangle i at (3 + i % 3, 2 + i % 2) of a FILL-filled surface, the files back to
    back (capacity: the twin's size + slack unless given).  -> (files or None, sizes, statuses); the guard behind every file is checked."""
    n = len(cases)
    bpp = 1 if cases[0][1] == "gray" else 4
    srcs, jobs, blobs, soff = [], [], [], 0
    for i, (img, sampling, q, ri) in enumerate(cases):
        h, w = img.shape[:2]
        x, y = 3 + i % 3, 2 + i % 2
        pitch = ((w + 8) * bpp + 3) & ~3
        s = np.full((h + 5, pitch), FILL, dtype=np.uint8)
        s[y:y + h, x * bpp:(x + w) * bpp] = img.reshape(h, w * bpp)
        blobs.append(s)
        srcs.append((soff, pitch, w + 8, h + 5))
        jobs.append((x, y, w, h, sampling, q, ri))
        soff += (s.size + 15) & ~15
    if caps is None:
        caps = [len(E.file_bytes(*c)) + slack for c in cases]
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    total = int(offs[-1]) + 16
    dsrc, ddst = ctx.malloc(soff), ctx.malloc(total)
    try:
        for s, (o, _, _, _) in zip(blobs, srcs):
            ctx.from_host(dsrc + o, s.reshape(-1))
        ctx.memset(ddst, FILL, total)
        before = encode_counts()
        nbytes, status = J.encode_surfaces(ctx, [(dsrc + o, p, w, h) for o, p, w, h in srcs], bpp, jobs, [ddst + int(o) for o in offs[:-1]], caps)
        after = encode_counts()
        assert {k: after[k] - before[k] for k in KERNELS} == dict(zip(KERNELS, (1, 1, 2, 1, 1, 1))), "a fixed number of launches a call"
        got = ctx.to_host(ddst, total)
    finally:
        ctx.free(dsrc)
        ctx.free(ddst)
    files = []
    for i in range(n):
        o = int(offs[i])
        if status[i] == 0:
            files.append(got[o:o + nbytes[i]].tobytes())
            assert np.all(got[o + nbytes[i]:o + caps[i]] == FILL), i
        else:
            files.append(None)
            assert np.all(got[o:o + caps[i]] == FILL), i
    assert np.all(got[int(offs[-1]):] == FILL)
    return files, nbytes, status


@pytest.mark.parametrize("k", range(6))
@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_whole_grid_one_call(sampling, k, gpu_ctx):
    cases, names = [], []
    for w, h in E.SIZES:
        for kind, q in GRID_PICTURES:
            ri = interval(w, h, sampling, k)
            cases.append((E.picture(kind, w, h, sampling), sampling, q, ri))
            names.append((kind, w, h, sampling, q, ri))
    if k == 2:      # more than eight intervals (RSTm wraps), and a row of more than 64 blocks
        cases.append((E.picture("noise", 129, 65, sampling, 5), sampling, 75, 2))
        names.append(("noise", 129, 65, sampling, 75, 2, 5))
        w = E.SECOND_TILE_WIDTH[sampling]
        cases.append((E.picture("noise", w, 9, sampling, 2), sampling, 90, 5))
        names.append(("noise", w, 9, sampling, 90, 5, 2))
    want = [twin(*nm) for nm in names]
    files, nbytes, status = encode_batch(gpu_ctx, cases, caps=[len(f) + 5 for f in want])
    assert status == [0] * len(cases)
    for f, wf, nm in zip(files, want, names):
        assert f == wf, nm


def test_fitting_and_too_small_capacities_in_one_call(gpu_ctx):
    cases = [(E.picture("noise", 33, 47, "4:2:0", s), "4:2:0", 75, ri) for s, ri in ((1, 0), (2, 3), (3, 0), (4, 1))]
    want = [E.file_bytes(*c) for c in cases]
    sizes = [len(f) for f in want]
    files, nbytes, status = encode_batch(gpu_ctx, cases, caps=[sizes[0], sizes[1] - 1, sizes[2] + 9, 0])      # (the guard of the short ones is checked in there)
    assert status == [0, MEMORY, 0, MEMORY] and nbytes == sizes
    assert files[0] == want[0] and files[2] == want[2] and files[1] is None and files[3] is None
    assert J.encode_bound(33, 47, "4:2:0", 3) >= max(sizes)


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_round_trip_through_the_products_decode(sampling, gpu_ctx, oracle):
    pt = J.GRAY8 if sampling == "gray" else J.RGB8888
    cases = [(E.picture(kind, w, h, sampling), sampling, q, ri) for (kind, q), (w, h), ri in zip(GRID_PICTURES, ((129, 65), (40, 40), (33, 47), (17, 9)), (0, 3, 1, 0))]
    files, nbytes, status = encode_batch(gpu_ctx, cases)
    for f, case in zip(files, cases):
        orc, want, err = oracle.decode_canvas(E.file_bytes(*case), pt, 0)
        rc, got, g = J.decode_to_host(gpu_ctx, f, pt, 0)
        assert orc == 1 and rc == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_long_jobs_one_call(sampling_class, gpu_ctx, oracle):
    """E.LONG_JOBS of one pixel size with 1 x 1 jobs between them in ONE call: what each is listed for is asserted from the twin; the
    files are the twin's; the first long file of every sampling comes back through the product's decode as the oracle decodes the twin's"""
    cases, whys = E.long_batch(sampling_class)
    want = [E.long_job_twin(why[0])[0] if why else E.file_bytes(*case) for case, why in zip(cases, whys)]
    for why in whys:
        assert why is None or E.long_job_holds(*why), why
    reached = set().union(*[set(why[1]) for why in whys if why])
    assert reached == ({"starts", "in_a_dword", "shared"} if sampling_class == "gray" else {"starts", "chunk_per"})
    files, nbytes, status = encode_batch(gpu_ctx, cases, caps=[len(f) + 5 for f in want])
    assert status == [0] * len(cases)
    decoded = set()
    for f, wf, case, why in zip(files, want, cases, whys):
        assert f == wf, why or case[1:]
        if why and case[1] not in decoded:
            decoded.add(case[1])
            pt = J.GRAY8 if case[1] == "gray" else J.RGB8888
            orc, px, err = oracle.decode_canvas(wf, pt, 0)
            rc, got, g = J.decode_to_host(gpu_ctx, f, pt, 0)
            assert orc == 1 and rc == 0 and np.array_equal(got, px), why
    assert decoded == ({"gray"} if sampling_class == "gray" else set(E.SAMPLINGS) - {"gray"})


def test_named_edges_and_zero_runs(gpu_ctx):
    """the inputs tests/test_encode_cpu.py picks by what the twin's file holds (every edge of ALL_EDGES: 0xFF bytes, interval starts and the
    scan's end against the 64-byte chunks, pad bits, shared dwords) and the picture of zero runs of 15 .. 62: one call a pixel size"""
    used = edge_cases()
    assert set().union(*[hit for case, hit in used]) == ALL_EDGES
    zrl = (E.zrl_picture(), "gray", E.ZRL_QUALITY, 0)
    assert zrl_symbols(twin_layout(*zrl)[2]) == ZRL_WANT
    cases = [case for case, hit in used] + [zrl]
    for gray in (True, False):
        batch = [c for c in cases if (c[1] == "gray") == gray]
        want = [twin_layout(*c)[0] for c in batch]
        files, nbytes, status = encode_batch(gpu_ctx, batch, caps=[len(f) + 5 for f in want])
        assert status == [0] * len(batch) and files == want


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_transcode_to_host(sampling, gpu_ctx, oracle):
    jpeg = jpeg_for(FILES[sampling])
    pt = J.GRAY8 if sampling == "gray" else J.RGB8888
    vis = visible_pixels(oracle, jpeg, pt, 0)
    flat = (lambda a: a[..., 0]) if sampling == "gray" else (lambda a: a)
    for rect, size, q, ri in (((13, 21, 100, 57), None, 75, 0), (None, (84, 55), 90, 4), ((40, 30, 200, 150), (50, 64), 60, 0), (None, None, 75, 7)):
        rc, f, n = J.transcode_to_host(gpu_ctx, jpeg, size, sampling, q, ri, 0, rect)
        x, y, w, h = rect or (0, 0, 333, 217)
        px = vis[y:y + h, x:x + w] if size is None or size == (w, h) else R.resize(vis, size[0], size[1], rect)
        want = E.file_bytes(np.ascontiguousarray(flat(px)), sampling, q, ri)
        assert rc == 0 and n == len(want) and f == want, (rect, size)
    # a scale bit of the caller's: the rectangle is in the scaled image's pixels
    rc, f, n = J.transcode_to_host(gpu_ctx, jpeg, (40, 30), sampling, 75, 0, J.SCALE_HALF, (5, 6, 120, 90))
    half = visible_pixels(oracle, jpeg, pt, J.SCALE_HALF)
    assert rc == 0 and f == E.file_bytes(np.ascontiguousarray(flat(R.resize(half, 40, 30, (5, 6, 120, 90)))), sampling, 75, 0)
    # a byte short: the size it needs, nothing delivered
    rc, f, n2 = J.transcode_to_host(gpu_ctx, jpeg, (40, 30), sampling, 75, 0, J.SCALE_HALF, (5, 6, 120, 90), capacity=n - 1)
    assert rc == MEMORY and f is None and n2 == n
    # refusals, before anything is encoded
    before = encode_counts()
    wrong = "4:2:0" if sampling == "gray" else "gray"
    for kw in (dict(sampling=wrong), dict(quality=0), dict(quality=101), dict(rect=(0, 0, 334, 10)), dict(size=(0, 5)), dict(restart_interval=65536)):
        args = dict(size=(40, 30), sampling=sampling, quality=75, restart_interval=0, options=0, rect=None)
        args.update(kw)
        rc, f, n = J.transcode_to_host(gpu_ctx, jpeg, capacity=1 << 16, **args)
        assert rc == INVALID and f is None and n == 0, kw
    assert encode_counts() == before


def test_transcode_to_host_bad_mcu(gpu_ctx, oracle):
    """a stream with a bad MCU: the MCUs from the bad one on are zeros BEFORE the cut or the resize, the file is delivered all the same, and
    the verdict is JDA_DECODE_ERROR -- cut and resized, the whole image as it is, and the progressive encoder behind the same decode"""
    bad, nok = U.bad_mcu_jpeg()
    vis = visible_pixels(oracle, bad, J.RGB8888, 0, zero_from=nok)
    for rect, size in (((250, 150, 83, 67), (40, 30)), (None, None)):
        rc, f, n = J.transcode_to_host(gpu_ctx, bad, size, "4:2:0", 75, 0, 0, rect)
        px = vis if size is None else R.resize(vis, size[0], size[1], rect)
        want = E.file_bytes(np.ascontiguousarray(px), "4:2:0", 75, 0)
        assert rc == DECODE_ERROR and n == len(want) and f == want, (rect, size, rc, n)
    rc, f, n = J.transcode_to_host(gpu_ctx, bad, (40, 30), "4:2:0", 75, 0, 0, (250, 150, 83, 67), progressive=True)
    want = P.file_bytes_prog(np.ascontiguousarray(R.resize(vis, 40, 30, (250, 150, 83, 67))), "4:2:0", 75)
    assert rc == DECODE_ERROR and n == len(want) and f == want, (rc, n)


def test_thumbnails_over_a_mixed_list(gpu_ctx, oracle):
    names = ("c420_333x217", "c444_333x217", "c422_333x217", "c440_200x120", "c444_384x192_q100_rst7")
    files = [jpeg_for(nm) for nm in names]
    H, W = 48, 64
    before = encode_counts()
    out = J.thumbnails(gpu_ctx, files, (H, W), quality=80, sampling="4:2:0", prescale=False)
    after = encode_counts()
    assert after["jda_encode_blocks"] == before["jda_encode_blocks"] + 1, "one encode call for the list"
    for f, t in zip(files, out):
        px = R.resize(visible_pixels(oracle, f, J.RGB8888, 0), W, H)
        assert t == E.file_bytes(px, "4:2:0", 80, 0)
    # crops, another sampling, restart markers; prescale: the DCT-domain shortcut first
    crops = [(10, 20, 300, 150), (0, 0, 200, 120), (1, 2, 33, 47), (0, 0, 200, 120), (383, 191, 1, 1)]
    out = J.thumbnails(gpu_ctx, files, (H, W), quality=75, sampling="4:4:4", crops=crops, restart_interval=2)
    for f, t, c in zip(files, out, crops):
        assert t == E.file_bytes(R.resize(visible_pixels(oracle, f, J.RGB8888, 0), W, H, c), "4:4:4", 75, 2)
    out = J.thumbnails(gpu_ctx, files[:2], (20, 30))
    for f, t in zip(files, out):
        assert t == E.file_bytes(R.resize(visible_pixels(oracle, f, J.RGB8888, J.SCALE_EIGHTH), 30, 20), "4:2:0", 75, 0)
    g = J.thumbnails(gpu_ctx, [jpeg_for("gray_333x217")], (H, W))
    assert g[0] == E.file_bytes(R.resize(visible_pixels(oracle, jpeg_for("gray_333x217"), J.GRAY8, J.SCALE_QUARTER), W, H)[..., 0], "gray", 75, 0)
    with pytest.raises(ValueError):
        J.thumbnails(gpu_ctx, [files[0], jpeg_for("gray_333x217")], (H, W))


def test_refusals_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    surf, dst = ctx.malloc(64 * 256), ctx.malloc(4096)
    try:
        ctx.memset(dst, FILL, 4096)
        before = encode_counts()
        good = dict(src=[(surf, 256, 64, 64)], bpp=4, jobs=[(0, 0, 16, 16, "4:2:0", 75, 0)], dst=[dst], caps=[4096])

        def refused(**kw):
            a = dict(good)
            a.update(kw)
            with pytest.raises(J.JdaError) as e:
                J.encode_surfaces(ctx, a["src"], a["bpp"], a["jobs"], a["dst"], a["caps"])
            return e.value.code

        for job in ((-1, 0, 16, 16, 3, 75, 0), (0, 0, 0, 16, 3, 75, 0), (49, 0, 16, 16, 3, 75, 0), (0, 49, 16, 16, 3, 75, 0), (0, 0, 16, 16, 3, 0, 0),
                    (0, 0, 16, 16, 3, 101, 0), (0, 0, 16, 16, 4, 75, 0), (0, 0, 16, 16, 0, 75, 0), (0, 0, 16, 16, 3, 75, 65536), (0, 0, 16, 16, 3, 75, -1)):
            assert refused(jobs=[job]) == INVALID, job
        assert refused(bpp=1) == INVALID and refused(bpp=2) == INVALID            # a colour sampling of a gray surface; no such pixel size
        assert refused(src=[(surf + 2, 256, 63, 64)]) == INVALID and refused(src=[(surf, 254, 63, 64)]) == INVALID and refused(src=[(surf, 252, 64, 64)]) == INVALID
        assert refused(dst=[surf + 5 * 256 + 8], caps=[8]) == INVALID              # a file over its own source rectangle
        assert refused(caps=[-1]) == INVALID
        two = dict(src=good["src"] * 2, jobs=good["jobs"] * 2)
        assert refused(dst=[dst, dst + 99], caps=[100, 100], **two) == INVALID     # two files that share a byte
        assert encode_counts() == before, "a refused call launches nothing"
        assert np.all(ctx.to_host(dst, 4096) == FILL)
        assert J.encode_surfaces(ctx, [], 4, [], [], []) == ([], [])               # n == 0: nothing to do, nothing launched
        assert encode_counts() == before
    finally:
        ctx.free(surf)
        ctx.free(dst)


def test_every_encode_kernel_is_counted(gpu_ctx):
    img = E.picture("smooth", 17, 9, "4:2:2")
    files, nbytes, status = encode_batch(gpu_ctx, [(img, "4:2:2", 75, 0)])
    assert files[0] == E.file_bytes(img, "4:2:2", 75, 0)
    counts = encode_counts()
    assert all(counts[k] > 0 for k in KERNELS), counts
    assert not [k for k in J.kernel_launch_counts() if "jda_encode" in k and not any(name in k for name in KERNELS)]


def test_measuring_hook_times_every_stage_of_the_same_call(gpu_ctx):
    """jda_internal_encode_time (tools/encode_bench.py): the call with each of its seven launches between two events -- the same files"""
    import ctypes as C
    from jpegdec_amd.binding import EncodeJob, Output
    ctx = gpu_ctx
    imgs = [E.picture("noise", 129, 65, "4:2:0", 7), E.picture("smooth", 40, 40, "4:2:0")]
    want = [E.file_bytes(im, "4:2:0", 75, 3) for im in imgs]
    src, dst = ctx.malloc(2 * 129 * 65 * 4), ctx.malloc(2 * 8192)
    try:
        for k, im in enumerate(imgs):
            ctx.from_host(src + k * 129 * 65 * 4, im.reshape(-1))
        o = (Output * 2)(*[Output(src + k * 129 * 65 * 4, im.shape[1] * 4, im.shape[1], im.shape[0]) for k, im in enumerate(imgs)])
        j = (EncodeJob * 2)(*[EncodeJob(0, 0, im.shape[1], im.shape[0], J.ENCODE_420, 75, 3, 0) for im in imgs])
        d, c = (C.c_void_p * 2)(dst, dst + 8192), (C.c_int64 * 2)(8192, 8192)
        nb, st, ms = (C.c_int64 * 2)(), (C.c_int32 * 2)(), (C.c_float * 7)()
        fn = ctx.lib.jda_internal_encode_time
        fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(EncodeJob), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                       C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        before = encode_counts()
        assert fn(ctx.handle, 2, o, 4, j, d, c, nb, st, ms) == 0
        after = encode_counts()
        assert {k: after[k] - before[k] for k in KERNELS} == dict(zip(KERNELS, (1, 1, 2, 1, 1, 1)))
        assert list(st) == [0, 0] and all(t > 0 for t in ms)
        assert [ctx.to_host(dst + k * 8192, nb[k]).tobytes() for k in range(2)] == want
        assert fn(ctx.handle, 2, o, 4, j, d, c, nb, st, None) == INVALID
    finally:
        ctx.free(src)
        ctx.free(dst)
