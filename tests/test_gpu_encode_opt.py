"""JDA_ENCODE_OPTIMIZE on the GPU (jda_encode_surfaces_ex, jda_transcode_to_host_ex, thumbnails(optimize=True)), against the Python twin
(tests/encode_opt_util.py; tests/test_encode_opt_cpu.py holds the twin to Pillow's optimize=True): (a) the whole grid and every edge of
encode_opt_util.edge_cases in ONE mixed-flag call per pixel size, the files back to back in a guard-filled allocation, nine launches; with
every flag zero the two new kernels are not launched; (b) a capacity between the optimised and the standard size; (c) the one-call
transcode; (d) thumbnails; (e) the same call twice.  All bit-exact."""
import io

import numpy as np
import pytest

import jpegdec_amd as J
from tests import encode_util as E
from tests import encode_opt_util as O
from tests import resize_util as R
from tests.cases import jpeg_for
from tests.test_gpu_resize import visible_pixels

pytestmark = pytest.mark.gpu

FILL = 0x5A
INVALID, UNSUPPORTED, MEMORY = 1, 3, 5
# in the order they first run in a call with an optimised job, and their launches in such a call
KERNELS = ("jda_encode_blocks", "jda_encode_lengths", "jda_huffopt_gather", "jda_huffopt_lengths", "jda_encode_scan", "jda_encode_emit", "jda_encode_count",
           "jda_encode_write")
LAUNCHES_OPT = (1, 1, 1, 1, 2, 1, 1, 1)
LAUNCHES_STD = (1, 1, 0, 0, 2, 1, 1, 1)


def counts():
    c = J.kernel_launch_counts()
    return {k: sum(v for name, v in c.items() if k in name) for k in KERNELS}


def encode_batch(ctx, cases, caps=None, slack=5, flags="own"):
    """cases: [(img, sampling, q, ri, flag)] of one pixel size.  Rectangle i at (3 + i % 3, 2 + i % 2) of a FILL-filled surface, the files back
    to back (capacity: the twin's size + slack unless given).  flags: "own" (every case's), None (jda_encode_surfaces) or a list.
    -> (files or None, sizes, statuses); the guard behind every file and the call's launch counts are checked."""
    n = len(cases)
    bpp = 1 if cases[0][1] == "gray" else 4
    srcs, jobs, blobs, soff = [], [], [], 0
    for i, (img, sampling, q, ri, flag) in enumerate(cases):
        h, w = img.shape[:2]
        x, y = 3 + i % 3, 2 + i % 2
        pitch = ((w + 8) * bpp + 3) & ~3
        s = np.full((h + 5, pitch), FILL, dtype=np.uint8)
        s[y:y + h, x * bpp:(x + w) * bpp] = img.reshape(h, w * bpp)
        blobs.append(s)
        srcs.append((soff, pitch, w + 8, h + 5))
        jobs.append((x, y, w, h, sampling, q, ri))
        soff += (s.size + 15) & ~15
    if flags == "own":
        flags = [c[4] for c in cases]
    if caps is None:
        caps = [len(O.twin(*c[:4], f)[0]) + slack for c, f in zip(cases, flags or [0] * n)]
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    total = int(offs[-1]) + 16
    dsrc, ddst = ctx.malloc(soff), ctx.malloc(total)
    try:
        for s, (o, _, _, _) in zip(blobs, srcs):
            ctx.from_host(dsrc + o, s.reshape(-1))
        ctx.memset(ddst, FILL, total)
        before = counts()
        nbytes, status = J.encode_surfaces(ctx, [(dsrc + o, p, w, h) for o, p, w, h in srcs], bpp, jobs, [ddst + int(o) for o in offs[:-1]], caps, flags)
        after = counts()
        want = LAUNCHES_OPT if flags and any(flags) else LAUNCHES_STD
        assert {k: after[k] - before[k] for k in KERNELS} == dict(zip(KERNELS, want)), "a fixed number of launches a call"
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


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_grid_and_edges_one_mixed_call(sampling_class, gpu_ctx):
    cases = O.batch(sampling_class)
    assert {c[4] for c in cases} == {0, 1}
    want = [O.twin(*c)[0] for c in cases]
    files, nbytes, status = encode_batch(gpu_ctx, cases, caps=[len(f) + 5 for f in want])
    assert status == [0] * len(cases)
    for f, wf, c in zip(files, want, cases):
        assert f == wf, (c[0].shape, c[1:])
    # the same call once more: the same bytes (the histograms are zeroed by the call, whatever the pool hands out)
    again, _, _ = encode_batch(gpu_ctx, cases, caps=[len(f) + 5 for f in want])
    assert again == files


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_all_flags_zero_launches_no_new_kernel(sampling_class, gpu_ctx):
    cases = [c[:4] + (0,) for c in O.edge_cases(sampling_class)]
    want = [E.file_bytes(*c[:4]) for c in cases]
    for flags in ([0] * len(cases), None):            # (encode_batch holds the launch counts to 1, 1, 0, 0, 2, 1, 1, 1)
        files, nbytes, status = encode_batch(gpu_ctx, cases, caps=[len(f) + 5 for f in want], flags=flags)
        assert status == [0] * len(cases) and files == want


def test_capacity_between_the_optimised_and_the_standard_size(gpu_ctx):
    cases = [(E.picture("noise", 33, 47, "4:2:0", s), "4:2:0", 75, ri, 1) for s, ri in ((1, 0), (2, 3), (3, 1))]
    std = [len(E.file_bytes(*c[:4])) for c in cases]
    want = [O.twin(*c)[0] for c in cases]
    opt = [len(f) for f in want]
    assert all(o < s - 1 for o, s in zip(opt, std))                                   # picked from the twin: the optimised file is the smaller
    files, nbytes, status = encode_batch(gpu_ctx, cases, caps=[std[0] - 1, opt[1] - 1, opt[2]])
    assert status == [0, MEMORY, 0] and nbytes == opt
    assert files[0] == want[0] and files[1] is None and files[2] == want[2]
    assert J.encode_bound(33, 47, "4:2:0", 3) >= max(std)


def test_refusals_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    surf, dst = ctx.malloc(64 * 256), ctx.malloc(4096)
    try:
        ctx.memset(dst, FILL, 4096)
        before = counts()
        args = ([(surf, 256, 64, 64)], 4, [(0, 0, 16, 16, "4:2:0", 75, 0)], [dst], [4096])
        for bad in (2, 3, 0x80000000, 0xFFFFFFFF):
            with pytest.raises(J.JdaError) as e:
                J.encode_surfaces(ctx, *args, [bad])
            assert e.value.code == INVALID
        assert counts() == before and np.all(ctx.to_host(dst, 4096) == FILL)
        assert J.encode_surfaces(ctx, [], 4, [], [], [], []) == ([], [])              # n == 0 with flags: nothing to do, nothing launched
        assert counts() == before
    finally:
        ctx.free(surf)
        ctx.free(dst)


def test_transcode_to_host_optimised(gpu_ctx, oracle):
    jpeg = jpeg_for("c420_333x217")
    vis = visible_pixels(oracle, jpeg, J.RGB8888, 0)
    for rect, size, q, ri in (((13, 21, 100, 57), None, 75, 0), (None, (84, 55), 90, 4)):
        x, y, w, h = rect or (0, 0, 333, 217)
        px = np.ascontiguousarray(vis[y:y + h, x:x + w] if size is None else R.resize(vis, size[0], size[1], rect))
        before = counts()
        rc, f, n = J.transcode_to_host(gpu_ctx, jpeg, size, "4:2:0", q, ri, 0, rect, optimize=True)
        after = counts()
        want = O.file_bytes_opt(px, "4:2:0", q, ri)
        assert rc == 0 and n == len(want) and f == want, (rect, size)
        assert {k: after[k] - before[k] for k in KERNELS} == dict(zip(KERNELS, LAUNCHES_OPT))
        rc, g, n2 = J.transcode_to_host(gpu_ctx, jpeg, size, "4:2:0", q, ri, 0, rect)
        assert rc == 0 and g == E.file_bytes(px, "4:2:0", q, ri) and n2 > n
    gray = jpeg_for("gray_333x217")
    px = np.ascontiguousarray(R.resize(visible_pixels(oracle, gray, J.GRAY8, 0), 40, 30)[..., 0])
    rc, f, n = J.transcode_to_host(gpu_ctx, gray, (40, 30), "gray", 60, 0, optimize=True)
    assert rc == 0 and f == O.file_bytes_opt(px, "gray", 60, 0)


def test_thumbnails_optimised(gpu_ctx, oracle):
    from PIL import Image
    names = ("c420_333x217", "c444_333x217", "c422_333x217")
    files = [jpeg_for(nm) for nm in names]
    H, W = 48, 64
    before = counts()
    out = J.thumbnails(gpu_ctx, files, (H, W), quality=80, sampling="4:2:0", prescale=False, optimize=True)
    after = counts()
    assert {k: after[k] - before[k] for k in KERNELS} == dict(zip(KERNELS, LAUNCHES_OPT)), "one encode call for the list"
    plain = J.thumbnails(gpu_ctx, files, (H, W), quality=80, sampling="4:2:0", prescale=False)
    for f, t, p in zip(files, out, plain):
        px = R.resize(visible_pixels(oracle, f, J.RGB8888, 0), W, H)
        assert t == O.file_bytes_opt(px, "4:2:0", 80, 0) and p == E.file_bytes(px, "4:2:0", 80, 0) and len(t) < len(p)
        a, b = Image.open(io.BytesIO(t)), Image.open(io.BytesIO(p))
        a.load(); b.load()
        assert a.size == (W, H) and np.array_equal(np.asarray(a), np.asarray(b))      # Pillow opens it: the same pixels as the standard file's
