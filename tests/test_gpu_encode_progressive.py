"""jda_encode_surfaces_progressive on the GPU (and jda_transcode_to_host_progressive, thumbnails(progressive=True)) against the Python twin
(tests/encode_prog_util.py; tests/test_encode_prog_cpu.py holds the twin to Pillow's progressive=True): (a) the whole grid, every edge of
encode_prog_util.edge_cases and -- gray -- the flat 1456 x 1456 picture in ONE call per pixel size, the files back to back in a guard-filled
allocation, eleven launches, twice; (b) capacities a byte short; (c) Pillow opens the files and this library decodes them
(JDA_PROGRESSIVE_FULL) to the pixels of the baseline file of the same coefficients; (d) the one-call transcode and thumbnails, and the calls
without the keyword; (e) the refusals.  All bit-exact."""
import io

import numpy as np
import pytest

import jpegdec_amd as J
from tests import coef_jpeg
from tests import encode_util as E
from tests import encode_prog_util as P
from tests import prog_cases as PC
from tests import resize_util as R
from tests.cases import jpeg_for
from tests.test_gpu_resize import visible_pixels

pytestmark = pytest.mark.gpu

FILL = 0x5A
INVALID, UNSUPPORTED, MEMORY = 1, 3, 5
# the eleven launches of a call, in the order the kernels first run
KERNELS = ("jda_encode_blocks", "jda_encode_lengths", "jda_progenc_classify", "jda_progenc_resolve", "jda_progenc_gather", "jda_progenc_lengths", "jda_progenc_scan",
           "jda_progenc_emit", "jda_progenc_count", "jda_progenc_write")
LAUNCHES = (1, 1, 1, 1, 1, 1, 2, 1, 1, 1)
BASELINE_ONLY = ("jda_encode_scan", "jda_encode_emit", "jda_encode_count", "jda_encode_write", "jda_huffopt_gather", "jda_huffopt_lengths")


def counts(names=KERNELS + BASELINE_ONLY):
    c = J.kernel_launch_counts()
    return {k: sum(v for name, v in c.items() if k in name) for k in names}


def delta(before, after, names):
    return {k: after[k] - before[k] for k in names}


def encode_batch(ctx, cases, caps=None):
    """cases: [(img, sampling, q)] of one pixel size.  Rectangle i at (3 + i % 3, 2 + i % 2) of a FILL-filled surface, the files back to back
    (capacity: the twin's size unless given).  -> (files or None, sizes, statuses); the guard behind every file and the call's launch counts
    are checked."""
    n = len(cases)
    bpp = 1 if cases[0][1] == "gray" else 4
    srcs, jobs, blobs, soff = [], [], [], 0
    for i, (img, sampling, q) in enumerate(cases):
        h, w = img.shape[:2]
        x, y = 3 + i % 3, 2 + i % 2
        pitch = ((w + 8) * bpp + 3) & ~3
        s = np.full((h + 5, pitch), FILL, dtype=np.uint8)
        s[y:y + h, x * bpp:(x + w) * bpp] = img.reshape(h, w * bpp)
        blobs.append(s)
        srcs.append((soff, pitch, w + 8, h + 5))
        jobs.append((x, y, w, h, sampling, q, 0))
        soff += (s.size + 15) & ~15
    if caps is None:
        caps = [len(P.file_bytes_prog(*c)) for c in cases]
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    total = int(offs[-1]) + 16
    dsrc, ddst = ctx.malloc(soff), ctx.malloc(total)
    try:
        for s, (o, _, _, _) in zip(blobs, srcs):
            ctx.from_host(dsrc + o, s.reshape(-1))
        ctx.memset(ddst, FILL, total)
        before = counts()
        nbytes, status = J.encode_surfaces_progressive(ctx, [(dsrc + o, p, w, h) for o, p, w, h in srcs], bpp, jobs, [ddst + int(o) for o in offs[:-1]], caps)
        after = counts()
        assert delta(before, after, KERNELS) == dict(zip(KERNELS, LAUNCHES)), "eleven launches a call"
        assert not any(delta(before, after, BASELINE_ONLY).values())
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


def batch(sampling_class):
    return P.batch(sampling_class) + ([(E.picture(*P.FLAT_LIMIT[:4]), "gray", P.FLAT_LIMIT[4])] if sampling_class == "gray" else [])


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_grid_and_edges_one_call(sampling_class, gpu_ctx):
    cases = batch(sampling_class)
    want = [P.file_bytes_prog(*c) for c in cases]
    files, nbytes, status = encode_batch(gpu_ctx, cases)
    assert status == [0] * len(cases)
    for f, wf, c in zip(files, want, cases):
        assert f == wf, (c[0].shape, c[1:])
    again, _, _ = encode_batch(gpu_ctx, cases)                  # the same call once more: the same bytes, whatever the pool hands out
    assert again == files


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_a_capacity_one_byte_short(sampling_class, gpu_ctx):
    cases = P.edge_cases(sampling_class)[:7]
    want = [P.file_bytes_prog(*c) for c in cases]
    caps = [len(f) - (1 if i in (1, 3, 6) else 0) for i, f in enumerate(want)]
    files, nbytes, status = encode_batch(gpu_ctx, cases, caps)
    assert nbytes == [len(f) for f in want]                     # the size it needs is reported
    assert status == [MEMORY if i in (1, 3, 6) else 0 for i in range(len(cases))]
    for i, (f, wf) in enumerate(zip(files, want)):              # (encode_batch: no byte of a refused file is written, the neighbours' guards hold)
        assert f == (None if i in (1, 3, 6) else wf)
    for img, s, q in cases:
        assert J.encode_bound_progressive(img.shape[1], img.shape[0], s) >= len(P.file_bytes_prog(img, s, q))


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_round_trip(sampling, gpu_ctx):
    from PIL import Image
    cases = [(E.picture(kind, w, h, sampling, 3), sampling, q) for (w, h), kind, q in (((129, 65), "noise", 75), ((33, 47), "smooth", 90), ((40, 40), "noise", 100))]
    files, _, status = encode_batch(gpu_ctx, cases)
    assert status == [0] * len(cases)
    pt = J.GRAY8 if sampling == "gray" else J.RGB8888
    for f, (img, s, q) in zip(files, cases):
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (img.shape[1], img.shape[0]) and im.info.get("progressive") == 1
        # the baseline file of the same coefficients, under tables with which the baseline reader has no truncation event
        base, events = PC.reencode_coefs(coef_jpeg.decode_coefs(E.file_bytes(img, s, q)))
        assert events == 0 and all(np.array_equal(a, b) for a, b in zip(coef_jpeg.decode_coefs(base)["coefs"], E.coefficients(img, s, q)))
        rc1, got, g1 = J.decode_to_host(gpu_ctx, f, pt, J.PROGRESSIVE_FULL)
        rc2, ref, g2 = J.decode_to_host(gpu_ctx, base, pt, 0)
        assert rc1 == 0 and rc2 == 0 and g1["out_w"] == g2["out_w"] and g1["out_h"] == g2["out_h"]
        w, h, bpp = g1["out_w"], g1["out_h"], g1["bpp"]
        assert np.array_equal(np.asarray(got)[:h, :w * bpp], np.asarray(ref)[:h, :w * bpp]), (s, img.shape)
        assert np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(base))))


def test_transcode_to_host_progressive(gpu_ctx, oracle):
    jpeg = jpeg_for("c420_333x217")
    vis = visible_pixels(oracle, jpeg, J.RGB8888, 0)
    for rect, size, q in ((None, None, 75), ((13, 21, 100, 57), None, 75), (None, (84, 55), 90)):
        x, y, w, h = rect or (0, 0, 333, 217)
        px = np.ascontiguousarray(vis[y:y + h, x:x + w] if size is None else R.resize(vis, size[0], size[1], rect))
        before = counts()
        rc, f, n = J.transcode_to_host(gpu_ctx, jpeg, size, "4:2:0", q, 0, 0, rect, progressive=True)
        after = counts()
        want = P.file_bytes_prog(px, "4:2:0", q)
        assert rc == 0 and n == len(want) and f == want, (rect, size)
        assert delta(before, after, KERNELS) == dict(zip(KERNELS, LAUNCHES)) and not any(delta(before, after, BASELINE_ONLY).values())
        rc, g, _ = J.transcode_to_host(gpu_ctx, jpeg, size, "4:2:0", q, 0, 0, rect, progressive=True, optimize=True)
        assert rc == 0 and g == want                            # optimize changes nothing in a progressive file
        before = counts()
        rc, g, _ = J.transcode_to_host(gpu_ctx, jpeg, size, "4:2:0", q, 0, 0, rect)
        assert rc == 0 and g == E.file_bytes(px, "4:2:0", q, 0)
        assert not any(delta(before, counts(), KERNELS[2:]).values())      # without the keyword: the baseline file, none of the new kernels
    rc, f, n = J.transcode_to_host(gpu_ctx, jpeg, None, "4:2:0", 75, 0, 0, None, capacity=1000, progressive=True)
    assert rc == MEMORY and f is None and n == len(P.file_bytes_prog(np.ascontiguousarray(vis), "4:2:0", 75))
    rc, f, n = J.transcode_to_host(gpu_ctx, jpeg, None, "4:2:0", 75, 4, 0, None, capacity=100000, progressive=True)
    assert rc == INVALID and n == 0
    gray = jpeg_for("gray_333x217")
    px = np.ascontiguousarray(R.resize(visible_pixels(oracle, gray, J.GRAY8, 0), 40, 30)[..., 0])
    rc, f, n = J.transcode_to_host(gpu_ctx, gray, (40, 30), "gray", 60, 0, progressive=True)
    assert rc == 0 and f == P.file_bytes_prog(px, "gray", 60)


def test_thumbnails_progressive(gpu_ctx, oracle):
    names = ("c420_333x217", "c444_333x217", "c422_333x217")
    files = [jpeg_for(nm) for nm in names]
    H, W = 48, 64
    before = counts()
    out = J.thumbnails(gpu_ctx, files, (H, W), quality=80, sampling="4:2:0", prescale=False, progressive=True)
    after = counts()
    assert delta(before, after, KERNELS) == dict(zip(KERNELS, LAUNCHES)), "one encode call for the list"
    both = J.thumbnails(gpu_ctx, files, (H, W), quality=80, sampling="4:2:0", prescale=False, progressive=True, optimize=True)
    before = counts()
    plain = J.thumbnails(gpu_ctx, files, (H, W), quality=80, sampling="4:2:0", prescale=False)
    assert not any(delta(before, counts(), KERNELS[2:]).values())
    for f, t, b, p in zip(files, out, both, plain):
        px = R.resize(visible_pixels(oracle, f, J.RGB8888, 0), W, H)
        assert t == P.file_bytes_prog(px, "4:2:0", 80) and b == t and p == E.file_bytes(px, "4:2:0", 80, 0)
    with pytest.raises(J.JdaError) as e:
        J.thumbnails(gpu_ctx, files, (H, W), quality=80, prescale=False, progressive=True, restart_interval=2)
    assert e.value.code == INVALID


def test_refusals_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    surf, dst = ctx.malloc(64 * 256), ctx.malloc(4096)
    try:
        ctx.memset(dst, FILL, 4096)
        before = counts()

        def refused(code, src=None, bpp=4, job=(0, 0, 16, 16, "4:2:0", 75, 0), d=None, cap=4096):
            with pytest.raises(J.JdaError) as e:
                J.encode_surfaces_progressive(ctx, [src or (surf, 256, 64, 64)], bpp, [job], [dst if d is None else d], [cap])
            assert e.value.code == code, job
        for ri in (1, 8, 65535):
            refused(INVALID, job=(0, 0, 16, 16, "4:2:0", 75, ri))                        # restart intervals are out of scope
        refused(INVALID, job=(0, 0, 16, 16, "gray", 75, 0))                              # a colour surface takes no gray sampling
        refused(INVALID, bpp=1, src=(surf, 256, 256, 64))
        refused(INVALID, job=(0, 0, 16, 16, "4:2:0", 0, 0))
        refused(INVALID, job=(0, 0, 16, 16, "4:2:0", 101, 0))
        refused(INVALID, job=(60, 0, 16, 16, "4:2:0", 75, 0))
        refused(INVALID, job=(0, 0, 0, 16, "4:2:0", 75, 0))
        refused(INVALID, job=(0, 0, 16, 16, 4, 75, 0))
        refused(INVALID, bpp=2)
        refused(INVALID, d=surf + 64, cap=64)                                            # a file over its own source
        refused(INVALID, cap=-1)
        assert counts() == before and np.all(ctx.to_host(dst, 4096) == FILL)
        assert J.encode_surfaces_progressive(ctx, [], 4, [], [], []) == ([], [])           # n == 0: nothing to do, nothing launched
        assert counts() == before
        with pytest.raises(J.JdaError):
            J.encode_bound_progressive(0, 8, "gray")
    finally:
        ctx.free(surf)
        ctx.free(dst)
