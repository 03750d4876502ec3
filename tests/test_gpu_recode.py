"""The lossless recode on the GPU (jda_recode_images, jda_recode_to_host, recode()), against Pillow's files and the suite's own
decoders (tests/recode_util.py; tests/test_recode_cpu.py steps the same stages lane by lane):
(a) ONE call per target form over Pillow's four files of every shape -- one-MCU images of the four layouts, the 333 x 217 shapes, 136 x 88 at
    4:2:0 (324 blocks: a workgroup straddles two jobs) -- and the written edge files, sources with a host index, with a device index and dense
    coefficient images side by side, the files back to back in a guard-filled allocation, a fixed number of launches, twice;
(b) restart intervals to their own, to none and to another; (c) a capacity a byte short; (d) jda_recode_to_host and recode();
(e) the pixels of a recoded file are the source's; (f) a fixture with truncation events gives T.81's coefficients; (g) the refusals."""
import numpy as np
import pytest

import jpegdec_amd as J
from tests import recode_util as U
from tests.cases import jpeg_for

pytestmark = pytest.mark.gpu

FILL = 0x5A
# the kernels of a call and their launches per target form, with sources of both kinds in the call
KERNELS = ("jda_rc_extract", "jda_rc_from_coef", "jda_encode_blocks", "jda_encode_lengths", "jda_huffopt_gather", "jda_huffopt_lengths", "jda_encode_scan", "jda_encode_emit",
           "jda_encode_count", "jda_encode_write", "jda_progenc_classify", "jda_progenc_resolve", "jda_progenc_gather", "jda_progenc_lengths", "jda_progenc_scan",
           "jda_progenc_emit", "jda_progenc_count", "jda_progenc_write")
LAUNCHES = {"baseline": (1, 1, 0, 1, 0, 0, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0),
            "optimize": (1, 1, 0, 1, 1, 1, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0),
            "progressive": (1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 1, 1, 1)}


def counts():
    c = J.kernel_launch_counts()
    return {k: sum(v for name, v in c.items() if k in name) for k in KERNELS}


class Sources:
    """resident sources of files: a baseline file with the host pre-scan's index ("host") or the device pre-scan's ("device"), a progressive
    file as a dense ("dense") or sparse ("sparse") coefficient image"""
    def __init__(self, ctx, files, kinds=None):
        self.ctx, self.items, self.keep = ctx, [], []
        for i, f in enumerate(files):
            prog = U.frame_header(f)[1] == 0xC2
            kind = (kinds[i] if kinds else None) or ("dense" if prog else ("host", "device")[i & 1])
            if prog:
                ci = J.CoefImage(f)
                self.keep.append(ci)
                self.items.append(J.DeviceCoef(ctx, ci, J.COEF_SPARSE if kind == "sparse" else J.COEF_DENSE))
            else:
                p = J.PreparedImage(f, device_prescan=(kind == "device"))
                self.keep.append(p)
                d = J.DeviceImage(ctx, p)
                assert kind == "device" or not d.prescan_on_device
                self.items.append(d)

    def close(self):
        for d in self.items:
            d.close()
        for p in self.keep:
            p.close()


def recode_batch(ctx, files, forms, ris, kinds=None, caps=None, expect_launches=True):
    """-> (files or None, sizes, statuses): the guard behind every file, around a file that is not written, and the call's launches are checked"""
    n = len(files)
    src = Sources(ctx, files, kinds)
    try:
        if caps is None:
            caps = []
            for d, f, r in zip(src.items, forms, ris):
                try:
                    caps.append(J.recode_bound(d.info, f, r))
                except J.JdaError:                       # (a source the call refuses has no bound: room that must stay untouched)
                    caps.append(4096)
        offs = np.concatenate([[0], np.cumsum([(c + 15) & ~15 for c in caps])]).astype(np.int64)
        total = int(offs[-1]) + 16
        ddst = ctx.malloc(total)
        try:
            ctx.memset(ddst, FILL, total)
            before = counts()
            nbytes, status = J.recode_images(ctx, src.items, list(zip(forms, ris)), [ddst + int(o) for o in offs[:-1]], caps)
            after = counts()
            if expect_launches:
                want = list(LAUNCHES[forms[0]])
                ran = [isinstance(d, J.DeviceImage) for d, st in zip(src.items, status) if st in (0, U.ERROR_MEMORY)]
                want[0], want[1] = int(any(ran)), int(any(not r for r in ran))
                assert {k: after[k] - before[k] for k in KERNELS} == dict(zip(KERNELS, want)), "a fixed number of launches a call"
            got = ctx.to_host(ddst, total)
        finally:
            ctx.free(ddst)
    finally:
        src.close()
    out = []
    for i in range(n):
        o, e = int(offs[i]), int(offs[i + 1])
        if status[i] == 0:
            out.append(got[o:o + nbytes[i]].tobytes())
            assert np.all(got[o + nbytes[i]:e] == FILL), i
        else:
            out.append(None)
            assert np.all(got[o:e] == FILL), i
    assert np.all(got[int(offs[-1]):] == FILL)
    return out, nbytes, status


@pytest.mark.parametrize("form", U.FORMS)
def test_one_call_over_every_source_gives_pillows_files(gpu_ctx, form):
    """Pillow's four files of every colour shape and the written edge files in one call: host-index, device-index and coefficient sources side
    by side; Pillow's file of the form from each of Pillow's, the source's coefficients and quantisers from each written one; twice"""
    pytest.importorskip("PIL")
    jobs = U.pillow_jobs(True)
    names = [k for k in sorted(U.written_specs()) if not k.endswith("gray")]
    files = [j[0] for j in jobs] + [U.written(k) for k in names] + [U.written_progressive()]
    forms = [form] * len(files)
    got, nbytes, status = recode_batch(gpu_ctx, files, forms, [None if form == "progressive" else 0] * len(files))
    assert status == [0] * len(files)
    for (src, pil), f in zip(jobs, got):
        U.is_pillow(f, U.want_of(pil, form, 0), form, source=src)
    for src, f in zip(files[len(jobs):], got[len(jobs):]):
        U.same_coefficients(src, f)
    again, nb2, st2 = recode_batch(gpu_ctx, files, forms, [None if form == "progressive" else 0] * len(files))
    assert again == got and nb2 == nbytes, "the same call once more: the same bytes, whatever the pool hands out"


@pytest.mark.parametrize("form", U.FORMS)
def test_gray_call(gpu_ctx, form):
    pytest.importorskip("PIL")
    jobs = U.pillow_jobs(False)
    files = [j[0] for j in jobs] + [U.written("huff_custom_gray"), U.written("quant16_gray")]
    got, nbytes, status = recode_batch(gpu_ctx, files, [form] * len(files), [None if form == "progressive" else 0] * len(files))
    assert status == [0] * len(files)
    for (src, pil), f in zip(jobs, got):
        U.is_pillow(f, U.want_of(pil, form, 0), form, source=src)
    for src, f in zip(files[len(jobs):], got[len(jobs):]):
        U.same_coefficients(src, f)


def test_host_index_and_device_index_give_the_same_file(gpu_ctx):
    files = [jpeg_for(n) for n in ("c420_1280x720", "c420_640x368_rstrow", "c444_384x192_q100_rst7", "gray_333x217")]
    src = Sources(gpu_ctx, files, ["device"] * 4)
    on_device = [d.prescan_on_device for d in src.items]
    src.close()
    assert on_device == [True] * 4, "the device pre-scan made these indexes"
    for form in ("baseline", "optimize"):
        a, _, sa = recode_batch(gpu_ctx, files, [form] * 4, [None] * 4, kinds=["host"] * 4)
        b, _, sb = recode_batch(gpu_ctx, files, [form] * 4, [None] * 4, kinds=["device"] * 4)
        assert sa == [0] * 4 and sb == [0] * 4 and a == b
    U.same_coefficients(files[3], a[3])


def test_restart_intervals(gpu_ctx):
    files, ris = [], []
    for f, mcus, cx in U.restart_sources():
        for t in U.RESTART_TARGETS:
            files.append(f)
            ris.append(t)
    for form in ("baseline", "optimize"):
        got, nbytes, status = recode_batch(gpu_ctx, files, [form] * len(files), ris)
        assert status == [0] * len(files)
        for src, t, f in zip(files, ris, got):
            U.same_coefficients(src, f)
            assert U.decode_any(f)["restart_interval"] == (U.decode_any(src)["restart_interval"] if t is None else t)
    pytest.importorskip("PIL")
    jobs = U.pillow_jobs(True, sources=("baseline", "optimize", "progressive"))
    got, nbytes, status = recode_batch(gpu_ctx, [j[0] for j in jobs], ["baseline"] * len(jobs), [U.PILLOW_RESTART] * len(jobs))
    assert status == [0] * len(jobs)
    for (src, pil), f in zip(jobs, got):
        U.is_pillow(f, pil["restart"], "baseline", source=src)


@pytest.mark.parametrize("form", U.FORMS)
def test_capacity_a_byte_short(gpu_ctx, form):
    files = [U.written("three_quantisers"), U.written("quant16"), U.written_progressive()]
    ris = [None if form == "progressive" else 0] * 3
    got, nbytes, status = recode_batch(gpu_ctx, files, [form] * 3, ris)
    assert status == [0] * 3
    short, nb2, st2 = recode_batch(gpu_ctx, files, [form] * 3, ris, caps=[nbytes[0], nbytes[1] - 1, nbytes[2]])
    assert st2 == [0, U.ERROR_MEMORY, 0] and nb2 == nbytes, "the size it needs, and no byte of it"
    assert short[0] == got[0] and short[2] == got[2]


def test_recode_to_host_and_recode(gpu_ctx):
    pytest.importorskip("PIL")
    pil = U.pillow_files("noise", 136, 88, "4:2:0")
    for src in ("baseline", "progressive", "restart"):
        for form in U.FORMS:
            rc, f, n = J.recode_to_host(gpu_ctx, pil[src], form, 0 if form != "progressive" else None)
            assert rc == 0 and n == len(f)
            U.is_pillow(f, U.want_of(pil, form, 0), form, source=pil[src])
    rc, f, n = J.recode_to_host(gpu_ctx, pil["restart"], "baseline")                       # the source's own interval
    assert rc == 0
    U.is_pillow(f, pil["restart"], "baseline")
    rc, f, n = J.recode_to_host(gpu_ctx, pil["baseline"], "optimize", capacity=len(pil["optimize"]) - 1)
    assert rc == U.ERROR_MEMORY and f is None and n == len(U.want_of(pil, "optimize", 0))
    assert J.recode_to_host(gpu_ctx, pil["baseline"], "progressive", 4)[0] == U.INVALID_PARAMETER
    assert J.recode_to_host(gpu_ctx, U.refused()["c440"][0], "optimize")[0] == U.UNSUPPORTED
    shapes = [s for s in U.PILLOW_SHAPES if s[1] >= 16 and s[3] != "gray"]      # (a progressive call takes gray or colour, not both)
    files = [U.pillow_files(*s)["baseline"] for s in shapes]
    before = counts()
    out = J.recode(gpu_ctx, files, "optimize")
    after = counts()
    assert after["jda_rc_extract"] - before["jda_rc_extract"] == 1 and after["jda_rc_from_coef"] == before["jda_rc_from_coef"], "one recode_images call"
    for s, f in zip(shapes, out):
        U.is_pillow(f, U.pillow_files(*s)["optimize"], "optimize")
    assert [len(f) for f in J.recode(gpu_ctx, files, "progressive")] == [len(U.pillow_files(*s)["progressive"]) for s in shapes]


def test_pixels_of_a_recoded_file_are_the_sources(gpu_ctx):
    """decode_to_host of a truncation-free source and of its recoded files: identical pixels (a progressive file through JDA_PROGRESSIVE_FULL)"""
    pytest.importorskip("PIL")
    for shape in (("smooth", 333, 217, "4:4:4"), ("noise", 136, 88, "4:2:0")):
        src = U.pillow_files(*shape)["baseline"]
        assert J.PreparedImage(src).truncation_events() == 0
        rc, want, g = J.decode_to_host(gpu_ctx, src, J.RGB8888, 0)
        assert rc == 0
        for form in U.FORMS:
            rc, f, n = J.recode_to_host(gpu_ctx, src, form, None)
            assert rc == 0
            if form != "progressive":
                assert J.PreparedImage(f).truncation_events() == 0
            rc, got, g2 = J.decode_to_host(gpu_ctx, f, J.RGB8888, J.PROGRESSIVE_FULL if form == "progressive" else 0)
            assert rc == 0 and np.array_equal(got, want), (shape, form)
        # .. and back: the progressive file made baseline again is the source's scan
        rc, p, n = J.recode_to_host(gpu_ctx, src, "progressive")
        rc2, back, n2 = J.recode_to_host(gpu_ctx, p, "baseline", 0)
        assert rc == 0 and rc2 == 0 and U.body(back) == U.body(src)


def test_truncation_events_do_not_reach_a_recoded_file(gpu_ctx):
    """blocks the reference reads short (JDA_INDEX_TRUNC): the recoded coefficients are T.81's -- the suite's own decoder's --,
    from the host index and from the device index"""
    f = jpeg_for("c420_256x256_q98")
    assert J.PreparedImage(f).truncation_events() > 0
    for kind in ("host", "device"):
        got, nbytes, status = recode_batch(gpu_ctx, [f, f], ["optimize"] * 2, [0, None], kinds=[kind] * 2)
        assert status == [0, 0] and got[0] == got[1]
        U.same_coefficients(f, got[0])


def test_refusals(gpu_ctx):
    ref = U.refused()
    names = sorted(ref)
    good = U.written("three_quantisers")
    files = [good] + [ref[k][0] for k in names] + [good]
    for form in U.FORMS:
        ris = [None if form == "progressive" else 0] * len(files)
        got, nbytes, status = recode_batch(gpu_ctx, files, [form] * len(files), ris, kinds=["host"] * len(files))
        assert status == [0] + [ref[k][1] for k in names] + [0], (form, status)
        assert nbytes[1:-1] == [0] * len(names)
        U.same_coefficients(good, got[0])
        assert got[-1] == got[0]
    prog = U.written_progressive()
    got, nbytes, status = recode_batch(gpu_ctx, [prog, prog, good], ["baseline"] * 3, [0] * 3, kinds=["sparse", "dense", "host"])
    assert status == [U.UNSUPPORTED, 0, 0] and got[0] is None
    U.same_coefficients(prog, got[1])
    src = Sources(gpu_ctx, [good, U.written("quant16_gray")])
    buf = gpu_ctx.malloc(1 << 16)
    try:
        d, g = src.items
        call = lambda s, j, dst=(buf, buf + (1 << 15)), caps=(1 << 15, 1 << 15): J.recode_images(gpu_ctx, s, j, list(dst[:len(s)]), list(caps[:len(s)]))
        for s, j in (([d, d], [("baseline", 0), ("progressive", None)]), ([d], [("progressive", 4)]), ([d, g], [("progressive", None)] * 2), ([d], [(3, 0)]),
                     ([d], [("baseline", 65536)])):
            with pytest.raises(J.JdaError) as e:
                call(s, j)
            assert e.value.code == U.INVALID_PARAMETER, j
        with pytest.raises(J.JdaError) as e:
            call([d, d], [("baseline", 0)] * 2, dst=(buf, buf + 100))
        assert e.value.code == U.INVALID_PARAMETER, "destinations that overlap"
        lib = J.load_library()
        both = (J.binding.RecodeSource * 1)(J.binding.RecodeSource(d.handle, None))
        both[0].coef = d.handle
        nb, st = (J.binding.C.c_int64 * 1)(), (J.binding.C.c_int32 * 1)()
        job = (J.binding.RecodeJob * 1)(J.binding.RecodeJob(0, 0, 0, 0))
        args = ((J.binding.C.c_void_p * 1)(buf), (J.binding.C.c_int64 * 1)(1 << 15), nb, st)
        assert lib.jda_recode_images(gpu_ctx.handle, 1, both, job, *args) == U.INVALID_PARAMETER, "a source with both pointers set"
        both[0].image = both[0].coef = None
        assert lib.jda_recode_images(gpu_ctx.handle, 1, both, job, *args) == U.INVALID_PARAMETER, "a source with neither"
    finally:
        gpu_ctx.free(buf)
        src.close()
