"""The lossless flip, rotate, transpose and MCU crop on the GPU (jda_recode_images_ex, jda_recode_to_host_ex, recode(transform=); DESIGN.md
5.15), against the numpy twin of tests/recode_xf_util.py (tests/test_recode_xf_cpu.py steps the same stages lane by lane):
(a) ONE _ex call per target form over Pillow's and the written sources under every operation, with crops and trims, sources with a host
    index, with a device index and dense coefficient images side by side, the files back to back in a guard-filled allocation, twice, with
    its launches: the _xf pair once each and the plain pair not at all -- and the other way round where no job asks for anything;
    every file = the plain recode (jda_recode_images, held to Pillow by tests/test_gpu_recode.py) of the twin-written file;
(b) host index = device index; (c) jda_recode_to_host_ex and recode(transform="exif") over a mixed list; (d) the pixels of a ROT_180 file
decoded by the library = the oracle's canvas of the twin's file; (e) the refusals and the call's argument errors; (f) the geometry and bound."""
import numpy as np
import pytest

import jpegdec_amd as J
from tests import recode_util as U
from tests import recode_xf_util as X
from tests.test_gpu_recode import FILL, KERNELS, LAUNCHES, Sources

pytestmark = pytest.mark.gpu

XF_KERNELS = ("jda_rc_extract_xf", "jda_rc_from_coef_xf")


def counts():
    """launches by kernel: the plain pair's names are prefixes of the _xf pair's, so those are told apart here"""
    c = J.kernel_launch_counts()
    out = {k: sum(v for name, v in c.items() if k in name and not any(x in name for x in XF_KERNELS)) for k in KERNELS}
    out.update({k: sum(v for name, v in c.items() if k in name) for k in XF_KERNELS})
    return out


def recode_batch(ctx, files, forms, ris, xforms=None, kinds=None, caps=None):
    """-> (files or None, sizes, statuses, launches of the call by kernel): the guard behind every file and around a file that is not written is checked"""
    n = len(files)
    src = Sources(ctx, files, kinds)
    try:
        if caps is None:
            caps = []
            for i, (d, f, r) in enumerate(zip(src.items, forms, ris)):
                try:
                    caps.append(J.recode_bound(d.info, f, r, None if xforms is None else xforms[i]))
                except J.JdaError:                       # (a job the call refuses has no bound: room that must stay untouched)
                    caps.append(4096)
        offs = np.concatenate([[0], np.cumsum([(c + 15) & ~15 for c in caps])]).astype(np.int64)
        total = int(offs[-1]) + 16
        ddst = ctx.malloc(total)
        try:
            ctx.memset(ddst, FILL, total)
            before = counts()
            nbytes, status = J.recode_images(ctx, src.items, list(zip(forms, ris)), [ddst + int(o) for o in offs[:-1]], caps, xforms)
            after = counts()
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
    return out, nbytes, status, {k: after[k] - before[k] for k in after}


def check_jobs(ctx, jobs, form, ri, kinds=None, twice=False):
    """one _ex call over jobs (src, op, rect, trim): every file is the plain recode of the twin-written file; the launches are the _xf pair's"""
    n = len(jobs)
    twins = [X.twin_file(*j) for j in jobs]
    keep = [i for i in range(n) if twins[i] is not None]
    ref, _, st, _ = recode_batch(ctx, [twins[i] for i in keep], [form] * len(keep), [ri] * len(keep), None, kinds=["host"] * len(keep))
    assert st == [0] * len(keep)
    want = [None] * n
    for i, f in zip(keep, ref):
        want[i] = f
    xf = [X.xform(op, rect, trim) for _, op, rect, trim in jobs]
    got, nbytes, status, ran = recode_batch(ctx, [j[0] for j in jobs], [form] * n, [ri] * n, xf, kinds)
    assert status == [0 if w is not None else U.UNSUPPORTED for w in want], status
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, ("job", k, jobs[k][1:])
    image = any(U.frame_header(j[0])[1] != 0xC2 for j, w in zip(jobs, want) if w is not None)
    coef = any(U.frame_header(j[0])[1] == 0xC2 for j, w in zip(jobs, want) if w is not None)
    expect = dict(zip(KERNELS, LAUNCHES[form]))
    expect.update({"jda_rc_extract": 0, "jda_rc_from_coef": 0, "jda_rc_extract_xf": int(image), "jda_rc_from_coef_xf": int(coef)})
    assert ran == expect, "a fixed number of launches a call: the _xf pair in the place of the plain pair"
    if twice:
        again, nb2, st2, _ = recode_batch(ctx, [j[0] for j in jobs], [form] * n, [ri] * n, xf, kinds)
        assert again == got and nb2 == nbytes, "the same call once more: the same bytes, whatever the pool hands out"
    return got


def _colour_jobs():
    base, prog = U.pillow_files("noise", 136, 88, "4:2:0")["baseline"], U.pillow_files("noise", 136, 88, "4:2:0")["progressive"]
    ragged = U.pillow_files("noise", 333, 217, "4:2:0")["baseline"]
    jobs = []
    for s in (("noise", 8, 8, "4:4:4"), ("noise", 16, 8, "4:2:2"), ("noise", 16, 16, "4:2:0")):         # one MCU of each layout
        f = U.pillow_files(*s)
        src = f["baseline"] if len(f["baseline"]) >= 256 else f["restart"]
        jobs += [(src, op, None, False) for op in X.OPS if s[3] != "4:2:2" or op not in X.TRANSPOSING]
    one_row, one_col = U.pillow_files("noise", 80, 16, "4:2:0")["baseline"], U.pillow_files("noise", 16, 80, "4:2:0")["baseline"]
    jobs += [(f, op, None, False) for f in (one_row, one_col) for op in ("flip_h", "rot90", "transverse")]
    # 324 blocks a job: a workgroup straddles jobs with different operations and source kinds
    jobs += [(base, "rot90", None, True), (prog, "flip_h", None, True), (base, "none", None, False), (prog, "transverse", None, True), (base, "flip_v", (1, 1, 5, 3), False),
             (prog, "rot270", (0, 2, 9, 4), True), (base, "transpose", None, False), (prog, "none", None, False), (base, "rot180", None, True)]
    jobs += [(ragged, "rot180", None, True), (ragged, "rot90", None, False), (ragged, "transpose", None, False), (ragged, "rot270", (20, 13, 1, 1), True)]
    for k in ("huff_custom_c444", "huff_custom_c420", "huff_custom_c422", "three_quantisers", "quant16", "ids_2_and_3"):
        src = U.written(k)
        jobs += [(src, op, None, True) for op in ("flip_h", "flip_v", "rot90", "transverse") if not (k.endswith("c422") and op in X.TRANSPOSING)]
    jobs += [(U.written_progressive(), op, None, True) for op in X.OPS]
    small = X.coef_jpeg.write_jpeg(**U._small("4:2:0", {0: list(range(2, 66)), 1: list(range(70, 6, -1))}, seed=31, w=64, h=48))
    jobs += [(small, op, r, False) for op in ("none", "rot90") for r in ((0, 0, 1, 1), (3, 2, 1, 1), (1, 0, 2, 3), (0, 1, 4, 2), (2, 1, 2, 1))]
    return jobs


@pytest.mark.parametrize("form", U.FORMS)
def test_one_call_over_every_kind_of_job(gpu_ctx, form):
    pytest.importorskip("PIL")
    check_jobs(gpu_ctx, _colour_jobs(), form, None if form == "progressive" else 0, twice=True)


@pytest.mark.parametrize("form", U.FORMS)
def test_gray_call(gpu_ctx, form):
    pytest.importorskip("PIL")
    srcs = [U.pillow_files("noise", 333, 217, "gray")["baseline"], U.pillow_files("noise", 333, 217, "gray")["progressive"], U.written("huff_custom_gray"), U.written("quant16_gray")]
    f = U.pillow_files("noise", 8, 8, "gray")
    srcs.append(f["baseline"] if len(f["baseline"]) >= 256 else f["restart"])
    jobs = [(s, op, None, True) for s in srcs for op in X.OPS] + [(srcs[0], "rot270", (40, 0, 2, 28), True), (srcs[1], "flip_v", (0, 27, 42, 1), True)]
    check_jobs(gpu_ctx, jobs, form, None if form == "progressive" else 0)


def test_restart_targets(gpu_ctx):
    for form in ("baseline", "optimize"):
        for ri in U.RESTART_TARGETS:
            jobs = [(f, op, None, True) for f, _, _ in U.restart_sources() for op in ("flip_h", "rot90")]
            got = check_jobs(gpu_ctx, jobs, form, ri)
            for (src, *_), f in zip(jobs, got):
                assert U.decode_any(f)["restart_interval"] == (U.decode_any(src)["restart_interval"] if ri is None else ri)


def test_no_transform_runs_the_plain_stage(gpu_ctx):
    """xforms of NONE with a zero rectangle (EXIF over a file without a tag included): jda_recode_images' launches and bytes"""
    pytest.importorskip("PIL")
    files = [U.pillow_files("noise", 136, 88, "4:2:0")[k] for k in ("baseline", "progressive", "restart")] + [U.written("three_quantisers")]
    for form in U.FORMS:
        ri = [None if form == "progressive" else 0] * len(files)
        plain, nb, st, ran = recode_batch(gpu_ctx, files, [form] * len(files), ri, None)
        none, nb2, st2, ran2 = recode_batch(gpu_ctx, files, [form] * len(files), ri, [X.xform("none"), X.xform("exif"), X.xform("none", None, True), X.xform("none")])
        assert st == [0] * len(files) and st2 == st and none == plain
        for r in (ran, ran2):
            assert (r["jda_rc_extract"], r["jda_rc_from_coef"], r["jda_rc_extract_xf"], r["jda_rc_from_coef_xf"]) == (1, 1, 0, 0)
        # one job with a rectangle: the _xf pair for every job of the call, the untouched jobs' bytes unchanged
        mixed, nb3, st3, ran3 = recode_batch(gpu_ctx, files, [form] * len(files), ri, [X.xform("none"), X.xform("none"), X.xform("none", (0, 0, 2, 2)), X.xform("none")])
        assert st3 == st and [mixed[0], mixed[1], mixed[3]] == [plain[0], plain[1], plain[3]] and mixed[2] != plain[2]
        assert (ran3["jda_rc_extract"], ran3["jda_rc_from_coef"], ran3["jda_rc_extract_xf"], ran3["jda_rc_from_coef_xf"]) == (0, 0, 1, 1)


def test_host_index_and_device_index_give_the_same_file(gpu_ctx):
    from tests.cases import jpeg_for
    files = [jpeg_for(n) for n in ("c420_640x368_rstrow", "c444_384x192_q100_rst7", "gray_333x217", "c420_333x217")]
    xf = [X.xform("rot90"), X.xform("flip_h"), X.xform("rot180", None, True), X.xform("transverse", (2, 1, 17, 11), True)]
    for form in ("baseline", "optimize"):
        a, _, sa, _ = recode_batch(gpu_ctx, files, [form] * 4, [None] * 4, xf, kinds=["host"] * 4)
        b, _, sb, _ = recode_batch(gpu_ctx, files, [form] * 4, [None] * 4, xf, kinds=["device"] * 4)
        assert sa == [0] * 4 and sb == [0] * 4 and a == b
    src = Sources(gpu_ctx, files, ["device"] * 4)
    on_device = [d.prescan_on_device for d in src.items]
    src.close()
    assert on_device == [True] * 4, "the device pre-scan made these indexes"
    assert a[2] is not None and U.decode_any(a[2])["width"] == 328


def test_recode_to_host_and_recode_with_a_transform(gpu_ctx):
    pytest.importorskip("PIL")
    pil = U.pillow_files("noise", 136, 88, "4:2:0")
    for src in ("baseline", "progressive"):
        for form in U.FORMS:
            ri = None if form == "progressive" else 0
            for op, rect, trim in (("rot90", None, True), ("flip_v", (2, 1, 4, 3), False)):
                rc, f, n = J.recode_to_host(gpu_ctx, pil[src], form, ri, transform=op, crop=rect, trim=trim)
                assert rc == 0 and n == len(f)
                rc, want, n = J.recode_to_host(gpu_ctx, X.twin_file(pil[src], op, rect, trim), form, ri)
                assert rc == 0 and f == want, (src, form, op)
    assert J.recode_to_host(gpu_ctx, pil["baseline"], "optimize", transform="rot180")[0] == U.UNSUPPORTED, "a ragged mirrored axis without trim"
    assert J.recode_to_host(gpu_ctx, pil["baseline"], "optimize", crop=(0, 0, 10, 1))[0] == U.INVALID_PARAMETER
    assert J.recode_to_host(gpu_ctx, U.pillow_files("noise", 333, 217, "4:2:2")["baseline"], "optimize", transform="transpose")[0] == U.UNSUPPORTED
    rc, f, n = J.recode_to_host(gpu_ctx, pil["baseline"], "optimize", capacity=100, transform="transpose")
    assert rc == U.ERROR_MEMORY and f is None and n == len(J.recode_to_host(gpu_ctx, pil["baseline"], "optimize", transform="transpose")[1])
    # a mixed list comes out upright: every orientation, one call
    uniform = dict(qtables=[[3] * 64, [5] * 64])
    pic = X.cell_picture("4:2:0", seed=5)
    files = [X.pillow_save(pic, "4:2:0", exif_orientation=o, **uniform) for o in range(1, 9)] + [X.pillow_save(pic, "4:2:0", **uniform)]
    before = counts()
    out = J.recode(gpu_ctx, files, "optimize", transform="exif")
    after = counts()
    assert after["jda_rc_extract_xf"] - before["jda_rc_extract_xf"] == 1 and after["jda_rc_extract"] == before["jda_rc_extract"], "one recode_images_ex call"
    for o, f in zip(list(range(1, 9)) + [0], out):
        U.is_pillow(f, X.pillow_save(X.pixel_turn(pic, X.EXIF_OP[o]), "4:2:0", optimize=True, **uniform), "optimize")
        assert J.parse(f)["orientation"] == 0
    assert J.recode(gpu_ctx, files[:1], "baseline") == J.recode(gpu_ctx, files[:1], "baseline", transform="exif"), "orientation 1: as it is"


def test_pixels_of_a_rot180_file(gpu_ctx, oracle):
    """the library's decode of a ROT_180 file = the oracle's canvas of the twin's file (the same coefficients under the same tables)"""
    pytest.importorskip("PIL")
    for shape in (("noise", 136, 88, "4:2:0"), ("smooth", 333, 217, "4:4:4"), ("noise", 333, 217, "gray")):
        src = U.pillow_files(*shape)["baseline"]
        rc, f, n = J.recode_to_host(gpu_ctx, src, "baseline", 0, transform="rot180", trim=True)
        assert rc == 0
        twin = X.twin_file(src, "rot180", None, True)
        assert U.body(f) == U.body(twin)
        rc, got, g = J.decode_to_host(gpu_ctx, f, J.RGB8888, 0)
        orc, want, err = oracle.decode_canvas(twin, J.RGB8888, 0)
        assert rc == 0 and orc == 1 and got.shape == want.shape and np.array_equal(got, want), shape


def test_refusals_and_argument_errors(gpu_ctx):
    ref = U.refused()
    names = sorted(ref)
    good = U.written("three_quantisers")
    files = [good] + [ref[k][0] for k in names] + [good, U.written("huff_custom_c422"), U.pillow_files("smooth", 17, 9, "4:2:0")["baseline"]]
    xf = [X.xform("flip_v", None, True)] * (len(names) + 2) + [X.xform("transpose"), X.xform("flip_v", None, True)]
    for form in U.FORMS:
        ris = [None if form == "progressive" else 0] * len(files)
        got, nbytes, status, _ = recode_batch(gpu_ctx, files, [form] * len(files), ris, xf, kinds=["host"] * len(files))
        assert status == [0] + [ref[k][1] for k in names] + [0, U.UNSUPPORTED, U.UNSUPPORTED], (form, status)
        assert nbytes[1:len(names) + 1] == [0] * len(names) and got[0] == got[len(names) + 1] and got[0] is not None
    prog = U.written_progressive()
    got, nbytes, status, _ = recode_batch(gpu_ctx, [prog, prog, good], ["baseline"] * 3, [0] * 3, [X.xform("rot90")] * 3, kinds=["sparse", "dense", "host"])
    assert status == [U.UNSUPPORTED, 0, 0] and got[0] is None
    src = Sources(gpu_ctx, [good])
    buf = gpu_ctx.malloc(1 << 16)
    try:
        d = src.items[0]
        for t in ((9, 0, 0, 0, 0, 0), (-1, 0, 0, 0, 0, 0), (1, 2, 0, 0, 0, 0), (0, 0, -1, 0, 1, 1), (0, 0, 0, 0, 1, -1), (0, 0, 3, 0, 1, 1), (0, 0, 0, 1, 1, 2), (0, 0, 0, 0, 0, 2),
                  (0, 0, 1, 0, 0, 0), (0, 0, 2, 0, 0x7FFFFFFF, 1)):
            with pytest.raises(J.JdaError) as e:
                J.recode_images(gpu_ctx, [d, d], [("baseline", 0)] * 2, [buf, buf + (1 << 15)], [1 << 15] * 2, [X.xform("flip_h"), t])
            assert e.value.code == U.INVALID_PARAMETER, t
            with pytest.raises(J.JdaError):
                J.recode_geometry(d.info, t)
        nb, st = J.recode_images(gpu_ctx, [d, d], [("baseline", 0)] * 2, [buf, buf + (1 << 15)], [1 << 15, 100], [X.xform("rot90"), X.xform("rot90")])
        assert st == [0, U.ERROR_MEMORY] and nb[1] == nb[0] > 100
        g = J.recode_geometry(d.info, "rot90", (1, 0, 2, 2))
        assert (g.width, g.height, g.mcus_x, g.mcus_y, g.orientation) == (16, 16, 2, 2, 0)
        assert J.recode_bound(d.info, "optimize", None, X.xform("rot90", (1, 0, 2, 2))) < J.recode_bound(d.info, "optimize")
    finally:
        gpu_ctx.free(buf)
        src.close()
