"""The lossless recode on the CPU (tests/hostsim/recode_sim.cpp: the plan of jda_recode_images and every lane of jda_rc_extract and
jda_rc_from_coef through the kernels' own code, every load and store held to the uploaded allocations):

* the coefficients and block words the stages leave = the twin's (tests/recode_util.py: the suite's own decoders over the source file),
  for Pillow's four files of every shape and for the written edge files;
* every later stage of the target form runs behind them as encode_sim.cpp, huffopt_sim.cpp and encode_prog_sim.cpp step it, the host's table
  and header steps between them: the files are Pillow's, from any of Pillow's four sources, in all three forms, with the source's interval,
  none, and another; the written sources come back coefficient for coefficient, quantiser for quantiser, in all three forms;
* the plan: DQT segments, bounds, the encoder's own headers through the generalised builders, every refusal;
* the plan and the lanes once more as a program of their own under ASan + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import encode_util as E
from tests import recode_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A


class Info(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "ncomp", "subsample", "bpp", "jpeg_type", "restart_interval", "orientation", "mcu_w", "mcu_h", "mcus_x",
                                         "mcus_y", "scan_offset", "blocks_per_mcu", "has_thumb", "thumb_w", "thumb_h", "thumb_offset", "scan_start", "scan_end", "approx")]


class Job(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("form", "restart_interval", "reserved0", "reserved1")]


class RcSrc(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("scan", "blk_index", "blk_dc", "tables", "coef")] + [("scan_len", C.c_uint32), ("kind", C.c_uint32), ("ac_id", C.c_uint32 * 3),
                                                                                              ("pad_", C.c_uint32)]


class Host(C.Structure):
    _fields_ = [("kind", C.c_int), ("info", Info), ("quant", C.c_uint16 * 192), ("q_id", C.c_uint8 * 3), ("adobe", C.c_int), ("n_mcus_ok", C.c_uint32), ("dev", RcSrc)]


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_recodesim.so"))
    lib.recodesim_files.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p]
    lib.recodesim_check.argtypes = [C.c_int, C.POINTER(Host), C.POINTER(Job), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.recodesim_bound.argtypes = [C.POINTER(Info), C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.recodesim_dqt.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.recodesim_quality_header.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int]
    return lib


def run_sim(sim, files, forms, ris, sparse=None, caps=None, cap_default=1 << 20):
    """-> (rc, files or None a job, sizes, statuses, coef (blocks, 64) int16, meta, bad words, info)"""
    n = len(files)
    caps = list(caps) if caps is not None else [cap_default] * n
    offs = np.concatenate([[0], np.cumsum([(c + 63) & ~63 for c in caps])]).astype(np.int64)
    blob = np.full(int(offs[-1]) + 64, GUARD, dtype=np.uint8)
    base = blob.ctypes.data
    import jpegdec_amd as J
    nb_max = 1
    for f in files:
        d = J.parse(f)
        nb_max += max(d["mcus_x"] * d["mcus_y"] * d["blocks_per_mcu"], 0)
    coef, meta = np.zeros((nb_max, 64), np.int16), np.zeros(nb_max, np.uint32)
    bad, info = np.zeros(n, np.uint32), np.zeros(4, np.uint64)
    nbytes, status = (C.c_int64 * n)(), (C.c_int32 * n)(*([-1] * n))
    hdr_len = C.c_int64(0)
    rc = sim.recodesim_files(n, (C.c_char_p * n)(*files), (C.c_int32 * n)(*[len(f) for f in files]), (C.c_int32 * n)(*[U.FORM_ID[f] if isinstance(f, str) else f for f in forms]),
                             (C.c_int32 * n)(*[-1 if r is None else r for r in ris]), None if sparse is None else (C.c_int32 * n)(*sparse),
                             (C.c_void_p * n)(*[base + int(o) for o in offs[:n]]), (C.c_int64 * n)(*caps), nbytes, status, coef.ctypes.data, meta.ctypes.data, bad.ctypes.data,
                             None, 0, C.byref(hdr_len), info.ctypes.data)
    out = []
    for i in range(n):
        lo, hi = int(offs[i]), int(offs[i + 1])
        written = status[i] == 0 and 0 < nbytes[i] <= caps[i]
        out.append(blob[lo:lo + nbytes[i]].tobytes() if written else None)
        assert (blob[lo + (nbytes[i] if written else 0):hi] == GUARD).all(), "a byte behind the file, or of a file that is not written"
    nb = int(info[0])
    return rc, out, list(nbytes), list(status), coef[:nb], meta[:nb], bad, info


def twin_arrays(files):
    cs, ms = [], []
    for f in files:
        c, m = U.twin_of(f)
        cs.append(c)
        ms.append(m)
    return np.concatenate(cs), np.concatenate(ms)


# ---- Pillow's files, any direction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", (False, True))
def test_baseline_targets_are_pillows_files(sim, colour):
    """one call over every Pillow source of every shape, per target interval: coef and meta are the twin's, the files Pillow's"""
    pytest.importorskip("PIL")
    jobs = U.pillow_jobs(colour)
    assert len(jobs) >= (5 if not colour else 25)
    files = [j[0] for j in jobs]
    want_c, want_m = twin_arrays(files)
    for ri in (0, U.PILLOW_RESTART):
        rc, got, nbytes, status, coef, meta, bad, info = run_sim(sim, files, ["baseline"] * len(files), [ri] * len(files))
        assert rc == 0 and status == [0] * len(files) and not bad.any()
        assert np.array_equal(coef, want_c) and np.array_equal(meta, want_m)
        assert info[2] == 1 and info[3] == 1, "one launch of each stage: the call mixes baseline and progressive sources"
        for (src, pil), f in zip(jobs, got):
            U.is_pillow(f, U.want_of(pil, "baseline", ri), "baseline", source=src)
    # the source's own interval: the restart file comes back as it is, the others without an interval
    rc, got, nbytes, status, coef, meta, bad, info = run_sim(sim, files, ["baseline"] * len(files), [None] * len(files))
    assert rc == 0 and status == [0] * len(files)
    for (src, pil), f in zip(jobs, got):
        own = U.decode_any(src)["restart_interval"]
        U.is_pillow(f, U.want_of(pil, "baseline", own), "baseline", source=src)


@pytest.mark.parametrize("form", ("optimize", "progressive"))
def test_other_targets_are_pillows_files(sim, form):
    """an optimised and a progressive call over every Pillow source, gray and colour: the arrays are the twin's (a workgroup straddling jobs),
    and the files through the simulated later stages -- the host's tables and headers with the source's DQT segments between them -- Pillow's"""
    pytest.importorskip("PIL")
    for colour in (False, True):
        jobs = U.pillow_jobs(colour)
        files = [j[0] for j in jobs]
        want_c, want_m = twin_arrays(files)
        rc, got, nbytes, status, coef, meta, bad, info = run_sim(sim, files, [form] * len(files), [None if form == "progressive" else 0] * len(files))
        assert rc == 0 and status == [0] * len(files) and not bad.any()
        assert np.array_equal(coef, want_c) and np.array_equal(meta, want_m)
        for (src, pil), f in zip(jobs, got):
            U.is_pillow(f, U.want_of(pil, form, 0), form, source=src)


# ---- written sources --------------------------------------------------------------------------------------------------------------
def test_written_sources_come_back_coefficient_for_coefficient(sim):
    names = sorted(U.written_specs())
    files = [U.written(k) for k in names] + [U.written_progressive()]
    want_c, want_m = twin_arrays(files)
    rc, got, nbytes, status, coef, meta, bad, info = run_sim(sim, files, ["baseline"] * len(files), [0] * len(files))
    assert rc == 0 and status == [0] * len(files) and not bad.any()
    assert np.array_equal(coef, want_c) and np.array_equal(meta, want_m)
    for name, src, f in zip(names + ["progressive"], files, got):
        U.same_coefficients(src, f)
        assert U.front(f).count(b"\xff\xfe") == 0 and b"\xff\xdb" in U.front(f), name
    # 16-bit entries make a 16-bit DQT, and only they; three tables make three segments under the source's ids
    by = dict(zip(names, got))
    # .. and under the other two forms: the headers with three tables, ids 2 and 3, one table for all and 16-bit entries through the host's
    # table steps (the room kept for an optimised job's header, the growth of a progressive file's), the same bytes in front of SOF
    colour = [k for k in names if not k.endswith("gray")]
    for form in ("optimize", "progressive"):
        for group in (colour + ["progressive"], [k for k in names if k.endswith("gray")]):
            srcs = [U.written_progressive() if k == "progressive" else U.written(k) for k in group]
            rc, out, nb2, st2, *_ = run_sim(sim, srcs, [form] * len(srcs), [None if form == "progressive" else 0] * len(srcs))
            assert rc == 0 and st2 == [0] * len(srcs), (form, st2)
            for k, src, f in zip(group, srcs, out):
                U.same_coefficients(src, f)
                if k != "progressive":
                    assert U.front(f) == U.front(by[k]), (form, k)
    assert U.front(by["quant16"]).count(b"\xff\xdb\x00\x83\x10") == 1 and U.front(by["quant16"]).count(b"\xff\xdb\x00\x43\x01") == 1
    assert [U.front(by["three_quantisers"]).count(b"\xff\xdb\x00\x43" + bytes([t])) for t in (0, 1, 2)] == [1, 1, 1]
    assert U.front(by["ids_2_and_3"]).count(b"\xff\xdb") == 2 and U.frame_header(by["ids_2_and_3"])[-9:] == bytes([1, 0x22, 2, 2, 0x11, 3, 3, 0x11, 3])
    assert U.front(by["one_table_for_all"]).count(b"\xff\xdb") == 1


def test_restart_intervals(sim):
    """sources with an interval of 1, of an MCU row and one that does not divide the MCU count, each to its own, to none and to another"""
    srcs = U.restart_sources()
    files, ris = [], []
    for f, mcus, cx in srcs:
        for t in U.RESTART_TARGETS:
            files.append(f)
            ris.append(t)
    rc, got, nbytes, status, coef, meta, bad, info = run_sim(sim, files, ["baseline"] * len(files), ris)
    assert rc == 0 and status == [0] * len(files)
    for src, t, f in zip(files, ris, got):
        U.same_coefficients(src, f)
        own = U.decode_any(src)["restart_interval"]
        assert U.decode_any(f)["restart_interval"] == (own if t is None else t)


def test_truncation_events_do_not_reach_the_arrays(sim):
    """a fixture whose blocks the reference reads short: the arrays are T.81's values, the suite's own decoder's"""
    import jpegdec_amd as J
    from tests.cases import jpeg_for
    f = jpeg_for("c420_256x256_q98")
    p = J.PreparedImage(f)
    assert p.truncation_events() > 0
    p.close()
    want_c, want_m = twin_arrays([f])
    rc, got, nbytes, status, coef, meta, bad, info = run_sim(sim, [f], ["baseline"], [0])
    assert rc == 0 and status == [0] and np.array_equal(coef, want_c) and np.array_equal(meta, want_m)
    U.same_coefficients(f, got[0])


# ---- refusals, capacity -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_rest_of_the_call_alone(sim):
    ref = U.refused()
    names = sorted(ref)
    good = U.written("three_quantisers")
    files = [good] + [ref[k][0] for k in names] + [good]
    for form in U.FORMS:
        rc, got, nbytes, status, coef, meta, bad, info = run_sim(sim, files, [form] * len(files), [None if form == "progressive" else 0] * len(files))
        assert rc == 0 and status == [0] + [ref[k][1] for k in names] + [0], (form, status)
        assert [bool(b) for b in bad] == [False] + [k in ("ac_1024", "dc_1024", "dc_minus_1025") for k in names] + [False]
        assert all(g is None for g in got[1:-1]) and nbytes[1:-1] == [0] * len(names)
        U.same_coefficients(good, got[0])
        assert got[-1] == got[0]
    # a sparse coefficient image; progressive mixed with baseline; a progressive target with an interval; gray with colour in a progressive call
    prog = U.written_progressive()
    rc, got, nbytes, status, *_ = run_sim(sim, [prog, good], ["baseline"] * 2, [0, 0], sparse=[1, 0])
    assert rc == 0 and status == [U.UNSUPPORTED, 0] and got[0] is None
    assert run_sim(sim, [good, good], ["baseline", "progressive"], [0, None])[0] == U.INVALID_PARAMETER
    assert run_sim(sim, [good], ["progressive"], [4])[0] == U.INVALID_PARAMETER
    assert run_sim(sim, [good, U.written("quant16_gray")], ["progressive"] * 2, [None] * 2)[0] == U.INVALID_PARAMETER
    assert run_sim(sim, [good], [3], [0])[0] == U.INVALID_PARAMETER and run_sim(sim, [good], ["baseline"], [65536])[0] == U.INVALID_PARAMETER


@pytest.mark.parametrize("form", U.FORMS)
def test_capacity_a_byte_short(sim, form):
    files = [U.written("three_quantisers"), U.written("quant16"), U.written("huff_custom_c420")]
    ris = [None if form == "progressive" else 0] * 3
    rc, got, nbytes, status, *_ = run_sim(sim, files, [form] * 3, ris)
    assert rc == 0 and status == [0] * 3
    caps = [nbytes[0], nbytes[1] - 1, nbytes[2]]
    rc, again, nb2, st2, *_ = run_sim(sim, files, [form] * 3, ris, caps=caps)
    assert rc == 0 and st2 == [0, U.ERROR_MEMORY, 0] and nb2 == nbytes, "the size it needs, and no byte of it"
    assert again[0] == got[0] and again[1] is None and again[2] == got[2]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_the_encoders_own_headers_are_what_they_were(sim):
    """jda_encode_header through the generalised builders = the bytes the numpy twin of the encoder writes in front of the scan"""
    for sampling in E.SAMPLINGS:
        for q, ri in ((75, 0), (30, 5), (100, 0)):
            img = E.picture("flat", 17, 9, sampling)
            twin = E.file_bytes(img, sampling, q, ri)
            buf = np.zeros(2048, np.uint8)
            n = sim.recodesim_quality_header(17, 9, E.SAMPLING_ID[sampling], q, ri, buf.ctypes.data, buf.size)
            assert 0 < n <= buf.size and buf[:n].tobytes() == twin[:n] and twin[:n].endswith(b"\x00\x3f\x00"), (sampling, q, ri)


def _info_of(jpeg):
    import jpegdec_amd as J
    d = J.parse(jpeg)
    assert d.pop("status") == 0
    return Info(**d)


def test_bounds_and_dqt(sim):
    import jpegdec_amd as J
    lib = J.load_library()
    for name in ("three_quantisers", "quant16", "quant16_gray", "huff_custom_c420"):
        f = U.written(name)
        info = _info_of(f)
        sampling = U.decode_any(f)["sampling"]
        for form, ri in (("baseline", 0), ("baseline", 3), ("optimize", 0), ("progressive", None)):
            b = C.c_int64()
            assert sim.recodesim_bound(C.byref(info), U.FORM_ID[form], -1 if ri is None else ri, C.byref(b)) == 0
            e = C.c_int64()
            if form == "progressive":
                assert lib.jda_encode_bound_progressive(info.width, info.height, E.SAMPLING_ID[sampling], C.byref(e)) == 0
            else:
                assert lib.jda_encode_bound(info.width, info.height, E.SAMPLING_ID[sampling], ri, C.byref(e)) == 0
            nc = info.ncomp
            assert b.value == e.value + nc * 133 - (69 if nc == 1 else 138), "the encoder's bound and the header's growth: a 16-bit table a component"
    b = C.c_int64()
    info = _info_of(U.refused()["c440"][0])
    assert sim.recodesim_bound(C.byref(info), 0, 0, C.byref(b)) == U.UNSUPPORTED
    info = _info_of(U.written("quant16"))
    assert sim.recodesim_bound(C.byref(info), 2, 5, C.byref(b)) == U.INVALID_PARAMETER and sim.recodesim_bound(C.byref(info), 2, -1, C.byref(b)) == 0
    # DQT: a segment per distinct id in the order Y, Cb, Cr first name it; a zero entry or one id with two contents is refused
    q = np.zeros((3, 64), np.uint16)
    q[0], q[1], q[2] = 3, 4, 4
    out = np.zeros(512, np.uint8)
    n = sim.recodesim_dqt(3, q.ctypes.data, (C.c_uint8 * 3)(1, 0, 0), out.ctypes.data, out.size)
    assert out[:n].tobytes() == b"\xff\xdb\x00\x43\x01" + bytes([3] * 64) + b"\xff\xdb\x00\x43\x00" + bytes([4] * 64)
    q[2, 5] = 9
    assert sim.recodesim_dqt(3, q.ctypes.data, (C.c_uint8 * 3)(1, 0, 0), out.ctypes.data, out.size) == -1
    assert sim.recodesim_dqt(3, q.ctypes.data, (C.c_uint8 * 3)(1, 0, 2), out.ctypes.data, out.size) == 3 * 69
    q[1, 63] = 0
    assert sim.recodesim_dqt(3, q.ctypes.data, (C.c_uint8 * 3)(1, 0, 2), out.ctypes.data, out.size) == -1


def test_plan_checks_on_described_sources(sim):
    """the checks on sources described by hand: a source of both kinds or none is the runtime's to refuse; here the per-job rules"""
    info = _info_of(U.written("three_quantisers"))
    h = Host()
    h.kind, h.info, h.n_mcus_ok = 0, info, info.mcus_x * info.mcus_y
    for i in range(192):
        h.quant[i] = 5
    h.q_id[0], h.q_id[1], h.q_id[2] = 0, 1, 1
    dst, cap, st = (C.c_void_p * 2)(0x10000, 0x20000), (C.c_int64 * 2)(4096, 4096), (C.c_int32 * 2)()
    hosts, jobs = (Host * 2)(h, h), (Job * 2)(Job(0, 0, 0, 0), Job(1, -1, 0, 0))
    assert sim.recodesim_check(2, hosts, jobs, dst, cap, st) == 0 and list(st) == [0, 0]
    hosts[1].n_mcus_ok -= 1
    assert sim.recodesim_check(2, hosts, jobs, dst, cap, st) == 0 and list(st) == [0, U.DECODE_ERROR]
    hosts[1].n_mcus_ok += 1
    hosts[0].adobe = 1
    assert sim.recodesim_check(2, hosts, jobs, dst, cap, st) == 0 and list(st) == [U.UNSUPPORTED, 0]
    hosts[0].adobe = 0
    dst[1] = 0x10000 + 4095
    assert sim.recodesim_check(2, hosts, jobs, dst, cap, st) == U.INVALID_PARAMETER, "destinations that overlap"
    dst[1] = 0x20000
    jobs[0].reserved1 = 1
    assert sim.recodesim_check(2, hosts, jobs, dst, cap, st) == U.INVALID_PARAMETER
    jobs[0].reserved1 = 0
    dst[0] = None
    assert sim.recodesim_check(2, hosts, jobs, dst, cap, st) == U.INVALID_PARAMETER


def test_sanitizers():
    """tests/hostsim/recode_main.cpp: a program of its own (make recodeasan), nothing preloaded"""
    subprocess.run(["make", "recodeasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    golden = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "recode_asan")] + [os.path.join(golden, n + ".jpg") for n in
                       ("c420_333x217", "c444_8x8_q30", "gray_64x64_rst3", "c422_333x217", "c444_384x192_q100_rst7", "p420_200x120", "pgray_100x100", "c440_200x120")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"recode_asan ok" in r.stdout, r.stdout[-2000:]
