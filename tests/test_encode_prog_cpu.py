"""jda_encode_surfaces_progressive without a GPU (rules 10 to 14):

* the Python twin (tests/encode_prog_util.py) = Pillow's Image.save(progressive=True), from SOF2 to EOI byte for byte, over
  encode_util.SIZES x samplings x seven pictures and over the edge pictures Pillow's output buffer takes;
* the edge pictures are what they are listed for -- asserted from the twin's layout: runs cut by the 937 rule, a run of 0x7FFF, ZRLs in
  first and refinement scans and a refinement block that writes none, a band that ends nonzero at position 63, runs open at a scan's end,
  runs across units 63 | 64 and 255 | 256 and across a row of blocks, dummy blocks;
* the stages lane by lane through the kernels' own code (tests/hostsim/encode_prog_sim.cpp over jda_pe_* of jda_device_core.h and the
  host plan jda_encode_prog_plan.h) under encode_sim.cpp's memory policy = the twin: unit records, run words, histograms, bit positions,
  every scan's header and size, the files; the run-resolution stage alone against a one-unit-after-the-other walk;
* the bound; every refusal; the same code as a program of its own under ASan + UBSan."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from tests import encode_util as E
from tests import encode_prog_util as P
from tests.encode_opt_util import PILLOW_PICTURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, MEMORY = 1, 3, 5
GUARD = 0x5A


class Output(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("pitch_bytes", C.c_int32), ("width_px", C.c_int32), ("rows", C.c_int32)]


class Job(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("x", "y", "w", "h", "sampling", "quality", "restart_interval", "reserved")]


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_encodeprogsim.so"))
    lib.encodeprogsim_lanes.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(Job), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int32)] + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p]
    lib.encodeprogsim_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.encodeprogsim_check.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(Job), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.encodeprogsim_bound.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int64)]
    return lib


def bound(sim, w, h, sampling):
    b = C.c_int64()
    assert sim.encodeprogsim_bound(w, h, E.SAMPLING_ID[sampling], C.byref(b)) == 0
    return b.value


def run_sim(sim, cases, caps=None):
    """cases: [(img, sampling, quality)] of ONE pixel size.  The rectangles sit at (3, 2) of guard-filled surfaces, the files back to back in
    one guard-filled block (capacity: the twin's size unless given).  -> (files or None, sizes, statuses, per case a list of per-scan dicts)"""
    n = len(cases)
    bpp = 1 if cases[0][1] == "gray" else 4
    surfs, outs, jobs = [], (Output * n)(), (Job * n)()
    twins = [P.file_bytes_prog(*c, return_layout=True) for c in cases]
    for i, (img, sampling, q) in enumerate(cases):
        h, w = img.shape[:2]
        s = np.full((h + 5, (w + 7) * bpp + 4 - (w + 7) * bpp % 4), GUARD, dtype=np.uint8)
        s[2:2 + h, 3 * bpp:(3 + w) * bpp] = img.reshape(h, w * bpp)
        surfs.append(s)
        outs[i] = Output(s.ctypes.data, s.shape[1], w + 7, h + 5)
        jobs[i] = Job(3, 2, w, h, E.SAMPLING_ID[sampling], q, 0, 0)
    if caps is None:
        caps = [len(t[0]) for t in twins]
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    block = np.full(int(offs[-1]) + 16, GUARD, dtype=np.uint8)
    dst = (C.c_void_p * n)(*[block.ctypes.data + int(o) for o in offs[:-1]])
    cap = (C.c_int64 * n)(*caps)
    nbytes, status = (C.c_int64 * n)(), (C.c_int32 * n)()
    nu = sum(L["n_units"] for t in twins for L in t[1])
    ns = sum(len(t[1]) for t in twins)
    cls, run, ln = (np.zeros(nu, dtype=np.uint32) for _ in range(3))
    end, hist, seginfo = np.zeros(nu, dtype=np.uint64), np.zeros((ns, 256), dtype=np.uint32), np.zeros((ns, 4), dtype=np.uint64)
    hdr, info = np.zeros(ns * 800, dtype=np.uint8), np.zeros(5, dtype=np.uint64)
    rc = sim.encodeprogsim_lanes(n, outs, bpp, jobs, dst, cap, nbytes, status, cls.ctypes.data, run.ctypes.data, ln.ctypes.data, end.ctypes.data, hist.ctypes.data,
                                 seginfo.ctypes.data, hdr.ctypes.data, len(hdr), info.ctypes.data)
    assert rc == 0, rc
    assert int(info[1]) == nu and int(info[2]) == ns
    files, per, s, h0 = [], [], 0, 0
    for i in range(n):
        o = int(offs[i])
        if status[i] == 0:
            files.append(block[o:o + nbytes[i]].tobytes())
            assert np.all(block[o + nbytes[i]:o + caps[i]] == GUARD)
        else:
            files.append(None)
            assert np.all(block[o:o + caps[i]] == GUARD)
        scans = []
        for _ in twins[i][1]:
            u0, k, hl, sb = (int(v) for v in seginfo[s])
            scans.append(dict(cls=cls[u0:u0 + k], run=run[u0:u0 + k], len=ln[u0:u0 + k], end=end[u0:u0 + k], hist=hist[s], header=hdr[h0:h0 + hl].tobytes(), unstuffed_bytes=sb))
            s, h0 = s + 1, h0 + hl
        per.append(scans)
    assert np.all(block[int(offs[-1]):] == GUARD)
    return files, list(nbytes), list(status), per


def check_case(got_file, scans, case):
    jpeg, lay = P.file_bytes_prog(*case, return_layout=True)
    assert len(scans) == len(lay)
    for k, (g, L) in enumerate(zip(scans, lay)):
        where = (case[1], case[0].shape, k)
        assert np.array_equal(g["cls"], L["cls"]), ("unit records", where)
        assert np.array_equal(g["run"], L["run"]), ("run words", where)
        assert np.array_equal(g["hist"], P.hist_words(L)), ("histogram", where)
        assert np.array_equal(g["len"].astype(np.int64), L["len"]), ("lengths", where)
        assert np.array_equal(g["end"].astype(np.int64), L["end"]), ("bit positions", where)
        assert g["unstuffed_bytes"] == L["unstuffed_bytes"], ("scan bytes", where)
        assert g["header"].endswith(L["header"]) and (k > 0) == (g["header"] == L["header"]), ("header", where)
    assert got_file == jpeg, "file"


# ---- the twin against Pillow -------------------------------------------------------------------------------------------------------
def pillow_file(img, sampling, q, **kw):
    from PIL import Image
    im = Image.fromarray(img) if sampling == "gray" else Image.fromarray(np.ascontiguousarray(img[..., :3]))
    if sampling != "gray":
        kw["subsampling"] = E.PILLOW_SUBSAMPLING[sampling]
    out = io.BytesIO()
    im.save(out, "JPEG", quality=q, progressive=True, **kw)
    return out.getvalue()


def from_sof2(f):
    return f[f.index(b"\xff\xc2"):]


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_twin_is_pillow_over_the_grid(sampling):
    pytest.importorskip("PIL")
    n = 0
    for w, h in E.SIZES:
        for kind, q in PILLOW_PICTURES:
            img = E.picture(kind, w, h, sampling)
            assert from_sof2(P.file_bytes_prog(img, sampling, q)) == from_sof2(pillow_file(img, sampling, q)), (w, h, kind, q)
            n += 1
    assert n == len(E.SIZES) * len(PILLOW_PICTURES)


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_twin_is_pillow_over_the_edges(sampling_class):
    """every edge picture lies inside Pillow's output buffer -- Pillow saves each of them --; optimize=True changes nothing"""
    pytest.importorskip("PIL")
    cases = P.edge_cases(sampling_class) + ([(E.picture(*P.FLAT_LIMIT[:4]), "gray", P.FLAT_LIMIT[4])] if sampling_class == "gray" else [])
    for img, sampling, q in cases:
        mine = P.file_bytes_prog(img, sampling, q)
        h, w = img.shape[:2]
        assert from_sof2(mine) == from_sof2(pillow_file(img, sampling, q)), (w, h, sampling, q)
        if w * h < 4096:
            assert from_sof2(mine) == from_sof2(pillow_file(img, sampling, q, optimize=True))


# ---- the edge pictures are what they are listed for ----------------------------------------------------------------------------------
def _layout(img, sampling, q):
    return P.file_bytes_prog(img, sampling, q, return_layout=True)[1]


def _refinements(lay):
    return [L for L in lay if L["ss"] and L["ah"]]


@pytest.mark.parametrize("sampling", ("gray", "4:4:4"))
def test_repeated_block_is_cut_by_the_937_rule(sampling):
    lay = _layout(P.repeated_block(sampling), sampling, 100)
    luma = [L for L in _refinements(lay) if L["comps"] == (0,)]
    assert len(luma) == 2
    for L in luma:
        assert not (L["cls"] & P.BREAKER).any()                                   # no coefficient of any block is newly nonzero
        cut = [r for r in L["runs"] if r[3] == "bits"]
        assert len(cut) >= 2 and all(r[2] > P.MAX_BE and r[2] - int((L["cls"][r[0] + r[1] - 1] >> 8) & 63) <= P.MAX_BE for r in cut)
        assert sum(r[1] for r in L["runs"]) == 40 and len(L["data"]) == 317


def test_flat_1456_runs_to_the_limit():
    lay = _layout(E.picture(*P.FLAT_LIMIT[:4]), "gray", P.FLAT_LIMIT[4])
    for L in lay:
        if L["ss"]:
            assert [(r[1], r[3]) for r in L["runs"]] == [(0x7FFF, "limit"), (33124 - 0x7FFF, "end")] and len(L["data"]) == 6


def test_zrl_picture_has_zrls_and_a_block_that_writes_none():
    """at ZRL_QUALITY the picture's coefficients of 2 and 3 first show in the refinement scan Ah 2 (ZRLs there, and blocks whose last 31 and more
    zeros lie behind their only newly nonzero coefficient); at quality 50 they are 4 and more and the first scan 6-63 has the ZRLs"""
    refs = _refinements(_layout(E.zrl_picture(), "gray", E.ZRL_QUALITY))
    assert sum(L["zrl"] for L in refs) > 0 and sum(L["no_zrl"] for L in refs) > 0
    assert sum(L["zrl"] for L in _layout(E.zrl_picture(), "gray", 50) if L["ss"] and not L["ah"]) > 0


def test_last_nonzero_picture_ends_its_band_at_63():
    lay = _layout(P.last_nonzero_picture(), "gray", 100)
    L = [L for L in lay if L["ss"] == 6 and not L["ah"]][0]
    assert int(L["cls"][1]) & 3 == P.BREAKER                                       # a symbol of its own and no run joined: the band ends nonzero
    assert all(int(c) & 3 == P.JOINS for c in (L["cls"][0], L["cls"][2]))


def test_runs_open_at_the_end_and_across_the_lane_edges():
    gray = P.edge_cases("gray")
    ends = [r[3] for c in gray for L in _layout(*c) for r in L["runs"]]
    assert ends.count("end") > 20 and ends.count("breaker") > 20
    for img, s, q in (gray[5], gray[7]):                                           # flat 2056 x 8 (257 units) and 264 x 240 (990 units, 33 a row)
        for L in _layout(img, s, q):
            if L["ss"]:
                assert len(L["runs"]) == 1 and L["runs"][0][:2] == (0, L["n_units"])       # one run over 63 | 64, 255 | 256 and every row
    smooth = _layout(*gray[9])                                                     # 264 x 16: runs that begin in one row of blocks and end in the next
    assert any(r[0] // 33 != (r[0] + r[1] - 1) // 33 and r[3] == "breaker" for L in smooth for r in L["runs"])


def test_dummy_blocks_are_in_the_dc_scans_only():
    dummies = 0
    for img, s, q in P.edge_cases("colour"):
        h, w = img.shape[:2]
        if s == "4:4:4" or (w, h) == (1, 1):
            continue
        lay = _layout(img, s, q)
        hs, vs = (2, 2) if s == "4:2:0" else (2, 1)
        cx, cy = -(-w // (8 * hs)), -(-h // (8 * vs))
        assert lay[0]["n_units"] == lay[6]["n_units"] == cx * cy * (hs * vs + 2)
        assert lay[1]["n_units"] == -(-w // 8) * -(-h // 8) and lay[2]["n_units"] == cx * cy
        dummies += lay[1]["n_units"] < cx * cy * hs * vs
    assert dummies == 4                                                            # 17 x 9 and 33 x 47 in both samplings (25 x 16 fills its MCUs)


# ---- the stages, lane by lane ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_lanes_are_the_twin(sim, sampling_class):
    cases = P.batch(sampling_class)
    files, sizes, status, per = run_sim(sim, cases)
    assert all(s == 0 for s in status)
    for f, scans, case in zip(files, per, cases):
        check_case(f, scans, case)


def test_lanes_flat_1456(sim):
    case = (E.picture(*P.FLAT_LIMIT[:4]), "gray", P.FLAT_LIMIT[4])
    files, sizes, status, per = run_sim(sim, [case])
    check_case(files[0], per[0], case)


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_a_byte_short(sim, sampling_class):
    cases = P.edge_cases(sampling_class)[:6]
    caps = [len(P.file_bytes_prog(*c)) for c in cases]
    caps[1] -= 1
    caps[4] -= 1
    files, sizes, status, per = run_sim(sim, cases, caps)
    for i, c in enumerate(cases):
        assert sizes[i] == len(P.file_bytes_prog(*c))
        assert status[i] == (MEMORY if i in (1, 4) else 0) and (files[i] is None) == (i in (1, 4))
        if files[i] is not None:
            assert files[i] == P.file_bytes_prog(*c)


def walk(cls):
    """the run words of unit records, one unit after the other, as jcphuff.c keeps EOBRUN and BE"""
    run = np.zeros(len(cls), dtype=np.uint32)
    first, n, be, offs = 0, 0, 0, []

    def flush():
        nonlocal n, be, offs
        if n:
            run[first] = P.IN_RUN | P.HEAD | (n << 10) | be
            for i, off in enumerate(offs[1:], 1):
                run[first + i] = P.IN_RUN | (i << 10) | off
        n, be, offs = 0, 0, []
    for u, c in enumerate(cls.tolist()):
        if c & P.BREAKER:
            flush()
        if c & P.JOINS:
            if not n:
                first = u
            offs.append(be)
            n, be = n + 1, be + ((c >> 8) & 63)
            if n == P.MAX_RUN or be > P.MAX_BE:
                flush()
    flush()
    return run


def resolve(sim, cls):
    cls = np.ascontiguousarray(cls, dtype=np.uint32)
    run = np.zeros(len(cls), dtype=np.uint32)
    assert sim.encodeprogsim_resolve(cls.ctypes.data, len(cls), run.ctypes.data) == 0
    return run


def test_resolve_alone(sim):
    J, B = P.JOINS, P.BREAKER
    bits = lambda k: J | (k << 8)
    chosen = {
        "937 exactly: no cut": [bits(63)] * 14 + [bits(55)] + [bits(1)] * 3,
        "938: a cut": [bits(63)] * 14 + [bits(56)] + [bits(1)] * 3,
        "32767": [J] * 32767,
        "32768": [J] * 32768,
        "32767 then a breaker": [J] * 32767 + [B] + [J] * 3,
        "stretches of one": [J, B, J, B, J, B | J, B | J, B, B, J],
        "breakers that join": [B | bits(5)] * 40 + [B] + [bits(63)] * 40,
        "a breaker opens the scan": [B | J, J, J, B],
        "no run at all": [B] * 300,
        "bits and the limit together": [bits(0)] * 32760 + [bits(63)] * 40,
    }
    for name, cls in chosen.items():
        cls = np.asarray(cls, dtype=np.uint32)
        got, want = resolve(sim, cls), walk(cls)
        assert np.array_equal(got, want), name
    got = resolve(sim, chosen["938: a cut"])
    assert int(got[0]) == P.IN_RUN | P.HEAD | (15 << 10) | 938 and int(got[15]) == P.IN_RUN | P.HEAD | (3 << 10) | 3
    got = resolve(sim, chosen["937 exactly: no cut"])
    assert int(got[0]) == P.IN_RUN | P.HEAD | (16 << 10) | 938 and int(got[14]) == P.IN_RUN | (14 << 10) | 882 and int(got[16]) == P.IN_RUN | P.HEAD | (2 << 10) | 2
    got = resolve(sim, chosen["32768"])
    assert int(got[0]) == P.IN_RUN | P.HEAD | (32767 << 10) and int(got[32767]) == P.IN_RUN | P.HEAD | (1 << 10)
    rng = np.random.default_rng(7)
    for trial in range(30):
        n = int(rng.integers(1, 3000))
        b = rng.random(n) < rng.choice([0.0, 0.02, 0.3])
        j = np.where(b, rng.random(n) < 0.5, True)
        cls = b * B + j * J + (rng.integers(0, 64, n) * (rng.random(n) < 0.8) * j << 8)
        assert np.array_equal(resolve(sim, cls), walk(cls.astype(np.uint32))), trial


# ---- the bound, the refusals, the sanitizers ------------------------------------------------------------------------------------------------
def test_bound_holds(sim):
    for s in E.SAMPLINGS:
        for w, h in E.SIZES:
            assert bound(sim, w, h, s) >= len(P.file_bytes_prog(E.picture("noise", w, h, s), s, 100)), (s, w, h)
    for cls in ("gray", "colour"):
        for img, s, q in P.edge_cases(cls):
            assert bound(sim, img.shape[1], img.shape[0], s) >= len(P.file_bytes_prog(img, s, q))
    b = C.c_int64()
    assert sim.encodeprogsim_bound(0, 8, 0, C.byref(b)) == INVALID and sim.encodeprogsim_bound(8, 65536, 0, C.byref(b)) == INVALID
    assert sim.encodeprogsim_bound(8, 8, 4, C.byref(b)) == INVALID and sim.encodeprogsim_bound(8, 8, 0, None) == INVALID


def test_refusals(sim):
    surf = np.zeros((64, 256), dtype=np.uint8)
    files = np.zeros(1 << 16, dtype=np.uint8)

    def check(job=(0, 0, 16, 16, 0, 75, 0, 0), out=None, bpp=1, n=1, dst=None, cap=4096):
        o = (Output * 1)(Output(*(out or (surf.ctypes.data, 256, 256 // bpp, 64))))
        j = (Job * 1)(Job(*job))
        dd = (C.c_void_p * 1)(files.ctypes.data if dst is None else dst)
        cc = (C.c_int64 * 1)(cap)
        return sim.encodeprogsim_check(n, o, bpp, j, dd, cc)
    assert check() == 0 and check(job=(0, 0, 16, 16, 3, 75, 0, 0), bpp=4) == 0
    for ri in (1, 7, 65535, -1):
        assert check(job=(0, 0, 16, 16, 0, 75, ri, 0)) == INVALID                            # restart intervals are out of scope
    assert check(n=0) == INVALID and check(bpp=2) == INVALID
    assert check(job=(0, 0, 16, 16, 1, 75, 0, 0)) == INVALID and check(job=(0, 0, 16, 16, 0, 75, 0, 0), bpp=4) == INVALID      # gray and colour do not mix
    assert check(job=(0, 0, 16, 16, 4, 75, 0, 0)) == INVALID and check(job=(0, 0, 16, 16, 0, 0, 0, 0)) == INVALID
    assert check(job=(0, 0, 16, 16, 0, 101, 0, 0)) == INVALID and check(job=(0, 0, 16, 16, 0, 75, 0, 1)) == INVALID
    assert check(job=(250, 0, 16, 16, 0, 75, 0, 0)) == INVALID and check(job=(0, 60, 16, 16, 0, 75, 0, 0)) == INVALID
    assert check(job=(0, 0, 0, 16, 0, 75, 0, 0)) == INVALID and check(cap=-1) == INVALID
    assert check(dst=surf.ctypes.data + 100, cap=64) == INVALID                              # a file over its own source
    assert check(out=(0, 256, 256, 64)) == INVALID
    wide, below = (surf.ctypes.data, 65536, 65535, 65535), surf.ctypes.data - (1 << 20)       # (never followed; the file lies in front of the surface)
    assert check(job=(0, 0, 25000, 40000, 0, 75, 0, 0), out=wide, dst=below) == 0                       # 15,625,000 blocks: the most
    assert check(job=(0, 0, 25000, 40001, 0, 75, 0, 0), out=wide, dst=below) == UNSUPPORTED


def test_sanitizers():
    """tests/hostsim/encode_prog_main.cpp: a program of its own (make encodeprogasan), nothing preloaded"""
    subprocess.run(["make", "encodeprogasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "encode_prog_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"encode_prog_asan ok" in r.stdout, r.stdout[-2000:]
