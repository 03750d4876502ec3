"""JDA_ENCODE_OPTIMIZE (jda_encode_surfaces_ex) without a GPU.  Every comparison is exact equality.

* the Python twin (tests/encode_opt_util.py: a port of libjpeg's jpeg_gen_optimal_table over the symbols of tests/encode_util.py's
  coefficients) = Pillow's Image.save(optimize=True): the DHT segments in the file's order and the bytes behind the SOS header, over
  encode_util.SIZES x samplings x seven pictures x intervals 0, 1, 3 -- Pillow saves every one of them, none is skipped -- and over the
  larger jobs of the edges, where Pillow's own output buffer (max(65536, w h) bytes, 2 w h from quality 95 up) may refuse the file: then
  the twin stands alone, and the test asserts that the file really is larger than that buffer;
* jda_encode_optimal_table = the port, on the grid's histograms, 1,000 random ones, one symbol, and counts without ties that pass 16 bits
  before the lengths are limited (asserted from the port: the folding loop runs);
* gather and the second lengths pass, lane by lane through the kernels' own code (tests/hostsim/huffopt_sim.cpp over jda_ho_* of
  jda_device_core.h), and the whole nine-stage call: histograms, code lengths and files against the twin, for the grid and the edges of
  encode_opt_util.edge_cases, optimised and standard jobs in one call;
* the refusals; NULL flags = the standard twin; jda_encode_bound holds for the optimised files of the noisiest and the emptiest jobs;
* the plan, the table builder and the simulator once more as a program under AddressSanitizer + UBSan (nothing is preloaded)."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from tests import coef_jpeg
from tests import encode_util as E
from tests import encode_opt_util as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, MEMORY = 1, 3, 5
GUARD = 0x5A
OPTIMIZE = 1


class Output(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("pitch_bytes", C.c_int32), ("width_px", C.c_int32), ("rows", C.c_int32)]


class Job(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("x", "y", "w", "h", "sampling", "quality", "restart_interval", "reserved")]


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_huffoptsim.so"))
    lib.huffoptsim_lanes.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(Job), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.huffoptsim_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    lib.huffoptsim_check.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(Job), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.encodesim_bound.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int64)]
    return lib


def bound(sim, w, h, sampling, ri):
    b = C.c_int64()
    assert sim.encodesim_bound(w, h, E.SAMPLING_ID[sampling], ri, C.byref(b)) == 0
    return b.value


def blocks_of(img, sampling):
    return sum(r * c for r, c in coef_jpeg.geometry(img.shape[1], img.shape[0], sampling)[2])


def run_sim(sim, cases, caps=None, no_flags=False):
    """cases: [(img, sampling, quality, ri, flag)] of ONE pixel size.  The rectangles sit at (3, 2) of guard-filled surfaces, the files back to
    back in one guard-filled block (capacity: jda_encode_bound unless given).  -> (files or None, sizes, statuses, per case dict(code, hist))"""
    n = len(cases)
    bpp = 1 if cases[0][1] == "gray" else 4
    surfs, outs, jobs = [], (Output * n)(), (Job * n)()
    for i, (img, sampling, q, ri, flag) in enumerate(cases):
        h, w = img.shape[:2]
        s = np.full((h + 5, (w + 7) * bpp + 4 - (w + 7) * bpp % 4), GUARD, dtype=np.uint8)
        s[2:2 + h, 3 * bpp:(3 + w) * bpp] = img.reshape(h, w * bpp)
        surfs.append(s)
        outs[i] = Output(s.ctypes.data, s.shape[1], w + 7, h + 5)
        jobs[i] = Job(3, 2, w, h, E.SAMPLING_ID[sampling], q, ri, 0)
    flags = np.asarray([c[4] for c in cases], dtype=np.uint32)
    if caps is None:
        caps = [bound(sim, c[0].shape[1], c[0].shape[0], c[1], c[3]) for c in cases]
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    block = np.full(int(offs[-1]) + 16, GUARD, dtype=np.uint8)
    dst = (C.c_void_p * n)(*[block.ctypes.data + int(o) for o in offs[:-1]])
    cap = (C.c_int64 * n)(*caps)
    nbytes, status = (C.c_int64 * n)(), (C.c_int32 * n)()
    nb = sum(blocks_of(c[0], c[1]) for c in cases)
    n_opt = 0 if no_flags else int(flags.sum())
    code, hist, info = np.zeros(nb, dtype=np.uint32), np.full((max(n_opt, 1), O.HUFF_DWORDS), 0xEEEEEEEE, dtype=np.uint32), np.zeros(5, dtype=np.uint64)
    rc = sim.huffoptsim_lanes(n, outs, bpp, jobs, None if no_flags else flags.ctypes.data, dst, cap, nbytes, status, None, code.ctypes.data, None, hist.ctypes.data,
                              info.ctypes.data)
    assert rc == 0, rc
    assert int(info[0]) == nb and int(info[4]) == n_opt
    files, per, b0, k = [], [], 0, 0
    for i, c in enumerate(cases):
        o = int(offs[i])
        if status[i] == 0:
            files.append(block[o:o + nbytes[i]].tobytes())
            assert np.all(block[o + nbytes[i]:o + caps[i]] == GUARD)
        else:
            files.append(None)
            assert np.all(block[o:o + caps[i]] == GUARD)
        nblk = blocks_of(c[0], c[1])
        per.append(dict(code=code[b0:b0 + nblk], hist=hist[k] if c[4] and not no_flags else None))
        b0 += nblk
        k += 1 if c[4] and not no_flags else 0
    assert np.all(block[int(offs[-1]):] == GUARD)
    return files, list(nbytes), list(status), per


def twin_hist(img, sampling, q, ri):
    h, w = img.shape[:2]
    return O.hist544(O.histograms(w, h, sampling, E.coefficients(img, sampling, q), ri))


def check_case(got_file, got, case):
    """the histogram (an optimised job), the code lengths behind the second lengths pass and the file, against the twin"""
    img, sampling, q, ri, flag = case
    jpeg, lay = O.twin(*case)
    if flag:
        assert np.array_equal(got["hist"], twin_hist(img, sampling, q, ri)), "histogram"
    else:
        assert got["hist"] is None
    want = [ln + s + sum(l + max(m, 0) for _, l, m in syms) for c, by, bx, (p, ln, s), syms in lay["blocks"]]
    assert np.array_equal((got["code"] & 0xFFFF).astype(np.int64), want), "code lengths"
    assert got_file == jpeg, "file"


# ---- the twin against Pillow -------------------------------------------------------------------------------------------------------
def pillow_file(img, sampling, q, ri):
    from PIL import Image
    im = Image.fromarray(img) if sampling == "gray" else Image.fromarray(np.ascontiguousarray(img[..., :3]))
    kw = {} if sampling == "gray" else dict(subsampling=E.PILLOW_SUBSAMPLING[sampling])
    if ri:
        kw["restart_marker_blocks"] = ri
    b = io.BytesIO()
    im.save(b, "JPEG", quality=q, optimize=True, **kw)
    return b.getvalue()


def body(jpeg):
    return jpeg[coef_jpeg._parse(jpeg)[5]:]


def same_as_pillow(mine, img, sampling, q, ri):
    theirs = pillow_file(img, sampling, q, ri)
    assert O.dht_segments(mine) == O.dht_segments(theirs), "the DHT segments, in the file's order"
    assert body(mine) == body(theirs), "the bytes behind the SOS header"


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_twin_is_pillow_over_the_grid(sampling):
    pytest.importorskip("PIL")
    n = 0
    for w, h in E.SIZES:
        for kind, q in O.PILLOW_PICTURES:
            img = E.picture(kind, w, h, sampling)
            for ri in O.PILLOW_INTERVALS:
                same_as_pillow(O.file_bytes_opt(img, sampling, q, ri), img, sampling, q, ri)      # (Pillow saves every one: none is skipped)
                n += 1
    assert n == len(E.SIZES) * 7 * 3
    # the order of the segments: a table after the other, DC then AC
    segs = [s[0] for s in O.dht_segments(O.file_bytes_opt(E.picture("noise", 17, 9, sampling), sampling, 75))]
    assert segs == ([0x00, 0x10] if sampling == "gray" else [0x00, 0x10, 0x01, 0x11])


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_twin_is_pillow_over_the_edges_where_pillow_saves(sampling_class):
    """the optimised jobs of the edges: Pillow's file where Pillow saves one; where it refuses ("Suspension not allowed here"), the file must
    be larger than Pillow's output buffer -- max(65536, w h) bytes, 2 w h from quality 95 up -- and the twin stands alone"""
    pytest.importorskip("PIL")
    pytest.importorskip("PIL")
    saved = 0
    refused = 0
    extra = [(E.picture("noise", 264, 240, "4:4:4"), "4:4:4", 75, 0, 1)] if sampling_class == "colour" else []      # 72,748 bytes: past the 65,536 of the buffer
    for img, sampling, q, ri, flag in O.edge_cases(sampling_class) + extra:
        if not flag:
            continue
        mine = O.twin(img, sampling, q, ri, 1)[0]
        h, w = img.shape[:2]
        try:
            same_as_pillow(mine, img, sampling, q, ri)
            saved += 1
        except OSError:                        # ("broken data stream when writing image file"; libjpeg prints "Suspension not allowed here")
            refused += 1
            assert len(mine) > (2 * w * h if q >= 95 else max(65536, w * h)), (w, h, sampling, q, len(mine))
    assert saved >= 8 and refused == len(extra)


# ---- the table function against the port ---------------------------------------------------------------------------------------------
def product_table(sim, freq):
    f = np.zeros(256, dtype=np.uint32)
    f[:len(freq)] = freq
    bits, vals, n = np.zeros(16, dtype=np.uint8), np.zeros(256, dtype=np.uint8), C.c_uint32()
    assert sim.huffoptsim_table(f.ctypes.data, bits.ctypes.data, vals.ctypes.data, C.byref(n)) == 0
    return bits.tolist(), vals[:n.value].tolist()


def strict_counts(n):
    """a(k) = a(k-1) + a(k-2) + 1: no two sums tie, so the tree is a chain and the longest code has n bits"""
    out, a, b = [], 1, 2
    for _ in range(n):
        out.append(a)
        a, b = b, a + b + 1
    return out


def test_table_function_is_the_port(sim):
    # the grid's own histograms
    n = 0
    for sampling in E.SAMPLINGS:
        for w, h in ((1, 1), (17, 9), (33, 47), (129, 65)):
            for kind, q in O.PILLOW_PICTURES:
                img = E.picture(kind, w, h, sampling)
                for key, f in O.histograms(w, h, sampling, E.coefficients(img, sampling, q), 1).items():
                    assert product_table(sim, f) == tuple(O.optimal_table(f)[:2]), (sampling, w, h, kind, q, key)
                    n += 1
    assert n == (2 + 3 * 4) * 4 * 7
    # 1,000 random histograms of 1 .. 162 symbols: small counts (many ties), large ones, mixed
    rng = np.random.RandomState(7)
    over = 0
    for k in range(1000):
        f = np.zeros(256, dtype=np.int64)
        syms = rng.choice(256, size=rng.randint(1, 163), replace=False)
        f[syms] = rng.randint(1, (4, 100, 1 << 20)[k % 3], size=len(syms)) if k % 5 else (1 << rng.randint(0, 20, size=len(syms)))
        want = O.optimal_table(f)
        over += want[2] > 16
        assert product_table(sim, f) == tuple(want[:2]), k
    assert over > 0
    # one symbol: a code of one bit
    f = np.zeros(256, dtype=np.int64)
    f[0x35] = 9
    assert product_table(sim, f) == ([1] + [0] * 15, [0x35]) == tuple(O.optimal_table(f)[:2])
    # counts without ties over 30 and 32 symbols: lengths above 16 before limiting, the folding loop runs -- asserted from the port
    for n_sym in (30, 32):
        f = np.zeros(256, dtype=np.int64)
        f[np.arange(n_sym) * 7] = strict_counts(n_sym)
        want = O.optimal_table(f)
        assert want[2] == n_sym > 16 and max(i + 1 for i, b in enumerate(want[0]) if b) == 16
        assert product_table(sim, f) == tuple(want[:2])
    # .. and past 32 bits libjpeg gives up; so does the function
    f = np.zeros(256, dtype=np.uint32)
    f[:34] = strict_counts(34)
    assert f.sum() < O.START
    bits, vals, n = np.zeros(16, dtype=np.uint8), np.zeros(256, dtype=np.uint8), C.c_uint32()
    assert sim.huffoptsim_table(f.ctypes.data, bits.ctypes.data, vals.ctypes.data, C.byref(n)) == 1
    with pytest.raises(AssertionError):
        O.optimal_table(f)


# ---- gather and the second lengths pass, lane by lane, and the whole call -----------------------------------------------------------------------
@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_lanes_are_the_twin_over_the_grid(sim, sampling):
    cases = O.grid_cases(sampling)
    assert {c[4] for c in cases} == {0, 1} and {c[3] for c in cases} >= {0, 1, 3}
    files, nbytes, status, per = run_sim(sim, cases)                                                # one call: optimised and standard jobs
    for f, st, got, case in zip(files, status, per, cases):
        assert st == 0
        check_case(f, got, case)


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_lanes_are_the_twin_over_the_edges(sim, sampling_class):
    cases = O.edge_cases(sampling_class)
    # what the list is there for, from the cases and the twin alone
    nblk = [blocks_of(c[0], c[1]) for c in cases]
    start = np.concatenate([[0], np.cumsum(nblk)])
    assert any(s % 64 and (s + nblk[i]) % 64 and cases[i][0].shape[:2] == (1, 1) for i, s in enumerate(start[:-1]))      # a 1 x 1 job that begins and ends inside a wavefront
    assert any(a[4] != b[4] for a, b in zip(cases, cases[1:])) and {c[4] for c in cases} == {0, 1}
    assert any(c[4] and c[3] == 1 for c in cases)                                                                    # an interval every MCU
    if sampling_class == "gray":
        assert any(c[4] and n == 990 for c, n in zip(cases, nblk)) and any(c[4] and n == 257 for c, n in zip(cases, nblk))
        zrl = [c for c in cases if c[2] == E.ZRL_QUALITY][0]
        h = twin_hist(*zrl[:4])
        assert h[0xF0] == 0 + 1 + 1 + 2 + 2 + 3 + 3 and h[0x00] == 6                                                   # ZRLs of runs 15 .. 62; the last block has no EOB
        flat = [c for c in cases if c[4] and c[0].shape == (1, 1) and c[0][0, 0] == 200 and c[2] == 75][0]
        assert [s[1] for s in O.dht_segments(O.twin(*flat)[0])] == [[1] + [0] * 15] * 2                              # one symbol a table, a code of one bit
    else:
        assert any(c[4] and c[1] == s and c[0].shape[:2] == hw for s in ("4:2:0", "4:2:2") for hw in ((9, 17), (16, 25)) for c in cases)
        top = [c for c in cases if c[4] and c[2] == 100 and c[0].shape[:2] == (47, 33)]
        hs = [twin_hist(*c[:4]) for c in top]
        assert any(h[512 + 11] for h in hs) and any(h[:512].reshape(2, 256)[:, 10::16].any() for h in hs)                                              # DC category 11, AC category 10
        assert any(c[4] and n > 256 for c, n in zip(cases, nblk))
    files, nbytes, status, per = run_sim(sim, cases)
    for f, st, got, case in zip(files, status, per, cases):
        assert st == 0
        check_case(f, got, case)
    # the same call twice: the same files (nothing of a call stays behind)
    assert run_sim(sim, cases)[0] == files


def test_null_flags_and_zero_flags_are_the_standard_call(sim):
    cases = [(E.picture("noise", 33, 47, "4:2:0", s), "4:2:0", 75, ri, 0) for s, ri in ((1, 0), (2, 3))] + [(E.picture("flat", 1, 1, "4:2:0"), "4:2:0", 50, 0, 0)]
    want = [E.file_bytes(*c[:4]) for c in cases]
    assert run_sim(sim, cases, no_flags=True)[0] == want
    assert run_sim(sim, cases)[0] == want


def test_capacity_between_the_two_sizes(sim):
    """an optimised job whose capacity is the STANDARD file's size minus one succeeds; its neighbour, a byte short of its optimised size, does not"""
    cases = [(E.picture("noise", 33, 47, "4:2:0", s), "4:2:0", 75, ri, 1) for s, ri in ((1, 0), (2, 3), (3, 1))]
    std = [len(E.file_bytes(*c[:4])) for c in cases]
    opt = [len(O.twin(*c)[0]) for c in cases]
    assert all(o < s - 1 for o, s in zip(opt, std))
    files, nbytes, status, per = run_sim(sim, cases, caps=[std[0] - 1, opt[1] - 1, opt[2]])
    assert status == [0, MEMORY, 0] and nbytes == opt
    assert files[0] == O.twin(*cases[0])[0] and files[1] is None and files[2] == O.twin(*cases[2])[0]


def test_bound_holds_for_optimised_files(sim):
    """jda_encode_bound is unchanged: the noisiest (quality 100) and the emptiest (quality 1) jobs of the grid"""
    for sampling in E.SAMPLINGS:
        for w, h in E.SIZES:
            for q in (100, 1):
                for ri in (0, 1):
                    size = len(O.file_bytes_opt(E.picture("noise", w, h, sampling), sampling, q, ri))
                    assert size <= bound(sim, w, h, sampling, ri), (sampling, w, h, q, ri)


def test_refusals(sim):
    mem = np.zeros(4096 + 64 * 256, dtype=np.uint8)          # dst in FRONT of surf: the source range `wide` claims below runs 2.6 GB on from surf and must not cover dst
    dst, surf = mem[:4096], mem[4096:].reshape(64, 256)

    def check(flags, n=1, job=(0, 0, 16, 16, 3, 75, 0, 0), out=None, bpp=4):
        o = (Output * max(n, 1))(*[Output(*(out or (surf.ctypes.data, 256, 64, 64)))] * max(n, 1))
        j = (Job * max(n, 1))(*[Job(*job)] * max(n, 1))
        dd = (C.c_void_p * max(n, 1))(*[dst.ctypes.data + 1024 * i for i in range(max(n, 1))])
        cc = (C.c_int64 * max(n, 1))(*[1024] * max(n, 1))
        f = None if flags is None else np.asarray(flags, dtype=np.uint32)
        return sim.huffoptsim_check(n, o, bpp, j, None if f is None else f.ctypes.data, dd, cc)

    assert check(None) == 0 and check([0]) == 0 and check([OPTIMIZE]) == 0 and check([0, OPTIMIZE, 0], n=3) == 0
    for bad in (2, 3, 4, 0x80000000, 0x80000001, 0xFFFFFFFF):
        assert check([bad]) == INVALID, bad
        assert check([OPTIMIZE, bad], n=2) == INVALID, bad
    assert check([OPTIMIZE], job=(0, 0, 16, 16, 3, 75, 0, 1)) == INVALID                    # reserved is still 0
    assert check([OPTIMIZE], n=0) == INVALID and check(None, n=0) == INVALID               # (n == 0 never reaches the plan: the call returns before it)
    # the block cap: 3125 x 5000 = 15,625,000 gray blocks are taken, a block row more is refused -- and taken again without the flag
    wide = (surf.ctypes.data, 65536, 65535, 65535)                                         # (never followed)
    assert check([OPTIMIZE], job=(0, 0, 25000, 40000, 0, 75, 0, 0), out=wide, bpp=1) == 0
    assert check([OPTIMIZE], job=(0, 0, 25000, 40001, 0, 75, 0, 0), out=wide, bpp=1) == UNSUPPORTED
    assert check([0], job=(0, 0, 25000, 40001, 0, 75, 0, 0), out=wide, bpp=1) == 0
    assert check(None, job=(0, 0, 25000, 40001, 0, 75, 0, 0), out=wide, bpp=1) == 0
    assert 3125 * 5000 == O.OPT_MAX_BLOCKS and O.OPT_MAX_BLOCKS * 64 == O.START


def test_plan_tables_and_lanes_under_the_sanitizers(built_checkers):
    """tests/hostsim/huffopt_main.cpp: a program of its own (make huffoptasan), nothing preloaded"""
    subprocess.run(["make", "huffoptasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "huffopt_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"huffopt_asan ok" in r.stdout, r.stdout[-2000:]


def test_exports():
    import inspect

    import jpegdec_amd as J
    assert J.ENCODE_OPTIMIZE == 1
    assert "flags" in inspect.signature(J.encode_surfaces).parameters
    assert "optimize" in inspect.signature(J.transcode_to_host).parameters and "optimize" in inspect.signature(J.thumbnails).parameters
