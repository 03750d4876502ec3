"""jda_encode_surfaces without a GPU.  Every comparison is exact equality.

* the numpy twin (tests/encode_util.py) = Pillow's Image.save(quality, subsampling, optimize=False, restart_marker_blocks): quantisers and
  coefficients (through tests/coef_jpeg.decode_coefs) for every quality on one image, the bytes behind the SOS header over the grid, and
  Pillow opens the twin's files (skipped where Pillow is absent);
* the six stages, lane by lane through the kernels' own code over the host plan's records (tests/hostsim/encode_sim.cpp over jda_en_* of
  jda_device_core.h), against the twin: coefficients, code lengths, bit positions and the file, for the grid, for one width per sampling
  that makes a row of more than 64 blocks, for the edges of the design and for zero runs of 15 .. 62, each asserted FROM THE TWIN to be in
  the input;
* the scan stage alone over lengths of the test's own against positions counted one after the other: runs of a lane with no, one, two and
  more interval starts, empty runs, positions past 2^32; and the long jobs of encode_util.LONG_JOBS through all six stages -- several
  interval starts in a lane's run, three and more chunks a lane, dwords that the blocks of two wavefronts and workgroups share;
* the reciprocal division, every divisor against every numerator; the header; every refusal; the capacity rule; jda_encode_bound;
* the plan, the header builder and the simulator once more as a program under AddressSanitizer + UBSan."""
import ctypes as C
import functools
import io
import os
import subprocess

import numpy as np
import pytest

from tests import coef_jpeg
from tests import encode_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, MEMORY = 1, 5
GUARD = 0x5A


class Output(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("pitch_bytes", C.c_int32), ("width_px", C.c_int32), ("rows", C.c_int32)]


class Job(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("x", "y", "w", "h", "sampling", "quality", "restart_interval", "reserved")]


@pytest.fixture(scope="module")
def sim(built_checkers):
    lib = C.CDLL(os.path.join(ROOT, "tests", "hostsim", "libjda_encodesim.so"))
    lib.encodesim_lanes.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(Job), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.encodesim_coefs.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.encodesim_check.argtypes = [C.c_int, C.POINTER(Output), C.c_int, C.POINTER(Job), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.encodesim_bound.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int64)]
    lib.encodesim_header.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int]
    lib.encodesim_divide.restype = C.c_int64
    lib.encodesim_scan.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    return lib


def bound(sim, w, h, sampling, ri):
    b = C.c_int64()
    assert sim.encodesim_bound(w, h, E.SAMPLING_ID[sampling], ri, C.byref(b)) == 0
    return b.value


def run_sim(sim, cases, caps=None):
    """cases: [(img, sampling, quality, ri)], ONE sampling class (gray or colour) a call.  The rectangles sit at (3, 2) of guard-filled
    surfaces with extra pitch and rows, the files back to back in one guard-filled block.  -> (files or None where the capacity was too
    small, dst_bytes, status, per-case dict(coef, code, end))"""
    n = len(cases)
    bpp = 1 if cases[0][1] == "gray" else 4
    surfs, outs, jobs = [], (Output * n)(), (Job * n)()
    for i, (img, sampling, q, ri) in enumerate(cases):
        h, w = img.shape[:2]
        s = np.full((h + 5, (w + 7) * bpp + 4 - (w + 7) * bpp % 4), GUARD, dtype=np.uint8)
        s[2:2 + h, 3 * bpp:(3 + w) * bpp] = img.reshape(h, w * bpp)
        surfs.append(s)
        outs[i] = Output(s.ctypes.data, s.shape[1], w + 7, h + 5)
        jobs[i] = Job(3, 2, w, h, E.SAMPLING_ID[sampling], q, ri, 0)
    if caps is None:
        caps = [bound(sim, img.shape[1], img.shape[0], s, ri) for img, s, q, ri in cases]
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    block = np.full(int(offs[-1]) + 16, GUARD, dtype=np.uint8)
    dst = (C.c_void_p * n)(*[block.ctypes.data + int(o) for o in offs[:-1]])
    cap = (C.c_int64 * n)(*caps)
    nbytes, status = (C.c_int64 * n)(), (C.c_int32 * n)()
    nb = sum(sum(r * c for r, c in coef_jpeg.geometry(img.shape[1], img.shape[0], s)[2]) for img, s, q, ri in cases)
    coef, code, end = np.zeros((nb, 64), dtype=np.int16), np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint64)
    info = np.zeros(4, dtype=np.uint64)
    rc = sim.encodesim_lanes(n, outs, bpp, jobs, dst, cap, nbytes, status, coef.ctypes.data, code.ctypes.data, end.ctypes.data, None, None, 0, info.ctypes.data)
    assert rc == 0, rc
    assert int(info[0]) == nb
    files, per, b0 = [], [], 0
    for i, (img, s, q, ri) in enumerate(cases):
        o = int(offs[i])
        if status[i] == 0:
            files.append(block[o:o + nbytes[i]].tobytes())
            assert np.all(block[o + nbytes[i]:o + caps[i]] == GUARD)
        else:
            files.append(None)
            assert np.all(block[o:o + caps[i]] == GUARD)
        k = sum(r * c for r, c in coef_jpeg.geometry(img.shape[1], img.shape[0], s)[2])
        per.append(dict(coef=coef[b0:b0 + k], code=code[b0:b0 + k], end=end[b0:b0 + k]))
        b0 += k
    assert np.all(block[int(offs[-1]):] == GUARD)
    return files, list(nbytes), list(status), per


_TWINS = {}


def twin_layout(img, sampling, q, ri):
    """the twin's file, and per block in the order of the scan (coefficients, first bit, code bits) in the unstuffed scan (computed once a case)"""
    key = (img.shape, img.tobytes(), sampling, q, ri)
    if key not in _TWINS:
        _TWINS[key] = _twin_layout(img, sampling, q, ri)
    return _TWINS[key]


def _twin_layout(img, sampling, q, ri):
    coefs = E.coefficients(img, sampling, q)
    jpeg, lay = E.file_bytes(img, sampling, q, ri, return_layout=True)
    rows = []
    for c, by, bx, (p, ln, s), syms in lay["blocks"]:
        rows.append((coefs[c][by, bx], p, ln + s + sum(l + max(m, 0) for _, l, m in syms)))
    return jpeg, rows, lay


def check_case(got_file, got, img, sampling, q, ri):
    jpeg, rows, lay = twin_layout(img, sampling, q, ri)
    assert len(rows) == len(got["code"])
    want_coef = np.stack([r[0] for r in rows])
    assert np.array_equal(got["coef"].astype(np.int64), want_coef), "coefficients"
    bits = (got["code"] & 0xFFFF).astype(np.int64)
    assert np.array_equal(bits, np.asarray([r[2] for r in rows])), "code lengths"
    assert np.array_equal(got["end"].astype(np.int64) - bits, np.asarray([r[1] for r in rows])), "bit positions"
    assert got_file == jpeg, "file"
    return jpeg, rows, lay


# ---- the twin against Pillow -------------------------------------------------------------------------------------------------------
def pillow_file(img, sampling, q, ri):
    from PIL import Image
    im = Image.fromarray(img) if sampling == "gray" else Image.fromarray(np.ascontiguousarray(img[..., :3]))
    kw = {} if sampling == "gray" else dict(subsampling=E.PILLOW_SUBSAMPLING[sampling])
    if ri:
        kw["restart_marker_blocks"] = ri
    b = io.BytesIO()
    im.save(b, "JPEG", quality=q, optimize=False, **kw)
    return b.getvalue()


def body(jpeg):
    return jpeg[coef_jpeg._parse(jpeg)[5]:]


GRID_PICTURES = (("noise", 75), ("smooth", 30), ("pixels", 100), ("blocks", 100))


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_twin_is_pillow_every_quality(sampling):
    pytest.importorskip("PIL")
    img = E.picture("noise", 25, 16, sampling, seed=3)
    for q in range(1, 101):
        dec = coef_jpeg.decode_coefs(pillow_file(img, sampling, q, 0))
        assert dec["quant"] == E.quant_tables(q, sampling), q
        for a, b in zip(dec["coefs"], E.coefficients(img, sampling, q)):
            assert np.array_equal(a, b), q


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_twin_is_pillow_over_the_grid(sampling):
    pytest.importorskip("PIL")
    from PIL import Image
    for w, h in E.SIZES:
        for kind, q in GRID_PICTURES:
            img = E.picture(kind, w, h, sampling)
            for ri in E.restart_intervals(w, h, sampling):
                mine = E.file_bytes(img, sampling, q, ri)
                assert body(mine) == body(pillow_file(img, sampling, q, ri)), (w, h, kind, q, ri)
                if ri in (0, 3):
                    back = Image.open(io.BytesIO(mine))
                    back.load()
                    assert back.size == (w, h)
    # more than eight intervals: RSTm wraps
    img = E.picture("noise", 129, 65, sampling, seed=5)
    mine = E.file_bytes(img, sampling, 75, 2)
    assert mine.count(b"\xff\xd0") >= 2 and body(mine) == body(pillow_file(img, sampling, 75, 2))
    if sampling == "4:2:0":
        # the checkerboards reach the ends of the tables: AC category 10, DC differences of category 11
        dec = coef_jpeg.decode_coefs(E.file_bytes(E.picture("pixels", 33, 47, sampling), sampling, 100))
        assert 0x0A in {s & 15 for s in dec["hist"][(1, 0)]}
        dec = coef_jpeg.decode_coefs(E.file_bytes(E.picture("blocks", 33, 47, sampling), sampling, 100))
        assert 11 in dec["hist"][(0, 0)]


# ---- the stages, lane by lane, against the twin -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_lanes_are_the_twin_over_the_grid(sim, sampling):
    for kind, q in GRID_PICTURES:
        cases = []
        for w, h in E.SIZES:
            img = E.picture(kind, w, h, sampling)
            ris = E.restart_intervals(w, h, sampling) if kind == "noise" else [0, 3]
            cases += [(img, sampling, q, ri) for ri in ris]
        if kind == "noise":
            cases.append((E.picture("noise", 129, 65, sampling, seed=5), sampling, 75, 2))          # RSTm wraps
        files, nbytes, status, per = run_sim(sim, cases)                                           # one call: a batch of jobs
        for f, st, got, case in zip(files, status, per, cases):
            assert st == 0
            check_case(f, got, *case)


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_lanes_second_tile_in_an_mcu_row(sim, sampling):
    w = E.SECOND_TILE_WIDTH[sampling]
    cx, cy, shapes, (hs, vs) = coef_jpeg.geometry(w, 9, sampling)
    assert cx * (1 if sampling == "gray" else hs * vs + 2) > 64             # the blocks of an MCU row
    cases = [(E.picture("noise", w, 9, sampling, seed=2), sampling, 90, ri) for ri in (0, 5)]
    files, nbytes, status, per = run_sim(sim, cases)
    for f, got, case in zip(files, per, cases):
        check_case(f, got, *case)


# ---- the scan stage alone, over lengths of the test's own -------------------------------------------------------------------------------------
LANES = 256


def scan_serial(vals, mask, period, intervals):
    """the positions, one element after the other: (end, istart in bytes, the position behind the last element)"""
    p, end, istart = 0, [], []
    for i, v in enumerate(vals.tolist()):
        if intervals and (i == 0 or (period and i % period == 0)):
            p = (p + 7) & ~7
            istart.append(p // 8)
        p += v & mask
        end.append(p)
    return np.asarray(end, dtype=np.uint64), np.asarray(istart, dtype=np.uint64), p


def scan_numpy(vals, mask, period, intervals):
    """the same without a loop: an interval starts on a byte, so ceil8(start + its bits) = start + ceil8(its bits)"""
    ln = (vals & np.uint32(mask)).astype(np.uint64)
    n = len(ln)
    if not intervals:
        end = np.cumsum(ln, dtype=np.uint64)
        return end, np.zeros(0, dtype=np.uint64), int(end[-1])
    k = period or n
    pad = np.concatenate([ln, np.zeros(-n % k, dtype=np.uint64)]).reshape(-1, k)
    within = np.cumsum(pad, axis=1, dtype=np.uint64)
    start = np.concatenate([[0], np.cumsum((within[:-1, -1] + np.uint64(7)) & ~np.uint64(7), dtype=np.uint64)]).astype(np.uint64)
    end = (within + start[:, None]).reshape(-1)[:n]
    return end, start >> np.uint64(3), int(end[-1])


def run_scan(sim, vals, bytes_mode, period):
    n = len(vals)
    end = np.zeros(n, dtype=np.uint64)
    istart = np.zeros(1 if bytes_mode else (-(-n // period) if period else 1), dtype=np.uint64)
    total = C.c_uint64(~0)
    rc = sim.encodesim_scan(vals.ctypes.data, n, int(bytes_mode), period, end.ctypes.data, istart.ctypes.data, C.byref(total))
    assert rc == 0, rc
    return end, (istart[:0] if bytes_mode else istart), total.value


def runs_of(n, period):
    """what the lanes' runs of per = ceil(n / 256) elements hold, from n and the period alone: the interval starts in every run that has an
    element, whether a run behind the first begins on a start, whether empty runs follow a run that is not full"""
    per = -(-n // LANES)
    first = np.zeros(n, dtype=np.int64)
    first[0] = 1
    if period:
        first[::period] = 1
    bounds = [(min(t * per, n), min(t * per + per, n)) for t in range(LANES)]
    counts = {int(first[a:b].sum()) for a, b in bounds if a < b}
    on_start = any(0 < a < b and first[a] for a, b in bounds)
    ragged = any(0 < b - a < per and bounds[t + 1][0] == bounds[t + 1][1] for t, (a, b) in enumerate(bounds[:-1]))
    return per, counts, on_start, ragged


def scan_lengths(kind, n, rng):
    if kind == "random":                      # 2 .. 1665 bits, and garbage above bit 15 that the mask of the blocks' scan takes off
        return (rng.randint(2, 1666, size=n).astype(np.uint32) | (rng.randint(0, 1 << 16, size=n).astype(np.uint32) << np.uint32(16))).astype(np.uint32)
    if kind == "bytes":                       # every element ends on a byte
        return (8 * rng.randint(1, 209, size=n)).astype(np.uint32)
    if kind == "odd":                         # every element one bit past a byte
        return (8 * rng.randint(0, 208, size=n) + 1).astype(np.uint32)
    return np.full(n, 1665, dtype=np.uint32)  # JDA_EN_BLOCK_BITS, the longest


SCAN_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 769, 1000, 4097)


def test_scan_runs_with_many_interval_starts(sim):
    """jda_en_scan_local / jda_en_scan_write over lengths of the test's own (encodesim_scan; the second half's lanes in reverse order), against
    positions counted one element after the other.  per = ceil(n / 256) elements a lane, an interval every `period`: the grid holds -- asserted
    from n and the period alone -- runs with 0, 1, 2 and more interval starts, a run that begins on a start, and empty runs behind a partly
    filled one; the blocks' scan takes only the low 16 bits of a value, the chunks' scan all of them."""
    rng = np.random.RandomState(5)
    seen, begins, ragged = set(), False, False
    for n in SCAN_SIZES:
        per = -(-n // LANES)
        for period in sorted({0, 1, 2, 3, per - 1, per, per + 1, 2 * per + 1, n - 1, n, n + 1} - {-1}):
            if period < 0:
                continue
            _, counts, b, r = runs_of(n, period)
            seen |= {min(c, 3) for c in counts}
            begins, ragged = begins or b, ragged or r
            for kind in ("random", "bytes", "odd", "longest"):
                vals = scan_lengths(kind, n, rng)
                want = scan_serial(vals, 0xFFFF, period, True)
                fast = scan_numpy(vals, 0xFFFF, period, True)
                assert all(np.array_equal(a, b) for a, b in zip(want[:2], fast[:2])) and want[2] == fast[2]
                end, istart, total = run_scan(sim, vals, False, period)
                where = (n, period, kind)
                assert np.array_equal(istart, want[1]), where
                assert np.array_equal(end, want[0]), where
                assert total == (want[2] + 7) // 8, where
        vals = rng.randint(0, 65, size=n).astype(np.uint32)                      # the 0xFF bytes of 64-byte chunks
        vals[rng.randint(0, n)] |= np.uint32(1 << 20)                            # (no mask here: a high bit counts)
        want = scan_serial(vals, 0xFFFFFFFF, 0, False)
        end, istart, total = run_scan(sim, vals, True, 0)
        assert np.array_equal(end, want[0]) and total == want[2] and np.array_equal(end, scan_numpy(vals, 0xFFFFFFFF, 0, False)[0]), n
    assert seen == {0, 1, 2, 3} and begins and ragged
    assert runs_of(257, 0)[3] and -(-257 // LANES) == 2                          # lane 128 holds one element, the lanes behind it none


def test_scan_positions_past_32_bits(sim):
    """about 2.6 M blocks of the longest code, an interval every 7: the positions pass 2^32 bits (the reference: numpy in 64 bits)"""
    n = 2_600_000
    vals = np.full(n, 1665, dtype=np.uint32)
    want_end, want_istart, last = scan_numpy(vals, 0xFFFF, 7, True)
    assert last > 1 << 32 and int(want_end[n // 2]) < 1 << 32 and min(runs_of(n, 7)[1]) > 1000
    end, istart, total = run_scan(sim, vals, False, 7)
    assert np.array_equal(istart, want_istart) and np.array_equal(end, want_end) and total == (last + 7) // 8


# ---- long jobs: runs of many blocks and chunks a lane, through all six stages ----------------------------------------------------------------
def test_long_jobs_are_what_they_are_listed_for():
    """from the twin alone: two or more interval starts in a lane's run, three or more chunks a lane of the chunks' scan, dwords of the
    unstuffed scan with bits of five blocks and more, and of the blocks either side of a wavefront's (63 | 64) and a workgroup's (255 | 256) edge"""
    reached = set()
    for job, why in E.LONG_JOBS:
        f = E.long_job_facts(job)
        assert E.long_job_holds(job, why), (job, f)
        assert f["per"] >= 2
        reached |= set(why)
        if "starts" in why:
            assert f["period"] and f["starts"] >= 2 and f["per"] > f["period"]
        if "chunk_per" in why:
            assert f["chunk_per"] >= 3 and len(E.long_job_twin(job)[0]) > 3 * LANES * 64 + 1024      # the file's size alone says so
        if "shared" in why:
            assert {(63, 64), (255, 256)} <= set(f["shared"]) and f["in_a_dword"] >= 5
    assert reached == {"starts", "chunk_per", "in_a_dword", "shared"}
    assert {job[3] for job, why in E.LONG_JOBS if "starts" in why} == set(E.SAMPLINGS)


@pytest.mark.parametrize("sampling_class", ("gray", "colour"))
def test_lanes_are_the_twin_over_long_jobs(sim, sampling_class):
    cases, whys = E.long_batch(sampling_class)
    files, nbytes, status, per = run_sim(sim, cases)                                                 # one call
    for f, st, got, case, why in zip(files, status, per, cases, whys):
        assert st == 0
        jpeg, rows, lay = check_case(f, got, *case)
        if why:
            assert jpeg == E.long_job_twin(why[0])[0]


def unstuffed(jpeg):
    """the entropy-coded bytes without stuffing and markers, and every interval's first byte in them"""
    b = body(jpeg)
    out, starts, i = bytearray(), [0], 0
    while True:
        if b[i] == 0xFF and b[i + 1] == 0:
            out.append(0xFF)
            i += 2
        elif b[i] == 0xFF and 0xD0 <= b[i + 1] <= 0xD7:
            starts.append(len(out))
            i += 2
        elif b[i] == 0xFF:
            assert b[i + 1] == 0xD9
            return bytes(out), starts
        else:
            out.append(b[i])
            i += 1


def edges_of(jpeg, rows, lay):
    """which edges of the design (64-byte stuffing chunks, dwords of the emit stage, padded intervals) the twin's file holds"""
    u, starts = unstuffed(jpeg)
    found = set()
    if any(u[i] == 0xFF for i in range(0, len(u), 64)):
        found.add("0xFF first in a chunk")
    if any(u[i] == 0xFF for i in range(63, len(u), 64)):
        found.add("0xFF last in a chunk")
    ends = [p + n for _, p, n in rows]
    last = [k for k in range(len(rows)) if k + 1 == len(rows) or rows[k + 1][1] in lay["restarts"]]      # the last block of every interval
    for k in last:
        if ends[k] % 8 == 0:
            found.add("interval without pad")
        elif u[ends[k] // 8] == 0xFF:
            found.add("0xFF pad byte")
    for k in range(1, len(rows) - 1):
        s, e = rows[k][1], ends[k]
        if s % 32 and e % 32 and s // 32 != (e - 1) // 32 and ends[k - 1] == s and rows[k + 1][1] == e:
            found.add("dwords shared with both neighbours")
    if any(b % 64 == 0 for b in starts[1:]):            # (behind the first interval: the ones that have a marker in front)
        found.add("interval starts on a chunk's first byte")
    if any(b % 64 == 63 for b in starts[1:]):
        found.add("interval starts on a chunk's last byte")
    if len(u) % 64 == 0:
        found.add("unstuffed size a multiple of 64")
    elif len(u) % 16 == 0:
        found.add("unstuffed size a multiple of 16 but not of 64")
    return found


ALL_EDGES = {"0xFF first in a chunk", "0xFF last in a chunk", "interval without pad", "0xFF pad byte", "dwords shared with both neighbours",
             "interval starts on a chunk's first byte", "interval starts on a chunk's last byte", "unstuffed size a multiple of 64",
             "unstuffed size a multiple of 16 but not of 64"}


def edge_candidates():
    """the noise pictures of every sampling first, then tiny gray ones with an interval a block (a few blocks: cheap, and every block's end
    is an interval's)"""
    for seed in range(40):
        sampling = E.SAMPLINGS[seed % 4]
        yield E.picture("noise", 64 + seed, 33, sampling, seed=seed), sampling, 100 if seed % 2 else 92, (1, 2, 7)[seed % 3]
    for seed in range(40, 1000):
        yield E.picture("noise", 24 + 8 * (seed % 4), 8, "gray", seed=seed), "gray", 100 if seed % 2 else 92, 1


@functools.lru_cache(maxsize=None)
def edge_cases():
    """((case, the edges it is there for), ..): inputs picked by what the TWIN's file holds until every edge of ALL_EDGES is covered.  Bounded
    and the same every time; the bounds were tried on the twin alone."""
    missing, used = set(ALL_EDGES), []
    for case in edge_candidates():
        hit = edges_of(*twin_layout(*case)) & missing
        if hit:
            used.append((case, frozenset(hit)))
            missing -= hit
        if not missing:
            break
    assert not missing, missing
    return tuple(used)


def test_lanes_edges_of_the_design(sim):
    """Inputs picked by what the TWIN's file holds -- an 0xFF as the first and as the last byte of a 64-byte stuffing chunk, a pad byte that
    is 0xFF, an interval that ends on a byte without pad bits, a block whose code shares a dword with the block before AND one with the
    block behind, an interval (behind the first) whose first byte is a chunk's first and one whose first byte is a chunk's last, an unstuffed
    scan of whole chunks (EOI behind a full last chunk) and one of whole 16-byte loads that is not -- until every edge is covered; each input
    then goes through the lanes."""
    used = edge_cases()
    assert set().union(*[hit for case, hit in used]) == ALL_EDGES
    for case, hit in used:
        files, nbytes, status, per = run_sim(sim, [case])
        jpeg, rows, lay = check_case(files[0], per[0], *case)
        assert hit <= edges_of(jpeg, rows, lay)


def zrl_symbols(lay):
    """per block of the twin's layout: (ZRL symbols, whether an EOB closes it)"""
    return [(sum(1 for _, ln, m in syms if m == 0), any(m == -1 for _, ln, m in syms)) for c, by, bx, dc, syms in lay["blocks"]]


ZRL_WANT = [(0, True), (1, True), (1, True), (2, True), (2, True), (3, True), (3, False)]


def test_lanes_zero_runs_from_a_picture(sim):
    """a block for every zero run of 15, 16, 31, 32, 47, 48 and 62 in front of its only AC coefficient: 0, 1, 1, 2, 2, 3, 3 ZRL symbols, the
    last block's coefficient at position 63 and so without EOB -- both the length the blocks stage counts and the code the emit stage writes"""
    img = E.zrl_picture()
    case = (img, "gray", E.ZRL_QUALITY, 0)
    jpeg, rows, lay = twin_layout(*case)
    for row, run in zip(rows, E.ZRL_RUNS):
        assert np.flatnonzero(row[0][1:]).tolist() == [run]
    assert zrl_symbols(lay) == ZRL_WANT
    files, nbytes, status, per = run_sim(sim, [case])
    check_case(files[0], per[0], *case)


def zrl_coefficients():
    """(w, h, coefficients): the same runs from chosen coefficients, the values of both signs and of categories 3 .. 9"""
    w, h = 8 * len(E.ZRL_RUNS), 8
    coefs = coef_jpeg.zero_coefs(w, h, "gray")
    for b, run in enumerate(E.ZRL_RUNS):
        coefs[0][0, b, 0] = 5 * b - 9
        coefs[0][0, b, run + 1] = (-1) ** b * ((1 << (b + 3)) - 1)
    return w, h, coefs


def test_lanes_zero_runs_from_coefficients(sim):
    w, h, coefs = zrl_coefficients()
    n = len(E.ZRL_RUNS)
    want, lay = coef_jpeg.write_jpeg(w, h, "gray", coefs, E.quant_tables(50, "gray"), pad_to=0, return_layout=True)
    assert zrl_symbols(lay) == ZRL_WANT
    flat = np.ascontiguousarray(coefs[0][0].astype(np.int16))
    cap = bound(sim, w, h, "gray", 0)
    dst = np.full(cap, GUARD, dtype=np.uint8)
    nbytes, status = C.c_int64(), C.c_int32()
    code, end = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
    assert sim.encodesim_coefs(w, h, 0, 50, 0, flat.ctypes.data, dst.ctypes.data, cap, C.byref(nbytes), C.byref(status), code.ctypes.data, end.ctypes.data, None) == 0
    assert status.value == 0 and dst[:nbytes.value].tobytes() == want and np.all(dst[nbytes.value:] == GUARD)
    assert np.array_equal(end.astype(np.int64) - (code & 0xFFFF), [blk[3][0] for blk in lay["blocks"]])


def test_lanes_longest_code_from_coefficients(sim):
    """More than a tile (66 gray blocks, two intervals) of the longest code a luma block can have -- no picture gives it: 63 AC terms of
    category 10 behind run 0 (16 + 10 bits, the most the Annex K tables ask for one coefficient) and DC differences of category 11 (9 + 11):
    1,658 bits a block, inside JDA_EN_BLOCK_BITS = 1,665 of jda_encode_bound."""
    huff = coef_jpeg.annex_k()[2]
    from jpegdec_amd.synth import _codes
    assert max(_codes(*huff[(1, t)])[rs][1] + (rs & 15) for t in (0, 1) for rs in coef_jpeg.AC_SYMBOLS) == 26
    w, h, ri = 8 * 66, 8, 40
    coefs = coef_jpeg.zero_coefs(w, h, "gray")
    for b in range(66):
        coefs[0][0, b, 0] = 1023 if b & 1 else -1024
        coefs[0][0, b, 1:] = [1023 if z & 1 else -1023 for z in range(1, 64)]
    quant = E.quant_tables(100, "gray")
    want, lay = coef_jpeg.write_jpeg(w, h, "gray", coefs, quant, restart_interval=ri, pad_to=0, return_layout=True)
    flat = np.ascontiguousarray(coefs[0][0].astype(np.int16))
    cap = bound(sim, w, h, "gray", ri)
    dst = np.full(cap, GUARD, dtype=np.uint8)
    nbytes, status = C.c_int64(), C.c_int32()
    code, end = np.zeros(66, dtype=np.uint32), np.zeros(66, dtype=np.uint64)
    assert sim.encodesim_coefs(w, h, 0, 100, ri, flat.ctypes.data, dst.ctypes.data, cap, C.byref(nbytes), C.byref(status), code.ctypes.data, end.ctypes.data, None) == 0
    assert status.value == 0 and dst[:nbytes.value].tobytes() == want and np.all(dst[nbytes.value:] == GUARD)
    assert set((code[1:] & 0xFFFF).tolist()) == {1658} and 1658 <= 1665
    assert np.array_equal(end.astype(np.int64) - (code & 0xFFFF), [blk[3][0] for blk in lay["blocks"]])


def test_reciprocal_division_is_exact(sim):
    """(|c| + d / 2) / d through the host-made reciprocal: every divisor d = 8 q, q = 1..255, against every numerator below 2^17"""
    assert sim.encodesim_divide() == 0


@pytest.mark.parametrize("sampling", E.SAMPLINGS)
def test_header_and_bound(sim, sampling):
    for (w, h), q, ri in (((1, 1), 1, 0), ((129, 65), 75, 3), ((65535, 65535), 100, 65535)):
        buf = np.zeros(1024, dtype=np.uint8)
        n = sim.encodesim_header(w, h, E.SAMPLING_ID[sampling], q, ri, buf.ctypes.data, 1024)
        if w <= 129:
            img = E.picture("smooth", w, h, sampling)
            want = E.file_bytes(img, sampling, q, ri)
            assert buf[:n].tobytes() == want[:coef_jpeg._parse(want)[5]]
            assert len(want) <= bound(sim, w, h, sampling, ri)
        else:
            assert buf[:2].tobytes() == b"\xff\xd8" and bound(sim, w, h, sampling, ri) > 0
    b = C.c_int64(7)
    for bad in ((0, 1, 0, 0), (1, 65536, 0, 0), (1, 1, 4, 0), (1, 1, -1, 0), (1, 1, 0, 65536), (1, 1, 0, -1)):
        assert sim.encodesim_bound(*bad, C.byref(b)) == INVALID and b.value == 0


def test_capacity_one_byte_short(sim):
    cases = [(E.picture("noise", 33, 47, "4:2:0", seed=s), "4:2:0", 75, ri) for s, ri in ((1, 0), (2, 3), (3, 0))]
    sizes = [len(E.file_bytes(*c)) for c in cases]
    files, nbytes, status, per = run_sim(sim, cases, caps=[sizes[0], sizes[1] - 1, sizes[2]])      # (run_sim holds the guard of the short one)
    assert status == [0, MEMORY, 0] and nbytes == sizes
    assert files[0] == E.file_bytes(*cases[0]) and files[1] is None and files[2] == E.file_bytes(*cases[2])


def test_refusals(sim):
    surf = np.zeros((64, 256), dtype=np.uint8)
    dst = np.zeros(4096, dtype=np.uint8)

    def check(out=None, job=None, bpp=4, d=None, cap=4096, n=1, outs=None, jobs=None, dsts=None, caps=None):
        o = (Output * n)(*(outs or [Output(*(out or (surf.ctypes.data, 256, 64, 64)))]))
        j = (Job * n)(*(jobs or [Job(*(job or (0, 0, 16, 16, 3, 75, 0, 0)))]))
        dd = (C.c_void_p * n)(*(dsts or [dst.ctypes.data if d is None else d]))
        cc = (C.c_int64 * n)(*(caps or [cap]))
        return sim.encodesim_check(n, o, bpp, j, dd, cc)

    assert check() == 0
    assert check(job=(0, 0, 16, 16, 0, 75, 0, 0), bpp=1) == 0
    for job in ((-1, 0, 16, 16, 3, 75, 0, 0), (0, -1, 16, 16, 3, 75, 0, 0), (0, 0, 0, 16, 3, 75, 0, 0), (0, 0, 16, 0, 3, 75, 0, 0),      # the rectangle
                (49, 0, 16, 16, 3, 75, 0, 0), (0, 49, 16, 16, 3, 75, 0, 0),
                (0, 0, 16, 16, 3, 0, 0, 0), (0, 0, 16, 16, 3, 101, 0, 0),                                                                # the quality
                (0, 0, 16, 16, 4, 75, 0, 0), (0, 0, 16, 16, -1, 75, 0, 0),                                                               # the sampling
                (0, 0, 16, 16, 3, 75, -1, 0), (0, 0, 16, 16, 3, 75, 65536, 0), (0, 0, 16, 16, 3, 75, 0, 1),                              # the interval, reserved
                (0, 0, 16, 16, 0, 75, 0, 0)):                                                                                            # gray sampling of a colour surface
        assert check(job=job) == INVALID, job
    assert check(job=(0, 0, 16, 16, 3, 75, 0, 0), bpp=1) == INVALID             # colour sampling of a gray surface
    for bpp in (0, 2, 3, 8):
        assert check(bpp=bpp) == INVALID
    assert check(out=(surf.ctypes.data + 2, 256, 63, 64)) == INVALID            # misaligned pixels
    assert check(out=(surf.ctypes.data, 254, 63, 64)) == INVALID                # .. pitch
    assert check(out=(surf.ctypes.data, 252, 64, 64)) == INVALID                # a pitch below the width
    assert check(out=(0, 256, 64, 64)) == INVALID and check(dsts=[None]) == INVALID
    assert check(cap=-1) == INVALID
    # a wide surface: 65536 pixels are refused, 65535 are taken
    wide = np.zeros((1, 65536), dtype=np.uint8)
    assert check(out=(wide.ctypes.data, 65536, 65536, 1), job=(0, 0, 65536, 1, 0, 75, 0, 0), bpp=1) == INVALID
    assert check(out=(wide.ctypes.data, 65536, 65536, 1), job=(0, 0, 65535, 1, 0, 75, 0, 0), bpp=1) == 0
    # a destination over its source rectangle, over the next one, and beside both
    inside = surf.ctypes.data + 5 * 256 + 8
    assert check(d=inside, cap=8) == INVALID
    assert check(d=surf.ctypes.data + 16 * 256, cap=64) == 0                    # behind the rectangle's last row: the surface's other rows are not the job's
    two = dict(n=2, outs=[Output(surf.ctypes.data, 256, 64, 64)] * 2, jobs=[Job(0, 0, 16, 16, 3, 75, 0, 0)] * 2)
    assert check(dsts=[dst.ctypes.data, dst.ctypes.data + 99], caps=[100, 100], **two) == INVALID
    assert check(dsts=[dst.ctypes.data, dst.ctypes.data + 100], caps=[100, 100], **two) == 0
    assert check(dsts=[dst.ctypes.data + 50, dst.ctypes.data], caps=[10, 100], **two) == INVALID


def test_plan_and_lanes_under_the_sanitizers(built_checkers):
    """tests/hostsim/encode_main.cpp: a program of its own (make encodeasan), nothing preloaded"""
    subprocess.run(["make", "encodeasan"], cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    r = subprocess.run([os.path.join(ROOT, "tests", "hostsim", "encode_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"encode_asan ok" in r.stdout, r.stdout[-2000:]


def test_exports():
    import jpegdec_amd as J
    assert (J.ENCODE_GRAY, J.ENCODE_444, J.ENCODE_422, J.ENCODE_420) == (0, 1, 2, 3)
    assert callable(J.encode_surfaces) and callable(J.encode_bound)
    assert J.encode_bound(129, 65, "4:2:0", 3) == J.encode_bound(129, 65, J.ENCODE_420, 3) > 0
