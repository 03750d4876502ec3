"""jda_prescan_plan.h -- the device pre-scan's array sizes, admission rule and verdict -- through the emulator's build of it.

The expected values are the formulae written out here; nothing is taken from a second call into the library.  (The constants are those of
jda_device_core.h / jda_internal.h in the default build: segments of 256 bytes.)"""
import ctypes as C
import itertools

import pytest

SEG_BYTES, SCAN_PAD, SEG_SUM_WORDS, SEG_START_WORDS = 256, 32, 8, 5
ST_BAD, ST_TERMINAL, ST_MAX_AC, ST_MAX_DC, ST_TRUNC, ST_RST_MISMATCH, ST_INDEX_OK, ST_SETTLED, ST_ROUND0, ST_NCAND, ST_WORDS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 66, 68
MAX_ROUND = 56
FIELDS = ("n_segs", "cand_cap", "scan", "entry", "seg_sum", "seg_start", "worklist", "restart_pos", "rst_events", "records", "cands")


def record_cap(mcu_min_bits, nblocks):
    """jda_record_cap (jda_internal.h)"""
    mcu_min_bits = max(mcu_min_bits, 2 * nblocks)
    return ((SEG_BYTES * 8 // mcu_min_bits + 2) * nblocks + 4 + 3) & ~3


def a16(v):
    return (v + 15) & ~15


def sizes_expected(length, n_intervals, rec_cap):
    n_segs = length // SEG_BYTES + 1
    cand_cap = max(1024, n_segs * 16)
    return dict(n_segs=n_segs, cand_cap=cand_cap,
                scan=a16(max(length + SCAN_PAD, n_segs * SEG_BYTES + 16)),
                entry=a16((n_segs + 1) * 4),
                seg_sum=a16(n_segs * 4 * SEG_SUM_WORDS),
                seg_start=a16(n_segs * 4 * SEG_START_WORDS),
                worklist=a16(n_segs * 8),
                restart_pos=a16((n_intervals + 1) * 4) if n_intervals else 0,
                rst_events=a16(n_intervals * 8) if n_intervals else 0,
                records=a16(n_segs * rec_cap * 4),
                cands=cand_cap * 16)


def admits_expected(length, rec_cap):
    return (length // SEG_BYTES + 1) * rec_cap * 4 <= 8 * length + (16 << 20)


@pytest.fixture(scope="module")
def plan(hostsim):
    hostsim.hostsim_prescan_sizes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    hostsim.hostsim_prescan_sizes.restype = None
    hostsim.hostsim_prescan_admits.argtypes = [C.c_uint32, C.c_uint32]
    hostsim.hostsim_prescan_verdict.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
    hostsim.hostsim_prescan_rounds_used.argtypes = [C.POINTER(C.c_uint32)]
    return hostsim


def words(values):
    return (C.c_uint32 * len(values))(*values)


def test_record_cap_of_the_densest_tables():
    assert record_cap(0, 6) == 1036          # 2 bits per block at least: 170 MCUs of six blocks in a segment's 2,048 bits, + 2 MCUs, + 4


@pytest.mark.parametrize("length", [0, 1, 255, 256, 257, 16383, 16384, 63 * 256, 64 * 256])
def test_sizes(plan, length):
    for n_intervals, rec_cap in itertools.product((0, 1, 2), (4, 400, record_cap(0, 6))):
        out = (C.c_uint64 * len(FIELDS))()
        plan.hostsim_prescan_sizes(length, n_intervals, rec_cap, out)
        got, want = dict(zip(FIELDS, out)), sizes_expected(length, n_intervals, rec_cap)
        for f in FIELDS:
            assert got[f] == want[f], (f, length, n_intervals, rec_cap, got[f], want[f])
        for f in FIELDS[2:]:
            assert got[f] % 16 == 0, (f, got[f])
        assert (got["restart_pos"] == 0) == (n_intervals == 0) and (got["rst_events"] == 0) == (n_intervals == 0)


def test_sizes_cases_lie_on_both_sides_of_the_steps():
    # both sides of the n_segs step, and of the step from 1,024 candidates to sixteen per segment
    assert [sizes_expected(n, 0, 4)["n_segs"] for n in (255, 256, 16383, 16384)] == [1, 2, 64, 65]
    assert [sizes_expected(n, 0, 4)["cand_cap"] for n in (63 * 256, 64 * 256)] == [1024, 65 * 16]


def test_admission_of_the_densest_tables(plan):
    rec_cap = record_cap(0, 6)
    # the record area steps up at a segment's first byte and the bound grows with every byte: the first length that is refused is a multiple of 256
    first = next(k * SEG_BYTES for k in itertools.count() if not admits_expected(k * SEG_BYTES, rec_cap))
    assert all(admits_expected(n, rec_cap) for n in range(first - 2 * SEG_BYTES, first))
    assert first == 8003 * 256          # 4,144 bytes of records per segment against 2,048 of bound: 16 MB of grace last 8,002.4 segments
    assert plan.hostsim_prescan_admits(first, rec_cap) == 0
    assert plan.hostsim_prescan_admits(first - 256, rec_cap) == 1
    assert plan.hostsim_prescan_admits(first - 1, rec_cap) == 1


def test_admission_of_the_usual_tables(plan):
    # 400 slots of four bytes per 256-byte segment are 6.25 x the scan (+ one segment's 1,600 bytes): never past 8 x + 16 MB
    lengths = sorted({n + d for n in range(0, 32 << 20, 48 * 1024 + 256) for d in (-1, 0, 1) if 0 <= n + d < (32 << 20)} | {(32 << 20) - 1, (32 << 20) - 256})
    assert all(admits_expected(n, 400) for n in lengths)
    assert all(plan.hostsim_prescan_admits(n, 400) == 1 for n in lengths)


def good_words():
    w = [0] * ST_WORDS
    w[ST_SETTLED] = 1; w[ST_INDEX_OK] = 1; w[ST_TERMINAL] = 1
    w[ST_MAX_AC] = 10; w[ST_MAX_DC] = 1000; w[ST_TRUNC] = 3; w[ST_NCAND] = 7          # (what a good stream may leave: none of it is a verdict)
    w[ST_ROUND0 + 2] = 40; w[ST_ROUND0 + 3] = 2
    return w


# one condition violated alone: SETTLED == 1, INDEX_OK == 1, BAD == 0, TERMINAL == 1, RST_MISMATCH == 0, and the word behind the last round's == 0.
# (The last two matter to jda_upload_batch, and to the pipeline for streams with intervals: the header holds them for every caller and says why
# no caller's kernels break them otherwise.)
VIOLATIONS = [(ST_SETTLED, 0), (ST_SETTLED, 2), (ST_INDEX_OK, 0), (ST_INDEX_OK, 2), (ST_BAD, 1), (ST_TERMINAL, 0), (ST_TERMINAL, 2), (ST_RST_MISMATCH, 1),
              (ST_ROUND0 + MAX_ROUND + 1, 1)]


def test_verdict(plan):
    null = C.POINTER(C.c_uint32)()
    markers_ok = words([123456, 4, 0, 0])          # the device filter's result: length, markers
    for fr, n_int in ((null, 0), (null, 5), (markers_ok, 5), (markers_ok, 0)):
        assert plan.hostsim_prescan_verdict(words(good_words()), fr, n_int) == 1
        for word, value in VIOLATIONS:
            w = good_words()
            w[word] = value
            assert plan.hostsim_prescan_verdict(words(w), fr, n_int) == 0, (word, value, n_int)


def test_verdict_marker_count_is_the_device_filters_alone(plan):
    null = C.POINTER(C.c_uint32)()
    good = words(good_words())
    for markers in (0, 3, 5, 6):                     # five intervals are four markers
        fr = words([123456, markers, 0, 0])
        assert plan.hostsim_prescan_verdict(good, fr, 5) == 0
        assert plan.hostsim_prescan_verdict(good, fr, 0) == 1          # no intervals: whatever the filter took for a marker does not count
        assert plan.hostsim_prescan_verdict(good, null, 5) == 1        # the host filter placed the markers: there is no count to compare


def test_rounds_used(plan):
    w = [0] * ST_WORDS
    w[ST_NCAND] = 9                                  # (not a list length)
    assert plan.hostsim_prescan_rounds_used(words(w)) == 2
    for k in (2, 3, 10, MAX_ROUND, MAX_ROUND + 1):
        w = [0] * ST_WORDS
        w[ST_NCAND] = 9
        for r in range(2, k + 1):
            w[ST_ROUND0 + r] = 1 + r
        assert plan.hostsim_prescan_rounds_used(words(w)) == k + 1
    assert ST_ROUND0 + MAX_ROUND + 1 < ST_NCAND      # the last word it reads
    w = [1] * ST_WORDS                               # every word nonzero: it stops behind the last round's
    assert plan.hostsim_prescan_rounds_used(words(w)) == MAX_ROUND + 2
