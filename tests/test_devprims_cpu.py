"""The host side of every `#if defined(__HIP_DEVICE_COMPILE__)` fork of jda_device_core.h against an independent definition, without a GPU.

The simulators of tests/hostsim run the kernels' lanes through the HOST sides of the header's forks; tests/test_gpu_devprims.py holds the
device sides to the same host sides on an MI355X.  Here:

* for every op of the four families (tests/devprims/devprims_ops.h), devprims_host_* = the numpy definition of tests/devprims_util.py,
  exactly, over inputs chosen per helper -- and the inputs hold the edge cases their generators name;
* every fork of the header is either in the library's op table or in the list of forks that have no value to compare, with its reason:
  a fork added later without a test fails here;
* the same host loops as a program of their own under ASan + UBSan give the same results (nothing is loaded into this process)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import devprims_util as D

U32 = np.uint32


@pytest.fixture(scope="module")
def lib():
    return D.load()


# ---- the inputs hold what their generators promise -----------------------------------------------------------------------------------------
def test_inputs_hold_their_edges():
    one = D.packed_one()
    assert one.size == 3 << 16
    assert set((one[:1 << 16] & 0xFFFF).tolist()) == set(range(1 << 16)) and set((one[1 << 16:2 << 16] >> 16).tolist()) == set(range(1 << 16))
    assert np.array_equal(one[:1 << 16] >> 16, (one[:1 << 16] & 0xFFFF) ^ 0xFFFF)
    a, b = D.packed_two()
    assert a.size == 12 ** 4 + (1 << 16)
    quads = set(zip((a & 0xFFFF).tolist(), (a >> 16).tolist(), (b & 0xFFFF).tolist(), (b >> 16).tolist()))
    assert all((p, q, r, s) in quads for p in D.PAIR_EDGES for q in (0, 0x8000, 0xFFFF) for r in D.PAIR_EDGES for s in (1, 0x7FFF, 0xFFFF))
    _, _, sel = D.perm_inputs()
    for pos in range(4):
        assert set(((sel >> (8 * pos)) & 0xFF).tolist()) == set(range(256))
    assert set(D.PERM_SELECTORS) <= set(sel.tolist())
    h0, l0, h1, l1 = D.PERM_SELECTOR_PARTS                  # the selectors jda_be64_from_words / jda_load_be64 make, at every byte shift
    assert {(((h << 32) | l) >> (8 * k)) & 0xFFFFFFFF for h, l in ((h0, l0), (h1, l1)) for k in range(4)} <= set(sel.tolist())
    _, _, c = D.shift_inputs("alignbyte")
    assert set(range(8)) <= set(c.tolist())
    _, _, c = D.shift_inputs("alignbit")
    assert set(range(64)) <= set(c.tolist())
    _, off, width = D.bfe_inputs()
    pairs = set(zip(off.tolist(), width.tolist()))
    assert all((o, w) in pairs for w in range(32) for o in range(32) if o + w <= 32) and all((o, 32) in pairs for o in range(32))
    a, b, _ = D.mul_inputs()
    sa, sb = a.astype(np.int32).astype(np.int64), b.astype(np.int32).astype(np.int64)
    for e in D.MUL_EDGES:
        assert e in sa.tolist()[:64] and e in sb.tolist()[:64]
    outside = (np.abs(sa) >= 1 << 23) | (np.abs(sb) >= 1 << 23)
    assert np.count_nonzero(outside) > 1 << 15 and np.count_nonzero(~outside) > 1 << 14      # outside 24 bits is where the stand-ins were loose
    a, b, c = D.udot4_inputs()
    full = (a == 0xFFFFFFFF) & (b == 0xFFFFFFFF)
    assert np.any(full & (c.astype(np.uint64) + 4 * 255 * 255 >= 1 << 32)) and np.any(full & (c.astype(np.uint64) + 4 * 255 * 255 == (1 << 32) - 1))
    U_, n, _ = D.lag_inputs()
    assert set(n.tolist()) == {0, 1, 2, 3}
    for k in range(6):
        f = (U_ >> (5 * k)) & 31
        assert np.any((f == 0) & (n == 3)) and np.any((f == 31) & (n == 3))
    assert np.array_equal(D.half_inputs()[0], np.arange(1 << 16))
    t, s, _ = D.shr_inputs("shr_upto32")
    assert set(range(33)) <= set(s.tolist())             # n == 32 included: both sides take n mod 32 now, see test_val
    t, s, _ = D.shr_inputs("extend_top")
    assert set(s.tolist()) == set(range(1, 32)) and np.any(t >> 31 == 1) and np.any(t >> 31 == 0)
    a, _, _ = D.rs_clip_inputs()
    have = set(a.tolist())
    for base in list(range(0, 1 << 32, 1 << 22)) + [(255 << 22) - (1 << 21), (1 << 30) - 1 - (1 << 21), (1 << 32) - (1 << 21)]:
        assert all((base + d) % (1 << 32) in have for d in range(-2, 3)), hex(base)
    assert a.size > 65536


def test_perm_selector_list_is_the_header_s():
    """PERM_SELECTORS is collected by hand: every 32-bit constant of a statement that calls jda_perm or picks its `sel` -- the parts of a
    computed selector aside, which are PERM_SELECTOR_PARTS -- is in it, and it holds nothing the header does not use.  A search of the
    project's own source for a call's constants, nothing else."""
    lines = open(os.path.join(D.ROOT, "jpegdec_amd", "csrc", "jda_device_core.h")).read().split("\n")
    found = set()
    for i, line in enumerate(lines):
        code = line.split("//")[0]
        picks = re.search(r"\bsel\s*=", code) is not None
        if "jda_perm(" not in code and not picks:
            continue
        if picks and not code.rstrip().endswith(";"):       # a selector chosen over two lines
            code += lines[i + 1].split("//")[0]
        found |= {int(m, 16) for m in re.findall(r"\b0x([0-9a-fA-F]{8})u\b", code)}
    assert len(found) >= 30
    bases = found - set(D.PERM_SELECTOR_PARTS)
    missing = sorted(bases - set(D.PERM_SELECTORS))
    assert not missing, "selector constants of the header that PERM_SELECTORS lacks: %s" % ", ".join("0x%08x" % m for m in missing)
    expanded = {0x0c0c0400 + p * 0x0101 for p in range(1, 4)} | {0x0d040100 + (p << 16) for p in range(1, 4)}
    stale = sorted(set(D.PERM_SELECTORS) - found - expanded)
    assert not stale, "listed, but not in the header: %s" % ", ".join("0x%08x" % m for m in stale)
    assert set(D.PERM_SELECTOR_PARTS) <= found


def test_wave_inputs_hold_their_edges():
    """the rows the wave helpers' generators name: all 0, all 1, each single lane, values whose sums wrap; every class everywhere, none
    (class 4), a single lane of the class; a permutation, every lane pulling one lane, sources >= 64; branches nobody, everybody and one
    lane enters, and a yes that stays outside"""
    rows = lambda a: {tuple(r) for r in a.tolist()}
    a, _ = D.wave_inputs("excl_sum")
    have = rows(a)
    assert (0,) * 64 in have and (1,) * 64 in have and (0xFFFFFFFF,) * 64 in have
    for lane in range(64):
        for v in (1, 0xFFFFFFFF):
            assert tuple(v if k == lane else 0 for k in range(64)) in have, lane
    assert np.any(a.astype(np.uint64).sum(axis=1) >= 1 << 32) and np.any(a.max(axis=1) == 0xFFFFFFFF)
    for c in range(4):
        a, _ = D.wave_inputs("class_rank%d" % c)
        have = rows(a)
        assert all((cls,) * 64 in have for cls in range(5)), c      # all equal, every class; class 4 = none
        for lane in range(64):
            assert tuple(c if k == lane else 4 for k in range(64)) in have, (c, lane)
        assert any(len(set(r)) == 5 for r in have)
    a, b = D.wave_inputs("lane_pull")
    assert any(sorted(r) == list(range(64)) for r in b.tolist())
    assert all((lane,) * 64 in rows(b) for lane in (0, 1, 31, 32, 63))
    assert any(min(r) >= 64 and sorted(x % 64 for x in r) == list(range(64)) for r in b.tolist())
    a, b = D.wave_inputs("wave_any_branch")
    inside, yes = b != 0, a != 0
    assert np.any(~inside.any(axis=1)) and np.any(inside.all(axis=1)) and np.any(inside.sum(axis=1) == 2)
    assert np.any(inside.any(axis=1) & ~(inside & yes).any(axis=1) & (~inside & yes).any(axis=1))      # the only yes stays outside
    assert np.any((inside.sum(axis=1) == 63) & (yes.sum(axis=1) == 1) & ~(inside & yes).any(axis=1))


def test_unpack_byte_pool_tells_fused_from_unfused():
    x, s, b, differ = D.unpack_byte_inputs()
    assert differ >= 16, differ
    xf = x.view(np.float32)
    assert np.any(np.isnan(xf) & (x & 0x00400000 == 0)) and np.any(np.isnan(xf) & (x & 0x00400000 != 0)) and np.any(np.isinf(xf))
    assert np.any((x & 0x7F800000 == 0) & (x & 0x007FFFFF != 0))


# ---- family 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", D.VAL_OPS)
def test_val(lib, op):
    """devprims_host_val = the definition.  jda_shr_upto32 used to be a fork that differed by design at n == 32 (host 0, device x: the
    shift takes n mod 32), "never used" -- but jda_q4_block used jda_extend_top(m, 0) for a run symbol without magnitude bits, so the
    emulator was right where the GPU was wrong.  Both sides are the hardware's shift now and n == 32 is among the inputs;
    jda_extend_top is held over s = 1 .. 31, the sizes that have a value."""
    a, b, c = D.val_inputs(op)
    want, got = D.define_val(op, a, b, c), D.host_val(lib, op, a, b, c)
    if op == "unpack_half":
        nan = np.isnan(a.astype(np.uint16).view(np.float16))
        assert np.count_nonzero(nan) == 2 * 1023
        assert np.all(got[nan] & 0x7FC00000 == 0x7FC00000), "a NaN must come out as a quiet NaN"
        want, got = want[~nan], got[~nan]
        a = a[~nan]
    assert lib.devprims_ops(1) == len(D.VAL_OPS)
    msg = D.first_difference(op, want, got, a, b, c)
    assert msg is None, msg


def test_pk_limit10_is_the_range_limit():
    """what jda_pk_limit10 is FOR: the high byte of each half = ucRangeTable[(v >> 5) & 0x3ff] = clamp(sext10(v >> 5) + 128)"""
    a = D.packed_one()
    r = D.define_val("pk_limit10", a, a, a)
    for sh in (0, 16):
        v = ((a >> sh) & 0xFFFF).astype(np.int64)
        f = (v >> 5) & 0x3FF
        want = np.clip(np.where(f >= 512, f - 1024, f) + 128, 0, 255)
        assert np.array_equal((r >> (sh + 8)) & 0xFF, want)


# ---- family 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", D.WAVE_OPS)
def test_wave(lib, op):
    """the host sides over the all[] arrays, as the emulator passes them (jda_wave_any: the lane's own answer, by design)"""
    a, b = D.wave_inputs(op)
    want, got = D.define_wave(op, a, b, host=True), D.host_wave(lib, op, a, b)
    assert lib.devprims_ops(2) == len(D.WAVE_OPS)
    msg = D.first_difference(op, want, got, np.repeat(a.reshape(-1), 2), np.repeat(b.reshape(-1), 2))
    assert msg is None, msg
    if op == "excl_sum":
        assert np.any(a.astype(np.uint64).sum(axis=1) >= 1 << 32)
    if op == "wave_any_branch":                             # the device's answer differs from the lane's own somewhere: the GPU test is not vacuous
        assert np.any(D.define_wave(op, a, b)[:, 0] != want[:, 0])
    if op == "lane_pull":
        assert np.any(b >= 64)


# ---- family 3 ----------------------------------------------------------------------------------------------------------------
def test_window_reader(lib):
    win = D.window()
    start, steps = D.wr_walks()
    assert {(int(s) >> 3, int(s) & 7) for s in start} == {(p, o) for p in range(16) for o in range(8)}
    assert steps.min() == 1 and steps.max() == 16
    want, got = D.define_wr(win, start, steps), D.host_wr(lib, win, start, steps)
    live = want != D.WR_STOP
    assert live[:, 0].all() and not live[:, -1].any()       # every walk starts inside and ends by itself
    msg = D.first_difference("wr", want, got, np.repeat(start, steps.shape[1]))
    assert msg is None, msg
    # the definition against the bit string, once by hand: bit 0 is the top bit of dword 0
    peeks = D.window_peeks(win)
    assert int(peeks[0]) == int(win[0]) and int(peeks[32]) == int(win[1]) and int(peeks[4]) == ((int(win[0]) << 4) & 0xFFFFFFFF) | (int(win[1]) >> 28)


@pytest.mark.parametrize("op", D.LDS_OPS)
def test_lds(lib, op):
    win = D.window()
    a, b = D.lds_inputs(op)
    want, got = D.define_lds(op, win, a, b), D.host_lds(lib, op, win, a, b)
    assert lib.devprims_ops(3) == len(D.LDS_OPS)
    msg = D.first_difference(op, want, got, a, b)
    assert msg is None, msg
    if op == "coef_store":
        assert np.any(a >> 8 != 0)                          # bits above byte 0 of t, which the store must ignore


# ---- family 4 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", D.CUBE_OPS)
def test_cube(lib, op):
    """all 2^24 (Y, Cb, Cr), in chunks"""
    assert lib.devprims_ops(4) == len(D.CUBE_OPS)
    chunk = 1 << 21
    for first in range(0, D.CUBE, chunk):
        want, got = D.define_cube(op, first, chunk), D.host_cube(lib, op, first, chunk)
        i = np.arange(first, first + chunk, dtype=U32)
        msg = D.first_difference(op, want, got, i >> 16, (i >> 8) & 255, i & 255)
        assert msg is None, msg


# ---- coverage --------------------------------------------------------------------------------------------------------------------
def forks_of(path):
    """(line number, the function or macro that encloses it) of every preprocessor fork on __HIP_DEVICE_COMPILE__: the function whose
    body holds the line, or -- at file level -- the first macro the fork defines"""
    lines = open(path).read().split("\n")
    out = []
    for i, line in enumerate(lines):
        if "__HIP_DEVICE_COMPILE__" not in line or not line.lstrip().startswith("#"):
            continue
        name = None
        for j in range(i - 1, -1, -1):
            if lines[j].startswith("}") or (lines[j].startswith(("JDA_HD", "template")) and lines[j].split("//")[0].rstrip().endswith("}")):
                break                                       # a body closed above (or opened and closed on one line): the fork is at file level
            m = re.match(r"(?:template\s*<[^>]*>\s*)?JDA_HD(?:_MEMBER)?\s.*?\b(\w+)\s*\(", lines[j])
            if m:
                name = m.group(1)
                break
        if name is None:
            for j in range(i + 1, len(lines)):
                m = re.match(r"#\s*define\s+(\w+)", lines[j])
                if m or lines[j].startswith("#endif"):
                    name = m.group(1) if m else None
                    break
        out.append((i + 1, name))
    return out


def test_every_fork_is_tested_or_exempt():
    csrc = os.path.join(D.ROOT, "jpegdec_amd", "csrc")
    forks = forks_of(os.path.join(csrc, "jda_device_core.h")) + forks_of(os.path.join(csrc, "jda_internal.h"))
    assert len(forks) >= 40 and forks[-1][1] == "JDA_GLOBAL"
    assert not set(D.FORK_OPS) & set(D.FORK_EXEMPT)
    known = {"val:" + o for o in D.VAL_OPS} | {"wave:" + o for o in D.WAVE_OPS} | {"lds:" + o for o in D.LDS_OPS} | {"wr"}
    for name, ops in D.FORK_OPS.items():
        assert ops and set(ops) <= known, name
    for line, name in forks:
        assert name is not None, "line %d: no function or macro found around the fork" % line
        assert name in D.FORK_OPS or name in D.FORK_EXEMPT, (
            "line %d: the fork in %s has neither an op in tests/devprims (devprims_ops.h, tests/devprims_util.FORK_OPS) nor a reason in FORK_EXEMPT" % (line, name))
    found = {name for _, name in forks}
    stale = (set(D.FORK_OPS) | set(D.FORK_EXEMPT)) - found
    assert not stale, "listed, but no fork there any more: %s" % sorted(stale)
    assert all(len(reason) > 20 for reason in D.FORK_EXEMPT.values())
    # no other file of the product forks on the symbol
    for fn in sorted(os.listdir(csrc)):
        if fn not in ("jda_device_core.h", "jda_internal.h"):
            assert "__HIP_DEVICE_COMPILE__" not in open(os.path.join(csrc, fn), errors="replace").read(), fn


# ---- the sanitizer program ---------------------------------------------------------------------------------------------------------
def test_sanitizer_program(lib, tmp_path):
    """the host loops over the same inputs as a program of their own under ASan + UBSan; its checksums = the library's host side"""
    D.build("devprimsasan")
    records, want = [], []

    def rec(family, op, n, maxsteps, arrays, out):
        records.append(np.array([family, op, n, maxsteps], dtype=U32).tobytes() + b"".join(np.ascontiguousarray(x).tobytes() for x in arrays))
        want.append((family, op, D.checksum(out)))
    for k, op in enumerate(D.VAL_OPS):
        a, b, c = D.val_inputs(op)
        rec(1, k, a.size, 0, (a, b, c), D.host_val(lib, op, a, b, c))
    for k, op in enumerate(D.WAVE_OPS):
        a, b = D.wave_inputs(op)
        rec(2, k, a.size, 0, (a, b), D.host_wave(lib, op, a, b))
    win = D.window()
    start, steps = D.wr_walks()
    pad = np.zeros(-steps.size % 4, np.uint8)
    rec(3, 0, start.size, steps.shape[1], (win, start, steps, pad), D.host_wr(lib, win, start, steps))
    for k, op in enumerate(D.LDS_OPS):
        a, b = D.lds_inputs(op)
        rec(5, k, a.size, 0, (win, a, b), D.host_lds(lib, op, win, a, b))
    for k, op in enumerate(D.CUBE_OPS):
        rec(4, k, D.CUBE, 0, (), D.host_cube(lib, op, 0, D.CUBE))
    path = tmp_path / "records.bin"
    path.write_bytes(b"".join(records))
    r = subprocess.run([D.ASAN_PROGRAM, str(path)], cwd=D.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "devprims_asan ok %d" % len(want) in r.stdout, r.stdout[-4000:]
    got = [(int(f), int(o), int(h, 16)) for _, _, f, o, h in (l.split() for l in r.stdout.splitlines() if l.startswith("rec "))]
    assert got == want
