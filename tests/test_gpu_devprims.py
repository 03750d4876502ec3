"""The device side of every `#if defined(__HIP_DEVICE_COMPILE__)` fork of jda_device_core.h against its host side, on an MI355X.

tests/devprims/libjda_devprims.so (make devprims: the product's compiler flags) reaches both sides of a fork through one call expression:
devprims_device_* in a plain kernel, devprims_host_* in a loop.  For every op, over the inputs of tests/devprims_util.py:
device == host == the numpy definition, exactly -- no tolerance anywhere.  A difference names the op, the first differing inputs and
both results.  The CPU simulators of tests/hostsim stand on the host sides; this is what ties them to what the GPU computes.

Two helpers have a rule of their own: a NaN out of jda_unpack_half must be a quiet NaN on both sides (its payload is not compared), and
jda_wave_any's host side is by design the lane's own answer -- the device's answer is held to the OR over the lanes inside the branch,
which is also the OR of the host's answers.

The output buffer is filled with a guard value and carries a guard tail, which must come back untouched.  The context serves malloc /
from_host / to_host / free alone; the launches are the library's own, on the null stream."""
import ctypes as C

import numpy as np
import pytest

from tests import devprims_util as D

pytestmark = pytest.mark.gpu
U32 = np.uint32
GUARD, TAIL = 0xA5A5A5A5, 64                     # the tail in words


@pytest.fixture(scope="module")
def lib():
    return D.load()


class Device:
    """device buffers for one call: inputs copied in, one guard-filled output with a guard tail"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 4))
        self.ptrs.append(p)
        if a.nbytes:
            self.ctx.from_host(p, a.view(np.uint8).reshape(-1))
        return C.c_void_p(p)

    def out(self, words):
        self.words = words
        self.out_ptr = self.put(np.full(words + TAIL, GUARD, U32))
        return self.out_ptr

    def result(self, status, name):
        assert status == 0, "%s: hipError_t %d" % (name, status)
        got = self.ctx.to_host(self.out_ptr.value, 4 * (self.words + TAIL)).view(U32)
        assert np.all(got[self.words:] == GUARD), "%s: the guard tail behind the output was written" % name
        return got[:self.words].copy()

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


def three_way(name, want, host, dev, *inputs):
    for label, x, y in (("host side against the definition", want, host), ("DEVICE side against the definition", want, dev), ("DEVICE side against the host side", host, dev)):
        msg = D.first_difference(name, x, y, *inputs)
        assert msg is None, label + " -- " + msg.replace("definition", "first").replace("got", "second")


@pytest.mark.parametrize("op", D.VAL_OPS)
def test_val(gpu_ctx, lib, op):
    """one launch an op.  (jda_shr_upto32: n == 32 included, n mod 32 on both sides; jda_extend_top: s = 1 .. 31)"""
    a, b, c = D.val_inputs(op)
    dv = Device(gpu_ctx)
    try:
        st = lib.devprims_device_val(D.VAL_OPS.index(op), dv.put(a), dv.put(b), dv.put(c), dv.out(a.size), a.size)
        dev = dv.result(st, op)
    finally:
        dv.free()
    want, host = D.define_val(op, a, b, c), D.host_val(lib, op, a, b, c)
    if op == "unpack_half":
        nan = np.isnan(a.astype(np.uint16).view(np.float16))
        for side, r in (("host", host), ("device", dev)):
            assert np.all(r[nan] & 0x7FC00000 == 0x7FC00000), "%s side: a NaN must come out as a quiet NaN" % side
        want, host, dev, a = want[~nan], host[~nan], dev[~nan], a[~nan]
    three_way(op, want, host, dev, a, b, c)


@pytest.mark.parametrize("op", D.WAVE_OPS)
def test_wave(gpu_ctx, lib, op):
    """one wavefront of 64 lanes a group, every lane present; jda_wave_any inside a branch that only some lanes enter"""
    a, b = D.wave_inputs(op)
    dv = Device(gpu_ctx)
    try:
        st = lib.devprims_device_wave(D.WAVE_OPS.index(op), dv.put(a), dv.put(b), dv.out(2 * a.size), a.size)
        dev = dv.result(st, op).reshape(-1, 2)
    finally:
        dv.free()
    host = D.host_wave(lib, op, a, b)
    ins = (np.repeat(a.reshape(-1), 2), np.repeat(b.reshape(-1), 2))
    if op != "wave_any_branch":
        three_way(op, D.define_wave(op, a, b), host, dev, *ins)
        return
    msg = D.first_difference(op, D.define_wave(op, a, b), dev, *ins)
    assert msg is None, "DEVICE side against the definition -- " + msg
    msg = D.first_difference(op, D.define_wave(op, a, b, host=True), host, *ins)
    assert msg is None, "host side (the lane's own answer) -- " + msg
    inside = (b != 0)
    ors = (inside & (host[:, 0].reshape(a.shape) == 1)).any(axis=1, keepdims=True)
    assert np.array_equal(np.where(inside, ors, D.WAVE_OUTSIDE).astype(U32), dev[:, 0].reshape(a.shape))


def test_window_reader(gpu_ctx, lib):
    """jda_wr_init / jda_wr_peek / jda_wr_consume over a window in LDS behind a 16-byte pad: every start, peek for peek"""
    win = D.window()
    start, steps = D.wr_walks()
    dv = Device(gpu_ctx)
    try:
        st = lib.devprims_device_wr(dv.put(win), dv.put(start), dv.put(steps), dv.out(steps.size), steps.shape[0], steps.shape[1])
        dev = dv.result(st, "wr")
    finally:
        dv.free()
    three_way("wr", D.define_wr(win, start, steps), D.host_wr(lib, win, start, steps), dev, np.repeat(start, steps.shape[1]))


@pytest.mark.parametrize("op", D.LDS_OPS)
def test_lds(gpu_ctx, lib, op):
    """jda_lds_bytes_apart, JDA_LDS_LOAD_U16 and JDA_COEF_STORE over the same window"""
    win = D.window()
    a, b = D.lds_inputs(op)
    dv = Device(gpu_ctx)
    try:
        st = lib.devprims_device_lds(D.LDS_OPS.index(op), dv.put(win), dv.put(a), dv.put(b), dv.out(a.size), a.size)
        dev = dv.result(st, op)
    finally:
        dv.free()
    three_way(op, D.define_lds(op, win, a, b), D.host_lds(lib, op, win, a, b), dev, a, b)


@pytest.fixture(scope="module")
def cube_buffer(gpu_ctx):
    """one 64 MiB output (+ tail) for the cube formulas, guard-filled anew for each"""
    p = gpu_ctx.malloc(4 * (D.CUBE + TAIL))
    yield p, np.full(D.CUBE + TAIL, GUARD, U32).view(np.uint8)
    gpu_ctx.free(p)


@pytest.mark.parametrize("op", D.CUBE_OPS)
def test_cube(gpu_ctx, lib, cube_buffer, op):
    """all 2^24 (Y, Cb, Cr): one launch, compared in chunks"""
    p, guard = cube_buffer
    gpu_ctx.from_host(p, guard)
    st = lib.devprims_device_cube(D.CUBE_OPS.index(op), C.c_void_p(p), 0, D.CUBE)
    assert st == 0, "%s: hipError_t %d" % (op, st)
    dev = gpu_ctx.to_host(p, 4 * (D.CUBE + TAIL)).view(U32)
    assert np.all(dev[D.CUBE:] == GUARD), "%s: the guard tail behind the output was written" % op
    chunk = 1 << 21
    for first in range(0, D.CUBE, chunk):
        i = np.arange(first, first + chunk, dtype=U32)
        three_way(op, D.define_cube(op, first, chunk), D.host_cube(lib, op, first, chunk), dev[first:first + chunk], i >> 16, (i >> 8) & 255, i & 255)
