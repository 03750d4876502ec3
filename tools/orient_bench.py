#!/usr/bin/env python3
"""Times of the EXIF-orientation pass (jda_orient_tiles) on the GPU, against same-run baselines.

  (a) the kernel alone: one 4096x4096 surface at 4, 2 and 1 bytes per pixel and a batch of 64 surfaces of 1280x720 (4 bytes per
      pixel), once per orientation 1..8, between two events on the context's stream (jda_internal_orient_time: the job records go up
      before the first event) -- and a device-to-device copy of the same bytes between the same two events (jda_internal_copy_time).
      Rounds alternate over the orientations and the copy, so that a drift of the clock hits them all alike.  Rate = (bytes read +
      bytes written) / time; ratio = the kernel's rate over the copy's.
  (b) one call: jda_decode_to_host_oriented of a 4096x4096 4:2:0 file at orientations 1 and 6 against jda_decode_to_host of the same
      file, alternating: a host clock around calls that end in a device synchronise.

Warm-up before every timed shape; each figure is the median of --repeat rounds with min and max beside it.  One JSON line on stdout
and, with --out, in a file.  Fails without a GPU.  `rocprofv3 --kernel-trace --stats -- python tools/orient_bench.py --kernel-only`
gives the kernel's own time in a run of its own; --counters-shape runs one shape for a counter collection."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from jpegdec_amd.binding import Output  # noqa: E402
from jpegdec_amd.synth import synth_jpeg  # noqa: E402


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5), "n": len(xs)}


def gbps(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e9, 1)


class Shape:
    """n surfaces of w x h pixels of bpp bytes, resident, and a destination for either axis order"""

    def __init__(self, ctx, n, w, h, bpp):
        self.ctx, self.n, self.w, self.h, self.bpp = ctx, n, w, h, bpp
        self.sp = (w * bpp + 15) & ~15
        self.tp = (h * bpp + 15) & ~15                  # pitch of a turned destination
        self.surf = max(self.sp * h, self.tp * w)
        self.surf = (self.surf + 255) & ~255
        self.src, self.dst = ctx.malloc(self.surf * n), ctx.malloc(self.surf * n)
        rng = np.random.RandomState(3)
        block = rng.randint(0, 256, self.surf).astype(np.uint8)
        for i in range(n):
            ctx.from_host(self.src + i * self.surf, block)
        self.moved = 2 * n * w * h * bpp                # bytes read + bytes written

    def outputs(self, o):
        turned = o >= 5
        s = (Output * self.n)(*[Output(self.src + i * self.surf, self.sp, self.w, self.h) for i in range(self.n)])
        d = (Output * self.n)(*[Output(self.dst + i * self.surf, self.tp if turned else self.sp, self.h if turned else self.w, self.w if turned else self.h)
                                for i in range(self.n)])
        return s, d

    def kernel_ms(self, o, reps=1):
        s, d = self.outputs(o)
        ms = (C.c_float * reps)()
        fn = self.ctx.lib.jda_internal_orient_time
        fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.POINTER(Output), C.c_int32, C.POINTER(C.c_float)]
        self.ctx.check(fn(self.ctx.handle, self.n, s, self.bpp, (C.c_int32 * self.n)(*([o] * self.n)), d, reps, ms), "jda_internal_orient_time")
        return list(ms)

    def copy_ms(self, reps=1):
        ms = (C.c_float * reps)()
        fn = self.ctx.lib.jda_internal_copy_time
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_float)]
        self.ctx.check(fn(self.ctx.handle, self.dst, self.src, self.n * self.w * self.h * self.bpp, reps, ms), "jda_internal_copy_time")
        return list(ms)

    def close(self):
        self.ctx.free(self.src)
        self.ctx.free(self.dst)


def kernel_leg(ctx, n, w, h, bpp, warmup, repeat, orientations=range(1, 9)):
    sh = Shape(ctx, n, w, h, bpp)
    t = {o: [] for o in orientations}
    tc = []
    for k in range(warmup + repeat):
        for o in orientations:
            ms = sh.kernel_ms(o)[0]
            if k >= warmup:
                t[o].append(ms)
        ms = sh.copy_ms()[0]
        if k >= warmup:
            tc.append(ms)
    sh.close()
    copy = dict(stats(tc), gbps=gbps(sh.moved, statistics.median(tc)))
    res = {"surfaces": n, "w": w, "h": h, "bytes_per_pixel": bpp, "bytes_read_plus_written": sh.moved, "copy_d2d": copy, "orientation": {}}
    for o in orientations:
        med = statistics.median(t[o])
        res["orientation"][str(o)] = dict(stats(t[o]), gbps=gbps(sh.moved, med), ratio_to_copy=round(statistics.median(tc) / med, 3))
    return res


def one_call_leg(ctx, jpeg, warmup, repeat):
    tp, t1, t6 = [], [], []
    canvas = up1 = up6 = None                           # (every call into a buffer of an earlier one: a fresh 64 MB array is milliseconds of page faults)
    for k in range(warmup + repeat):
        a = time.perf_counter()
        rc, canvas, _ = J.decode_to_host(ctx, jpeg, J.RGB8888, 0, out=canvas)
        b = time.perf_counter()
        assert rc == 0
        rc, up1, _ = J.decode_oriented_to_host(ctx, jpeg, J.RGB8888, 0, 1, out=up1)
        c = time.perf_counter()
        assert rc == 0
        rc, up6, _ = J.decode_oriented_to_host(ctx, jpeg, J.RGB8888, 0, 6, out=up6)
        d = time.perf_counter()
        assert rc == 0
        if k >= warmup:
            tp.append((b - a) * 1e3)
            t1.append((c - b) * 1e3)
            t6.append((d - c) * 1e3)
    return {"decode_to_host": stats(tp), "oriented_1": stats(t1), "oriented_6": stats(t6),
            "oriented_6_minus_decode_to_host_median_ms": round(statistics.median(t6) - statistics.median(tp), 4),
            "oriented_6_minus_oriented_1_median_ms": round(statistics.median(t6) - statistics.median(t1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--kernel-only", action="store_true", help="only (a), few rounds: the workload of a rocprofv3 kernel trace")
    ap.add_argument("--counters-shape", help="BPP:ORIENTATION -- only that 4096x4096 shape, a few launches: the workload of a counter collection")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = J.Context(0)
    res = {"what": "orient_bench", "kernel": {}, "one_call": {}}
    try:
        if a.counters_shape:
            bpp, o = (int(v) for v in a.counters_shape.split(":"))
            res["kernel"]["4096x4096_%dB" % bpp] = kernel_leg(ctx, 1, 4096, 4096, bpp, 1, 3, orientations=[o])
        else:
            wu, rp = (1, 3) if a.kernel_only else (a.warmup, a.repeat)
            for bpp in (4, 2, 1):
                res["kernel"]["4096x4096_%dB" % bpp] = kernel_leg(ctx, 1, 4096, 4096, bpp, wu, rp)
            res["kernel"]["%dx_1280x720_4B" % a.batch] = kernel_leg(ctx, a.batch, 1280, 720, 4, wu, rp)
            if not a.kernel_only:
                res["one_call"]["c420_4096x4096_rgb8888"] = one_call_leg(ctx, synth_jpeg(4096, 4096, "4:2:0", seed=91), a.warmup, a.repeat)
    finally:
        ctx.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
