#!/usr/bin/env python3
"""Times of the reduce pass (jda_reduce_tiles) and of thumbnails(pillow=True) on the GPU, in one run.

Reduce: 64 RGB8888 surfaces of 4096 x 4096, every surface a buffer of its own filled with random bytes (more source bytes than the Infinity
Cache holds), shrunk by 2, 4 and 8 on both axes.  The launch runs between the context's two timer events (jda_internal_reduce_time: the job
records go up before the first event), and so does a plain device copy of the same source bytes (jda_internal_copy_time), the yardstick of
DESIGN 6.7 and 6.10.  Rounds alternate over reduce and copy, so that a drift of the clock hits both alike; warm-up rounds first; each figure
is the median of --repeat rounds with min and max beside it.  gbps = SOURCE bytes read over the time.

Thumbnails: thumbnails(pillow=True) beside thumbnails() as it was (pillow=False: the reference road's decode, its prescale, one resize to a
fixed size), wall clock around the call and a device synchronisation, alternating, median of --repeat: --files-720 files of 1280 x 720
(4:2:0) to 128 and --files-4096 of 4096 x 4096 to 224.  The two calls do not make the same files: the new one makes Pillow's.

One JSON line on stdout and, with --out, in a file.  Fails without a GPU."""
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


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5), "n": len(xs)}


def reduce_workload(ctx, n, w, h, factors, warmup, repeat):
    from jpegdec_amd.binding import Output
    lib = ctx.lib
    lib.jda_internal_reduce_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(Output), C.c_int32,
                                             C.POINTER(C.c_float)]
    lib.jda_internal_copy_time.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_float)]
    pitch = (w * 4 + 15) & ~15
    surf = (pitch * h + 255) & ~255
    src_mem, copy_mem = ctx.malloc(surf * n), ctx.malloc(surf * n)
    one = np.random.RandomState(17).randint(0, 256, surf).astype(np.uint8)
    for i in range(n):
        ctx.from_host(src_mem + i * surf, one)
    src = (Output * n)(*[Output(src_mem + i * surf, pitch, w, h) for i in range(n)])
    res = {}
    try:
        for f in factors:
            ow, oh = -(-w // f), -(-h // f)
            opitch = (ow * 4 + 15) & ~15
            osurf = (opitch * oh + 255) & ~255
            dst_mem = ctx.malloc(osurf * n)
            dst = (Output * n)(*[Output(dst_mem + i * osurf, opitch, ow, oh) for i in range(n)])
            fac = (C.c_int32 * (2 * n))(*([f, f] * n))
            t_reduce, t_copy = [], []
            try:
                for k in range(warmup + repeat):
                    out = (C.c_float * 1)()
                    ctx.check(lib.jda_internal_reduce_time(ctx.handle, n, src, 4, fac, None, dst, 1, out), "jda_internal_reduce_time")
                    if k >= warmup:
                        t_reduce.append(out[0])
                    ctx.check(lib.jda_internal_copy_time(ctx.handle, copy_mem, src_mem, surf * n, 1, out), "jda_internal_copy_time")
                    if k >= warmup:
                        t_copy.append(out[0])
            finally:
                ctx.free(dst_mem)
            read = n * w * h * 4
            med, cmed = statistics.median(t_reduce), statistics.median(t_copy)
            res["factor_%d" % f] = {"out_w": ow, "out_h": oh, "source_bytes": read, "reduce": dict(stats(t_reduce), gbps=round(read / (med * 1e-3) / 1e9, 1)),
                                    "copy_of_the_sources": dict(stats(t_copy), gbps_read=round(surf * n / (cmed * 1e-3) / 1e9, 1)), "reduce_over_copy_time": round(med / cmed, 3)}
    finally:
        ctx.free(src_mem)
        ctx.free(copy_mem)
    return {"images": n, "w": w, "h": h, "format": "RGB8888", **res}


def thumbnails_workload(J, ctx, n, w, h, size, warmup, repeat):
    from jpegdec_amd.synth import synth_jpeg
    files = [synth_jpeg(w, h, "4:2:0", seed=91)] * n
    old, new = [], []
    for k in range(warmup + repeat):
        for kw, into in ((dict(resample="bicubic"), old), (dict(resample="bicubic", pillow=True), new)):
            t0 = time.perf_counter()
            out = J.thumbnails(ctx, files, (size, size), quality=75, **kw)          # (returns once the files are on the host)
            ms = (time.perf_counter() - t0) * 1e3
            assert len(out) == n
            if k >= warmup:
                into.append(ms)
    plan = J.thumbnail_plan(w, h, (size, size), J.binding.RESIZE_BICUBIC, 2.0)
    return {"files": n, "w": w, "h": h, "size": size, "plan": {k: plan[k] for k in ("out", "scale", "factors", "reduced")}, "thumbnails": stats(old),
            "thumbnails_pillow": stats(new), "pillow_over_plain_time": round(statistics.median(new) / statistics.median(old), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--files-720", type=int, default=1024)
    ap.add_argument("--files-4096", type=int, default=64)
    ap.add_argument("--skip-thumbnails", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import jpegdec_amd as J
    ctx = J.Context(0)
    try:
        res = {"what": "thumbnail_bench", "reduce_4096": reduce_workload(ctx, 64, 4096, 4096, (2, 4, 8), a.warmup, a.repeat)}
        if not a.skip_thumbnails:
            res["thumbnails_1280x720_to_128"] = thumbnails_workload(J, ctx, a.files_720, 1280, 720, 128, 1, max(3, a.repeat // 2))
            res["thumbnails_4096_to_224"] = thumbnails_workload(J, ctx, a.files_4096, 4096, 4096, 224, 1, max(3, a.repeat // 2))
    finally:
        ctx.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a").write(line + "\n")


if __name__ == "__main__":
    main()
