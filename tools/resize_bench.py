#!/usr/bin/env python3
"""Times of the resize pass (jda_resize_tiles) on the GPU, next to a plain device copy of the same source bytes, in one run.

Two workloads, RGB8888, every surface a buffer of its own filled with random bytes: 1,024 surfaces of 500 x 375 -> 224 x 224 (a training
loader's batch) and 64 of 4096 x 4096 -> 224 x 224 (thumbnails of large files; more source bytes than the Infinity Cache holds).  The
resize launch runs between the context's two timer events (jda_internal_resize_time: job records and taps go up before the first event),
the copy likewise (jda_internal_copy_time).  Rounds alternate over resize and copy, so that a drift of the clock hits both alike; warm-up
rounds first; each figure is the median of --repeat rounds with min and max beside it.  gbps = SOURCE bytes read (4 a pixel of the box)
over the time; the copy's figure counts the bytes it reads, too.  One JSON line on stdout and, with --out, in a file.
--filter NAME (bilinear, box, hamming, bicubic, lanczos; the default is bilinear through the hook of jda_resize_surfaces itself): Pillow's
filter of that name through jda_internal_resize_time_ex -- BICUBIC and LANCZOS run the signed instances, with 2 and 3 times the taps.

--tensors: decode_to_tensors(size=(224, 224)) against the same call without size, wall clock around the call and a device
synchronisation, --batch files of 500 x 375 (4:2:0), alternating, median of --repeat.  torch is imported first (jpegdec_amd/tensors.py).
Fails without a GPU."""
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


def kernel_workload(J, ctx, n, w, h, ow, oh, warmup, repeat, filt=0):
    from jpegdec_amd.binding import Output
    lib = ctx.lib
    lib.jda_internal_resize_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.POINTER(Output), C.c_int32, C.POINTER(C.c_float)]
    lib.jda_internal_resize_time_ex.argtypes = lib.jda_internal_resize_time.argtypes[:6] + [C.c_int32] + lib.jda_internal_resize_time.argtypes[6:]
    lib.jda_internal_copy_time.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_float)]
    pitch, opitch = (w * 4 + 15) & ~15, (ow * 4 + 15) & ~15
    surf, osurf = (pitch * h + 255) & ~255, (opitch * oh + 255) & ~255
    src_mem, dst_mem, copy_mem = ctx.malloc(surf * n), ctx.malloc(osurf * n), ctx.malloc(surf * n)
    one = np.random.RandomState(17).randint(0, 256, surf).astype(np.uint8)
    for i in range(n):
        ctx.from_host(src_mem + i * surf, one)
    src = (Output * n)(*[Output(src_mem + i * surf, pitch, w, h) for i in range(n)])
    dst = (Output * n)(*[Output(dst_mem + i * osurf, opitch, ow, oh) for i in range(n)])
    t_resize, t_copy = [], []
    try:
        for k in range(warmup + repeat):
            out = (C.c_float * 1)()
            if filt == 0:
                ctx.check(lib.jda_internal_resize_time(ctx.handle, n, src, 4, None, dst, 1, out), "jda_internal_resize_time")
            else:
                ctx.check(lib.jda_internal_resize_time_ex(ctx.handle, n, src, 4, None, dst, filt, 1, out), "jda_internal_resize_time_ex")
            if k >= warmup:
                t_resize.append(out[0])
            ctx.check(lib.jda_internal_copy_time(ctx.handle, copy_mem, src_mem, surf * n, 1, out), "jda_internal_copy_time")
            if k >= warmup:
                t_copy.append(out[0])
    finally:
        for p in (src_mem, dst_mem, copy_mem):
            ctx.free(p)
    read = n * w * h * 4
    med, cmed = statistics.median(t_resize), statistics.median(t_copy)
    return {"images": n, "w": w, "h": h, "out_w": ow, "out_h": oh, "source_bytes": read, "resize": dict(stats(t_resize), gbps=round(read / (med * 1e-3) / 1e9, 1)),
            "copy_of_the_sources": dict(stats(t_copy), gbps_read=round(surf * n / (cmed * 1e-3) / 1e9, 1)), "resize_over_copy_time": round(med / cmed, 3)}


def tensors_workload(batch, warmup, repeat):
    import torch  # noqa: F401  (before anything loads libjpegdec_amd.so)
    import jpegdec_amd as J
    from jpegdec_amd.synth import synth_jpeg
    ctx = J.Context(0)
    files = [synth_jpeg(500, 375, "4:2:0", seed=91)] * batch
    plain, sized = [], []
    try:
        for k in range(warmup + repeat):
            for kw, into in ((dict(), plain), (dict(size=(224, 224)), sized)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t = J.decode_to_tensors(ctx, files, **kw)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                del t
                if k >= warmup:
                    into.append(ms)
    finally:
        ctx.close()
    return {"what": "resize_bench --tensors", "files": batch, "w": 500, "h": 375, "size": [224, 224], "decode_to_tensors": stats(plain),
            "decode_to_tensors_size": stats(sized), "ratio": round(statistics.median(sized) / statistics.median(plain), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--tensors", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--filter", default="bilinear")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.tensors:
        res = tensors_workload(a.batch, a.warmup, a.repeat)
    else:
        import jpegdec_amd as J
        filt = J.resize_filter(a.filter)
        ctx = J.Context(0)
        try:
            res = {"what": "resize_bench", "format": "RGB8888", "source": "random bytes, a buffer a surface", "filter": a.filter.lower(),
                   "loader_500x375": kernel_workload(J, ctx, 1024, 500, 375, 224, 224, a.warmup, a.repeat, filt),
                   "thumbnail_4096": kernel_workload(J, ctx, 64, 4096, 4096, 224, 224, a.warmup, a.repeat, filt)}
        finally:
            ctx.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a").write(line + "\n")


if __name__ == "__main__":
    main()
