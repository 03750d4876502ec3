#!/usr/bin/env python3
"""Times of the pack pass (jda_pack_tiles) on the GPU next to the decode launch that fills its sources, in one run.

A batch of --batch images of --size x --size pixels (4:2:0, the benchmark's file) is decoded to resident RGB8888 canvases: the decode
launch between the context's two timer events.  The canvases are then packed, all of them in one launch, as U8 HWC, U8 CHW and F32 CHW
(normalise_table) between the same two events (jda_internal_pack_time: the job records go up before the first event).  Rounds alternate
over the three formats and the decode, so that a drift of the clock hits them all alike; warm-up rounds first; each figure is the
median of --repeat rounds with min and max beside it.  bytes = source bytes read (4 a pixel) + destination bytes written; fraction of
8 TB/s = that rate over the HBM peak; ratio to the copy = that rate over the 4.59 TB/s a plain device copy reached (read + write,
profiles/r06_hbm_ceiling.txt).  One JSON line on stdout and, with --out, in a file.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from jpegdec_amd.binding import Output  # noqa: E402
from jpegdec_amd.synth import synth_jpeg  # noqa: E402

HBM_PEAK = 8.0e12
COPY_RATE = 4.59e12          # profiles/r06_hbm_ceiling.txt: "copy grid 4096 x 256 (read + write)"


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    n, size = a.batch, a.size
    ctx = J.Context(0)
    lib = ctx.lib
    lib.jda_internal_pack_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p,
                                           C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_float)]
    jpeg = synth_jpeg(size, size, "4:2:0", seed=91)
    prep = J.PreparedImage(jpeg)
    g = prep.geometry(J.RGB8888, 0)
    pitch = (g["canvas_w"] * 4 + 15) & ~15
    surf = (pitch * g["canvas_h"] + 255) & ~255
    dimg = J.DeviceImage(ctx, prep)
    canvases = ctx.malloc(surf * n)
    px = g["out_w"] * g["out_h"]
    dense_f32 = px * 3 * 4
    dst = ctx.malloc(dense_f32 * n + 16)
    table = np.ascontiguousarray(J.normalise_table((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), np.float32)).view(np.uint8).reshape(-1)
    dtable = ctx.malloc(table.size)
    ctx.from_host(dtable, table)
    batch = J.Batch(ctx, [dimg] * n, [(canvases + i * surf, pitch, g["canvas_w"], g["canvas_h"]) for i in range(n)], [J.RGB8888] * n, [0] * n)
    src = (Output * n)(*[Output(canvases + i * surf, pitch, g["out_w"], g["out_h"]) for i in range(n)])
    formats = {"u8_hwc": (J.PACK_HWC, J.PACK_U8, None, 1), "u8_chw": (J.PACK_CHW, J.PACK_U8, None, 1), "f32_chw": (J.PACK_CHW, J.PACK_F32, dtable, 4)}
    times = {k: [] for k in formats}
    t_decode = []
    try:
        for k in range(a.warmup + a.repeat):
            ctx.timer_start()
            batch.decode()
            ctx.timer_stop()
            ms = ctx.timer_elapsed_ms()
            if k >= a.warmup:
                t_decode.append(ms)
            for name, (layout, elem, tab, es) in formats.items():
                # image i of the batch tensor at its own offset, one byte (one element) off a 16-byte boundary where the sizes allow it
                ptrs = (C.c_void_p * n)(*[dst + es + i * px * 3 * es for i in range(n)])
                out = (C.c_float * 1)()
                ctx.check(lib.jda_internal_pack_time(ctx.handle, n, src, 4, None, layout, elem, tab, ptrs, 1, out), "jda_internal_pack_time")
                if k >= a.warmup:
                    times[name].append(out[0])
    finally:
        batch.close()
        dimg.close()
        prep.close()
        for p in (canvases, dst, dtable):
            ctx.free(p)
        ctx.close()
    res = {"what": "pack_bench", "images": n, "w": g["out_w"], "h": g["out_h"], "source": "RGB8888 canvases of a 4:2:0 batch, decoded in the same run",
           "hbm_peak_tbps": HBM_PEAK / 1e12, "copy_tbps": COPY_RATE / 1e12, "decode_launch": stats(t_decode), "pack": {}}
    for name, (layout, elem, tab, es) in formats.items():
        med = statistics.median(times[name])
        moved = n * px * (4 + 3 * es)
        rate = moved / (med * 1e-3)
        res["pack"][name] = dict(stats(times[name]), bytes_read_plus_written=moved, tbps=round(rate / 1e12, 3), fraction_of_hbm_peak=round(rate / HBM_PEAK, 3),
                                 ratio_to_copy=round(rate / COPY_RATE, 3), ratio_to_decode_launch=round(med / statistics.median(t_decode), 3))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
