#!/usr/bin/env python3
"""Times of jda_encode_surfaces_progressive on the GPU beside the optimised baseline call of the same session: the two workloads of
tools/encode_bench.py (64 surfaces of 4096 x 4096 and 1,024 thumbnails of 256 x 256, RGB8888 -> 4:2:0 at quality 75, its pictures).

Per round, warm-up rounds first, each figure the median of --repeat rounds with min and max beside it:
  optimised     jda_encode_surfaces_ex with JDA_ENCODE_OPTIMIZE on every job, as a caller sees it (the yardstick);
  progressive   jda_encode_surfaces_progressive as a caller sees it -- eleven launches and the host's two steps between its parts;
  stages        the same call through jda_internal_progenc_time: every launch between the context's two timer events on its own, and the
                host's two steps together (the copies back, the waits, the tables, the placement, the uploads: wall time).
The files' bytes against the optimised baseline files'; equals_pillow: the first and the last file are one file and, from SOF2 on, Pillow's
Image.save(quality=75, subsampling=2, progressive=True) for the same picture.
flat: ONE flat 4096 x 4096 image -- every AC scan one stretch of 262,144 (luma) or 65,536 units that a single lane of the resolve stage walks.
One JSON line on stdout and, with --out FILE (profiles/encode_prog_bench.json is the place for a run on an MI355X), in a file.  Fails without a GPU."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from encode_bench import picture, stats  # noqa: E402

STAGES = ("blocks", "dc_lengths", "classify", "resolve", "gather", "lengths", "scan_bits", "emit", "count", "scan_bytes", "write", "host_steps")
NEW = ("classify", "resolve", "gather", "lengths", "scan_bits", "emit", "count", "scan_bytes", "write")


def pillow_file(img):
    try:
        from PIL import Image
    except ImportError:
        return None
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., :3])).save(b, "JPEG", quality=75, subsampling=2, progressive=True)
    return b.getvalue()


def workload(J, ctx, n, w, h, warmup, repeat, img, yardstick=True):
    from jpegdec_amd.binding import EncodeJob, Output
    pitch = w * 4
    surf = (pitch * h + 255) & ~255
    cap = J.encode_bound_progressive(w, h, "4:2:0")
    src, dst = ctx.malloc(surf * n), ctx.malloc(cap * n)
    try:
        for k in range(n):
            ctx.from_host(src + k * surf, img.reshape(-1))
        srcs = [(src + k * surf, pitch, w, h) for k in range(n)]
        jobs = [(0, 0, w, h, "4:2:0", 75, 0)] * n
        dsts, caps = [dst + k * cap for k in range(n)], [cap] * n
        so = (Output * n)(*[Output(*o) for o in srcs])
        sj = (EncodeJob * n)(*[EncodeJob(0, 0, w, h, J.ENCODE_420, 75, 0, 0)] * n)
        sd, sc = (C.c_void_p * n)(*dsts), (C.c_int64 * n)(*caps)
        sb, ss = (C.c_int64 * n)(), (C.c_int32 * n)()
        ctx.lib.jda_internal_progenc_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(EncodeJob), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                      C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        opt_ms, prog_ms, per_stage, opt_bytes, nbytes = [], [], [], None, None
        for r in range(warmup + repeat):
            if yardstick:
                ctx.timer_start()
                opt_bytes, status = J.encode_surfaces(ctx, srcs, 4, jobs, dsts, caps, [J.ENCODE_OPTIMIZE] * n)
                ctx.timer_stop()
                assert not any(status)
                t_opt = ctx.timer_elapsed_ms()
            ctx.timer_start()
            nbytes, status = J.encode_surfaces_progressive(ctx, srcs, 4, jobs, dsts, caps)
            ctx.timer_stop()
            assert not any(status)
            t = ctx.timer_elapsed_ms()
            st = (C.c_float * len(STAGES))()
            ctx.check(ctx.lib.jda_internal_progenc_time(ctx.handle, n, so, 4, sj, sd, sc, sb, ss, st), "jda_internal_progenc_time")
            assert list(sb) == nbytes and not any(ss)
            if r >= warmup:
                prog_ms.append(t)
                per_stage.append(list(st))
                if yardstick:
                    opt_ms.append(t_opt)
        first, last = (ctx.to_host(dsts[k], nbytes[k]).tobytes() for k in (0, n - 1))
    finally:
        ctx.free(src)
        ctx.free(dst)
    want = pillow_file(img)
    stages = {name: stats([row[k] for row in per_stage]) for k, name in enumerate(STAGES)}
    out = {"images": n, "width": w, "height": h, "call": stats(prog_ms), "file_bytes": int(sum(nbytes)), "stages": stages,
           "kernel_ms_new_stages": round(sum(stages[k]["median_ms"] for k in NEW), 4), "kernel_ms_all_stages": round(sum(stages[k]["median_ms"] for k in STAGES[:-1]), 4),
           "megapixels_per_s": round(n * w * h / statistics.median(prog_ms) / 1e3, 1),
           "equals_pillow": "Pillow is not installed" if want is None else bool(first == last and first[first.index(b"\xff\xc2"):] == want[want.index(b"\xff\xc2"):])}
    if yardstick:
        out["optimised_baseline"] = {"call": stats(opt_ms), "file_bytes": int(sum(opt_bytes))}
        out["call_over_optimised"] = round(statistics.median(prog_ms) / statistics.median(opt_ms), 4)
        out["file_bytes_over_optimised"] = round(sum(nbytes) / sum(opt_bytes), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="an eighth of the images (a first look)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    div = 8 if args.small else 1
    import jpegdec_amd as J
    ctx = J.Context(0)
    try:
        res = {"tool": "tools/encode_prog_bench.py", "sampling": "4:2:0", "quality": 75}
        for name, (n, w, h) in {"large": (64 // div, 4096, 4096), "thumbnails": (1024 // div, 256, 256)}.items():
            res[name] = workload(J, ctx, n, w, h, args.warmup, args.repeat, picture(w, h))
        res["flat"] = workload(J, ctx, 1, 4096, 4096, 1, args.repeat, np.full((4096, 4096, 4), 200, dtype=np.uint8), yardstick=False)
    finally:
        ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
