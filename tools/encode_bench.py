#!/usr/bin/env python3
"""Times of jda_encode_surfaces on the GPU: 64 surfaces of 4096 x 4096 and 1,024 thumbnails of 256 x 256, RGB8888 -> 4:2:0 at quality 75.

The surfaces are one smooth-plus-noise picture per workload, copied n times (every job reads its own copy).  Two kinds of rounds alternate,
warm-up rounds first, each figure the median of --repeat rounds with min and max beside it:
  call    jda_encode_surfaces as a caller sees it -- the seven launches AND the host's look at the sizes between its halves -- between the
          context's two timer events (hipEvents on its stream);
  stages  the same call through jda_internal_encode_time, every one of the seven launches between those two events on its own: kernel time
          per stage.  Beside each: the bytes the stage reads and writes (the table of DESIGN.md 5.13 with this run's block, chunk and file
          counts) and the fraction of the HBM roofline (--hbm-gbps, default 8000) those bytes over that stage's time imply.
Where Pillow is present the same pictures are saved by Image.save(quality=75, subsampling=2) on --cpus processes (default 16) for comparison:
in freshly SPAWNED processes that never open the GPU, before this process creates its context.  equals_pillow: the first and the last file
of the timed size are one file, and its entropy-coded bytes are Pillow's for the same picture.
--optimize adds a leg per workload: the same jobs through jda_encode_surfaces_ex with JDA_ENCODE_OPTIMIZE on every job (Pillow's optimize=True) --
the call as a caller sees it beside the standard call of the same round, its nine launches one by one through jda_internal_encode_time_ex
(gather and the second lengths pass are the two new ones), the host's step between those two (the copy of 2,176 bytes of counts per job, the
wait, the tables, their upload: wall time) and the files' sizes.  profiles/encode_opt_bench.json is the place for such a run on an MI355X.
--no-pillow leaves the Pillow comparison out.
One JSON line on stdout and, with --out FILE (profiles/encode_bench.json is the place for a run on an MI355X), in a file.  Fails without a GPU."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def picture(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.RandomState(3)
    a = np.stack([(xx * 255 // max(w - 1, 1)), (128 + 100 * np.sin(xx / 37.0) * np.cos(yy / 23.0)), (yy * 255 // max(h - 1, 1)), xx * 0 + 255], -1)
    return np.clip(a + rng.randint(-6, 7, a.shape), 0, 255).astype(np.uint8)


def _pillow_one(args):
    from PIL import Image
    rgb, reps = args
    im = Image.fromarray(rgb)
    for _ in range(reps):
        b = io.BytesIO()
        im.save(b, "JPEG", quality=75, subsampling=2, optimize=False)
    return len(b.getvalue())


def entropy_coded(jpeg):
    """the bytes behind the SOS header"""
    i = jpeg.index(b"\xff\xda")
    return jpeg[i + 2 + ((jpeg[i + 2] << 8) | jpeg[i + 3]):]


def pillow_file(img):
    try:
        from PIL import Image
    except ImportError:
        return None
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., :3])).save(b, "JPEG", quality=75, subsampling=2, optimize=False)
    return b.getvalue()


def pillow_ms(img, n, cpus):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return None
    import multiprocessing as mp
    rgb = np.ascontiguousarray(img[..., :3])
    per = [n // cpus + (1 if k < n % cpus else 0) for k in range(cpus)]
    with mp.get_context("spawn").Pool(cpus) as pool:      # (never a fork: no child inherits anything of a HIP runtime)
        pool.map(_pillow_one, [(rgb, 1)] * cpus)          # warm-up
        t0 = time.perf_counter()
        pool.map(_pillow_one, [(rgb, p) for p in per if p])
        return round((time.perf_counter() - t0) * 1e3, 2)


STAGES = ("blocks", "lengths", "scan_bits", "emit", "count", "scan_bytes", "write")
OPT_STAGES = STAGES + ("gather", "huffopt_lengths", "host_between_gather_and_lengths")      # jda_internal_encode_time_ex: ids 7 and 8, then the host's step


def workload(J, ctx, n, w, h, warmup, repeat, hbm_gbps, pillow, want, optimize=False):
    import ctypes as C
    from jpegdec_amd.binding import EncodeJob, Output
    img = picture(w, h)
    pitch = w * 4
    surf = (pitch * h + 255) & ~255
    cap = J.encode_bound(w, h, "4:2:0", 0)
    src, dst = ctx.malloc(surf * n), ctx.malloc(cap * n)
    try:
        for k in range(n):
            ctx.from_host(src + k * surf, img.reshape(-1))
        srcs = [(src + k * surf, pitch, w, h) for k in range(n)]
        jobs = [(0, 0, w, h, "4:2:0", 75, 0)] * n
        dsts, caps = [dst + k * cap for k in range(n)], [cap] * n
        ms, per_stage, nbytes = [], [], None
        so = (Output * n)(*[Output(*o) for o in srcs])
        sj = (EncodeJob * n)(*[EncodeJob(0, 0, w, h, J.ENCODE_420, 75, 0, 0)] * n)
        sd, sc = (C.c_void_p * n)(*dsts), (C.c_int64 * n)(*caps)
        sb, ss = (C.c_int64 * n)(), (C.c_int32 * n)()
        ctx.lib.jda_internal_encode_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(EncodeJob), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                     C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        ctx.lib.jda_internal_encode_time_ex.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(EncodeJob), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
                                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        sf = (C.c_uint32 * n)(*[J.ENCODE_OPTIMIZE] * n)
        opt_ms, opt_stage, opt_bytes = [], [], None
        first = None
        for r in range(warmup + repeat):
            ctx.timer_start()
            nbytes, status = J.encode_surfaces(ctx, srcs, 4, jobs, dsts, caps)
            ctx.timer_stop()
            assert not any(status)
            t = ctx.timer_elapsed_ms()
            st = (C.c_float * len(STAGES))()
            ctx.check(ctx.lib.jda_internal_encode_time(ctx.handle, n, so, 4, sj, sd, sc, sb, ss, st), "jda_internal_encode_time")
            assert list(sb) == nbytes and not any(ss)
            if r >= warmup:
                ms.append(t)
                per_stage.append(list(st))
            if optimize:                                   # (behind the standard call of the same round; the files are overwritten)
                ctx.timer_start()
                opt_bytes, status = J.encode_surfaces(ctx, srcs, 4, jobs, dsts, caps, [J.ENCODE_OPTIMIZE] * n)
                ctx.timer_stop()
                assert not any(status)
                t = ctx.timer_elapsed_ms()
                st = (C.c_float * len(OPT_STAGES))()
                ctx.check(ctx.lib.jda_internal_encode_time_ex(ctx.handle, n, so, 4, sj, sf, sd, sc, sb, ss, st), "jda_internal_encode_time_ex")
                assert list(sb) == opt_bytes and not any(ss)
                if r >= warmup:
                    opt_ms.append(t)
                    opt_stage.append(list(st))
        if optimize:
            nbytes, status = J.encode_surfaces(ctx, srcs, 4, jobs, dsts, caps)      # (the standard files once more, for the comparison below)
        first, last = (ctx.to_host(dsts[k], nbytes[k]).tobytes() for k in (0, n - 1))
    finally:
        ctx.free(src)
        ctx.free(dst)
    mcus = n * ((w + 15) // 16) * ((h + 15) // 16)
    blocks = mcus * 6
    files = int(sum(nbytes))
    chunks = files // 64 + n * 11
    stage_bytes = {                                    # (read, written): DESIGN.md 5.13
        "blocks": (mcus * (4 * 256 + 2 * 1024), blocks * 132),                             # an MCU: four luma blocks of 256 B of pixels, Cb and Cr 1 KiB each
        "lengths": (blocks * 8, blocks * 4),
        "scan_bits": (blocks * 8, blocks * 8),
        "emit": (blocks * 140, files),
        "count": (files, chunks * 4),
        "scan_bytes": (chunks * 8, chunks * 8),
        "write": (files + chunks * 12, files),
    }
    total = sum(a + b for a, b in stage_bytes.values())
    med = statistics.median(ms)
    stages = {}
    for k, name in enumerate(STAGES):
        st = stats([row[k] for row in per_stage])
        rd, wr = stage_bytes[name]
        st.update(bytes_read=rd, bytes_written=wr, hbm_roofline_fraction=round((rd + wr) / (st["median_ms"] * 1e-3) / (hbm_gbps * 1e9), 4) if st["median_ms"] > 0 else None)
        stages[name] = st
    opt = None
    if optimize:
        opt = {"call": stats(opt_ms), "call_over_standard": round(statistics.median(opt_ms) / med, 4), "file_bytes": int(sum(opt_bytes)),
               "file_bytes_over_standard": round(sum(opt_bytes) / files, 4), "histogram_bytes_copied": n * 2176,
               "stages": {name: stats([row[k] for row in opt_stage]) for k, name in enumerate(OPT_STAGES)}}
        opt["kernel_ms_new_stages"] = round(opt["stages"]["gather"]["median_ms"] + opt["stages"]["huffopt_lengths"]["median_ms"], 4)
    return {"images": n, "width": w, "height": h, "optimize": opt, "call": stats(ms), "megapixels_per_s": round(n * w * h / med / 1e3, 1), "file_bytes": files, "blocks": blocks,
            "stages": stages, "kernel_ms_all_stages": round(sum(v["median_ms"] for v in stages.values()), 4), "bytes_all_stages": total, "pillow": pillow,
            "equals_pillow": "Pillow is not installed" if want is None else bool(first == last and entropy_coded(first) == entropy_coded(want))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--small", action="store_true", help="an eighth of the images (a first look)")
    ap.add_argument("--optimize", action="store_true", help="add the JDA_ENCODE_OPTIMIZE leg")
    ap.add_argument("--no-pillow", action="store_true", help="leave the Pillow comparison out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    div = 8 if args.small else 1
    shapes = {"large": (64 // div, 4096, 4096), "thumbnails": (1024 // div, 256, 256)}
    # Pillow first, in spawned processes, while this process has not touched the GPU: no child ever holds it
    pillow, files = {}, {}
    for name, (n, w, h) in shapes.items():
        p = None if args.no_pillow else pillow_ms(picture(w, h), n, args.cpus)
        pillow[name] = {"cpus": args.cpus, "ms": p} if p is not None else "left out" if args.no_pillow else "Pillow is not installed"
        files[name] = pillow_file(picture(w, h))
    import jpegdec_amd as J
    ctx = J.Context(0)
    try:
        res = {"tool": "tools/encode_bench.py", "sampling": "4:2:0", "quality": 75}
        for name, (n, w, h) in shapes.items():
            res[name] = workload(J, ctx, n, w, h, args.warmup, args.repeat, args.hbm_gbps, pillow[name], files[name], args.optimize)
    finally:
        ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
