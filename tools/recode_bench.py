#!/usr/bin/env python3
"""Times of jda_recode_images on the GPU against the road through pixels, in one process on the same resident images: 64 files of 4096 x 4096
and 1,024 thumbnails of 256 x 256, 4:2:0 at quality 75 (the workloads of profiles/encode_opt_bench.json), recoded to optimised and to
progressive files.

The source is Pillow's baseline file of one smooth-plus-noise picture per workload, prepared with the device pre-scan and uploaded n times.
Warm-up rounds first, every figure the median of --repeat rounds with min and max beside it, all between the context's two timer events:
  recode        jda_recode_images as a caller sees it (its launches and the host's looks at the sizes between them);
  pixel_road    jda_batch_decode of the same images to RGB8888 surfaces + jda_encode_surfaces_ex (JDA_ENCODE_OPTIMIZE) / jda_encode_surfaces_progressive
                of those surfaces: what jda_transcode_to_host* runs for every file, here over the whole batch (the decode's launch plan is
                made before the first event);
  stages        the optimised recode through jda_internal_recode_time and the optimised encode through jda_internal_encode_time_ex, every
                launch on its own: `extract` (jda_rc_extract) beside `blocks` (jda_encode_blocks), the stage it replaces.
The output sizes ride along: the recoded files are the source's coefficients, the pixel road's are not (it quantises again).
One JSON line on stdout and, with --out FILE (profiles/recode_bench.json is the place for a run on an MI355X), in a file.  Fails without a GPU.

--transform measures the lossless flip / rotate (jda_recode_images_ex) on the same two workloads instead
(profiles/recode_xf_bench.json is the place for its --out):
  stage         the launch in the place of the blocks stage, through jda_internal_recode_time[_ex]: jda_rc_extract (no transform) beside
                jda_rc_extract_xf under NONE (asked for with the whole grid as the rectangle), FLIP_H and ROT_90;
  call          the whole optimised call as a caller sees it: jda_recode_images beside jda_recode_images_ex under NONE, FLIP_H and ROT_90;
  pixel_road    jda_batch_decode + jda_orient_surfaces (orientation 2 / 6) + jda_encode_surfaces_ex (JDA_ENCODE_OPTIMIZE) of the turned surfaces."""
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

from tools.encode_bench import OPT_STAGES, picture, stats      # noqa: E402


def source_file(w, h):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(picture(w, h)[..., :3])).save(b, "JPEG", quality=75, subsampling=2)
    return b.getvalue()


def workload(J, ctx, n, w, h, warmup, repeat):
    from jpegdec_amd.binding import EncodeJob, Output, RecodeJob, RecodeSource
    jpeg = source_file(w, h)
    prepared = J.prepare_batch([jpeg] * n, device_prescan=True)
    images = J.upload_batch(ctx, prepared)
    g = prepared[0].geometry(J.RGB8888, 0)
    pitch = g["canvas_w"] * 4
    surf = (pitch * g["canvas_h"] + 255) & ~255
    cap = 2 * len(jpeg) + 65536                        # (far below the bounds, far above any file of this picture: a file that did not fit would fail the run)
    canvases, dst = ctx.malloc(surf * n), ctx.malloc(cap * n)
    res = {"images": n, "width": w, "height": h, "source_file_bytes": len(jpeg) * n, "index_on_device": all(im.prescan_on_device for im in images)}
    try:
        outs = [(canvases + k * surf, pitch, g["canvas_w"], g["canvas_h"]) for k in range(n)]
        batch = J.Batch(ctx, images, outs, [J.RGB8888] * n, [0] * n)
        srcs = [(canvases + k * surf, pitch, w, h) for k in range(n)]
        ejobs = [(0, 0, w, h, "4:2:0", 75, 0)] * n
        dsts, caps = [dst + k * cap for k in range(n)], [cap] * n
        for form in ("optimize", "progressive"):
            rc_ms, px_ms, rc_bytes, px_bytes = [], [], None, None
            for r in range(warmup + repeat):
                ctx.timer_start()
                rc_bytes, status = J.recode_images(ctx, images, [(form, 0 if form == "optimize" else None)] * n, dsts, caps)
                ctx.timer_stop()
                assert not any(status), status[:4]
                t_rc = ctx.timer_elapsed_ms()
                ctx.timer_start()
                batch.decode()
                if form == "optimize":
                    px_bytes, status = J.encode_surfaces(ctx, srcs, 4, ejobs, dsts, caps, [J.ENCODE_OPTIMIZE] * n)
                else:
                    px_bytes, status = J.encode_surfaces_progressive(ctx, srcs, 4, ejobs, dsts, caps)
                ctx.timer_stop()
                assert not any(status), status[:4]
                if r >= warmup:
                    rc_ms.append(t_rc)
                    px_ms.append(ctx.timer_elapsed_ms())
            res[form] = {"recode": stats(rc_ms), "pixel_road": stats(px_ms), "recode_over_pixel_road": round(statistics.median(rc_ms) / statistics.median(px_ms), 4),
                         "recode_file_bytes": int(sum(rc_bytes)), "recode_file_bytes_over_source": round(sum(rc_bytes) / (len(jpeg) * n), 4),
                         "pixel_road_file_bytes": int(sum(px_bytes))}
        # the launches one by one: the optimised recode beside the optimised encode of the decoded surfaces
        lib = ctx.lib
        lib.jda_internal_recode_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RecodeSource), C.POINTER(RecodeJob), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        lib.jda_internal_encode_time_ex.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(EncodeJob), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
                                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        rs = (RecodeSource * n)(*[RecodeSource(im.handle, None) for im in images])
        rj = (RecodeJob * n)(*[RecodeJob(J.RECODE_OPTIMIZE, 0, 0, 0)] * n)
        so = (Output * n)(*[Output(*o) for o in srcs])
        sj = (EncodeJob * n)(*[EncodeJob(0, 0, w, h, J.ENCODE_420, 75, 0, 0)] * n)
        sf = (C.c_uint32 * n)(*[J.ENCODE_OPTIMIZE] * n)
        sd, sc, sb, ss = (C.c_void_p * n)(*dsts), (C.c_int64 * n)(*caps), (C.c_int64 * n)(), (C.c_int32 * n)()
        rows_rc, rows_px = [], []
        for r in range(warmup + repeat):
            a, b = (C.c_float * len(OPT_STAGES))(), (C.c_float * len(OPT_STAGES))()
            ctx.check(lib.jda_internal_recode_time(ctx.handle, n, rs, rj, sd, sc, sb, ss, a), "jda_internal_recode_time")
            assert not any(ss)
            ctx.check(lib.jda_internal_encode_time_ex(ctx.handle, n, so, 4, sj, sf, sd, sc, sb, ss, b), "jda_internal_encode_time_ex")
            assert not any(ss)
            if r >= warmup:
                rows_rc.append(list(a))
                rows_px.append(list(b))
        names = ("extract",) + OPT_STAGES[1:]
        res["stages_recode_optimize"] = {name: stats([row[k] for row in rows_rc]) for k, name in enumerate(names)}
        res["stages_encode_optimize"] = {name: stats([row[k] for row in rows_px]) for k, name in enumerate(OPT_STAGES)}
        res["extract_over_blocks"] = round(res["stages_recode_optimize"]["extract"]["median_ms"] / res["stages_encode_optimize"]["blocks"]["median_ms"], 4)
        batch.close()
    finally:
        ctx.free(canvases)
        ctx.free(dst)
        for im in images:
            im.close()
        for p in prepared:
            p.close()
    return res


XF_CASES = (("none", None), ("flip_h", 2), ("rot90", 6))      # (operation, the EXIF orientation that makes the same turn on the pixel road)


def xf_workload(J, ctx, n, w, h, warmup, repeat):
    from jpegdec_amd.binding import RecodeJob, RecodeSource, RecodeXform
    jpeg = source_file(w, h)
    prepared = J.prepare_batch([jpeg] * n, device_prescan=True)
    images = J.upload_batch(ctx, prepared)
    info = images[0].info
    g = prepared[0].geometry(J.RGB8888, 0)
    pitch = g["canvas_w"] * 4
    surf = (pitch * g["canvas_h"] + 255) & ~255
    cap = 2 * len(jpeg) + 65536
    canvases, turned, dst = ctx.malloc(surf * n), ctx.malloc(surf * n), ctx.malloc(cap * n)
    res = {"images": n, "width": w, "height": h, "source_file_bytes": len(jpeg) * n, "index_on_device": all(im.prescan_on_device for im in images)}
    try:
        outs = [(canvases + k * surf, pitch, g["canvas_w"], g["canvas_h"]) for k in range(n)]
        batch = J.Batch(ctx, images, outs, [J.RGB8888] * n, [0] * n)
        dsts, caps = [dst + k * cap for k in range(n)], [cap] * n
        jobs = [("optimize", 0)] * n
        whole = (0, 0, info.mcus_x, info.mcus_y)
        lib = ctx.lib
        head = [C.c_void_p, C.c_int32, C.POINTER(RecodeSource), C.POINTER(RecodeJob)]
        tail = [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        lib.jda_internal_recode_time.argtypes = head + tail
        lib.jda_internal_recode_time_ex.argtypes = head + [C.POINTER(RecodeXform)] + tail
        rs = (RecodeSource * n)(*[RecodeSource(im.handle, None) for im in images])
        rj = (RecodeJob * n)(*[RecodeJob(J.RECODE_OPTIMIZE, 0, 0, 0)] * n)
        sd, sc, sb, ss = (C.c_void_p * n)(*dsts), (C.c_int64 * n)(*caps), (C.c_int64 * n)(), (C.c_int32 * n)()
        cases = [("plain", None, None)] + [(op, J.recode_xform(op, whole if op == "none" else None), o) for op, o in XF_CASES]
        stage, call, road, sizes = {}, {}, {}, {}
        setup = []
        for name, xf, orientation in cases:
            xs = None if xf is None else (RecodeXform * n)(*[xf] * n)
            tsrc = tdst = ejobs = None
            if orientation is not None:
                tw, th = (h, w) if orientation >= 5 else (w, h)
                tsrc = [(canvases + k * surf, pitch, w, h) for k in range(n)]
                tdst = [(turned + k * surf, ((tw * 4 + 15) & ~15), tw, th) for k in range(n)]
                ejobs = [(0, 0, tw, th, "4:2:0", 75, 0)] * n
            setup.append((name, xs, orientation, tsrc, tdst, ejobs))
            stage[name], call[name], road[name] = [], [], []
        for r in range(warmup + repeat):                    # the cases take turns inside a round, the first one another each round: drift hits all alike
            for name, xs, orientation, tsrc, tdst, ejobs in setup[r % len(setup):] + setup[:r % len(setup)]:
                a = (C.c_float * len(OPT_STAGES))()
                if xs is None:
                    ctx.check(lib.jda_internal_recode_time(ctx.handle, n, rs, rj, sd, sc, sb, ss, a), "jda_internal_recode_time")
                else:
                    ctx.check(lib.jda_internal_recode_time_ex(ctx.handle, n, rs, rj, xs, sd, sc, sb, ss, a), "jda_internal_recode_time_ex")
                assert not any(ss), list(ss)[:4]
                ctx.timer_start()
                nbytes, status = J.recode_images(ctx, images, jobs, dsts, caps, xs)
                ctx.timer_stop()
                assert not any(status), status[:4]
                t_call = ctx.timer_elapsed_ms()
                sizes[name] = int(sum(nbytes))
                if orientation is not None:
                    ctx.timer_start()
                    batch.decode()
                    J.orient_surfaces(ctx, tsrc, 4, [orientation] * n, tdst)
                    px_bytes, status = J.encode_surfaces(ctx, tdst, 4, ejobs, dsts, caps, [J.ENCODE_OPTIMIZE] * n)
                    ctx.timer_stop()
                    assert not any(status), status[:4]
                    if r >= warmup:
                        road[name].append(ctx.timer_elapsed_ms())
                if r >= warmup:
                    stage[name].append(a[0])
                    call[name].append(t_call)
        stage, call, road = {k: stats(v) for k, v in stage.items()}, {k: stats(v) for k, v in call.items()}, {k: stats(v) for k, v in road.items() if v}
        res["stage"], res["call_optimize"], res["pixel_road_optimize"], res["file_bytes"] = stage, call, road, sizes
        res["stage_over_plain_extract"] = {k: round(stage[k]["median_ms"] / stage["plain"]["median_ms"], 4) for k, _ in XF_CASES}
        res["call_over_plain_recode"] = {k: round(call[k]["median_ms"] / call["plain"]["median_ms"], 4) for k, _ in XF_CASES}
        res["call_over_pixel_road"] = {k: round(call[k]["median_ms"] / road[k]["median_ms"], 4) for k in road}
        batch.close()
    finally:
        ctx.free(canvases)
        ctx.free(turned)
        ctx.free(dst)
        for im in images:
            im.close()
        for p in prepared:
            p.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="an eighth of the images (a first look)")
    ap.add_argument("--transform", action="store_true", help="the lossless flip / rotate against the plain recode and the pixel road")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    div = 8 if args.small else 1
    shapes = {"large": (64 // div, 4096, 4096), "thumbnails": (1024 // div, 256, 256)}
    import jpegdec_amd as J
    ctx = J.Context(0)
    try:
        res = {"tool": "tools/recode_bench.py %s--repeat %d" % ("--transform " if args.transform else "", args.repeat), "sampling": "4:2:0", "quality": 75, "warmup": args.warmup}
        for name, (n, w, h) in shapes.items():
            res[name] = (xf_workload if args.transform else workload)(J, ctx, n, w, h, args.warmup, args.repeat)
    finally:
        ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
