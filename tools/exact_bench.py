#!/usr/bin/env python3
"""Times of the libjpeg-exact decode (jda_exact_decode_surfaces) on the GPU beside jda_batch_decode of the same resident
images, in one process: 64 files of 4096 x 4096, 4:2:0 at quality 75, to RGB8888 surfaces.

The source is Pillow's baseline file of one smooth-plus-noise picture (tools/encode_bench.picture), prepared with the device pre-scan and
uploaded n times; and Pillow's progressive file of the same picture as a coefficient image (jda_progressive_prepare), uploaded n times in the
form JDA_COEF_AUTO picks.  Warm-up rounds first, every figure the median of --repeat rounds with min and max beside it:
  exact_call      jda_exact_decode_surfaces as a caller sees it, between the context's two timer events (plan, blob copy, launches, wait);
  stages          the same call through jda_internal_exact_time, its launches between events of their own: planes, colour;
  batch_decode    jda_batch_decode of the baseline images to the same surfaces (the launch plan made before the first event).
By bytes the exact road moves about 7 B a pixel (planes written 1.5, read 1.5, RGB8888 written 4) where the decode kernel writes 4.
--scale 2,4,8: the scaled decode instead -- jda_exact_decode_surfaces_scaled of the same resident images at each scale named
and at scale 1, all in the same rounds: the call, and its planes / colour launches through jda_internal_exact_time_scaled; no batch_decode
leg.  profiles/exact_scaled_bench.json is the place for that run.
--rect: the rectangle decode instead -- each resident baseline image with a fixed-seed random-resized-crop rectangle (area
8 % to 100 % of the image, aspect 3/4 to 4/3) through jda_exact_decode_surfaces_rect, beside jda_exact_decode_surfaces of the same images
and beside a rectangle EQUAL to the whole image and one that leaves out its first column and row (the new colour kernel over every pixel,
aligned and with every read unaligned: its price against jda_exact_colour), all in the same rounds; per leg the call and its planes / colour launches (jda_internal_exact_time_rect), the planes
tiles launched against those of the whole images, and the bytes the stages move.  profiles/exact_rect_bench.json is the place for that run.
Nothing here is a gate.
One JSON line on stdout and, with --out FILE (profiles/exact_bench.json is the place for a run on an MI355X), in a file.  Fails without a GPU."""
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

from tools.encode_bench import picture, stats      # noqa: E402


def files(w, h):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(picture(w, h)[..., :3]))
    out = []
    for kw in ({}, dict(progressive=True)):
        b = io.BytesIO()
        im.save(b, "JPEG", quality=75, subsampling=2, **kw)
        out.append(b.getvalue())
    return out


def scaled(ctx, J, a, n, w, h, images, coefs, outs, res):
    """--scale: every scale of a.scale and scale 1 in the same rounds, per road: the call and its two stages"""
    from jpegdec_amd.binding import Output, RecodeSource
    lib = ctx.lib
    lib.jda_internal_exact_time_scaled.restype = C.c_int
    lib.jda_internal_exact_time_scaled.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    so = (Output * n)(*[Output(*o) for o in outs])
    st = (C.c_int32 * n)()
    roads = {"baseline": (images, (RecodeSource * n)(*[RecodeSource(im.handle, None) for im in images])),
             "coefficients": (coefs, (RecodeSource * n)(*[RecodeSource(None, d.handle) for d in coefs]))}
    scales = [1] + [s for s in a.scale if s != 1]
    call = {(k, s): [] for k in roads for s in scales}
    stages = {(k, s): [] for k in roads for s in scales}
    for r in range(a.warmup + a.repeat):
        for name, (items, rs) in roads.items():
            for s in scales:
                ctx.timer_start()
                status = J.exact_decode(ctx, items, outs, None, [s] * n)
                ctx.timer_stop()
                assert not any(status), status[:4]
                t_call = ctx.timer_elapsed_ms()
                ms = (C.c_float * 2)()
                ctx.check(lib.jda_internal_exact_time_scaled(ctx.handle, n, rs, so, None, (C.c_int32 * n)(*[s] * n), st, ms), "jda_internal_exact_time_scaled")
                assert not any(st)
                if r >= a.warmup:
                    call[name, s].append(t_call)
                    stages[name, s].append(list(ms))
    for name in roads:
        res[name] = {}
        for s in scales:
            row = {"exact_call": stats(call[name, s]), "stages": {k: stats([x[i] for x in stages[name, s]]) for i, k in enumerate(("planes", "colour"))}}
            row["call_over_scale_1"] = round(statistics.median(call[name, s]) / statistics.median(call[name, 1]), 3)
            res[name]["scale_%d" % s] = row


def crop_rects(n, w, h, seed=20):
    """torchvision's RandomResizedCrop boxes: area 8 % .. 100 % of the image, log-uniform aspect 3/4 .. 4/3, fixed seed"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        area = w * h * rng.uniform(0.08, 1.0)
        aspect = float(np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3))))
        cw, ch = int(round(np.sqrt(area * aspect))), int(round(np.sqrt(area / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            out.append((int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch))
    return out


def rect(ctx, J, a, n, w, h, images, outs, res, file):
    """--rect: whole images, random crops and a rectangle equal to the image in the same rounds: the call and its two stages"""
    from jpegdec_amd.binding import Output, RecodeSource
    lib = ctx.lib
    lib.jda_internal_exact_time_rect.restype = C.c_int
    lib.jda_internal_exact_time_rect.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32,
                                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    rs = (RecodeSource * n)(*[RecodeSource(im.handle, None) for im in images])
    st = (C.c_int32 * n)()
    crops = crop_rects(n, w, h)
    # (.. and the image without its first column and row: every Y dword unaligned, the chroma phase odd, over nearly the same pixels)
    legs = {"whole": None, "crops": crops, "rect_equal_to_image": [(0, 0, w, h)] * n, "rect_from_1_1": [(1, 1, w - 1, h - 1)] * n}
    per, mw, mh = 10, 16, 16                                             # a 4:2:0 tile: 10 MCUs of 16 x 16 pixels
    whole_tiles = n * -(-h // mh) * -(-(-(-w // mw)) // per)
    call = {k: [] for k in legs}
    stages = {k: [] for k in legs}
    for r in range(a.warmup + a.repeat):
        for name, rects in legs.items():
            # (a rectangle's surface holds the rectangle: its pitch is the rectangle's)
            o = outs if rects is None else [(outs[k][0], (rects[k][2] * 4 + 15) & ~15, rects[k][2], rects[k][3]) for k in range(n)]
            so = (Output * n)(*[Output(*q) for q in o])
            flat = None if rects is None else (C.c_int32 * (4 * n))(*[v for q in rects for v in q])
            ctx.timer_start()
            status = J.exact_decode(ctx, images, o, None, None, False, rects=rects) if rects is not None else J.exact_decode(ctx, images, o)
            ctx.timer_stop()
            assert not any(status), status[:4]
            t_call = ctx.timer_elapsed_ms()
            ms = (C.c_float * 2)()
            ctx.check(lib.jda_internal_exact_time_rect(ctx.handle, n, rs, so, None, None, 0, flat, st, ms), "jda_internal_exact_time_rect")
            assert not any(st)
            if r >= a.warmup:
                call[name].append(t_call)
                stages[name].append(list(ms))
    for name, rects in legs.items():
        row = {"exact_call": stats(call[name]), "stages": {k: stats([x[i] for x in stages[name]]) for i, k in enumerate(("planes", "colour"))}}
        if rects is None:
            tiles, pixels, mcu_pixels = whole_tiles, n * w * h, n * -(-w // mw) * mw * -(-h // mh) * mh
        else:
            tiles = pixels = mcu_pixels = 0
            for q in rects:
                mx0, my0, mx1, my1 = J.exact_rect_mcus(file, q)
                tiles += (my1 - my0) * -(-(mx1 - mx0) // per)
                pixels += q[2] * q[3]
                mcu_pixels += (mx1 - mx0) * (my1 - my0) * mw * mh
        row.update(planes_tiles=tiles, planes_tiles_of_the_whole_images=whole_tiles, pixels=pixels,
                   # 4:2:0: the planes stage writes 1.5 B a pixel of the MCUs it decodes; the colour stage reads 1.5 B and writes 4 B a pixel of the output
                   bytes_moved=int(1.5 * mcu_pixels + 5.5 * pixels), call_over_whole=round(statistics.median(call[name]) / statistics.median(call["whole"]), 3))
        row["colour_ps_per_pixel"] = round(row["stages"]["colour"]["median_ms"] * 1e9 / pixels, 3)
        row["planes_ps_per_mcu_pixel"] = round(row["stages"]["planes"]["median_ms"] * 1e9 / mcu_pixels, 3)
        res[name] = row
    for name in ("crops", "rect_equal_to_image", "rect_from_1_1"):
        res[name]["colour_per_pixel_over_whole"] = round(res[name]["colour_ps_per_pixel"] / res["whole"]["colour_ps_per_pixel"], 3)
    res["crop_area_fraction"] = round(res["crops"]["pixels"] / res["whole"]["pixels"], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--scale", type=lambda v: [int(x) for x in v.split(",")], help="e.g. 2,4,8: the scaled decode at these scales beside scale 1")
    ap.add_argument("--rect", action="store_true", help="random-resized-crop rectangles through jda_exact_decode_surfaces_rect beside the whole images")
    ap.add_argument("--out")
    a = ap.parse_args()
    import jpegdec_amd as J
    from jpegdec_amd.binding import Output, RecodeSource
    ctx = J.Context(0)
    n, w, h = a.images, a.size, a.size
    base_file, prog_file = files(w, h)
    prepared = J.prepare_batch([base_file] * n, device_prescan=True)
    images = J.upload_batch(ctx, prepared)
    host = None if a.rect else J.CoefImage(prog_file)                   # (--rect times the resident baseline images alone)
    coefs = [] if a.rect else [J.DeviceCoef(ctx, host, J.COEF_AUTO) for _ in range(n)]
    g = prepared[0].geometry(J.RGB8888, 0)
    pitch = g["canvas_w"] * 4
    surf = (pitch * g["canvas_h"] + 255) & ~255
    canvases = ctx.malloc(surf * n)
    res = {"images": n, "width": w, "height": h, "pixels": n * w * h, "index_on_device": all(im.prescan_on_device for im in images),
           "coef_form": None if a.rect else "sparse" if coefs[0].form == J.COEF_SPARSE else "dense"}
    try:
        outs = [(canvases + k * surf, pitch, g["canvas_w"], g["canvas_h"]) for k in range(n)]
        if a.rect:
            rect(ctx, J, a, n, w, h, images, outs, res, base_file)
            line = json.dumps(res)
            print(line)
            if a.out:
                with open(a.out, "w") as f:
                    f.write(line + "\n")
            return
        if a.scale:
            res["scales"] = a.scale
            scaled(ctx, J, a, n, w, h, images, coefs, outs, res)
            line = json.dumps(res)
            print(line)
            if a.out:
                with open(a.out, "w") as f:
                    f.write(line + "\n")
            return
        batch = J.Batch(ctx, images, outs, [J.RGB8888] * n, [0] * n)
        lib = ctx.lib
        lib.jda_internal_exact_time.restype = C.c_int
        lib.jda_internal_exact_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        so = (Output * n)(*[Output(*o) for o in outs])
        st = (C.c_int32 * n)()
        roads = {"baseline": (images, (RecodeSource * n)(*[RecodeSource(im.handle, None) for im in images])),
                 "coefficients": (coefs, (RecodeSource * n)(*[RecodeSource(None, d.handle) for d in coefs]))}
        call = {k: [] for k in roads}
        stages = {k: [] for k in roads}
        dec = []
        for r in range(a.warmup + a.repeat):
            for name, (items, rs) in roads.items():
                ctx.timer_start()
                status = J.exact_decode(ctx, items, outs)
                ctx.timer_stop()
                assert not any(status), status[:4]
                t_call = ctx.timer_elapsed_ms()
                ms = (C.c_float * 2)()
                ctx.check(lib.jda_internal_exact_time(ctx.handle, n, rs, so, None, st, ms), "jda_internal_exact_time")
                assert not any(st)
                if r >= a.warmup:
                    call[name].append(t_call)
                    stages[name].append(list(ms))
            ctx.timer_start()
            batch.decode()
            ctx.timer_stop()
            if r >= a.warmup:
                dec.append(ctx.timer_elapsed_ms())
        res["batch_decode"] = stats(dec)
        for name in roads:
            res[name] = {"exact_call": stats(call[name]),
                         "stages": {s: stats([row[k] for row in stages[name]]) for k, s in enumerate(("planes", "colour"))},
                         "exact_call_over_batch_decode": round(statistics.median(call[name]) / statistics.median(dec), 3)}
            med = {s: res[name]["stages"][s]["median_ms"] for s in ("planes", "colour")}
            res[name]["gpixels_per_s_kernels"] = round(n * w * h / (sum(med.values()) * 1e6), 2)
        batch.close()
    finally:
        ctx.free(canvases)
        for d in coefs:
            d.close()
        if host is not None:
            host.close()
        for im in images:
            im.close()
        for p in prepared:
            p.close()
        ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
