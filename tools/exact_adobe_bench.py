#!/usr/bin/env python3
"""Times of the four-component exact decode (jda_exact_decode_surfaces_ex with JDA_EXACT_COLOUR_MODELS) on the GPU beside the
three-component one of the same picture and size: 64 files of 4096 x 4096 at quality 75, to RGB8888 surfaces.

Four legs, each a process of its own under a time limit of its own, run one after the other and stopped at the first that fails (what a
shell writes as `timeout .. leg1 && timeout .. leg2 && ..`):
  cmyk444   Pillow's CMYK file (Adobe transform 0) at 4:4:4: sampling 11,11,11,11
  ycck420   Pillow's CMYK file at subsampling 2 with the transform byte patched to 2 (YCCK): sampling 22,11,11,11.  Photoshop's 22,11,11,22
            has no writer here but the suite's Python one, which is too slow for 4096 x 4096: its K plane is four times this one's.
  ycc444    Pillow's YCbCr file at 4:4:4 through jda_exact_decode_surfaces: the kernels and the numbers of the plain call
  ycc420    the same at 4:2:0
A four-component file is resident as the dense coefficient image of jda_coef_prepare, uploaded n times; a YCbCr one as the dense coefficient
image of the same coefficients (the same load phase, so that the extra plane is the difference) and as a baseline image with the device
pre-scan's index.  Warm-up rounds first, every figure the median of --repeat rounds with min and max beside it:
  call      the call as a caller sees it, between the context's two timer events (plan, blob copy, launches, wait);
  stages    the same call through jda_internal_exact_time_ex, its launches between events of their own: `planes` (jda_exact_planes, K's gray
            tiles among them) and `colour` (jda_exact_colour4 / jda_exact_colour).
plane_bytes: what the planes stage writes and the colour stage reads again (each plane's own extent), beside 4 B a pixel of surface: the
comparison is the extra plane's bytes against the extra time.  Nothing here is a gate.
One JSON line on stdout and, with --out FILE (profiles/exact_adobe_bench.json is the place for a run on an MI355X), in a file.  Fails without a GPU."""
import argparse
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.encode_bench import picture, stats      # noqa: E402

LEGS = ("cmyk444", "ycck420", "ycc444", "ycc420")


def source_file(leg, w, h):
    from PIL import Image
    a = picture(w, h)
    b = io.BytesIO()
    if leg in ("cmyk444", "ycck420"):
        a = a.copy()
        a[..., 3] = 255 - a[..., 1]                                    # (the picture's fourth channel is flat: a K plane with content)
        Image.fromarray(a, "CMYK").save(b, "JPEG", quality=75, subsampling=0 if leg == "cmyk444" else 2)
        f = b.getvalue()
        if leg == "ycck420":
            i = f.index(b"Adobe")
            f = f[:i + 11] + b"\x02" + f[i + 12:]
        return f
    Image.fromarray(np.ascontiguousarray(a[..., :3])).save(b, "JPEG", quality=75, subsampling=0 if leg == "ycc444" else 2)
    return b.getvalue()


def run_leg(a):
    import jpegdec_amd as J
    from jpegdec_amd.binding import Output, RecodeSource
    sys.path.insert(0, os.path.join(ROOT))
    ctx = J.Context(0)
    lib = ctx.lib
    lib.jda_internal_exact_time_ex.restype = C.c_int
    lib.jda_internal_exact_time_ex.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    n, w, h = a.images, a.size, a.size
    jpeg = source_file(a.leg, w, h)
    four = a.leg in ("cmyk444", "ycck420")
    sub = 1 if a.leg.endswith("444") else 2
    cw, ch = -(-w // sub), -(-h // sub)
    probe = J.exact_probe(jpeg)
    res = {"leg": a.leg, "images": n, "width": w, "height": h, "pixels": n * w * h, "file_bytes": len(jpeg), "model": probe["model"],
           "sampling": "%s,11,11%s" % ("11" if sub == 1 else "22", ",11" if four else ""),
           "plane_bytes_per_image": w * h + 2 * cw * ch + (cw * ch if four else 0), "surface_bytes_per_image": 4 * w * h}
    keep, roads = [], {}
    host = J.CoefImage.from_file(jpeg)
    keep.append(host)
    roads["coefficients"] = [J.DeviceCoef(ctx, host, J.COEF_DENSE) for _ in range(n)]
    if not four:
        prepared = J.prepare_batch([jpeg] * n, device_prescan=True)
        keep += list(prepared)
        roads["baseline"] = J.upload_batch(ctx, prepared)
    pitch = (w * 4 + 15) & ~15
    surf = (pitch * h + 255) & ~255
    canvases = ctx.malloc(surf * n)
    try:
        outs = [(canvases + k * surf, pitch, w, h) for k in range(n)]
        so = (Output * n)(*[Output(*o) for o in outs])
        st = (C.c_int32 * n)()
        flags = J.EXACT_COLOUR_MODELS if four else 0
        for name, items in roads.items():
            rs = (RecodeSource * n)(*[RecodeSource(d.handle, None) if name == "baseline" else RecodeSource(None, d.handle) for d in items])
            call, stages = [], []
            for r in range(a.warmup + a.repeat):
                ctx.timer_start()
                status = J.exact_decode(ctx, items, outs, colour_models=four)
                ctx.timer_stop()
                assert not any(status), status[:4]
                t_call = ctx.timer_elapsed_ms()
                ms = (C.c_float * 2)()
                ctx.check(lib.jda_internal_exact_time_ex(ctx.handle, n, rs, so, None, None, flags, st, ms), "jda_internal_exact_time_ex")
                assert not any(st)
                if r >= a.warmup:
                    call.append(t_call)
                    stages.append(list(ms))
            row = {"call": stats(call), "stages": {s: stats([x[k] for x in stages]) for k, s in enumerate(("planes", "colour"))}}
            row["colour_gbytes_per_s"] = round(n * (res["plane_bytes_per_image"] + res["surface_bytes_per_image"]) / (row["stages"]["colour"]["median_ms"] * 1e6), 1)
            res[name] = row
    finally:
        ctx.free(canvases)
        for items in roads.values():
            for d in items:
                d.close()
        for p in keep:
            p.close()
        ctx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--leg", choices=LEGS, help="one leg, in this process (what the driver starts)")
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.leg:
        run_leg(a)
        return
    res = {"images": a.images, "width": a.size, "height": a.size, "legs": {}}
    for leg in LEGS:                                                   # one after the other; the first that fails ends the run
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--images", str(a.images), "--size", str(a.size),
               "--warmup", str(a.warmup), "--repeat", str(a.repeat)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("leg %s ended with status %d: nothing more is started" % (leg, r.returncode))
        res["legs"][leg] = json.loads(r.stdout.strip().splitlines()[-1])
    L = res["legs"]
    for four, three in (("cmyk444", "ycc444"), ("ycck420", "ycc420")):  # the extra plane's bytes against the extra time, same load phase
        res[four + "_over_" + three] = {
            "plane_bytes": round(L[four]["plane_bytes_per_image"] / L[three]["plane_bytes_per_image"], 3),
            "colour_ms": round(L[four]["coefficients"]["stages"]["colour"]["median_ms"] / L[three]["coefficients"]["stages"]["colour"]["median_ms"], 3),
            "planes_ms": round(L[four]["coefficients"]["stages"]["planes"]["median_ms"] / L[three]["coefficients"]["stages"]["planes"]["median_ms"], 3),
            "call_ms": round(L[four]["coefficients"]["call"]["median_ms"] / L[three]["coefficients"]["call"]["median_ms"], 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
