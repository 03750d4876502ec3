#!/usr/bin/env python3
"""Where the time of a JPEG_PROGRESSIVE_FULL decode goes, stage by stage, against the plain decode of the file's baseline twin.

For 640x480, 1920x1080 and 4096x4096 pictures in 4:2:0 and 4:4:4 (Pillow, quality 85: progressive=True with libjpeg's default
10-scan script, and the baseline twin of the same pixels), RGB8888:

  scan_decode_ms   jda_progressive_prepare: every scan decoded on the host into coefficient planes (one thread, a host clock)
  h2d_ms           jda_coef_upload: quantisers + 128 bytes a block to HBM (a host clock around a call that ends in a synchronise)
  kernel_ms        jda_coef_decode_surfaces between two events on the context's stream (jda_timer_start / _stop around the public call:
                   the kernel AND the upload of its launch plan -- descriptors and tile records, 16 bytes a tile -- with the
                   synchronise behind it; `rocprofv3 --kernel-trace --stats` gives the kernel alone)
  one_call_ms      jda_decode_to_host with the bit: prepare + upload + kernel + copy back of the canvas (a host clock)
  baseline_*       the twin: one_call_ms of jda_decode_to_host, and kernel_ms of its plain decode -- jda_batch_decode of the resident image
                   between the same two events.  With --baseline-lib PATH (a build of the parent commit) the twin's figures are taken in a
                   child process that loads that library; without it, with this build (the decode kernels are the same code).

With --sparse the tool measures the sparse coefficient form instead and writes profiles/progressive_sparse.json (or --out).
Per file -- Pillow's progressive files of tests/prog_cases.py, one synthetic 2048x2048 quality-75 photograph-like file of jpegdec_amd.synth,
and this tool's own pictures --:

  dense_bytes / sparse_bytes / auto   128 bytes a block; 4 bytes a block + 4 a nonzero coefficient; the form JDA_COEF_AUTO picks
  sparse_pack_ms                      jda_coef_image_sparse on a fresh image (one thread, a host clock)
and, unless --no-gpu (then the figures above are all there is: they need no device):
  upload_ms {dense, sparse}           jda_coef_upload_ex of that form (a host clock around a call that ends in a synchronise; pageable source)
  kernel_ms {dense, sparse}           jda_coef_decode_surfaces_rect over that one image between two events: jda_coef_tiles / jda_sparse_tiles AND
                                      the upload of the launch plan, as kernel_ms above
  pipeline                            a batch of --batch copies of the file submitted with JDA_SUBMIT_PROGRESSIVE_FULL (submit + wait, a host clock,
                                      scans on the pipeline's workers) against the same files sent one by one through jda_decode_to_host with the
                                      bit -- with --baseline-lib in a child process on the parent commit's build, else on this build

Warm-up before every timed figure; each is the median of --repeat rounds with min and max beside it.  One JSON line on stdout and,
with --out, in a file.  Nothing is asserted: no timing threshold gates anything.  Fails without a GPU."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from jpegdec_amd.binding import Output  # noqa: E402

SHAPES = ((640, 480), (1920, 1080), (4096, 4096))
SAMPLINGS = ("4:2:0", "4:4:4")


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def picture(w, h, seed=5):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([128 + 100 * np.sin(x / 37 + y / 51), 128 + 90 * np.cos(x / 23 - y / 41), 128 + 80 * np.sin(x / 17) * np.cos(y / 29)], axis=-1)
    a += rng.normal(0, 6.0, (h, w, 3)).astype(np.float32)
    from PIL import Image
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))


def encode(im, sampling, progressive):
    b = io.BytesIO()
    im.save(b, "JPEG", quality=85, subsampling=sampling, progressive=progressive)
    return b.getvalue()


def host_ms(fn, repeat, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def baseline_figures(ctx, jpeg, repeat):
    """the twin's one call, and its decode kernel alone (resident image, events around jda_batch_decode)"""
    canvas = [None]

    def one_call():
        rc, canvas[0], g = J.decode_to_host(ctx, jpeg, J.RGB8888, 0, out=canvas[0])
        assert rc == 0
    one = host_ms(one_call, repeat)
    prep = J.PreparedImage(jpeg)
    g = prep.geometry(J.RGB8888, 0)
    pitch = (g["canvas_w"] * 4 + 15) & ~15
    dimg = J.DeviceImage(ctx, prep)
    surf = ctx.malloc(pitch * g["canvas_h"])
    batch = J.Batch(ctx, [dimg], [(surf, pitch, g["canvas_w"], g["canvas_h"])], [J.RGB8888], [0])
    kern = []
    for k in range(repeat + 2):
        ctx.timer_start()
        batch.decode()
        ctx.timer_stop()
        ms = ctx.timer_elapsed_ms()
        if k >= 2:
            kern.append(ms)
    batch.close(); ctx.free(surf); dimg.close(); prep.close()
    return {"one_call": stats(one), "kernel": stats(kern), "file_bytes": len(jpeg)}


def progressive_figures(ctx, jpeg, repeat):
    lib = ctx.lib
    imgs = []

    def prepare():
        imgs.append(J.CoefImage(jpeg))
        if len(imgs) > 1:
            imgs.pop(0).close()
    scan = host_ms(prepare, max(3, repeat // 4))
    img = imgs[0]
    n_blocks = img.info.mcus_x * img.info.mcus_y * img.info.blocks_per_mcu
    devs = []

    def upload():
        err = C.c_int32(0)
        d = lib.jda_coef_upload(ctx.handle, img.handle, C.byref(err))
        assert d and err.value == 0
        devs.append(d)
        if len(devs) > 1:
            lib.jda_dev_coef_free(ctx.handle, devs.pop(0))
    h2d = host_ms(upload, repeat)
    g = img.geometry(J.RGB8888, 0)
    pitch = (g["canvas_w"] * 4 + 15) & ~15
    surf = ctx.malloc(pitch * g["canvas_h"])
    outs = (Output * 1)(Output(surf, pitch, g["canvas_w"], g["canvas_h"]))
    kern = []
    one_img, pts, opts = (C.c_void_p * 1)(devs[0]), (C.c_int32 * 1)(J.RGB8888), (C.c_int32 * 1)(J.PROGRESSIVE_FULL)
    for k in range(repeat + 2):
        ctx.timer_start()
        ctx.check(lib.jda_coef_decode_surfaces(ctx.handle, 1, one_img, outs, pts, opts), "jda_coef_decode_surfaces")
        ctx.timer_stop()
        ms = ctx.timer_elapsed_ms()
        if k >= 2:
            kern.append(ms)
    ctx.free(surf)
    lib.jda_dev_coef_free(ctx.handle, devs[0])
    img.close()
    canvas = [None]

    def one_call():
        rc, canvas[0], gg = J.decode_to_host(ctx, jpeg, J.RGB8888, J.PROGRESSIVE_FULL, out=canvas[0])
        assert rc == 0
    one = host_ms(one_call, max(3, repeat // 4))
    return {"scan_decode": stats(scan), "h2d": stats(h2d), "kernel": stats(kern), "one_call": stats(one), "file_bytes": len(jpeg),
            "coefficient_bytes": n_blocks * 128, "canvas_bytes": g["canvas_w"] * g["canvas_h"] * 4}


def sparse_files(with_large):
    from tests import prog_cases as PC
    from jpegdec_amd.synth import synth_jpeg
    files = [("fixture_" + n, PC.files(n)[0]) for n in sorted(PC.CASES)]
    files.append(("synth_2048x2048_420_q75", synth_jpeg(2048, 2048, "4:2:0", seed=11, quality=75, progressive=True)))
    if with_large:
        for w, h in SHAPES:
            im = picture(w, h)
            for sampling in SAMPLINGS:
                files.append(("picture_%dx%d_%s_q85" % (w, h, sampling.replace(":", "")), encode(im, sampling, True)))
    return files


def one_by_one(ctx, jpeg, batch, repeat):
    canvas = [None]

    def run():
        for _ in range(batch):
            rc, canvas[0], g = J.decode_to_host(ctx, jpeg, J.RGB8888 if J.parse(jpeg)["ncomp"] == 3 else J.GRAY8, J.PROGRESSIVE_FULL, out=canvas[0])
            assert rc == 0
    return stats(host_ms(run, repeat))


def sparse_figures(ctx, jpeg, repeat, batch):
    """the byte counts and the pack time; with a context the upload, kernel and pipeline times"""
    lib = J.load_library()
    pack = []
    for _ in range(max(3, repeat // 4)):
        img = J.CoefImage(jpeg)
        t = time.perf_counter()
        img.sparse()
        pack.append((time.perf_counter() - t) * 1e3)
        img.close()
    img = J.CoefImage(jpeg)
    first, entries = img.sparse()
    dense_b, sparse_b = img.dense_bytes(), img.sparse_bytes()
    res = {"file_bytes": len(jpeg), "blocks": int(first.size - 1), "nonzero_coefficients": int(entries.size), "dense_bytes": dense_b, "sparse_bytes": sparse_b,
           "auto": "sparse" if sparse_b < dense_b else "dense", "sparse_pack": stats(pack)}
    if ctx is None:
        img.close()
        return res
    pt = J.RGB8888 if img.info.ncomp == 3 else J.GRAY8
    g = img.geometry(pt, 0)
    pitch = (g["canvas_w"] * g["bpp"] + 15) & ~15
    surf = ctx.malloc(pitch * g["canvas_h"])
    outs = (Output * 1)(Output(surf, pitch, g["canvas_w"], g["canvas_h"]))
    res["upload"], res["kernel"] = {}, {}
    for name, form in (("dense", J.COEF_DENSE), ("sparse", J.COEF_SPARSE)):
        devs = []

        def upload():
            err = C.c_int32(0)
            d = lib.jda_coef_upload_ex(ctx.handle, img.handle, form, C.byref(err))
            assert d and err.value == 0
            devs.append(d)
            if len(devs) > 1:
                lib.jda_dev_coef_free(ctx.handle, devs.pop(0))
        res["upload"][name] = stats(host_ms(upload, repeat))
        one_img, pts, opts = (C.c_void_p * 1)(devs[0]), (C.c_int32 * 1)(pt), (C.c_int32 * 1)(0)
        kern = []
        for k in range(repeat + 2):
            ctx.timer_start()
            ctx.check(lib.jda_coef_decode_surfaces_rect(ctx.handle, 1, one_img, outs, pts, opts, None), "jda_coef_decode_surfaces_rect")
            ctx.timer_stop()
            ms = ctx.timer_elapsed_ms()
            if k >= 2:
                kern.append(ms)
        res["kernel"][name] = stats(kern)
        lib.jda_dev_coef_free(ctx.handle, devs[0])
    img.close()
    # a pipeline batch of `batch` copies, every one into the same surface (what is timed is the path, not the pixels)
    pipe = J.Pipeline(ctx, max_images=batch, depth=1)
    packed = pipe.pack([jpeg] * batch, [(surf, pitch, g["canvas_w"], g["canvas_h"])] * batch, [pt] * batch, [J.PROGRESSIVE_FULL] * batch)

    def run():
        st = pipe.wait(pipe.submit_packed(packed, J.SUBMIT_PROGRESSIVE_FULL))
        assert st == [0] * batch, st
    res["pipeline"] = {"batch": batch, "submit_and_wait": stats(host_ms(run, max(3, repeat // 2)))}
    pipe.close()
    ctx.free(surf)
    return res


def sparse_main(args):
    if args.baseline_only:
        raw = C.CDLL(J.library_path())
        J.binding._PROTOTYPES[:] = [p for p in J.binding._PROTOTYPES if hasattr(raw, p[0])]
        ctx = J.Context(0)
        res = {"cases": {name: {"one_by_one": one_by_one(ctx, jpeg, args.batch, max(3, args.repeat // 2))} for name, jpeg in sparse_files(True)}}
        ctx.close()
        print(json.dumps(res))
        return
    ctx = None if args.no_gpu else J.Context(0)
    res = {"tool": "progressive_bench --sparse", "library": os.path.relpath(J.library_path(), ROOT), "gpu": ctx is not None, "cases": {}}
    for name, jpeg in sparse_files(ctx is not None):
        res["cases"][name] = sparse_figures(ctx, jpeg, args.repeat, args.batch)
        if ctx is not None and not args.baseline_lib:
            res["cases"][name]["pipeline"]["one_by_one"] = one_by_one(ctx, jpeg, args.batch, max(3, args.repeat // 2))
    if ctx is not None:
        ctx.close()
    if ctx is not None and args.baseline_lib:
        env = dict(os.environ, JDA_LIBRARY=os.path.abspath(args.baseline_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sparse", "--baseline-only", "--repeat", str(args.repeat), "--batch", str(args.batch)],
                           env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("baseline child failed: " + r.stderr[-2000:])
        child = json.loads(r.stdout.strip().splitlines()[-1])
        res["one_by_one_library"] = "the parent commit's build"
        for name, v in child["cases"].items():
            res["cases"][name]["pipeline"]["one_by_one"] = v["one_by_one"]
    if args.note:
        res["note"] = args.note
    print(json.dumps(res))
    out = args.out or os.path.join(ROOT, "profiles", "progressive_sparse.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sparse", action="store_true", help="measure the sparse coefficient form (profiles/progressive_sparse.json)")
    ap.add_argument("--no-gpu", action="store_true", help="--sparse: the byte counts and the pack time only")
    ap.add_argument("--batch", type=int, default=8, help="--sparse: files in the pipeline batch")
    ap.add_argument("--note", default=None, help="--sparse: a line on the machine's load, kept in the file")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-lib", default=None, help="libjpegdec_amd.so of the parent commit: the twin's figures are measured with it")
    ap.add_argument("--baseline-only", action="store_true", help="(the child process of --baseline-lib)")
    args = ap.parse_args()
    if args.sparse:
        return sparse_main(args)
    if args.baseline_only:
        # (an older build of the library lacks the entry points this tool's other half measures: bind what it has)
        raw = C.CDLL(J.library_path())
        J.binding._PROTOTYPES[:] = [p for p in J.binding._PROTOTYPES if hasattr(raw, p[0])]
    ctx = J.Context(0)
    res = {"tool": "progressive_bench", "library": J.library_path(), "pixel_type": "RGB8888", "quality": 85, "cases": {}}
    for w, h in SHAPES:
        im = picture(w, h)
        for sampling in SAMPLINGS:
            key = "%dx%d_%s" % (w, h, sampling.replace(":", ""))
            twin = encode(im, sampling, False)
            if args.baseline_only:
                res["cases"][key] = {"baseline": baseline_figures(ctx, twin, args.repeat)}
                continue
            res["cases"][key] = {"progressive": progressive_figures(ctx, encode(im, sampling, True), args.repeat)}
            if not args.baseline_lib:
                res["cases"][key]["baseline"] = baseline_figures(ctx, twin, args.repeat)
    ctx.close()
    if args.baseline_lib and not args.baseline_only:
        env = dict(os.environ, JDA_LIBRARY=os.path.abspath(args.baseline_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-only", "--repeat", str(args.repeat)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("baseline child failed: " + r.stderr[-2000:])
        child = json.loads(r.stdout.strip().splitlines()[-1])
        res["baseline_library"] = "the parent commit's build"
        for key, v in child["cases"].items():
            res["cases"][key]["baseline"] = v["baseline"]
    res["library"] = os.path.relpath(res["library"], ROOT)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
