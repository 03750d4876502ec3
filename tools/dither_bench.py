#!/usr/bin/env python3
"""Times of the dithered (4 / 2 / 1 bits per pixel) output path on the GPU, against same-run baselines.

  (a) the dither kernel alone (jda_dither_surfaces) on 1 and on 64 resident 4096x4096 GRAY8 canvases and on one of 3600x2848 (squirrel_dither's), 1 bpp and 4 bpp: hipEvents on the
      context's stream around the call (the launch, the copy of its job records in front of it and of its flag behind it);
  (b) decode_dither_to_host of squirrel_dither.jpg and of a 4096x4096 gray file against decode_to_host to GRAY8 of the same files,
      alternating in the same run: a host clock around calls that end in a device synchronise;
  (c) the unmodified reference's decodeDither on one thread of the same host (its SSE2 build: oracle/_ref, where it exists).

Warm-up before every timed shape; each figure is the median of --repeat runs with min and max beside it.  One JSON line on stdout
and, with --out, in a file.  Fails without a GPU.  A kernel-only time comes from `rocprofv3 --kernel-trace --stats -- python
tools/dither_bench.py --kernel-only` in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from jpegdec_amd.synth import synth_jpeg  # noqa: E402
from tests import ref_dither as R  # noqa: E402
from tests.ref_fixtures import ref_jpeg  # noqa: E402


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4), "n": len(xs)}


def kernel_alone(ctx, n_images, pt, warmup, repeat, width=4096, height=4096):
    rng = np.random.RandomState(5)
    ramp = ((np.arange(width)[None, :] // 16 + np.arange(height)[:, None] // 16) % 256).astype(np.uint8)
    canvas = np.clip(ramp.astype(np.int32) + rng.randint(-24, 25, ramp.shape), 0, 255).astype(np.uint8)      # gradients and texture, as a photograph has
    assert width % 16 == 0
    d = J.dither_geometry(width, height, pt)
    pp = (d["pitch"] + 15) & ~15
    gray, packed = [], []
    for _ in range(n_images):
        g, p = ctx.malloc(width * height), ctx.malloc(pp * height)
        ctx.from_host(g, canvas)
        gray.append((g, width, width, height))
        packed.append((p, pp, width, height))
    times = []
    for k in range(warmup + repeat):
        ctx.timer_start()
        J.dither_surfaces(ctx, gray, [16] * n_images, [pt] * n_images, packed)
        ctx.timer_stop()
        ms = ctx.lib.jda_timer_elapsed_ms(ctx.handle)
        if k >= warmup:
            times.append(ms)
    for (g, _, _, _), (p, _, _, _) in zip(gray, packed):
        ctx.free(g)
        ctx.free(p)
    return dict(stats(times), images=n_images, gray_bytes=n_images * width * height, packed_bytes=n_images * d["pitch"] * height)


def one_call_pair(ctx, jpeg, pt, warmup, repeat):
    """the dithered call and the GRAY8 call of the same file, alternating"""
    td, tg = [], []
    canvas = None
    for k in range(warmup + repeat):
        t0 = time.perf_counter()
        rc, packed, g = J.decode_dither_to_host(ctx, jpeg, pt, 0)
        t1 = time.perf_counter()
        assert rc == 0
        rc, canvas, _ = J.decode_to_host(ctx, jpeg, J.GRAY8, 0, out=canvas)
        t2 = time.perf_counter()
        assert rc == 0
        if k >= warmup:
            td.append((t1 - t0) * 1e3)
            tg.append((t2 - t1) * 1e3)
    return {"dithered": stats(td), "gray8": stats(tg), "dithered_minus_gray8_median_ms": round(statistics.median(td) - statistics.median(tg), 4)}


def reference_one_thread(jpeg, pt, repeat):
    path = R.REF_SSE2 if os.path.exists(R.REF_SSE2) else R.REF_SCALAR
    if not os.path.exists(path):
        return None
    ts = []
    for _ in range(1 + repeat):
        t0 = time.perf_counter()
        rc, err, log, strips = R.ref_decode_dither(jpeg, pt, 0, lib_path=path)
        ts.append((time.perf_counter() - t0) * 1e3)
        assert rc == 1
    return dict(stats(ts[1:]), build=os.path.basename(path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--kernel-only", action="store_true", help="only (a), few runs: the workload of a rocprofv3 kernel trace")
    ap.add_argument("--one-call-only", action="store_true", help="only squirrel_dither through decode_dither_to_host, few runs: the workload of a kernel + memory-copy trace")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = J.Context(0)
    res = {"what": "dither_bench", "kernel": {}, "one_call": {}, "reference_one_thread": {}}
    try:
        if a.one_call_only:
            for name, pt in (("1bpp", J.ONE_BIT_DITHERED), ("4bpp", J.FOUR_BIT_DITHERED)):
                res["one_call"]["squirrel_dither_3596x2840_%s" % name] = one_call_pair(ctx, ref_jpeg("squirrel_dither"), pt, 1, 3)
        for name, pt in (("1bpp", J.ONE_BIT_DITHERED), ("4bpp", J.FOUR_BIT_DITHERED)):
            if a.one_call_only:
                break
            for n in (1, a.batch):
                res["kernel"]["%s_x%d" % (name, n)] = kernel_alone(ctx, n, pt, 1 if a.kernel_only else a.warmup, 2 if a.kernel_only else a.repeat)
            # squirrel_dither's canvas (3600 x 2848 padded): the one-call figures of that file are held against THIS kernel time
            res["kernel"]["%s_3600x2848_x1" % name] = kernel_alone(ctx, 1, pt, 1 if a.kernel_only else a.warmup, 2 if a.kernel_only else a.repeat, 3600, 2848)
        if not a.kernel_only and not a.one_call_only:
            files = {"squirrel_dither_3596x2840": ref_jpeg("squirrel_dither"), "gray_4096x4096": synth_jpeg(4096, 4096, "gray", seed=91)}
            for fname, jpeg in files.items():
                for name, pt in (("1bpp", J.ONE_BIT_DITHERED), ("4bpp", J.FOUR_BIT_DITHERED)):
                    pair = one_call_pair(ctx, jpeg, pt, a.warmup, a.repeat)
                    ref = reference_one_thread(jpeg, pt, 3)
                    if ref:
                        pair["reference_over_product"] = round(ref["median_ms"] / pair["dithered"]["median_ms"], 2)
                    res["one_call"]["%s_%s" % (fname, name)] = pair
                    res["reference_one_thread"]["%s_%s" % (fname, name)] = ref
    finally:
        ctx.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
