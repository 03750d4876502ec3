#!/usr/bin/env python3
"""Times of the unpack pass (jda_unpack_tiles) on the GPU beside a device-to-device copy of the same destination bytes and beside the pack
pass (jda_pack_tiles) of the same shapes, all taken in one run; and encode_tensors of the batch beside jda_encode_surfaces alone.

--batch surfaces of --size x --size RGB8888 pixels (random bytes) are packed, all of them in one launch, as U8 HWC, U8 CHW and F32 CHW
(normalise_table): that launch is timed (jda_internal_pack_time) and leaves the dense tensors the unpack launch turns back into surfaces
(jda_internal_unpack_time; F32 through denormalise_params), and the surfaces it made are copied device to device (jda_internal_copy_time:
width * 4 * height bytes an image, the bytes the unpack launch writes).  Every launch lies between the context's two timer events on its
stream, the job records go up before the first.  Rounds alternate over the three formats and the three passes, so that a drift of the
clock hits them all alike; warm-up rounds first; each figure is the median of --repeat rounds with min and max beside it.  bytes = source
bytes read + destination bytes written.  The first image of every unpacked batch is held against the source surface (A = 0xFF).
Then (with torch): a [batch, 3, size, size] uint8 tensor -- a gradient under a little noise -- through encode_tensors (wall clock, device
synchronised, quality 75, 4:2:0) and the same pixels, already unpacked into surfaces, through jda_encode_surfaces alone.
One JSON line on stdout and in --out (profiles/unpack_bench.json); --code-object-out (profiles/unpack_code_object.txt): the registers, LDS and
scratch of the six instances, read from the library's code object.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

try:
    import torch  # noqa: F401  (before anything loads libjpegdec_amd.so: one process, one HIP runtime)
except ImportError:
    torch = None

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpegdec_amd as J  # noqa: E402
from jpegdec_amd.binding import Output  # noqa: E402

HBM_PEAK = 8.0e12
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5), "max_ms": round(max(xs), 5), "n": len(xs)}


def code_object_report(path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_object
    rows = [k for k in code_object.kernels(J.library_path()) if "jda_unpack_tiles" in k["name"]]
    with open(path, "w") as f:
        f.write("the instances of jda_unpack_tiles<HWC, ES> in the gfx950 code object of jpegdec_amd/libjpegdec_amd.so (tools/code_object.py: the code object's own figures)\n")
        f.write("%-44s %5s %5s %7s %7s %7s %7s\n" % ("kernel", "vgpr", "sgpr", "s-spill", "v-spill", "lds", "scratch"))
        for k in sorted(rows, key=lambda r: r["name"]):
            f.write("%-44s %5d %5d %7d %7d %7d %7d\n" % (k["name"].split("(")[0].replace("void ", ""), k["vgpr"], k["sgpr"], k["sgpr_spill"], k["vgpr_spill"], k["lds"], k["scratch"]))
        f.write("(HWC = 1 the pixel-major kernel, 0 the planar one -- three planes, or the one of a gray image; ES = bytes of an element.  No LDS, no scratch, no spills:\n"
                "scale and bias are kernel arguments.)\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack_bench.json"))
    ap.add_argument("--code-object-out", default=os.path.join(ROOT, "profiles", "unpack_code_object.txt"))
    ap.add_argument("--no-encode", action="store_true")
    a = ap.parse_args()
    if a.code_object_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.code_object_out)), exist_ok=True)
        code_object_report(a.code_object_out)
    n, size = a.batch, a.size
    ctx = J.Context(0)
    lib = ctx.lib
    lib.jda_internal_pack_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p,
                                           C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_float)]
    lib.jda_internal_unpack_time.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(Output), C.c_int32,
                                             C.c_int32, C.POINTER(C.c_float)]
    lib.jda_internal_copy_time.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_float)]
    pitch, px = size * 4, size * size
    surf = pitch * size
    one = np.random.RandomState(5).randint(0, 256, surf).astype(np.uint8)
    src_surfaces, dst_surfaces, copies, dense = ctx.malloc(surf * n), ctx.malloc(surf * n), ctx.malloc(surf * n), ctx.malloc(px * 3 * 4 * n + 16)
    for i in range(n):
        ctx.from_host(src_surfaces + i * surf, one)
    table = np.ascontiguousarray(J.normalise_table(MEAN, STD, np.float32)).view(np.uint8).reshape(-1)
    dtable = ctx.malloc(table.size)
    ctx.from_host(dtable, table)
    sb = (C.c_float * 6)(*[float(v) for v in J.denormalise_params(MEAN, STD).reshape(-1)])
    s_out = (Output * n)(*[Output(src_surfaces + i * surf, pitch, size, size) for i in range(n)])
    d_out = (Output * n)(*[Output(dst_surfaces + i * surf, pitch, size, size) for i in range(n)])
    formats = {"u8_hwc": (J.PACK_HWC, J.PACK_U8, None, None, 1), "u8_chw": (J.PACK_CHW, J.PACK_U8, None, None, 1), "f32_chw": (J.PACK_CHW, J.PACK_F32, dtable, sb, 4)}
    t_pack, t_unpack, t_copy = {k: [] for k in formats}, {k: [] for k in formats}, []
    want = one.reshape(size, size, 4).copy()
    want[..., 3] = 0xFF
    res = {"what": "unpack_bench", "images": n, "w": size, "h": size, "hbm_peak_tbps": HBM_PEAK / 1e12, "unpack": {}, "pack": {}}
    out = (C.c_float * 1)()
    try:
        for k in range(a.warmup + a.repeat):
            for name, (layout, elem, tab, scale_bias, es) in formats.items():
                # image i of the batch tensor at its own offset, one element off a 16-byte boundary
                ptrs = (C.c_void_p * n)(*[dense + es + i * px * 3 * es for i in range(n)])
                ctx.check(lib.jda_internal_pack_time(ctx.handle, n, s_out, 4, None, layout, elem, tab, ptrs, 1, out), "jda_internal_pack_time")
                if k >= a.warmup:
                    t_pack[name].append(out[0])
                ctx.check(lib.jda_internal_unpack_time(ctx.handle, n, ptrs, layout, elem, scale_bias, d_out, 4, 1, out), "jda_internal_unpack_time")
                if k >= a.warmup:
                    t_unpack[name].append(out[0])
                if k == 0:
                    got = ctx.to_host(dst_surfaces, surf).reshape(size, size, 4)
                    assert np.array_equal(got, want), "%s: the unpacked surface differs from the source" % name
                ctx.check(lib.jda_internal_copy_time(ctx.handle, copies, dst_surfaces, surf * n, 1, out), "jda_internal_copy_time")
                if k >= a.warmup:
                    t_copy.append(out[0])
        copy_med = statistics.median(t_copy)
        res["copy_same_destination_bytes"] = dict(stats(t_copy), bytes_read_plus_written=2 * surf * n, tbps=round(2 * surf * n / (copy_med * 1e-3) / 1e12, 3))
        for name, (layout, elem, tab, scale_bias, es) in formats.items():
            moved = n * px * (4 + 3 * es)
            for key, times in (("unpack", t_unpack), ("pack", t_pack)):
                med = statistics.median(times[name])
                rate = moved / (med * 1e-3)
                res[key][name] = dict(stats(times[name]), bytes_read_plus_written=moved, tbps=round(rate / 1e12, 3), fraction_of_hbm_peak=round(rate / HBM_PEAK, 3),
                                      time_over_copy=round(med / copy_med, 3))
            res["unpack"][name]["time_over_pack"] = round(statistics.median(t_unpack[name]) / statistics.median(t_pack[name]), 3)
        for p in (src_surfaces, copies, dense, dtable):
            ctx.free(p)
        if torch is None or a.no_encode:
            res["encode_tensors"] = "not measured"
        else:
            dev = torch.device("cuda", ctx.device)
            yy, xx = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing="ij")
            g = torch.Generator(device=dev)
            g.manual_seed(7)
            planes = [((xx * 3 + yy * 2) // 16) % 224, ((xx + yy * 5) // 24) % 224, ((xx * 2 + yy) // 12) % 224]
            img = torch.stack(planes).to(torch.int32)
            t = torch.empty((n, 3, size, size), dtype=torch.uint8, device=dev)
            for i in range(n):
                t[i] = (img + torch.randint(0, 32, (3, size, size), device=dev, generator=g, dtype=torch.int32)).to(torch.uint8)
            torch.cuda.synchronize(dev)
            per = 3 * px
            J.unpack_surfaces(ctx, [t.data_ptr() + i * per for i in range(n)], [(dst_surfaces + i * surf, pitch, size, size) for i in range(n)], 4, J.PACK_CHW, J.PACK_U8)
            cap = J.encode_bound(size, size, "4:2:0")
            fbase = ctx.malloc(cap * n)
            jobs = [(0, 0, size, size, "4:2:0", 75, 0)] * n
            t_whole, t_encode, nbytes = [], [], None
            for k in range(a.warmup + a.repeat):
                t0 = time.perf_counter()
                files = J.encode_tensors(ctx, t, quality=75, sampling="4:2:0")
                t1 = time.perf_counter()
                nbytes, st = J.encode_surfaces(ctx, [(dst_surfaces + i * surf, pitch, size, size) for i in range(n)], 4, jobs, [fbase + i * cap for i in range(n)], [cap] * n)
                ctx.sync()
                t2 = time.perf_counter()
                assert not any(st) and [len(f) for f in files] == list(nbytes)
                if k >= a.warmup:
                    t_whole.append((t1 - t0) * 1e3)
                    t_encode.append((t2 - t1) * 1e3)
            ctx.free(fbase)
            res["encode_tensors"] = {"quality": 75, "sampling": "4:2:0", "file_bytes_total": int(sum(nbytes)), "encode_tensors_wall": stats(t_whole),
                                     "encode_surfaces_alone_wall": stats(t_encode),
                                     "ratio": round(statistics.median(t_whole) / statistics.median(t_encode), 3),
                                     "note": "encode_tensors = allocation, one unpack launch, the encode call and the copy of the files to the host; encode_surfaces alone leaves the files in HBM"}
    finally:
        ctx.free(dst_surfaces)
        ctx.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
