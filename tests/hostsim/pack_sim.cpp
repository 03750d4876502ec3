// tests/hostsim/pack_sim.cpp -- TEST INFRASTRUCTURE: the pack kernel's schedule on the CPU.
//
// packsim_lanes runs jda_pack_tiles (jpegdec_amd/csrc/jda_kernels.hip) the way the GPU runs it: every tile of the job, the 256 lanes of a
// tile one after the other through the kernel's OWN code (jda_pack_stage_table / jda_pack_tile of jda_device_core.h), the table staged by
// all lanes before any lane packs (the workgroup barrier).  Memory goes through an IO policy that holds every access to what the kernel
// promises: source loads are aligned dwords inside the aligned extent of the rectangle's rows and inside the pitch; table loads are
// aligned vectors inside the table; every store is aligned to its own width, lies inside [dst, dst + bytes), is narrower than a vector
// only where the vector is the first or the last of its run, and no destination byte is written twice; LDS is read only where it was
// written.  packsim_rowmajor is the twin that knows none of this (pack_twin.h); packsim_check runs the argument checks of
// jda_pack_surfaces (jda_pack_plan.h) without a GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_pack_plan.h"
#include "pack_twin.h"

namespace {
struct SimIO {
    const uint8_t *src; uint32_t src_pitch, src_rows, bpp, rx, ry, rw, rh;
    const uint8_t *table; uint32_t table_bytes;
    uint8_t *dst; size_t dst_bytes; uint32_t run_bytes, runs;
    std::vector<uint8_t> written;
    std::vector<uint32_t> lds; std::vector<uint8_t> lds_set;
    int err;
    void fail(int e) { if (!err) err = e; }
    uint32_t ld32(const uint8_t *p)
    {
        const size_t off = (size_t)(p - src);
        if (p < src || (off & 3u) || off + 4u > (size_t)src_pitch * src_rows) { fail(-10); return 0; }
        const uint32_t row = (uint32_t)(off / src_pitch), in_row = (uint32_t)(off % src_pitch);
        if (in_row + 4u > src_pitch) { fail(-11); return 0; }
        if (row < ry || row >= ry + rh || in_row < ((rx * bpp) & ~3u) || in_row + 4u > (((rx + rw) * bpp + 3u) & ~3u)) { fail(-12); return 0; }   // (not a dword of the rectangle)
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    void ld_table128(const uint8_t *p, uint32_t *v)
    {
        const size_t off = (size_t)(p - table);
        if (!table || p < table || (off & 15u) || off + 16u > table_bytes) { fail(-13); memset(v, 0, 16); return; }
        memcpy(v, p, 16);
    }
    bool dst_ok(uint8_t *p, uint32_t n)
    {
        if (((uintptr_t)p % n) != 0) { fail(-20); return false; }
        if (p < dst || (size_t)(p - dst) + n > dst_bytes) { fail(-21); return false; }        // a neighbour's bytes
        const size_t off = (size_t)(p - dst);
        if (n < 16u) {
            // the aligned vector around the store must reach in front of its run or behind it
            const uint32_t run = (uint32_t)(off / run_bytes);
            const uintptr_t v0 = (uintptr_t)p & ~(uintptr_t)15, r0 = (uintptr_t)dst + (size_t)run * run_bytes, r1 = r0 + run_bytes;
            if (v0 >= r0 && v0 + 16u <= r1) { fail(-22); return false; }
        }
        for (uint32_t i = 0; i < n; i++) { uint8_t &w = written[off + i]; if (w) fail(-23); w = 1; }
        return true;
    }
    void st128(uint8_t *p, const uint32_t *v) { if (dst_ok(p, 16)) memcpy(p, v, 16); }
    void st32(uint8_t *p, uint32_t v) { if (dst_ok(p, 4)) memcpy(p, &v, 4); }
    void st16(uint8_t *p, uint32_t v) { const uint16_t h = (uint16_t)v; if (dst_ok(p, 2)) memcpy(p, &h, 2); }
    void st8(uint8_t *p, uint32_t v) { if (dst_ok(p, 1)) *p = (uint8_t)v; }
    void lds_wr(uint32_t i, uint32_t v) { if (i >= lds.size()) { fail(-30); return; } lds[i] = v; lds_set[i] = 1; }
    uint32_t lds_rd32(uint32_t i) { if (i >= lds.size() || !lds_set[i]) { fail(-31); return 0; } return lds[i]; }
    uint32_t lds_rd16(uint32_t i) { if (i / 2u >= lds.size() || !lds_set[i / 2u]) { fail(-31); return 0; } return (lds[i / 2u] >> (16u * (i & 1u))) & 0xffffu; }
};
template <int HWC, int ES> int run(SimIO &io, const jda_pack_geo &G, const uint8_t *table)
{
    const uint32_t channels = G.bpp == 4u ? 3u : 1u, tiles = jda_pack_tiles_of(jda_pack_run_bytes(HWC, ES, G.w, G.h));
    // the kernel's own way from a flat tile number to its job: three jobs, this one in the middle
    jda_pack_job jobs[3];
    memset(jobs, 0, sizeof(jobs));
    jobs[0].tile0 = 0; jobs[1].tile0 = 5; jobs[2].tile0 = 5 + tiles;
    for (uint32_t tile = 5; tile < 5 + tiles; tile++) {
        if (jda_pack_find_job(jobs, 3, tile) != 1u) return -40;
        std::fill(io.lds_set.begin(), io.lds_set.end(), 0);      // a workgroup finds nothing in LDS
        if (ES > 1) for (uint32_t tid = 0; tid < JDA_PACK_THREADS; tid++) jda_pack_stage_table<ES>(io, table, channels, tid);
        for (uint32_t tid = 0; tid < JDA_PACK_THREADS; tid++) jda_pack_tile<HWC, ES>(G, tile - 5u, tid, io);
    }
    return io.err;
}
}

extern "C" int packsim_rowmajor(const uint8_t *src, int pitch, int bpp, int x, int y, int w, int h, int layout_flags, int elem_type, const void *table, void *dst)
{
    return pack_twin_rowmajor(src, pitch, bpp, x, y, w, h, layout_flags, elem_type, table, dst);
}

// src: rows rows of pitch bytes (16-byte aligned); {x, y, w, h}: the rectangle; dst: dense, aligned to its element.  0, or the first promise
// broken (-1x loads, -2x stores, -3x LDS, -24: a destination byte not written), or the code the argument checks of jda_pack_surfaces give.
extern "C" int packsim_lanes(const uint8_t *src, int pitch, int width_px, int rows, int bpp, int x, int y, int w, int h, int layout_flags, int elem_type,
                             const void *table, void *dst)
{
    jda_output S;
    S.pixels = (void *)src; S.pitch_bytes = pitch; S.width_px = width_px; S.rows = rows;
    const int32_t rect[4] = { x, y, w, h };
    void *const dsts[1] = { dst };
    jda_pack_plan_out plan;
    const int rc = jda_pack_plan_jobs(1, &S, bpp, rect, layout_flags, elem_type, table, dsts, &plan);
    if (rc != JDA_SUCCESS) return rc;
    const jda_pack_job &J = plan.jobs[0];
    jda_pack_geo G;
    G.src = J.src; G.dst = J.dst; G.src_pitch = J.src_pitch; G.x = J.x; G.y = J.y; G.w = J.w; G.h = J.h;
    G.bpp = (uint32_t)bpp; G.bgr = (layout_flags & JDA_PACK_BGR) ? 1u : 0u;
    if (plan.n_tiles != jda_pack_tiles_of(jda_pack_run_bytes(plan.hwc != 0, plan.es, G.w, G.h))) return -41;
    SimIO io;
    io.src = src; io.src_pitch = (uint32_t)pitch; io.src_rows = (uint32_t)rows; io.bpp = (uint32_t)bpp; io.rx = G.x; io.ry = G.y; io.rw = G.w; io.rh = G.h;
    const uint32_t channels = bpp == 4 ? 3u : 1u;
    io.table = (const uint8_t *)table; io.table_bytes = table ? channels * 256u * plan.es : 0u;
    io.dst = (uint8_t *)dst; io.dst_bytes = (size_t)G.w * G.h * channels * plan.es;
    io.run_bytes = jda_pack_run_bytes(plan.hwc != 0, plan.es, G.w, G.h); io.runs = jda_pack_runs(plan.hwc != 0, G.bpp);
    io.written.assign(io.dst_bytes, 0);
    io.lds.assign(JDA_PACK_LDS_DWORDS(plan.es), 0xEEEEEEEEu); io.lds_set.assign(io.lds.size(), 0);
    io.err = 0;
    int e;
    if (plan.hwc) e = plan.es == 1u ? run<1, 1>(io, G, io.table) : plan.es == 2u ? run<1, 2>(io, G, io.table) : run<1, 4>(io, G, io.table);
    else e = plan.es == 1u ? run<0, 1>(io, G, io.table) : plan.es == 2u ? run<0, 2>(io, G, io.table) : run<0, 4>(io, G, io.table);
    if (e) return e;
    for (uint8_t b : io.written) if (!b) return -24;
    return 0;
}

// the argument checks of jda_pack_surfaces (behind its ctx / n == 0 checks) on HOST pointers that are never followed: the status it
// would return, and in *n_tiles (may be NULL) the size of the launch
extern "C" int packsim_check(int n, const jda_output *src, int bpp, const int32_t *rects, int layout_flags, int elem_type, const void *table, void *const *dst,
                             uint32_t *n_tiles)
{
    jda_pack_plan_out plan;
    const int rc = jda_pack_plan_jobs(n, src, bpp, rects, layout_flags, elem_type, table, dst, &plan);
    if (n_tiles) *n_tiles = plan.n_tiles;
    return rc;
}
