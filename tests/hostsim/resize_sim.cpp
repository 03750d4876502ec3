// tests/hostsim/resize_sim.cpp -- TEST INFRASTRUCTURE: the resize kernel's schedule on the CPU.
//
// resizesim_lanes runs jda_resize_tiles (jpegdec_amd/csrc/jda_kernels.hip) the way the GPU runs it: every tile of the plan's tile list, the
// 256 lanes of a tile one after the other through the kernel's OWN code (jda_rs_tile_rows / jda_rs_horizontal / jda_rs_vertical of
// jda_device_core.h), the horizontal pass of all lanes before the vertical pass of any (the workgroup barrier), over the job record and the
// tap tables the host plan makes (jda_resize_plan.h).  Memory goes through an IO policy that holds every access to what the kernel promises:
// source loads are aligned dwords inside the pitch that hold a byte of a pixel the horizontal taps read, in a row this tile's vertical
// taps read; tap loads lie inside the job's two tables; LDS is written inside the tile's span x 64 dwords and read only where this
// workgroup wrote it; every store is aligned to its own width, lies inside out_w * bpp of a row in front of out_h, is narrower than a
// vector only in the vector that holds the row's end, and no destination byte is written twice -- and in the end every one once.
// resizesim_rowmajor is the twin that knows none of this (resize_twin.h); resizesim_taps gives the host's tap table of one axis;
// resizesim_check runs the argument checks of jda_resize_surfaces without a GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_resize_plan.h"
#include "resize_twin.h"

namespace {
struct SimIO {
    const uint8_t *src; uint32_t src_pitch, src_rows, bpp;
    int32_t rd[4];                                   // the job's source pixels {x0, y0, x1, y1}
    uint32_t tile_row0, tile_span;                   // the source rows of the tile that runs
    const int32_t *tables; uint32_t htab0, htab1, vtab0, vtab1;
    uint8_t *dst; uint32_t dst_pitch, out_w, out_h;
    std::vector<uint8_t> written;                    // out_h x out_w * bpp
    std::vector<uint32_t> lds; std::vector<uint8_t> lds_set;
    int err;
    void fail(int e) { if (!err) err = e; }
    uint32_t ld32(const uint8_t *p)
    {
        const size_t off = (size_t)(p - src);
        if (p < src || (off & 3u) || off + 4u > (size_t)src_pitch * src_rows) { fail(-10); return 0; }
        const uint32_t row = (uint32_t)(off / src_pitch), in_row = (uint32_t)(off % src_pitch);
        if (in_row + 4u > src_pitch) { fail(-11); return 0; }
        if (row < tile_row0 || row >= tile_row0 + tile_span || row < (uint32_t)rd[1] || row >= (uint32_t)rd[3]) { fail(-12); return 0; }      // (not a row the vertical taps name)
        if (in_row < (((uint32_t)rd[0] * bpp) & ~3u) || in_row + 4u > (((uint32_t)rd[2] * bpp + 3u) & ~3u)) { fail(-13); return 0; }        // (no byte of a pixel the taps read)
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    uint32_t ld_tap(uint32_t i)
    {
        if (!((i >= htab0 && i < htab1) || (i >= vtab0 && i < vtab1))) { fail(-14); return 0; }
        return (uint32_t)tables[i];
    }
    bool dst_ok(uint8_t *p, uint32_t n)
    {
        if (((uintptr_t)p % n) != 0) { fail(-20); return false; }
        const size_t off = (size_t)(p - dst);
        const uint32_t row = (uint32_t)(off / dst_pitch), in_row = (uint32_t)(off % dst_pitch), row_bytes = out_w * bpp;
        if (p < dst || row >= out_h || in_row + n > row_bytes) { fail(-21); return false; }      // behind the row or behind the image
        if (n < 16u && (in_row & ~15u) + 16u <= row_bytes) { fail(-22); return false; }            // a narrow store in a whole vector
        for (uint32_t i = 0; i < n; i++) { uint8_t &w = written[(size_t)row * row_bytes + in_row + i]; if (w) fail(-23); w = 1; }
        return true;
    }
    void st128(uint8_t *p, const uint32_t *v) { if (dst_ok(p, 16)) memcpy(p, v, 16); }
    void st32(uint8_t *p, uint32_t v) { if (dst_ok(p, 4)) memcpy(p, &v, 4); }
    void st8(uint8_t *p, uint32_t v) { if (dst_ok(p, 1)) *p = (uint8_t)v; }
    void lds_wr(uint32_t i, uint32_t v) { if (i >= lds.size() || i >= tile_span * JDA_RS_TILE_DWORDS) { fail(-30); return; } lds[i] = v; lds_set[i] = 1; }
    void lds_rd128(uint32_t i, uint32_t *v)
    {
        if ((i & 3u) || i + 4u > lds.size() || !lds_set[i] || !lds_set[i + 1] || !lds_set[i + 2] || !lds_set[i + 3]) { fail(-31); memset(v, 0, 16); return; }
        memcpy(v, &lds[i], 16);
    }
};
template <int BPP> int run(SimIO &io, const jda_resize_job &J, uint32_t n_tiles)
{
    jda_rs_geo G;
    G.src = J.src; G.dst = J.dst; G.src_pitch = J.src_pitch; G.dst_pitch = J.dst_pitch; G.out_w = J.out_w; G.out_h = J.out_h;
    G.htab = J.htab; G.vtab = J.vtab; G.hk = J.hk; G.vk = J.vk; G.th = J.th;
    // the kernel's own way from a flat tile number to its job: three jobs, this one in the middle
    jda_resize_job jobs[3];
    memset(jobs, 0, sizeof(jobs));
    jobs[0].tile0 = 0; jobs[1] = J; jobs[1].tile0 = 5; jobs[2].tile0 = 5 + n_tiles;
    for (uint32_t tile = 5; tile < 5 + n_tiles; tile++) {
        if (jda_rs_find_job(jobs, 3, tile) != 1u) return -40;
        const uint32_t local = tile - 5u, ty = local / J.tiles_x, tx = local - ty * J.tiles_x;
        std::fill(io.lds_set.begin(), io.lds_set.end(), 0);      // a workgroup finds nothing in LDS
        uint32_t oy0, row0, span;
        io.tile_row0 = 0; io.tile_span = 0;
        jda_rs_tile_rows(G, ty, io, oy0, row0, span);
        if (span == 0u || span > JDA_RS_LDS_ROWS || span * JDA_RS_TILE_DWORDS > io.lds.size()) return -41;
        io.tile_row0 = row0; io.tile_span = span;
        for (uint32_t tid = 0; tid < JDA_RS_THREADS; tid++) jda_rs_horizontal<BPP>(G, tx, row0, span, tid, io);
        for (uint32_t tid = 0; tid < JDA_RS_THREADS; tid++) jda_rs_vertical<BPP>(G, tx, oy0, row0, tid, io);
    }
    return io.err;
}
}

extern "C" int resizesim_rowmajor(const uint8_t *src, int pitch, int width, int rows, int bpp, int x, int y, int w, int h, uint8_t *dst, int dst_pitch, int out_w, int out_h)
{
    return resize_twin_rowmajor(src, pitch, width, rows, bpp, x, y, w, h, dst, dst_pitch, out_w, out_h);
}

// the host's table of one axis (jda_resize_plan.h): out[2 i] = min, out[2 i + 1] = cnt, out[2 out_size + i ksize + x] = k[x]; returns
// ksize, or minus the status the plan gives, or -100 when cap (dwords) is too small
extern "C" int resizesim_taps(int in_size, int in0, int in1, int out_size, int32_t *out, int cap)
{
    uint32_t ksize;
    const int rc = jda_resize_axis_ksize(in0, in1, out_size, &ksize);
    if (rc != JDA_SUCCESS) return -rc;
    if ((int64_t)out_size * (2 + (int64_t)ksize) > cap) return -100;
    jda_resize_axis_taps(in_size, in0, in1, out_size, ksize, out);
    return (int)ksize;
}

// src: rows rows of pitch bytes (16-byte aligned), width_px pixels wide; {x, y, w, h}: the box; dst: out_w x out_h pixels at dst_pitch.
// 0, or the first promise broken (-1x loads, -2x stores, -3x LDS, -24: a destination byte not written, -4x the tile list), or the code
// the argument checks of jda_resize_surfaces give.  info (may be NULL): {tiles, tile rows, lds bytes, horizontal ksize, vertical ksize}.
extern "C" int resizesim_lanes(const uint8_t *src, int pitch, int width_px, int rows, int bpp, int x, int y, int w, int h, uint8_t *dst, int dst_pitch,
                               int out_w, int out_h, uint32_t *info)
{
    jda_output S, D;
    S.pixels = (void *)src; S.pitch_bytes = pitch; S.width_px = width_px; S.rows = rows;
    D.pixels = dst; D.pitch_bytes = dst_pitch; D.width_px = out_w; D.rows = out_h;
    const int32_t rect[4] = { x, y, w, h };
    jda_resize_plan_out plan;
    const int rc = jda_resize_plan_jobs(1, &S, bpp, rect, &D, &plan);
    if (rc != JDA_SUCCESS) return rc;
    const jda_resize_job &J = plan.jobs[0];
    if (info) { info[0] = plan.n_tiles; info[1] = J.th; info[2] = plan.lds_bytes; info[3] = J.hk; info[4] = J.vk; }
    if (J.th == 0u || J.th > JDA_RS_TILE_ROWS || plan.n_tiles != J.tiles_x * ((J.out_h + J.th - 1u) / J.th)) return -42;
    SimIO io;
    io.src = src; io.src_pitch = (uint32_t)pitch; io.src_rows = (uint32_t)rows; io.bpp = (uint32_t)bpp;
    memcpy(io.rd, plan.reads.data(), sizeof(io.rd));
    io.tables = plan.tables.data();
    io.htab0 = J.htab; io.htab1 = J.htab + J.out_w * (2u + J.hk); io.vtab0 = J.vtab; io.vtab1 = J.vtab + J.out_h * (2u + J.vk);
    if (io.htab1 > plan.tables.size() || io.vtab1 > plan.tables.size()) return -43;
    io.dst = dst; io.dst_pitch = (uint32_t)dst_pitch; io.out_w = J.out_w; io.out_h = J.out_h;
    io.written.assign((size_t)J.out_h * J.out_w * (uint32_t)bpp, 0);
    io.lds.assign(plan.lds_bytes / 4u, 0xEEEEEEEEu); io.lds_set.assign(io.lds.size(), 0);
    io.err = 0;
    const int e = bpp == 4 ? run<4>(io, J, plan.n_tiles) : run<1>(io, J, plan.n_tiles);
    if (e) return e;
    for (uint8_t b : io.written) if (!b) return -24;
    return 0;
}

// the argument checks of jda_resize_surfaces (behind its ctx / n == 0 checks) on HOST pointers that are never followed: the status it
// would return; tables_at (may be NULL: not checked): where the launch's tables would lie.  info (may be NULL): {tiles, lds bytes, table bytes}.
extern "C" int resizesim_check(int n, const jda_output *src, int bpp, const int32_t *rects, const jda_output *dst, const void *tables_at, uint32_t *info)
{
    jda_resize_plan_out plan;
    int rc = jda_resize_plan_jobs(n, src, bpp, rects, dst, &plan);
    if (rc == JDA_SUCCESS && tables_at) rc = jda_resize_plan_place(&plan, tables_at);
    if (info) { info[0] = plan.n_tiles; info[1] = plan.lds_bytes; info[2] = (uint32_t)(plan.tables.size() * 4u); }
    return rc;
}
