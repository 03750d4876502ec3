// tests/hostsim/reduce_sim.cpp -- TEST INFRASTRUCTURE: the reduce kernel's schedule, the float-box taps and the thumbnail plan on the CPU.
//
// reducesim_lanes runs jda_reduce_tiles (jpegdec_amd/csrc/jda_kernels.hip) the way the GPU runs it: every tile of the plan's tile list, the
// 256 lanes of a tile one after the other through the kernel's OWN code (jda_rd_load / jda_rd_store of jda_device_core.h), the load phase of
// all lanes before the store phase of any (the workgroup barrier), over the job record the host plan makes (jda_reduce_plan.h).  Memory goes
// through an IO policy that holds every access to what the kernel promises: source loads are aligned dwords inside the source allocation
// that hold a byte of a pixel of the box, in a row of the tile that runs; LDS (poisoned before every tile) is written inside the tile's
// th x row_entries entries, no entry twice, and read only where this workgroup wrote it; every store is aligned to its own width, lies
// inside out_w * bpp of a row in front of out_h, is narrower than a vector only in the vector that holds the row's end, and no destination
// byte is written twice -- and in the end every one once.  The caller guard-fills the surface around out_w x out_h.
// The rest are the host's own functions behind C names: the argument checks of jda_reduce_surfaces and jda_resize_surfaces_box, the tap
// table of an axis with fractional ends, the tables a resize plan makes, and jda_thumbnail_plan.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_thumbnail_plan.h"

namespace {
struct RdIO {
    const uint8_t *src; uint32_t src_pitch, src_rows, bpp;
    uint32_t bx0, by0, bx1, by1;                     // the job's box
    uint32_t tile_y0, tile_y1;                       // the source rows of the tile that runs
    uint8_t *dst; uint32_t dst_pitch, out_w, out_h;
    std::vector<uint8_t> written;                    // out_h x out_w * bpp
    std::vector<uint32_t> lds; std::vector<uint8_t> lds_set;      // (per 8-byte entry)
    uint32_t tile_entries;
    uint64_t loads;
    int err;
    void fail(int e) { if (!err) err = e; }
    uint32_t ld32(const uint8_t *p)
    {
        const size_t off = (size_t)(p - src);
        if (p < src || (off & 3u) || off + 4u > (size_t)src_pitch * src_rows) { fail(-10); return 0; }
        const uint32_t row = (uint32_t)(off / src_pitch), in_row = (uint32_t)(off % src_pitch);
        if (in_row + 4u > src_pitch) { fail(-11); return 0; }
        if (row < tile_y0 || row >= tile_y1 || row < by0 || row >= by1) { fail(-12); return 0; }                       // (not a row of this tile's cells)
        if (in_row < ((bx0 * bpp) & ~3u) || in_row + 4u > ((bx1 * bpp + 3u) & ~3u)) { fail(-13); return 0; }            // (no byte of a pixel of the box)
        loads++;
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
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
    void lds_wr64(uint32_t e, uint32_t w0, uint32_t w1)
    {
        if (e >= tile_entries || 2u * e + 2u > lds.size()) { fail(-30); return; }
        if (lds_set[e]) fail(-32);
        lds[2u * e] = w0; lds[2u * e + 1u] = w1; lds_set[e] = 1;
    }
    void lds_rd64(uint32_t e, uint32_t *v)
    {
        if (e >= tile_entries || !lds_set[e]) { fail(-31); v[0] = v[1] = 0; return; }
        v[0] = lds[2u * e]; v[1] = lds[2u * e + 1u];
    }
    uint32_t lds_rd16(uint32_t h)
    {
        const uint32_t e = h >> 2;
        if (e >= tile_entries || !lds_set[e]) { fail(-31); return 0; }
        return (lds[h >> 1] >> (16u * (h & 1u))) & 0xffffu;
    }
};
template <int BPP> int run(RdIO &io, const jda_reduce_job &J, uint32_t n_tiles)
{
    jda_rd_geo G;
    G.src = J.src; G.dst = J.dst; G.src_pitch = J.src_pitch; G.dst_pitch = J.dst_pitch; G.x0 = J.x0; G.y0 = J.y0; G.bw = J.bw; G.bh = J.bh;
    G.fx = J.fx; G.fy = J.fy; G.out_w = J.out_w; G.out_h = J.out_h; G.th = J.th; G.row_entries = J.row_entries;
    G.mul_whole = J.mul[0]; G.mul_right = J.mul[1]; G.mul_bottom = J.mul[2]; G.mul_corner = J.mul[3];
    // the kernel's own way from a flat tile number to its job: three jobs, this one in the middle
    jda_reduce_job jobs[3];
    memset(jobs, 0, sizeof(jobs));
    jobs[0].tile0 = 0; jobs[1] = J; jobs[1].tile0 = 5; jobs[2].tile0 = 5 + n_tiles;
    for (uint32_t tile = 5; tile < 5 + n_tiles; tile++) {
        if (jda_rd_find_job(jobs, 3, tile) != 1u) return -40;
        const uint32_t local = tile - 5u, ty = local / J.tiles_x, tx = local - ty * J.tiles_x;
        std::fill(io.lds_set.begin(), io.lds_set.end(), 0);      // a workgroup finds nothing in LDS
        std::fill(io.lds.begin(), io.lds.end(), 0xEEEEEEEEu);
        const uint32_t oy0 = ty * J.th, oy1 = oy0 + J.th < J.out_h ? oy0 + J.th : J.out_h;
        io.tile_y0 = J.y0 + oy0 * J.fy;
        io.tile_y1 = J.y0 + (oy1 * J.fy < J.bh ? oy1 * J.fy : J.bh);
        for (uint32_t tid = 0; tid < JDA_RD_THREADS; tid++) jda_rd_load<BPP>(G, tx, ty, tid, io);
        for (uint32_t tid = 0; tid < JDA_RD_THREADS; tid++) jda_rd_store<BPP>(G, tx, ty, tid, io);
    }
    return io.err;
}
void output_of(jda_output &O, const void *p, int pitch, int w, int rows) { O.pixels = (void *)p; O.pitch_bytes = pitch; O.width_px = w; O.rows = rows; }
}

extern "C" int reducesim_geometry(int box_w, int box_h, int fx, int fy, int32_t *out_w, int32_t *out_h)
{
    return jda_reduce_geometry_of(box_w, box_h, fx, fy, out_w, out_h);
}

// src: rows rows of pitch bytes (16-byte aligned), width_px pixels wide; box: {x0, y0, x1, y1} or NULL; dst: out_w x out_h pixels at
// dst_pitch.  0, or the first promise broken (-1x loads, -2x stores, -3x LDS, -24: a destination byte not written, -4x the tile list), or the
// code the argument checks of jda_reduce_surfaces give.  info (may be NULL): {tiles, tile rows, lds bytes, row entries, dword loads}.
extern "C" int reducesim_lanes(const uint8_t *src, int pitch, int width_px, int rows, int bpp, int fx, int fy, const int32_t *box, uint8_t *dst, int dst_pitch,
                               int out_w, int out_h, uint32_t *info)
{
    jda_output S, D;
    output_of(S, src, pitch, width_px, rows);
    output_of(D, dst, dst_pitch, out_w, out_h);
    const int32_t factors[2] = { fx, fy };
    jda_reduce_plan_out plan;
    const int rc = jda_reduce_plan_jobs(1, &S, bpp, factors, box, &D, &plan);
    if (rc != JDA_SUCCESS) return rc;
    const jda_reduce_job &J = plan.jobs[0];
    if (J.th == 0u || J.th > JDA_RD_TILE_ROWS || plan.n_tiles != J.tiles_x * ((J.out_h + J.th - 1u) / J.th)) return -42;
    if (plan.lds_bytes != J.th * J.row_entries * 8u || plan.lds_bytes > JDA_RD_LDS_BYTES) return -43;
    RdIO io;
    io.src = src; io.src_pitch = (uint32_t)pitch; io.src_rows = (uint32_t)rows; io.bpp = (uint32_t)bpp;
    io.bx0 = J.x0; io.by0 = J.y0; io.bx1 = J.x0 + J.bw; io.by1 = J.y0 + J.bh;
    io.dst = dst; io.dst_pitch = (uint32_t)dst_pitch; io.out_w = J.out_w; io.out_h = J.out_h;
    io.written.assign((size_t)J.out_h * J.out_w * (uint32_t)bpp, 0);
    io.lds.assign(plan.lds_bytes / 4u, 0xEEEEEEEEu); io.lds_set.assign(plan.lds_bytes / 8u, 0);
    io.tile_entries = J.th * J.row_entries;
    io.loads = 0; io.err = 0;
    const int e = bpp == 4 ? run<4>(io, J, plan.n_tiles) : run<1>(io, J, plan.n_tiles);
    if (info) { info[0] = plan.n_tiles; info[1] = J.th; info[2] = plan.lds_bytes; info[3] = J.row_entries; info[4] = (uint32_t)io.loads; }
    if (e) return e;
    for (uint8_t b : io.written) if (!b) return -24;
    return 0;
}

// the argument checks of jda_reduce_surfaces (behind its ctx / n == 0 checks) on HOST pointers that are never followed: the status it
// would return.  info (may be NULL): {tiles, lds bytes}.
extern "C" int reducesim_check(int n, const jda_output *src, int bpp, const int32_t *factors, const int32_t *boxes, const jda_output *dst, uint32_t *info)
{
    jda_reduce_plan_out plan;
    const int rc = jda_reduce_plan_jobs(n, src, bpp, factors, boxes, dst, &plan);
    if (info) { info[0] = plan.n_tiles; info[1] = plan.lds_bytes; }
    return rc;
}

// the host's table of one axis with fractional ends (jda_resize_plan.h): out[2 i] = min, out[2 i + 1] = cnt, out[2 out_size + i ksize + x] =
// k[x]; returns ksize, or minus the status the plan gives, or -100 when cap (dwords) is too small
extern "C" int reducesim_taps_box(int filter, int in_size, float in0, float in1, int out_size, int32_t *out, int cap)
{
    uint32_t ksize;
    const int rc = jda_resize_axis_ksize(in0, in1, out_size, &ksize, filter);
    if (rc != JDA_SUCCESS) return -rc;
    if ((int64_t)out_size * (2 + (int64_t)ksize) > cap) return -100;
    const int grc = jda_resize_axis_taps(in_size, in0, in1, out_size, ksize, out, filter);
    return grc == JDA_SUCCESS ? (int)ksize : -grc;
}

// the plan of one resize job on HOST pointers that are never followed: rect = {x, y, w, h} through jda_resize_plan_jobs (the integer entry)
// or, rect == NULL, fbox = {x0, y0, x1, y1} through jda_resize_plan_jobs_box.  The status; tables (may be NULL) receives the launch's
// table block when it fits cap dwords; info: {table dwords, tiles, lds bytes, reads x0, y0, x1, y1}.
extern "C" int reducesim_resize_plan(const jda_output *src, int bpp, const int32_t *rect, const float *fbox, const jda_output *dst, int filter, int32_t *tables, int cap,
                                     int32_t *info)
{
    jda_resize_plan_out plan;
    const int rc = rect ? jda_resize_plan_jobs(1, src, bpp, rect, dst, &plan, filter) : jda_resize_plan_jobs_box(1, src, bpp, fbox, dst, &plan, filter);
    if (info) {
        info[0] = (int32_t)plan.tables.size(); info[1] = (int32_t)plan.n_tiles; info[2] = (int32_t)plan.lds_bytes;
        for (int i = 0; i < 4; i++) info[3 + i] = plan.reads.size() >= 4 ? plan.reads[(size_t)i] : 0;
    }
    if (rc == JDA_SUCCESS && tables && (int)plan.tables.size() <= cap) memcpy(tables, plan.tables.data(), plan.tables.size() * sizeof(int32_t));
    return rc;
}

// n float-box jobs: the argument checks of jda_resize_surfaces_box
extern "C" int reducesim_resize_check_box(int n, const jda_output *src, int bpp, const float *boxes, const jda_output *dst, int filter)
{
    jda_resize_plan_out plan;
    return jda_resize_plan_jobs_box(n, src, bpp, boxes, dst, &plan, filter);
}

extern "C" int reducesim_thumbnail_plan(int src_w, int src_h, int req_w, int req_h, int filter, double gap, jda_thumbnail_steps *plan)
{
    return jda_thumbnail_plan_of(src_w, src_h, req_w, req_h, filter, gap, plan);
}
