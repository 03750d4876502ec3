// tests/hostsim/orient_sim.cpp -- TEST INFRASTRUCTURE: the orient kernel's tile schedule on the CPU.
//
// orientsim_lanes runs jda_orient_tiles (jpegdec_amd/csrc/jda_kernels.hip) the way the GPU runs it: every tile of the destination, the
// 256 lanes of a tile one after the other through the kernel's OWN code (jda_orient_rows / _stage / _emit of jda_device_core.h), the
// stage of all lanes before the emit of any (the workgroup barrier).  Memory goes through an IO policy that holds every access to what
// the kernel promises: aligned, inside the source rows' aligned extent, inside the destination's visible rectangle, narrower than a
// dword only in a row's last partial dword (narrower than a vector only in its last partial vector, orientations 0-4), every
// destination byte written once; LDS reads only what the stage wrote; and it counts the LDS bank conflicts of every wavefront-wide
// access (bank = dword address % 32, per 32-lane half).  orientsim_rowmajor is the twin that knows none of this (orient_twin.h).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_device_core.h"
#include "orient_twin.h"

namespace {
struct SimIO {
    const uint8_t *src; size_t src_bytes; uint32_t src_pitch, src_row_bytes, src_vec;      // src_vec: 16 (0-4) or 4 (5-8): the unit rows are read in
    uint8_t *dst; uint32_t dst_pitch, dst_row_bytes, dst_rows;
    bool transposing;
    std::vector<uint8_t> *written;
    std::vector<uint32_t> lds; std::vector<uint8_t> lds_set;
    std::vector<uint32_t> *log;              // this lane's LDS dword addresses, in program order
    int err;
    void fail(int e) { if (!err) err = e; }
    bool src_ok(const uint8_t *p, uint32_t n)
    {
        const size_t off = (size_t)(p - src);
        if (p < src || off + n > src_bytes || (off % n)) { fail(-10); return false; }
        const uint32_t in_row = (uint32_t)(off % src_pitch);
        const uint32_t extent = (src_row_bytes + src_vec - 1u) / src_vec * src_vec;
        if (in_row + n > extent) { fail(-11); return false; }       // (behind the aligned end of the row's pixels)
        return true;
    }
    uint32_t ld32(const uint8_t *p) { uint32_t v = 0; if (src_ok(p, 4)) memcpy(&v, p, 4); return v; }
    void ld128(const uint8_t *p, uint32_t *v) { if (src_ok(p, 16)) memcpy(v, p, 16); else memset(v, 0, 16); }
    bool dst_ok(uint8_t *p, uint32_t n)
    {
        const size_t off = (size_t)(p - dst);
        if (p < dst || (off % n)) { fail(-20); return false; }
        const uint32_t row = (uint32_t)(off / dst_pitch), in_row = (uint32_t)(off % dst_pitch);
        if (row >= dst_rows || in_row + n > dst_row_bytes) { fail(-21); return false; }      // outside the visible rectangle
        // narrower than the path's unit only in the row's last partial unit
        const uint32_t unit = transposing ? 4u : 16u;
        if (n < unit && in_row < dst_row_bytes / unit * unit) { fail(-22); return false; }
        for (uint32_t i = 0; i < n; i++) { uint8_t &w = (*written)[(size_t)row * dst_row_bytes + in_row + i]; if (w) fail(-23); w = 1; }
        return true;
    }
    void st128(uint8_t *p, const uint32_t *v) { if (dst_ok(p, 16)) memcpy(p, v, 16); }
    void st32(uint8_t *p, uint32_t v) { if (dst_ok(p, 4)) memcpy(p, &v, 4); }
    void st16(uint8_t *p, uint32_t v) { const uint16_t h = (uint16_t)v; if (dst_ok(p, 2)) memcpy(p, &h, 2); }
    void st8(uint8_t *p, uint32_t v) { if (dst_ok(p, 1)) *p = (uint8_t)v; }
    void lds_wr(uint32_t i, uint32_t v) { if (i >= lds.size()) { fail(-30); return; } lds[i] = v; lds_set[i] = 1; log->push_back(i); }
    uint32_t lds_rd(uint32_t i) { if (i >= lds.size() || !lds_set[i]) { fail(-31); return 0; } log->push_back(i); return lds[i]; }
};
// extra LDS cycles of the accesses the 64 lanes of a wavefront made (the k-th access of every lane is one instruction)
long conflicts_of(const std::vector<uint32_t> *logs)
{
    long extra = 0;
    size_t n = 0;
    for (int l = 0; l < 64; l++) if (logs[l].size() > n) n = logs[l].size();
    for (size_t k = 0; k < n; k++)
        for (int half = 0; half < 2; half++) {
            std::vector<uint32_t> bank[32];
            for (int l = half * 32; l < half * 32 + 32; l++) {
                if (logs[l].size() <= k) continue;
                const uint32_t a = logs[l][k];
                std::vector<uint32_t> &b = bank[a % 32u];
                bool seen = false;
                for (uint32_t x : b) seen |= x == a;               // the same address is a broadcast
                if (!seen) b.push_back(a);
            }
            size_t worst = 1;
            for (int b = 0; b < 32; b++) if (bank[b].size() > worst) worst = bank[b].size();
            extra += (long)worst - 1;
        }
    return extra;
}
template <int BPP> int run(SimIO &io, const jda_orient_geo &G, long *conflicts)
{
    uint32_t tiles_x, tiles_y;
    jda_orient_tile_grid(G.o, BPP, G.w, G.h, tiles_x, tiles_y);
    // the kernel's own way from a flat tile number to its surface and tile: three jobs, this one in the middle
    jda_orient_job jobs[3];
    memset(jobs, 0, sizeof(jobs));
    jobs[0].tile0 = 0; jobs[1].tile0 = 7; jobs[2].tile0 = 7 + tiles_x * tiles_y;
    const bool trans = jda_orient_transposes(G.o);
    for (uint32_t tile = 7; tile < 7 + tiles_x * tiles_y; tile++) {
        if (jda_orient_find_job(jobs, 3, tile) != 1u) return -40;
        const uint32_t local = tile - 7u, ty = local / tiles_x, tx = local - ty * tiles_x;
        std::fill(io.lds_set.begin(), io.lds_set.end(), 0);
        std::vector<uint32_t> logs[JDA_ORIENT_THREADS];
        for (uint32_t tid = 0; tid < JDA_ORIENT_THREADS; tid++) {
            io.log = &logs[tid];
            if (!trans) jda_orient_rows<BPP>(G, tx, ty, tid, io); else jda_orient_stage<BPP>(G, tx, ty, tid, io);
        }
        if (!trans) continue;
        for (int w = 0; w < JDA_ORIENT_THREADS / 64; w++) *conflicts += conflicts_of(&logs[64 * w]);
        for (uint32_t tid = 0; tid < JDA_ORIENT_THREADS; tid++) { logs[tid].clear(); io.log = &logs[tid]; jda_orient_emit<BPP>(G, tx, ty, tid, io); }
        for (int w = 0; w < JDA_ORIENT_THREADS / 64; w++) *conflicts += conflicts_of(&logs[64 * w]);
    }
    return io.err;
}
}

extern "C" int orientsim_rowmajor(const uint8_t *src, int src_pitch, int w, int h, int bpp, int o, uint8_t *dst, int dst_pitch)
{
    return orient_twin_rowmajor(src, src_pitch, w, h, bpp, o, dst, dst_pitch);
}

// src: h rows of src_pitch bytes; dst: the oriented rows of dst_pitch bytes.  *lds_conflicts (may be NULL): extra LDS cycles over every
// wavefront-wide LDS access.  0, or the first promise broken (-1x source, -2x destination, -3x LDS, -24: a visible byte not written).
extern "C" int orientsim_lanes(const uint8_t *src, int src_pitch, int w, int h, int bpp, int o, uint8_t *dst, int dst_pitch, long *lds_conflicts)
{
    if (w <= 0 || h <= 0 || o < 0 || o > 8 || (bpp != 1 && bpp != 2 && bpp != 4) || (src_pitch & 15) || (dst_pitch & 15)) return -1;
    if (((uintptr_t)src & 15u) || ((uintptr_t)dst & 15u)) return -1;
    jda_orient_geo G;
    G.src = src; G.dst = dst; G.src_pitch = (uint32_t)src_pitch; G.dst_pitch = (uint32_t)dst_pitch; G.w = (uint32_t)w; G.h = (uint32_t)h; G.o = (uint32_t)o;
    uint32_t dw, dh;
    jda_orient_dims(G.o, G.w, G.h, dw, dh);
    if ((uint32_t)src_pitch < G.w * (uint32_t)bpp || (uint32_t)dst_pitch < dw * (uint32_t)bpp) return -1;
    std::vector<uint8_t> written((size_t)dw * bpp * dh, 0);
    SimIO io;
    io.src = src; io.src_bytes = (size_t)src_pitch * h; io.src_pitch = G.src_pitch; io.src_row_bytes = G.w * (uint32_t)bpp;
    io.transposing = jda_orient_transposes(G.o); io.src_vec = io.transposing ? 4u : 16u;
    io.dst = dst; io.dst_pitch = G.dst_pitch; io.dst_row_bytes = dw * (uint32_t)bpp; io.dst_rows = dh;
    io.written = &written; io.err = 0; io.log = NULL;
    io.lds.assign(JDA_ORIENT_LDS_DWORDS((uint32_t)bpp), 0xEEEEEEEEu); io.lds_set.assign(io.lds.size(), 0);
    long conflicts = 0;
    const int rc = bpp == 4 ? run<4>(io, G, &conflicts) : bpp == 2 ? run<2>(io, G, &conflicts) : run<1>(io, G, &conflicts);
    if (lds_conflicts) *lds_conflicts = conflicts;
    if (rc) return rc;
    for (uint8_t b : written) if (!b) return -24;
    return 0;
}
