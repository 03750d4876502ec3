// tests/hostsim/unpack_sim.cpp -- TEST INFRASTRUCTURE: the unpack kernel's schedule on the CPU.
//
// unpacksim_lanes runs jda_unpack_tiles (jpegdec_amd/csrc/jda_kernels.hip) the way the GPU runs it: every tile of the job, the 256 lanes of
// a tile one after the other through the kernel's OWN code (jda_unpack_tile of jda_device_core.h).  Memory goes through an IO policy that
// holds every access to what the kernel promises: a source load is an aligned dword that holds at least one byte of the job's dense image;
// every store is aligned to its own width, lies inside the w * bpp bytes of one of the h rows, is narrower than a vector only in the last
// vector of its row, and no destination byte is written twice; at the end every byte of every row has been written.  unpacksim_rowmajor is
// the twin that knows none of this (unpack_twin.h); unpacksim_check runs the argument checks of jda_unpack_surfaces (jda_unpack_plan.h)
// without a GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_unpack_plan.h"
#include "unpack_twin.h"

namespace {
struct SimIO {
    const uint8_t *src; size_t src_bytes;
    uint8_t *dst; uint32_t pitch, row_bytes, rows;
    std::vector<uint8_t> written;        // rows * row_bytes
    int err;
    void fail(int e) { if (!err) err = e; }
    uint32_t ld32(const uint8_t *p)
    {
        if ((uintptr_t)p & 3u) { fail(-10); return 0; }
        if (p + 4 <= src || p >= src + src_bytes) { fail(-11); return 0; }        // (no byte of the image in it)
        uint32_t v;
        memcpy(&v, p, 4);
        return v;
    }
    bool dst_ok(uint8_t *p, uint32_t n)
    {
        if (((uintptr_t)p % n) != 0) { fail(-20); return false; }
        if (p < dst) { fail(-21); return false; }
        const size_t off = (size_t)(p - dst), row = off / pitch, in_row = off % pitch;
        if (row >= rows || in_row + n > row_bytes) { fail(-21); return false; }      // the padding, or behind the last row
        if (n < 16u && (in_row & ~(size_t)15) + 16u <= row_bytes) { fail(-22); return false; }       // a narrow store inside a whole vector
        for (uint32_t i = 0; i < n; i++) { uint8_t &w = written[row * row_bytes + in_row + i]; if (w) fail(-23); w = 1; }
        return true;
    }
    void st128(uint8_t *p, const uint32_t *v) { if (dst_ok(p, 16)) memcpy(p, v, 16); }
    void st32(uint8_t *p, uint32_t v) { if (dst_ok(p, 4)) memcpy(p, &v, 4); }
    void st16(uint8_t *p, uint32_t v) { const uint16_t h = (uint16_t)v; if (dst_ok(p, 2)) memcpy(p, &h, 2); }
    void st8(uint8_t *p, uint32_t v) { if (dst_ok(p, 1)) *p = (uint8_t)v; }
};
template <int HWC, int ES> int run(SimIO &io, const jda_unpack_geo &G)
{
    const uint32_t tiles = jda_unpack_tiles_of(G.w, G.h, G.bpp);
    // the kernel's own way from a flat tile number to its job: three jobs, this one in the middle
    jda_unpack_job jobs[3];
    memset(jobs, 0, sizeof(jobs));
    jobs[0].tile0 = 0; jobs[1].tile0 = 5; jobs[2].tile0 = 5 + tiles;
    for (uint32_t tile = 5; tile < 5 + tiles; tile++) {
        if (jda_unpack_find_job(jobs, 3, tile) != 1u) return -40;
        for (uint32_t tid = 0; tid < JDA_UNPACK_THREADS; tid++) jda_unpack_tile<HWC, ES>(G, tile - 5u, tid, io);
    }
    return io.err;
}
}

extern "C" int unpacksim_rowmajor(const void *src, int w, int h, int layout_flags, int elem_type, const float *scale_bias, uint8_t *dst, int pitch, int bpp)
{
    return unpack_twin_rowmajor(src, w, h, layout_flags, elem_type, scale_bias, dst, pitch, bpp);
}

// src: dense, aligned to its element; dst: h rows at pitch (16-byte aligned).  0, or the first promise broken (-1x loads, -2x stores, -24: a
// byte of a row not written), or the code the argument checks of jda_unpack_surfaces give.
extern "C" int unpacksim_lanes(const void *src, int w, int h, int layout_flags, int elem_type, const float *scale_bias, uint8_t *dst, int pitch, int bpp)
{
    jda_output D;
    D.pixels = dst; D.pitch_bytes = pitch; D.width_px = w; D.rows = h;
    const void *const srcs[1] = { src };
    jda_unpack_plan_out plan;
    const int rc = jda_unpack_plan_jobs(1, srcs, layout_flags, elem_type, scale_bias, &D, bpp, &plan);
    if (rc != JDA_SUCCESS) return rc;
    const jda_unpack_job &J = plan.jobs[0];
    jda_unpack_geo G;
    G.src = J.src; G.dst = J.dst; G.dst_pitch = J.dst_pitch; G.w = J.w; G.h = J.h;
    G.bpp = (uint32_t)bpp; G.bgr = (layout_flags & JDA_PACK_BGR) ? 1u : 0u;
    for (int c = 0; c < 3; c++) { G.p.scale[c] = plan.scale_bias[c]; G.p.bias[c] = plan.scale_bias[3 + c]; }
    if (plan.n_tiles != jda_unpack_tiles_of(G.w, G.h, G.bpp)) return -41;
    SimIO io;
    io.src = (const uint8_t *)src; io.src_bytes = (size_t)G.w * G.h * (bpp == 4 ? 3u : 1u) * plan.es;
    io.dst = dst; io.pitch = (uint32_t)pitch; io.row_bytes = G.w * G.bpp; io.rows = G.h;
    io.written.assign((size_t)io.rows * io.row_bytes, 0);
    io.err = 0;
    int e;
    if (plan.hwc) e = plan.es == 1u ? run<1, 1>(io, G) : plan.es == 2u ? run<1, 2>(io, G) : run<1, 4>(io, G);
    else e = plan.es == 1u ? run<0, 1>(io, G) : plan.es == 2u ? run<0, 2>(io, G) : run<0, 4>(io, G);
    if (e) return e;
    for (uint8_t b : io.written) if (!b) return -24;
    return 0;
}

// the argument checks of jda_unpack_surfaces (behind its ctx / n == 0 checks) on HOST pointers that are never followed: the status it
// would return, and in *n_tiles (may be NULL) the size of the launch
extern "C" int unpacksim_check(int n, const void *const *src, int layout_flags, int elem_type, const float *scale_bias, const jda_output *dst, int bpp,
                               uint32_t *n_tiles)
{
    jda_unpack_plan_out plan;
    const int rc = jda_unpack_plan_jobs(n, src, layout_flags, elem_type, scale_bias, dst, bpp, &plan);
    if (n_tiles) *n_tiles = plan.n_tiles;
    return rc;
}
