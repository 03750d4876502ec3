// jda_pack_plan.h -- HOST: the arguments of jda_pack_surfaces checked and turned into the job records of one jda_pack_tiles launch.
// No HIP in here: the runtime (jda_runtime.cpp) and the CPU tests (tests/hostsim/pack_sim.cpp) run the same checks.
#ifndef JDA_PACK_PLAN_H
#define JDA_PACK_PLAN_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jda_device_core.h"

struct jda_pack_plan_out {
    std::vector<jda_pack_job> jobs;
    uint32_t n_tiles, es, hwc;       // es: bytes of an element; hwc: the launch takes the pixel-major kernel (a gray source never does: one plane)
};

static inline uint32_t jda_pack_elem_bytes(int32_t elem_type) { return elem_type == JDA_PACK_U8 ? 1u : elem_type == JDA_PACK_F16 ? 2u : elem_type == JDA_PACK_F32 ? 4u : 0u; }

// what the call says about every job; JDA_SUCCESS or JDA_INVALID_PARAMETER
static inline int jda_pack_check_format(int32_t src_bytes_per_pixel, int32_t layout_flags, int32_t elem_type, const void *table)
{
    if (src_bytes_per_pixel != 1 && src_bytes_per_pixel != 4) return JDA_INVALID_PARAMETER;
    if (layout_flags & ~(JDA_PACK_CHW | JDA_PACK_BGR)) return JDA_INVALID_PARAMETER;
    const uint32_t es = jda_pack_elem_bytes(elem_type);
    if (!es) return JDA_INVALID_PARAMETER;
    if ((es == 1u) != (table == NULL)) return JDA_INVALID_PARAMETER;                   // a table with U8, none with F16 / F32
    if (table && ((uintptr_t)table & 15u)) return JDA_INVALID_PARAMETER;
    if ((layout_flags & JDA_PACK_BGR) && src_bytes_per_pixel == 1) return JDA_INVALID_PARAMETER;
    return JDA_SUCCESS;
}

// n >= 1 jobs.  rects: {x, y, w, h} per job, or NULL: the whole width_px x rows of every surface.
static inline int jda_pack_plan_jobs(int32_t n, const jda_output *src, int32_t src_bytes_per_pixel, const int32_t *rects, int32_t layout_flags,
                                     int32_t elem_type, const void *table, void *const *dst, jda_pack_plan_out *plan)
{
    plan->jobs.clear(); plan->n_tiles = 0; plan->es = 0; plan->hwc = 0;
    const int frc = jda_pack_check_format(src_bytes_per_pixel, layout_flags, elem_type, table);
    if (frc != JDA_SUCCESS) return frc;
    if (n <= 0 || !src || !dst) return JDA_INVALID_PARAMETER;
    const uint32_t bpp = (uint32_t)src_bytes_per_pixel, es = jda_pack_elem_bytes(elem_type), channels = bpp == 4u ? 3u : 1u;
    const bool hwc = !(layout_flags & JDA_PACK_CHW) && channels == 3u;
    plan->es = es; plan->hwc = hwc ? 1u : 0u;
    plan->jobs.resize((size_t)n);
    struct range { uintptr_t a, b; bool is_dst; };
    std::vector<range> ranges;
    ranges.reserve((size_t)n * 2 + 1);
    if (table) ranges.push_back({ (uintptr_t)table, (uintptr_t)table + (size_t)channels * 256u * es, false });
    uint64_t tiles = 0;
    for (int i = 0; i < n; i++) {
        const jda_output &S = src[i];
        if (!S.pixels || !dst[i] || S.width_px <= 0 || S.rows <= 0) return JDA_INVALID_PARAMETER;
        if (((uintptr_t)S.pixels & 15u) || (S.pitch_bytes & 15) || ((uintptr_t)dst[i] & (es - 1u))) return JDA_INVALID_PARAMETER;
        if ((int64_t)S.pitch_bytes < (int64_t)S.width_px * bpp) return JDA_INVALID_PARAMETER;
        const int64_t x = rects ? rects[4 * i] : 0, y = rects ? rects[4 * i + 1] : 0, w = rects ? rects[4 * i + 2] : S.width_px, h = rects ? rects[4 * i + 3] : S.rows;
        if (x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > S.width_px || y + h > S.rows) return JDA_INVALID_PARAMETER;
        const uint64_t bytes = (uint64_t)w * (uint64_t)h * channels * es;
        if (bytes > JDA_PACK_MAX_BYTES) return JDA_INVALID_PARAMETER;
        // what the launch reads (the aligned dwords that hold a pixel of the rectangle) and what it writes
        const uintptr_t s0 = (uintptr_t)S.pixels + (size_t)y * (size_t)S.pitch_bytes + ((size_t)(x * bpp) & ~(size_t)3);
        const uintptr_t s1 = (uintptr_t)S.pixels + (size_t)(y + h - 1) * (size_t)S.pitch_bytes + (((size_t)((x + w) * bpp) + 3u) & ~(size_t)3);
        ranges.push_back({ s0, s1, false });
        ranges.push_back({ (uintptr_t)dst[i], (uintptr_t)dst[i] + (size_t)bytes, true });
        jda_pack_job &J = plan->jobs[(size_t)i];
        J.src = (const uint8_t *)S.pixels; J.dst = (uint8_t *)dst[i];
        J.src_pitch = (uint32_t)S.pitch_bytes; J.x = (uint32_t)x; J.y = (uint32_t)y; J.w = (uint32_t)w; J.h = (uint32_t)h;
        J.tile0 = (uint32_t)tiles;
        tiles += jda_pack_tiles_of(jda_pack_run_bytes(hwc, es, J.w, J.h));
        if (tiles > 0x7fffffffull) return JDA_INVALID_PARAMETER;
    }
    // a destination may share no byte with a source (the table is one) or with another destination (as jda_orient_surfaces checks it)
    std::sort(ranges.begin(), ranges.end(), [](const range &p, const range &q) { return p.a < q.a; });
    uintptr_t end_any = 0, end_dst = 0;
    for (const range &r : ranges) {
        if (r.is_dst ? r.a < end_any : r.a < end_dst) return JDA_INVALID_PARAMETER;
        end_any = std::max(end_any, r.b);
        if (r.is_dst) end_dst = std::max(end_dst, r.b);
    }
    plan->n_tiles = (uint32_t)tiles;
    return JDA_SUCCESS;
}

#endif
