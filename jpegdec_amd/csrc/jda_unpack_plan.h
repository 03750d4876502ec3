// jda_unpack_plan.h -- HOST: the arguments of jda_unpack_surfaces checked and turned into the job records of one jda_unpack_tiles launch.
// No HIP in here: the runtime (jda_runtime.cpp) and the CPU tests (tests/hostsim/unpack_sim.cpp) run the same checks.
#ifndef JDA_UNPACK_PLAN_H
#define JDA_UNPACK_PLAN_H

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jda_pack_plan.h"

struct jda_unpack_plan_out {
    std::vector<jda_unpack_job> jobs;
    uint32_t n_tiles, es, hwc;       // es: bytes of an element; hwc: the launch takes the pixel-major kernel (a gray image never does: one plane)
    float scale_bias[6];             // scale[0..2], bias[0..2] per tensor channel, the default (255, 0) where the caller gave none
};

// what the call says about every job; JDA_SUCCESS or JDA_INVALID_PARAMETER.  scale_bias: HOST, scale[0..C-1] then bias[0..C-1], or NULL
static inline int jda_unpack_check_format(int32_t dst_bytes_per_pixel, int32_t layout_flags, int32_t elem_type, const float *scale_bias)
{
    if (dst_bytes_per_pixel != 1 && dst_bytes_per_pixel != 4) return JDA_INVALID_PARAMETER;
    if (layout_flags & ~(JDA_PACK_CHW | JDA_PACK_BGR)) return JDA_INVALID_PARAMETER;
    const uint32_t es = jda_pack_elem_bytes(elem_type);
    if (!es) return JDA_INVALID_PARAMETER;
    if (es == 1u && scale_bias) return JDA_INVALID_PARAMETER;                          // bytes are taken as they are
    if ((layout_flags & JDA_PACK_BGR) && dst_bytes_per_pixel == 1) return JDA_INVALID_PARAMETER;
    if (scale_bias) {
        const int channels = dst_bytes_per_pixel == 4 ? 3 : 1;
        for (int i = 0; i < 2 * channels; i++) if (!std::isfinite(scale_bias[i])) return JDA_INVALID_PARAMETER;
    }
    return JDA_SUCCESS;
}

// a source (one dense piece: rows = 1) or the bytes a destination's rows hold: rows pieces of row_bytes, pitch apart
struct jda_unpack_range { uintptr_t a, end; size_t pitch, row_bytes, rows; bool is_dst; };
// does [s, e) share a byte with a piece of R?
static inline bool jda_unpack_piece_hits(uintptr_t s, uintptr_t e, const jda_unpack_range &R)
{
    if (e <= R.a || s >= R.end) return false;
    const size_t k = s <= R.a ? 0 : (size_t)(s - R.a) / R.pitch;                     // the last piece that begins at or in front of s
    if (k < R.rows && s < R.a + k * R.pitch + R.row_bytes) return true;
    return k + 1 < R.rows && e > R.a + (k + 1) * R.pitch;
}
static inline bool jda_unpack_ranges_hit(const jda_unpack_range &P, const jda_unpack_range &Q)
{
    const jda_unpack_range &few = P.rows <= Q.rows ? P : Q, &many = P.rows <= Q.rows ? Q : P;
    for (size_t r = 0; r < few.rows; r++)
        if (jda_unpack_piece_hits(few.a + r * few.pitch, few.a + r * few.pitch + few.row_bytes, many)) return true;
    return false;
}

// n >= 1 jobs: src[i] = the dense image of dst[i].width_px x dst[i].rows pixels
static inline int jda_unpack_plan_jobs(int32_t n, const void *const *src, int32_t layout_flags, int32_t elem_type, const float *scale_bias,
                                       const jda_output *dst, int32_t dst_bytes_per_pixel, jda_unpack_plan_out *plan)
{
    plan->jobs.clear(); plan->n_tiles = 0; plan->es = 0; plan->hwc = 0;
    for (int i = 0; i < 6; i++) plan->scale_bias[i] = i < 3 ? 255.f : 0.f;
    const int frc = jda_unpack_check_format(dst_bytes_per_pixel, layout_flags, elem_type, scale_bias);
    if (frc != JDA_SUCCESS) return frc;
    if (n <= 0 || !src || !dst) return JDA_INVALID_PARAMETER;
    const uint32_t bpp = (uint32_t)dst_bytes_per_pixel, es = jda_pack_elem_bytes(elem_type), channels = bpp == 4u ? 3u : 1u;
    const bool hwc = !(layout_flags & JDA_PACK_CHW) && channels == 3u;
    plan->es = es; plan->hwc = hwc ? 1u : 0u;
    if (scale_bias) for (uint32_t c = 0; c < channels; c++) { plan->scale_bias[c] = scale_bias[c]; plan->scale_bias[3 + c] = scale_bias[channels + c]; }
    plan->jobs.resize((size_t)n);
    std::vector<jda_unpack_range> ranges;
    ranges.reserve((size_t)n * 2);
    uint64_t tiles = 0;
    for (int i = 0; i < n; i++) {
        const jda_output &D = dst[i];
        if (!D.pixels || !src[i] || D.width_px <= 0 || D.rows <= 0) return JDA_INVALID_PARAMETER;
        if (((uintptr_t)D.pixels & 15u) || (D.pitch_bytes & 15) || ((uintptr_t)src[i] & (es - 1u))) return JDA_INVALID_PARAMETER;
        if ((int64_t)D.pitch_bytes < (int64_t)D.width_px * bpp) return JDA_INVALID_PARAMETER;
        const uint64_t bytes = (uint64_t)D.width_px * (uint64_t)D.rows * channels * es;
        if (bytes > JDA_PACK_MAX_BYTES) return JDA_INVALID_PARAMETER;
        // what the launch reads (the aligned dwords that hold a byte of the dense image) and what it writes (w * bpp bytes of every row)
        const uintptr_t s0 = (uintptr_t)src[i] & ~(uintptr_t)3, s1 = ((uintptr_t)src[i] + (size_t)bytes + 3u) & ~(uintptr_t)3;
        ranges.push_back({ s0, s1, (size_t)(s1 - s0), (size_t)(s1 - s0), 1, false });
        const size_t rb = (size_t)D.width_px * bpp;
        ranges.push_back({ (uintptr_t)D.pixels, (uintptr_t)D.pixels + (size_t)(D.rows - 1) * (size_t)D.pitch_bytes + rb, (size_t)D.pitch_bytes, rb, (size_t)D.rows, true });
        jda_unpack_job &J = plan->jobs[(size_t)i];
        J.src = (const uint8_t *)src[i]; J.dst = (uint8_t *)D.pixels;
        J.dst_pitch = (uint32_t)D.pitch_bytes; J.w = (uint32_t)D.width_px; J.h = (uint32_t)D.rows;
        J.tile0 = (uint32_t)tiles;
        tiles += jda_unpack_tiles_of(J.w, J.h, bpp);
        if (tiles > 0x7fffffffull) return JDA_INVALID_PARAMETER;
    }
    // a destination's written bytes may share no byte with a source or with another destination's: sorted by start, every range is held
    // against the ranges before it that end behind its start, row by row (the padding of a surface's rows is not written: two surfaces
    // may lie side by side in one canvas) -- two sources may share anything
    std::sort(ranges.begin(), ranges.end(), [](const jda_unpack_range &p, const jda_unpack_range &q) { return p.a < q.a; });
    std::vector<const jda_unpack_range *> open;
    for (const jda_unpack_range &r : ranges) {
        size_t keep = 0;
        for (size_t k = 0; k < open.size(); k++) if (open[k]->end > r.a) open[keep++] = open[k];
        open.resize(keep);
        for (const jda_unpack_range *q : open) if ((r.is_dst || q->is_dst) && jda_unpack_ranges_hit(r, *q)) return JDA_INVALID_PARAMETER;
        open.push_back(&r);
    }
    plan->n_tiles = (uint32_t)tiles;
    return JDA_SUCCESS;
}

#endif
