// jda_reduce_plan.h -- HOST: the arguments of jda_reduce_surfaces checked and turned into the job records and the tile list of one
// jda_reduce_tiles launch.  No HIP in here: the runtime (jda_runtime.cpp) and the CPU tests (tests/hostsim/reduce_sim.cpp) run the same
// checks and build the same records.  The rule, the tile and its LDS image: jda_rd_* in jda_device_core.h.
#ifndef JDA_REDUCE_PLAN_H
#define JDA_REDUCE_PLAN_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jda_device_core.h"

struct jda_reduce_plan_out {
    std::vector<jda_reduce_job> jobs;
    struct range { uintptr_t a, b; bool is_dst; };
    std::vector<range> ranges;           // what the launch reads and writes, sorted by start
    uint32_t n_tiles, lds_bytes;         // lds_bytes: what the largest tile of the launch needs
};

// Pillow's size of Image.reduce((fx, fy), box): ceil(box_w / fx) x ceil(box_h / fy).  JDA_INVALID_PARAMETER for a size or a factor below
// 1, JDA_UNSUPPORTED_FEATURE for a factor beyond JDA_REDUCE_MAX_FACTOR.
static inline int jda_reduce_geometry_of(int32_t box_w, int32_t box_h, int32_t fx, int32_t fy, int32_t *out_w, int32_t *out_h)
{
    if (out_w) *out_w = 0;
    if (out_h) *out_h = 0;
    if (box_w <= 0 || box_h <= 0 || fx <= 0 || fy <= 0) return JDA_INVALID_PARAMETER;
    if (fx > JDA_REDUCE_MAX_FACTOR || fy > JDA_REDUCE_MAX_FACTOR) return JDA_UNSUPPORTED_FEATURE;
    if (out_w) *out_w = (int32_t)(((int64_t)box_w + fx - 1) / fx);
    if (out_h) *out_h = (int32_t)(((int64_t)box_h + fy - 1) / fy);
    return JDA_SUCCESS;
}

// output rows of a tile: the most (<= JDA_RD_TILE_ROWS) whose LDS rows fit the budget (one at the factor cap)
static inline uint32_t jda_reduce_tile_rows(uint32_t fx, uint32_t out_h)
{
    const uint32_t fit = JDA_RD_LDS_BYTES / (jda_rd_row_entries(fx) * 8u);
    return std::max(1u, std::min(std::min<uint32_t>(JDA_RD_TILE_ROWS, out_h), fit));
}

// n >= 1 jobs.  factors: {fx, fy} per job.  boxes: {x0, y0, x1, y1} per job (half open, pixels), or NULL: the whole width_px x rows of
// every source.  dst[i].width_px x rows must be the reduced size of its box.
static inline int jda_reduce_plan_jobs(int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *factors, const int32_t *boxes,
                                       const jda_output *dst, jda_reduce_plan_out *plan)
{
    plan->jobs.clear(); plan->ranges.clear(); plan->n_tiles = 0; plan->lds_bytes = 0;
    if (bytes_per_pixel != 1 && bytes_per_pixel != 4) return JDA_INVALID_PARAMETER;
    if (n <= 0 || !src || !dst || !factors) return JDA_INVALID_PARAMETER;
    const uint32_t bpp = (uint32_t)bytes_per_pixel;
    plan->jobs.resize((size_t)n);
    plan->ranges.reserve((size_t)n * 2);
    uint64_t tiles = 0;
    uint32_t lds = 0;
    for (int i = 0; i < n; i++) {
        const jda_output &S = src[i], &D = dst[i];
        if (!S.pixels || !D.pixels || S.width_px <= 0 || S.rows <= 0 || D.width_px <= 0 || D.rows <= 0) return JDA_INVALID_PARAMETER;
        if (S.width_px > (1 << 24) || S.rows > (1 << 24) || D.width_px > (1 << 24) || D.rows > (1 << 24)) return JDA_INVALID_PARAMETER;
        if (((uintptr_t)S.pixels & 15u) || ((uintptr_t)D.pixels & 15u) || (S.pitch_bytes & 15) || (D.pitch_bytes & 15)) return JDA_INVALID_PARAMETER;
        if ((int64_t)S.pitch_bytes < (int64_t)S.width_px * bpp || (int64_t)D.pitch_bytes < (int64_t)D.width_px * bpp) return JDA_INVALID_PARAMETER;
        const int64_t x0 = boxes ? boxes[4 * i] : 0, y0 = boxes ? boxes[4 * i + 1] : 0, x1 = boxes ? boxes[4 * i + 2] : S.width_px, y1 = boxes ? boxes[4 * i + 3] : S.rows;
        if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > S.width_px || y1 > S.rows) return JDA_INVALID_PARAMETER;
        const int32_t fx = factors[2 * i], fy = factors[2 * i + 1];
        int32_t ow, oh;
        const int grc = jda_reduce_geometry_of((int32_t)(x1 - x0), (int32_t)(y1 - y0), fx, fy, &ow, &oh);
        if (grc != JDA_SUCCESS) return grc;
        if (D.width_px != ow || D.rows != oh) return JDA_INVALID_PARAMETER;
        // what the launch reads (the aligned dwords that hold a byte of a pixel of the box) and what it writes
        const uintptr_t s0 = (uintptr_t)S.pixels + (size_t)y0 * (size_t)S.pitch_bytes + (((size_t)x0 * bpp) & ~(size_t)3);
        const uintptr_t s1 = (uintptr_t)S.pixels + (size_t)(y1 - 1) * (size_t)S.pitch_bytes + (((size_t)x1 * bpp + 3u) & ~(size_t)3);
        plan->ranges.push_back({ s0, s1, false });
        plan->ranges.push_back({ (uintptr_t)D.pixels, (uintptr_t)D.pixels + (size_t)(D.rows - 1) * (size_t)D.pitch_bytes + (size_t)D.width_px * bpp, true });
        jda_reduce_job &J = plan->jobs[(size_t)i];
        J.src = (const uint8_t *)S.pixels; J.dst = (uint8_t *)D.pixels;
        J.src_pitch = (uint32_t)S.pitch_bytes; J.dst_pitch = (uint32_t)D.pitch_bytes;
        J.x0 = (uint32_t)x0; J.y0 = (uint32_t)y0; J.bw = (uint32_t)(x1 - x0); J.bh = (uint32_t)(y1 - y0);
        J.fx = (uint32_t)fx; J.fy = (uint32_t)fy; J.out_w = (uint32_t)ow; J.out_h = (uint32_t)oh;
        J.th = jda_reduce_tile_rows(J.fx, J.out_h);
        J.row_entries = jda_rd_row_entries(J.fx);
        const uint32_t rx = J.bw % J.fx ? J.bw % J.fx : J.fx, ry = J.bh % J.fy ? J.bh % J.fy : J.fy;      // the last column's and the last row's cells
        J.mul[0] = (1u << 24) / (J.fx * J.fy); J.mul[1] = (1u << 24) / (rx * J.fy); J.mul[2] = (1u << 24) / (J.fx * ry); J.mul[3] = (1u << 24) / (rx * ry);
        J.tiles_x = (J.out_w * bpp + JDA_RD_TILE_BYTES - 1u) / JDA_RD_TILE_BYTES;
        J.tile0 = (uint32_t)tiles;
        tiles += (uint64_t)J.tiles_x * ((J.out_h + J.th - 1u) / J.th);
        if (tiles > 0x7fffffffull) return JDA_INVALID_PARAMETER;
        lds = std::max(lds, J.th * J.row_entries * 8u);
    }
    // a destination may share no byte with a source or with another destination (as jda_resize_plan_jobs checks it)
    std::sort(plan->ranges.begin(), plan->ranges.end(), [](const jda_reduce_plan_out::range &p, const jda_reduce_plan_out::range &q) { return p.a < q.a; });
    uintptr_t end_any = 0, end_dst = 0;
    for (const jda_reduce_plan_out::range &r : plan->ranges) {
        if (r.is_dst ? r.a < end_any : r.a < end_dst) return JDA_INVALID_PARAMETER;
        end_any = std::max(end_any, r.b);
        if (r.is_dst) end_dst = std::max(end_dst, r.b);
    }
    plan->n_tiles = (uint32_t)tiles;
    plan->lds_bytes = lds;
    return JDA_SUCCESS;
}

#endif
