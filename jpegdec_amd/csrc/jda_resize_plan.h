// jda_resize_plan.h -- HOST: the arguments of jda_resize_surfaces checked and turned into the job records, the tap tables and the tile
// list of one jda_resize_tiles launch.  No HIP in here: the runtime (jda_runtime.cpp) and the CPU tests (tests/hostsim/resize_sim.cpp)
// run the same checks and build the same tables.
//
// The taps are Pillow's (src/libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc with one of its five filters), in double, in
// Pillow's order of operations: compile this header with -ffp-contract=off -- a fused multiply-add in `center` or in w / ww moves a
// coefficient by one.
#ifndef JDA_RESIZE_PLAN_H
#define JDA_RESIZE_PLAN_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <vector>

#include "jda_device_core.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

struct jda_resize_plan_out {
    std::vector<jda_resize_job> jobs;
    std::vector<int32_t> tables;         // every axis table of the launch (the layout: jda_rs_* in jda_device_core.h); jobs with equal axes share
    std::vector<int32_t> reads;          // per job {x0, y0, x1, y1}: the source pixels its taps read (half open)
    struct range { uintptr_t a, b; bool is_dst; };
    std::vector<range> ranges;           // what the launch reads and writes, sorted by start (the table block is not among them)
    uint32_t n_tiles, lds_bytes;         // lds_bytes: what the largest tile of the launch needs
};

// The filters (the ids of include/jpegdec_amd.h: JDA_RESIZE_BILINEAR .. JDA_RESIZE_LANCZOS) are Pillow's, in double, in Pillow's order of
// operations, with the C library's sin / cos.  Support, the taps of an upscale and the largest downscale below JDA_RESIZE_MAX_KSIZE = 161:
//   BOX 0.5: 3 taps, 160 : 1     BILINEAR 1: 3 taps, 80 : 1     HAMMING 1: 3 taps, 80 : 1     BICUBIC 2: 5 taps, 40 : 1
//   LANCZOS 3: 7 taps, 26.6 : 1
// BICUBIC and LANCZOS have negative taps: the SIGNED filters, for which the kernel has instances of its own (jda_rs_* in jda_device_core.h).
#define JDA_RESIZE_FILTERS 5
// (Pillow writes the window's two constants as float literals: they enter the double arithmetic as 0.54f and 0.46f, and a tap in a few
// hundred differs by one from what 0.54 and 0.46 give)
#define JDA_RESIZE_HAMMING_A ((double)0.54f)
#define JDA_RESIZE_HAMMING_B ((double)0.46f)
static inline bool jda_resize_filter_signed(int32_t filter) { return filter == JDA_RESIZE_BICUBIC || filter == JDA_RESIZE_LANCZOS; }
static inline double jda_resize_filter_support(int32_t filter)
{
    return filter == JDA_RESIZE_BOX ? 0.5 : filter == JDA_RESIZE_BICUBIC ? 2.0 : filter == JDA_RESIZE_LANCZOS ? 3.0 : 1.0;
}
static inline double jda_resize_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static inline double jda_resize_filter_weight(int32_t filter, double x)
{
    switch (filter) {
    case JDA_RESIZE_BOX:
        return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case JDA_RESIZE_HAMMING:
        if (x < 0.0) x = -x;
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * M_PI;
        return sin(x) / x * (JDA_RESIZE_HAMMING_A + JDA_RESIZE_HAMMING_B * cos(x));
    case JDA_RESIZE_BICUBIC: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    case JDA_RESIZE_LANCZOS:
        return -3.0 <= x && x < 3.0 ? jda_resize_sinc(x) * jda_resize_sinc(x / 3) : 0.0;
    default:
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
}

// coefficients per output coordinate of an axis that takes [in0, in1) to out_size; JDA_UNSUPPORTED_FEATURE past JDA_RESIZE_MAX_KSIZE,
// JDA_INVALID_PARAMETER for a filter id that is none
static inline int jda_resize_scale_ksize(double scale, uint32_t *ksize, int32_t filter)
{
    *ksize = 0;
    if (filter < 0 || filter >= JDA_RESIZE_FILTERS) return JDA_INVALID_PARAMETER;
    const double support = jda_resize_filter_support(filter) * (scale < 1.0 ? 1.0 : scale);
    const double c = ceil(support);
    if (c * 2.0 + 1.0 > (double)JDA_RESIZE_MAX_KSIZE) return JDA_UNSUPPORTED_FEATURE;
    *ksize = (uint32_t)((int)c * 2 + 1);
    return JDA_SUCCESS;
}
static inline int jda_resize_axis_ksize(int32_t in0, int32_t in1, int32_t out_size, uint32_t *ksize, int32_t filter = JDA_RESIZE_BILINEAR)
{
    return jda_resize_scale_ksize((double)(in1 - in0) / (double)out_size, ksize, filter);
}
// A FRACTIONAL [in0, in1), Pillow's resize(box = a float box): Pillow's C side holds the box as `float`, so both ends are float32 values
// (a caller's double is rounded when it becomes the argument) and the box's length is their difference ROUNDED TO FLOAT32 (in1 - in0 of two
// floats); only then everything is double: scale = (double)(in1 - in0) / out_size, center = in0 + (xx + 0.5) * scale.  A box kept in
// double, or a length taken in double, moves a tap by one in about a case in a hundred.  Whole numbers below 2^24 give the integer
// entry points' values.
static inline double jda_resize_box_scale(float in0, float in1, int32_t out_size)
{
    const volatile float len = in1 - in0;            // (volatile: rounded to float32 whatever precision the compiler evaluates in)
    return (double)len / (double)out_size;
}
static inline int jda_resize_axis_ksize(float in0, float in1, int32_t out_size, uint32_t *ksize, int32_t filter = JDA_RESIZE_BILINEAR)
{
    return jda_resize_scale_ksize(jda_resize_box_scale(in0, in1, out_size), ksize, filter);
}

// what the kernel's arithmetic leans on, checked on every table made for a filter other than BILINEAR (whose taps are 0 .. 2^22 by
// construction): a signed filter's taps fit the signed 24-bit multiply (|k| < 2^23) and the 32-bit sum of every output coordinate
// (255 * the positive taps + 2^21 < 2^31, 255 * the negative taps + 2^21 > -2^31); BOX and HAMMING have no negative tap, as the unsigned
// instances need.  JDA_UNSUPPORTED_FEATURE for a table that fails.
static inline int jda_resize_axis_guard(int32_t filter, const int32_t *tab, int32_t out_size, uint32_t ksize)
{
    if (filter == JDA_RESIZE_BILINEAR) return JDA_SUCCESS;
    const bool sgn = jda_resize_filter_signed(filter);
    const int32_t *k = tab + 2 * (size_t)out_size;
    for (int32_t xx = 0; xx < out_size; xx++, k += ksize) {
        int64_t pos = 0, neg = 0;
        for (uint32_t x = 0; x < ksize; x++) {
            if (k[x] <= -(1 << 23) || k[x] >= (1 << 23) || (!sgn && k[x] < 0)) return JDA_UNSUPPORTED_FEATURE;
            if (k[x] > 0) pos += k[x]; else neg += k[x];
        }
        if (255 * pos + (1 << 21) >= ((int64_t)1 << 31) || 255 * neg + (1 << 21) <= -((int64_t)1 << 31)) return JDA_UNSUPPORTED_FEATURE;
    }
    return JDA_SUCCESS;
}

// the table of one axis: tab[2 i] = min, tab[2 i + 1] = cnt, tab[2 out_size + i ksize + x] = k[x] (zero behind cnt); the guard's answer
static inline int jda_resize_scale_taps(int32_t in_size, double in0, double scale, int32_t out_size, uint32_t ksize, int32_t *tab, int32_t filter)
{
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = jda_resize_filter_support(filter) * fs, ss = 1.0 / fs;
    std::vector<double> w((size_t)ksize);
    int32_t *k = tab + 2 * (size_t)out_size;
    for (int32_t xx = 0; xx < out_size; xx++, k += ksize) {
        const double center = in0 + ((double)xx + 0.5) * scale;
        int32_t xmin = (int32_t)(center - support + 0.5), xmax = (int32_t)(center + support + 0.5);
        if (xmin < 0) xmin = 0;
        if (xmax > in_size) xmax = in_size;
        const int32_t cnt = xmax - xmin;
        double ww = 0.0;
        for (int32_t x = 0; x < cnt; x++) {
            w[(size_t)x] = jda_resize_filter_weight(filter, ((double)(x + xmin) - center + 0.5) * ss);
            ww += w[(size_t)x];
        }
        for (int32_t x = 0; x < (int32_t)ksize; x++) {
            if (x >= cnt) { k[x] = 0; continue; }
            const double v = ww != 0.0 ? w[(size_t)x] / ww : w[(size_t)x];
            k[x] = v < 0.0 ? (int32_t)(-0.5 + v * 4194304.0) : (int32_t)(0.5 + v * 4194304.0);
        }
        tab[2 * xx] = xmin; tab[2 * xx + 1] = cnt;
    }
    return jda_resize_axis_guard(filter, tab, out_size, ksize);
}
static inline int jda_resize_axis_taps(int32_t in_size, int32_t in0, int32_t in1, int32_t out_size, uint32_t ksize, int32_t *tab,
                                       int32_t filter = JDA_RESIZE_BILINEAR)
{
    return jda_resize_scale_taps(in_size, (double)in0, (double)(in1 - in0) / (double)out_size, out_size, ksize, tab, filter);
}
// .. of a fractional [in0, in1) (see jda_resize_axis_ksize's)
static inline int jda_resize_axis_taps(int32_t in_size, float in0, float in1, int32_t out_size, uint32_t ksize, int32_t *tab,
                                       int32_t filter = JDA_RESIZE_BILINEAR)
{
    return jda_resize_scale_taps(in_size, (double)in0, jda_resize_box_scale(in0, in1, out_size), out_size, ksize, tab, filter);
}

// output rows of a tile: the most (<= JDA_RS_TILE_ROWS) with which every tile's source rows fit the LDS budget (one at the ksize cap)
static inline uint32_t jda_resize_tile_rows(const int32_t *vtab, uint32_t out_h, uint32_t *max_span)
{
    for (uint32_t th = std::min<uint32_t>(JDA_RS_TILE_ROWS, out_h); th >= 1u; th--) {
        uint32_t worst = 0;
        for (uint32_t oy0 = 0; oy0 < out_h; oy0 += th) {
            const uint32_t last = std::min(oy0 + th, out_h) - 1u;
            worst = std::max(worst, (uint32_t)(vtab[2 * last] + vtab[2 * last + 1] - vtab[2 * oy0]));
        }
        if (worst <= JDA_RS_LDS_ROWS || th == 1u) { *max_span = worst; return th; }
    }
    *max_span = 0;
    return 1u;
}

// n >= 1 jobs, one filter for all of them.  rects: {x, y, w, h} per job, or NULL: the whole width_px x rows of every source.  dst[i].width_px x rows is the output size.
// fboxes (jda_resize_surfaces_box; rects is then NULL): {x0, y0, x1, y1} per job, fractional, Pillow's conditions on them: 0 <= x0 < x1 <=
// width_px and the same for y (a NaN fails them).  An axis table is shared by the jobs whose key -- source size, the two ends (the
// floats' bits, and a mark that they are floats) and output size -- is the same.
static inline int jda_resize_plan_jobs_any(int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const float *fboxes,
                                           const jda_output *dst, jda_resize_plan_out *plan, int32_t filter)
{
    plan->jobs.clear(); plan->tables.clear(); plan->reads.clear(); plan->ranges.clear(); plan->n_tiles = 0; plan->lds_bytes = 0;
    if (bytes_per_pixel != 1 && bytes_per_pixel != 4) return JDA_INVALID_PARAMETER;
    if (n <= 0 || !src || !dst || filter < 0 || filter >= JDA_RESIZE_FILTERS) return JDA_INVALID_PARAMETER;
    const uint32_t bpp = (uint32_t)bytes_per_pixel;
    struct axis { uint32_t off, ksize, th, span; int32_t r0, r1; };
    std::map<std::array<int32_t, 5>, axis> axes;
    plan->jobs.resize((size_t)n);
    plan->reads.resize((size_t)n * 4);
    plan->ranges.reserve((size_t)n * 2);
    uint64_t tiles = 0;
    uint32_t max_span = 0;
    for (int i = 0; i < n; i++) {
        const jda_output &S = src[i], &D = dst[i];
        if (!S.pixels || !D.pixels || S.width_px <= 0 || S.rows <= 0 || D.width_px <= 0 || D.rows <= 0) return JDA_INVALID_PARAMETER;
        if (S.width_px > (1 << 24) || S.rows > (1 << 24) || D.width_px > (1 << 24) || D.rows > (1 << 24)) return JDA_INVALID_PARAMETER;
        if (((uintptr_t)S.pixels & 15u) || ((uintptr_t)D.pixels & 15u) || (S.pitch_bytes & 15) || (D.pitch_bytes & 15)) return JDA_INVALID_PARAMETER;
        if ((int64_t)S.pitch_bytes < (int64_t)S.width_px * bpp || (int64_t)D.pitch_bytes < (int64_t)D.width_px * bpp) return JDA_INVALID_PARAMETER;
        const int64_t x = rects ? rects[4 * i] : 0, y = rects ? rects[4 * i + 1] : 0, w = rects ? rects[4 * i + 2] : S.width_px, h = rects ? rects[4 * i + 3] : S.rows;
        if (!fboxes && (x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > S.width_px || y + h > S.rows)) return JDA_INVALID_PARAMETER;
        std::array<int32_t, 5> keys[2] = { { S.width_px, (int32_t)x, (int32_t)(x + w), D.width_px, 0 }, { S.rows, (int32_t)y, (int32_t)(y + h), D.rows, 0 } };
        const float *fb = fboxes ? fboxes + 4 * (size_t)i : NULL;
        if (fb) {
            if (!(fb[0] >= 0.0f && fb[0] < fb[2] && fb[2] <= (float)S.width_px && fb[1] >= 0.0f && fb[1] < fb[3] && fb[3] <= (float)S.rows)) return JDA_INVALID_PARAMETER;
            for (int a = 0; a < 2; a++) { memcpy(&keys[a][1], &fb[a], 4); memcpy(&keys[a][2], &fb[2 + a], 4); keys[a][4] = 1; }
        }
        const axis *A[2];
        for (int a = 0; a < 2; a++) {
            auto it = axes.find(keys[a]);
            if (it == axes.end()) {
                axis N;
                const int krc = fb ? jda_resize_axis_ksize(fb[a], fb[2 + a], keys[a][3], &N.ksize, filter) : jda_resize_axis_ksize(keys[a][1], keys[a][2], keys[a][3], &N.ksize, filter);
                if (krc != JDA_SUCCESS) return krc;
                const uint64_t dwords = (uint64_t)keys[a][3] * (2u + N.ksize);
                if ((plan->tables.size() + dwords) * 4u > (uint64_t)JDA_RESIZE_MAX_TABLE_BYTES) return JDA_UNSUPPORTED_FEATURE;
                N.off = (uint32_t)plan->tables.size();
                plan->tables.resize(plan->tables.size() + (size_t)dwords);
                int32_t *tab = plan->tables.data() + N.off;
                const int grc = fb ? jda_resize_axis_taps(keys[a][0], fb[a], fb[2 + a], keys[a][3], N.ksize, tab, filter)
                                   : jda_resize_axis_taps(keys[a][0], keys[a][1], keys[a][2], keys[a][3], N.ksize, tab, filter);
                if (grc != JDA_SUCCESS) return grc;
                const int32_t last = keys[a][3] - 1;
                N.r0 = tab[0]; N.r1 = tab[2 * last] + tab[2 * last + 1];
                N.th = 0; N.span = 0;
                it = axes.emplace(keys[a], N).first;
            }
            if (a == 1 && it->second.th == 0u) it->second.th = jda_resize_tile_rows(plan->tables.data() + it->second.off, (uint32_t)D.rows, &it->second.span);
            A[a] = &it->second;
        }
        if (A[1]->span > JDA_RS_LDS_ROWS) return JDA_UNSUPPORTED_FEATURE;          // (cannot happen below the ksize cap: cnt <= ksize)
        max_span = std::max(max_span, A[1]->span);
        int32_t *R = &plan->reads[(size_t)i * 4];
        R[0] = A[0]->r0; R[1] = A[1]->r0; R[2] = A[0]->r1; R[3] = A[1]->r1;
        // what the launch reads (the aligned dwords that hold a byte of a pixel the taps name) and what it writes
        const uintptr_t s0 = (uintptr_t)S.pixels + (size_t)R[1] * (size_t)S.pitch_bytes + (((size_t)R[0] * bpp) & ~(size_t)3);
        const uintptr_t s1 = (uintptr_t)S.pixels + (size_t)(R[3] - 1) * (size_t)S.pitch_bytes + (((size_t)R[2] * bpp + 3u) & ~(size_t)3);
        plan->ranges.push_back({ s0, s1, false });
        plan->ranges.push_back({ (uintptr_t)D.pixels, (uintptr_t)D.pixels + (size_t)(D.rows - 1) * (size_t)D.pitch_bytes + (size_t)D.width_px * bpp, true });
        jda_resize_job &J = plan->jobs[(size_t)i];
        J.src = (const uint8_t *)S.pixels; J.dst = (uint8_t *)D.pixels;
        J.src_pitch = (uint32_t)S.pitch_bytes; J.dst_pitch = (uint32_t)D.pitch_bytes;
        J.out_w = (uint32_t)D.width_px; J.out_h = (uint32_t)D.rows;
        J.htab = A[0]->off; J.vtab = A[1]->off; J.hk = A[0]->ksize; J.vk = A[1]->ksize;
        J.th = A[1]->th; J.pad_ = 0;
        J.tiles_x = (J.out_w * bpp + JDA_RS_TILE_DWORDS * 4u - 1u) / (JDA_RS_TILE_DWORDS * 4u);
        J.tile0 = (uint32_t)tiles;
        tiles += (uint64_t)J.tiles_x * ((J.out_h + J.th - 1u) / J.th);
        if (tiles > 0x7fffffffull) return JDA_INVALID_PARAMETER;
    }
    // a destination may share no byte with a source or with another destination (as jda_orient_surfaces checks it)
    std::sort(plan->ranges.begin(), plan->ranges.end(), [](const jda_resize_plan_out::range &p, const jda_resize_plan_out::range &q) { return p.a < q.a; });
    uintptr_t end_any = 0, end_dst = 0;
    for (const jda_resize_plan_out::range &r : plan->ranges) {
        if (r.is_dst ? r.a < end_any : r.a < end_dst) return JDA_INVALID_PARAMETER;
        end_any = std::max(end_any, r.b);
        if (r.is_dst) end_dst = std::max(end_dst, r.b);
    }
    plan->n_tiles = (uint32_t)tiles;
    plan->lds_bytes = max_span * JDA_RS_TILE_DWORDS * 4u;
    return JDA_SUCCESS;
}

static inline int jda_resize_plan_jobs(int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst,
                                       jda_resize_plan_out *plan, int32_t filter = JDA_RESIZE_BILINEAR)
{
    return jda_resize_plan_jobs_any(n, src, bytes_per_pixel, rects, NULL, dst, plan, filter);
}
// Pillow's resize(size, F, box = a float box) per job: boxes = {x0, y0, x1, y1} (NULL is an error: jda_resize_surfaces takes whole sources)
static inline int jda_resize_plan_jobs_box(int32_t n, const jda_output *src, int32_t bytes_per_pixel, const float *boxes, const jda_output *dst,
                                           jda_resize_plan_out *plan, int32_t filter)
{
    if (!boxes) { plan->jobs.clear(); plan->tables.clear(); plan->reads.clear(); plan->ranges.clear(); plan->n_tiles = 0; plan->lds_bytes = 0; return JDA_INVALID_PARAMETER; }
    return jda_resize_plan_jobs_any(n, src, bytes_per_pixel, NULL, boxes, dst, plan, filter);
}

// .. nor with the launch's tables, once it is known where they lie: [tables_at, tables_at + 4 * tables.size())
static inline int jda_resize_plan_place(const jda_resize_plan_out *plan, const void *tables_at)
{
    const uintptr_t a = (uintptr_t)tables_at, b = a + plan->tables.size() * sizeof(int32_t);
    if (!tables_at || (a & 15u)) return JDA_INVALID_PARAMETER;
    for (const jda_resize_plan_out::range &r : plan->ranges)
        if (r.is_dst && r.a < b && a < r.b) return JDA_INVALID_PARAMETER;
    return JDA_SUCCESS;
}

#endif
