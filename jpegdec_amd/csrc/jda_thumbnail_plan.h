// jda_thumbnail_plan.h -- HOST: Pillow 12's Image.thumbnail((req_w, req_h), F, reducing_gap) of a JPEG file restated in C doubles: the
// aspect-preserving final size (preserve_aspect_ratio / round_aspect), JpegImageFile.draft's scale and box, and the reducing_gap branch of
// Image.resize (the factors, _get_safe_box, the box the resize receives behind the reduce).  Python's floats are IEEE doubles and every
// step below is one Python operation: compile this header with -ffp-contract=off, as jda_resize_plan.h.  No HIP in here: the runtime
// (jda_thumbnail_plan, jda_decode_to_host_thumbnail) and the CPU tests (tests/hostsim/reduce_sim.cpp) run the same code.
#ifndef JDA_THUMBNAIL_PLAN_H
#define JDA_THUMBNAIL_PLAN_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "jda_reduce_plan.h"
#include "jda_resize_plan.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// draft()'s scale: the largest of 8, 4, 2, 1 not above min(w / req_w, h / req_h), integer divisions (jda_exact_draft_scale's rule)
static inline int32_t jda_thumbnail_draft_scale(int32_t w, int32_t h, int32_t req_w, int32_t req_h)
{
    if (req_w <= 0 || req_h <= 0 || w <= 0 || h <= 0) return 1;
    const int32_t a = w / req_w, b = h / req_h, k = a < b ? a : b;
    return k >= 8 ? 8 : k >= 4 ? 4 : k >= 2 ? 2 : 1;
}
// int(v) of a positive Python float, held inside an int32 (a request that large divides every image to 0: scale 1)
static inline int32_t jda_thumbnail_int(double v) { return v >= 2147483647.0 ? 2147483647 : (int32_t)v; }

static inline int jda_thumbnail_plan_of(int32_t src_w, int32_t src_h, int32_t req_w, int32_t req_h, int32_t filter, double gap, jda_thumbnail_steps *P)
{
    if (!P) return JDA_INVALID_PARAMETER;
    memset(P, 0, sizeof(*P));
    P->scale = 1; P->fx = P->fy = 1;
    if (src_w <= 0 || src_h <= 0 || req_w <= 0 || req_h <= 0 || filter < 0 || filter >= JDA_RESIZE_FILTERS) return JDA_INVALID_PARAMETER;
    if (!(gap == 0.0 || gap >= 1.0)) return JDA_INVALID_PARAMETER;                     // (a NaN fails both)
    P->out_w = P->draft_w = P->reduced_w = src_w; P->out_h = P->draft_h = P->reduced_h = src_h;
    P->reduce_box[2] = src_w; P->reduce_box[3] = src_h; P->box[2] = (float)src_w; P->box[3] = (float)src_h;
    if (req_w >= src_w && req_h >= src_h) return JDA_SUCCESS;                          // the request holds the image: thumbnail() returns at once
    // preserve_aspect_ratio: the side the request does not bind follows the aspect; of floor and ceil the one that keeps it better, the
    // floor on a tie (min takes the first), at least 1
    {
        const double aspect = (double)src_w / (double)src_h;
        double x = (double)req_w, y = (double)req_h;
        if (x / y >= aspect) {
            const double number = y * aspect, f = floor(number), c = ceil(number);
            const double kf = fabs(aspect - f / y), kc = fabs(aspect - c / y);
            x = kc < kf ? c : f;
            if (x < 1.0) x = 1.0;
        } else {
            const double number = x / aspect, f = floor(number), c = ceil(number);
            const double kf = f == 0.0 ? 0.0 : fabs(aspect - x / f), kc = c == 0.0 ? 0.0 : fabs(aspect - x / c);
            y = kc < kf ? c : f;
            if (y < 1.0) y = 1.0;
        }
        P->out_w = (int32_t)x; P->out_h = (int32_t)y;
    }
    // draft(None, (int(req_w gap), int(req_h gap))): the decode's scale, im.size and the box draft() hands back
    if (gap != 0.0) P->scale = jda_thumbnail_draft_scale(src_w, src_h, jda_thumbnail_int((double)req_w * gap), jda_thumbnail_int((double)req_h * gap));
    P->draft_w = P->reduced_w = (src_w + P->scale - 1) / P->scale; P->draft_h = P->reduced_h = (src_h + P->scale - 1) / P->scale;
    double box[4] = { 0.0, 0.0, (double)src_w / (double)P->scale, (double)src_h / (double)P->scale };
    P->reduce_box[2] = P->draft_w; P->reduce_box[3] = P->draft_h;
    for (int i = 0; i < 4; i++) P->box[i] = (float)box[i];
    if (P->draft_w == P->out_w && P->draft_h == P->out_h) return JDA_SUCCESS;          // im.size == final_size: no resize
    P->resize = 1;
    int rc = JDA_SUCCESS;
    if (gap != 0.0) {
        // resize(reducing_gap=): whole factors that leave the resize at least `gap` to do, and the box the taps may read around
        const double fxd = (box[2] - box[0]) / (double)P->out_w / gap, fyd = (box[3] - box[1]) / (double)P->out_h / gap;
        const int32_t fx = jda_thumbnail_int(fxd) ? jda_thumbnail_int(fxd) : 1, fy = jda_thumbnail_int(fyd) ? jda_thumbnail_int(fyd) : 1;
        if (fx > 1 || fy > 1) {
            const double support = jda_resize_filter_support(filter) - 0.5;
            const double sx = support * ((box[2] - box[0]) / (double)P->out_w), sy = support * ((box[3] - box[1]) / (double)P->out_h);
            const double lo[2] = { box[0] - sx, box[1] - sy }, hi[2] = { ceil(box[2] + sx), ceil(box[3] + sy) };
            const int32_t size[2] = { P->draft_w, P->draft_h };
            for (int a = 0; a < 2; a++) {
                const int32_t l = (int32_t)lo[a];                                     // int(): towards zero
                P->reduce_box[a] = l > 0 ? l : 0;
                P->reduce_box[2 + a] = hi[a] < (double)size[a] ? (int32_t)hi[a] : size[a];
            }
            P->fx = fx; P->fy = fy;
            P->reduced_w = (int32_t)(((int64_t)P->reduce_box[2] - P->reduce_box[0] + fx - 1) / fx);
            P->reduced_h = (int32_t)(((int64_t)P->reduce_box[3] - P->reduce_box[1] + fy - 1) / fy);
            const double nb[4] = { (box[0] - (double)P->reduce_box[0]) / (double)fx, (box[1] - (double)P->reduce_box[1]) / (double)fy,
                                   (box[2] - (double)P->reduce_box[0]) / (double)fx, (box[3] - (double)P->reduce_box[1]) / (double)fy };
            for (int i = 0; i < 4; i++) { box[i] = nb[i]; P->box[i] = (float)nb[i]; }
            if (fx > JDA_REDUCE_MAX_FACTOR || fy > JDA_REDUCE_MAX_FACTOR) rc = JDA_UNSUPPORTED_FEATURE;
        }
    }
    // Pillow resizes an image more than 100 times as tall as wide in the other order of passes: other intermediates, not ours
    if ((int64_t)P->reduced_h > (int64_t)P->reduced_w * 100 && P->out_h < P->reduced_h) rc = JDA_UNSUPPORTED_FEATURE;
    if (rc == JDA_SUCCESS) {
        uint32_t k;
        rc = jda_resize_axis_ksize(P->box[0], P->box[2], P->out_w, &k, filter);
        if (rc == JDA_SUCCESS) rc = jda_resize_axis_ksize(P->box[1], P->box[3], P->out_h, &k, filter);
    }
    return rc;
}

#endif
