// tests/hostsim/thumb_main.cpp -- TEST INFRASTRUCTURE: the reduce plan and lane simulator, the float-box taps and the thumbnail plan
// (reduce_sim.cpp) as a program of its own, built under AddressSanitizer + UBSan (make thumbasan): nothing is loaded into an interpreter.
// It runs the reduce lanes for both pixel sizes over exactly sized heap blocks -- factors from 1 to the cap, boxes with an origin, partial
// cells, widths that end inside a vector and cross a tile --, compares them with the rule written out plainly, builds float-box tables into
// exactly sized blocks, walks the thumbnail plan over a grid of sizes, and asks for the refusals.  Exit status 0 and "thumb_asan ok" when
// every call answers as it must.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int reducesim_geometry(int box_w, int box_h, int fx, int fy, int32_t *out_w, int32_t *out_h);
extern "C" int reducesim_lanes(const uint8_t *src, int pitch, int width_px, int rows, int bpp, int fx, int fy, const int32_t *box, uint8_t *dst, int dst_pitch,
                               int out_w, int out_h, uint32_t *info);
extern "C" int reducesim_check(int n, const jda_output *src, int bpp, const int32_t *factors, const int32_t *boxes, const jda_output *dst, uint32_t *info);
extern "C" int reducesim_taps_box(int filter, int in_size, float in0, float in1, int out_size, int32_t *out, int cap);
extern "C" int reducesim_resize_check_box(int n, const jda_output *src, int bpp, const float *boxes, const jda_output *dst, int filter);
extern "C" int reducesim_thumbnail_plan(int src_w, int src_h, int req_w, int req_h, int filter, double gap, jda_thumbnail_steps *plan);

#define CHECK(c) do { if (!(c)) { printf("thumb_asan: line %d: %s\n", __LINE__, #c); fflush(stdout); return 1; } } while (0)

int main()
{
    uint32_t seed = 99991u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
    // {w, h, x0, y0, x1, y1, fx, fy}
    const int jobs[][8] = { { 70, 45, 0, 0, 70, 45, 2, 2 }, { 70, 45, 9, 6, 59, 37, 3, 5 }, { 333, 40, 1, 0, 333, 40, 1, 1 }, { 300, 70, 3, 2, 299, 69, 4, 7 },
                            { 64, 64, 0, 0, 64, 64, 32, 32 }, { 65, 33, 0, 0, 65, 33, 32, 1 }, { 33, 65, 0, 0, 33, 65, 1, 32 }, { 1, 1, 0, 0, 1, 1, 8, 8 },
                            { 1100, 20, 5, 1, 1099, 19, 2, 3 }, { 57, 23, 7, 0, 52, 23, 5, 11 } };
    for (const auto &j : jobs)
        for (int bpp = 1; bpp <= 4; bpp += 3) {
            int32_t ow, oh;
            CHECK(reducesim_geometry(j[4] - j[2], j[5] - j[3], j[6], j[7], &ow, &oh) == JDA_SUCCESS);
            const int spitch = (j[0] * bpp + 15) & ~15, dpitch = (ow * bpp + 15) & ~15;
            uint8_t *s = (uint8_t *)aligned_alloc(16, (size_t)spitch * j[1]), *d = (uint8_t *)aligned_alloc(16, (size_t)dpitch * oh);      // exactly the surfaces
            CHECK(s && d);
            for (size_t i = 0; i < (size_t)spitch * j[1]; i++) s[i] = (uint8_t)((rnd() & 1u) ? 255u : rnd());
            memset(d, 0x5a, (size_t)dpitch * oh);
            const int32_t box[4] = { j[2], j[3], j[4], j[5] };
            uint32_t info[5];
            CHECK(reducesim_lanes(s, spitch, j[0], j[1], bpp, j[6], j[7], box, d, dpitch, ow, oh, info) == 0);
            for (int oy = 0; oy < oh; oy++) {
                for (int ox = 0; ox < ow; ox++)
                    for (int c = 0; c < bpp; c++) {
                        uint32_t sum = 0, n = 0;
                        for (int y = j[3] + oy * j[7]; y < j[3] + (oy + 1) * j[7] && y < j[5]; y++)
                            for (int x = j[2] + ox * j[6]; x < j[2] + (ox + 1) * j[6] && x < j[4]; x++) { sum += s[(size_t)y * spitch + x * bpp + c]; n++; }
                        CHECK(d[(size_t)oy * dpitch + ox * bpp + c] == (uint8_t)(((sum + n / 2u) * ((1u << 24) / n)) >> 24));
                    }
                for (int b = ow * bpp; b < dpitch; b++) CHECK(d[(size_t)oy * dpitch + b] == 0x5a);
            }
            free(s); free(d);
        }
    // refusals of the reduce plan
    {
        jda_output S, D;
        S.pixels = (void *)0x10000000; S.pitch_bytes = 64; S.width_px = 50; S.rows = 40;
        D.pixels = (void *)0x20000000; D.pitch_bytes = 32; D.width_px = 25; D.rows = 20;
        int32_t f[2] = { 2, 2 };
        CHECK(reducesim_check(1, &S, 1, f, NULL, &D, NULL) == JDA_SUCCESS);
        f[0] = 33;
        CHECK(reducesim_check(1, &S, 1, f, NULL, &D, NULL) == JDA_UNSUPPORTED_FEATURE);
        f[0] = 0;
        CHECK(reducesim_check(1, &S, 1, f, NULL, &D, NULL) == JDA_INVALID_PARAMETER);
        f[0] = 2; D.width_px = 24;
        CHECK(reducesim_check(1, &S, 1, f, NULL, &D, NULL) == JDA_INVALID_PARAMETER);
        D.width_px = 25;
        const int32_t bad[4] = { 0, 0, 51, 40 };
        CHECK(reducesim_check(1, &S, 1, f, bad, &D, NULL) == JDA_INVALID_PARAMETER);
        D.pixels = S.pixels;
        CHECK(reducesim_check(1, &S, 1, f, NULL, &D, NULL) == JDA_INVALID_PARAMETER);
        CHECK(reducesim_check(1, &S, 2, f, NULL, &D, NULL) == JDA_INVALID_PARAMETER && reducesim_check(0, &S, 1, f, NULL, &D, NULL) == JDA_INVALID_PARAMETER);
    }
    // float-box tables into exactly sized blocks, and the float-box checks
    for (int filter = 0; filter < 5; filter++) {
        const float boxes[][2] = { { 0.f, 333.f / 2 }, { 0.f, 217.f / 4 }, { 3.25f, 77.125f }, { 0.5f, 1.5f }, { 10.f, 40.f } };
        for (const auto &b : boxes)
            for (int out = 1; out <= 41; out += 8) {
                std::vector<int32_t> probe((size_t)out * (2 + JDA_RESIZE_MAX_KSIZE));
                const int ks = reducesim_taps_box(filter, 200, b[0], b[1], out, probe.data(), (int)probe.size());
                if (ks < 0) { CHECK(-ks == JDA_UNSUPPORTED_FEATURE); continue; }
                std::vector<int32_t> tab((size_t)out * (2 + ks));
                CHECK(reducesim_taps_box(filter, 200, b[0], b[1], out, tab.data(), (int)tab.size()) == ks);
                for (int i = 0; i < out; i++) CHECK(tab[2 * i] >= 0 && tab[2 * i + 1] >= 1 && tab[2 * i + 1] <= ks && tab[2 * i] + tab[2 * i + 1] <= 200);
            }
        jda_output S, D;
        S.pixels = (void *)0x10000000; S.pitch_bytes = 64; S.width_px = 50; S.rows = 40;
        D.pixels = (void *)0x20000000; D.pitch_bytes = 32; D.width_px = 25; D.rows = 20;
        float fb[4] = { 0.f, 0.f, 49.5f, 39.75f };
        CHECK(reducesim_resize_check_box(1, &S, 1, fb, &D, filter) == JDA_SUCCESS);
        fb[2] = 50.5f;
        CHECK(reducesim_resize_check_box(1, &S, 1, fb, &D, filter) == JDA_INVALID_PARAMETER);
        fb[2] = 0.f;
        CHECK(reducesim_resize_check_box(1, &S, 1, fb, &D, filter) == JDA_INVALID_PARAMETER);
        fb[2] = 20.f; fb[1] = -0.25f;
        CHECK(reducesim_resize_check_box(1, &S, 1, fb, &D, filter) == JDA_INVALID_PARAMETER);
        CHECK(reducesim_resize_check_box(1, &S, 1, NULL, &D, filter) == JDA_INVALID_PARAMETER);
    }
    // the thumbnail plan over a grid: every answer is a status the header names, and a plan that succeeds is consistent
    const double gaps[4] = { 0.0, 1.0, 2.0, 3.0 };
    for (int w = 1; w <= 2100; w = w < 40 ? w + 1 : w * 2 + 1)
        for (int h = 1; h <= 2100; h = h < 40 ? h + 1 : h * 2 + 1)
            for (int r = 1; r <= 300; r = r * 3 + 1)
                for (int g = 0; g < 4; g++)
                    for (int filter = 0; filter < 5; filter++) {
                        jda_thumbnail_steps T;
                        const int rc = reducesim_thumbnail_plan(w, h, r, r + 3, filter, gaps[g], &T);
                        CHECK(rc == JDA_SUCCESS || rc == JDA_UNSUPPORTED_FEATURE);
                        CHECK(T.out_w >= 1 && T.out_h >= 1 && T.out_w <= w && T.out_h <= h && T.fx >= 1 && T.fy >= 1);
                        CHECK(T.scale == 1 || T.scale == 2 || T.scale == 4 || T.scale == 8);
                        CHECK(T.reduce_box[0] >= 0 && T.reduce_box[1] >= 0 && T.reduce_box[2] <= T.draft_w && T.reduce_box[3] <= T.draft_h);
                        if (rc == JDA_SUCCESS && T.resize) CHECK(T.box[0] >= 0.f && T.box[0] < T.box[2] && T.box[2] <= (float)T.reduced_w && T.box[1] >= 0.f && T.box[1] < T.box[3] && T.box[3] <= (float)T.reduced_h);
                    }
    {
        jda_thumbnail_steps T;
        CHECK(reducesim_thumbnail_plan(100, 100, 10, 10, 0, 0.5, &T) == JDA_INVALID_PARAMETER && reducesim_thumbnail_plan(0, 100, 10, 10, 0, 2.0, &T) == JDA_INVALID_PARAMETER);
        CHECK(reducesim_thumbnail_plan(100, 100, 10, 0, 0, 2.0, &T) == JDA_INVALID_PARAMETER && reducesim_thumbnail_plan(100, 100, 10, 10, 5, 2.0, &T) == JDA_INVALID_PARAMETER);
        CHECK(reducesim_thumbnail_plan(16, 1700, 5, 50, 0, 0.0, &T) == JDA_UNSUPPORTED_FEATURE);        // more than 100 times as tall as wide
        CHECK(reducesim_thumbnail_plan(17, 1700, 5, 50, 0, 0.0, &T) == JDA_SUCCESS);                    // exactly 100 times: Pillow's usual order
        CHECK(reducesim_thumbnail_plan(100, 100, 10, 10, 0, 2.0, NULL) == JDA_INVALID_PARAMETER);
    }
    printf("thumb_asan ok\n");
    return 0;
}
