// tests/hostsim/resize_filters_main.cpp -- TEST INFRASTRUCTURE: the resize plan and the lane simulator for Pillow's filters
// (resize_filters_sim.cpp) as a program of its own, built under AddressSanitizer + UBSan (make resizefiltersasan): nothing is loaded into an
// interpreter.  It runs the plan and the lane schedule of an unsigned filter (HAMMING) and of the two signed ones (BICUBIC, LANCZOS) for both
// pixel sizes over exactly sized heap blocks -- a crop inside a picture, an upscale wider than a tile, a downscale taller than one, the job
// at each filter's tap cap --, the guard on tables of its own, and the refusals.  Exit status 0 and "resize_filters_asan ok" when every call
// answers as it must.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int resizefsim_taps(int filter, int in_size, int in0, int in1, int out_size, int32_t *out, int cap);
extern "C" int resizefsim_guard(int filter, const int32_t *tab, int out_size, int ksize);
extern "C" int resizefsim_lanes(int filter, const uint8_t *src, int pitch, int width_px, int rows, int bpp, int x, int y, int w, int h, uint8_t *dst,
                                int dst_pitch, int out_w, int out_h, uint32_t *info);
extern "C" int resizefsim_check(int filter, int n, const jda_output *src, int bpp, const int32_t *rects, const jda_output *dst, const void *tables_at, uint32_t *info);

#define CHECK(c) do { if (!(c)) { printf("resize_filters_asan: line %d: %s\n", __LINE__, #c); fflush(stdout); return 1; } } while (0)

int main()
{
    uint32_t seed = 4711u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
    const int filters[3] = { JDA_RESIZE_HAMMING, JDA_RESIZE_BICUBIC, JDA_RESIZE_LANCZOS };
    const int cap_rows[3] = { 6, 12, 18 }, beyond_rows[3] = { 486, 481, 481 };
    const uint32_t cap_th[3] = { 1, 1, 2 };        // (161 source rows an output row; LANCZOS' rows lie 26.7 apart: two of them read 188 <= 192, the LDS budget)
    for (int fi = 0; fi < 3; fi++) {
        const int f = filters[fi];
        // {w, h, x, y, bw, bh, ow, oh}
        const int jobs[][8] = { { 70, 45, 9, 6, 50, 31, 33, 21 }, { 31, 9, 0, 0, 31, 9, 301, 35 }, { 70, 300, 0, 0, 70, 300, 67, 37 }, { 1, 1, 0, 0, 1, 1, 5, 3 },
                                { 33, 480, 0, 0, 33, 480, 17, cap_rows[fi] } };
        for (const auto &j : jobs)
            for (int bpp = 1; bpp <= 4; bpp += 3) {
                const int spitch = (j[0] * bpp + 15) & ~15, dpitch = (j[6] * bpp + 15) & ~15;
                uint8_t *s = (uint8_t *)aligned_alloc(16, (size_t)spitch * j[1]), *d = (uint8_t *)aligned_alloc(16, (size_t)dpitch * j[7]);      // exactly the surfaces
                CHECK(s && d);
                for (size_t i = 0; i < (size_t)spitch * j[1]; i++) s[i] = (uint8_t)((rnd() & 1u) ? 255u : (rnd() & 2u) ? 0u : rnd());              // many 0 / 255: both clips
                memset(d, 0x5a, (size_t)dpitch * j[7]);
                uint32_t info[6];
                CHECK(resizefsim_lanes(f, s, spitch, j[0], j[1], bpp, j[2], j[3], j[4], j[5], d, dpitch, j[6], j[7], info) == 0);
                CHECK(info[5] == (f == JDA_RESIZE_HAMMING ? 0u : 1u));
                if (j[1] == 480) CHECK(info[1] == cap_th[fi] && info[4] == (uint32_t)JDA_RESIZE_MAX_KSIZE && info[0] == (uint32_t)cap_rows[fi] / cap_th[fi]);
                for (int r = 0; r < j[7]; r++)
                    for (int b = j[6] * bpp; b < dpitch; b++) CHECK(d[(size_t)r * dpitch + b] == 0x5a);
                free(s); free(d);
            }
        // one step beyond the cap, on each axis: refused by the plan
        jda_output S, D;
        S.pixels = (void *)0x10000000; S.pitch_bytes = 48; S.width_px = 33; S.rows = beyond_rows[fi];
        D.pixels = (void *)0x20000000; D.pitch_bytes = 32; D.width_px = 17; D.rows = cap_rows[fi];
        CHECK(resizefsim_check(f, 1, &S, 1, NULL, &D, NULL, NULL) == JDA_UNSUPPORTED_FEATURE);
        S.pitch_bytes = 496; S.width_px = beyond_rows[fi]; S.rows = 33; D.width_px = cap_rows[fi]; D.rows = 17;
        CHECK(resizefsim_check(f, 1, &S, 1, NULL, &D, NULL, NULL) == JDA_UNSUPPORTED_FEATURE);
        S.width_px = 480;
        CHECK(resizefsim_check(f, 1, &S, 1, NULL, &D, NULL, NULL) == JDA_SUCCESS);
        CHECK(resizefsim_check(5, 1, &S, 1, NULL, &D, NULL, NULL) == JDA_INVALID_PARAMETER && resizefsim_check(-1, 1, &S, 1, NULL, &D, NULL, NULL) == JDA_INVALID_PARAMETER);
        // the host's table into an exactly sized block, then the guard on tables made by hand
        std::vector<int32_t> tab((size_t)224 * (2 + 15));
        const int ks = resizefsim_taps(f, 500, 0, 500, 224, tab.data(), (int)tab.size());
        CHECK(ks == (f == JDA_RESIZE_HAMMING ? 7 : f == JDA_RESIZE_BICUBIC ? 11 : 15));
    }
    int32_t t[2 + 3] = { 0, 3, 1 << 22, 0, 0 };
    CHECK(resizefsim_guard(JDA_RESIZE_LANCZOS, t, 1, 3) == JDA_SUCCESS && resizefsim_guard(JDA_RESIZE_BOX, t, 1, 3) == JDA_SUCCESS);
    t[3] = -1;
    CHECK(resizefsim_guard(JDA_RESIZE_BICUBIC, t, 1, 3) == JDA_SUCCESS && resizefsim_guard(JDA_RESIZE_HAMMING, t, 1, 3) == JDA_UNSUPPORTED_FEATURE);
    t[2] = 1 << 23;
    CHECK(resizefsim_guard(JDA_RESIZE_BICUBIC, t, 1, 3) == JDA_UNSUPPORTED_FEATURE);
    t[2] = (1 << 23) - 1; t[3] = (1 << 23) - 1; t[4] = 1 << 20;
    CHECK(resizefsim_guard(JDA_RESIZE_LANCZOS, t, 1, 3) == JDA_UNSUPPORTED_FEATURE);        // 255 * the positive taps leave 31 bits
    t[2] = -(1 << 23) + 1; t[3] = -(1 << 23) + 1; t[4] = -(1 << 20);
    CHECK(resizefsim_guard(JDA_RESIZE_LANCZOS, t, 1, 3) == JDA_UNSUPPORTED_FEATURE);
    printf("resize_filters_asan ok\n");
    return 0;
}
