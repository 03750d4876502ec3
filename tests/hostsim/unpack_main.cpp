// tests/hostsim/unpack_main.cpp -- TEST INFRASTRUCTURE: the plan and the lanes of jda_unpack_surfaces (unpack_sim.cpp) as a program of
// their own, built with AddressSanitizer + UBSan (make unpackasan): a reduced grid of sizes, source offsets, pitches, formats and element
// types, sources and surfaces in heap blocks of exactly their size -- a load or store one byte outside is the sanitizer's to find -- each
// result held against the row-major twin, and the refusals of the plan.  Prints "unpack_asan ok".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int unpacksim_rowmajor(const void *src, int w, int h, int layout_flags, int elem_type, const float *scale_bias, uint8_t *dst, int pitch, int bpp);
extern "C" int unpacksim_lanes(const void *src, int w, int h, int layout_flags, int elem_type, const float *scale_bias, uint8_t *dst, int pitch, int bpp);
extern "C" int unpacksim_check(int n, const void *const *src, int layout_flags, int elem_type, const float *scale_bias, const jda_output *dst, int bpp, uint32_t *n_tiles);

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int fail(const char *what, int a, int b, int c, int d)
{
    fprintf(stderr, "unpack_asan: %s (%d %d %d %d)\n", what, a, b, c, d);
    return 1;
}

int main()
{
    static const int widths[] = { 1, 3, 4, 5, 16, 17, 65 }, heights[] = { 1, 2, 9 }, offsets[] = { 0, 1, 3 };
    static const int formats[][2] = { { 4, JDA_PACK_HWC }, { 4, JDA_PACK_CHW }, { 4, JDA_PACK_HWC | JDA_PACK_BGR }, { 4, JDA_PACK_CHW | JDA_PACK_BGR }, { 1, JDA_PACK_CHW } };
    static const float params[6] = { 255.f, -3.5f, 1.f, 0.f, 300.f, 0.25f };
    int runs = 0;
    for (const auto &f : formats)
        for (int elem = JDA_PACK_U8; elem <= JDA_PACK_F32; elem++)
            for (int w : widths)
                for (int h : heights)
                    for (int off : offsets) {
                        const int bpp = f[0], flags = f[1], channels = bpp == 4 ? 3 : 1, es = 1 << elem;
                        const size_t nbytes = (size_t)w * h * channels * es;
                        // the dense image `off` elements behind an aligned dword, in a block that ends where the image's last dword does
                        const size_t lead = (size_t)off * es, block = (lead + nbytes + 3) & ~(size_t)3;
                        uint8_t *sblock = (uint8_t *)malloc(block);                                 // (malloc's blocks are 16-byte aligned)
                        uint8_t *src = sblock + lead;
                        for (size_t i = 0; i < nbytes; i++) src[i] = (uint8_t)rnd();
                        const int pitch = ((w * bpp + 15) & ~15) + 16 * (runs & 1);
                        const size_t sbytes = (size_t)pitch * (h - 1) + (size_t)w * bpp;      // (the last row's padding is not there)
                        uint8_t *got = (uint8_t *)malloc(sbytes), *want = (uint8_t *)malloc(sbytes);
                        memset(got, 0xA5, sbytes); memset(want, 0xA5, sbytes);
                        const float gray_params[2] = { params[1], params[4] };
                        const float *sb = elem == JDA_PACK_U8 || (runs % 3) == 0 ? NULL : bpp == 4 ? params : gray_params;
                        const int rc = unpacksim_lanes(src, w, h, flags, elem, sb, got, pitch, bpp);
                        if (rc != 0) return fail("the schedule broke a promise", rc, w, h, elem);
                        if (unpacksim_rowmajor(src, w, h, flags, elem, sb, want, pitch, bpp) != 0) return fail("twin", w, h, flags, elem);
                        if (memcmp(got, want, sbytes) != 0) return fail("differs from the twin", w, h, flags, elem);
                        free(sblock); free(got); free(want);
                        runs++;
                    }
    // refusals of the plan
    uint8_t *a = (uint8_t *)aligned_alloc(16, 4096), *b = (uint8_t *)aligned_alloc(16, 4096);
    const void *srcs[1] = { a + 1 };
    jda_output D = { b, 64, 10, 20 };
    uint32_t tiles = 0;
    if (unpacksim_check(1, srcs, JDA_PACK_HWC, JDA_PACK_U8, NULL, &D, 4, &tiles) != JDA_SUCCESS || tiles != 1u) return fail("a good call", (int)tiles, 0, 0, 0);
    const float bad[6] = { 1.f, INFINITY, 1.f, 0.f, 0.f, 0.f };
    if (unpacksim_check(1, srcs, JDA_PACK_HWC, JDA_PACK_F32, bad, &D, 4, NULL) != JDA_INVALID_PARAMETER) return fail("infinite scale", 0, 0, 0, 0);
    if (unpacksim_check(1, srcs, JDA_PACK_HWC, JDA_PACK_F16, NULL, &D, 4, NULL) != JDA_INVALID_PARAMETER) return fail("misaligned F16", 0, 0, 0, 0);
    if (unpacksim_check(1, srcs, JDA_PACK_BGR, JDA_PACK_U8, NULL, &D, 1, NULL) != JDA_INVALID_PARAMETER) return fail("BGR gray", 0, 0, 0, 0);
    srcs[0] = b + 100;
    if (unpacksim_check(1, srcs, JDA_PACK_HWC, JDA_PACK_U8, NULL, &D, 4, NULL) != JDA_INVALID_PARAMETER) return fail("overlap", 0, 0, 0, 0);
    free(a); free(b);
    printf("unpack_asan ok: %d jobs\n", runs);
    return 0;
}
