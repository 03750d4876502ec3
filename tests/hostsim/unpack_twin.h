// tests/hostsim/unpack_twin.h -- TEST INFRASTRUCTURE: jda_unpack_surfaces restated row by row, pixel by pixel.
//
// Knows nothing of vectors, tiles, lanes or aligned dwords: surface byte c (2 - c with JDA_PACK_BGR) of pixel (y, x) is element (y, x, c) of
// the dense HWC or CHW image -- the byte itself, or clamp(rint(x32 * scale[c] + bias[c]), 0, 255) with the product and the sum each rounded
// to float32 (volatile: no fused multiply-add, whatever the build) --, and the fourth byte of an RGB8888 pixel is 0xFF.  The checker of
// tests/hostsim/unpack_sim.cpp and of tests/test_unpack_cpu.py.
#ifndef JDA_UNPACK_TWIN_H
#define JDA_UNPACK_TWIN_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/jpegdec_amd.h"

static inline float unpack_twin_half(uint16_t h)
{
    const int e = (h >> 10) & 31, m = h & 0x3ff;
    float v;
    if (e == 31) v = m ? NAN : INFINITY;
    else if (e == 0) v = ldexpf((float)m, -24);
    else v = ldexpf((float)(m | 0x400), e - 25);
    return (h & 0x8000) ? -v : v;
}
static inline uint8_t unpack_twin_byte(float x, float s, float b)
{
    volatile float p = x * s;
    volatile float t = p + b;
    const float r = nearbyintf(t);
    if (!(r >= 0.f)) return 0;
    return r > 255.f ? 255 : (uint8_t)r;
}
// src: dense, w * h * channels elements; scale_bias: scale[0..C-1], bias[0..C-1] or NULL (255, 0); dst: the surface at pitch (bpp 4: R, G,
// B, 0xFF; bpp 1: gray).  0, or -1 for arguments the twin does not know.
static inline int unpack_twin_rowmajor(const void *src, int w, int h, int layout_flags, int elem_type, const float *scale_bias, uint8_t *dst, int pitch, int bpp)
{
    if ((bpp != 1 && bpp != 4) || w <= 0 || h <= 0 || elem_type < JDA_PACK_U8 || elem_type > JDA_PACK_F32) return -1;
    const int channels = bpp == 4 ? 3 : 1;
    const bool chw = (layout_flags & JDA_PACK_CHW) != 0, bgr = (layout_flags & JDA_PACK_BGR) != 0;
    if ((elem_type == JDA_PACK_U8 && scale_bias) || (bgr && channels == 1)) return -1;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            uint8_t *px = dst + (size_t)y * pitch + (size_t)x * bpp;
            for (int c = 0; c < channels; c++) {
                const size_t e = chw ? ((size_t)c * h + y) * w + x : ((size_t)y * w + x) * channels + c;
                uint8_t v;
                if (elem_type == JDA_PACK_U8) v = ((const uint8_t *)src)[e];
                else {
                    float f;
                    if (elem_type == JDA_PACK_F16) { uint16_t hb; memcpy(&hb, (const uint8_t *)src + 2 * e, 2); f = unpack_twin_half(hb); }
                    else memcpy(&f, (const uint8_t *)src + 4 * e, 4);
                    v = unpack_twin_byte(f, scale_bias ? scale_bias[c] : 255.f, scale_bias ? scale_bias[channels + c] : 0.f);
                }
                px[bgr ? 2 - c : c] = v;
            }
            if (bpp == 4) px[3] = 0xff;
        }
    return 0;
}

#endif
