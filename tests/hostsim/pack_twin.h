// tests/hostsim/pack_twin.h -- TEST INFRASTRUCTURE: jda_pack_surfaces restated row by row, pixel by pixel.
//
// Knows nothing of runs, vectors, tiles or lanes: destination element (y, x, c) of a dense HWC or CHW image is source byte c (2 - c with
// JDA_PACK_BGR) of pixel (ry + y, rx + x), or table[c][that byte].  The checker of tests/hostsim/pack_sim.cpp and of tests/test_pack_cpu.py.
#ifndef JDA_PACK_TWIN_H
#define JDA_PACK_TWIN_H

#include <stdint.h>
#include <string.h>

#include "../../include/jpegdec_amd.h"

// src: the surface (bpp 4: R, G, B, A; bpp 1: gray) at pitch; {rx, ry, w, h}: the rectangle; table: channels * 256 elements of the
// destination type (NULL with JDA_PACK_U8); dst: dense.  0, or -1 for arguments the twin does not know.
static inline int pack_twin_rowmajor(const uint8_t *src, int pitch, int bpp, int rx, int ry, int w, int h, int layout_flags, int elem_type,
                                     const void *table, void *dst)
{
    if ((bpp != 1 && bpp != 4) || w <= 0 || h <= 0 || elem_type < JDA_PACK_U8 || elem_type > JDA_PACK_F32) return -1;
    const int channels = bpp == 4 ? 3 : 1, es = elem_type == JDA_PACK_U8 ? 1 : elem_type == JDA_PACK_F16 ? 2 : 4;
    const bool chw = (layout_flags & JDA_PACK_CHW) != 0, bgr = (layout_flags & JDA_PACK_BGR) != 0;
    if ((es == 1) != (table == NULL) || (bgr && channels == 1)) return -1;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < channels; c++) {
                const uint8_t v = src[(size_t)(ry + y) * pitch + (size_t)(rx + x) * bpp + (bgr ? 2 - c : c)];
                const size_t e = chw ? ((size_t)c * h + y) * w + x : ((size_t)y * w + x) * channels + c;
                if (es == 1) ((uint8_t *)dst)[e] = v;
                else memcpy((uint8_t *)dst + e * es, (const uint8_t *)table + ((size_t)c * 256 + v) * es, (size_t)es);
            }
    return 0;
}

#endif
