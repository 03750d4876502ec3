// tests/hostsim/coef_twin.h -- TEST INFRASTRUCTURE: the row-major twin of jda_coef_tiles (jpegdec_amd/csrc/jda_kernels.hip).
//
// The same arithmetic -- jda_idct_col, jda_idct_row, jda_output_pixel of jda_device_core.h -- with none of the kernel's schedule: no
// tiles, no lanes, no work lists, no LDS.  MCU after MCU, block after block: the occupancy flags from a plain loop over the 63 AC
// coefficients (jpeg.inl:2207-2208), the DC-only bypass (:5146-5154) or the column pass over the occupied columns and the row pass
// of the block's class (:2555-2561, :2686-2688), then pixel after pixel.  tests/test_progressive_full_cpu.py holds the lane schedule
// (coef_sim.cpp) to it, and the class's CPU stand-in build (tests/class_cpu/stub_coef.cpp) draws its pixels with it.
#ifndef JDA_COEF_TWIN_H
#define JDA_COEF_TWIN_H

#include <stdint.h>
#include <string.h>

#include "../../jpegdec_amd/csrc/jda_device_core.h"

// the flags JPEGDecodeMCU forms while it stores a block's coefficients, from the coefficients themselves
static inline uint32_t coef_twin_flags(const int16_t *coef)
{
    uint32_t flags = 0;
    for (uint32_t n = 1; n < 64; n++) if (coef[n] != 0) flags |= (1u << (n & 7u)) | (n << 8);
    return flags & 0xffffu;
}

// one block: coefficients (natural order) + its prescaled quantisers -> 64 samples at slot[0..63]
static inline void coef_twin_block(const int16_t *coef, const int16_t *quant, uint8_t *slot)
{
    const uint32_t flags = coef_twin_flags(coef);
    if (flags == 0) {
        memset(slot, (int)jda_range_limit5((int32_t)coef[0] * (int32_t)quant[0]), 64);
        return;
    }
    int16_t w[64];
    memcpy(w, coef, 128);
    const uint32_t colmask = (flags & 0xffu) | 1u;
    const bool half = (flags & 0x2000u) == 0;
    for (uint32_t col = 0; col < 8; col++) {
        if (!((colmask >> col) & 1u)) continue;
        int32_t cv[8], qv[8], r[8];
        for (int row = 0; row < 8; row++) {
            if (half && row >= 4) { cv[row] = 0; qv[row] = 0; }
            else { cv[row] = w[row * 8 + col]; qv[row] = quant[row * 8 + col]; }
        }
        if (half) jda_idct_col<false, true>(cv, qv, r); else jda_idct_col<false, false>(cv, qv, r);
        for (int row = 0; row < 8; row++) w[row * 8 + col] = (int16_t)r[row];
    }
    const int cls = (flags & 0xf0u) ? 2 : ((flags & 0xfcu) ? 1 : 0);
    for (int row = 0; row < 8; row++) {
        int32_t sv[8];
        for (int k = 0; k < 8; k++) sv[k] = (k < 4 || cls == 2) ? w[row * 8 + k] : 0;
        const jda_row8 p = cls == 2 ? jda_idct_row<2>(sv) : (cls == 1 ? jda_idct_row<1>(sv) : jda_idct_row<0>(sv));
        memcpy(slot + row * 8, &p.lo, 4);
        memcpy(slot + row * 8 + 4, &p.hi, 4);
    }
}

// a whole image.  pixel_type: as the descriptor holds it (LUMA_ONLY folded, a gray file's RGB8888 turned into RGB565 big endian);
// out: width_px x rows of the MCU-padded canvas are written (the clip of jda_output)
template <int MODE>
static inline void coef_twin_image(uint32_t mcus_x, uint32_t mcus_y, const uint8_t q_id[3], const int16_t *quant, const int16_t *coefs, int pixel_type,
                                   uint8_t *out, uint32_t pitch, uint32_t width_px, uint32_t rows)
{
    typedef jda_mode_traits<MODE> T;
    const bool luma_only = MODE != JDA_MODE_GRAY && pixel_type == JDA_EIGHT_BIT_GRAYSCALE;
    uint8_t planes[T::NBLK * JDA_COEF_STRIDE];
    for (uint32_t my = 0; my < mcus_y; my++)
        for (uint32_t mx = 0; mx < mcus_x; mx++) {
            memset(planes, 0, sizeof(planes));
            for (uint32_t b = 0; b < (uint32_t)T::NBLK; b++) {
                const uint32_t c = b < (uint32_t)T::NLUMA ? 0u : b - T::NLUMA + 1u;
                if (luma_only && c) continue;
                coef_twin_block(coefs + ((size_t)(my * mcus_x + mx) * T::NBLK + b) * 64, quant + 64 * (q_id[c] & 3), planes + b * JDA_COEF_STRIDE);
            }
            for (uint32_t py = 0; py < (uint32_t)T::MCU_H; py++)
                for (uint32_t px = 0; px < (uint32_t)T::MCU_W; px++) {
                    const uint32_t X = mx * T::MCU_W + px, Y = my * T::MCU_H + py;
                    if (X >= width_px || Y >= rows) continue;
                    const uint32_t v = jda_output_pixel<MODE>(planes, px, py, 0, pixel_type);
                    uint8_t *row = out + (size_t)Y * pitch;
                    if (pixel_type == JDA_RGB8888) memcpy(row + 4 * X, &v, 4);
                    else if (pixel_type == JDA_EIGHT_BIT_GRAYSCALE) row[X] = (uint8_t)v;
                    else { const uint16_t h = (uint16_t)v; memcpy(row + 2 * X, &h, 2); }
                }
        }
}

static inline int coef_twin_decode(int mode, uint32_t mcus_x, uint32_t mcus_y, const uint8_t q_id[3], const int16_t *quant, const int16_t *coefs, int pixel_type,
                                   uint8_t *out, uint32_t pitch, uint32_t width_px, uint32_t rows)
{
    switch (mode) {
    case JDA_MODE_GRAY: coef_twin_image<JDA_MODE_GRAY>(mcus_x, mcus_y, q_id, quant, coefs, pixel_type, out, pitch, width_px, rows); return 0;
    case JDA_MODE_444: coef_twin_image<JDA_MODE_444>(mcus_x, mcus_y, q_id, quant, coefs, pixel_type, out, pitch, width_px, rows); return 0;
    case JDA_MODE_420: coef_twin_image<JDA_MODE_420>(mcus_x, mcus_y, q_id, quant, coefs, pixel_type, out, pitch, width_px, rows); return 0;
    case JDA_MODE_422: coef_twin_image<JDA_MODE_422>(mcus_x, mcus_y, q_id, quant, coefs, pixel_type, out, pitch, width_px, rows); return 0;
    case JDA_MODE_440: coef_twin_image<JDA_MODE_440>(mcus_x, mcus_y, q_id, quant, coefs, pixel_type, out, pitch, width_px, rows); return 0;
    default: return -1;
    }
}

#endif
