// tests/hostsim/dither_sim.cpp -- TEST INFRASTRUCTURE: the dither kernel's lane schedule on the CPU.
//
// dithersim_skewed steps jda_dither_rows (jpegdec_amd/csrc/jda_kernels.hip) the way the GPU runs it -- 64-row groups dealt round robin
// to `waves` wavefronts, lane r of a group two pixels behind lane r - 1, the value handed down taken from the lane above as it stood
// after the step before, the last lane's values through the wavefront's hand-over row -- with the kernel's own per-pixel step, tail
// rule and dword packing (jda_device_core.h).  The groups run one after the other: the kernel's waits make exactly that order of
// values, whatever the timing.  dithersim_rowmajor is the twin that knows none of this (dither_twin.h).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_device_core.h"
#include "dither_twin.h"

extern "C" int dithersim_rowmajor(const uint8_t *gray, int gray_pitch, int w, int h, int strip_rows, int pixel_type, const uint8_t *seed, uint8_t *out, int out_pitch)
{
    return dither_twin_rowmajor(gray, gray_pitch, w, h, strip_rows, (int)jda_dither_bits(pixel_type), seed, out, out_pitch);
}

extern "C" int dithersim_skewed(const uint8_t *gray, int gray_pitch, int w, int h, int strip_rows, int pixel_type, const uint8_t *seed, uint8_t *out, int out_pitch, int waves)
{
    const uint32_t bits = jda_dither_bits(pixel_type), W = (uint32_t)w, H = (uint32_t)h, strip = (uint32_t)strip_rows;
    if (!bits || w <= 0 || h <= 0 || strip_rows <= 0 || waves < 1 || waves > JDA_DITHER_MAX_WAVES) return -1;
    const uint32_t dpitch = jda_dither_pitch(W, bits), tail_bits = (W * bits) & 31u, ppd = 32u / bits;
    if ((uint32_t)out_pitch < dpitch) return -1;
    std::vector<std::vector<uint8_t>> hand((size_t)waves, std::vector<uint8_t>((size_t)W + 16, 0xEE));     // (LDS is not zero either)
    const uint32_t n_groups = (H + 63u) / 64u;
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t wave = g % (uint32_t)waves, prod = (wave + (uint32_t)waves - 1u) % (uint32_t)waves, row0 = g * 64u;
        const bool has_prod = g > 0;
        // a wavefront with one hand-over row (waves == 1) reads it while it writes it, 127 steps apart: the copy the reader sees
        // is the live row, as in LDS
        std::vector<uint8_t> &hand_mine = hand[wave];
        const std::vector<uint8_t> &hand_prod = hand[prod];
        jda_dither_lane L[64];
        uint32_t handed[64], acc[64], curw[64], pend_word[64], pend_at[64];
        bool pend[64];
        jda_dither_feed F[64];
        auto load_chunk = [&](uint32_t row, int32_t c, uint32_t *dst) {      // an aligned 16-byte load of the row (what lies behind the row's last pixel is never used)
            uint8_t b[16] = { 0 };
            if (row < H && c >= 0 && (uint32_t)c * 16u < W) memcpy(b, gray + (size_t)row * gray_pitch + (size_t)c * 16u, W - (uint32_t)c * 16u < 16u ? W - (uint32_t)c * 16u : 16u);
            memcpy(dst, b, 16);
        };
        for (int r = 0; r < 64; r++) {
            L[r].fwd = L[r].a = L[r].b = 0; handed[r] = 0; acc[r] = 0; curw[r] = 0; pend[r] = false;
            memset(&F[r], 0, sizeof(F[r]));
            if (-(int32_t)((JDA_DITHER_LAG * (uint32_t)r) >> 4) == 0) load_chunk(row0 + (uint32_t)r, 0, F[r].n);
        }
        const uint32_t steps = W + 2u * 63u + 1u;
        for (uint32_t t = 0; t < steps; t++) {
            uint32_t before[64];
            memcpy(before, handed, sizeof(before));          // every lane reads its neighbour as the step began
            for (uint32_t lane = 0; lane < 64; lane++) {
                const int32_t x = (int32_t)t - (int32_t)(JDA_DITHER_LAG * lane);
                const uint32_t row = row0 + lane;
                const bool row_ok = row < H, in_row = x >= 0 && (uint32_t)x < W, live = row_ok && in_row;
                uint8_t *orow = out + (size_t)(row_ok ? row : 0u) * out_pitch;
                const uint32_t phase = (JDA_DITHER_LAG * lane) & 15u;
                const int32_t chunk0 = -(int32_t)((JDA_DITHER_LAG * lane) >> 4);
                if ((t & 7u) == 0) {                         // the kernel's wave-uniform memory steps
                    if ((t & 15u) == 0) {
                        jda_dither_feed_turn(F[lane], phase);
                        load_chunk(row, chunk0 + (int32_t)(t >> 4) + 1, F[lane].n);
                    }
                    if (pend[lane]) { memcpy(orow + pend_at[lane], &pend_word[lane], 4); pend[lane] = false; }
                }
                if ((t & 3u) == 0) { curw[lane] = F[lane].w[0]; F[lane].w[0] = F[lane].w[1]; F[lane].w[1] = F[lane].w[2]; F[lane].w[2] = F[lane].w[3]; }
                const uint32_t gpx = curw[lane] & 0xffu;
                curw[lane] >>= 8;
                uint32_t down = lane ? before[lane - 1] : 0u;
                if (lane == 0) {
                    down = (has_prod && in_row) ? (uint32_t)hand_prod[(size_t)x] : 0u;
                    if (!has_prod && seed && in_row && (uint32_t)x + 1u < JDA_DITHER_SEED_BYTES) down = seed[x + 1];
                }
                if (x == 1 && row % strip == 0) down = 0;
                uint32_t px;
                handed[lane] = jda_dither_step(L[lane], live, x, gpx, down, bits, px);
                if (lane == 63u && x >= 1 && (uint32_t)x <= W) hand_mine[(size_t)x - 1] = (uint8_t)handed[lane];
                if (!live) continue;
                acc[lane] = (acc[lane] << bits) | px;
                const uint32_t done = (uint32_t)x + 1u;
                if (done % ppd == 0) {
                    pend_word[lane] = __builtin_bswap32(acc[lane]); pend_at[lane] = (done / ppd - 1u) * 4u; pend[lane] = true;
                } else if (done == W) {
                    uint8_t *tp = orow + (size_t)(W / ppd) * 4u;
                    const uint32_t whole = tail_bits >> 3;
                    for (uint32_t k = 0; k < whole; k++) tp[k] = (uint8_t)(acc[lane] >> (tail_bits - 8u * (k + 1u)));
                    if (tail_bits & 7u) {
                        uint32_t sr, sc;
                        jda_dither_stale_src(row % strip, W, dpitch, sr, sc);
                        const uint32_t srow = row - row % strip + sr;
                        tp[whole] = srow < H ? gray[(size_t)srow * gray_pitch + sc] : (uint8_t)0;
                    }
                }
            }
        }
        for (uint32_t lane = 0; lane < 64; lane++)
            if (pend[lane]) memcpy(out + (size_t)(row0 + lane) * out_pitch + pend_at[lane], &pend_word[lane], 4);
    }
    return 0;
}
