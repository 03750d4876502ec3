// tests/hostsim/dither_twin.h -- TEST INFRASTRUCTURE: the row-major twin of the dither kernel.
//
// The 4 / 2 / 1-bpp error diffusion of the reference (JPEGDither, jpeg.inl:4871-4940) restated the way the reference runs it: strip by
// strip, row by row, pixel by pixel, over ONE byte row of errors that lives as long as the image and a strip buffer that is packed in
// place.  Nothing of the kernel's formulation (jda_dither_step: the error a row hands down as a sum, lanes = rows) is used here, so
// that the two can be held against each other -- and both against what the unmodified reference recorded (tests/golden/dither).
#ifndef JDA_DITHER_TWIN_H
#define JDA_DITHER_TWIN_H
#include <stdint.h>
#include <string.h>

#include <vector>

// seed: the JDA_DITHER_SEED_BYTES the error row holds before the first strip (NULL: zeros)
// gray: w x h bytes at gray_pitch; out: h rows of (w * bits + 7) / 8 bytes at out_pitch; strip_rows: rows dithered at a time
static inline int dither_twin_rowmajor(const uint8_t *gray, int gray_pitch, int w, int h, int strip_rows, int bits, const uint8_t *seed, uint8_t *out, int out_pitch)
{
    if (w <= 0 || h <= 0 || strip_rows <= 0 || (bits != 4 && bits != 2 && bits != 1)) return -1;
    const int per_byte = 8 / bits, dpitch = (w * bits + 7) / 8;
    const int keep = 0xff & ~(0xff >> bits);                 // the bits of a pixel that are output
    std::vector<uint8_t> err((size_t)w + 2 > 2184 ? (size_t)w + 2 : 2184, 0);       // never cleared as a whole
    if (seed) memcpy(err.data(), seed, 2184);                // what the header parse left in the buffer the row lies in
    std::vector<uint8_t> buf((size_t)w * strip_rows);
    for (int y0 = 0; y0 < h; y0 += strip_rows) {
        const int rows = y0 + strip_rows <= h ? strip_rows : h - y0;
        for (int r = 0; r < rows; r++) memcpy(&buf[(size_t)r * w], gray + (size_t)(y0 + r) * gray_pitch, (size_t)w);
        err[0] = err[1] = err[2] = 0;                        // all that a new strip clears
        for (int r = 0; r < rows; r++) {
            const uint8_t *src = &buf[(size_t)r * w];
            uint8_t *dst = &buf[(size_t)r * dpitch];         // in place: the packed rows trail the gray ones
            int carry = 0, pack = 0;
            for (int x = 0; x < w; x++) {
                int v = src[x] + carry;
                if (v > 255) v = 255;
                pack = ((pack << bits) | (v >> (8 - bits))) & 0xff;
                if (x % per_byte == per_byte - 1) { *dst++ = (uint8_t)pack; pack = 0; }      // (an unfinished last byte is never stored)
                const int half = (v - (v & keep)) >> 1;
                const int right = (7 * half) >> 3, below_right = half - right, below = (5 * half) >> 3, below_left = half - below;
                carry = right + err[x + 2];
                err[x + 2] = (uint8_t)below_right;
                err[x + 1] = (uint8_t)(err[x + 1] + below);
                err[x] = (uint8_t)(err[x] + below_left);
            }
        }
        for (int r = 0; r < rows; r++) memcpy(out + (size_t)(y0 + r) * out_pitch, &buf[(size_t)r * dpitch], (size_t)dpitch);
    }
    return 0;
}
#endif
