// tests/hostsim/orient_twin.h -- TEST INFRASTRUCTURE: the row-major twin of the orient kernel.
//
// The EXIF orientation as a table, destination pixel by destination pixel: dst(y', x') = src(y, x) with (y, x) read off the case list
// below (include/jpegdec_amd.h, jda_orient_surfaces).  Nothing of the kernel's formulation -- tiles, mirrors applied on the load side,
// blocks transposed in registers (jda_device_core.h) -- is used here, so that the two can be held against each other.
#ifndef JDA_ORIENT_TWIN_H
#define JDA_ORIENT_TWIN_H
#include <stdint.h>
#include <string.h>

// src: w x h pixels of bpp bytes at src_pitch; dst: the oriented rectangle (h x w pixels for 5-8) at dst_pitch; any o outside 2..8: a copy
static inline int orient_twin_rowmajor(const uint8_t *src, int src_pitch, int w, int h, int bpp, int o, uint8_t *dst, int dst_pitch)
{
    if (w <= 0 || h <= 0 || bpp <= 0) return -1;
    const int dw = (o >= 5 && o <= 8) ? h : w, dh = (o >= 5 && o <= 8) ? w : h;
    for (int yd = 0; yd < dh; yd++)
        for (int xd = 0; xd < dw; xd++) {
            int y = yd, x = xd;
            switch (o) {
            case 2: y = yd;         x = w - 1 - xd; break;
            case 3: y = h - 1 - yd; x = w - 1 - xd; break;
            case 4: y = h - 1 - yd; x = xd;         break;
            case 5: y = xd;         x = yd;         break;
            case 6: y = h - 1 - xd; x = yd;         break;
            case 7: y = h - 1 - xd; x = w - 1 - yd; break;
            case 8: y = xd;         x = w - 1 - yd; break;
            default: break;
            }
            memcpy(dst + (size_t)yd * dst_pitch + (size_t)xd * bpp, src + (size_t)y * src_pitch + (size_t)x * bpp, (size_t)bpp);
        }
    return 0;
}
#endif
