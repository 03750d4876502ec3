// tests/hostsim/resize_twin.h -- TEST INFRASTRUCTURE: jda_resize_surfaces restated row by row, pixel by pixel.
//
// Knows nothing of tables in device memory, tiles, lanes or LDS: Pillow's Image.resize(BILINEAR, box) -- per axis the triangle filter's
// taps in double, normalised and rounded to 22-bit fixed point; a horizontal pass over the source rows the vertical taps read, into an
// 8-bit intermediate image; a vertical pass over that.  The checker of tests/hostsim/resize_sim.cpp and of tests/test_resize_cpu.py
// (build with -ffp-contract=off).
#ifndef JDA_RESIZE_TWIN_H
#define JDA_RESIZE_TWIN_H

#include <math.h>
#include <stdint.h>

#include <vector>

struct resize_twin_axis {
    int ksize;
    std::vector<int> min, cnt, k;      // k[i * ksize + x]
};

static inline void resize_twin_taps(int in_size, int in0, int in1, int out_size, resize_twin_axis *A)
{
    const double scale = (double)(in1 - in0) / out_size, fs = scale < 1.0 ? 1.0 : scale, support = fs;
    A->ksize = (int)ceil(support) * 2 + 1;
    A->min.assign((size_t)out_size, 0); A->cnt.assign((size_t)out_size, 0); A->k.assign((size_t)out_size * A->ksize, 0);
    std::vector<double> w((size_t)A->ksize);
    for (int xx = 0; xx < out_size; xx++) {
        const double center = in0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5), xmax = (int)(center + support + 0.5);
        if (xmin < 0) xmin = 0;
        if (xmax > in_size) xmax = in_size;
        double ww = 0.0;
        for (int x = 0; x < xmax - xmin; x++) {
            const double a = fabs((x + xmin - center + 0.5) * (1.0 / fs));
            w[(size_t)x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[(size_t)x];
        }
        for (int x = 0; x < xmax - xmin; x++) A->k[(size_t)xx * A->ksize + x] = (int)(0.5 + (ww != 0.0 ? w[(size_t)x] / ww : w[(size_t)x]) * 4194304.0);
        A->min[(size_t)xx] = xmin; A->cnt[(size_t)xx] = xmax - xmin;
    }
}

static inline uint8_t resize_twin_clip(int64_t acc)
{
    const int64_t v = (acc + (1 << 21)) >> 22;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// src: width x rows pixels of bpp bytes at pitch; {x, y, w, h}: the box; dst: out_w x out_h pixels at dst_pitch.  0, or -1 for arguments
// the twin does not know.
static inline int resize_twin_rowmajor(const uint8_t *src, int pitch, int width, int rows, int bpp, int x, int y, int w, int h,
                                       uint8_t *dst, int dst_pitch, int out_w, int out_h)
{
    if ((bpp != 1 && bpp != 4) || w <= 0 || h <= 0 || out_w <= 0 || out_h <= 0 || x < 0 || y < 0 || x + w > width || y + h > rows) return -1;
    resize_twin_axis H, V;
    resize_twin_taps(width, x, x + w, out_w, &H);
    resize_twin_taps(rows, y, y + h, out_h, &V);
    const int r0 = V.min[0], r1 = V.min[(size_t)out_h - 1] + V.cnt[(size_t)out_h - 1];
    std::vector<uint8_t> tmp((size_t)(r1 - r0) * out_w * bpp);
    for (int r = r0; r < r1; r++)
        for (int xx = 0; xx < out_w; xx++)
            for (int c = 0; c < bpp; c++) {
                int64_t acc = 0;
                for (int t = 0; t < H.cnt[(size_t)xx]; t++) acc += (int64_t)src[(size_t)r * pitch + (size_t)(H.min[(size_t)xx] + t) * bpp + c] * H.k[(size_t)xx * H.ksize + t];
                tmp[((size_t)(r - r0) * out_w + xx) * bpp + c] = resize_twin_clip(acc);
            }
    for (int yy = 0; yy < out_h; yy++)
        for (int xx = 0; xx < out_w; xx++)
            for (int c = 0; c < bpp; c++) {
                int64_t acc = 0;
                for (int t = 0; t < V.cnt[(size_t)yy]; t++) acc += (int64_t)tmp[((size_t)(V.min[(size_t)yy] + t - r0) * out_w + xx) * bpp + c] * V.k[(size_t)yy * V.ksize + t];
                dst[(size_t)yy * dst_pitch + (size_t)xx * bpp + c] = resize_twin_clip(acc);
            }
    return 0;
}

#endif
