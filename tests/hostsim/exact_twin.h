// tests/hostsim/exact_twin.h -- TEST INFRASTRUCTURE: the libjpeg-exact decode written row-major in plain C++, the way
// libjpeg's own files read (jidctint.c, jdsample.c, jdcolor.c), sharing no code with the kernels' per-lane functions.  tests/test_exact_cpu.py
// holds it to the numpy twin (tests/exact_util.py), and tests/hostsim/exact_sim.cpp holds the kernels' lanes to it.
#ifndef EXACT_TWIN_H
#define EXACT_TWIN_H

#include <stdint.h>
#include <string.h>

#include <vector>

namespace exact_twin {

inline int32_t descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }
// one pass of jpeg_idct_islow over in[0], in[stride], ..; 32-bit integers that wrap
inline void pass(const int32_t *in, int stride, int32_t *out, int ostride, int shift)
{
    const uint32_t d0 = (uint32_t)in[0], d1 = (uint32_t)in[stride], d2 = (uint32_t)in[2 * stride], d3 = (uint32_t)in[3 * stride], d4 = (uint32_t)in[4 * stride],
                   d5 = (uint32_t)in[5 * stride], d6 = (uint32_t)in[6 * stride], d7 = (uint32_t)in[7 * stride];
    uint32_t z1 = (d2 + d6) * 4433u;
    const uint32_t tmp2 = z1 - d6 * 15137u, tmp3 = z1 + d2 * 6270u;
    const uint32_t tmp0 = (d0 + d4) << 13, tmp1 = (d0 - d4) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    uint32_t t0 = d7, t1 = d5, t2 = d3, t3 = d1;
    z1 = t0 + t3;
    uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 *= (uint32_t)-16069; z4 *= (uint32_t)-3196;
    z3 += z5; z4 += z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    out[0] = descale(tmp10 + t3, shift); out[7 * ostride] = descale(tmp10 - t3, shift);
    out[ostride] = descale(tmp11 + t2, shift); out[6 * ostride] = descale(tmp11 - t2, shift);
    out[2 * ostride] = descale(tmp12 + t1, shift); out[5 * ostride] = descale(tmp12 - t1, shift);
    out[3 * ostride] = descale(tmp13 + t0, shift); out[4 * ostride] = descale(tmp13 - t0, shift);
}
inline uint8_t limit(int32_t x)
{
    static uint8_t table[1024];
    static bool made = false;
    if (!made) {                                             // libjpeg's prepare_range_limit_table, read from its centre
        for (int i = 0; i < 1024; i++) table[i] = (uint8_t)(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
        made = true;
    }
    return table[x & 1023];
}

struct Image {
    int w, h, ncomp, hs, vs, mcus_x, mcus_y;                 // hs x vs: luma blocks of an MCU
    int cw, ch;                                              // a chroma component's own extent
    std::vector<uint8_t> plane[3];                           // over the MCU grid
    int pitch[3];
    int32_t lo, hi;                                          // the extremes of the pre-limit row results
};

// coefs: 64 x int16 a block in natural order, the blocks in the order of the interleaved scan; quant: Y, Cb, Cr in NATURAL order
inline void planes(Image &M, const int16_t *coefs, const uint16_t quant[3][64])
{
    const int bpm = M.ncomp == 3 ? M.hs * M.vs + 2 : 1;
    M.cw = (M.w + M.hs - 1) / M.hs; M.ch = (M.h + M.vs - 1) / M.vs;
    M.lo = 0; M.hi = 0;
    for (int c = 0; c < M.ncomp; c++) {
        M.pitch[c] = M.mcus_x * 8 * (c ? 1 : M.hs);
        M.plane[c].assign((size_t)M.pitch[c] * M.mcus_y * 8 * (c ? 1 : M.vs), 0);
    }
    for (int my = 0; my < M.mcus_y; my++)
        for (int mx = 0; mx < M.mcus_x; mx++)
            for (int k = 0; k < bpm; k++) {
                const int16_t *blk = coefs + ((size_t)(my * M.mcus_x + mx) * bpm + k) * 64;
                const int nl = M.ncomp == 3 ? M.hs * M.vs : 1, c = k < nl ? 0 : k - nl + 1;
                const int bx = c ? mx : mx * M.hs + k % M.hs, by = c ? my : my * M.vs + k / M.hs;
                int32_t deq[64], ws[64], row[8];
                for (int i = 0; i < 64; i++) deq[i] = (int32_t)((uint32_t)(int32_t)blk[i] * (uint32_t)quant[c][i]);
                for (int x = 0; x < 8; x++) pass(deq + x, 8, ws + x, 8, 11);
                for (int y = 0; y < 8; y++) {
                    pass(ws + 8 * y, 1, row, 1, 18);
                    for (int x = 0; x < 8; x++) {
                        if (row[x] < M.lo) M.lo = row[x];
                        if (row[x] > M.hi) M.hi = row[x];
                        M.plane[c][(size_t)(by * 8 + y) * M.pitch[c] + bx * 8 + x] = limit(row[x]);
                    }
                }
            }
}

// the upsampled sample of chroma component c at output pixel (x, y): jdsample.c's fancy upsampling over the component's own extent
inline int chroma_at(const Image &M, int c, int x, int y)
{
    const uint8_t *p = M.plane[c].data();
    const int pitch = M.pitch[c];
    auto s = [&](int j, int i) { j = j < 0 ? 0 : j >= M.ch ? M.ch - 1 : j; i = i < 0 ? 0 : i >= M.cw ? M.cw - 1 : i; return (int)p[(size_t)j * pitch + i]; };
    if (M.hs == 1 && M.vs == 1) return s(y, x);
    if (M.vs == 1) { const int i = x >> 1; return (x & 1) ? (3 * s(y, i) + s(y, i + 1) + 2) >> 2 : (3 * s(y, i) + s(y, i - 1) + 1) >> 2; }
    const int j = y >> 1, jn = (y & 1) ? j + 1 : j - 1;
    if (M.hs == 1) return (3 * s(j, x) + s(jn, x) + ((y & 1) ? 2 : 1)) >> 2;
    const int i = x >> 1;
    auto t = [&](int ii) { return 3 * s(j, ii) + s(jn, ii); };
    return (x & 1) ? (3 * t(i) + t(i + 1) + 7) >> 4 : (3 * t(i) + t(i - 1) + 8) >> 4;
}
inline int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// out: h rows of w pixels -- RGBA (A = 0xFF), or gray: the Y plane
inline void pixels(const Image &M, bool gray, uint8_t *out, size_t pitch)
{
    for (int y = 0; y < M.h; y++)
        for (int x = 0; x < M.w; x++) {
            const int Y = M.plane[0][(size_t)y * M.pitch[0] + x];
            if (gray) { out[y * pitch + x] = (uint8_t)Y; continue; }
            int cb = 0, cr = 0;
            if (M.ncomp == 3) { cb = chroma_at(M, 1, x, y) - 128; cr = chroma_at(M, 2, x, y) - 128; }
            uint8_t *px = out + y * pitch + 4 * (size_t)x;
            px[0] = (uint8_t)clamp255(Y + ((91881 * cr + 32768) >> 16));
            px[1] = (uint8_t)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            px[2] = (uint8_t)clamp255(Y + ((116130 * cb + 32768) >> 16));
            px[3] = 255;
        }
}

} // namespace exact_twin
#endif
