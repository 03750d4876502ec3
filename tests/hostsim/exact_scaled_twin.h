// tests/hostsim/exact_scaled_twin.h -- TEST INFRASTRUCTURE: the libjpeg-exact decode at 1/2, 1/4 and 1/8 written row-major
// in plain C++, the way libjpeg's own files read (jdmaster.c, jidctred.c, jdsample.c, jdcolor.c), sharing no code with the kernels' per-lane
// functions.  tests/test_exact_scaled_cpu.py holds it to the numpy twin (tests/exact_scaled_util.py), and exact_scaled_sim.cpp holds the
// kernels' lanes to it.  The 8x8 pass and the range limit are exact_twin.h's.
#ifndef EXACT_SCALED_TWIN_H
#define EXACT_SCALED_TWIN_H

#include "exact_twin.h"

namespace exact_scaled_twin {

enum { UP_NONE = 0, UP_H2V1_FANCY = 1, UP_H2V1_REPLICATE = 2, UP_H1V2_FANCY = 3, UP_H1V2_REPLICATE = 4 };

struct Image {
    int w, h, ncomp, hs, vs, mcus_x, mcus_y, scale;          // w x h: the FILE's size; hs x vs: luma blocks of an MCU
    int ss[3], ow, oh, ew[3], eh[3], up;                     // per component: IDCT size, own extent; ow x oh: the output
    std::vector<uint8_t> plane[3];                           // over the MCU grid, ss x ss samples a block
    int pitch[3];
    int32_t lo, hi;                                          // the extremes of the pre-limit results
};

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// jdmaster.c: the scaled sizes
inline void geometry(Image &M)
{
    const int mn = 8 / M.scale;
    for (int c = 0; c < M.ncomp; c++) {
        const int h_c = c ? 1 : M.hs, v_c = c ? 1 : M.vs;
        int ss = mn;
        while (ss < 8 && (M.hs * mn) % (h_c * ss * 2) == 0 && (M.vs * mn) % (v_c * ss * 2) == 0) ss *= 2;
        M.ss[c] = ss;
        M.ew[c] = ceil_div((long long)M.w * h_c * ss, M.hs * 8);
        M.eh[c] = ceil_div((long long)M.h * v_c * ss, M.vs * 8);
    }
    M.ow = ceil_div(M.w, M.scale); M.oh = ceil_div(M.h, M.scale);
    M.up = UP_NONE;
    if (M.ncomp == 3) {
        const int hx = M.hs * mn / M.ss[1], vx = M.vs * mn / M.ss[1];      // the expansion that is left
        const bool fancy = mn > 1;
        if (hx == 2 && vx == 1) M.up = fancy && M.ew[1] > 2 ? UP_H2V1_FANCY : UP_H2V1_REPLICATE;
        else if (hx == 1 && vx == 2) M.up = fancy ? UP_H1V2_FANCY : UP_H1V2_REPLICATE;
    }
}

inline int32_t mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
inline int32_t add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
inline int32_t sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
inline int32_t shl(int32_t a, int n) { return (int32_t)((uint32_t)a << n); }
inline int32_t descale(int32_t x, int n) { return add(x, 1 << (n - 1)) >> n; }

// jidctred.c, jpeg_idct_4x4: in[k * stride] is frequency k; four results
inline void pass4(const int32_t *in, int stride, int32_t *out, int ostride, int shift)
{
    const int32_t tmp0 = shl(in[0], 14);
    const int32_t tmp2 = add(mul(in[2 * stride], 15137), mul(in[6 * stride], -6270));
    const int32_t tmp10 = add(tmp0, tmp2), tmp12 = sub(tmp0, tmp2);
    const int32_t z1 = in[7 * stride], z2 = in[5 * stride], z3 = in[3 * stride], z4 = in[stride];
    const int32_t o1 = add(add(mul(z1, -1730), mul(z2, 11893)), add(mul(z3, -17799), mul(z4, 8697)));
    const int32_t o2 = add(add(mul(z1, -4176), mul(z2, -4926)), add(mul(z3, 7373), mul(z4, 20995)));
    out[0] = descale(add(tmp10, o2), shift); out[3 * ostride] = descale(sub(tmp10, o2), shift);
    out[ostride] = descale(add(tmp12, o1), shift); out[2 * ostride] = descale(sub(tmp12, o1), shift);
}
// jpeg_idct_2x2
inline void pass2(const int32_t *in, int stride, int32_t *out, int ostride, int shift)
{
    const int32_t tmp10 = shl(in[0], 15);
    const int32_t tmp0 = add(add(mul(in[7 * stride], -5906), mul(in[5 * stride], 6967)), add(mul(in[3 * stride], -10426), mul(in[stride], 29692)));
    out[0] = descale(add(tmp10, tmp0), shift); out[ostride] = descale(sub(tmp10, tmp0), shift);
}

// deq: 64 dequantised coefficients in natural order -> ss x ss pre-limit results in res (row-major)
inline void idct(const int32_t *deq, int ss, int32_t *res)
{
    int32_t ws[64];
    memset(ws, 0, sizeof(ws));
    if (ss == 8) {
        for (int x = 0; x < 8; x++) exact_twin::pass(deq + x, 8, ws + x, 8, 11);
        for (int y = 0; y < 8; y++) exact_twin::pass(ws + 8 * y, 1, res + 8 * y, 1, 18);
    } else if (ss == 4) {
        for (int x = 0; x < 8; x++) if (x != 4) pass4(deq + x, 8, ws + x, 8, 12);
        for (int y = 0; y < 4; y++) pass4(ws + 8 * y, 1, res + 4 * y, 1, 19);
    } else if (ss == 2) {
        for (int x = 0; x < 8; x++) if (x == 0 || (x & 1)) pass2(deq + x, 8, ws + x, 8, 13);
        for (int y = 0; y < 2; y++) pass2(ws + 8 * y, 1, res + 2 * y, 1, 20);
    } else res[0] = descale(deq[0], 3);
}

// coefs: 64 x int16 a block in natural order, the blocks in the order of the interleaved scan; quant: Y, Cb, Cr in NATURAL order
inline void planes(Image &M, const int16_t *coefs, const uint16_t quant[3][64])
{
    geometry(M);
    const int bpm = M.ncomp == 3 ? M.hs * M.vs + 2 : 1;
    M.lo = 0; M.hi = 0;
    for (int c = 0; c < M.ncomp; c++) {
        M.pitch[c] = M.mcus_x * M.ss[c] * (c ? 1 : M.hs);
        M.plane[c].assign((size_t)M.pitch[c] * M.mcus_y * M.ss[c] * (c ? 1 : M.vs), 0);
    }
    for (int my = 0; my < M.mcus_y; my++)
        for (int mx = 0; mx < M.mcus_x; mx++)
            for (int k = 0; k < bpm; k++) {
                const int16_t *blk = coefs + ((size_t)(my * M.mcus_x + mx) * bpm + k) * 64;
                const int nl = M.ncomp == 3 ? M.hs * M.vs : 1, c = k < nl ? 0 : k - nl + 1, ss = M.ss[c];
                const int bx = c ? mx : mx * M.hs + k % M.hs, by = c ? my : my * M.vs + k / M.hs;
                int32_t deq[64], res[64];
                for (int i = 0; i < 64; i++) deq[i] = mul((int32_t)blk[i], (int32_t)quant[c][i]);
                idct(deq, ss, res);
                for (int y = 0; y < ss; y++)
                    for (int x = 0; x < ss; x++) {
                        const int32_t v = res[y * ss + x];
                        if (v < M.lo) M.lo = v;
                        if (v > M.hi) M.hi = v;
                        M.plane[c][(size_t)(by * ss + y) * M.pitch[c] + bx * ss + x] = exact_twin::limit(v);
                    }
            }
}

// jdsample.c at the image's scale: the sample of chroma component c under output pixel (x, y)
inline int chroma_at(const Image &M, int c, int x, int y)
{
    const uint8_t *p = M.plane[c].data();
    const int pitch = M.pitch[c], cw = M.ew[c], ch = M.eh[c];
    auto s = [&](int j, int i) { j = j < 0 ? 0 : j >= ch ? ch - 1 : j; i = i < 0 ? 0 : i >= cw ? cw - 1 : i; return (int)p[(size_t)j * pitch + i]; };
    switch (M.up) {
    case UP_NONE: return s(y, x);
    case UP_H2V1_REPLICATE: return s(y, x >> 1);
    case UP_H1V2_REPLICATE: return s(y >> 1, x);
    case UP_H2V1_FANCY: { const int i = x >> 1; return (x & 1) ? (3 * s(y, i) + s(y, i + 1) + 2) >> 2 : (3 * s(y, i) + s(y, i - 1) + 1) >> 2; }
    default: { const int j = y >> 1; return (y & 1) ? (3 * s(j, x) + s(j + 1, x) + 2) >> 2 : (3 * s(j, x) + s(j - 1, x) + 1) >> 2; }
    }
}
// out: oh rows of ow pixels -- RGBA (A = 0xFF), or gray: the Y plane
inline void pixels(const Image &M, bool gray, uint8_t *out, size_t pitch)
{
    for (int y = 0; y < M.oh; y++)
        for (int x = 0; x < M.ow; x++) {
            const int Y = M.plane[0][(size_t)y * M.pitch[0] + x];
            if (gray) { out[y * pitch + x] = (uint8_t)Y; continue; }
            int cb = 0, cr = 0;
            if (M.ncomp == 3) { cb = chroma_at(M, 1, x, y) - 128; cr = chroma_at(M, 2, x, y) - 128; }
            uint8_t *px = out + y * pitch + 4 * (size_t)x;
            px[0] = (uint8_t)exact_twin::clamp255(Y + ((91881 * cr + 32768) >> 16));
            px[1] = (uint8_t)exact_twin::clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            px[2] = (uint8_t)exact_twin::clamp255(Y + ((116130 * cb + 32768) >> 16));
            px[3] = 255;
        }
}

} // namespace exact_scaled_twin
#endif
