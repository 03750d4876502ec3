// tests/hostsim/exact_adobe_sim.cpp -- TEST INFRASTRUCTURE: the colour models of the libjpeg-exact decode lane by lane on the
// CPU, over the plan the runtime makes (jda_exact_check_cs, jda_exact_geometry4, jda_exact_fill4 of jda_exact_plan.h): jda_exact_colour4 of
// every layout, K sampling, model and pixel type, and the RGB instances of the colour stages (jda_exact_colour_rgb, jda_exact_colour_scaled_rgb).
//
// exactadobesim_run lays a file out as the runtime has it resident -- the dense coefficient image of jda_coef_prepare, a four-component
// file's component 3 as the gray image beside it, each an allocation of exactly its size --, runs every tile through the kernels' OWN
// per-lane functions the way a wavefront runs them (exact_sim.cpp's scheme: the 64 lanes one after the other through a phase, the LDS share
// poisoned before every tile; K's tiles as gray tiles into the fourth plane), every global access held to its allocation and alignment, the
// surface's stores counted byte by byte.  At full size the planes and the pixels are then compared with a row-major twin: exact_twin.h's
// planes, and the colour rules written out once more below.  Not part of libjpegdec_amd.so; nothing in the product calls it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_exact_plan.h"
#include "exact_twin.h"

extern "C" void jda_coef_image_raw_quant(const jda_coef_image *img, uint16_t *quant_zz, uint8_t *q_id, int32_t *adobe);

namespace {
struct Region { const uint8_t *base; size_t bytes; bool writable; };
struct AdobeIO {
    std::vector<Region> regions;
    uint8_t *surface; size_t surface_bytes;
    std::vector<uint8_t> hits;                               // per byte of the surface: stores that touched it
    int err;
    AdobeIO() : surface(NULL), surface_bytes(0), err(0) {}
    void add(const void *p, size_t n, bool w) { Region r = { (const uint8_t *)p, n, w }; regions.push_back(r); }
    bool inside(const void *q, size_t n, bool write)
    {
        const uint8_t *p = (const uint8_t *)q;
        if (((uintptr_t)p & (n - 1)) != 0) return false;
        for (const Region &r : regions)
            if (p >= r.base && (size_t)(p - r.base) + n <= r.bytes && (!write || r.writable)) return true;
        return false;
    }
    void fail(int code) { if (!err) err = code; }
    void ld128(const uint8_t *b, uint32_t i, uint32_t *v) { const uint8_t *p = b + (size_t)i * 16u; if (!inside(p, 16, false)) { fail(-10); memset(v, 0, 16); return; } memcpy(v, p, 16); }
    uint32_t ld32u(const uint8_t *b, uint32_t i) { return ld32(b, 4u * i); }
    uint32_t ld32(const void *b, uint32_t off) { const uint8_t *p = (const uint8_t *)b + off; uint32_t v = 0; if (!inside(p, 4, false)) { fail(-11); return 0; } memcpy(&v, p, 4); return v; }
    uint32_t ld32(const uint32_t *p) { return ld32(p, 0u); }
    template <class P> const void *ldptr(P const *p) { if (!inside(p, 8, false)) { fail(-12); return NULL; } return (const void *)*p; }
    uint32_t ld8(const uint8_t *b, uint32_t off) { if (!inside(b + off, 1, false)) { fail(-13); return 0; } return b[off]; }
    void store(uint8_t *b, uint32_t off, const void *v, size_t n)
    {
        uint8_t *p = b + off;
        if (!inside(p, n, true)) { fail(-14 - (n == 16 ? 0 : n == 8 ? 1 : n == 4 ? 2 : 3)); return; }
        memcpy(p, v, n);
        if (surface && p >= surface && p < surface + surface_bytes)
            for (size_t k = 0; k < n; k++) if (hits[(size_t)(p - surface) + k] < 255) hits[(size_t)(p - surface) + k]++;
    }
    void st64(uint8_t *b, uint32_t off, uint32_t lo, uint32_t hi) { const uint32_t v[2] = { lo, hi }; store(b, off, v, 8); }
    void st128(uint8_t *b, uint32_t off, const uint32_t *w) { store(b, off, w, 16); }
    void st32(uint8_t *b, uint32_t off, uint32_t v) { store(b, off, &v, 4); }
    void st8(uint8_t *b, uint32_t off, uint32_t v) { const uint8_t c = (uint8_t)v; store(b, off, &c, 1); }
};

// the planes stage of one image's tiles from its dense coefficient image, at full size
template <int MODE>
void planes_full(const jda_dev_desc &D, const jda_ex_desc *Xp, const std::vector<jda_strip> &tiles, AdobeIO &io, int32_t *info)
{
    typedef jda_mode_traits<MODE> T;
    std::vector<uint64_t> store((jda_ex_layout<MODE>::WAVE_BYTES + 7) / 8);
    uint8_t *qt = (uint8_t *)store.data(), *wl = qt + JDA_EX_QUANT_BYTES;
    const jda_ex_desc X = *Xp;
    for (const jda_strip &S : tiles) {
        if (S.count == 0) continue;
        memset(qt, 0xA5, jda_ex_layout<MODE>::WAVE_BYTES);
        jda_tile_ctx C;
        C.first_mcu = S.mcu_y * D.mcus_x + S.mcu_x0; C.count = S.count; C.first_block = C.first_mcu * (uint32_t)T::NBLK;
        C.win_lo = C.win_len = C.win_need = 0;
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ex_tables(io, Xp, t, qt);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_load<MODE>(io, D, C, t, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ex_block<MODE>(io, X, S, C, t, wl, qt);
        info[0]++;
    }
}
// .. and at 1/2, 1/4, 1/8
template <int MODE, int SCALE>
void planes_scaled(const jda_dev_desc &D, const jda_ex_desc *Xp, const std::vector<jda_strip> &tiles, AdobeIO &io, int32_t *info)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    std::vector<uint64_t> store((jda_ex_layout<MODE>::WAVE_BYTES + 7) / 8);
    uint8_t *qt = (uint8_t *)store.data(), *wl = qt + JDA_EX_QUANT_BYTES;
    const jda_ex_desc X = *Xp;
    for (const jda_strip &S : tiles) {
        if (S.count == 0) continue;
        memset(qt, 0xA5, jda_ex_layout<MODE>::WAVE_BYTES);
        jda_tile_ctx C;
        C.first_mcu = S.mcu_y * D.mcus_x + S.mcu_x0; C.count = S.count; C.first_block = C.first_mcu * (uint32_t)T::NBLK;
        C.win_lo = C.win_len = C.win_need = 0;
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ex_tables(io, Xp, t, qt);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_load<MODE>(io, D, C, t, wl);
        uint32_t px[JDA_TILE_THREADS][16];
        memset(px, 0xA5, sizeof(px));
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_block<MODE, SCALE, 0>(io, X, (const jda_ex_src *)NULL, C, t, wl, qt, px[t]);
        memset(wl + L::COEF_OFF, 0x5A, L::BLOCKS * JDA_COEF_STRIDE);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_stage<MODE, SCALE>(X, S, C, t, wl + L::COEF_OFF, px[t]);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_store<MODE, SCALE>(io, X, S, t, wl + L::COEF_OFF);
        info[0]++;
    }
}
// kind: 0 jda_exact_colour[_scaled], 1 the RGB instance, 2 jda_exact_colour4
template <int MODE>
void run_image(int scale, int kind, const jda_dev_desc &D, const jda_ex_desc *Xp, const std::vector<jda_strip> &tiles, bool colour, AdobeIO &io, int32_t *info)
{
    if (scale == 1) planes_full<MODE>(D, Xp, tiles, io, info);
    else if (scale == 2) planes_scaled<MODE, 2>(D, Xp, tiles, io, info);
    else if (scale == 4) planes_scaled<MODE, 4>(D, Xp, tiles, io, info);
    else planes_scaled<MODE, 8>(D, Xp, tiles, io, info);
    if (!colour) return;
    const jda_ex_desc X = *Xp;
    for (const jda_strip &S : tiles) {
        if (S.count == 0) continue;
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) {
            if (kind == 2) jda_ex4_colour_tile<MODE>(io, X, S, t);
            else if (scale == 1) { if (kind == 1) jda_ex_colour_tile<MODE, true>(io, X, S, t); else jda_ex_colour_tile<MODE>(io, X, S, t); }
            else { if (kind == 1) jda_exs_colour_tile<MODE, true>(io, X, S, t); else jda_exs_colour_tile<MODE>(io, X, S, t); }
        }
    }
}
template <class T> T *dup(const T *p, size_t n, size_t extra = 0)      // an allocation of exactly n (+ extra zero) elements' bytes, 16-byte aligned
{
    void *q = NULL;
    if (posix_memalign(&q, 16, (n + extra) * sizeof(T) + 16) != 0) return NULL;
    memset(q, 0, (n + extra) * sizeof(T) + 16);
    if (n) memcpy(q, p, n * sizeof(T));
    return (T *)q;
}
// a dense coefficient image as it is resident: quantisers | coefficients
uint8_t *resident(const jda_coef_image *img, AdobeIO &io, std::vector<void *> &owned, jda_dev_desc &D)
{
    uint32_t nb = 0;
    const int16_t *cf = jda_coef_image_coefficients(img, &nb);
    const int16_t *quant = jda_coef_image_quant(img, NULL);
    uint8_t *blk = dup<uint8_t>(NULL, 0, JDA_CT_QUANT_BYTES + (size_t)nb * 128);
    owned.push_back(blk);
    memcpy(blk, quant, JDA_CT_QUANT_BYTES); memcpy(blk + JDA_CT_QUANT_BYTES, cf, (size_t)nb * 128);
    io.add(blk, JDA_CT_QUANT_BYTES + (size_t)nb * 128, false);
    D.tables = blk; D.scan = blk + JDA_CT_QUANT_BYTES;
    return blk;
}
// the row-major twin of the colour rules: a sample of a 1x1 component under the output pixel (x, y) -- jdsample.c's fancy upsampling, or
// replication where the component is at most two samples wide --, Pillow's MULDIV255 and cmyk2rgb
int sample_at(const exact_twin::Image &M, int c, int x, int y)
{
    if (M.hs == 2 && M.cw <= 2) {
        const int i = (x >> 1) < M.cw ? (x >> 1) : M.cw - 1, j = M.vs == 2 ? y >> 1 : y;
        return M.plane[c][(size_t)j * M.pitch[c] + i];
    }
    return exact_twin::chroma_at(M, c, x, y);
}
int muldiv255(int a, int b) { const int t = a * b + 128; return ((t >> 8) + t) >> 8; }
} // namespace

// the plan alone: jda_exact_check_cs's answer for a header of that shape, and (out, 16 entries) hs, vs, pitch_y, pitch_c, rows_y, rows_c,
// cw, ch, off[1], off[2], off_k, k_full, pitch_k, rows_k, kw * 65536 + kh, bytes
extern "C" int exactadobesim_plan(int width, int height, int ncomp, int subsample, int k_hv, int colour, int pixel_type, int scale, int baseline_image, int64_t *out)
{
    jda_image_info I;
    memset(&I, 0, sizeof(I));
    I.width = width; I.height = height; I.ncomp = ncomp; I.subsample = subsample;
    const int mode = jda_mode_of(I);
    const int mw = (mode == JDA_MODE_420 || mode == JDA_MODE_422) ? 16 : 8, mh = (mode == JDA_MODE_420 || mode == JDA_MODE_440) ? 16 : 8;
    I.mcus_x = (width + mw - 1) / mw; I.mcus_y = (height + mh - 1) / mh;
    int rc = jda_exact_check_cs(I, colour, pixel_type, baseline_image, (uint32_t)(I.mcus_x * I.mcus_y), scale, k_hv);
    if (rc != JDA_SUCCESS) return rc;
    jda_exact_geo G;
    if (ncomp == 4) { I.ncomp = 3; rc = jda_exact_geometry4(I, k_hv != 0x11, &G); }
    else rc = jda_exact_geometry_scaled(I, false, scale, &G);
    if (rc != JDA_SUCCESS) return rc;
    const int64_t v[16] = { G.hs, G.vs, G.pitch_y, G.pitch_c, G.rows_y, G.rows_c, G.cw, G.ch, (int64_t)G.off[1], (int64_t)G.off[2], (int64_t)G.off_k, G.k_full, G.pitch_k,
                            G.rows_k, (int64_t)G.kw * 65536 + G.kh, (int64_t)G.bytes };
    memcpy(out, v, sizeof(v));
    return JDA_SUCCESS;
}

// jda_exact_check's answers, as they were (the old calls keep them): for the CPU test that holds them unchanged
extern "C" int exactadobesim_old_check(int width, int height, int ncomp, int subsample, int adobe, int pixel_type)
{
    jda_image_info I;
    memset(&I, 0, sizeof(I));
    I.width = width; I.height = height; I.ncomp = ncomp; I.subsample = subsample; I.mcus_x = I.mcus_y = 1;
    return jda_exact_check(I, adobe, pixel_type, 0, 0);
}

// One file through jda_coef_prepare and the lanes.  out: the surface (JDA_RGB8888 or JDA_CMYK8888; pitch, width_px, rows as jda_output's);
// twin_out (full size only): h x w x 4 bytes from the row-major twin, dense; planes_out: the components' planes at their own extents, dense,
// one behind the other, from the lanes.  info[0]: tiles run (K's included), info[1] / info[2]: the twin's extremes of the pre-limit row
// results, info[3]: bytes of the surface written more than once, info[4]: written bytes outside the clip, info[5]: the colour model,
// info[6]: plane bytes that differ from the twin's (full size), info[7]: 1 where twin_out was made.
// Returns 0, a JDA_* code (> 0) or a violation (< 0: -10 .. -17 an access outside its allocation or misaligned, -20 a visible byte no lane wrote).
extern "C" int exactadobesim_run(const uint8_t *jpeg, int len, int pixel_type, int scale, uint8_t *out, int pitch, int width_px, int rows, uint8_t *twin_out,
                                 uint8_t *planes_out, int32_t *info)
{
    int32_t err = 0, dummy[8];
    if (!info) info = dummy;
    memset(info, 0, 8 * sizeof(int32_t));
    jda_exact_file E;
    int rc = jda_exact_probe(jpeg, len, &E);
    if (rc != JDA_SUCCESS) return rc;
    info[5] = E.colour_model;
    jda_coef_image *cimg = jda_coef_prepare(jpeg, len, &err);
    if (!cimg) return err;
    const jda_coef_image *kimg = jda_coef_image_component3(cimg);
    jda_image_info I = *jda_coef_image_get_info(cimg);
    rc = jda_exact_check_cs(I, E.colour_model, pixel_type, 0, 0, scale, E.k_sampling);
    if (rc == JDA_SUCCESS && !jda_exact_scale_ok(scale)) rc = JDA_INVALID_PARAMETER;
    const bool four = I.ncomp == 4, rgb = E.colour_model == JDA_CS_RGB;
    if (rc == JDA_SUCCESS && four && !kimg) rc = JDA_UNSUPPORTED_FEATURE;
    if (four) { I.ncomp = 3; I.bpp = 24; }
    jda_exact_geo G;
    if (rc == JDA_SUCCESS) rc = four ? jda_exact_geometry4(I, E.k_sampling != 0x11, &G) : jda_exact_geometry_scaled(I, false, scale, &G);
    const int clip_w = width_px < (int)G.w ? width_px : (int)G.w, clip_h = rows < (int)G.h ? rows : (int)G.h;
    if (rc == JDA_SUCCESS && out && (pitch < clip_w * 4 || (pitch & 15) || ((uintptr_t)out & 15) || width_px < 0 || rows < 0)) rc = JDA_INVALID_PARAMETER;
    if (rc != JDA_SUCCESS) { jda_coef_image_free(cimg); return rc; }
    AdobeIO io;
    std::vector<void *> owned;
    uint16_t qzz[3][64], qk[3][64];
    uint8_t qid[3];
    int32_t adobe = 0;
    jda_coef_image_raw_quant(cimg, &qzz[0][0], qid, &adobe);
    if (kimg) jda_coef_image_raw_quant(kimg, &qk[0][0], qid, &adobe);
    jda_dev_desc D, DK;
    memset(&D, 0, sizeof(D)); memset(&DK, 0, sizeof(DK));
    D.mode = (uint8_t)jda_mode_of(I); D.ncomp = (uint8_t)I.ncomp; D.mcus_x = (uint32_t)I.mcus_x; D.mcus_y = (uint32_t)I.mcus_y;
    resident(cimg, io, owned, D);
    if (four) {
        const jda_image_info &KI = *jda_coef_image_get_info(kimg);
        DK.mode = (uint8_t)JDA_MODE_GRAY; DK.ncomp = 1; DK.mcus_x = (uint32_t)KI.mcus_x; DK.mcus_y = (uint32_t)KI.mcus_y;
        resident(kimg, io, owned, DK);
    }
    uint8_t *scratch = dup<uint8_t>(NULL, 0, G.bytes);
    owned.push_back(scratch);
    memset(scratch, 0xA5, G.bytes);
    io.add(scratch, G.bytes, true);
    jda_ex_desc *X = dup<jda_ex_desc>(NULL, 0, 2);
    owned.push_back(X);
    io.add(X, 2 * sizeof(jda_ex_desc), false);
    jda_output O;
    O.pixels = out; O.pitch_bytes = pitch; O.width_px = width_px; O.rows = rows;
    if (four) jda_exact_fill4(X[0], X[1], I, qzz, qk[0], G, scratch, out ? &O : NULL, pixel_type, E.colour_model == JDA_CS_YCCK);
    else jda_exact_fill_scaled(X[0], I, qzz, G, scratch, out ? &O : NULL, pixel_type, false);
    if (out) {
        io.surface = out; io.surface_bytes = (size_t)pitch * (size_t)(clip_h > 0 ? clip_h : 0);
        io.hits.assign(io.surface_bytes, 0);
        io.add(out, io.surface_bytes, true);
    }
    std::vector<jda_strip> tiles, ktiles;
    jda_append_strips(tiles, 0, D.mcus_x, D.mcus_y, D.mode);
    if (four) {                                              // (K's tiles first: the gray launch comes before the colour stage, in any order with the others)
        jda_append_strips(ktiles, 1, DK.mcus_x, DK.mcus_y, JDA_MODE_GRAY);
        run_image<JDA_MODE_GRAY>(1, 0, DK, X + 1, ktiles, false, io, info);
    }
    const int kind = four ? 2 : rgb ? 1 : 0;
    switch (D.mode) {
    case JDA_MODE_GRAY: run_image<JDA_MODE_GRAY>(scale, 0, D, X, tiles, out != NULL, io, info); break;
    case JDA_MODE_444: run_image<JDA_MODE_444>(scale, kind, D, X, tiles, out != NULL, io, info); break;
    case JDA_MODE_420: run_image<JDA_MODE_420>(scale, kind, D, X, tiles, out != NULL, io, info); break;
    case JDA_MODE_422: run_image<JDA_MODE_422>(scale, kind, D, X, tiles, out != NULL, io, info); break;
    default: run_image<JDA_MODE_440>(scale, kind, D, X, tiles, out != NULL, io, info); break;
    }
    rc = io.err;
    for (size_t k = 0; k < io.hits.size(); k++) {
        const size_t y = k / (size_t)pitch, x = k % (size_t)pitch;
        if (io.hits[k] > 1) info[3]++;
        if (io.hits[k] && ((int)y >= clip_h || (int)x >= clip_w * 4)) info[4]++;
        if (!io.hits[k] && (int)y < clip_h && (int)x < clip_w * 4 && rc == 0) rc = -20;
    }
    // the planes as the lanes left them, at their own extents
    const int ncomp = four ? 4 : I.ncomp;
    const uint32_t w0 = G.scale > 1u ? G.w : (uint32_t)I.width, h0 = G.scale > 1u ? G.h : (uint32_t)I.height;
    if (planes_out) {
        size_t at = 0;
        for (int c = 0; c < ncomp; c++) {
            const uint32_t ew = c == 3 ? G.kw : c ? G.cw : w0, eh = c == 3 ? G.kh : c ? G.ch : h0, p = c == 3 ? G.pitch_k : c ? G.pitch_c : G.pitch_y;
            for (uint32_t y = 0; y < eh; y++, at += ew) memcpy(planes_out + at, scratch + (c == 3 ? G.off_k : G.off[c]) + (size_t)y * p, ew);
        }
    }
    if (scale == 1) {
        exact_twin::Image M, MK;
        M.w = I.width; M.h = I.height; M.ncomp = I.ncomp; M.hs = (int)G.hs; M.vs = (int)G.vs; M.mcus_x = I.mcus_x; M.mcus_y = I.mcus_y;
        uint16_t qn[3][64];
        uint32_t nb = 0;
        for (int c = 0; c < 3; c++) for (uint32_t z = 0; z < 64; z++) qn[c][jda_en_zigzag(z)] = qzz[c][z];
        exact_twin::planes(M, jda_coef_image_coefficients(cimg, &nb), qn);
        info[1] = M.lo; info[2] = M.hi;
        if (four) {                                          // K: a gray image over its own grid
            const jda_image_info &KI = *jda_coef_image_get_info(kimg);
            MK.w = KI.width; MK.h = KI.height; MK.ncomp = 1; MK.hs = MK.vs = 1; MK.mcus_x = KI.mcus_x; MK.mcus_y = KI.mcus_y;
            for (uint32_t z = 0; z < 64; z++) qn[0][jda_en_zigzag(z)] = qk[0][z];
            exact_twin::planes(MK, jda_coef_image_coefficients(kimg, &nb), qn);
            if (MK.lo < info[1]) info[1] = MK.lo;
            if (MK.hi > info[2]) info[2] = MK.hi;
        }
        for (int c = 0; c < ncomp; c++) {
            const uint32_t ew = c == 3 ? G.kw : c ? G.cw : w0, eh = c == 3 ? G.kh : c ? G.ch : h0, p = c == 3 ? G.pitch_k : c ? G.pitch_c : G.pitch_y;
            const exact_twin::Image &T = c == 3 ? MK : M;
            for (uint32_t y = 0; y < eh; y++)
                for (uint32_t x = 0; x < ew; x++)
                    if (scratch[(c == 3 ? G.off_k : G.off[c]) + (size_t)y * p + x] != T.plane[c == 3 ? 0 : c][(size_t)y * T.pitch[c == 3 ? 0 : c] + x]) info[6]++;
        }
        if (twin_out) {
            exact_twin::Image MC = M;                        // K at 1x1 under a subsampled component 0: a chroma plane's geometry
            if (four && !G.k_full) { MC.plane[1] = MK.plane[0]; MC.pitch[1] = MK.pitch[0]; }
            for (int y = 0; y < I.height; y++)
                for (int x = 0; x < I.width; x++) {
                    uint8_t *px = twin_out + ((size_t)y * I.width + x) * 4;
                    const int s0 = M.plane[0][(size_t)y * M.pitch[0] + x];
                    const int s1 = I.ncomp == 3 ? sample_at(M, 1, x, y) : 128, s2 = I.ncomp == 3 ? sample_at(M, 2, x, y) : 128;
                    int r = s0, g = s1, b = s2;
                    if (!rgb && !(four && E.colour_model == JDA_CS_CMYK)) {      // jdcolor.c's YCbCr -> RGB
                        r = exact_twin::clamp255(s0 + ((91881 * (s2 - 128) + 32768) >> 16));
                        g = exact_twin::clamp255(s0 + ((-22554 * (s1 - 128) - 46802 * (s2 - 128) + 32768) >> 16));
                        b = exact_twin::clamp255(s0 + ((116130 * (s1 - 128) + 32768) >> 16));
                    }
                    if (!four) { px[0] = (uint8_t)r; px[1] = (uint8_t)g; px[2] = (uint8_t)b; px[3] = 255; continue; }
                    const int k = G.k_full ? MK.plane[0][(size_t)y * MK.pitch[0] + x] : sample_at(MC, 1, x, y);
                    // Pillow's "CMYK;I" bytes: a CMYK file's samples inverted; a YCCK file's R, G, B (libjpeg's 255 - R inverted again) and 255 - K
                    const int c4[4] = { E.colour_model == JDA_CS_CMYK ? 255 - s0 : r, E.colour_model == JDA_CS_CMYK ? 255 - s1 : g, E.colour_model == JDA_CS_CMYK ? 255 - s2 : b, 255 - k };
                    if (pixel_type == JDA_CMYK8888) { for (int i = 0; i < 4; i++) px[i] = (uint8_t)c4[i]; continue; }
                    const int nk = 255 - c4[3];
                    for (int i = 0; i < 3; i++) px[i] = (uint8_t)exact_twin::clamp255(nk - muldiv255(c4[i], nk));
                    px[3] = 255;
                }
            info[7] = 1;
        }
    }
    for (void *p : owned) free(p);
    jda_coef_image_free(cimg);
    return rc;
}
