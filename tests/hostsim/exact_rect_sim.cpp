// tests/hostsim/exact_rect_sim.cpp -- TEST INFRASTRUCTURE: the libjpeg-exact decode of a pixel rectangle lane by lane on the
// CPU: the plan (a rectangle = a call of one image through jda_exact_plan_build / _place of jda_exact_plan.h, whose block holds the records
// and both tile lists; exactrectsim_call_plan: the plan of a whole call from header numbers), the EXISTING planes lanes (jda_ex_* at full size, jda_exs_*
// at 1/2, 1/4, 1/8; all three load phases) over the rectangle's tile list into a POISONED scratch, then the new colour lanes (jda_exr_* of
// jda_device_core.h, what jda_exact_colour_rect runs) over the destination's tile list.
//
// One source set-up serves many rectangles.  Per rectangle the scratch is poisoned and a written-bitmap cleared; every global access goes
// through an IO policy that holds it to its allocation and alignment, marks every plane byte a store touches and refuses a load of a plane
// byte no store of THIS rectangle's planes stage touched (-21) -- which proves the plan's MCU rectangle sufficient --; the surface's bytes
// are counted store by store: each byte inside the clip exactly once, none outside.  The whole image's row-major twin (exact_twin.h /
// exact_scaled_twin.h) is returned for the caller to crop.
// Not part of libjpegdec_amd.so; nothing in the product calls it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_exact_plan.h"
#include "exact_twin.h"
#include "exact_scaled_twin.h"

extern "C" void jda_image_raw_quant(const jda_image *img, uint16_t *quant_zz, int32_t *adobe);
extern "C" void jda_coef_image_raw_quant(const jda_coef_image *img, uint16_t *quant_zz, uint8_t *q_id, int32_t *adobe);

namespace {
struct Region { const uint8_t *base; size_t bytes; bool writable; };
struct RectIO {
    std::vector<Region> regions;
    uint8_t *surface; size_t surface_bytes;
    uint8_t *scratch; size_t scratch_bytes;
    std::vector<uint8_t> hits, written;                      // per byte of the surface: stores; per byte of the planes: stores of this rectangle
    int err;
    RectIO() : surface(NULL), surface_bytes(0), scratch(NULL), scratch_bytes(0), err(0) {}
    void add(const void *p, size_t n, bool w) { Region r = { (const uint8_t *)p, n, w }; regions.push_back(r); }
    bool inside(const void *q, size_t n, bool write)
    {
        const uint8_t *p = (const uint8_t *)q;
        if (((uintptr_t)p & (n - 1)) != 0) return false;
        if (surface && p >= surface && p < surface + surface_bytes) return write && (size_t)(p - surface) + n <= surface_bytes;
        if (scratch && p >= scratch && p < scratch + scratch_bytes) {
            if ((size_t)(p - scratch) + n > scratch_bytes) return false;
            if (!write) for (size_t k = 0; k < n; k++) if (!written[(size_t)(p - scratch) + k]) { fail(-21); return true; }
            return true;
        }
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
        if (scratch && p >= scratch && p < scratch + scratch_bytes)
            for (size_t k = 0; k < n; k++) if (written[(size_t)(p - scratch) + k] < 255) written[(size_t)(p - scratch) + k]++;
    }
    void st64(uint8_t *b, uint32_t off, uint32_t lo, uint32_t hi) { const uint32_t v[2] = { lo, hi }; store(b, off, v, 8); }
    void st128(uint8_t *b, uint32_t off, const uint32_t *w) { store(b, off, w, 16); }
    void st32(uint8_t *b, uint32_t off, uint32_t v) { store(b, off, &v, 4); }
    void st8(uint8_t *b, uint32_t off, uint32_t v) { const uint8_t c = (uint8_t)v; store(b, off, &c, 1); }
};

template <int MODE, int SOURCE> void load_phase(RectIO &io, const jda_dev_desc &D, const jda_tile_ctx &C, uint8_t *wl)
{
    if (SOURCE == 1) {
        uint32_t e0 = 0, e1 = 0;
        jda_cs_range<MODE>(io, D, C, &e0, &e1);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_cs_zero<MODE>(C, t, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_cs_scatter<MODE>(io, D, C, t, e0, e1, wl);
    } else {
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_load<MODE>(io, D, C, t, wl);
    }
}
// the planes stage of the existing kernels over `tiles`: jda_exact_planes<MODE, SOURCE> (SCALE 1) or jda_exact_planes_scaled<MODE, SOURCE, SCALE>
template <int MODE, int SCALE, int SOURCE>
void planes_at(const jda_dev_desc &D, const jda_ex_desc *Xp, const jda_ex_src *src, const std::vector<jda_strip> &tiles, RectIO &io, int32_t *n_tiles)
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
        if (SCALE == 1) {
            if (SOURCE == 2) for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ex_load_baseline<MODE>(io, src, C, t, wl);
            else load_phase<MODE, SOURCE>(io, D, C, wl);
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ex_block<MODE>(io, X, S, C, t, wl, qt);
        } else {
            enum { SC = SCALE == 1 ? 2 : SCALE };
            if (SOURCE == 2) for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_load_baseline<MODE, SC>(io, X, src, C, t, wl);
            else load_phase<MODE, SOURCE>(io, D, C, wl);
            uint32_t px[JDA_TILE_THREADS][16];
            memset(px, 0xA5, sizeof(px));
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_block<MODE, SC, SOURCE>(io, X, src, C, t, wl, qt, px[t]);
            memset(wl + L::COEF_OFF, 0x5A, L::BLOCKS * JDA_COEF_STRIDE);
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_stage<MODE, SC>(X, S, C, t, wl + L::COEF_OFF, px[t]);
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_store<MODE, SC>(io, X, S, t, wl + L::COEF_OFF);
        }
        (*n_tiles)++;
    }
}
template <int MODE, int SCALE>
void planes_src(int source, const jda_dev_desc &D, const jda_ex_desc *Xp, const jda_ex_src *src, const std::vector<jda_strip> &tiles, RectIO &io, int32_t *n_tiles)
{
    if (source == 2) planes_at<MODE, SCALE, 2>(D, Xp, src, tiles, io, n_tiles);
    else if (source == 1) planes_at<MODE, SCALE, 1>(D, Xp, src, tiles, io, n_tiles);
    else planes_at<MODE, SCALE, 0>(D, Xp, src, tiles, io, n_tiles);
}
template <int MODE>
void run_rect(int scale, int source, const jda_dev_desc &D, const jda_ex_desc *Xp, const jda_exr_rec *Rp, const jda_ex_src *src, const std::vector<jda_strip> &tiles,
              const std::vector<jda_strip> &ctiles, RectIO &io, int32_t *n_tiles)
{
    if (scale == 1) planes_src<MODE, 1>(source, D, Xp, src, tiles, io, n_tiles);
    else if (scale == 2) planes_src<MODE, 2>(source, D, Xp, src, tiles, io, n_tiles);
    else if (scale == 4) planes_src<MODE, 4>(source, D, Xp, src, tiles, io, n_tiles);
    else planes_src<MODE, 8>(source, D, Xp, src, tiles, io, n_tiles);
    const jda_ex_desc X = *Xp;
    const jda_exr_rec R = *Rp;
    for (const jda_strip &S : ctiles) {
        if (S.count == 0) continue;
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exr_colour_tile<MODE, false>(io, X, R, S, t);
    }
}
template <class T> T *dup(const T *p, size_t n, size_t extra = 0)
{
    void *q = NULL;
    if (posix_memalign(&q, 16, (n + extra) * sizeof(T) + 16) != 0) return NULL;
    memset(q, 0, (n + extra) * sizeof(T) + 16);
    if (n) memcpy(q, p, n * sizeof(T));
    return (T *)q;
}
jda_image_info info_of(int width, int height, int ncomp, int subsample)
{
    jda_image_info I;
    memset(&I, 0, sizeof(I));
    I.width = width; I.height = height; I.ncomp = ncomp; I.subsample = subsample;
    const int mode = jda_mode_of(I);
    const int mw = (mode == JDA_MODE_420 || mode == JDA_MODE_422) ? 16 : 8, mh = (mode == JDA_MODE_420 || mode == JDA_MODE_440) ? 16 : 8;
    I.mcus_x = (width + mw - 1) / mw; I.mcus_y = (height + mh - 1) / mh;
    return I;
}
} // namespace

// the plan alone, from a header's numbers: mcu = {mx0, my0, mx1, my1}; returns jda_exact_check's / the geometry's / jda_exact_rect_plan's code
extern "C" int exactrectsim_plan(int width, int height, int ncomp, int subsample, int pixel_type, int scale, const int32_t *rect, int32_t *mcu)
{
    const jda_image_info I = info_of(width, height, ncomp, subsample);
    int rc = jda_exact_check(I, 0, pixel_type, 0, 0);
    if (rc != JDA_SUCCESS) return rc;
    jda_exact_geo G;
    const bool luma_only = pixel_type == JDA_EIGHT_BIT_GRAYSCALE && ncomp == 3;
    rc = jda_exact_geometry_scaled(I, luma_only, scale, &G);
    if (rc != JDA_SUCCESS) return rc;
    return jda_exact_rect_plan(I, G, luma_only, rect, mcu);
}

// the records a workgroup of the planes kernels takes: what jda_append_strips pads an image's tiles to
extern "C" int exactrectsim_tiles_per_wg(int mode) { return (int)jda_tiles_per_wg(mode); }

// The plan of a whole call (jda_exact_plan_build + jda_exact_plan_place) from header numbers alone, nothing decoded.  hdr: n x 14 --
// width, height, ncomp, subsample, source kind (0 dense, 1 sparse, 2 baseline), colour model (JDA_CS_*), pixel type, scale, the rectangle
// {x, y, w, h}, the surface's width_px and rows.  A four-component image gets a component 3 of component 0's sampling.  with_rects == 0: the
// call has no rectangles (the hdr's are ignored).  The sources' and surfaces' addresses are made up (nothing reads through them); the block
// is real.  Out: status (n); launches: up to cap x 5 {kind, mode, scale, blob offset, tile records}, *n_launches; blob: the placed blob (up
// to blob_cap bytes); layout[10]: blob bytes, o_ex, o_src, o_rect, o_scratch, scratch, colour_begin, n_rec, n_planned, the block's address;
// image: n x 10 {kind or -1, plane_at, plane bytes, Y plane's offset from the block, mcu[4], jda_exact_tile_count of the MCU rectangle and
// of the whole image}.  Returns the build's code, or -1 where cap or blob_cap is too small.
extern "C" int exactrectsim_call_plan(int n, const int32_t *hdr, uint32_t flags, int with_rects, int32_t *status, int64_t *launches, int cap, int32_t *n_launches,
                                      uint8_t *blob, int64_t blob_cap, int64_t *layout, int64_t *image)
{
    std::vector<jda_exact_source> src(2u * (size_t)(n > 0 ? n : 0));
    std::vector<jda_output> outs((size_t)(n > 0 ? n : 0));
    std::vector<int32_t> pts, scales, rects;
    for (int i = 0; i < n; i++) {
        const int32_t *h = hdr + 14 * i;
        jda_exact_source &S = src[(size_t)i];
        memset(&S, 0, sizeof(S));
        S.info = info_of(h[0], h[1], h[2], h[3]);
        const int mode = jda_mode_of(S.info);
        const int hs = (mode == JDA_MODE_420 || mode == JDA_MODE_422) ? 2 : 1, vs = (mode == JDA_MODE_420 || mode == JDA_MODE_440) ? 2 : 1;
        S.info.blocks_per_mcu = h[2] == 1 ? 1 : hs * vs + 2; S.info.bpp = h[2] * 8; S.info.mcu_w = 8 * hs; S.info.mcu_h = 8 * vs;
        S.kind = (jda_exact_kind)h[4]; S.colour = h[5]; S.n_mcus_ok = (uint32_t)(S.info.mcus_x * S.info.mcus_y);
        for (int c = 0; c < 3; c++) for (int z = 0; z < 64; z++) S.quant[c][z] = (uint16_t)(1 + c + z);
        S.tables = (const uint8_t *)(uintptr_t)(0x10000000u + 0x100000u * (uint32_t)i); S.scan = S.tables + 0x1000;
        S.index = (const uint32_t *)(S.tables + 0x40000); S.dc = (const int16_t *)(S.tables + 0x80000); S.scan_len = 64;
        if (h[2] == 4) {
            jda_exact_source &K = src[(size_t)n + (size_t)i];
            memset(&K, 0, sizeof(K));
            K.info = info_of(h[0], h[1], 1, 0);
            K.info.mcus_x = S.info.mcus_x * hs; K.info.mcus_y = S.info.mcus_y * vs; K.info.blocks_per_mcu = 1; K.info.bpp = 8;
            K.kind = JDA_EXK_PLANES_DENSE; K.colour = JDA_CS_GRAY;
            for (int z = 0; z < 64; z++) K.quant[0][z] = (uint16_t)(7 + z);
            K.tables = S.tables + 0xC0000; K.scan = K.tables + 0x1000;
            S.k = &K;
        }
        pts.push_back(h[6]); scales.push_back(h[7]);
        rects.insert(rects.end(), h + 8, h + 12);
        jda_output &O = outs[(size_t)i];
        O.pixels = (void *)(uintptr_t)(0x40000000u + 0x1000000u * (uint32_t)i);
        O.width_px = h[12]; O.rows = h[13]; O.pitch_bytes = (h[12] * (h[6] == JDA_EIGHT_BIT_GRAYSCALE ? 1 : 4) + 15) & ~15;
    }
    jda_exact_plan plan;
    const int rc = jda_exact_plan_build(n, src.data(), outs.data(), pts.data(), NULL, scales.data(), flags, with_rects ? rects.data() : NULL, status, &plan);
    uint8_t *block = dup<uint8_t>(NULL, 0, plan.o_scratch + plan.scratch);
    if (rc == JDA_SUCCESS) jda_exact_plan_place(&plan, block);
    const int64_t lay[10] = { (int64_t)plan.blob.size(), (int64_t)plan.o_ex, (int64_t)plan.o_src, (int64_t)plan.o_rect, (int64_t)plan.o_scratch, (int64_t)plan.scratch,
                              (int64_t)plan.colour_begin, (int64_t)plan.n_rec, plan.n_planned, (int64_t)(uintptr_t)block };
    memcpy(layout, lay, sizeof(lay));
    *n_launches = (int32_t)plan.launches.size();
    const bool fits = plan.launches.size() <= (size_t)cap && plan.blob.size() <= (size_t)blob_cap;
    for (size_t k = 0; fits && k < plan.launches.size(); k++) {
        const jda_exact_launch &L = plan.launches[k];
        const int64_t row[5] = { (int64_t)L.kind, L.mode, L.scale, (int64_t)L.off, (int64_t)L.n_tiles };
        memcpy(launches + 5 * k, row, sizeof(row));
    }
    if (fits && !plan.blob.empty()) memcpy(blob, plan.blob.data(), plan.blob.size());
    for (size_t i = 0; i < plan.images.size(); i++) {
        const jda_exact_image &M = plan.images[i];
        int64_t *q = image + 10 * i;
        memset(q, 0, 10 * sizeof(int64_t));
        q[0] = M.kind;
        if (M.kind < 0) continue;
        q[1] = (int64_t)M.plane_at; q[2] = (int64_t)M.G.bytes; q[3] = (int64_t)(plan.o_scratch + M.plane_at + M.G.off[0]);
        for (int k = 0; k < 4; k++) q[4 + k] = M.rect ? M.mcu[k] : (k == 2 ? M.info.mcus_x : k == 3 ? M.info.mcus_y : 0);
        q[8] = jda_exact_tile_count(M.info, M.rect ? M.mcu : NULL); q[9] = jda_exact_tile_count(M.info, NULL);
    }
    free(block);
    return fits ? rc : -1;
}

// source: 0 a dense coefficient image, 1 a sparse one, 2 a resident baseline image; coefs == NULL with source 0 / 1: jda_progressive_prepare's.
// rects: n_rects x {x, y, w, h}; clips: n_rects x {width_px, rows} (NULL: the rectangle's own size); out: the rectangles' clipped pixels, dense,
// one after the other (min(w, width_px) * bpp bytes a row, min(h, rows) rows); twin_out: the WHOLE image from the row-major twin, dense.
// status: a code a rectangle (0, a JDA_* code of the plan, or a violation < 0: -10 .. -17 an access outside its allocation or misaligned,
// -20 a byte of the clip not written, -21 a load of a plane byte this rectangle's planes stage did not store, -22 a surface byte written twice,
// -23 one written outside the clip, -24 a plane byte written twice).  info[0]: planes tiles run in all, info[1]: colour tile records in all.
extern "C" int exactrectsim_run(const uint8_t *jpeg, int len, const int16_t *coefs, uint32_t n_blocks, int source, int pixel_type, int scale, int n_rects,
                                const int32_t *rects, const int32_t *clips, uint8_t *out, uint8_t *twin_out, int32_t *status, int32_t *info)
{
    int32_t err = 0, dummy[2];
    if (!info) info = dummy;
    info[0] = info[1] = 0;
    jda_image *bimg = NULL;
    jda_coef_image *cimg = NULL;
    jda_image_info I;
    uint16_t qzz[3][64];
    int32_t adobe = 0;
    memset(qzz, 0, sizeof(qzz));
    std::vector<int16_t> twin_coefs;
    RectIO io;
    jda_exact_source V;                                      // the source as the plan reads it (jda_exact_plan.h)
    memset(&V, 0, sizeof(V));
    std::vector<void *> owned;
    if (source == 2) {
        bimg = jda_prepare(jpeg, len, &err);
        if (!bimg) return err;
        I = *jda_image_get_info(bimg);
        uint16_t all[4][64];
        uint8_t dc_id[3], ac_id[3], q_id[3];
        jda_image_raw_quant(bimg, &all[0][0], &adobe);
        jda_image_component_ids(bimg, dc_id, ac_id, q_id);
        for (int c = 0; c < 3; c++) memcpy(qzz[c], all[q_id[c] & 3], sizeof(qzz[c]));
    } else {
        cimg = coefs ? jda_coef_image_from_coefficients(jpeg, len, coefs, n_blocks, &err) : jda_progressive_prepare(jpeg, len, &err);
        if (!cimg) return err;
        I = *jda_coef_image_get_info(cimg);
        uint8_t qid[3];
        jda_coef_image_raw_quant(cimg, &qzz[0][0], qid, &adobe);
    }
    uint32_t n_ok_all = 0;
    if (bimg) (void)jda_image_block_index(bimg, &n_ok_all);
    int rc = jda_exact_check(I, adobe, pixel_type, source == 2, n_ok_all);
    const bool gray = pixel_type == JDA_EIGHT_BIT_GRAYSCALE, luma_only = gray && I.ncomp == 3;
    jda_exact_geo G;
    if (rc == JDA_SUCCESS) rc = jda_exact_geometry_scaled(I, luma_only, scale, &G);
    if (rc != JDA_SUCCESS) { if (bimg) jda_image_free(bimg); if (cimg) jda_coef_image_free(cimg); return rc; }
    const int bpp = gray ? 1 : 4;
    const uint32_t nb = (uint32_t)(I.mcus_x * I.mcus_y * I.blocks_per_mcu);
    V.kind = (jda_exact_kind)source; V.info = I; V.adobe = adobe; V.colour = I.ncomp == 1 ? JDA_CS_GRAY : JDA_CS_YCBCR; V.n_mcus_ok = n_ok_all;
    memcpy(V.quant, qzz, sizeof(V.quant));
    if (source == 2) {
        uint32_t scan_len = 0, n_ok = 0, tb = 0;
        const uint8_t *scan = jda_image_scan(bimg, &scan_len);
        const uint32_t *index = jda_image_block_index(bimg, &n_ok);
        const uint8_t *tables = jda_image_tables(bimg, &tb);
        uint8_t *d_scan = dup(scan, scan_len, JDA_SCAN_PAD), *d_tab = dup(tables, tb);
        uint32_t *d_ix = dup(index, (size_t)nb + 1);
        int16_t *d_dc = dup(jda_image_block_dc(bimg), nb, nb & 1u);
        owned.insert(owned.end(), { (void *)d_scan, (void *)d_tab, (void *)d_ix, (void *)d_dc });
        io.add(d_scan, scan_len + JDA_SCAN_PAD, false); io.add(d_tab, tb, false); io.add(d_ix, ((size_t)nb + 1) * 4, false);
        io.add(d_dc, ((size_t)nb + (nb & 1u)) * 2, false);
        uint8_t dc_id[3], q_id[3];
        jda_image_component_ids(bimg, dc_id, V.ac_id, q_id);
        V.scan = d_scan; V.index = d_ix; V.dc = d_dc; V.tables = d_tab; V.scan_len = scan_len;
    } else {
        uint32_t nbc = 0, ne = 0;
        const int16_t *cf = jda_coef_image_coefficients(cimg, &nbc);
        twin_coefs.assign(cf, cf + (size_t)nbc * 64);
        const int16_t *quant = jda_coef_image_quant(cimg, NULL);
        if (source == 0) {
            uint8_t *blk = dup<uint8_t>(NULL, 0, JDA_CT_QUANT_BYTES + (size_t)nbc * 128);
            owned.push_back(blk);
            memcpy(blk, quant, JDA_CT_QUANT_BYTES); memcpy(blk + JDA_CT_QUANT_BYTES, cf, (size_t)nbc * 128);
            io.add(blk, JDA_CT_QUANT_BYTES + (size_t)nbc * 128, false);
            V.tables = blk; V.scan = blk + JDA_CT_QUANT_BYTES;
        } else {
            const uint32_t *first = NULL;
            const uint32_t *entries = jda_coef_image_sparse(cimg, &first, &ne);
            if (!entries) rc = JDA_UNSUPPORTED_FEATURE;
            else {
                const size_t fb = (((size_t)nbc + 1) * 4 + 15) & ~(size_t)15, eb = ((size_t)ne * 4 + 15) & ~(size_t)15;
                uint8_t *blk = dup<uint8_t>(NULL, 0, JDA_CT_QUANT_BYTES + fb + eb);
                owned.push_back(blk);
                memcpy(blk, quant, JDA_CT_QUANT_BYTES); memcpy(blk + JDA_CT_QUANT_BYTES, first, ((size_t)nbc + 1) * 4);
                if (ne) memcpy(blk + JDA_CT_QUANT_BYTES + fb, entries, (size_t)ne * 4);
                io.add(blk, JDA_CT_QUANT_BYTES + fb + eb, false);
                V.tables = blk; V.scan = blk + JDA_CT_QUANT_BYTES + fb;
            }
        }
    }
    // a rectangle = a call of one image, as the runtime makes it: the plan, a block for the blob and the scratch behind it, the records and
    // the two tile lists read back out of the block
    size_t at = 0;
    for (int k = 0; k < n_rects && rc == JDA_SUCCESS; k++) {
        const int32_t *rq = rects + 4 * k;
        int32_t inside[4];                                             // (judged before a surface is made for it; all zero is an empty rectangle here)
        status[k] = jda_exact_rect_plan(I, G, luma_only, rq, inside);
        if (status[k] != JDA_SUCCESS) continue;
        const int width_px = clips ? clips[2 * k] : rq[2], rows = clips ? clips[2 * k + 1] : rq[3];
        const int clip_w = width_px < rq[2] ? (width_px < 0 ? 0 : width_px) : rq[2], clip_h = rows < rq[3] ? (rows < 0 ? 0 : rows) : rq[3];
        const int pitch = (rq[2] * bpp + 15) & ~15;
        uint8_t *surf = dup<uint8_t>(NULL, 0, (size_t)pitch * rq[3]);
        jda_output O;
        O.pixels = surf; O.pitch_bytes = pitch; O.width_px = width_px; O.rows = rows;
        jda_exact_plan plan;
        const int prc = jda_exact_plan_build(1, &V, &O, &pixel_type, NULL, &scale, 0u, rq, &status[k], &plan);
        if (prc != JDA_SUCCESS) status[k] = prc;
        // the planes launch of the source's kind and, unless the clip is empty, the rectangle's colour launch
        const size_t nl = plan.launches.size();
        if (status[k] != JDA_SUCCESS || nl < 1u || nl > 2u || plan.launches[0].kind != V.kind || (nl == 2u && plan.launches[1].kind != JDA_EXK_COLOUR_RECT) ||
            (nl == 2u) != (clip_w > 0 && clip_h > 0)) {
            if (status[k] == JDA_SUCCESS) status[k] = -30;
            free(surf);
            continue;
        }
        uint8_t *block = dup<uint8_t>(NULL, 0, plan.o_scratch + plan.scratch);
        jda_exact_plan_place(&plan, block);
        memcpy(block, plan.blob.data(), plan.blob.size());
        memset(surf, 0x5A, (size_t)pitch * rq[3]);
        memset(block + plan.o_scratch, 0xA5, plan.scratch);
        io.scratch = block + plan.o_scratch; io.scratch_bytes = plan.scratch;
        io.written.assign(plan.scratch, 0);
        io.surface = surf; io.surface_bytes = (size_t)pitch * (size_t)clip_h;
        io.hits.assign(io.surface_bytes, 0);
        io.err = 0;
        io.add(block, plan.blob.size(), false);
        const jda_dev_desc D = *(const jda_dev_desc *)block;
        const jda_ex_desc *X = (const jda_ex_desc *)(block + plan.o_ex);
        const jda_exr_rec *R = (const jda_exr_rec *)(block + plan.o_rect);
        const jda_ex_src *esrc = (const jda_ex_src *)(block + plan.o_src);
        const jda_strip *t0 = (const jda_strip *)(block + plan.launches[0].off), *t1 = (const jda_strip *)(block + plan.launches[nl - 1u].off);
        const std::vector<jda_strip> tiles(t0, t0 + plan.launches[0].n_tiles), ctiles(t1, t1 + (nl == 2u ? plan.launches[1].n_tiles : 0u));
        for (const jda_strip &s : ctiles) info[1] += s.count ? 1 : 0;
        switch (D.mode) {
        case JDA_MODE_GRAY: run_rect<JDA_MODE_GRAY>(scale, source, D, X, R, esrc, tiles, ctiles, io, info); break;
        case JDA_MODE_444: run_rect<JDA_MODE_444>(scale, source, D, X, R, esrc, tiles, ctiles, io, info); break;
        case JDA_MODE_420: run_rect<JDA_MODE_420>(scale, source, D, X, R, esrc, tiles, ctiles, io, info); break;
        case JDA_MODE_422: run_rect<JDA_MODE_422>(scale, source, D, X, R, esrc, tiles, ctiles, io, info); break;
        default: run_rect<JDA_MODE_440>(scale, source, D, X, R, esrc, tiles, ctiles, io, info); break;
        }
        io.regions.pop_back();
        int st = io.err;
        for (size_t b = 0; b < io.hits.size() && st == 0; b++) {
            const size_t x = b % (size_t)pitch;
            if (io.hits[b] > 1) st = -22;
            else if (io.hits[b] && (int)x >= clip_w * bpp) st = -23;
            else if (!io.hits[b] && (int)x < clip_w * bpp) st = -20;
        }
        for (size_t b = 0; b < io.written.size() && st == 0; b++) if (io.written[b] > 1) st = -24;
        for (size_t b = (size_t)pitch * clip_h; b < (size_t)pitch * rq[3] && st == 0; b++) if (surf[b] != 0x5A) st = -23;
        status[k] = st;
        for (int y = 0; y < clip_h; y++) { memcpy(out + at, surf + (size_t)y * pitch, (size_t)clip_w * bpp); at += (size_t)clip_w * bpp; }
        free(surf);
        free(block);
    }
    io.surface = NULL; io.surface_bytes = 0; io.scratch = NULL; io.scratch_bytes = 0;
    if (rc == JDA_SUCCESS && twin_out && source != 2) {
        uint16_t qn[3][64];
        for (int c = 0; c < 3; c++) for (uint32_t z = 0; z < 64; z++) qn[c][jda_en_zigzag(z)] = qzz[c][z];
        if (scale == 1) {
            exact_twin::Image M;
            M.w = I.width; M.h = I.height; M.ncomp = I.ncomp; M.hs = (int)G.hs; M.vs = (int)G.vs; M.mcus_x = I.mcus_x; M.mcus_y = I.mcus_y;
            exact_twin::planes(M, twin_coefs.data(), qn);
            exact_twin::pixels(M, gray, twin_out, (size_t)I.width * bpp);
        } else {
            exact_scaled_twin::Image M;
            M.w = I.width; M.h = I.height; M.ncomp = I.ncomp; M.hs = (int)G.hs; M.vs = (int)G.vs; M.mcus_x = I.mcus_x; M.mcus_y = I.mcus_y; M.scale = scale;
            exact_scaled_twin::planes(M, twin_coefs.data(), qn);
            exact_scaled_twin::pixels(M, gray, twin_out, (size_t)M.ow * bpp);
        }
    }
    for (void *p : owned) free(p);
    if (bimg) jda_image_free(bimg);
    if (cimg) jda_coef_image_free(cimg);
    return rc;
}
