// tests/hostsim/exact_scaled_sim.cpp -- TEST INFRASTRUCTURE: the scaled libjpeg-exact decode's kernels (jda_exact_planes_scaled of all three
// load phases and scales, jda_exact_colour_scaled of jpegdec_amd/csrc/jda_kernels.hip) lane by lane on the CPU, over the plan the runtime
// makes (jda_exact_plan.h).
//
// As exact_sim.cpp: the file laid out as the runtime has it resident, every tile of the launch list through the kernels' OWN per-lane
// functions (jda_exs_* of jda_device_core.h), the 64 lanes one after the other through a phase before any lane starts the next -- load,
// block (what a lane keeps in registers between the phases is kept per lane here), stage, store --, over a byte array that stands for the
// wavefront's share of the LDS, poisoned before every tile.  Every global access goes through an IO policy that holds it to its
// allocation and its alignment; loads from the scan are counted (the DC-only load phase reads none); the stores to the surface and to the
// planes are counted byte by byte, so that a byte written twice, a visible byte not written or a byte outside the clip is a violation.
// The planes and the pixels are then compared with the row-major twin (exact_scaled_twin.h).
// Not part of libjpegdec_amd.so; nothing in the product calls it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_exact_plan.h"
#include "exact_scaled_twin.h"

extern "C" void jda_image_raw_quant(const jda_image *img, uint16_t *quant_zz, int32_t *adobe);
extern "C" void jda_coef_image_raw_quant(const jda_coef_image *img, uint16_t *quant_zz, uint8_t *q_id, int32_t *adobe);

namespace {
struct Region { const uint8_t *base; size_t bytes; bool writable; };
struct ScaledIO {
    std::vector<Region> regions;
    uint8_t *surface; size_t surface_bytes;
    uint8_t *scratch; size_t scratch_bytes;
    const uint8_t *scan; size_t scan_bytes;
    std::vector<uint8_t> hits, plane_hits;                   // per byte of the surface / of the planes: stores that touched it
    int err;
    int64_t scan_loads;
    ScaledIO() : surface(NULL), surface_bytes(0), scratch(NULL), scratch_bytes(0), scan(NULL), scan_bytes(0), err(0), scan_loads(0) {}
    void add(const void *p, size_t n, bool w) { Region r = { (const uint8_t *)p, n, w }; regions.push_back(r); }
    bool inside(const void *q, size_t n, bool write)
    {
        const uint8_t *p = (const uint8_t *)q;
        if (((uintptr_t)p & (n - 1)) != 0) return false;
        if (!write && scan && p >= scan && p < scan + scan_bytes) scan_loads++;
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
            for (size_t k = 0; k < n; k++) if (plane_hits[(size_t)(p - scratch) + k] < 255) plane_hits[(size_t)(p - scratch) + k]++;
    }
    void st64(uint8_t *b, uint32_t off, uint32_t lo, uint32_t hi) { const uint32_t v[2] = { lo, hi }; store(b, off, v, 8); }
    void st128(uint8_t *b, uint32_t off, const uint32_t *w) { store(b, off, w, 16); }
    void st32(uint8_t *b, uint32_t off, uint32_t v) { store(b, off, &v, 4); }
    void st8(uint8_t *b, uint32_t off, uint32_t v) { const uint8_t c = (uint8_t)v; store(b, off, &c, 1); }
};

template <int MODE, int SCALE, int SOURCE>
void run_tiles_at(const jda_dev_desc &D, const jda_ex_desc *Xp, const jda_ex_src *src, const std::vector<jda_strip> &tiles, bool colour, ScaledIO &io, int16_t *keep, int32_t *info)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    typedef jda_exs_layout<MODE, SCALE> Z;
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
        if (SOURCE == 2) {
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_load_baseline<MODE, SCALE>(io, X, src, C, t, wl);
            // (what the twin decodes: the slots of the lanes that walked; a DC-only lane's coefficient is the index's DC value)
            for (uint32_t t = 0; keep && t < C.count * (uint32_t)T::NBLK; t++) {
                uint32_t c, bx, by;
                jda_exs_place<MODE>(t, &c, &bx, &by);
                int16_t *dst = keep + (size_t)(C.first_block + t) * 64;
                if ((c ? (int)Z::SS_C : (int)Z::SS_Y) == 1 || (c && X.luma_only)) { memset(dst, 0, 128); dst[0] = src->S.blk_dc[C.first_block + t]; }
                else memcpy(dst, wl + L::COEF_OFF + t * JDA_COEF_STRIDE, 128);
            }
        } else if (SOURCE == 1) {
            uint32_t e0 = 0, e1 = 0;
            jda_cs_range<MODE>(io, D, C, &e0, &e1);
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_cs_zero<MODE>(C, t, wl);
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_cs_scatter<MODE>(io, D, C, t, e0, e1, wl);
        } else {
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_load<MODE>(io, D, C, t, wl);
        }
        uint32_t px[JDA_TILE_THREADS][16];
        memset(px, 0xA5, sizeof(px));
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_block<MODE, SCALE, SOURCE>(io, X, src, C, t, wl, qt, px[t]);
        memset(wl + L::COEF_OFF, 0x5A, L::BLOCKS * JDA_COEF_STRIDE);     // (the slots are dead: whatever the store phase reads of them it must not store)
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_stage<MODE, SCALE>(X, S, C, t, wl + L::COEF_OFF, px[t]);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_store<MODE, SCALE>(io, X, S, t, wl + L::COEF_OFF);
        info[0]++;
    }
    if (colour)
        for (const jda_strip &S : tiles) {
            if (S.count == 0) continue;
            for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_exs_colour_tile<MODE>(io, X, S, t);
        }
}
template <int MODE, int SCALE>
void run_tiles_src(const jda_dev_desc &D, const jda_ex_desc *Xp, const jda_ex_src *src, const std::vector<jda_strip> &tiles, int source, bool colour, ScaledIO &io, int16_t *keep,
                   int32_t *info)
{
    if (source == 2) run_tiles_at<MODE, SCALE, 2>(D, Xp, src, tiles, colour, io, keep, info);
    else if (source == 1) run_tiles_at<MODE, SCALE, 1>(D, Xp, src, tiles, colour, io, keep, info);
    else run_tiles_at<MODE, SCALE, 0>(D, Xp, src, tiles, colour, io, keep, info);
}
template <int MODE>
void run_tiles(int scale, const jda_dev_desc &D, const jda_ex_desc *Xp, const jda_ex_src *src, const std::vector<jda_strip> &tiles, int source, bool colour, ScaledIO &io,
               int16_t *keep, int32_t *info)
{
    if (scale == 2) run_tiles_src<MODE, 2>(D, Xp, src, tiles, source, colour, io, keep, info);
    else if (scale == 4) run_tiles_src<MODE, 4>(D, Xp, src, tiles, source, colour, io, keep, info);
    else run_tiles_src<MODE, 8>(D, Xp, src, tiles, source, colour, io, keep, info);
}
template <class T> T *dup(const T *p, size_t n, size_t extra = 0)      // an allocation of exactly n (+ extra zero) elements' bytes, 16-byte aligned
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

// the plan alone: out[0..15] = scale, ss_y, ss_c, w, h, cw, ch, up, pitch_y, pitch_c, rows_y, rows_c, off[1], off[2], bytes, tiles of the launch list;
// returns jda_exact_check's / jda_exact_geometry_scaled's code
extern "C" int exactscaledsim_plan(int width, int height, int ncomp, int subsample, int adobe, int pixel_type, int luma_only, int scale, int64_t *out)
{
    const jda_image_info I = info_of(width, height, ncomp, subsample);
    int rc = jda_exact_check(I, adobe, pixel_type, 0, 0);
    if (rc != JDA_SUCCESS) return rc;
    jda_exact_geo G;
    rc = jda_exact_geometry_scaled(I, luma_only != 0, scale, &G);
    if (rc != JDA_SUCCESS) return rc;
    std::vector<jda_strip> tiles;
    jda_append_strips(tiles, 0, (uint32_t)I.mcus_x, (uint32_t)I.mcus_y, jda_mode_of(I));
    int64_t n = 0;
    for (const jda_strip &s : tiles) n += s.count ? 1 : 0;
    const int64_t v[16] = { G.scale, G.ss_y, G.ss_c, G.w, G.h, G.cw, G.ch, G.up, G.pitch_y, G.pitch_c, G.rows_y, G.rows_c, (int64_t)G.off[1], (int64_t)G.off[2], (int64_t)G.bytes, n };
    memcpy(out, v, sizeof(v));
    return JDA_SUCCESS;
}
// jda_exact_draft_scale's rule
extern "C" int exactscaledsim_draft(int width, int height, int req_w, int req_h)
{
    const jda_image_info I = info_of(width, height, 3, 0x11);
    return jda_exact_draft(I, req_w, req_h);
}

// As exactsim_run, at scale 2, 4 or 8.  out: the surface; twin_out: oh x ow pixels of the same kind from the row-major twin, dense; planes_out /
// twin_planes: Y | Cb | Cr at their own scaled extents, dense.  info[0]: tiles run, info[1] / info[2]: the twin's extremes of the pre-limit
// results, info[3]: bytes of the surface written more than once, info[4]: written bytes outside the clip, info[5]: loads from the scan,
// info[6]: bytes of the planes written more than once, info[7]: bytes of a plane's MCU grid no lane wrote.
// Returns 0, a JDA_* code (> 0) or a violation (< 0: -10 .. -17 an access outside its allocation or misaligned, -20 a visible byte not written).
extern "C" int exactscaledsim_run(const uint8_t *jpeg, int len, const int16_t *coefs, uint32_t n_blocks, int source, int pixel_type, int scale, uint8_t *out, int pitch,
                                  int width_px, int rows, uint8_t *twin_out, uint8_t *planes_out, uint8_t *twin_planes, int32_t *info)
{
    int32_t err = 0, dummy[8];
    if (!info) info = dummy;
    memset(info, 0, 8 * sizeof(int32_t));
    if (scale != 2 && scale != 4 && scale != 8) return JDA_INVALID_PARAMETER;
    jda_image *bimg = NULL;
    jda_coef_image *cimg = NULL;
    jda_image_info I;
    uint16_t qzz[3][64];
    int32_t adobe = 0;
    memset(qzz, 0, sizeof(qzz));
    std::vector<int16_t> twin_coefs;
    ScaledIO io;
    jda_dev_desc D;
    memset(&D, 0, sizeof(D));
    std::vector<void *> owned;
    jda_ex_src *esrc = NULL;
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
    const bool gray = pixel_type == JDA_EIGHT_BIT_GRAYSCALE, luma_only = gray && I.ncomp == 3 && !planes_out;
    jda_exact_geo G;
    if (rc == JDA_SUCCESS) rc = jda_exact_geometry_scaled(I, luma_only, scale, &G);
    const int bpp = gray ? 1 : 4;
    const int clip_w = width_px < (int)G.w ? width_px : (int)G.w, clip_h = rows < (int)G.h ? rows : (int)G.h;
    if (rc == JDA_SUCCESS && out && (pitch < clip_w * bpp || (pitch & 15) || ((uintptr_t)out & 15) || width_px < 0 || rows < 0)) rc = JDA_INVALID_PARAMETER;
    if (rc != JDA_SUCCESS) { if (bimg) jda_image_free(bimg); if (cimg) jda_coef_image_free(cimg); return rc; }
    const uint32_t nb = (uint32_t)(I.mcus_x * I.mcus_y * I.blocks_per_mcu);
    D.mode = (uint8_t)jda_mode_of(I); D.ncomp = (uint8_t)I.ncomp; D.mcus_x = (uint32_t)I.mcus_x; D.mcus_y = (uint32_t)I.mcus_y;
    uint8_t *scratch = dup<uint8_t>(NULL, 0, G.bytes);
    owned.push_back(scratch);
    memset(scratch, 0xA5, G.bytes);
    io.add(scratch, G.bytes, true);
    io.scratch = scratch; io.scratch_bytes = G.bytes; io.plane_hits.assign(G.bytes, 0);
    if (source == 2) {
        uint32_t scan_len = 0, n_ok = 0, tb = 0;
        const uint8_t *scan = jda_image_scan(bimg, &scan_len);
        const uint32_t *index = jda_image_block_index(bimg, &n_ok);
        const uint8_t *tables = jda_image_tables(bimg, &tb);
        uint8_t *d_scan = dup(scan, scan_len, JDA_SCAN_PAD), *d_tab = dup(tables, tb);
        uint32_t *d_ix = dup(index, (size_t)nb + 1);
        int16_t *d_dc = dup(jda_image_block_dc(bimg), nb, nb & 1u);
        esrc = dup<jda_ex_src>(NULL, 0, 1);
        owned.insert(owned.end(), { (void *)d_scan, (void *)d_tab, (void *)d_ix, (void *)d_dc, (void *)esrc });
        io.add(d_scan, scan_len + JDA_SCAN_PAD, false); io.add(d_tab, tb, false); io.add(d_ix, ((size_t)nb + 1) * 4, false);
        io.add(d_dc, ((size_t)nb + (nb & 1u)) * 2, false); io.add(esrc, sizeof(jda_ex_src), false);
        io.scan = d_scan; io.scan_bytes = scan_len + JDA_SCAN_PAD;
        uint8_t dc_id[3], ac_id[3], q_id[3];
        jda_image_component_ids(bimg, dc_id, ac_id, q_id);
        esrc->S.scan = d_scan; esrc->S.blk_index = d_ix; esrc->S.blk_dc = d_dc; esrc->S.tables = d_tab; esrc->S.scan_len = scan_len; esrc->S.kind = JDA_RC_IMAGE;
        for (int c = 0; c < 3; c++) esrc->S.ac_id[c] = ac_id[c];
        esrc->bpm = (uint32_t)I.blocks_per_mcu; esrc->nluma = I.ncomp == 3 ? esrc->bpm - 2u : 1u;
        twin_coefs.assign((size_t)nb * 64, 0);
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
            D.tables = blk; D.scan = blk + JDA_CT_QUANT_BYTES;
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
                D.tables = blk; D.scan = blk + JDA_CT_QUANT_BYTES + fb;
            }
        }
    }
    jda_ex_desc *X = dup<jda_ex_desc>(NULL, 0, 1);
    owned.push_back(X);
    io.add(X, sizeof(jda_ex_desc), false);
    if (rc == JDA_SUCCESS) {
        jda_output O;
        O.pixels = out; O.pitch_bytes = pitch; O.width_px = width_px; O.rows = rows;
        jda_exact_fill_scaled(*X, I, qzz, G, scratch, out ? &O : NULL, pixel_type, luma_only);
        if (out) {
            io.surface = out; io.surface_bytes = (size_t)pitch * (size_t)(clip_h > 0 ? clip_h : 0);      // (the rows the clip leaves: a store behind them is outside every allocation)
            io.hits.assign(io.surface_bytes, 0);
            io.add(out, io.surface_bytes, true);
        }
        std::vector<jda_strip> tiles;
        jda_append_strips(tiles, 0, D.mcus_x, D.mcus_y, D.mode);
        const bool col = out != NULL;
        int16_t *keep = source == 2 ? twin_coefs.data() : NULL;
        switch (D.mode) {
        case JDA_MODE_GRAY: run_tiles<JDA_MODE_GRAY>(scale, D, X, esrc, tiles, source, col, io, keep, info); break;
        case JDA_MODE_444: run_tiles<JDA_MODE_444>(scale, D, X, esrc, tiles, source, col, io, keep, info); break;
        case JDA_MODE_420: run_tiles<JDA_MODE_420>(scale, D, X, esrc, tiles, source, col, io, keep, info); break;
        case JDA_MODE_422: run_tiles<JDA_MODE_422>(scale, D, X, esrc, tiles, source, col, io, keep, info); break;
        default: run_tiles<JDA_MODE_440>(scale, D, X, esrc, tiles, source, col, io, keep, info); break;
        }
        rc = io.err;
        info[5] = (int32_t)io.scan_loads;
        for (size_t k = 0; k < io.hits.size(); k++) {
            const size_t y = k / (size_t)pitch, x = k % (size_t)pitch;
            if (io.hits[k] > 1) info[3]++;
            if (io.hits[k] && ((int)y >= clip_h || (int)x >= clip_w * bpp)) info[4]++;
            if (!io.hits[k] && (int)y < clip_h && (int)x < clip_w * bpp && rc == 0) rc = -20;      // a visible byte no lane wrote
        }
        // the planes: every byte of a decoded component's MCU grid exactly once, no other byte of the scratch
        for (int c = 0; c < (I.ncomp == 3 && !luma_only ? 3 : 1); c++) {
            const uint32_t ss = c ? G.ss_c : G.ss_y, pw = (uint32_t)I.mcus_x * ss * (c ? 1u : G.hs), pp = c ? G.pitch_c : G.pitch_y, pr = c ? G.rows_c : G.rows_y;
            for (uint32_t y = 0; y < pr; y++)
                for (uint32_t x = 0; x < pp; x++) {
                    uint8_t &h = io.plane_hits[G.off[c] + (size_t)y * pp + x];
                    if (x < pw && h == 0) info[7]++;
                    if (x < pw ? h > 1 : h > 0) info[6]++;
                    h = 0;
                }
        }
        for (size_t k = 0; k < io.plane_hits.size(); k++) if (io.plane_hits[k]) info[6]++;
        exact_scaled_twin::Image M;
        M.w = I.width; M.h = I.height; M.ncomp = I.ncomp; M.hs = (int)G.hs; M.vs = (int)G.vs; M.mcus_x = I.mcus_x; M.mcus_y = I.mcus_y; M.scale = scale;
        uint16_t qn[3][64];
        for (int c = 0; c < 3; c++) for (uint32_t z = 0; z < 64; z++) qn[c][jda_en_zigzag(z)] = qzz[c][z];
        exact_scaled_twin::planes(M, twin_coefs.data(), qn);
        info[1] = M.lo; info[2] = M.hi;
        if (twin_out) exact_scaled_twin::pixels(M, gray, twin_out, (size_t)M.ow * bpp);
        size_t at = 0;
        for (int c = 0; c < I.ncomp; c++) {
            for (int y = 0; y < M.eh[c]; y++) {
                if (twin_planes) memcpy(twin_planes + at, M.plane[c].data() + (size_t)y * M.pitch[c], M.ew[c]);
                if (planes_out && !(c && luma_only)) memcpy(planes_out + at, scratch + G.off[c] + (size_t)y * (c ? G.pitch_c : G.pitch_y), M.ew[c]);
                at += M.ew[c];
            }
        }
        if ((int)G.w != M.ow || (int)G.h != M.oh || (I.ncomp == 3 && ((int)G.cw != M.ew[1] || (int)G.ch != M.eh[1] || (int)G.up != M.up || (int)G.ss_c != M.ss[1])) ||
            (int)G.ss_y != M.ss[0]) { if (rc == 0) rc = -30; }      // the plan's geometry is the twin's
    }
    for (void *p : owned) free(p);
    if (bimg) jda_image_free(bimg);
    if (cimg) jda_coef_image_free(cimg);
    return rc;
}
