// tests/hostsim/coef_sparse_sim.cpp -- TEST INFRASTRUCTURE: jda_sparse_tiles (jpegdec_amd/csrc/jda_kernels.hip) lane by lane on the CPU.
//
// coefsparsesim_run packs a coefficient image into its sparse form (jda_coef_image_sparse), lays it out as jda_coef_upload_ex does --
// ONE allocation of exactly the uploaded size: quantisers | first[] | entries[] --, and runs every tile of the launch list through the
// kernel's OWN load phase (jda_cs_range / jda_cs_zero / jda_cs_scatter of jda_device_core.h) the way a wavefront runs it: the 64 lanes one
// after the other through a phase before any lane starts the next, over a byte array that stands for the wavefront's share of the LDS,
// poisoned before every tile.  Every global load goes through an IO policy that holds it to that allocation and to its alignment (16
// bytes for a vector, 4 for a word).  Behind the load phase the slots and chunk words are compared with those of the dense load phase
// (jda_ct_load over the dense coefficients, in a second, equally poisoned array); then the stages behind it run on the sparse one's LDS and
// write the pixels.  Not part of libjpegdec_amd.so; nothing in the product calls it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_device_core.h"
#include "../../jpegdec_amd/csrc/jda_plan.h"

extern "C" int jda_coef_image_sparse_status(const jda_coef_image *img);

namespace {
struct SparseIO {
    const uint8_t *base; size_t bytes;
    int err;
    bool inside(const uint8_t *p, size_t n) const { return p >= base && (size_t)(p - base) + n <= bytes && ((size_t)(p - base) & (n - 1)) == 0; }
    void ld128(const uint8_t *b, uint32_t i, uint32_t *v)
    {
        const uint8_t *p = b + (size_t)i * 16u;
        if (!inside(p, 16)) { if (!err) err = -10; memset(v, 0, 16); return; }
        memcpy(v, p, 16);
    }
    uint32_t ld32u(const uint8_t *b, uint32_t i)
    {
        const uint8_t *p = b + (size_t)i * 4u;
        uint32_t v = 0;
        if (!inside(p, 4)) { if (!err) err = -11; return 0; }
        memcpy(&v, p, 4);
        return v;
    }
};
struct DenseIO {
    const uint8_t *coefs; size_t coef_bytes;
    int err;
    void ld128(const uint8_t *b, uint32_t i, uint32_t *v)
    {
        const uint8_t *p = b + (size_t)i * 16u;
        if (!(p >= coefs && (size_t)(p - coefs) + 16 <= coef_bytes && ((size_t)(p - coefs) & 15u) == 0)) { if (!err) err = -12; memset(v, 0, 16); return; }
        memcpy(v, p, 16);
    }
};

template <int MODE>
int run_tiles(const jda_dev_desc &D, const jda_dev_desc &Ddense, const std::vector<jda_strip> &tiles, SparseIO &io, DenseIO &dio, bool pixels, int32_t *info)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    std::vector<uint64_t> store((jda_ct_layout<MODE>::WAVE_BYTES + 7) / 8), store2((jda_ct_layout<MODE>::WAVE_BYTES + 7) / 8);
    uint8_t *tab = (uint8_t *)store.data(), *wl = tab + JDA_CT_TAB_BYTES;
    uint8_t *wl2 = (uint8_t *)store2.data() + JDA_CT_TAB_BYTES;
    int32_t ti = -1;
    for (const jda_strip &S : tiles) {
        if (S.count == 0) continue;
        ti++;
        memset(tab, 0xA5, jda_ct_layout<MODE>::WAVE_BYTES);
        memset(store2.data(), 0xA5, jda_ct_layout<MODE>::WAVE_BYTES);
        jda_tile_ctx C;
        C.first_mcu = S.mcu_y * D.mcus_x + S.mcu_x0; C.count = S.count; C.first_block = C.first_mcu * (uint32_t)T::NBLK;
        C.win_lo = C.win_len = C.win_need = 0;
        const uint32_t nb = C.count * (uint32_t)T::NBLK;
        uint32_t e0 = 0, e1 = 0;
        jda_cs_range<MODE>(io, D, C, &e0, &e1);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_tables(io, D.tables, t, tab);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_cs_zero<MODE>(C, t, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_cs_scatter<MODE>(io, D, C, t, e0, e1, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_load<MODE>(dio, Ddense, C, t, wl2);
        info[0]++;
        if ((int32_t)(e1 - e0) > info[2]) info[2] = (int32_t)(e1 - e0);
        if (io.err || dio.err) return io.err ? io.err : dio.err;
        for (uint32_t b = 0; b < nb; b++)
            if (memcmp(wl + L::COEF_OFF + b * JDA_COEF_STRIDE, wl2 + L::COEF_OFF + b * JDA_COEF_STRIDE, 128)) { info[1] = ti; return -20; }
        if (memcmp(wl + L::COLLIST_OFF, wl2 + L::COLLIST_OFF, (size_t)nb * 16u)) { info[1] = ti; return -21; }
        if (!pixels) continue;
        jda_lane_pre LP[JDA_TILE_THREADS];
        uint32_t flags[JDA_TILE_THREADS];
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_lane_prepare<MODE>(LP[t], D, t);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) flags[t] = jda_ct_flags<MODE>(D, C, LP[t], t, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_p1_lists<MODE>(D, LP[t], t, flags[t], flags, tab, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_p2_columns<MODE, false>(D, t, tab, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_p3_rows<MODE>(D, t, tab, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) {
            jda_p4_pre P4;
            jda_p4_prepare<MODE>(P4, D, t);
            jda_p4_output<MODE>(D, S, C, t, wl, P4);
        }
    }
    return 0;
}
} // namespace

// tiles with something to decode in the launch list of an image under `rect` ({mx0, my0, mx1, my1} in MCUs, NULL: the whole image):
// the list jda_coef_decode_surfaces_rect plans (jda_append_strips); first_xy (may be NULL): mcu_x0 / mcu_y of its first such tile
extern "C" int coefsparsesim_plan_tiles(uint32_t mcus_x, uint32_t mcus_y, int mode, const int32_t *rect, int32_t *first_xy)
{
    std::vector<jda_strip> tiles;
    jda_append_strips(tiles, 0, mcus_x, mcus_y, mode, 0, rect);
    int n = 0;
    for (const jda_strip &s : tiles) {
        if (!s.count) continue;
        if (s.mcu_x0 + (uint32_t)s.count > mcus_x || s.mcu_y >= mcus_y) return -1;      // (a tile outside the image)
        if (!n && first_xy) { first_xy[0] = s.mcu_x0; first_xy[1] = s.mcu_y; }
        n++;
    }
    return n;
}

// coefs == NULL: every scan of the (progressive) file decoded by jda_progressive_prepare.  out == NULL: the load phases only.
// info[0]: tiles run, info[1]: the tile whose slots (-20) / chunk words (-21) differ, info[2]: the longest entry range of a tile.
// Returns 0, a JDA_* error (> 0) or a violation (< 0: -10 / -11 a vector / word load outside the allocation or misaligned, -12 the same of
// the dense load, -20 / -21, -30 the sparse form re-expanded is not the dense one).
extern "C" int coefsparsesim_run(const uint8_t *jpeg, int len, const int16_t *coefs, uint32_t n_blocks, int pixel_type, int options, const int32_t *rect,
                                 uint8_t *out, int pitch, int width_px, int rows, int32_t *info)
{
    int32_t err = 0, dummy[3];
    if (!info) info = dummy;
    info[0] = 0; info[1] = -1; info[2] = 0;
    jda_coef_image *img = coefs ? jda_coef_image_from_coefficients(jpeg, len, coefs, n_blocks, &err) : jda_progressive_prepare(jpeg, len, &err);
    if (!img) return err;
    jda_image_info I = *jda_coef_image_get_info(img);
    I.jpeg_type = 0;
    uint8_t q_id[3];
    const int16_t *quant = jda_coef_image_quant(img, q_id);
    uint32_t nb = 0, ne = 0;
    const int16_t *cf = jda_coef_image_coefficients(img, &nb);
    const uint32_t *first = NULL;
    const uint32_t *entries = jda_coef_image_sparse(img, &first, &ne);
    if (!entries) { const int st = jda_coef_image_sparse_status(img); jda_coef_image_free(img); return st; }
    // re-expand
    {
        std::vector<int16_t> back((size_t)nb * 64, 0);
        bool ok = first[nb] == ne;
        for (uint32_t g = 0; g < nb && ok; g++)
            for (uint32_t k = first[g]; k < first[g + 1]; k++) {
                const uint32_t e = entries[k];
                if ((e >> 22) != (g & 1023u) || (uint16_t)e == 0 || (k > first[g] && ((entries[k - 1] >> 16) & 63u) >= ((e >> 16) & 63u))) { ok = false; break; }
                back[(size_t)g * 64 + ((e >> 16) & 63u)] = (int16_t)(uint16_t)e;
            }
        if (!ok || memcmp(back.data(), cf, (size_t)nb * 128)) { jda_coef_image_free(img); return -30; }
    }
    const size_t first_bytes = (((size_t)nb + 1) * 4 + 15) & ~(size_t)15, entry_bytes = ((size_t)ne * 4 + 15) & ~(size_t)15;
    const size_t bytes = JDA_CT_QUANT_BYTES + first_bytes + entry_bytes;
    uint8_t *blk = NULL;
    if (posix_memalign((void **)&blk, 16, bytes) != 0) { jda_coef_image_free(img); return JDA_ERROR_MEMORY; }
    memcpy(blk, quant, JDA_CT_QUANT_BYTES);
    memcpy(blk + JDA_CT_QUANT_BYTES, first, first_bytes);
    if (entry_bytes) memcpy(blk + JDA_CT_QUANT_BYTES + first_bytes, entries, entry_bytes);

    int pt = pixel_type;
    const int opt = options & ~JDA_PROGRESSIVE_FULL;
    int rc = 0;
    if (pt < 0 || pt > JDA_EIGHT_BIT_GRAYSCALE) rc = JDA_INVALID_PARAMETER;
    if (!rc && (opt & (JDA_SCALE_HALF | JDA_SCALE_QUARTER | JDA_SCALE_EIGHTH))) rc = JDA_UNSUPPORTED_FEATURE;
    int bpp = 0, ow, oh, cw = 0, ch = 0;
    if (!rc) {
        if ((opt & JDA_LUMA_ONLY) && pt < JDA_EIGHT_BIT_GRAYSCALE) pt = JDA_EIGHT_BIT_GRAYSCALE;
        rc = jda_output_geometry(&I, pt, opt, &bpp, &ow, &oh, &cw, &ch);
    }
    if (!rc) {
        jda_dev_desc D;
        memset(&D, 0, sizeof(D));
        D.mode = (uint8_t)jda_mode_of(I); D.ncomp = (uint8_t)I.ncomp;
        D.pixel_type = (uint8_t)((D.mode == JDA_MODE_GRAY && pt == JDA_RGB8888) ? JDA_RGB565_BIG_ENDIAN : pt);
        D.gray_from_color = (uint8_t)(D.mode != JDA_MODE_GRAY && pt == JDA_EIGHT_BIT_GRAYSCALE);
        memcpy(D.q_id, q_id, 3);
        D.mcus_x = (uint32_t)I.mcus_x; D.mcus_y = (uint32_t)I.mcus_y; D.n_mcus_ok = D.mcus_x * D.mcus_y;
        D.out = out; D.out_pitch = (uint32_t)pitch;
        D.out_w = (uint32_t)(width_px < cw ? width_px : cw); D.out_rows = (uint32_t)(rows < ch ? rows : ch);
        D.tables = blk; D.scan = blk + JDA_CT_QUANT_BYTES + first_bytes;
        jda_dev_desc Dd = D;
        Dd.tables = (const uint8_t *)quant; Dd.scan = (const uint8_t *)cf;
        if (out && (pitch < (int)D.out_w * bpp || (pitch & 15) || ((uintptr_t)out & 15))) rc = JDA_INVALID_PARAMETER;
        else {
            std::vector<jda_strip> tiles;
            jda_append_strips(tiles, 0, D.mcus_x, D.mcus_y, D.mode, 0, rect);
            SparseIO io;
            io.base = blk; io.bytes = bytes; io.err = 0;
            DenseIO dio;
            dio.coefs = (const uint8_t *)cf; dio.coef_bytes = (size_t)nb * JDA_CT_BLOCK_BYTES; dio.err = 0;
            switch (D.mode) {
            case JDA_MODE_GRAY: rc = run_tiles<JDA_MODE_GRAY>(D, Dd, tiles, io, dio, out != NULL, info); break;
            case JDA_MODE_444: rc = run_tiles<JDA_MODE_444>(D, Dd, tiles, io, dio, out != NULL, info); break;
            case JDA_MODE_420: rc = run_tiles<JDA_MODE_420>(D, Dd, tiles, io, dio, out != NULL, info); break;
            case JDA_MODE_422: rc = run_tiles<JDA_MODE_422>(D, Dd, tiles, io, dio, out != NULL, info); break;
            default: rc = run_tiles<JDA_MODE_440>(D, Dd, tiles, io, dio, out != NULL, info); break;
            }
        }
    }
    free(blk);
    jda_coef_image_free(img);
    return rc;
}
