// tests/hostsim/coef_sim.cpp -- TEST INFRASTRUCTURE: jda_coef_tiles (jpegdec_amd/csrc/jda_kernels.hip) lane by lane on the CPU.
//
// coefsim_decode runs a coefficient image through the kernel's OWN per-lane code (jda_ct_* and the decode kernel's list, column, row
// and colour stages of jda_device_core.h) the way a wavefront runs it: tile after tile of the launch list jda_coef_decode_surfaces
// builds (jda_append_strips), the 64 lanes one after the other through a phase before any lane starts the next (the wave-local
// fences), over byte arrays that stand for the wavefront's share of the LDS -- poisoned before every tile, as LDS is never cleared.
// The loads go through an IO policy that holds them to the coefficient array: 16-byte aligned, inside it.  mode 1 is the row-major
// twin that knows no schedule (coef_twin.h).  Not part of libjpegdec_amd.so; nothing in the product calls it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_device_core.h"
#include "../../jpegdec_amd/csrc/jda_plan.h"
#include "coef_twin.h"

namespace {
struct SimIO {
    const uint8_t *coefs; size_t coef_bytes;
    const uint8_t *quant;
    int err;
    void ld128(const uint8_t *base, uint32_t i, uint32_t *v)
    {
        const uint8_t *p = base + (size_t)i * 16u;
        const bool in_coefs = p >= coefs && (size_t)(p - coefs) + 16 <= coef_bytes && ((size_t)(p - coefs) & 15u) == 0;
        const bool in_quant = p >= quant && (size_t)(p - quant) + 16 <= JDA_CT_QUANT_BYTES && ((size_t)(p - quant) & 15u) == 0;
        if (!in_coefs && !in_quant) { if (!err) err = -10; memset(v, 0, 16); return; }
        memcpy(v, p, 16);
    }
};

template <int MODE>
int run_tiles(const jda_dev_desc &D, const std::vector<jda_strip> &tiles, SimIO &io, uint32_t *flags_out)
{
    typedef jda_mode_traits<MODE> T;
    std::vector<uint64_t> store((jda_ct_layout<MODE>::WAVE_BYTES + 7) / 8);
    uint8_t *tab = (uint8_t *)store.data(), *wl = tab + JDA_CT_TAB_BYTES;
    for (const jda_strip &S : tiles) {
        if (S.count == 0) continue;
        memset(tab, 0xA5, jda_ct_layout<MODE>::WAVE_BYTES);
        jda_tile_ctx C;
        C.first_mcu = S.mcu_y * D.mcus_x + S.mcu_x0; C.count = S.count; C.first_block = C.first_mcu * (uint32_t)T::NBLK;
        C.win_lo = C.win_len = C.win_need = 0;
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_tables(io, D.tables, t, tab);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_load<MODE>(io, D, C, t, wl);
        jda_lane_pre LP[JDA_TILE_THREADS];
        uint32_t flags[JDA_TILE_THREADS];
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_ct_lane_prepare<MODE>(LP[t], D, t);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) flags[t] = jda_ct_flags<MODE>(D, C, LP[t], t, wl);
        if (flags_out) for (uint32_t t = 0; t < C.count * (uint32_t)T::NBLK; t++) flags_out[C.first_block + t] = flags[t];
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_p1_lists<MODE>(D, LP[t], t, flags[t], flags, tab, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_p2_columns<MODE, false>(D, t, tab, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) jda_p3_rows<MODE>(D, t, tab, wl);
        for (uint32_t t = 0; t < JDA_TILE_THREADS; t++) {
            jda_p4_pre P4;
            jda_p4_prepare<MODE>(P4, D, t);
            jda_p4_output<MODE>(D, S, C, t, wl, P4);
        }
    }
    return io.err;
}
} // namespace

// mode 0: the kernel's lane schedule; 1: the row-major twin.  out: pitch x rows bytes (pitch a multiple of 16, 16-byte aligned);
// flags_out (may be NULL; mode 0): n_blocks words, a block's u16MCUFlags as the load phase formed them (0xffffffff: not listed).
// Returns 0, a JDA_* error (> 0) or a policy violation (< 0).
extern "C" int coefsim_decode(const uint8_t *jpeg, int len, const int16_t *coefs, uint32_t n_blocks, int pixel_type, int options, int mode,
                              uint8_t *out, int pitch, int width_px, int rows, uint32_t *flags_out)
{
    int32_t err = 0;
    jda_coef_image *img = jda_coef_image_from_coefficients(jpeg, len, coefs, n_blocks, &err);
    if (!img) return err;
    jda_image_info I = *jda_coef_image_get_info(img);
    I.jpeg_type = 0;
    uint8_t q_id[3];
    const int16_t *quant = jda_coef_image_quant(img, q_id);
    const int16_t *cf = jda_coef_image_coefficients(img, NULL);
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
        D.tables = (const uint8_t *)quant; D.scan = (const uint8_t *)cf;
        if (pitch < (int)D.out_w * bpp || (pitch & 15) || ((uintptr_t)out & 15)) rc = JDA_INVALID_PARAMETER;
        else if (mode == 1) rc = coef_twin_decode(D.mode, D.mcus_x, D.mcus_y, q_id, quant, cf, D.pixel_type, out, D.out_pitch, D.out_w, D.out_rows);
        else {
            std::vector<jda_strip> tiles;
            jda_append_strips(tiles, 0, D.mcus_x, D.mcus_y, D.mode);
            SimIO io;
            io.coefs = (const uint8_t *)cf; io.coef_bytes = (size_t)n_blocks * JDA_CT_BLOCK_BYTES; io.quant = (const uint8_t *)quant; io.err = 0;
            if (flags_out) memset(flags_out, 0xff, (size_t)n_blocks * 4);
            switch (D.mode) {
            case JDA_MODE_GRAY: rc = run_tiles<JDA_MODE_GRAY>(D, tiles, io, flags_out); break;
            case JDA_MODE_444: rc = run_tiles<JDA_MODE_444>(D, tiles, io, flags_out); break;
            case JDA_MODE_420: rc = run_tiles<JDA_MODE_420>(D, tiles, io, flags_out); break;
            case JDA_MODE_422: rc = run_tiles<JDA_MODE_422>(D, tiles, io, flags_out); break;
            default: rc = run_tiles<JDA_MODE_440>(D, tiles, io, flags_out); break;
            }
        }
    }
    jda_coef_image_free(img);
    return rc;
}
