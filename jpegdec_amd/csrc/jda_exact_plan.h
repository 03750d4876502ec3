// jda_exact_plan.h -- the host side of the libjpeg-exact decode (jda_exact_decode_surfaces / _planes): what is refused,
// the component planes of an image in the call's scratch, and its record for the kernels.  Host work only, no HIP: the runtime and
// tests/hostsim/exact_sim.cpp share it.
#ifndef JDA_EXACT_PLAN_H
#define JDA_EXACT_PLAN_H

#include <string.h>

#include "jda_device_core.h"
#include "jda_plan.h"

// What the exact road takes: a gray or YCbCr file as libjpeg would read it (no Adobe APP14 segment: its transform flag changes how the
// components are read), an RGB8888 or 8-bit gray surface.  baseline_image: the source is a resident baseline image, whose pre-scan
// validated n_mcus_ok MCUs -- all of them, or the reader would walk index entries nothing stands behind (JDA_DECODE_ERROR, the recode's
// rule) -- and which is no progressive file's (its first scan only: the whole file comes as a coefficient image).
inline int jda_exact_check(const jda_image_info &I, int adobe, int pixel_type, int baseline_image, uint32_t n_mcus_ok)
{
    if (pixel_type != JDA_RGB8888 && pixel_type != JDA_EIGHT_BIT_GRAYSCALE) return JDA_INVALID_PARAMETER;
    if ((I.ncomp != 1 && I.ncomp != 3) || adobe) return JDA_UNSUPPORTED_FEATURE;
    if (I.width <= 0 || I.height <= 0 || I.mcus_x <= 0 || I.mcus_y <= 0) return JDA_INVALID_PARAMETER;
    if (baseline_image && I.jpeg_type != 0) return JDA_UNSUPPORTED_FEATURE;
    if (baseline_image && n_mcus_ok < (uint32_t)I.mcus_x * (uint32_t)I.mcus_y) return JDA_DECODE_ERROR;
    return JDA_SUCCESS;
}

// The same with the file's resolved colour model (JDA_CS_*, jda_colour_model) in the place of the Adobe flag: what the _ex calls take with
// JDA_EXACT_COLOUR_MODELS.  An Adobe segment refuses nothing by itself; gray and YCbCr go the kernels' way as ever, an
// RGB-coded file (three components of a colour layout) to an RGB8888 surface only -- its component 0 is red, not luma.  Four components
// (CMYK, YCCK; I as the file's header has it, k_hv component 3's sampling byte): a coefficient image only, at full size only, components
// 0..2 of a colour layout, component 3 at 1x1 or at component 0's factors, to an RGB8888 or a CMYK8888 surface.  JDA_CMYK8888 is a
// pixel type of four-component sources alone.
inline int jda_exact_check_cs(const jda_image_info &I, int colour, int pixel_type, int baseline_image, uint32_t n_mcus_ok, int scale = 1, int k_hv = 0)
{
    if (I.ncomp == 4) {
        if (pixel_type == JDA_EIGHT_BIT_GRAYSCALE) return JDA_UNSUPPORTED_FEATURE;      // (Pillow's draft("L") does nothing for CMYK)
        if (pixel_type != JDA_RGB8888 && pixel_type != JDA_CMYK8888) return JDA_INVALID_PARAMETER;
        if (I.width <= 0 || I.height <= 0 || I.mcus_x <= 0 || I.mcus_y <= 0) return JDA_INVALID_PARAMETER;
        if (colour != JDA_CS_CMYK && colour != JDA_CS_YCCK) return JDA_UNSUPPORTED_FEATURE;
        if (baseline_image || jda_mode_of(I) == JDA_MODE_GRAY || (k_hv != 0x11 && k_hv != I.subsample)) return JDA_UNSUPPORTED_FEATURE;
        if (scale == 2 || scale == 4 || scale == 8) return JDA_UNSUPPORTED_FEATURE;
        return JDA_SUCCESS;
    }
    const int rc = jda_exact_check(I, 0, pixel_type, baseline_image, n_mcus_ok);
    if (rc != JDA_SUCCESS) return rc;
    if (I.ncomp == 1 ? colour != JDA_CS_GRAY : (colour != JDA_CS_YCBCR && colour != JDA_CS_RGB)) return JDA_UNSUPPORTED_FEATURE;
    if (colour == JDA_CS_RGB && (pixel_type == JDA_EIGHT_BIT_GRAYSCALE || jda_mode_of(I) == JDA_MODE_GRAY)) return JDA_UNSUPPORTED_FEATURE;
    return JDA_SUCCESS;
}

// The planes of one image: Y over the whole MCU grid, Cb and Cr (a colour file decoded in colour) over theirs, the rows a multiple of
// 16 bytes apart, each plane's start a multiple of 256 from the image's.  cw x ch: a chroma component's own extent.
struct jda_exact_geo {
    uint32_t hs, vs, pitch_y, pitch_c, rows_y, rows_c, cw, ch;
    size_t off[3], bytes;
    uint32_t scale, ss_y, ss_c, w, h, up;                    // jda_exact_geometry_scaled's (zeros from jda_exact_geometry)
    // jda_exact_geometry4's (zeros from the others): component 3's plane -- component 0's pitch, rows and extent where it has its
    // sampling (k_full), a chroma plane's otherwise
    size_t off_k;
    uint32_t k_full, pitch_k, rows_k, kw, kh;
};
inline int jda_exact_geometry(const jda_image_info &I, bool luma_only, jda_exact_geo *G)
{
    const int mode = jda_mode_of(I);
    memset(G, 0, sizeof(*G));
    G->hs = (mode == JDA_MODE_420 || mode == JDA_MODE_422) ? 2u : 1u;
    G->vs = (mode == JDA_MODE_420 || mode == JDA_MODE_440) ? 2u : 1u;
    G->pitch_y = ((uint32_t)I.mcus_x * 8u * G->hs + 15u) & ~15u;
    G->rows_y = (uint32_t)I.mcus_y * 8u * G->vs;
    G->cw = ((uint32_t)I.width + G->hs - 1u) / G->hs;
    G->ch = ((uint32_t)I.height + G->vs - 1u) / G->vs;
    // the kernels address a plane with 32-bit byte offsets
    if ((uint64_t)G->pitch_y * G->rows_y >= (1ull << 32)) return JDA_UNSUPPORTED_FEATURE;
    size_t at = ((size_t)G->pitch_y * G->rows_y + 255u) & ~(size_t)255u;
    if (mode != JDA_MODE_GRAY && !luma_only) {
        G->pitch_c = ((uint32_t)I.mcus_x * 8u + 15u) & ~15u;
        G->rows_c = (uint32_t)I.mcus_y * 8u;
        for (int c = 1; c < 3; c++) { G->off[c] = at; at += ((size_t)G->pitch_c * G->rows_c + 255u) & ~(size_t)255u; }
    }
    G->bytes = at;
    return JDA_SUCCESS;
}

// The image's record.  quant_zz: the DQT entries of Y, Cb, Cr as the file lists them (zig-zag order); scratch: where the image's planes
// begin (device); out == NULL: no surface (jda_exact_decode_planes runs the first stage only).
inline void jda_exact_fill(jda_ex_desc &X, const jda_image_info &I, const uint16_t (*quant_zz)[64], const jda_exact_geo &G, uint8_t *scratch, const jda_output *out,
                           int pixel_type, bool luma_only)
{
    memset(&X, 0, sizeof(X));
    for (int c = 0; c < 3; c++) X.plane[c] = scratch + G.off[c];
    X.pitch_y = G.pitch_y; X.pitch_c = G.pitch_c;
    X.w = (uint32_t)I.width; X.h = (uint32_t)I.height; X.cw = G.cw; X.ch = G.ch;
    X.luma_only = luma_only ? 1u : 0u;
    X.gray_out = pixel_type == JDA_EIGHT_BIT_GRAYSCALE ? 1u : 0u;
    if (out) {
        X.out = (uint8_t *)out->pixels; X.out_pitch = (uint32_t)out->pitch_bytes;
        X.out_w = out->width_px < I.width ? (uint32_t)(out->width_px < 0 ? 0 : out->width_px) : (uint32_t)I.width;
        X.out_rows = out->rows < I.height ? (uint32_t)(out->rows < 0 ? 0 : out->rows) : (uint32_t)I.height;
    }
    for (int c = 0; c < 3; c++)
        for (uint32_t z = 0; z < 64u; z++) X.quant[c][jda_en_zigzag(z)] = quant_zz[c][z];
}

// ---- four components.  I3: the header with components 0..2 alone (ncomp 3); k_full: component 3 has component 0's sampling.
// The three planes are jda_exact_geometry's, field for field; component 3's follows them, its start a multiple of 256 like theirs.
inline int jda_exact_geometry4(const jda_image_info &I3, bool k_full, jda_exact_geo *G)
{
    const int rc = jda_exact_geometry(I3, false, G);
    if (rc != JDA_SUCCESS) return rc;
    G->scale = 1u; G->ss_y = G->ss_c = 8u; G->w = (uint32_t)I3.width; G->h = (uint32_t)I3.height;
    G->k_full = k_full || jda_mode_of(I3) == JDA_MODE_444 ? 1u : 0u;
    G->pitch_k = G->k_full ? G->pitch_y : G->pitch_c;
    G->rows_k = G->k_full ? G->rows_y : G->rows_c;
    G->kw = G->k_full ? G->w : G->cw; G->kh = G->k_full ? G->h : G->ch;
    if ((uint64_t)G->pitch_k * G->rows_k >= (1ull << 32)) return JDA_UNSUPPORTED_FEATURE;
    G->off_k = G->bytes;
    G->bytes += ((size_t)G->pitch_k * G->rows_k + 255u) & ~(size_t)255u;
    return JDA_SUCCESS;
}
// The records of a four-component image: X for its components 0..2 (jda_exact_fill's for a three-component image of their layout, with
// the colour word and component 3's plane: what jda_exact_colour4 reads) and XK for component 3's gray tiles in the planes stage (its
// plane as plane[0], quant_k_zz its DQT entries).  pixel_type: JDA_RGB8888 or JDA_CMYK8888.
inline void jda_exact_fill4(jda_ex_desc &X, jda_ex_desc &XK, const jda_image_info &I3, const uint16_t (*quant_zz)[64], const uint16_t *quant_k_zz, const jda_exact_geo &G,
                            uint8_t *scratch, const jda_output *out, int pixel_type, bool ycck)
{
    jda_exact_fill(X, I3, quant_zz, G, scratch, out, JDA_RGB8888, false);
    X.cs4 = (ycck ? JDA_EX4_YCCK : 0u) | (G.k_full ? JDA_EX4_K_FULL : 0u) | (pixel_type == JDA_CMYK8888 ? JDA_EX4_CMYK_OUT : 0u);
    X.plane3 = scratch + G.off_k;
    memset(&XK, 0, sizeof(XK));
    XK.plane[0] = scratch + G.off_k;
    XK.pitch_y = G.pitch_k; XK.w = G.kw; XK.h = G.kh;
    for (uint32_t z = 0; z < 64u; z++) XK.quant[0][jda_en_zigzag(z)] = quant_k_zz[z];
}

// ---- the scaled decode: libjpeg's 1/2, 1/4 and 1/8 as Pillow's draft() drives them
inline bool jda_exact_scale_ok(int scale) { return scale == 1 || scale == 2 || scale == 4 || scale == 8; }
// Pillow's choice for a requested req_w x req_h: the largest of 8, 4, 2, 1 that does not exceed min(W / req_w, H / req_h)
inline int jda_exact_draft(const jda_image_info &I, int req_w, int req_h)
{
    if (req_w <= 0 || req_h <= 0 || I.width <= 0 || I.height <= 0) return 1;
    const int a = I.width / req_w, b = I.height / req_h, k = a < b ? a : b;
    return k >= 8 ? 8 : k >= 4 ? 4 : k >= 2 ? 2 : 1;
}
// jdmaster.c: the IDCT size of a component of h_c x v_c blocks an MCU: from min = 8 / scale, doubled while it stays below 8 and the
// component still divides the MCU's scaled extent both ways
inline uint32_t jda_exact_idct_size(uint32_t scale, uint32_t hmax, uint32_t vmax, uint32_t h_c, uint32_t v_c)
{
    const uint32_t mn = 8u / scale;
    uint32_t ss = mn;
    while (ss < 8u && (hmax * mn) % (h_c * ss * 2u) == 0u && (vmax * mn) % (v_c * ss * 2u) == 0u) ss *= 2u;
    return ss;
}
// The planes of one image at `scale`: as jda_exact_geometry, every block ss_y x ss_y (luma) or ss_c x ss_c (chroma) samples; w x h: the
// output, ceil(width / scale) x ceil(height / scale); cw x ch: a chroma component's own scaled extent; up: jdsample.c's choice.  Scale 1:
// jda_exact_geometry's numbers, field for field.
inline int jda_exact_geometry_scaled(const jda_image_info &I, bool luma_only, int scale, jda_exact_geo *G)
{
    if (!jda_exact_scale_ok(scale)) { memset(G, 0, sizeof(*G)); return JDA_INVALID_PARAMETER; }
    if (scale == 1) {
        const int rc = jda_exact_geometry(I, luma_only, G);
        G->scale = 1u; G->ss_y = G->ss_c = 8u; G->w = (uint32_t)I.width; G->h = (uint32_t)I.height;
        return rc;
    }
    const int mode = jda_mode_of(I);
    memset(G, 0, sizeof(*G));
    const uint32_t s = (uint32_t)scale, mn = 8u / s;
    G->hs = (mode == JDA_MODE_420 || mode == JDA_MODE_422) ? 2u : 1u;
    G->vs = (mode == JDA_MODE_420 || mode == JDA_MODE_440) ? 2u : 1u;
    G->scale = s;
    G->ss_y = jda_exact_idct_size(s, G->hs, G->vs, G->hs, G->vs);
    G->ss_c = jda_exact_idct_size(s, G->hs, G->vs, 1u, 1u);
    G->w = ((uint32_t)I.width + s - 1u) / s; G->h = ((uint32_t)I.height + s - 1u) / s;
    G->pitch_y = ((uint32_t)I.mcus_x * G->ss_y * G->hs + 15u) & ~15u;
    G->rows_y = (uint32_t)I.mcus_y * G->ss_y * G->vs;
    G->cw = (uint32_t)(((uint64_t)I.width * G->ss_c + G->hs * 8u - 1u) / (G->hs * 8u));
    G->ch = (uint32_t)(((uint64_t)I.height * G->ss_c + G->vs * 8u - 1u) / (G->vs * 8u));
    // (the upsampling factors that are left: hs min / ss_c by vs min / ss_c -- 4:2:0's chroma needs none below full size)
    const bool fancy = mn > 1u;
    if (mode == JDA_MODE_422) G->up = fancy && G->cw > 2u ? JDA_EX_UP_H2V1_FANCY : JDA_EX_UP_H2V1_REPLICATE;
    else if (mode == JDA_MODE_440) G->up = fancy ? JDA_EX_UP_H1V2_FANCY : JDA_EX_UP_H1V2_REPLICATE;
    else G->up = JDA_EX_UP_NONE;
    if ((uint64_t)G->pitch_y * G->rows_y >= (1ull << 32)) return JDA_UNSUPPORTED_FEATURE;
    size_t at = ((size_t)G->pitch_y * G->rows_y + 255u) & ~(size_t)255u;
    if (mode != JDA_MODE_GRAY && !luma_only) {
        G->pitch_c = ((uint32_t)I.mcus_x * G->ss_c + 15u) & ~15u;
        G->rows_c = (uint32_t)I.mcus_y * G->ss_c;
        if ((uint64_t)G->pitch_c * G->rows_c >= (1ull << 32)) return JDA_UNSUPPORTED_FEATURE;
        for (int c = 1; c < 3; c++) { G->off[c] = at; at += ((size_t)G->pitch_c * G->rows_c + 255u) & ~(size_t)255u; }
    }
    G->bytes = at;
    return JDA_SUCCESS;
}
// The image's record at G's scale.  Scale 1: jda_exact_fill's record (scale and up stay 0: the full-size kernels' record as it was).
inline void jda_exact_fill_scaled(jda_ex_desc &X, const jda_image_info &I, const uint16_t (*quant_zz)[64], const jda_exact_geo &G, uint8_t *scratch, const jda_output *out,
                                  int pixel_type, bool luma_only)
{
    jda_exact_fill(X, I, quant_zz, G, scratch, out, pixel_type, luma_only);
    if (G.scale <= 1u) return;
    X.w = G.w; X.h = G.h; X.scale = G.scale; X.up = G.up;
    if (out) {
        X.out_w = out->width_px < (int32_t)G.w ? (uint32_t)(out->width_px < 0 ? 0 : out->width_px) : G.w;
        X.out_rows = out->rows < (int32_t)G.h ? (uint32_t)(out->rows < 0 ? 0 : out->rows) : G.h;
    }
}

// ---- a pixel rectangle.  rect = {x, y, w, h} in pixels of the image at G's scale (G.w x G.h); mcu = {mx0, my0, mx1, my1}:
// the smallest half-open MCU rectangle that holds every plane sample the definition reads for those pixels -- luma the pixels' own
// samples, a chroma component what its upsampling reads an axis (jda_exr_kinds / jda_exr_reads, the functions the colour stage runs),
// clamped to its own extent; luma_only: chroma adds nothing.  Refused (JDA_INVALID_PARAMETER): an empty rectangle, a negative origin,
// one that leaves the image.
inline int jda_exact_rect_plan(const jda_image_info &I, const jda_exact_geo &G, bool luma_only, const int32_t *rect, int32_t *mcu)
{
    if (!rect || rect[2] < 1 || rect[3] < 1 || rect[0] < 0 || rect[1] < 0) return JDA_INVALID_PARAMETER;
    if ((int64_t)rect[0] + rect[2] > (int64_t)G.w || (int64_t)rect[1] + rect[3] > (int64_t)G.h) return JDA_INVALID_PARAMETER;
    const uint32_t x0 = (uint32_t)rect[0], x1 = x0 + (uint32_t)rect[2] - 1u, y0 = (uint32_t)rect[1], y1 = y0 + (uint32_t)rect[3] - 1u;
    const uint32_t lw = G.hs * G.ss_y, lh = G.vs * G.ss_y;       // luma samples an MCU
    uint32_t mx0 = x0 / lw, mx1 = x1 / lw, my0 = y0 / lh, my1 = y1 / lh;
    if (jda_mode_of(I) != JDA_MODE_GRAY && !luma_only) {
        uint32_t kh, kv, a, b;
        jda_exr_kinds(G.hs, G.vs, G.scale, G.up, G.cw, &kh, &kv);
        jda_exr_reads(kh, x0, x1, G.cw, &a, &b);
        if (a / G.ss_c < mx0) mx0 = a / G.ss_c;
        if (b / G.ss_c > mx1) mx1 = b / G.ss_c;
        jda_exr_reads(kv, y0, y1, G.ch, &a, &b);
        if (a / G.ss_c < my0) my0 = a / G.ss_c;
        if (b / G.ss_c > my1) my1 = b / G.ss_c;
    }
    mcu[0] = (int32_t)mx0; mcu[1] = (int32_t)my0;
    mcu[2] = (int32_t)(mx1 + 1u < (uint32_t)I.mcus_x ? mx1 + 1u : (uint32_t)I.mcus_x); mcu[3] = (int32_t)(my1 + 1u < (uint32_t)I.mcus_y ? my1 + 1u : (uint32_t)I.mcus_y);
    return JDA_SUCCESS;
}
// The colour stage's tile list over the destination rectangle: out_w x out_rows pixels (the clip), a record per JDA_EXR_TILE_QUADS quads
// of JDA_EXR_TILE_ROWS rows (mcu_x0, mcu_y: the tile's place in those units; count 1), padded to whole workgroups as jda_append_strips pads.
inline void jda_exact_rect_tiles(std::vector<jda_strip> &v, uint32_t image, uint32_t out_w, uint32_t out_rows)
{
    const uint32_t tx = ((out_w + 3u) / 4u + JDA_EXR_TILE_QUADS - 1u) / JDA_EXR_TILE_QUADS, ty = (out_rows + JDA_EXR_TILE_ROWS - 1u) / JDA_EXR_TILE_ROWS;
    for (uint32_t y = 0; y < ty; y++)
        for (uint32_t x = 0; x < tx; x++) {
            jda_strip s;
            memset(&s, 0, sizeof(s));
            s.image = image; s.mcu_y = (uint16_t)y; s.mcu_x0 = (uint16_t)x; s.count = 1;
            v.push_back(s);
        }
    while (v.size() % JDA_EXR_WAVES) {
        jda_strip s;
        memset(&s, 0, sizeof(s));
        s.image = image;
        v.push_back(s);
    }
}
// The image's record of a rectangle decode: jda_exact_fill_scaled's, the clip that of the RECTANGLE (the surface holds it, not the image),
// and the rectangle beside it.  At scale 1 the record's scale and up stay 0, as ever.
inline void jda_exact_fill_rect(jda_ex_desc &X, jda_exr_rec &R, const jda_image_info &I, const uint16_t (*quant_zz)[64], const jda_exact_geo &G, uint8_t *scratch,
                                const jda_output *out, int pixel_type, bool luma_only, const int32_t *rect)
{
    jda_exact_fill_scaled(X, I, quant_zz, G, scratch, out, pixel_type, luma_only);
    R.x = (uint32_t)rect[0]; R.y = (uint32_t)rect[1]; R.w = (uint32_t)rect[2]; R.h = (uint32_t)rect[3];
    X.out_w = out->width_px < rect[2] ? (uint32_t)(out->width_px < 0 ? 0 : out->width_px) : R.w;
    X.out_rows = out->rows < rect[3] ? (uint32_t)(out->rows < 0 ? 0 : out->rows) : R.h;
}

#endif
