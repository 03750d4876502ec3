// jda_exact_plan.h -- the host side of the libjpeg-exact decode (jda_exact_decode_* ): what is refused, the
// component planes of an image in the call's scratch, its record for the kernels, and the plan of a whole call -- its blob, tile lists and
// launches.  Host work only, no HIP: the runtime and the exact sims of tests/hostsim share it.
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

// ---- the plan of a call (jda_exact_decode_* in jda_runtime.cpp): everything the call decides before it has device
// memory (jda_exact_plan_build) and what it writes once it knows where its block lies (jda_exact_plan_place).
// The kernel family of a launch.  The first three are also the kinds of a source: the planes kernel that reads it.
enum jda_exact_kind {
    JDA_EXK_PLANES_DENSE = 0,        // jda_exact_planes / _planes_scaled over tiles of dense coefficient images
    JDA_EXK_PLANES_SPARSE,           // .. of sparse ones
    JDA_EXK_PLANES_BASELINE,         // .. of resident baseline images
    JDA_EXK_COLOUR,                  // jda_exact_colour / _colour_scaled over tiles of gray and YCbCr images
    JDA_EXK_COLOUR_RGB,              // jda_exact_colour_rgb / _colour_scaled_rgb over tiles of RGB-coded images
    JDA_EXK_COLOUR4,                 // jda_exact_colour4 over tiles of four-component images (components 0..2 of the launch's layout)
    JDA_EXK_COLOUR_RECT,             // jda_exact_colour_rect<.., false> over tile records of destination rectangles
    JDA_EXK_COLOUR_RECT_RGB          // jda_exact_colour_rect<.., true>: the rectangles of RGB-coded images
};
// One resident source as the plan reads it (device pointers): a coefficient image -- tables its quantisers (and first[], sparse), scan its
// coefficients or entries -- or a baseline image -- its tables, scan, block index and DC values.  quant: the DQT entries of its components
// as the file lists them.  k: component 3 of a four-component image, a gray coefficient image of its own; NULL otherwise.
struct jda_exact_source {
    jda_exact_kind kind;
    jda_image_info info;
    int adobe, colour;
    uint32_t n_mcus_ok;
    uint16_t quant[3][64];
    const uint8_t *tables, *scan;
    const uint32_t *index;
    const int16_t *dc;
    uint32_t scan_len;
    uint8_t ac_id[3];
    const jda_exact_source *k;
};
// One launch: `n_tiles` tile records at `off` of the blob, of images of layout `mode` decoded at `scale`
struct jda_exact_launch { jda_exact_kind kind; int mode, scale; size_t off; uint32_t n_tiles; };
// A planned image (kind < 0: refused, nothing of it is launched): its header (a four-component image's with components 0..2 alone), its
// planes G at plane_at of the scratch, its MCU rectangle and what jda_exact_plan_place fills its record from
struct jda_exact_image {
    int kind;
    jda_image_info info;
    uint16_t quant[3][64], quant_k[64];
    jda_exact_geo G;
    size_t plane_at;
    bool luma_only, rgb, four, rect, has_out;
    int colour, pixel_type;
    int32_t mcu[4], rq[4];
    jda_output out;
};
// The block of a call: the blob (descs | records | baseline sources, `n_rec` of each: one an image, two with flags | the tile lists, in
// launch order | a rectangle record an image, in a call with a rectangle), the scratch at o_scratch (a multiple of 256) behind it: every
// planned image's planes.  launches: in launch order, the planes stage's before colour_begin.
struct jda_exact_plan {
    std::vector<uint8_t> blob;
    std::vector<jda_exact_launch> launches;
    size_t colour_begin;
    size_t o_ex, o_src, o_rect, o_scratch, scratch;
    std::vector<jda_exact_image> images;
    size_t n_rec;
    int32_t n_planned;
};
// the tiles of an image's planes stage that hold MCUs (jda_append_strips' records without its padding); mcu: jda_exact_rect_plan's, NULL: whole
// (what jda_decode_to_host_exact_rect reports, whether or not a plan is ever made)
inline int32_t jda_exact_tile_count(const jda_image_info &I, const int32_t *mcu)
{
    const uint32_t per = jda_mcus_per_tile(jda_mode_of(I));
    const uint32_t w = mcu ? (uint32_t)(mcu[2] - mcu[0]) : (uint32_t)I.mcus_x, h = mcu ? (uint32_t)(mcu[3] - mcu[1]) : (uint32_t)I.mcus_y;
    return (int32_t)(h * ((w + per - 1u) / per));
}
// A tile list of the call.  The table of them is made in launch order -- the planes lists by (layout, scale, source); the colour stage's own
// by (layout, scale, YCbCr or gray | RGB-coded), the four-component images' by layout, the rectangles' by (layout, YCbCr or gray | RGB-coded)
// -- and lies in the blob in that order, so the dense, sparse and baseline lists of a (layout, scale) are one contiguous range.
struct jda_exact_list { jda_exact_kind kind; int mode, g; std::vector<jda_strip> tiles; size_t off; };
// where a list stands in the table (g: log2 scale; source: a planes kind; rgb: the RGB-coded images' list).  A new family gets its place
// here and its entries in jda_exact_lists_init; placing, copying and launching follow the table.
enum { JDA_EXACT_L_COLOUR = JDA_N_MODES * 4 * 3, JDA_EXACT_L_FOUR = JDA_EXACT_L_COLOUR + JDA_N_MODES * 4 * 2, JDA_EXACT_L_RECT = JDA_EXACT_L_FOUR + JDA_N_MODES,
       JDA_EXACT_N_LISTS = JDA_EXACT_L_RECT + JDA_N_MODES * 2 };
inline size_t jda_exact_l_planes(int mode, int g, int source) { return ((size_t)mode * 4 + (size_t)g) * 3 + (size_t)source; }
inline size_t jda_exact_l_colour(int mode, int g, bool rgb) { return JDA_EXACT_L_COLOUR + ((size_t)mode * 4 + (size_t)g) * 2 + (rgb ? 1u : 0u); }
inline size_t jda_exact_l_four(int mode) { return JDA_EXACT_L_FOUR + (size_t)mode; }
inline size_t jda_exact_l_rect(int mode, bool rgb) { return JDA_EXACT_L_RECT + (size_t)mode * 2 + (rgb ? 1u : 0u); }
inline void jda_exact_lists_init(jda_exact_list *L)
{
    for (int m = 0; m < JDA_N_MODES; m++) {
        for (int g = 0; g < 4; g++) {
            for (int f = 0; f < 3; f++) { jda_exact_list &l = L[jda_exact_l_planes(m, g, f)]; l.kind = (jda_exact_kind)f; l.mode = m; l.g = g; }
            for (int f = 0; f < 2; f++) { jda_exact_list &l = L[jda_exact_l_colour(m, g, f != 0)]; l.kind = f ? JDA_EXK_COLOUR_RGB : JDA_EXK_COLOUR; l.mode = m; l.g = g; }
        }
        { jda_exact_list &l = L[jda_exact_l_four(m)]; l.kind = JDA_EXK_COLOUR4; l.mode = m; l.g = 0; }
        for (int f = 0; f < 2; f++) { jda_exact_list &l = L[jda_exact_l_rect(m, f != 0)]; l.kind = f ? JDA_EXK_COLOUR_RECT_RGB : JDA_EXK_COLOUR_RECT; l.mode = m; l.g = 0; }
    }
}
inline size_t jda_exact_align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// What a call does before it allocates.  sources: n views; outputs / pixel_types (NULL: RGB8888) or planes (three entries an image, four
// with flags): the call's; scales (NULL: all 1), flags (JDA_EXACT_COLOUR_MODELS or 0), rects (NULL: none; {x, y, w, h} an image, all zero:
// whole): the call's.  status[i]: JDA_SUCCESS, or why image i is refused -- it is left out (its records stay zero) and the call goes on.
// Without flags and rectangles the colour stage walks the planes lists: one launch a (layout, scale) over its three lists.  Otherwise those
// hold tiles the whole-image colour kernels must not walk (component 3's gray tiles, a rectangle's), and the colour stage has lists of its own.
inline int jda_exact_plan_build(int32_t n, const jda_exact_source *src, const jda_output *outputs, const int32_t *pixel_types, const jda_output *planes, const int32_t *scales,
                                uint32_t flags, const int32_t *rects, int32_t *status, jda_exact_plan *plan)
{
    plan->blob.clear(); plan->launches.clear(); plan->images.clear();
    plan->colour_begin = plan->o_ex = plan->o_src = plan->o_rect = plan->o_scratch = plan->scratch = plan->n_rec = 0;
    plan->n_planned = 0;
    if (n < 0 || (n > 0 && (!src || !status || (!outputs && !planes)))) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    const size_t nrec = flags ? 2u * (size_t)n : (size_t)n;    // (a four-component image's component 3 is record n + i)
    const int ps = flags ? 4 : 3;                               // entries an image in planes
    std::vector<jda_dev_desc> descs(nrec);
    std::vector<jda_ex_src> esrc(nrec);
    memset(descs.data(), 0, nrec * sizeof(jda_dev_desc)); memset(esrc.data(), 0, nrec * sizeof(jda_ex_src));
    plan->images.resize((size_t)n);
    plan->n_rec = nrec;
    bool any_rect = false;
    for (int i = 0; i < n && rects && outputs; i++) any_rect = any_rect || rects[4 * i] || rects[4 * i + 1] || rects[4 * i + 2] || rects[4 * i + 3];
    const bool own_cs = flags || any_rect;                      // the colour stage has lists of its own
    jda_exact_list L[JDA_EXACT_N_LISTS];
    const size_t nl = JDA_EXACT_N_LISTS;
    jda_exact_lists_init(L);
    for (int i = 0; i < n; i++) {
        jda_exact_image &M = plan->images[(size_t)i];
        jda_dev_desc &D = descs[(size_t)i];
        const jda_exact_source &S = src[i];
        M.kind = (int)S.kind; M.info = S.info;
        memcpy(M.quant, S.quant, sizeof(M.quant)); memset(M.quant_k, 0, sizeof(M.quant_k));
        const jda_image_info &I = M.info;
        const int pt = outputs ? (pixel_types ? pixel_types[i] : JDA_RGB8888) : JDA_RGB8888;
        const int scale = scales ? scales[i] : 1;
        const bool baseline = S.kind == JDA_EXK_PLANES_BASELINE;
        const jda_exact_source *kd = S.k;
        int rc = (flags & JDA_EXACT_COLOUR_MODELS) ? jda_exact_check_cs(I, S.colour, pt, baseline, S.n_mcus_ok, scale, kd ? (kd->info.mcus_x == I.mcus_x && kd->info.mcus_y == I.mcus_y ? 0x11 : I.subsample) : 0)
                                                   : jda_exact_check(I, S.adobe, pt, baseline, S.n_mcus_ok);
        M.rgb = (flags & JDA_EXACT_COLOUR_MODELS) && S.colour == JDA_CS_RGB;
        M.four = (flags & JDA_EXACT_COLOUR_MODELS) && I.ncomp == 4;
        M.colour = S.colour; M.pixel_type = pt;
        M.luma_only = outputs && pt == JDA_EIGHT_BIT_GRAYSCALE && I.ncomp == 3;
        M.has_out = outputs != NULL;
        if (outputs) M.out = outputs[i]; else memset(&M.out, 0, sizeof(M.out));
        if (rc == JDA_SUCCESS && M.four && (!kd || S.kind != JDA_EXK_PLANES_DENSE)) rc = JDA_UNSUPPORTED_FEATURE;      // (dense, with component 3 beside it)
        if (M.four) { M.info.ncomp = 3; M.info.bpp = 24; }     // (components 0..2 from here on: I is M.info)
        if (rc == JDA_SUCCESS && !jda_exact_scale_ok(scale)) rc = JDA_INVALID_PARAMETER;
        if (rc == JDA_SUCCESS) rc = M.four ? jda_exact_geometry4(I, kd->info.mcus_x != I.mcus_x || kd->info.mcus_y != I.mcus_y, &M.G) : jda_exact_geometry_scaled(I, M.luma_only, scale, &M.G);
        const int32_t *rq = any_rect ? rects + 4 * i : NULL;
        M.rect = rq && (rq[0] || rq[1] || rq[2] || rq[3]);
        for (int k = 0; k < 4; k++) M.rq[k] = rq ? rq[k] : 0;
        if (rc == JDA_SUCCESS && M.rect) rc = M.four ? JDA_UNSUPPORTED_FEATURE : jda_exact_rect_plan(I, M.G, M.luma_only, rq, M.mcu);
        if (rc == JDA_SUCCESS && outputs) {
            jda_image_info B = I;
            B.jpeg_type = 0;
            const uint8_t none[3] = { 0, 0, 0 };
            jda_output O = outputs[i];                         // (a scaled image: the surface is held to the scaled size, not to the file's)
            if (scale > 1 && O.width_px > (int32_t)M.G.w) O.width_px = (int32_t)M.G.w;
            if (scale > 1 && O.rows > (int32_t)M.G.h) O.rows = (int32_t)M.G.h;
            if (M.rect && O.width_px > rq[2]) O.width_px = rq[2];      // (a rectangle: the surface holds it, not the image)
            if (M.rect && O.rows > rq[3]) O.rows = rq[3];
            rc = jda_fill_launch_desc(D, B, none, none, none, 0, 0, (uint32_t)(I.mcus_x * I.mcus_y), 0, O, pt == JDA_CMYK8888 ? JDA_RGB8888 : pt, 0, NULL);      // (four bytes a pixel either way)
        } else if (rc == JDA_SUCCESS) {
            D.mode = (uint8_t)jda_mode_of(I); D.ncomp = (uint8_t)I.ncomp; D.mcus_x = (uint32_t)I.mcus_x; D.mcus_y = (uint32_t)I.mcus_y;
            for (int c = 0; c < (M.four ? 4 : I.ncomp == 3 ? 3 : 1) && rc == JDA_SUCCESS; c++) {
                const jda_output &P = planes[ps * i + c];
                const int32_t ew = c == 3 ? (int32_t)M.G.kw : c ? (int32_t)M.G.cw : (int32_t)M.G.w;
                if (!P.pixels || P.width_px < 0 || P.rows < 0 || P.pitch_bytes < (P.width_px < ew ? P.width_px : ew)) rc = JDA_INVALID_PARAMETER;
            }
        }
        if (rc != JDA_SUCCESS) { status[i] = rc; memset(&D, 0, sizeof(D)); M.kind = -1; continue; }
        status[i] = JDA_SUCCESS;
        plan->n_planned++;
        M.plane_at = plan->scratch; plan->scratch += M.G.bytes;
        if (baseline) {
            jda_ex_src &J = esrc[(size_t)i];
            J.S.scan = S.scan; J.S.blk_index = S.index; J.S.blk_dc = S.dc; J.S.tables = S.tables; J.S.scan_len = S.scan_len; J.S.kind = JDA_RC_IMAGE;
            for (int c = 0; c < 3; c++) J.S.ac_id[c] = S.ac_id[c];
            J.bpm = (uint32_t)I.blocks_per_mcu; J.nluma = I.ncomp == 3 ? J.bpm - 2u : 1u;
        } else {
            D.tables = S.tables; D.scan = S.scan;
        }
        const int g = M.G.scale == 8u ? 3 : M.G.scale == 4u ? 2 : M.G.scale == 2u ? 1 : 0;
        jda_append_strips(L[jda_exact_l_planes(D.mode, g, M.kind)].tiles, (uint32_t)i, D.mcus_x, D.mcus_y, D.mode, 0, M.rect ? M.mcu : NULL);
        if (M.four) {
            jda_dev_desc &DK = descs[(size_t)n + (size_t)i];
            memcpy(M.quant_k, kd->quant[0], sizeof(M.quant_k));
            DK.mode = (uint8_t)JDA_MODE_GRAY; DK.ncomp = 1; DK.mcus_x = (uint32_t)kd->info.mcus_x; DK.mcus_y = (uint32_t)kd->info.mcus_y;
            DK.tables = kd->tables; DK.scan = kd->scan;
            jda_append_strips(L[jda_exact_l_planes(JDA_MODE_GRAY, 0, JDA_EXK_PLANES_DENSE)].tiles, (uint32_t)(n + i), DK.mcus_x, DK.mcus_y, JDA_MODE_GRAY);
            if (outputs) jda_append_strips(L[jda_exact_l_four(D.mode)].tiles, (uint32_t)i, D.mcus_x, D.mcus_y, D.mode);
        } else if (M.rect) {
            const jda_output &O = outputs[i];
            jda_exact_rect_tiles(L[jda_exact_l_rect(D.mode, M.rgb)].tiles, (uint32_t)i, (uint32_t)(O.width_px < rq[2] ? (O.width_px < 0 ? 0 : O.width_px) : rq[2]),
                                 (uint32_t)(O.rows < rq[3] ? (O.rows < 0 ? 0 : O.rows) : rq[3]));
        } else if (own_cs && outputs) jda_append_strips(L[jda_exact_l_colour(D.mode, g, M.rgb)].tiles, (uint32_t)i, D.mcus_x, D.mcus_y, D.mode);
    }
    if (!plan->n_planned) return JDA_SUCCESS;
    plan->o_ex = jda_exact_align16(nrec * sizeof(jda_dev_desc));
    plan->o_src = plan->o_ex + jda_exact_align16(nrec * sizeof(jda_ex_desc));
    size_t bytes = plan->o_src + jda_exact_align16(nrec * sizeof(jda_ex_src));
    for (size_t k = 0; k < nl; k++) { L[k].off = bytes; bytes += L[k].tiles.size() * sizeof(jda_strip); }
    plan->o_rect = bytes;
    if (any_rect) bytes += (size_t)n * sizeof(jda_exr_rec);
    plan->o_scratch = (bytes + 255u) & ~(size_t)255u;
    plan->blob.assign(bytes, 0);
    memcpy(plan->blob.data(), descs.data(), nrec * sizeof(jda_dev_desc));
    memcpy(plan->blob.data() + plan->o_src, esrc.data(), nrec * sizeof(jda_ex_src));
    for (size_t k = 0; k < nl; k++) {
        if (k == JDA_EXACT_L_COLOUR) {
            plan->colour_begin = plan->launches.size();
            for (int m = 0; m < JDA_N_MODES && outputs && !own_cs; m++)      // the shared lists: dense | sparse | baseline as one range
                for (int g = 0; g < 4; g++) {
                    const jda_exact_list *P = &L[jda_exact_l_planes(m, g, 0)];
                    const size_t cnt = P[0].tiles.size() + P[1].tiles.size() + P[2].tiles.size();
                    if (cnt) plan->launches.push_back(jda_exact_launch{ JDA_EXK_COLOUR, m, 1 << g, P[0].off, (uint32_t)cnt });
                }
        }
        if (L[k].tiles.empty()) continue;
        memcpy(plan->blob.data() + L[k].off, L[k].tiles.data(), L[k].tiles.size() * sizeof(jda_strip));
        plan->launches.push_back(jda_exact_launch{ L[k].kind, L[k].mode, 1 << L[k].g, L[k].off, (uint32_t)L[k].tiles.size() });
    }
    return JDA_SUCCESS;
}

// .. and once the call's block lies at `block` (device memory of o_scratch + scratch bytes; the plan never reads it): the images' records,
// their planes at block + o_scratch + plane_at, which complete the blob
inline void jda_exact_plan_place(jda_exact_plan *plan, uint8_t *block)
{
    const size_t n = plan->images.size();
    uint8_t *ex = plan->blob.data() + plan->o_ex;
    for (size_t i = 0; i < n; i++) {
        const jda_exact_image &M = plan->images[i];
        if (M.kind < 0) continue;
        uint8_t *at = block + plan->o_scratch + M.plane_at;
        const jda_output *O = M.has_out ? &M.out : NULL;
        jda_ex_desc X;
        if (M.four) {
            jda_ex_desc XK;
            jda_exact_fill4(X, XK, M.info, M.quant, M.quant_k, M.G, at, O, M.pixel_type, M.colour == JDA_CS_YCCK);
            memcpy(ex + (n + i) * sizeof(jda_ex_desc), &XK, sizeof(XK));
        } else if (M.rect) {
            jda_exr_rec R;
            jda_exact_fill_rect(X, R, M.info, M.quant, M.G, at, O, M.pixel_type, M.luma_only, M.rq);
            memcpy(plan->blob.data() + plan->o_rect + i * sizeof(jda_exr_rec), &R, sizeof(R));
        } else jda_exact_fill_scaled(X, M.info, M.quant, M.G, at, O, M.pixel_type, M.luma_only);
        memcpy(ex + i * sizeof(jda_ex_desc), &X, sizeof(X));
    }
}

#endif
