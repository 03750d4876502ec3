// devprims_ops.h -- one dispatcher per family of the device-only helper branches of jda_device_core.h, op -> helper.
//
// Test infrastructure.  A dispatcher is __host__ __device__: devprims.hip calls it from a plain kernel (lane = element) and
// from a host loop, so that the SAME call expression reaches both sides of every `#if defined(__HIP_DEVICE_COMPILE__)` fork;
// devprims_main.cpp compiles the host loops alone, under AddressSanitizer + UBSan.  The op numbers are tests/devprims_util.py's.
#ifndef DEVPRIMS_OPS_H
#define DEVPRIMS_OPS_H

#include "../../jpegdec_amd/csrc/jda_device_core.h"

// ---- family 1: lane-local value helpers, out = f(a, b, c) -------------------------------------------------------------------
enum {
    DP_ALIGNBYTE = 0, DP_ALIGNBIT, DP_PERM, DP_DUP8, DP_DUP16, DP_PACK16,
    DP_PK_ADD16, DP_PK_SUB16, DP_PK_ADD16_BHI, DP_PK_ADD16_ALO, DP_PK_ADD16_AHI,
    DP_PK_SEXT10_AT5, DP_PK_LIMIT10, DP_SAT_PK_U8, DP_PK_CLAMP255, DP_PK_ASHR2,
    DP_MAD24, DP_UMUL24, DP_MULC_FAST, DP_MULC_FULL, DP_RS_MUL_U, DP_RS_MUL_S,
    DP_UDOT4, DP_UDOT4_ACC, DP_SHR_UPTO32, DP_EXTEND_TOP, DP_ADD_BYTE0, DP_BFE, DP_LAG_ADD,
    DP_UNPACK_HALF, DP_UNPACK_BYTE, DP_RS_CLIP_U, DP_RS_CLIP_S, DP_VAL_OPS
};
JDA_HD uint32_t dp_val(int op, uint32_t a, uint32_t b, uint32_t c)
{
    switch (op) {
    case DP_ALIGNBYTE: return jda_alignbyte(a, b, c);
    case DP_ALIGNBIT: return jda_alignbit(a, b, c);
    case DP_PERM: return jda_perm(a, b, c);
    case DP_DUP8: return jda_dup8(a);
    case DP_DUP16: return jda_dup16((int32_t)a);
    case DP_PACK16: return jda_pack16((int32_t)a, (int32_t)b);
    case DP_PK_ADD16: return jda_pk_add16(a, b);
    case DP_PK_SUB16: return jda_pk_sub16(a, b);
    case DP_PK_ADD16_BHI: return jda_pk_add16_bhi(a, b);
    case DP_PK_ADD16_ALO: return jda_pk_add16_alo(a, b);
    case DP_PK_ADD16_AHI: return jda_pk_add16_ahi(a, b);
    case DP_PK_SEXT10_AT5: return jda_pk_sext10_at5(a);
    case DP_PK_LIMIT10: return jda_pk_limit10(a);
    case DP_SAT_PK_U8: return jda_sat_pk_u8(a);
    case DP_PK_CLAMP255: return jda_pk_clamp255(a);
    case DP_PK_ASHR2: return jda_pk_ashr2(a);
    case DP_MAD24: return (uint32_t)jda_mad24((int32_t)a, (int32_t)b, (int32_t)c);
    case DP_UMUL24: return jda_umul24(a, b);
    case DP_MULC_FAST: return (uint32_t)jda_mulc<true>((int32_t)a, (int32_t)b);
    case DP_MULC_FULL: return (uint32_t)jda_mulc<false>((int32_t)a, (int32_t)b);
    case DP_RS_MUL_U: return jda_rs_mul(a, b);
    case DP_RS_MUL_S: return (uint32_t)jda_rs_mul(a, (int32_t)b);
    case DP_UDOT4: return jda_udot4(a, b);
    case DP_UDOT4_ACC: return jda_udot4_acc(a, b, c);
    case DP_SHR_UPTO32: return jda_shr_upto32(a, b);
    case DP_EXTEND_TOP: return (uint32_t)jda_extend_top(a, b);
    case DP_ADD_BYTE0: return jda_add_byte0(a, b);
    case DP_BFE: return jda_bfe(a, b, c);
    case DP_LAG_ADD: return jda_lag_add(a, b);
    case DP_UNPACK_HALF: { const float f = jda_unpack_half(a); uint32_t r; __builtin_memcpy(&r, &f, 4); return r; }
    case DP_UNPACK_BYTE: return jda_unpack_byte(jda_unpack_f32(a), jda_unpack_f32(b), jda_unpack_f32(c));
    case DP_RS_CLIP_U: return jda_rs_clip(a);
    case DP_RS_CLIP_S: return jda_rs_clip((int32_t)a);
    }
    return 0xdeadbeefu;
}

// ---- family 2: wave helpers, one wavefront of 64 lanes, all present; two words a lane ----------------------------------------
// all_a / all_b: the 64 lanes' operands (host: what the emulator hands in; device: not read)
enum { DP_EXCL_SUM = 0, DP_CLASS_RANK0, DP_CLASS_RANK1, DP_CLASS_RANK2, DP_CLASS_RANK3, DP_LANE_PULL, DP_WAVE_ANY_BRANCH, DP_WAVE_OPS };
#define DP_WAVE_OUTSIDE 0x0badf00du          // DP_WAVE_ANY_BRANCH: what a lane that stays out of the branch reports
JDA_HD void dp_wave(int op, uint32_t lane, uint32_t a, uint32_t b, const uint32_t *all_a, uint32_t &r0, uint32_t &r1)
{
    r0 = r1 = 0xdeadbeefu;
    switch (op) {
    case DP_EXCL_SUM: r0 = jda_wave_excl_sum(a, lane, all_a, r1); break;
    case DP_CLASS_RANK0: case DP_CLASS_RANK1: case DP_CLASS_RANK2: case DP_CLASS_RANK3:
        r0 = jda_wave_class_rank(a, (uint32_t)(op - DP_CLASS_RANK0), lane, all_a, r1); break;
    case DP_LANE_PULL: r0 = jda_lane_pull(a, b, all_a); r1 = 0u; break;
    case DP_WAVE_ANY_BRANCH:                                     // the lanes with b != 0 go in; inside, "does some lane here have a != 0?"
        r0 = DP_WAVE_OUTSIDE; r1 = jda_wave_any(b != 0u) ? 1u : 0u;          // (.. and outside the branch, over all lanes: "did any go in?")
        if (b != 0u) r0 = jda_wave_any(a != 0u) ? 1u : 0u;
        break;
    }
}

// ---- family 3: LDS helpers over a 256-byte window behind a 16-byte pad ------------------------------------------------------
#define DP_WIN_BYTES 256u
#define DP_WIN_PAD 16u
#define DP_WR_STOP 0xdeadbeefu               // a walk's entries behind its last peek
// one walk of the window reader: peeks[s] = the peek before step s's bits are consumed; a step of 0 ends the walk, and so does a
// position whose peek would read outside [pad .. window end): that is the kernel's own bound, whatever the test hands in
JDA_HD void dp_wr_walk(const uint8_t *win, uint32_t pos, uint32_t off, const uint8_t *steps, uint32_t *peeks, uint32_t maxsteps)
{
    jda_wreader R;
    jda_wr_init(R, win, pos, off);
    int32_t rel = (int32_t)((pos << 3) + off) - 1;               // R.m counted from the window's first bit
    for (uint32_t s = 0; s < maxsteps; s++) peeks[s] = DP_WR_STOP;
    for (uint32_t s = 0; s < maxsteps; s++) {
        if (rel < -1 || (rel >> 5) + 1 >= (int32_t)(DP_WIN_BYTES / 4u)) break;
        peeks[s] = jda_wr_peek(R);
        const uint32_t n = steps[s];
        if (n == 0u || n > 32u) break;
        jda_wr_consume(R, n);
        rel += (int32_t)n;
    }
}
enum { DP_BYTES_APART = 0, DP_LOAD_U16, DP_COEF_STORE, DP_LDS_OPS };
// lane-local reads: a = byte offset (step / table offset), b = delta.  Offsets are reduced to the window here.
JDA_HD uint32_t dp_lds_read(int op, const uint8_t *win, uint32_t a, uint32_t b)
{
    if (op == DP_BYTES_APART) {
        const uint32_t step = a % (DP_WIN_BYTES / 2u), delta = b % (DP_WIN_BYTES / 2u);
        uint32_t b0, b1;
        jda_lds_bytes_apart(win, step, delta, b0, b1);
        return b0 | (b1 << 8);
    }
    const uint32_t o = (a % (DP_WIN_BYTES - 1u)) & ~1u;          // an even offset, the 16-bit entry inside the window
    return JDA_LDS_LOAD_U16(win, JDA_LDS_A32(win) + o);
}
// the store: t's byte 0 is the offset (even: the zigzag table's entries are), the rest of t must be ignored
JDA_HD void dp_coef_store(uint8_t *win, uint32_t t, uint32_t v)
{
    int16_t *coef = (int16_t *)win;
    JDA_COEF_STORE(coef, t & ~1u, v);
}

// ---- family 4: the pixel formulas over the (Y, Cb, Cr) cube, element i = (Y << 16) | (Cb << 8) | Cr ----------------------------
enum {
    DP_EX_RGBA = 0, DP_PIXEL_RGBA, DP_PIXEL_565_LE, DP_PIXEL_565_BE,
    DP_PAIR_RGBA_PX0, DP_PAIR_RGBA_PX1, DP_PAIR_565_LE, DP_PAIR_565_BE,
    DP_PAIR2_RGBA_PX0, DP_PAIR2_RGBA_PX1,
    DP_HALF_RGBA_PX0, DP_HALF_RGBA_PX1, DP_HALF_565_LE, DP_HALF_565_BE,
    DP_RGB_PIXEL_RGBA, DP_RGB_PIXEL_565_LE, DP_RGB_PIXEL_565_BE, DP_CUBE_OPS
};
// A pair's second pixel: luma 255 - Y; where the two pixels have chroma samples of their own, the second's are (Cr, Cb).
// Half size: the 2x2 luma sums are 4 Y + (Cr & 3) and 1023 less that.
JDA_HD uint32_t dp_cube(int op, uint32_t i)
{
    const uint32_t y = (i >> 16) & 255u, cb = (i >> 8) & 255u, cr = i & 255u;
    const uint32_t ypair = y | ((255u - y) << 16);
    const uint32_t s0 = 4u * y + (cr & 3u), ysum2 = s0 | ((1023u - s0) << 16);
    uint32_t px0 = 0, px1 = 0;
    switch (op) {
    case DP_EX_RGBA: return jda_ex_rgba(y, cb, cr);
    case DP_PIXEL_RGBA: { jda_ycc p = { (int32_t)(y << 12), (int32_t)cb, (int32_t)cr }; return jda_pixel_rgba(p); }
    case DP_PIXEL_565_LE: case DP_PIXEL_565_BE: { jda_ycc p = { (int32_t)(y << 12), (int32_t)cb, (int32_t)cr }; return jda_pixel_565(p, op == DP_PIXEL_565_BE); }
    case DP_PAIR_RGBA_PX0: case DP_PAIR_RGBA_PX1: {
        const jda_chroma2 d = jda_chroma_terms16(cb, cr);
        const uint32_t rg = jda_pack_hi16(d.r, d.g);
        jda_rgba_pair_rg<true>(ypair, rg, rg, d.b, px0, px1);
        return op == DP_PAIR_RGBA_PX0 ? px0 : px1;
    }
    case DP_PAIR_565_LE: return jda_565_pair_t16<JDA_RGB565_LITTLE_ENDIAN>(ypair, jda_chroma_terms16(cb, cr));
    case DP_PAIR_565_BE: return jda_565_pair_t16<JDA_RGB565_BIG_ENDIAN>(ypair, jda_chroma_terms16(cb, cr));
    case DP_PAIR2_RGBA_PX0: case DP_PAIR2_RGBA_PX1: {
        const jda_chroma2 c0 = jda_chroma_terms16(cb, cr), c1 = jda_chroma_terms16(cr, cb);
        jda_rgba_pair_rg<false>(ypair, jda_pack_hi16(c0.r, c0.g), jda_pack_hi16(c1.r, c1.g), jda_pack_hi16(c0.b, c1.b), px0, px1);
        return op == DP_PAIR2_RGBA_PX0 ? px0 : px1;
    }
    case DP_HALF_RGBA_PX0: case DP_HALF_RGBA_PX1: {
        const jda_chroma2 c0 = jda_chroma_terms64(cb, cr), c1 = jda_chroma_terms64(cr, cb);
        jda_rgba_pair_half(ysum2, jda_pack_hi16(c0.r, c1.r), jda_pack_hi16(c0.g, c1.g), jda_pack_hi16(c0.b, c1.b), px0, px1);
        return op == DP_HALF_RGBA_PX0 ? px0 : px1;
    }
    case DP_HALF_565_LE: case DP_HALF_565_BE: {
        const jda_chroma2 c0 = jda_chroma_terms64(cb, cr), c1 = jda_chroma_terms64(cr, cb);
        const uint32_t tr = jda_pack_hi16(c0.r, c1.r), tg = jda_pack_hi16(c0.g, c1.g), tb = jda_pack_hi16(c0.b, c1.b);
        return op == DP_HALF_565_LE ? jda_565_pair_half<JDA_RGB565_LITTLE_ENDIAN>(ysum2, tr, tg, tb) : jda_565_pair_half<JDA_RGB565_BIG_ENDIAN>(ysum2, tr, tg, tb);
    }
    case DP_RGB_PIXEL_RGBA: return jda_rgb_pixel<JDA_RGB8888>(y, jda_chroma_terms(cb, cr));
    case DP_RGB_PIXEL_565_LE: return jda_rgb_pixel<JDA_RGB565_LITTLE_ENDIAN>(y, jda_chroma_terms(cb, cr));
    case DP_RGB_PIXEL_565_BE: return jda_rgb_pixel<JDA_RGB565_BIG_ENDIAN>(y, jda_chroma_terms(cb, cr));
    }
    return 0xdeadbeefu;
}

// ---- the host loops (the host side of every fork) ---------------------------------------------------------------------------
static void dp_host_val(int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, int n)
{
    for (int i = 0; i < n; i++) out[i] = dp_val(op, a[i], b[i], c[i]);
}
static void dp_host_wave(int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int n)      // n: a multiple of 64; out: 2 n words
{
    for (int w = 0; w + 64 <= n; w += 64)
        for (uint32_t l = 0; l < 64u; l++) dp_wave(op, l, a[w + l], b[w + l], a + w, out[2 * (w + l)], out[2 * (w + l) + 1]);
}
// win: the 64 dwords of the window as they lie in LDS; start[w] = pos << 3 | off; steps: maxsteps bytes a walk; out: maxsteps words a walk
static void dp_host_wr(const uint32_t *win, const uint32_t *start, const uint8_t *steps, uint32_t *out, int nwalks, int maxsteps)
{
    uint32_t buf[(DP_WIN_PAD + DP_WIN_BYTES) / 4u + 4u];
    for (uint32_t i = 0; i < DP_WIN_PAD / 4u; i++) buf[i] = 0x5a5a5a5au;
    for (uint32_t i = 0; i < DP_WIN_BYTES / 4u; i++) buf[DP_WIN_PAD / 4u + i] = win[i];
    for (uint32_t i = 0; i < 4u; i++) buf[(DP_WIN_PAD + DP_WIN_BYTES) / 4u + i] = 0x5a5a5a5au;
    for (int w = 0; w < nwalks; w++)
        dp_wr_walk((const uint8_t *)buf + DP_WIN_PAD, start[w] >> 3, start[w] & 7u, steps + (size_t)w * maxsteps, out + (size_t)w * maxsteps, (uint32_t)maxsteps);
}
// n: a multiple of 64.  DP_COEF_STORE: every group of 64 lanes stores into a fresh copy of the window (the test hands a group distinct
// offsets), and lane l reports dword l of it afterwards
static void dp_host_lds(int op, const uint32_t *win, const uint32_t *a, const uint32_t *b, uint32_t *out, int n)
{
    // (bytes, filled and read back as bytes: the helpers read and write them as 16-bit entries, as the kernels' tables are)
    uint8_t buf[DP_WIN_PAD + DP_WIN_BYTES] __attribute__((aligned(16)));
    uint8_t *w8 = buf + DP_WIN_PAD;
    for (int g = 0; g + 64 <= n; g += 64) {
        __builtin_memset(buf, 0x5a, DP_WIN_PAD);
        __builtin_memcpy(w8, win, DP_WIN_BYTES);
        if (op == DP_COEF_STORE) {
            for (int l = 0; l < 64; l++) dp_coef_store(w8, a[g + l], b[g + l]);
            for (int l = 0; l < 64; l++) __builtin_memcpy(&out[g + l], w8 + 4 * l, 4);
        } else
            for (int l = 0; l < 64; l++) out[g + l] = dp_lds_read(op, w8, a[g + l], b[g + l]);
    }
}
static void dp_host_cube(int op, uint32_t *out, uint32_t first, int n)
{
    for (int i = 0; i < n; i++) out[i] = dp_cube(op, first + (uint32_t)i);
}

#endif
