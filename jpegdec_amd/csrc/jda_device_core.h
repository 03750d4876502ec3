// jda_device_core.h -- the per-lane decode logic of the HIP kernels.
//
// Everything here is written once and compiled twice: by hipcc into the gfx950 kernels of
// jda_kernels.hip, and by g++ into tests/hostsim (a lane-by-lane CPU emulation of one wavefront
// used ONLY by the unit tests to check the kernel logic where no GPU exists).  The product path
// never runs this on the CPU.
//
// One wavefront decodes one tile: up to 64 consecutive 8x8 blocks of one MCU row (10 MCUs of 4:2:0).
//   P1  lane = block: Huffman/RLE expand into the block's int16[64] slot in LDS   <- JPEGDecodeMCU  jpeg.inl:2090-2274
//       + the wave builds the IDCT work lists (prefix sum / ballots)
//   P2  lane = (block, non-empty column): dequant + IDCT column stage           <- JPEGIDCT       jpeg.inl:2553-2679
//   P3  lane = (block, row): IDCT row stage + range limit -> 64 bytes in place   <- JPEGIDCT       jpeg.inl:2680-2797
//                                                                                  DC-only bypass jpeg.inl:5146-5154
//   P4  lanes tile the output rows: YCbCr -> RGB565/RGB8888/gray, chroma        <- JPEGPutMCU*    jpeg.inl:2799-4868
//       upsample, 1/2-1/4-1/8, coalesced stores                                    JPEGPixel*     jpeg.inl:3101-3278
// plus the segment walk of the device pre-scan (jda_seg_walk) and the tables it stages (jda_walk_tables_from).
// The bit reader reproduces the reference's 64-bit window and refill rule exactly, so that the
// low-bit truncation of SURVEY.md fact 6 is reproduced by construction.
#ifndef JDA_DEVICE_CORE_H
#define JDA_DEVICE_CORE_H

#include <stdint.h>

#include "jda_internal.h"

#if defined(__HIPCC__)
#define JDA_HD __host__ __device__ __forceinline__
#define JDA_HD_MEMBER __host__ __device__ __forceinline__
#else
#define JDA_HD static inline __attribute__((always_inline))
#define JDA_HD_MEMBER inline __attribute__((always_inline))
#endif

// ---- tile and LDS layout -------------------------------------------------------------------------
// One wavefront (64 threads) decodes one "tile": up to 64 consecutive 8x8 blocks of one MCU row =
// 10 MCUs of 4:2:0 (60 blocks), 20 MCUs of 4:4:4 (60 blocks) or 64 MCUs of a gray image.  The four
// wavefronts of a workgroup share nothing but the image's tables in LDS, so after the tables are
// staged there is no workgroup barrier: every phase boundary is a wave-local fence.
#define JDA_TILE_THREADS 64
#ifndef JDA_P1_TRACE
#define JDA_P1_TRACE(slot) ((void)0)      // profiling hook, defined by jda_kernels.hip
#endif
#define JDA_COEF_STRIDE 136      // bytes per block in LDS: 64 int16 + 8 pad (row reads stay 8-byte aligned)
// per-wave LDS window over the tile's slice of the filtered scan: jda_lds_layout<MODE>::WIN_BYTES.  Only P1 reads it, and the
// column work list is only alive from the end of P1 to the end of P2 -- so the two share their bytes: the next tile's slice
// is stored when this tile's column stage is over.

template <int MODE> struct jda_mode_traits;
template <> struct jda_mode_traits<JDA_MODE_GRAY> { enum { NLUMA = 1, NBLK = 1, MCU_W = 8, MCU_H = 8, MCU_W_LOG2 = 3 }; };
template <> struct jda_mode_traits<JDA_MODE_444>  { enum { NLUMA = 1, NBLK = 3, MCU_W = 8, MCU_H = 8, MCU_W_LOG2 = 3 }; };
template <> struct jda_mode_traits<JDA_MODE_420>  { enum { NLUMA = 4, NBLK = 6, MCU_W = 16, MCU_H = 16, MCU_W_LOG2 = 4 }; };
template <> struct jda_mode_traits<JDA_MODE_422>  { enum { NLUMA = 2, NBLK = 4, MCU_W = 16, MCU_H = 8, MCU_W_LOG2 = 4 }; };   // Y0 Y1 (side by side) Cb Cr
template <> struct jda_mode_traits<JDA_MODE_440>  { enum { NLUMA = 2, NBLK = 4, MCU_W = 8, MCU_H = 16, MCU_W_LOG2 = 3 }; };   // Y0 Y1 (one above the other) Cb Cr

// LDS copy of the table blob (one per workgroup): DC LUTs, the SHORT halves of the AC LUTs (codes
// that do not start with six 1 bits; the long halves are rare and stay in global memory),
// quantisers, zigzag.
#define JDA_LT_DC      0         // 2 x 1024
#define JDA_LT_AC      2048      // 2 tables x (1024 short + 1024 long) uint16, re-laid out while staging (jda_ac_entry): the long half
                                 // (codes starting 111111, the reference's usHuffAC[1024 + ..]) right behind the short one, so that ONE
                                 // 11-bit key finds an entry: (w >> 22) for a short code, (w >> 16) & 0x7ff = 1024 + the next 10 bits for a long one
// The prescaled quantiser tables (4 x 64 int16) sit in the DC LUTs' unused bytes: a DC LUT (the reference's layout, jpeg.inl:1098-1152)
// is indexed 0..61 and 128..255 (+ 512 for the folded values), so bytes 256..511 of each 1024-byte LUT are never read --
// room for two 128-byte tables each.  512 bytes less per workgroup is what lets 16 wavefronts of the 64-block tile layouts fit.
#define JDA_LT_QUANT_OFF(q) ((((q) >> 1) * 1024u) + 256u + (((q) & 1u) * 128u))
#define JDA_LT_NIB     96        // 16 x uint16: the set bits of a nibble, lowest first, as 3-bit fields (jda_p1_lists); same DC LUT bytes
#define JDA_LT_EOB     64        // 2 x uint32: JDA_TB_EOB, in never-read bytes of DC LUT 0
#define JDA_LT_ZZ      10240     // 144 x uint16, built while staging: where the coefficient at zigzag position j goes
#define JDA_ZZ_ENTRIES 144       //   j < 64: (column bit 1 << (n & 7)) << 8 | 2 n (n = natural index: the byte offset in the
                                 //   block); j >= 64 (past the block, or 64 + j for a symbol that stores nothing): 128 = the
                                 //   block's padding, no flags.  j <= 63 + 15 + 64.
#define JDA_ZZ_DUMP    134u      // (the last two of the slot's eight pad bytes; bytes 128..131 are the block's shared flag word in P1's chunked mode)
#define JDA_SLOT_FLAGS  128u      // byte offset in a block's slot: OR of the flag words of the chunks other lanes decoded (jda_p1c_*)
#define JDA_LT_BYTES   10528
#define JDA_LT_LONG_BYTES 0           // (the long halves are part of JDA_LT_AC now)

// AC LUT entry as the kernels keep it in LDS, made from the reference's (length << 8) | RS:
//   (length - 1) << 12 | S << 8 | Z,   Z = 2 (R + 64 nostore)  -- or 0xff for EOB, 0xfe for "no such code" (raw 0)
// (a code has 1..16 bits: four bits hold length - 1)
// nostore = a symbol with S == 0 that is not EOB (ZRL).  Z is the byte offset the symbol adds to the zigzag lookup
// (2-byte entries): R + 64 steers it to the padding entry, so the store needs no condition (jpeg.inl:2246-2256:
// "if (S && k < limit)"), and bits 4:1 of Z are still R for the position update.  One byte compare finds EOB.
#define JDA_AC_EOB 0xffu
#define JDA_AC_NONE 0xfeu
#define JDA_AC_STOPS(e) (((e) & 0xfeu) == 0xfeu)      // EOB or no code: the block's symbols end here
JDA_HD uint32_t jda_ac_entry(uint32_t raw)
{
    const uint32_t rs = raw & 0xffu, len = raw >> 8;
    if (len == 0u) return JDA_AC_NONE;
    if (rs == 0u) return ((len - 1u) << 12) | JDA_AC_EOB;
    const uint32_t r = rs >> 4, sz = rs & 0xfu;
    return ((len - 1u) << 12) | (sz << 8) | ((r + (sz == 0u ? 64u : 0u)) << 1);
}

#ifndef JDA_LONG_LDS_MODES
#define JDA_LONG_LDS_MODES 0x1fu     // bit per JDA_MODE_*: the layouts that stage the long AC halves
#endif
// The per-WAVE region.  BIG = 1: one wavefront less per workgroup, its LDS shared out as a larger scan window -- the kernel
// variant for high-bitrate images (a tile whose slice of the scan does not fit the window takes the general reader, which
// goes to HBM at every refill: 3-4x slower in P1).
template <int MODE, int BIG = 0> struct jda_lds_layout {
    enum {
        // MCUs per tile: 10 (4:2:0) / 20 (4:4:4) / 16 / 64.  4:4:4 takes 20 of the 21 that would fit: 160 pixels = 640-byte rows of
        // RGB8888 (whole 128-byte lines: 168-pixel tiles wrote 1.9 % more than they stored) and 320 colour-stage items = exactly five passes
        MCUS = MODE == JDA_MODE_444 ? 20 : JDA_TILE_THREADS / jda_mode_traits<MODE>::NBLK,
        BLOCKS = MCUS * jda_mode_traits<MODE>::NBLK,                 // blocks per tile: 60 / 63 / 64
        // one 136-byte slot per block: int16[64] coefficients, later (first 64 bytes) its 8x8 samples --
        // the row stage stores its bytes over the block it has just read, as the reference does (:2682)
        COEF_OFF = 0,
        ROWLIST_OFF = COEF_OFF + BLOCKS * JDA_COEF_STRIDE,          // 64 block ids (uint8), grouped by row class
        CNT_OFF = ROWLIST_OFF + JDA_TILE_THREADS,                   // 8 uint32 counters
        // the column list comes last, and the scan window lies over it and over everything that is left of the wavefront's
        // share of the LDS behind it.  (A block writes eight column items whatever it has (jda_p1_lists), up to seven past
        // the list's end: window bytes, dead by then.)
        COLLIST_OFF = (CNT_OFF + 32 + 15) / 16 * 16,                // uint16 items
        COLLIST_ENTRIES = BLOCKS * 8,                               // every column of every block
        WIN_OFF = COLLIST_OFF,
        BASE_BYTES = COLLIST_OFF + COLLIST_ENTRIES * 2 + 16,        // what a wavefront needs at least
        PLANE_OFF = COEF_OFF,
        PLANE_STRIDE = jda_mode_traits<MODE>::NBLK * JDA_COEF_STRIDE, // bytes between consecutive MCUs' samples
        // Codes that start 111111 -- every code of 10 bits and more of the Annex K tables -- are looked up in the long halves of
        // the AC LUTs.  They are some percent of the symbols, i.e. SOME lane of a wavefront meets one in most trips of the
        // entropy loop: from the table blob in HBM that was a global load per trip, behind a wait that also drains the
        // tile's output stores.  So the long halves are staged too
        LONG_LDS = 1,
        TAB_BYTES = JDA_LT_BYTES,
        // wavefronts per workgroup = per CU: as many as fit in the 160 KB of LDS next to one table copy (and the 16-byte draw
        // counter), 16 at most; every wavefront gets an equal share of what is there, and what it does not need is window
        LDS_FREE = 160 * 1024 - TAB_BYTES - 16,
        WAVES_MAX = LDS_FREE / BASE_BYTES > 16 ? 16 : LDS_FREE / BASE_BYTES,
        WAVES = WAVES_MAX - BIG,
        WAVE_BYTES = LDS_FREE / WAVES / 16 * 16,                    // 9,568 B (4:2:0), 10,208 B with BIG
        WIN_BYTES = WAVE_BYTES - WIN_OFF > 2048 ? 2048 : WAVE_BYTES - WIN_OFF,     // 1,312 B (4:2:0), 1,952 B with BIG
        WIN_CHUNKS = (WIN_BYTES + 1023) / 1024                      // 16-byte chunks a lane copies when the window is staged
    };
};

// ---- small helpers ---------------------------------------------------------------------------
// type-punned wide accesses to the int16 / uint8 LDS arrays must not be reordered by TBAA
typedef uint64_t __attribute__((may_alias)) jda_u64_alias;
typedef uint32_t __attribute__((may_alias)) jda_u32_alias;

JDA_HD uint32_t jda_alignbyte(uint32_t hi, uint32_t lo, uint32_t byte_shift)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, byte_shift);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (byte_shift & 3)));
#endif
}

// Hides a value from instruction selection.  Needed because hipcc (ROCm 7.2) fuses
//   clamp255(a >> 12) | clamp255(b >> 12) << 8   into gfx950's v_ashr_pk_u8_i32 and then treats
// the result as a zero-extended 16-bit value, but the instruction leaves garbage in bits 31:16
// (observed on MI355X: low bits of the blue channel corrupted).  Breaking the pattern costs nothing.
#if defined(__HIP_DEVICE_COMPILE__)
#define JDA_OPAQUE(x) asm("" : "+v"(x))
#define JDA_STORE_ORDER() asm volatile("" ::: "memory")      // the compiler keeps memory accesses on their side of it (LDS serves a wavefront's accesses in order)
#else
#define JDA_OPAQUE(x) ((void)0)
#define JDA_STORE_ORDER() ((void)0)
#endif

// The host side of a fork computes what the device side's instruction gives for EVERY input (tests/devprims holds the two sides
// together); a domain the callers keep to stands in a comment, not in a looser formula.
// bits 23:0 of a word, sign-extended: the operand of the 24-bit multiplier (v_mul_i32_i24, v_mad_i32_i24)
JDA_HD int32_t jda_sext24(int32_t v) { return (int32_t)((uint32_t)v << 8) >> 8; }

// ---- packed 16-bit helpers (two pixels per VALU instruction in the colour stage) ---------------
// v_perm_b32: result byte i = byte (sel >> 8i & 0xff) of the 8-byte pool {hi = bytes 4-7, lo = bytes 0-3};
// selectors 8, 9, 10, 11 give the replicated bit 15 of lo, 31 of lo, 15 of hi, 31 of hi, selector 0x0c gives 0x00 and
// 0x0d and above give 0xff.  (The callers use 0..7, 0x0c and 0x0d.)
JDA_HD uint32_t jda_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t pool = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t k = (sel >> (8 * i)) & 0xffu;
        const uint32_t b = k < 8 ? (uint32_t)(pool >> (8 * k)) & 0xffu
                         : k < 12 ? (((pool >> (16 * (k - 8) + 15)) & 1u) ? 0xffu : 0u) : (k == 0x0c ? 0u : 0xffu);
        r |= b << (8 * i);
    }
    return r;
#endif
}
// two independent 16-bit adds (v_pk_add_u16)
JDA_HD uint32_t jda_pk_add16(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short jda_us2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(jda_us2, a) + __builtin_bit_cast(jda_us2, b));
#else
    return ((a + b) & 0xffffu) | ((a & 0xffff0000u) + (b & 0xffff0000u));
#endif
}
// two independent 16-bit subtracts (v_pk_sub_u16)
JDA_HD uint32_t jda_pk_sub16(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short jda_us2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(jda_us2, a) - __builtin_bit_cast(jda_us2, b));
#else
    return ((a - b) & 0xffffu) | (((a & 0xffff0000u) - (b & 0xffff0000u)) & 0xffff0000u);
#endif
}
// a.lo + b.hi and a.hi + b.hi (v_pk_add_u16 with op_sel: the second operand's UPPER half feeds both lanes -- a value that sits in
// bits 31:16 of a word is added to a pixel pair without being copied into the lower half first)
JDA_HD uint32_t jda_pk_add16_bhi(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_pk_add_u16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    const uint32_t h = b >> 16;
    return ((a + h) & 0xffffu) | ((a + (h << 16)) & 0xffff0000u);
#endif
}
// a.lo + b.lo, a.lo + b.hi  /  a.hi + b.lo, a.hi + b.hi (v_pk_add_u16 with op_sel on the FIRST operand: one half of it feeds both lanes --
// one pixel's luma sample is added to its red and green terms in one instruction)
JDA_HD uint32_t jda_pk_add16_alo(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_pk_add_u16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    const uint32_t l = a & 0xffffu;
    return ((l + b) & 0xffffu) | (((l << 16) + (b & 0xffff0000u)) & 0xffff0000u);
#endif
}
JDA_HD uint32_t jda_pk_add16_ahi(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_pk_add_u16 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    const uint32_t h = a >> 16;
    return ((h + b) & 0xffffu) | (((h << 16) + (b & 0xffff0000u)) & 0xffff0000u);
#endif
}
// Two bytes of LDS `delta` apart, at p + step, read through an address of their own (ds_read_u8 x 2): the compiler joins neighbouring
// byte loads into wider loads and spends a VALU instruction per byte on taking them apart again -- the colour stage is bound by
// its VALU instructions more than by its LDS accesses.  The address is made where it is used (one add; asm volatile: a copy kept in
// a register across the tile loop per pass of the colour stage sent the general kernels' registers to scratch memory).
JDA_HD void jda_lds_bytes_apart(const uint8_t *p, uint32_t step, uint32_t delta, uint32_t &b0, uint32_t &b1)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t a;
    asm volatile("v_add_u32 %0, %1, %2" : "=v"(a) : "v"((uint32_t)(uintptr_t)p), "v"(step));
    const uint8_t __attribute__((address_space(3))) *q = (const uint8_t __attribute__((address_space(3))) *)a;
    b0 = q[0]; b1 = q[delta];
#else
    b0 = p[step]; b1 = p[step + delta];
#endif
}
// a * b + c on operands that fit in 24 signed bits (v_mad_i32_i24, full rate: bits 23:0 of a and of b, sign-extended; the
// low 32 bits of their product, + c)
JDA_HD int32_t jda_mad24(int32_t a, int32_t b, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b) + c;
#else
    return (int32_t)((uint32_t)jda_sext24(a) * (uint32_t)jda_sext24(b) + (uint32_t)c);
#endif
}
// per 16-bit lane: the sign-extended 10-bit field at bits 14:5  (v_pk_lshlrev_b16 1, v_pk_ashrrev_i16 6)
JDA_HD uint32_t jda_pk_sext10_at5(uint32_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short jda_s2 __attribute__((ext_vector_type(2)));
    jda_s2 v = __builtin_bit_cast(jda_s2, a);
    v = v << 1;
    v = v >> 6;
    return __builtin_bit_cast(uint32_t, v);
#else
    const int32_t lo = (int16_t)(uint16_t)((a & 0xffffu) << 1) >> 6, hi = (int16_t)(uint16_t)(((a >> 16) & 0xffffu) << 1) >> 6;
    return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
#endif
}
// per 16-bit lane: the range limit of a sample, ucRangeTable[(v >> 5) & 0x3ff] = clamp(sext10(v >> 5) + 128) (jpeg.inl:159-222), in
// three packed instructions: v * 2 + 0x8000 modulo 2^16 (v_pk_mad_u16) puts the 10-bit field at bits 15:6 in OFFSET-BINARY form
// (signed value + 512; bit 15 of v, which the table's index drops, falls out), subtracting 384 << 6 with unsigned saturation
// (v_pk_sub_u16 clamp) leaves max(value + 128, 0) << 6 in 0..639 << 6, and x 4 with unsigned saturation (v_pk_mad_u16 clamp) caps
// it at 255 in the lane's HIGH byte (the low byte is junk; the byte permute that assembles a row picks bytes 1 and 3).
// (Rounds 3-5 added the offset -- 512 << 5 -- to the DC term of the column stage instead: a compare and a select per column item
// that the multiply-add's third operand does for nothing.)
JDA_HD uint32_t jda_pk_limit10(uint32_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short jda_us2 __attribute__((ext_vector_type(2)));
    uint32_t r, flip = 0x80008000u, four = 4u;
    asm("v_pk_mad_u16 %0, %1, 2, %2 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(flip));      // the field to bits 15:6, its sign bit flipped
    jda_us2 v = __builtin_bit_cast(jda_us2, r);
    const jda_us2 k = { 24576, 24576 };
    v = __builtin_elementwise_sub_sat(v, k);                // max(value + 128, 0) << 6          (v_pk_sub_u16 clamp)
    r = __builtin_bit_cast(uint32_t, v);
    asm("v_pk_mad_u16 %0, %1, %2, 0 op_sel_hi:[1,0,0] clamp" : "=v"(r) : "v"(r), "v"(four));   // x 4, saturating: high byte = min(.., 255)
    return r;
#else
    uint32_t r = 0;
    for (int h = 0; h < 2; h++) {
        uint32_t x = (((a >> (16 * h)) << 1) + 0x8000u) & 0xffffu;
        x = x > 24576u ? x - 24576u : 0u;
        x *= 4u;
        if (x > 0xffffu) x = 0xffffu;
        r |= x << (16 * h);
    }
    return r;
#endif
}
// two signed 16-bit values -> two bytes saturated to 0..255 in bits 15:0, bits 31:16 zero (v_sat_pk_u8_i16)
JDA_HD uint32_t jda_sat_pk_u8(uint32_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_sat_pk_u8_i16 %0, %1" : "=v"(r) : "v"(a));
    return r;
#else
    const int32_t lo = (int16_t)(a & 0xffffu), hi = (int16_t)(a >> 16);
    const uint32_t l = lo < 0 ? 0u : (lo > 255 ? 255u : (uint32_t)lo), h = hi < 0 ? 0u : (hi > 255 ? 255u : (uint32_t)hi);
    return l | (h << 8);
#endif
}

// low 32 bits of the product of two values below 2^24 (v_mul_u32_u24, full rate)
JDA_HD uint32_t jda_umul24(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return (a & 0xffffffu) * (b & 0xffffffu);
#endif
}
// a byte in all four bytes of a word (one v_perm_b32 where `x * 0x01010101` is a quarter-rate v_mul_lo_u32)
JDA_HD uint32_t jda_dup8(uint32_t v) { return jda_perm(0, v, 0x00000000u); }
// sum of the four byte products a.b[i] * b.b[i]  (v_dot4_u32_u8)
JDA_HD uint32_t jda_udot4(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, 0u, false);
#else
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) r += ((a >> (8 * i)) & 0xffu) * ((b >> (8 * i)) & 0xffu);
    return r;
#endif
}
JDA_HD uint32_t jda_udot4_acc(uint32_t a, uint32_t b, uint32_t c)      // a . b + c (bytes, unsigned)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    return jda_udot4(a, b) + c;
#endif
}
JDA_HD uint32_t jda_dup16(int32_t v) { return jda_perm(0, (uint32_t)v, 0x01000100u); }        // low half in both halves
JDA_HD uint32_t jda_pack16(int32_t lo, int32_t hi) { return jda_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u); }

// sign-extended 10-bit field starting at bit `lo` (the reference's "& 0x3ff" table index)
JDA_HD int32_t jda_sext10_at(int32_t v, int lo) { return (int32_t)((uint32_t)v << (22 - lo)) >> 22; }
JDA_HD int32_t jda_clamp255(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// ucRangeTable[(v >> 5) & 0x3ff]  (jpeg.inl:159-222, 2786-2793)
JDA_HD uint32_t jda_range_limit5(int32_t v) { return (uint32_t)jda_clamp255(jda_sext10_at(v, 5) + 128); }

// 64-bit big-endian window at an arbitrary byte position (MOTOLONG, src/JPEGDEC.h:316-318),
// assembled from three aligned dword loads.
JDA_HD uint64_t jda_be64_from_words(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t pos)
{
    // byte alignment and byte swap in one permute per half: result byte 3 = stream byte sh, .. byte 0 = stream byte sh + 3
    // 0x00010203 + (pos & 3) * 0x01010101 without the multiply: four bytes of the descending run 6 5 4 3 2 1 0
    const uint32_t sel = jda_alignbyte(0x00000102u, 0x03040506u, ~pos);
    return ((uint64_t)jda_perm(w1, w0, sel) << 32) | jda_perm(w2, w1, sel);
}

// The workgroup's view of the filtered scan: bytes [win_lo, win_lo + win_len) are staged in LDS (copied
// with coalesced 16-byte loads by jda_window_fill); anything beyond is read from HBM directly.
struct jda_bitreader {
    const uint8_t JDA_GLOBAL *base;     // filtered scan in global memory (4-byte aligned, zero padded)
    const uint8_t *win;      // LDS copy
    uint32_t win_lo;         // 16-byte aligned scan offset of win[0]
    uint32_t win_len;        // bytes staged (multiple of 16)
    uint32_t pos;            // bb.pBuf - start of filtered scan
    uint32_t off;            // bb.ulBitOff
    uint64_t bits;           // bb.ulBits
};

JDA_HD uint64_t jda_load_be64(const jda_bitreader &br, uint32_t pos)
{
    const uint32_t a = pos & ~3u;
    const uint32_t rel = a - br.win_lo;
    if (rel + 12u <= br.win_len) {                      // (a < win_lo wraps to a huge rel: falls through)
        // the LDS window holds the stream as byte-swapped dwords (jda_window_store): only the byte alignment is left
        const jda_u32_alias *p = (const jda_u32_alias *)(br.win + rel);
        const uint32_t sel = jda_alignbyte(0x08070605u, 0x04030201u, ~pos);      // 0x07060504 - (pos & 3) * 0x01010101
        return ((uint64_t)jda_perm(p[0], p[1], sel) << 32) | jda_perm(p[1], p[2], sel);
    }
    const jda_u32_alias JDA_GLOBAL *p = (const jda_u32_alias JDA_GLOBAL *)(br.base + a);
    return jda_be64_from_words(p[0], p[1], p[2], pos);
}

JDA_HD void jda_refill(jda_bitreader &br)
{
    if (br.off > 47) {                                   // jpeg.inl:2110-2114 (REGISTER_WIDTH-17)
        br.pos += br.off >> 3;
        br.off &= 7;
        br.bits = jda_load_be64(br, br.pos);
    }
}

// Cooperative copy of the tile's part of the scan into the wave's LDS window: lane l copies the
// 16-byte chunks l, l+64, ...  Every lane of the wave calls it; a wave fence follows.
struct jda_chunk16 { uint32_t w[4]; };
typedef jda_chunk16 __attribute__((may_alias)) jda_chunk16_alias;
// the same copy split in two so the HBM load can be issued early and the LDS store done late
// (the window is NCH x 64 lanes x 16 bytes at most: lane l copies chunks l, l + 64, ..)
template <int NCH> struct jda_chunks { jda_chunk16 c[NCH]; };
template <int NCH>
JDA_HD jda_chunks<NCH> jda_window_load(const uint8_t JDA_GLOBAL *scan, uint32_t win_lo, uint32_t win_len, uint32_t lane)
{
    jda_chunks<NCH> r;
    const jda_chunk16_alias JDA_GLOBAL *src = (const jda_chunk16_alias JDA_GLOBAL *)(scan + win_lo);
    // Every lane loads: one whose chunk lies behind the slice reads the slice's last chunk again (jda_window_store stores what belongs
    // to the window only).  A load under a lane condition, merged with zeros for the others, came out of the compiler as load -> wait ->
    // copy: the wavefront sat out the load's latency where the column stage was meant to cover it.
    const uint32_t n16 = win_len >> 4, last = n16 ? n16 - 1u : 0u;
#pragma unroll
    for (int k = 0; k < NCH; k++) {
        const uint32_t i = lane + 64u * (uint32_t)k;
        const jda_chunk16_alias v = src[i < last ? i : last];
        r.c[k].w[0] = v.w[0]; r.c[k].w[1] = v.w[1]; r.c[k].w[2] = v.w[2]; r.c[k].w[3] = v.w[3];
    }
    return r;
}
template <int NCH>
JDA_HD void jda_window_store(uint8_t *win, uint32_t win_len, uint32_t lane, const jda_chunks<NCH> &r)
{
    jda_chunk16_alias *dst = (jda_chunk16_alias *)win;
#pragma unroll
    for (int k = 0; k < NCH; k++)
        if (lane + 64u * (uint32_t)k < (win_len >> 4)) {
            jda_chunk16_alias v;                        // every dword with the stream's first byte on top: P1's bit buffer takes them as they are
            v.w[0] = __builtin_bswap32(r.c[k].w[0]); v.w[1] = __builtin_bswap32(r.c[k].w[1]); v.w[2] = __builtin_bswap32(r.c[k].w[2]); v.w[3] = __builtin_bswap32(r.c[k].w[3]);
            dst[lane + 64u * (uint32_t)k] = v;
        }
}

JDA_HD void jda_window_fill(const uint8_t JDA_GLOBAL *scan, uint32_t win_lo, uint32_t win_len, uint8_t *win, uint32_t lane)
{
    const jda_chunk16_alias JDA_GLOBAL *src = (const jda_chunk16_alias JDA_GLOBAL *)(scan + win_lo);
    jda_chunk16_alias *dst = (jda_chunk16_alias *)win;
    for (uint32_t i = lane; i < (win_len >> 4); i += JDA_TILE_THREADS) {
        jda_chunk16_alias v = src[i];
        v.w[0] = __builtin_bswap32(v.w[0]); v.w[1] = __builtin_bswap32(v.w[1]); v.w[2] = __builtin_bswap32(v.w[2]); v.w[3] = __builtin_bswap32(v.w[3]);
        dst[i] = v;
    }
}

// EXTEND of the next s bits of the (un-refilled) window (jpeg.inl:2249-2252, 2155-2158)
JDA_HD int32_t jda_take_extend(uint64_t bits, uint32_t off, uint32_t s)
{
    const uint32_t top = (uint32_t)((bits << off) >> 32);      // zeros enter when off + s > 64
    const uint32_t v = top >> (32 - s);
    return (top & 0x80000000u) ? (int32_t)v : (int32_t)v - (int32_t)((1u << s) - 1u);
}

// ---- wave-level combine (list building without LDS atomics) -------------------------------------
// On the GPU these are DPP / ballot operations over the 64 lanes of the wavefront.  The host emulator
// steps lanes one after another, so it hands in the value of every lane (all[]) and the same results
// are computed by plain loops.
// Exclusive prefix sum of v over the lanes below `lane`, and the sum over all lanes.
JDA_HD uint32_t jda_wave_excl_sum(uint32_t v, uint32_t lane, const uint32_t *all, uint32_t &total)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)all; (void)lane;
    int x = (int)v;                                  // inclusive scan: row_shr 1,2,4,8 then row_bcast 15 / 31 (gfx9 DPP)
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    total = (uint32_t)__builtin_amdgcn_readlane(x, 63);
    return (uint32_t)x - v;
#else
    uint32_t below = 0, sum = 0;
    for (uint32_t l = 0; l < JDA_TILE_THREADS; l++) { if (l < lane) below += all[l]; sum += all[l]; }
    total = sum;
    return below;
#endif
}
// How many lanes below `lane` have cls[l] == c, and how many lanes in all (c = 0..3; cls 4 = none).
JDA_HD uint32_t jda_wave_class_rank(uint32_t my_cls, uint32_t c, uint32_t lane, const uint32_t *all_cls, uint32_t &count)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)all_cls; (void)lane;
    const uint64_t m = __builtin_amdgcn_ballot_w64(my_cls == c);
    count = (uint32_t)__builtin_popcountll(m);
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#else
    uint32_t below = 0, n = 0;
    for (uint32_t l = 0; l < JDA_TILE_THREADS; l++) if (all_cls[l] == c) { n++; if (l < lane) below++; }
    count = n;
    return below;
#endif
}

JDA_HD uint32_t jda_popcount8(uint32_t v)
{
    return (uint32_t)__builtin_popcount(v & 0xffu);
}

// ---- Huffman / RLE expand of one 8x8 block (jpeg.inl:2090-2274) ------------------------------
// LIMIT: 64 = store every coefficient; 5 = 1/4 scale (zigzag 1..4 only, jpeg.inl:2117-2119);
//        1 = 1/8 scale: only the DC term is wanted.
// Because every block has its own index entry, decoding may stop as soon as the wanted
// coefficients are known (the reference has to walk to EOB to find the next block).
// coef: the block's int16[64] in LDS (natural order).  Returns the reference's u16MCUFlags.
struct jda_tables {
    const uint8_t *dc;        // LDS: 1024-byte DC LUT of this block's component
    const uint16_t *ac_short; // LDS: 1024 entries in the jda_ac_entry layout
    const uint16_t JDA_GLOBAL *ac_long;  // global: 1024 entries (codes starting 111111), the reference's layout
    const uint16_t *ac_long_lds;         // LDS: the same in the jda_ac_entry layout (layouts with LONG_LDS)
    const uint16_t *zz;       // LDS: JDA_ZZ_ENTRIES entries (see JDA_LT_ZZ)
    uint32_t eob_sh, eob_code;   // the window-only reader finds EOB by comparing stream bits (jda_lane_pre)
};

// The index entry of a block is the reader at its FIRST AC SYMBOL (after the refill at the top of the AC loop, jpeg.inl:2225-2230) and
// its DC value comes with it (index format 2: both pre-scans decode the DC symbol, jpeg.inl:2129-2165, as they pass it), so a block's
// decode starts with coefficient 1.
// exact: the block is flagged JDA_INDEX_TRUNC -- its index entry is the reference reader's true phase, and magnitude reads lose the
// bits the reference's window does not hold.  An unflagged block's entry may be canonical (the device pre-scan's: same bit
// position, another phase), and the reference truncates nothing in it: the reader refills instead of reading short.
template <int LIMIT>
JDA_HD uint32_t jda_decode_block(jda_bitreader &br, const jda_tables &T, int16_t *coef, int32_t dc, bool exact = true)
{
    uint32_t flags = 0;
    if (LIMIT == 64) {
        jda_u64_alias *z = (jda_u64_alias *)coef;       // memset(pMCU, 0, 128)  :2121
#pragma unroll
        for (int i = 0; i < 16; i++) z[i] = 0;
    } else if (LIMIT == 5) {
        coef[1] = 0; coef[8] = 0; coef[9] = 0;          // :2118
    }
    coef[0] = (int16_t)dc;
    // AC  (:2223-2265).  The reference refills at the top AND the bottom of every iteration; the top
    // one is a no-op after a bottom one, so one refill before the loop + one per iteration is identical.
    uint32_t code, e;
    int k = 1;
    jda_refill(br);
    while (k < LIMIT) {
        code = (uint32_t)(br.bits >> (48 - br.off)) & 0xffffu;
        if (code >= 0xfc00u) e = T.ac_long_lds[code & 0x3ffu];               // usHuffAC[1024 + ...]  :2232-2233
        else e = T.ac_short[code >> 6];
        if (JDA_AC_STOPS(e)) break;                     // EOB (no refill follows; the block's reader state is not needed any more)
        br.off += (e >> 12) + 1u;
        k += (int)((e >> 1) & 0xfu);
        const uint32_t ms = (e >> 8) & 0xfu;
        if (!exact && br.off + ms > 64u) { br.pos += br.off >> 3; br.off &= 7u; br.bits = jda_load_be64(br, br.pos); }
        if (k < LIMIT && ms) {
            const uint32_t n = (T.zz[k] & 0xffu) >> 1;
            flags |= (1u << (n & 7u)) | (n << 8);
            coef[n] = (int16_t)jda_take_extend(br.bits, br.off, ms);
        }
        br.off += ms;
        k++;
        jda_refill(br);
    }
    return flags;
}

// ---- the same, for a tile whose whole scan slice is in the LDS window (the normal case) ----------
// No lane can leave the window, so the reader needs no bounds check and no HBM path, and the block
// decode below is written without divergent branches: P1 is bound by the latency of its dependent
// chain (stream bits -> LUT -> bit offset -> stream bits), not by instruction issue, and every
// exec-mask region in that chain costs a VALU->SALU->branch round trip.
// x >> n for n in 0..31, as the hardware's shift takes it: n mod 32.  n == 32 gives x, not 0 -- on the host too (it used to give 0 there,
// and a caller that used the result was right in the emulator and wrong on the GPU: jda_q4_block) -- so no caller may use that result
JDA_HD uint32_t jda_shr_upto32(uint32_t x, uint32_t n) { return x >> (n & 31u); }
// EXTEND (jpeg.inl:2249-2252) of the s bits at the top of the 32-bit word t, s = 1 .. 31 (s == 0: t itself, see above -- a symbol
// without magnitude bits has no value)
JDA_HD int32_t jda_extend_top(uint32_t t, uint32_t s)
{
    const uint32_t v = jda_shr_upto32(t, 32u - s);
    const uint32_t neg = ~(uint32_t)((int32_t)t >> 31);          // all ones when the leading bit is 0
    return (int32_t)(v + (neg & ((0xffffffffu << s) + 1u)));
}

// The reader of the window-only path (the window in LDS holds byte-swapped dwords, so they are taken as they are).
// The window-only reader keeps ONE number: the position of the last consumed bit (GPU: counted from LDS address 0, so that the
// dword it sits in is at byte address (m >> 3) & ~3).  A peek reads that dword and the next (one ds_read2_b32) and funnel-shifts;
// consuming n bits is m += n.  Five instructions a symbol where sliding hi / lo / next by selects took nine; the price is a second
// LDS read on the symbol's dependent chain.
struct jda_wreader {
    uint32_t m;              // bits up to and including the last consumed one (window start = LDS address * 8; host: = 0), minus 1
    const uint8_t *base;     // host emulator: the window's first byte
};
// a + (b & 0xff) in one instruction (the byte select rides on the add: SDWA)
JDA_HD uint32_t jda_add_byte0(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(a), "v"(b));
    return r;
#else
    return a + (b & 0xffu);
#endif
}
// v_bfe_u32: (v >> off) & ((1 << width) - 1), off + width <= 32, width <= 31 (the instruction takes off & 31 and width & 31: a width
// of 32 is a width of 0)
JDA_HD uint32_t jda_bfe(uint32_t v, uint32_t off, uint32_t width)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ubfe(v, off, width);
#else
    return (v >> (off & 31u)) & ((1u << (width & 31u)) - 1u);
#endif
}
JDA_HD uint32_t jda_alignbit(uint32_t hi, uint32_t lo, uint32_t sh)      // low 32 bits of {hi, lo} >> sh, sh = 0..31
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u));
#endif
}
JDA_HD void jda_wr_init(jda_wreader &R, const uint8_t *wbase, uint32_t pos, uint32_t off)
{
    // (for bit 0 of the window the last consumed bit is in the four bytes in front of it -- other LDS data, all "consumed")
#if defined(__HIP_DEVICE_COMPILE__)
    R.m = ((uint32_t)(uintptr_t)wbase << 3) + (pos << 3) + off - 1u;       // (the window is 16-byte aligned and not at LDS address 0)
    R.base = wbase;
#else
    R.m = (pos << 3) + off - 1u;
    R.base = wbase;
#endif
}
JDA_HD uint32_t jda_wr_peek(const jda_wreader &R)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t a = (R.m >> 3) & ~3u;
    const uint32_t __attribute__((address_space(3))) *p = (const uint32_t __attribute__((address_space(3))) *)a;
    return jda_alignbit(p[0], p[1], ~R.m);                         // (- (m + 1)) & 31 bits of the first dword are consumed
#else
    const uint8_t *p = R.base + (((int32_t)R.m >> 5) * 4);
    return jda_alignbit(*(const jda_u32_alias *)p, *(const jda_u32_alias *)(p + 4), ~R.m);
#endif
}
JDA_HD void jda_wr_consume(jda_wreader &R, uint32_t n) { R.m += n; }
// the reference's refill (jpeg.inl:2110-2114) as far as its ulBitOff is concerned
JDA_HD uint32_t jda_ref_refill(uint32_t roff) { return roff > 47u ? (roff & 7u) : roff; }

// LDS accesses by 32-bit address in the entropy loop (GPU): the zigzag lookup and the deferred coefficient store take their
// address from an SDWA add (a + byte 0 of b), which the compiler can only keep in the LDS address space if it is told so
#if defined(__HIP_DEVICE_COMPILE__)
#define JDA_LDS_A32(p) ((uint32_t)(uintptr_t)(p))
#define JDA_LDS_LOAD_U16(base_ptr, a32) ((uint32_t)*(const uint16_t __attribute__((address_space(3))) *)(a32))
#define JDA_COEF_STORE(coef, t, v) (*(int16_t __attribute__((address_space(3))) *)jda_add_byte0(JDA_LDS_A32(coef), (t)) = (int16_t)(v))
#else
#define JDA_LDS_A32(p) 0u
#define JDA_LDS_LOAD_U16(base_ptr, a32) ((uint32_t)*(const uint16_t *)((const uint8_t *)(base_ptr) + (a32)))
#define JDA_COEF_STORE(coef, t, v) (*(int16_t *)((uint8_t *)(coef) + ((t) & 0xffu)) = (int16_t)(v))
#endif
// EXACT = false leaves the reference's ulBitOff out (five instructions and a branch less per symbol): only right for a block
// in which the reference truncates no magnitude read, i.e. one whose index entry lacks JDA_INDEX_TRUNC.
// zero_fill: clear the block first.
// trunc: this lane's block is the flagged one (EXACT runs for the whole wavefront when any lane's is).
template <int LIMIT, bool EXACT, bool LONG_LDS>
JDA_HD uint32_t jda_decode_block_win(uint32_t pos, uint32_t off, const uint8_t *wbase, const jda_tables &T, int16_t *coef, int32_t dc, bool zero_fill, bool trunc = true)
{
    jda_wreader R;
    jda_wr_init(R, wbase, pos, off);
    uint32_t fl = 0;                                     // OR of zz entries of the stored coefficients
    uint32_t roff = EXACT ? jda_ref_refill(off) : 0u;   // the reference's ulBitOff at the block's first AC symbol
    // (the pre-scan decoded the DC symbol, jpeg.inl:2129-2165: the entry points behind it, the value rides on the block's clearing)
    if (LIMIT == 64 && zero_fill) {
#if defined(__HIP_DEVICE_COMPILE__)
        // (the block's address in ONE register the compiler cannot see through: sixteen stores at offsets 0 .. 120 from it -- left to
        // itself it folds the wavefront's constant part of the address into every store and adds it back seven times)
        uint32_t za = JDA_LDS_A32(coef);
        asm volatile("" : "+v"(za));
        jda_u64_alias __attribute__((address_space(3))) *z = (jda_u64_alias __attribute__((address_space(3))) *)za;
#else
        jda_u64_alias *z = (jda_u64_alias *)coef;
#endif
        z[0] = (uint64_t)(uint16_t)dc;
#pragma unroll
        for (int i = 1; i < 16; i++) z[i] = 0;
    } else {
        if (LIMIT == 5) { coef[1] = 0; coef[8] = 0; coef[9] = 0; }
        coef[0] = (int16_t)dc;
    }
    uint32_t w, e;
    const uint32_t zzb = JDA_LDS_A32(T.zz);              // (GPU: the zigzag table's LDS address rides in k2, so a lookup's address is one add)
    uint32_t k2 = zzb + 2;                               // twice the zigzag position: the byte offset into the zigzag table
    // EOB is recognised on the stream bits themselves -- one code per table, checked by the host (JDA_DESC_GENERAL_P1) --
    // before the symbol is looked up: a block costs one trip per coefficient symbol, none for its EOB, and the wavefront
    // runs as many trips as its longest block needs.  (A block of a decoded MCU holds no invalid code: the pre-scan ends
    // the image at the first bad MCU.)
    // A symbol's value is stored one trip later, while the next symbol's lookup is under way: the zigzag entry it needs was
    // asked for a trip earlier and LDS answers in order, so the trip waits for LDS once, not twice.  (The first trip stores a
    // zero to the block's padding.)
    uint32_t t_prev = JDA_ZZ_DUMP;
    int32_t v_prev = 0;
    w = jda_wr_peek(R);
    if ((w >> T.eob_sh) != T.eob_code) for (;;) {
        // codes starting 111111 (usHuffAC[1024 + ...], :2232-2233) sit right behind the short half: one 11-bit key, one lookup,
        // no branch -- the key is a bit field whose position depends on the code's class
        e = T.ac_short[jda_bfe(w, w >= 0xfc000000u ? 16u : 22u, 11u)];
        fl |= t_prev;
        JDA_COEF_STORE(coef, t_prev, v_prev);
        // the zigzag lookup decides where the value goes: position k + R of the block, or the padding when that is past
        // the block or the symbol carries no value (ZRL: the entry's low byte reads 2 (R + 64))
        const uint32_t kk2 = jda_add_byte0(k2, e);
        uint32_t t = JDA_LDS_LOAD_U16(T.zz, kk2);
        if (LIMIT != 64 && kk2 >= zzb + 2u * (uint32_t)LIMIT) t = JDA_ZZ_DUMP;     // 1/4 scale keeps zigzag 1..4 only (:2117-2119)
        const uint32_t len = (e >> 12) + 1u, ms = (e >> 8) & 0xfu;
        uint32_t m = w << len;
        const uint32_t n = len + ms;
        if (EXACT) {
            roff += n;                                   // the reference's ulBitOff after its magnitude read (:2249-2252)
            if (__builtin_expect(roff > 64u && trunc, 0)) m &= ~(0xffffffffu >> (64u + ms - roff));      // its window ended inside the magnitude
            roff = jda_ref_refill(roff);
        }
        v_prev = jda_extend_top(m, ms);
        t_prev = t;
        jda_wr_consume(R, n);
        k2 += (e & 0x1eu) + 2u;
        w = jda_wr_peek(R);
        if (k2 >= zzb + 2u * (uint32_t)LIMIT || (w >> T.eob_sh) == T.eob_code) break;
    }
    fl |= t_prev;
    JDA_COEF_STORE(coef, t_prev, v_prev);
    // A.2: column bits in 7:0, (n << 8) bits above -- only bit 13 (some n >= 32) is ever tested; fl holds 2n in 7:0
    return (fl >> 8) | ((fl & 0x40u) << 7);
}

// ---- a CHUNK of a block: at most JDA_CONT_SYMS AC symbols from a continuation entry (or from the block's first AC symbol), so that
// the lanes of a wavefront share its long blocks (jda_p1c_*).  The loop is jda_decode_block_win's; it starts at zigzag position k0 and
// ends at EOB, behind coefficient 63 or after max_syms symbols.  Returns the OR of the zigzag entries of what it stored (the caller
// folds the chunks' words into the block's flags: jda_p1c_fold).  Only for blocks the reference reads without truncation.
JDA_HD uint32_t jda_decode_chunk_win(uint32_t bitpos, const uint8_t *wbase, const jda_tables &T, int16_t *coef, uint32_t k0, uint32_t max_syms)
{
    jda_wreader R;
    jda_wr_init(R, wbase, bitpos >> 3, bitpos & 7u);
    uint32_t fl = 0;
    const uint32_t zzb = JDA_LDS_A32(T.zz);
    uint32_t k2 = zzb + 2u * k0;
    uint32_t t_prev = JDA_ZZ_DUMP;
    int32_t v_prev = 0;
    uint32_t w = jda_wr_peek(R), left = max_syms;
    if ((w >> T.eob_sh) != T.eob_code) for (;;) {
        const uint32_t e = T.ac_short[jda_bfe(w, w >= 0xfc000000u ? 16u : 22u, 11u)];
        fl |= t_prev;
        JDA_COEF_STORE(coef, t_prev, v_prev);
        const uint32_t kk2 = jda_add_byte0(k2, e);
        const uint32_t t = JDA_LDS_LOAD_U16(T.zz, kk2);
        const uint32_t len = (e >> 12) + 1u, ms = (e >> 8) & 0xfu;
        const uint32_t m = w << len;
        v_prev = jda_extend_top(m, ms);
        t_prev = t;
        jda_wr_consume(R, len + ms);
        k2 += (e & 0x1eu) + 2u;
        w = jda_wr_peek(R);
        left--;
        if (left == 0u || k2 >= zzb + 128u || (w >> T.eob_sh) == T.eob_code) break;
    }
    fl |= t_prev;
    JDA_COEF_STORE(coef, t_prev, v_prev);
    return fl;
}
// the block's flags (A.2) from the OR of its chunks' words: column bits in 7:0, bit 13 = some coefficient in rows 4-7
JDA_HD uint32_t jda_p1c_fold(uint32_t fl) { return ((fl >> 8) & 0xffu) | ((fl & 0x40u) << 7); }

// Does some lane of the wavefront (of those that are here) say yes?  The host emulator steps the lanes one after another:
// there a lane answers for itself (the exact decoder is right for every block, the short one for every unflagged block).
JDA_HD bool jda_wave_any(bool v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(v) != 0ull;
#else
    return v;
#endif
}

// Multiplication by an IDCT constant.  FAST: both operands are known to fit in 24 signed bits (the
// host checks max|coef| * max|quant| < 2^21 for the image, see jda_frontend.cpp), so the full-rate
// 24-bit multiplier gives the exact low 32 bits; otherwise the full 32-bit multiply (quarter rate).
template <bool FAST> JDA_HD int32_t jda_mulc(int32_t x, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (FAST) return __mul24(x, c);     // v_mul_i32_i24 (hip_runtime.h is included by the .hip file)
    return x * c;
#else
    if (FAST) return (int32_t)((uint32_t)jda_sext24(x) * (uint32_t)jda_sext24(c));   // the 24-bit operands of v_mul_i32_i24
    return (int32_t)((uint32_t)x * (uint32_t)c);
#endif
}

// ---- dequant + IDCT + range limit (jpeg.inl:2553-2797) ---------------------------------------
// One 1-D pass of the reference's row stage on eight int32 inputs, block-level variant chosen by
// the occupancy flags (jpeg.inl:2686-2743).  Returns the eight range-limited bytes packed LE.
struct jda_row8 { uint32_t lo, hi; };

// RC: 0 = only columns 0-1 occupied, 1 = columns 0-3, 2 = any (the block-level tests of :2686-2688)
template <int RC>
JDA_HD jda_row8 jda_idct_row(const int32_t s[8])
{
    // The even part's four terms are only ever needed as the packed pairs (t0, t1) and (t3, t2) of the final butterflies, and only
    // modulo 2^16 (below): they are made there -- pair + pair and pair - pair -- instead of four 32-bit sums and two packs.
    int32_t t4, t5, t6, t7;
    uint32_t p01, p32;
    if (RC == 0) {                                                   // :2688-2697
        p01 = p32 = jda_dup16(s[0]);
        t7 = s[1];
        t6 = (t7 * 217) >> 8;
        t5 = (t7 * 145) >> 8;
        t4 = -((t7 * 51) >> 8);
    } else if (RC == 1) {                                            // :2698-2718
        const int32_t c = s[2];
        const int32_t m = (c * 106) >> 8;
        const uint32_t pa = jda_dup16(s[0]), pc = jda_pack16(c, m);
        p01 = jda_pk_add16(pa, pc);                                  // t0 = a + c, t1 = a + m
        p32 = jda_pk_sub16(pa, pc);                                  // t3 = a - c, t2 = a - m
        const int32_t z13 = s[3], z11 = s[1];
        t7 = z11 + z13;
        const int32_t t11 = ((z11 - z13) * 362) >> 8;
        const int32_t z5 = ((z11 - z13) * 473) >> 8;
        const int32_t t10 = ((z11 * 277) >> 8) - z5;
        const int32_t t12 = ((z13 * 669) >> 8) + z5;
        t6 = t12 - t7; t5 = t11 - t6; t4 = t10 + t5;
    } else {                                                         // :2720-2743
        const int32_t t10 = s[0] + s[4], t11 = s[0] - s[4];
        const int32_t t13 = s[2] + s[6];
        const int32_t t12 = (((s[2] - s[6]) * 362) >> 8) - t13;
        const uint32_t pe = jda_pack16(t10, t11), pf = jda_pack16(t13, t12);
        p01 = jda_pk_add16(pe, pf);                                  // t0 = t10 + t13, t1 = t11 + t12
        p32 = jda_pk_sub16(pe, pf);                                  // t3 = t10 - t13, t2 = t11 - t12
        const int32_t z13 = s[5] + s[3], z10 = s[5] - s[3];
        const int32_t z11 = s[1] + s[7], z12 = s[1] - s[7];
        t7 = z11 + z13;
        const int32_t u11 = ((z11 - z13) * 362) >> 8;
        const int32_t z5 = ((z10 + z12) * 473) >> 8;
        const int32_t u10 = ((z12 * 277) >> 8) - z5;
        const int32_t u12 = ((z10 * -669) >> 8) + z5;
        t6 = u12 - t7; t5 = u11 - t6; t4 = u10 + t5;
    }
    // :2745-2793  the eight outputs t_a +- t_b and ucRangeTable[(v >> 5) & 0x3ff], two per instruction.
    // Only bits 14:5 of an output reach the table index, so the final adds can be done modulo 2^16 on
    // packed pairs: (o0,o1) = (t0,t1) + (t7,t6), (o7,o6) = (t0,t1) - (t7,t6), (o3,o2) = (t3,t2) + (-t4,t5),
    // (o4,o5) = (t3,t2) - (-t4,t5).  Then the 10-bit sign-extended field (the table's wrap: << 1, >> 6
    // arithmetic on 16-bit lanes), + 128, saturate to a byte.
    const uint32_t q76 = jda_pack16(t7, t6), q45 = jda_pack16(-t4, t5);
    const uint32_t s01 = jda_pk_limit10(jda_pk_add16(p01, q76));      // samples in bytes 1 and 3
    const uint32_t s76 = jda_pk_limit10(jda_pk_sub16(p01, q76));
    const uint32_t s32 = jda_pk_limit10(jda_pk_add16(p32, q45));
    const uint32_t s45 = jda_pk_limit10(jda_pk_sub16(p32, q45));
    jda_row8 r;
    r.lo = jda_perm(s32, s01, 0x05070301u);          // bytes o0 o1 o2 o3  (s32 = [o3,o2])
    r.hi = jda_perm(s76, s45, 0x05070301u);          // bytes o4 o5 o6 o7  (s45 = [o4,o5], s76 = [o7,o6])
    return r;
}

// Column stage for one column (jpeg.inl:2561-2676): c[r] = raw coefficient of row r, q[r] its
// prescaled quantiser; results truncated to int16 as the reference stores them back.
template <bool FAST, bool HALF>
JDA_HD void jda_idct_col(const int32_t c[8], const int32_t q[8], int32_t out[8])
{
    int32_t t0, t1, t2, t3, t4, t5, t6, t7;
    if (HALF) {                                              // :2561-2601
        const int32_t a = c[0] * q[0];
        const int32_t b = c[2] * q[2];
        const int32_t m = jda_mulc<FAST>(b, 106) >> 8;
        t0 = a + b; t3 = a - b; t1 = a + m; t2 = a - m;
        t4 = c[1] * q[1];
        if (c[3] != 0) {
            const int32_t d = c[3] * q[3];
            t7 = t4 + d;
            const int32_t t11 = jda_mulc<FAST>(t4 - d, 362) >> 8;
            const int32_t z5 = jda_mulc<FAST>(t4 - d, 473) >> 8;
            const int32_t t12 = (jda_mulc<FAST>(d, 669) >> 8) + z5;               // (-tmp5 * -669) >> 8
            t6 = t12 - t7;
            t5 = t11 - t6;
            const int32_t t10 = (jda_mulc<FAST>(t4, 277) >> 8) - z5;
            t4 = t10 + t5;
        } else {
            t7 = t4;
            t5 = jda_mulc<FAST>(t4, 145) >> 8;
            t6 = jda_mulc<FAST>(t4, 217) >> 8;
            t4 = jda_mulc<FAST>(t4, -51) >> 8;
        }
    } else {                                                         // :2602-2676
        // the reference's zero tests on rows 4..7 only skip work; the arithmetic is identical
        const int32_t e0 = c[0] * q[0], e4 = c[4] * q[4];
        const int32_t t10 = e0 + e4, t11 = e0 - e4;
        const int32_t e2 = c[2] * q[2], e6 = c[6] * q[6];
        const int32_t t13 = e2 + e6;
        const int32_t t12 = (jda_mulc<FAST>(e2 - e6, 362) >> 8) - t13;
        t0 = t10 + t13; t3 = t10 - t13; t1 = t11 + t12; t2 = t11 - t12;
        const int32_t o3 = c[3] * q[3], o5 = c[5] * q[5];
        const int32_t z13 = o5 + o3, z10 = o5 - o3;
        const int32_t o1 = c[1] * q[1], o7 = c[7] * q[7];
        const int32_t z11 = o1 + o7, z12 = o1 - o7;
        t7 = z11 + z13;
        const int32_t u11 = jda_mulc<FAST>(z11 - z13, 362) >> 8;
        const int32_t z5 = jda_mulc<FAST>(z10 + z12, 473) >> 8;
        const int32_t u12 = (jda_mulc<FAST>(z10, -669) >> 8) + z5;
        t6 = u12 - t7;
        t5 = u11 - t6;
        const int32_t u10 = (jda_mulc<FAST>(z12, 277) >> 8) - z5;
        t4 = u10 + t5;
    }
    out[0] = (int16_t)(t0 + t7); out[1] = (int16_t)(t1 + t6);
    out[2] = (int16_t)(t2 + t5); out[3] = (int16_t)(t3 - t4);
    out[4] = (int16_t)(t3 + t4); out[5] = (int16_t)(t2 - t5);
    out[6] = (int16_t)(t1 - t6); out[7] = (int16_t)(t0 - t7);
}

// 1/4 scale: 2x2 block from coefficients 0,1,8,9 (jpeg.inl:2305-2326) -> 4 bytes
JDA_HD uint32_t jda_idct_2x2(const int16_t *coef, const int16_t *quant)
{
    const int32_t a = coef[0] * quant[0], b = coef[8] * quant[8];
    const int32_t c = coef[1] * quant[1], d = coef[9] * quant[9];
    const int32_t t0 = a + b, t2 = a - b, t1 = c + d, t3 = c - d;
    return jda_range_limit5(t0 + t1) | (jda_range_limit5(t0 - t1) << 8) |
           (jda_range_limit5(t2 + t3) << 16) | (jda_range_limit5(t2 - t3) << 24);
}

// ---- colour conversion (jpeg.inl:3101-3278) -------------------------------------------------
struct jda_ycc { int32_t y; int32_t cb; int32_t cr; };   // y pre-scaled by 2^12 (or sum<<10)

JDA_HD uint32_t jda_pixel_rgba(jda_ycc p)
{
    const int32_t cb = p.cb - 128, cr = p.cr - 128;
    const int32_t r = jda_clamp255((5742 * cr + p.y) >> 12);
    int32_t g = jda_clamp255((-1409 * cb - 2925 * cr + p.y) >> 12);
    const int32_t b = jda_clamp255((7258 * cb + p.y) >> 12);
    JDA_OPAQUE(g);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | 0xff000000u;
}

JDA_HD uint32_t jda_pixel_565(jda_ycc p, bool big_endian)
{
    const int32_t cb = p.cb - 128, cr = p.cr - 128;
    // usRangeTableR/G/B[(x >> 12) & 0x3ff]: 10-bit wrap, then clamp
    const int32_t r = jda_clamp255(jda_sext10_at(5742 * cr + p.y, 12));
    const int32_t g = jda_clamp255(jda_sext10_at(-1409 * cb - 2925 * cr + p.y, 12));
    const int32_t b = jda_clamp255(jda_sext10_at(7258 * cb + p.y, 12));
    uint32_t v = (uint32_t)((r >> 3) << 11) | (uint32_t)((g >> 2) << 5) | (uint32_t)(b >> 3);
    if (big_endian) v = ((v & 0xffu) << 8) | (v >> 8);
    return v;
}

JDA_HD uint32_t jda_gray_565(uint32_t y, bool big_endian)
{
    uint32_t v = ((y >> 3) << 11) | ((y >> 2) << 5) | (y >> 3);     // usGrayTo565
    if (big_endian) v = ((v & 0xffu) << 8) | (v >> 8);
    return v;
}

// Sample fetch for output pixel (px,py) of one MCU's output tile, per subsampling mode and scale
// shift.  planes: the MCU's blocks, 64 bytes each, block order Y.. Cb Cr.  `luma` = only the
// luma value is wanted (GRAY8 output / gray JPEG): returned in .y UNscaled (0..255).
template <int MODE>
JDA_HD jda_ycc jda_fetch(const uint8_t *planes, uint32_t px, uint32_t py, int shift, bool luma)
{
    typedef jda_mode_traits<MODE> T;
    jda_ycc o;
    o.cb = 128; o.cr = 128;
    const uint8_t *Y = planes;
    uint32_t cidx = 0;                                  // index into the 8x8 chroma blocks
    if (MODE == JDA_MODE_420) {
        // which luma block, and the position inside it
        const uint32_t bsz = 8u >> shift;               // block edge in output pixels: 8,4,2,1
        const uint32_t q = (py / bsz) * 2 + (px / bsz);
        Y = planes + JDA_COEF_STRIDE * q;
        const uint32_t bx = px & (bsz - 1), by = py & (bsz - 1);
        if (shift == 0) { o.y = Y[by * 8 + bx]; cidx = (py >> 1) * 8 + (px >> 1); }         // :4333-4543
        else if (shift == 1) {                                                              // :3577-3626
            const uint8_t *s = Y + by * 16 + bx * 2;
            o.y = s[0] + s[1] + s[8] + s[9];
            cidx = py * 8 + px;
        } else if (shift == 2) { o.y = Y[by * 2 + bx]; cidx = q; }                          // :3664-3748
        else { o.y = Y[0]; cidx = 0; }                                                      // :3627-3663
        if (!luma) {
            o.cb = planes[JDA_COEF_STRIDE * 4 + cidx];
            o.cr = planes[JDA_COEF_STRIDE * 5 + cidx];
            o.y = (shift == 1) ? (o.y << 10) : (o.y << 12);
        } else if (shift == 1) o.y = (o.y + 2) >> 2;                                        // :2979-2999
    } else if (MODE == JDA_MODE_422 || MODE == JDA_MODE_440) {
        // two luma blocks side by side (4:2:2, JPEGPutMCU21 jpeg.inl:4721-4868) or one above the other (4:4:0,
        // JPEGPutMCU12 :4546-4719); chroma blocks in slots 2, 3.  a = coordinate along which the blocks are stacked
        // and the chroma is subsampled, c = the other one.
        const bool horiz = MODE == JDA_MODE_422;
        const uint32_t bsz = 8u >> shift;
        const uint32_t a = horiz ? px : py, c = horiz ? py : px;
        const uint32_t q = a / bsz, ba = a & (bsz - 1);
        Y = planes + JDA_COEF_STRIDE * q;
        const uint32_t bx = horiz ? ba : c, by = horiz ? c : ba;          // position inside the luma block
        const uint8_t *Cb = planes + 2 * JDA_COEF_STRIDE, *Cr = planes + 3 * JDA_COEF_STRIDE;
        uint32_t cb = 128, cr = 128;
        if (shift == 0) {
            o.y = Y[by * 8 + bx];
            cidx = horiz ? (py * 8 + q * 4 + (bx >> 1)) : ((py >> 1) * 8 + px);
            cb = Cb[cidx]; cr = Cr[cidx];
        } else if (shift == 1) {
            const uint8_t *s = Y + by * 16 + bx * 2;
            o.y = s[0] + s[1] + s[8] + s[9];
            // the chroma of the two source pixels across the non-subsampled direction is averaged, + 1 (:4743-4744, :4567-4568)
            cidx = horiz ? (py * 16 + q * 4 + bx) : (py * 8 + px * 2);
            const uint32_t step = horiz ? 8u : 1u;
            if (!luma) { cb = (Cb[cidx] + Cb[cidx + step] + 1u) >> 1; cr = (Cr[cidx] + Cr[cidx + step] + 1u) >> 1; }
        } else if (shift == 2) {
            o.y = Y[by * 2 + bx];
            cidx = horiz ? (py * 2 + q) : (q * 2 + px);                   // :4789-4838, :4610-4682
            cb = Cb[cidx]; cr = Cr[cidx];
        } else { o.y = Y[0]; cb = Cb[0]; cr = Cr[0]; }
        if (!luma) { o.cb = (int32_t)cb; o.cr = (int32_t)cr; o.y = (shift == 1) ? (o.y << 10) : (o.y << 12); }
        else if (shift == 1) o.y = (o.y + 2) >> 2;                         // JPEGPutMCU8BitGray :2857-2873, :2907-2923
    } else {
        if (shift == 0) { cidx = py * 8 + px; o.y = Y[cidx]; }
        else if (shift == 1) {
            cidx = py * 16 + px * 2;
            o.y = Y[cidx] + Y[cidx + 1] + Y[cidx + 8] + Y[cidx + 9];
        } else if (shift == 2) { cidx = py * 2 + px; o.y = Y[cidx]; }
        else { cidx = 0; o.y = Y[0]; }
        if (MODE == JDA_MODE_444 && !luma) {
            const uint8_t *Cb = planes + JDA_COEF_STRIDE, *Cr = planes + 2 * JDA_COEF_STRIDE;
            if (shift == 1) {                                                               // :3297-3322
                o.cb = (Cb[cidx] + Cb[cidx + 1] + Cb[cidx + 8] + Cb[cidx + 9] + 2) >> 2;
                o.cr = (Cr[cidx] + Cr[cidx + 1] + Cr[cidx + 8] + Cr[cidx + 9] + 2) >> 2;
                o.y <<= 10;
            } else { o.cb = Cb[cidx]; o.cr = Cr[cidx]; o.y <<= 12; }
        } else if (shift == 1) o.y = (o.y + 2) >> 2;                                        // :2812-2827, 3043-3069
        (void)T::NBLK;
    }
    return o;
}

// value of one output pixel in its final format
template <int MODE>
JDA_HD uint32_t jda_output_pixel(const uint8_t *planes, uint32_t px, uint32_t py, int shift, int pixel_type)
{
    if (pixel_type == JDA_EIGHT_BIT_GRAYSCALE) return (uint32_t)jda_fetch<MODE>(planes, px, py, shift, true).y;
    if (MODE == JDA_MODE_GRAY)                     // gray JPEG -> RGB565 (JPEGPutMCUGray, :3037-3099)
        return jda_gray_565((uint32_t)jda_fetch<MODE>(planes, px, py, shift, true).y, pixel_type != JDA_RGB565_LITTLE_ENDIAN);
    const jda_ycc p = jda_fetch<MODE>(planes, px, py, shift, false);
    if (pixel_type == JDA_RGB8888) return jda_pixel_rgba(p);
    return jda_pixel_565(p, pixel_type == JDA_RGB565_BIG_ENDIAN);
}


// ---- device pre-scan ----------------------------------------------------------------
// The filtered scan is cut into segments of JDA_SEG_BYTES; one lane walks one segment's Huffman symbols in skip mode.
// A lane does not know the decoder state at its segment's first bit -- (bit offset of the next symbol, block within the
// MCU, zigzag position) -- so it guesses "a block starts here" and walks: Huffman streams re-synchronise by themselves
// after a few symbols, and an EOB re-synchronises the zigzag position.  The passes (jda_kernels.hip):
//   round 0   every lane walks its segment from the guess and hands the state at the segment's end to the next segment
//   round 1.. walk again from the entry state the segment before handed over, now counting (block starts, per-component DC sums, how
//             the reference's window phase propagates: six byte lags in flight); a walk whose exit differs from what the next segment
//             was entered with puts that segment on the next round's list.  Segment 0's entry state is known, so a round that
//             leaves its list empty is the fixed point E[i+1] = walk(i, E[i]) with E[0] true: the serial decoder's states
//   sums      exclusive scan over the segments: first block ordinal, DC predictors, window phase at every entry
//   WRITE     the walk once more, now writing the per-block index and DC predictors exactly as the serial host pre-scan does.
// State at a symbol boundary (after the reference's bottom-of-loop refill, before its next top-of-loop refill):
//   bits 5:0 bit offset from the segment's first bit (entry: how far the previous segment's last symbol reached in),
//   bits 8:6 block within the MCU, bits 14:9 zigzag position k (0 = the next symbol is a DC code).
#define JDA_SEG_BITS  (JDA_SEG_BYTES * 8u)
#define JDA_SEG_SLOT  (JDA_SEG_BYTES + 12u)           // bytes a lane reads: its segment + 12 bytes of the next; 67 dwords per lane in LDS (odd: no bank conflicts)
#define JDA_SEG_DEAD  0x7fffffffu    // state of a walk that met an invalid code (bit 31 is the rounds' "changed" mark)
#define JDA_SEG_CHANGED 0x80000000u // entry-state word: "differs from the previous round's" (the walker's own bits are 14:0)
enum { JDA_SEG_SPEC = 0 /* round 0: the exit state only */, JDA_SEG_RECORD = 4 /* + the segment's sums, one record per block start, truncation candidates (jda_segscan_finalize) */ };
#define JDA_SEG_SUM_WORDS 8u         // per segment: block starts, DC sums [3], phase map, bad | has-restart | max AC category << 4, lag word at the last block start, round
#define JDA_SEG_START_WORDS 5u       // per segment: first block ordinal, DC predictors [3], byte lag j of the reference window at its entry
// the result words (jda_segscan_params.stats), zeroed by the caller: who writes them is said at jda_segscan_params; what they add up to, in jda_prescan_plan.h
#define JDA_ST_BAD 0u                // a predictor out of range, a stream read on into its padding, more records or candidates than their arrays hold
#define JDA_ST_TERMINAL 1u           // closing index entries written: 1 for a good stream
#define JDA_ST_MAX_AC 2u             // largest AC category
#define JDA_ST_MAX_DC 3u             // largest |DC|
#define JDA_ST_TRUNC 4u              // truncated reads (the serial pre-scan's count)
#define JDA_ST_RST_MISMATCH 5u       // a restart marker is not where the MCU count puts it
#define JDA_ST_INDEX_OK 6u           // the sums: enough blocks, no bad code before the end
#define JDA_ST_SETTLED 7u            // the last round left nothing to walk (0: JDA_PRESCAN_MAX_ROUND reached)
#define JDA_ST_ROUND0 8u             // + r: length of round r's work list (r >= 2; round r - 1 appends to it)
#define JDA_ST_NCAND 66u             // truncation candidates appended (RECORD)
#define JDA_ST_WORDS 68u
#define JDA_PRESCAN_LIST_ROUNDS 4u   // rounds launched one by one (a round with an empty work list returns at once); the rest in one launch (jda_segscan_tail)
#define JDA_PRESCAN_MAX_ROUND 56u    // no list round has this number or a higher one: the states-first order's recording round takes it
static_assert(JDA_ST_ROUND0 + JDA_PRESCAN_MAX_ROUND + 1u < JDA_ST_NCAND, "every round's list length has a result word of its own");
#define JDA_REC_POS_BITS 12u         // a record: bit position of the block's first AC symbol, counted from its segment's first bit (the block's DC symbol starts in the
                                     // segment: <= 2047 + 27) | running DC sum of its component, the block's own difference included, << 12
#define JDA_SEG_FIRST_RST_SHIFT 8u   // seg_sum word 5, bits 31:8: the ordinal of the segment's first block behind an interval end (its sums count from a restart)

struct jda_segscan_params {          // one per image
    const uint8_t *scan;             // filtered scan (global), zero padded to n_segs * JDA_SEG_BYTES + 16
    const uint8_t *tables;           // table blob (global)
    uint32_t *entry_cur, *entry_nxt; // n_segs + 1 entry states, zeroed: the rounds read and replace them in place (entry_cur; entry_nxt is not read)
    uint32_t *seg_sum;               // every RECORD walk out, JDA_SEG_SUM_WORDS words per segment; the sums, finalize and the candidates in
    const uint32_t *seg_start;       // the sums out, JDA_SEG_START_WORDS words per segment; finalize and the candidates in
    uint32_t *blk_index;             // finalize out, flagged entries by the candidates: n_blocks_total + 1
    int16_t *blk_dc;                 // finalize out: n_blocks_total
    // JDA_ST_WORDS result words (JDA_ST_*), zeroed: list lengths by the rounds, SETTLED by jda_segscan_tail, NCAND by the RECORD walks, INDEX_OK and
    // MAX_AC by the sums, BAD / TERMINAL / MAX_DC by finalize, RST_MISMATCH / TRUNC (and BAD: more candidates than cand_cap) by the candidates' pass
    uint32_t *stats;
    uint32_t scan_len, n_segs, n_blocks_total, first_round;      // (first_round is not read)
    uint8_t nluma, nblocks, dc_id[3], ac_id[3];
    const uint32_t *filter_result;   // device filter ran (jda_pipeline): [0] = the filtered length; scan_len / n_segs above are upper bounds then
    uint32_t *worklist;              // jda_segscan_fused: two lists of n_segs (upper bound) segment numbers -- who walks in the next round
    uint32_t worklist_cap;
    // streams with restart intervals (0 / NULL otherwise): where in the FILTERED scan every interval starts -- restart_pos[0] = 0,
    // restart_pos[1 .. n_intervals - 1] = the positions the RSTn markers stood at, restart_pos[n_intervals] = JDA_RST_SENTINEL --,
    // blocks per interval (DRI x blocks per MCU), and whether the last interval is a whole one (the closing index entry is then
    // rounded up to a byte like every interval end, jpeg.inl:5339-5346)
    const uint32_t *restart_pos;
    uint32_t n_intervals, interval_blocks, round_last;
    // the walk's four tables (JDA_WT_BYTES) as jda_walk_tables_build makes them from the blob, once per image: a walker's workgroup
    // copies them (one wait) instead of converting the blob itself
    uint8_t *walk_tables;
    uint32_t walk_tables_shared;      // 1: another image of the batch (same tables, same table ids) builds them
    // RECORD mode (every caller's: finalize and the candidates' pass return at once without records): the walk leaves one record per
    // block start -- rec_cap slots per segment (more than its 2,048 bits can start blocks: jda_record_cap), 16-byte groups -- and the
    // rare magnitude read that SOME entry lag would truncate as a candidate (16 bytes: segment, ordinal + 1 | round << 16, lag word at
    // the block's start, the lags that truncate); jda_segscan_finalize turns records into index entries and predictors,
    // jda_segscan_resolve_cands the candidates of the true lag into flagged entries.  Neither array needs clearing.
    uint32_t *records;
    uint32_t rec_cap;
    uint32_t *cands;
    uint32_t cand_cap;
    // RECORD mode with restart intervals: two words per interval start nr = 1 .. n_intervals - 1, zeroed -- the walk that ends the
    // interval in front of it leaves (its segment << 11 | blocks it had started by then + 1, its round): jda_segscan_resolve_cands
    // checks that every marker ended an interval of a settled walk exactly where the MCU count puts it (JDA_ST_RST_MISMATCH)
    uint32_t *rst_events;
};
#define JDA_RST_SENTINEL 0x1fffffffu      // (a byte position no scan reaches: the index packs positions in 25 bits)
#define JDA_SEG_HAS_RESTART 2u           // seg_sum word 5, bit 1: an interval ends inside the segment (its DC sums count from there)
// the parameters with what only the device knows filled in
JDA_HD jda_segscan_params jda_segscan_resolve(const jda_segscan_params &in)
{
    jda_segscan_params P = in;
    if (P.filter_result) {
        P.scan_len = JDA_G(const uint32_t, P.filter_result)[0]; P.n_segs = P.scan_len / JDA_SEG_BYTES + 1u;
        // as many RSTn markers as the MCU count asks for?  If not, nothing walks (restart_pos is not what the walk takes it for) and
        // the result words stay "no index": the serial pre-scan does what the reference does with such a file
        if (P.restart_pos && JDA_G(const uint32_t, P.filter_result)[1] + 1u != P.n_intervals) P.n_segs = 0;
    }
    return P;
}
struct jda_seg_sum { uint32_t nblk; int32_t dcsum[3]; uint32_t phase_map, bad, lag_last, max_ac; };
struct jda_seg_stats { uint32_t bad, terminal, max_ac_bits, max_abs_dc, trunc_events, mismatch; };

JDA_HD uint32_t jda_atomic_inc_u32(uint32_t *p)                   // the value before
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return (*p)++;                                   // (the emulator steps the lanes one after another)
#endif
}
JDA_HD void jda_atomic_or_u32(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p |= v;                                         // (the emulator steps the lanes one after another)
#endif
}
// The walk's view of its segment: 64 stream bits in two registers and the three dwords after them (the segment is read where it
// lies -- global memory, L2 -- and nothing of the scan is staged in LDS: the tables are all a workgroup keeps there, and the
// wavefronts a CU holds are bounded by registers, not by 17 KB of slots each).  A symbol is at most 31 bits (code <= 16, magnitude
// <= 15), so a step advances the window by at most one dword -- a register shuffle, no load: the five dwords are (re)loaded for
// ALL lanes of the wavefront at once, from wherever each lane stands, every JDA_SEG_REFILL_STEPS steps (jda_seg_walk).  A load
// inside the step ("the lane that crosses a dword boundary fetches the next one") was a load + its wait in EVERY step of the
// wavefront: one of 64 unsynchronised lanes crosses every time.  Five dwords are at least 97 bits ahead of the lane: 12 bits per
// symbol over eight steps; the lane that runs out anyway (or, at an interval end, steps over a dword) reloads on its own (rare).
struct jda_seg_reader {
    const uint32_t JDA_GLOBAL *d;   // the segment's first dword (readable: JDA_SEG_SLOT bytes)
    uint32_t idx, base;             // dword index of hi now / when the registers were loaded
    uint32_t hi, lo;                // stream bits, first byte on top
    uint32_t n1, n2, n3;            // the dwords behind lo (first byte on top, like hi and lo); valid while idx - base <= 3
};
#ifndef JDA_SEG_REFILL_STEPS
#define JDA_SEG_REFILL_STEPS 8u
#endif
JDA_HD void jda_seg_reader_init(jda_seg_reader &R, const uint32_t JDA_GLOBAL *d, uint32_t p)
{
    R.d = d; R.idx = R.base = p >> 5;
    R.hi = __builtin_bswap32(d[R.idx]); R.lo = __builtin_bswap32(d[R.idx + 1u]);
    R.n1 = __builtin_bswap32(d[R.idx + 2u]); R.n2 = __builtin_bswap32(d[R.idx + 3u]); R.n3 = __builtin_bswap32(d[R.idx + 4u]);      // (swapped here, once a reload: the slide is in every step)
}
// the next 32 bits of the stream at bit p of the segment
// (the window slides by selects, no branch: the walk's loop sees to it that p stays within the loaded dwords -- jda_seg_reader_holds --
// and reloads for the whole wavefront otherwise; a peek is at most one dword ahead of the last one)
JDA_HD uint32_t jda_seg_reader_peek(jda_seg_reader &R, uint32_t p)
{
    const uint32_t wi = p >> 5;
    const bool adv = wi != R.idx;
    R.hi = adv ? R.lo : R.hi;
    R.lo = adv ? R.n1 : R.lo;
    R.n1 = adv ? R.n2 : R.n1;
    R.n2 = adv ? R.n3 : R.n2;
    R.idx = wi;
    const uint64_t v = ((uint64_t)R.hi << 32) | R.lo;
    return (uint32_t)((v << (p & 31u)) >> 32);
}
JDA_HD bool jda_seg_reader_holds(const jda_seg_reader &R, uint32_t p) { return (p >> 5) - R.base <= 3u; }
#define JDA_SEG_READ_DWORDS (JDA_SEG_BYTES / 4u + 4u)     // dwords of the scan a walk may touch from its segment's start (64 + the window's reach)

// The walks' DC entries: the reference's DC LUT (jpeg.inl:1098-1152) re-laid out like the AC entries -- (code length - 1) << 12 |
// SSSS << 8 | folded -- so that one lookup serves a DC and an AC symbol alike.  "folded" (bit 0): the reference takes code
// and magnitude from the LUT in one step (:1132-1152) and does not refill between them.
//   JDA_WT_* (the segment walk's own LDS layout): FOUR tables of 2048 entries -- AC 0, AC 1, DC 0, DC 1 -- under the AC tables'
//   11-bit key (the stream's top 10 bits, or 1024 + the 10 bits behind six leading ones), so that a step computes ONE address:
//   table number from the block's place in the MCU, key from the stream.  A DC entry under that key is the reference's for every
//   stream that has those bits, provided no DC code 111110.. is longer than 10 bits (jda_dc_lut_walkable: the front end keeps
//   such a file -- none seen -- on the serial pre-scan).
//   An entry is 32 bits: the low half the symbol (the decode kernel's jda_ac_entry layout / jda_dc16_entry), the high half -- AC
//   tables, short keys -- the symbol BEHIND it where the key's ten bits hold that one's code too: two symbols a step (JDA_WT_PAIR_*;
//   the second is described by what a walk needs of it: bits it takes, coefficients it moves on by, its magnitude's size).
#define JDA_WT_TABLE_BYTES 8192u
#define JDA_WT_BYTES (4u * JDA_WT_TABLE_BYTES)
#define JDA_WT_PAIR_VALID 0x8000u                     // | size << 10 | (run + 1, 0 = EOB) << 5 | code + magnitude bits (<= 16)
// the pair half of the entry ea under `key` (< 1024): ac = the 2048 raw entries (length << 8 | RS, 0 = no code) of the AC table that
// decodes the symbol behind it -- the table itself for an AC entry, the table of the component for a DC entry (jda_wt_dc_follow)
JDA_HD uint32_t jda_wt_pair(uint32_t ea, const uint16_t JDA_GLOBAL *ac, uint32_t key)
{
    if (JDA_AC_STOPS(ea)) return 0u;                                // EOB ends the block, no code ends the walk's luck: no second symbol
    const uint32_t bits_a = (ea >> 12) + 1u + ((ea >> 8) & 15u);
    if (bits_a > 9u) return 0u;
    const uint32_t left = 10u - bits_a, key_b = (key << bits_a) & 1023u;      // the key's bits behind A, zeros behind them
    if ((key_b >> 4) == 63u) return 0u;                             // six ones: a code of the table's long half
    const uint32_t eb = jda_ac_entry(ac[key_b]);
    if ((eb & 0xffu) == JDA_AC_NONE) return 0u;
    const uint32_t len_b = (eb >> 12) + 1u;
    if (len_b > left) return 0u;                                    // B's code is not all there (a longer code matched the zeros)
    const bool eob = (eb & 0xffu) == JDA_AC_EOB;
    const uint32_t sz_b = eob ? 0u : (eb >> 8) & 15u, run_b = (eb >> 1) & 15u;
    if (len_b + sz_b > 16u) return 0u;                              // (a magnitude read the reference may truncate is a step of its own)
    return JDA_WT_PAIR_VALID | (sz_b << 10) | ((eob ? 0u : run_b + 1u) << 5) | (len_b + sz_b);
}
JDA_HD uint32_t jda_dc16_entry(uint32_t e8, int32_t folded)
{
    if (e8 == 0u) return JDA_AC_NONE;
    const uint32_t s = e8 & 15u, tot = e8 >> 4;
    const bool fold = s != 0u && folded != 0;
    const uint32_t len = fold ? tot - s : tot;                   // a folded entry holds code + magnitude length
    return ((len - 1u) << 12) | (s << 8) | (fold ? 1u : 0u);
}

// which AC table decodes the symbol behind a DC symbol of DC table t (2 bits per t; 2: none -- the components that share the DC
// table do not share an AC table): the DC entries take their pair halves from it
JDA_HD uint32_t jda_wt_dc_follow(const jda_segscan_params &P)
{
    const uint32_t ncomp = P.nblocks > P.nluma ? 3u : 1u;
    uint32_t f = 0;
    for (uint32_t t = 0; t < 2u; t++) {
        uint32_t seen = 3u;                                         // 3: no component uses DC table t
        for (uint32_t c = 0; c < ncomp; c++) {
            if ((P.dc_id[c] & 1u) != t) continue;
            const uint32_t a = P.ac_id[c] & 1u;
            seen = seen == 3u ? a : (seen == a ? a : 2u);
        }
        f |= (seen == 3u ? 2u : seen) << (2u * t);
    }
    return f;
}
// the segment walk's tables, staged by its workgroup (tid = thread in workgroup): wt holds JDA_WT_BYTES
JDA_HD void jda_walk_tables_from(const uint8_t *tables, uint32_t follow, uint32_t tid, uint32_t nthreads, uint8_t *wt)
{
    const uint16_t JDA_GLOBAL *ac = JDA_G(const uint16_t, tables + JDA_TB_AC);
    uint32_t *out = (uint32_t *)wt;
    for (uint32_t j = tid; j < 4096u; j += nthreads) {                              // both halves of both AC tables -> the kernels' entries
        const uint32_t t = j >> 11, key = j & 2047u;
        const uint32_t ea = jda_ac_entry(ac[j]);
        out[j] = ea | (key < 1024u ? jda_wt_pair(ea, ac + t * 2048u, key) << 16 : 0u);
    }
    for (uint32_t j = tid; j < 4096u; j += nthreads) {                              // the DC tables under the same key
        const uint32_t t = j >> 11, idx = jda_dc_lut_index(jda_walk_key_code12(j & 2047u, 0u));
        const uint8_t JDA_GLOBAL *dc = JDA_G(const uint8_t, tables) + JDA_TB_DC + t * 1024u;
        const uint32_t ea = jda_dc16_entry(dc[idx], (int8_t)dc[idx + 512u]), key = j & 2047u, fa = (follow >> (2u * t)) & 3u;
        out[4096u + j] = ea | (key < 1024u && fa < 2u ? jda_wt_pair(ea, ac + fa * 2048u, key) << 16 : 0u);
    }
}
// what a walker's workgroup does: a copy of the image's prepared tables (jda_walk_tables_build; 32 KB, one wait)
JDA_HD void jda_walk_tables_stage(const uint8_t *prepared, uint32_t tid, uint32_t nthreads, uint8_t *wt)
{
    const jda_chunk16_alias JDA_GLOBAL *src = JDA_G(const jda_chunk16_alias, prepared);
    jda_chunk16_alias *out = (jda_chunk16_alias *)wt;
    for (uint32_t i = tid; i < JDA_WT_BYTES / 16u; i += nthreads) out[i] = src[i];
}
// One walk of a segment.  wt: the walk's tables (jda_walk_tables_from); segw: the segment's first dword in the (zero-padded)
// filtered scan.
//
// A step decodes a symbol (and the one behind it where the table entry describes it: JDA_WT_PAIR_*), DC or AC alike, without a branch on which it is: the lanes of a wavefront sit at unrelated places
// of their blocks, so "if DC .. else AC .." ran both sides every step -- and every small `if` in the body costs an exec-mask
// region (s_and_saveexec / s_cbranch / s_or), so the body is written with selects; what stays a branch is what is rare (a
// truncated magnitude, an invalid code) or has to store (a block's start and end in the WRITE pass).  The reference's refills
// (jpeg.inl:2110-2114) happen at fixed places -- before a block's first symbol, before a DC magnitude that is not folded into
// its LUT entry, at the top and the bottom of the AC loop -- and two of them in a row at the same bit are one; so a step is:
// [refill before an unfolded DC magnitude] .. refill at its end (bottom of the AC loop / top of it after the DC symbol / opening
// refill of the next block after EOB: same position, same result).  State at a step boundary, hence at a segment boundary:
// after that refill.
//   SPEC   exit state only.
//   COUNT  + block starts, DC sums per component, and how the reference window's BYTE LAG u = (p >> 3) - pBuf propagates: the
//          six lags a boundary state can have (a refill leaves off <= 47) ride in 5-bit fields of one word (4 value bits + a
//          guard bit for the compare); bits consumed advance all of them by the same number of bytes, a refill resets those
//          that reached 6 bytes.  phase_map: field j (3 bits) = exit lag for entry lag j.
//   WRITE  the reader itself (pBuf, ulBitOff), block ordinals and DC predictors from seg_start: index entries (held back to the
//          block's end so that a truncation flag joins its entry in the register; only a block that crosses into the next segment
//          is ORed in atomically), blk_dc -- both collected in registers and stored as aligned 16-byte groups (below) --,
//          maxima, truncation count.
// RST: the stream has restart intervals.  The filter recorded where every interval starts (byte aligned: the rest of the byte in
// front is padding); a walk that finishes an MCU within 7 bits of the next start has finished the interval: it steps over the
// padding, the reference rounds ulBitOff up WITHOUT a refill (jpeg.inl:5339-5346; so the refill after an interval's closing EOB
// waits for the next block's opening one), the DC predictors restart at zero.  The reference itself counts MCUs and never
// looks at marker positions: the WRITE pass checks that the two agree (every interval end at a multiple of interval_blocks,
// every such multiple an interval end) and sends the image to the serial pre-scan when they do not.
JDA_HD void jda_store_u32x4(void *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)      // one 16-byte store (p: global memory, 16-byte aligned)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *JDA_G(uint4, p) = make_uint4(a, b, c, d);
#else
    uint32_t *o = (uint32_t *)p; o[0] = a; o[1] = b; o[2] = c; o[3] = d;
#endif
}
// the six 5-bit byte lags of a counting walk + n each (n <= 3): U + n * 0x02108421 on the 24-bit multiplier and a shift-add
// (the 26-bit constant makes the product a quarter-rate v_mad_u64_u32, twice per symbol)
JDA_HD uint32_t jda_lag_add(uint32_t U, uint32_t n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;                                                     // (written out: the compiler puts any product + sum it recognises back on v_mad_u64_u32)
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(n), "s"(0x00108421u), "v"(U));
    return r + (n << 25);
#else
    return U + n * 0x02108421u;
#endif
}
template <int OP, bool RST = false>
JDA_HD uint32_t jda_seg_walk(const jda_segscan_params &P, uint32_t seg, uint32_t entry, const uint32_t JDA_GLOBAL *segw, const uint8_t *wt,
                             jda_seg_sum &S, jda_seg_stats &ST, uint32_t round = 0)
{
    const bool REC = OP == JDA_SEG_RECORD;                            // sums + one record per block start + truncation candidates (else: the exit state only)
#ifndef JDA_SEG_PAIR_OFF
#define JDA_SEG_PAIR_OFF() false                                             // (host simulator: a switch, to count what the pairs save)
#endif
    const bool PAIR = !JDA_SEG_PAIR_OFF();                           // two AC symbols a step where the table holds the second (JDA_WT_PAIR_*)
    (void)ST;
    S.nblk = 0; S.dcsum[0] = S.dcsum[1] = S.dcsum[2] = 0; S.phase_map = 0; S.bad = 0; S.lag_last = 0; S.max_ac = 0;
    if (entry == JDA_SEG_DEAD) { S.bad = 1; return JDA_SEG_DEAD; }
    uint32_t p = entry & 63u, b2 = ((entry >> 6) & 7u) * 2u, k = (entry >> 9) & 63u;      // b2: twice the block's place in the MCU
    // per place in the MCU, in 2-bit fields (uniform): the block's component, and which of the walk's four tables decodes its
    // AC symbols (0 / 1) and its DC symbol (2 / 3)
    uint32_t csel = 0, acsel = 0, dcsel = 0;
    const uint32_t nluma = P.nluma, nblocks2 = 2u * P.nblocks;
    const uint32_t aid0 = P.ac_id[0] & 1u, aid1 = P.ac_id[1] & 1u, aid2 = P.ac_id[2] & 1u, did0 = P.dc_id[0] & 1u, did1 = P.dc_id[1] & 1u, did2 = P.dc_id[2] & 1u;
#pragma unroll
    for (uint32_t i = 0; i < 6u; i++) {                             // (constant indices only: a dynamic one would move P to scratch memory)
        const uint32_t ci = i < nluma ? 0u : i - nluma + 1u;
        const uint32_t a = ci == 0u ? aid0 : (ci == 1u ? aid1 : aid2), d = ci == 0u ? did0 : (ci == 1u ? did1 : did2);
        if (i < P.nblocks && ci < 3u) { csel |= ci << (2u * i); acsel |= a << (2u * i); dcsel |= (2u + d) << (2u * i); }
    }
    uint32_t U = 0;                                                 // the six byte lags
    const uint32_t kOnes = 0x02108421u, kGuard = 0x21084210u;       // 1 / 16 in each 5-bit field
    uint32_t nblk = 0;
    bool sbad = false;                                              // (a flag per lane: the compiler keeps it as a lane mask on the scalar unit)
    int32_t ds0 = 0, ds1 = 0, ds2 = 0;
    uint32_t max_ac = 0;
    if (REC) U = 0u | (1u << 5) | (2u << 10) | (3u << 15) | (4u << 20) | (5u << 25);
    // RECORD: the last four records (newest last; a group of four is stored when it is complete: the segment's slots are its own),
    // the lag word at the first AC symbol of the block in progress
    uint32_t rb0 = 0, rb1 = 0, rb2 = 0, rb3 = 0, Ublk = 0;
    uint32_t JDA_GLOBAL *recs = REC ? JDA_G(uint32_t, P.records) + (size_t)seg * P.rec_cap : (uint32_t JDA_GLOBAL *)0;
    // RST: the next interval start ahead of the walk (as a bit position relative to the segment); the ordinal of the segment's first
    // block behind an interval end (its DC sums count from there)
    const uint32_t JDA_GLOBAL *rpos = JDA_G(const uint32_t, P.restart_pos);
    const uint32_t seg_bit0 = seg * JDA_SEG_BITS;
    uint32_t nr = 0, next_bit = 0xffffffffu, has_rst = 0, first_rst = 0;
    if (RST) {
        const uint32_t byte0 = (seg_bit0 + p) >> 3;                 // smallest nr >= 1 with restart_pos[nr] * 8 > the entry position
        uint32_t lo = 1, hi = P.n_intervals;                        // (restart_pos[n_intervals] is the sentinel)
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (rpos[mid] > byte0) hi = mid; else lo = mid + 1; }
        nr = lo;
        next_bit = (rpos[nr] << 3) - seg_bit0;
    }
    jda_seg_reader R;
    bool go = p < JDA_SEG_BITS;
    while (go) {
    jda_seg_reader_init(R, segw, p);                                // every lane of the wavefront from where it stands: one wait for all of them
    uint32_t since = 0;
    bool jumped = false;                                            // RST: this step went over an interval's padding
    do {
#ifdef JDA_SEG_STEP_HOOK
        JDA_SEG_STEP_HOOK();                                        // (host simulator: counts the steps of a walk)
#endif
        if (RST && p >= next_bit) {                                 // (a walk off the decoder's path ran over an interval start: catch up)
            nr++; next_bit = (rpos[nr] << 3) - seg_bit0;
            if (nr > P.n_intervals) { nr = P.n_intervals; next_bit = 0xffffffffu; }
        }
        const bool isdc0 = k == 0;
        const uint32_t c = jda_bfe(csel, b2, 2u);
        const uint32_t w = jda_seg_reader_peek(R, p);
        // one lookup, one address: the table by the block's place in the MCU and DC / AC, the entry by the 11-bit key (the
        // stream's top 10 bits, or 1024 + the 10 bits behind six leading ones)
        const uint32_t tsel = jda_bfe(isdc0 ? dcsel : acsel, b2, 2u);
        const uint32_t key = jda_bfe(w, w >= 0xfc000000u ? 16u : 22u, 11u);
        const uint32_t e32 = *(const jda_u32_alias *)(wt + (tsel << 13) + (key << 2));      // (sums: two shift-adds onto the tables' address)
        const uint32_t e = e32 & 0xffffu;
        const uint32_t elow = e & 0xffu;
        // no such code (:2137-2138, :2237-2238).  A walk that is not on the decoder's path yet may meet anything: it steps
        // on one bit and keeps looking (a walk that gave up would hand "dead" down the chain of segments, one per round) -- a
        // one-bit symbol without effects, by selects; its sums are void from there on (sbad).
        const bool inval = elow == JDA_AC_NONE;
        sbad |= inval;
        const bool live = !inval;                                   // the step's effects count
        const bool isdc = isdc0 & live;
        const bool eob = (elow == JDA_AC_EOB) & !inval;
        const uint32_t len = inval ? 1u : (e >> 12) + 1u, sz = (eob | inval) ? 0u : (e >> 8) & 15u;
        const uint32_t kk = k + ((e >> 1) & 15u);                   // (DC: + 0)
        const bool dcmag = isdc & (sz != 0u) & ((e & 1u) == 0u);    // a DC magnitude the reference refills for (not folded into the LUT entry)
        const bool acmag = !isdc0 & live & (sz != 0u) & (kk < 64u); // an AC magnitude that is stored
        const uint32_t p1 = p + len;
        bool counted = false;
        if (REC) {
            // a counted block starts here: its record is its DC VALUE so far as the segment knows it -- the running sum of its
            // component's differences (:2155-2165; a folded entry holds the same value), its own included -- and the place of its first AC symbol
            // a DC category no 8-bit baseline stream has does not fit the record's 20-bit sum: such a file keeps to the serial pre-scan
            sbad |= isdc & (sz > 11u);
            counted = isdc & !sbad;
            const int32_t diff = (counted & (sz != 0u)) ? jda_extend_top(w << len, sz) : 0;
            ds0 += c == 0 ? diff : 0; ds1 += c == 1 ? diff : 0; ds2 += c >= 2 ? diff : 0;
            const int32_t run = c == 0 ? ds0 : (c == 1 ? ds1 : ds2);
            const uint32_t rec = (p1 + sz) | ((uint32_t)run << JDA_REC_POS_BITS);          // (<= 2047 + 27: twelve bits)
            rb0 = counted ? rb1 : rb0; rb1 = counted ? rb2 : rb1; rb2 = counted ? rb3 : rb2; rb3 = counted ? rec : rb3;
            const bool group = counted & ((nblk & 3u) == 3u), fits = nblk < P.rec_cap;      // (one branch region, not two nested ones)
            if (group & fits) jda_store_u32x4(recs + (nblk - 3u), rb0, rb1, rb2, rb3);
            sbad |= group & !fits;                                  // (jda_record_cap leaves no room for this; memory stays ours anyway)
            nblk += counted ? 1u : 0u;
            U = jda_lag_add(U, ((p & 7u) + len) >> 3);                   // whole bytes the code bits advance the stream position by
            const uint32_t f1 = ((U | kGuard) - 6u * kOnes) & kGuard;
            // SURVEY fact 6 without knowing the entry lag: the reference reads the magnitude at ulBitOff = 8 u + (p1 & 7) and loses
            // bits when that + sz > 64 -- u >= 7 for (p1 & 7) + sz in 9..16, u >= 6 above 16 (u <= 7 here) -- so the six candidate
            // lags are tested at once; the rare hit is kept with the lag word at the block's first AC symbol (jda_segscan_resolve)
            // (ulBitOff <= 47 in front of the code for every candidate lag: code + magnitude must be 17 bits and more -- rare symbols)
            const uint32_t m = acmag ? sz : 0u;
            max_ac = m > max_ac ? m : max_ac;
            if (__builtin_expect(acmag && len + sz > 16u && !sbad, 0)) {
                const uint32_t t = (p1 & 7u) + sz;
                const uint32_t f7 = ((U | kGuard) - 7u * kOnes) & kGuard;
                const uint32_t hit = t > 16u ? f1 : (t > 8u ? f7 : 0u);
                if (hit != 0u) {
                    const uint32_t at = jda_atomic_inc_u32(P.stats + JDA_ST_NCAND);
                    if (at < P.cand_cap) jda_store_u32x4(P.cands + (size_t)at * 4u, seg, nblk | (round << 16), Ublk, hit);
                }
            }
            U &= dcmag ? ~(f1 - (f1 >> 4)) : 0xffffffffu;           // the refill before an unfolded DC magnitude
            U = jda_lag_add(U, ((p1 & 7u) + sz) >> 3);
        }
        p = p1 + sz;
        const bool ends = (eob | (kk + 1u >= 64u)) & !inval;
        const uint32_t bn = b2 + 2u == nblocks2 ? 0u : b2 + 2u;
        // RST: this symbol completes an MCU within 7 bits of the next interval's start = it completes the interval
        const bool iend = RST & ends & live & (bn == 0u) & (next_bit - p < 8u);
#ifdef JDA_SEG_TRACE_HOOK
        JDA_SEG_TRACE_HOOK(OP, seg, p, k, kk, b2, bn, ends, iend, next_bit, nr, nblk, e, inval);
#endif
        const bool hold = iend & eob;                               // the refill after an interval's closing EOB waits for the rounding
        // ---- the refill at the end of the step (not after EOB in the reference -- there it is the next block's opening one)
        if (REC) {
            const uint32_t f = ((U | kGuard) - 6u * kOnes) & kGuard;
            U &= hold ? 0xffffffffu : ~(f - (f >> 4));
            Ublk = counted ? U : Ublk;                              // the lags at the block's first AC symbol (behind the refill at the top of the AC loop)
        }
        k = (ends | inval) ? 0u : kk + 1u;
        b2 = ends ? bn : b2;
        if (PAIR) {
            // the symbol behind an AC symbol that leaves its block open, where the table knows it (jda_wt_pair) and the segment goes
            // on: what a step of its own would do to the walk's state -- an AC symbol moves p, k, the lags and the largest size
            const uint32_t pd = e32 >> 16;
            const uint32_t dk = (pd >> 5) & 31u, kend = kk + 1u + dk;
            const bool last_b = (dk == 0u) | (kend >= 64u);         // B would end its block
            // (RST: a symbol that completes an MCU may complete the interval -- a step of its own, for the test above)
            const bool pair = (pd != 0u) & live & !ends & (p < JDA_SEG_BITS) & !(RST & last_b & (bn == 0u));
            const uint32_t bits_b = pair ? pd & 31u : 0u;
            const bool ends_b = pair & last_b;
            if (REC) {
                const uint32_t m = (pair & (dk != 0u) & (kend <= 64u)) ? (pd >> 10) & 15u : 0u;      // (a stored magnitude: the coefficient's place is in the block)
                max_ac = m > max_ac ? m : max_ac;
                U = jda_lag_add(U, ((p & 7u) + bits_b) >> 3);       // (no pair: no bytes, and no lag is at 6 behind the refill above ..
                const uint32_t f = ((U | kGuard) - 6u * kOnes) & kGuard;
                U &= (RST && !pair) ? 0xffffffffu : ~(f - (f >> 4)); // .. but behind an interval's closing EOB, whose refill waits: RST)
            }
            p += bits_b;
            k = pair ? (ends_b ? 0u : kend) : k;
            b2 = ends_b ? bn : b2;
        }
        if (RST) {
            if (iend) {                                             // over the padding to the next interval's first byte
                const uint32_t frac = (p & 7u) ? 1u : 0u;           // (interval starts are byte aligned, so are segment starts)
                if (REC) {
                    U = jda_lag_add(U, frac);
                    const uint32_t f = ((U | kGuard) - 6u * kOnes) & kGuard;
                    U &= ~(f - (f >> 4));
                    ds0 = ds1 = ds2 = 0;
                    first_rst = has_rst ? first_rst : nblk; has_rst = JDA_SEG_HAS_RESTART;
                }
                if (REC && !sbad && nr < P.n_intervals) {      // who ended the interval in front of start nr, and after how many of its blocks
                    uint32_t JDA_GLOBAL *ev = JDA_G(uint32_t, P.rst_events) + 2u * (size_t)nr;
                    ev[0] = (seg << 11) | (nblk + 1u); ev[1] = round;
                }
                p = next_bit;
                jumped = true;
                nr++; next_bit = nr <= P.n_intervals ? (rpos[nr] << 3) - seg_bit0 : 0xffffffffu;
            }
        }
        go = p < JDA_SEG_BITS;
        since++;
        // (the next peek must find p within the loaded dwords and at most one dword on: a lane that has used them up, or jumped over an
        // interval's padding, sits out the rest of the wavefront's steps until the reload)
    } while (go & (since < JDA_SEG_REFILL_STEPS) & jda_seg_reader_holds(R, p) & !(RST && jumped));
    }
    if (REC) {                                                      // what is left of the last group, slot by slot
        const uint32_t r = nblk & 3u, n4 = nblk & ~3u;
        if (nblk <= P.rec_cap) {
            if (r > 0u) recs[n4 + r - 1u] = rb3;
            if (r > 1u) recs[n4 + r - 2u] = rb2;
            if (r > 2u) recs[n4 + r - 3u] = rb1;
        }
        S.lag_last = Ublk; S.max_ac = max_ac;
        uint32_t map = 0;
        for (int j = 0; j < 6; j++) map |= ((U >> (5 * j)) & 7u) << (3 * j);
        S.phase_map = map;
    }
    S.nblk = nblk; S.dcsum[0] = ds0; S.dcsum[1] = ds1; S.dcsum[2] = ds2;
    S.bad = (sbad ? 1u : 0u) | has_rst | (first_rst << JDA_SEG_FIRST_RST_SHIFT);
    return (p - JDA_SEG_BITS) | (b2 << 5) | (k << 9);
}

// ---- the marker filter's state machine on sixteen bytes at once (jda_filter_*, jda_kernels.hip) ------------------------------
// JPEGFilter (jpeg.inl:1431-1540) is a two-state machine: an FF in state 0 waits for its partner (state 1); the partner is dropped
// with it unless it is 00 (then FF is emitted); state 0 again.  After any byte that is not FF the state is 0, so the state in front
// of byte i is the parity of its distance from the start of the run of FFs that ends at i - 1: runs that start at an even position
// put state 1 in front of odd positions and vice versa, and adding the start bits of the even-started runs to the FF mask clears
// exactly those runs (the carry runs through a run and stops behind it).  cin: the state in front of byte 0 -- then byte 0 is a
// partner, and a run of FFs from byte 0 on counts as started at -1.
struct jda_filter_bits { uint32_t S, E, R; };       // state in front of byte i (bits 0..16), byte i is emitted / a restart marker's second byte (bits 0..15)
JDA_HD uint32_t jda_zero_byte_bits(uint32_t x)      // bit 7 of every byte that is zero
{
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
// bits 7, 15, 23, 31 -> 0..3 (one dot product of bytes; the multiply-and-shift of the textbook is a quarter-rate v_mul_lo_u32)
JDA_HD uint32_t jda_byte_flags_to_nibble(uint32_t f) { return jda_udot4(f >> 7, 0x08040201u); }
struct jda_filter_masks { uint32_t ff, zero, rst; };  // per byte of the sixteen: is FF / is 00 / is D0..D7
JDA_HD jda_filter_masks jda_filter_classify(const uint32_t b[4])
{
    jda_filter_masks M;
    M.ff = M.zero = M.rst = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        M.ff |= jda_byte_flags_to_nibble(jda_zero_byte_bits(~b[d])) << (4 * d);
        M.zero |= jda_byte_flags_to_nibble(jda_zero_byte_bits(b[d])) << (4 * d);
        M.rst |= jda_byte_flags_to_nibble(jda_zero_byte_bits((b[d] & 0xf8f8f8f8u) ^ 0xd0d0d0d0u)) << (4 * d);
    }
    return M;
}
JDA_HD jda_filter_bits jda_filter_run(const jda_filter_masks &M, uint32_t valid, uint32_t cin)
{
    const uint32_t V = (1u << valid) - 1u;                           // valid <= 16
    const uint32_t starts = M.ff & ~(M.ff << 1);
    const uint32_t es = starts & 0x5555u & ~cin;                    // (cin: a run from byte 0 on is the tail of one that started at -1)
    const uint32_t Re = M.ff & ~(M.ff + es), Ro = M.ff & ~Re;
    jda_filter_bits F;
    F.S = ((Re << 1) & 0x0aaaau) | ((Ro << 1) & 0x15555u) | cin;
    F.E = V & ((~F.S & ~M.ff) | (F.S & M.zero));
    F.R = V & F.S & M.rst;
    return F;
}

// ---- from records to the index (block-parallel) ----------------------------------------------------------
// Index format 2: entry = the reader at the block's FIRST AC SYMBOL, blk_dc = the block's own DC value.  The entry of a block the
// reference reads without truncation is CANONICAL here: (p >> 3) << 7 | (p & 7) for the bit position p -- P1 needs p alone
// (pos * 8 + off, whatever the split); only a block flagged JDA_INDEX_TRUNC carries the reference reader's true (pBuf, ulBitOff)
// there, which its emulation starts from.  The serial pre-scan writes the true phase everywhere: the two indexes agree on p and
// on the flag of every block and on the whole entry of a flagged one.  The closing entry (behind the last block) bounds the scan
// from above: the serial pre-scan's is the reader as the last block left it, this one's lies behind the DC symbol that the stream's
// padding decodes to -- at most 34 bits further on (nothing reads it as a position: the last tile's window ends there).
JDA_HD uint32_t jda_index_canonical(uint32_t p_abs) { return ((p_abs >> 3) << JDA_INDEX_OFF_BITS) | (p_abs & 7u); }
struct jda_fin_acc { uint32_t bad, terminal, max_abs_dc; };
// record i of segment seg (first block ordinal g0, DC values pr0..2 of the components at its entry: jda_segscan_sums; rst_from: the
// segment's first record behind an interval end, 0xffffffff without one) -> index entry, DC value
// b0 = g0 % P.nblocks, inv = jda_fin_recip(P.nblocks): the block's place in the MCU without a division per record
JDA_HD uint32_t jda_fin_recip(uint32_t nblocks) { return (65536u + nblocks - 1u) / nblocks; }      // x / n = x * inv >> 16 while x * n < 65536
// (the record's load apart from its use: the kernel asks for the records of several segments before it waits for the first)
JDA_HD uint32_t jda_finalize_load(const jda_segscan_params &P, uint32_t seg, uint32_t i) { return JDA_G(const uint32_t, P.records)[(size_t)seg * P.rec_cap + i]; }
JDA_HD uint32_t jda_fin_rst_from(uint32_t sum5) { return (sum5 & JDA_SEG_HAS_RESTART) ? sum5 >> JDA_SEG_FIRST_RST_SHIFT : 0xffffffffu; }
JDA_HD void jda_finalize_apply(const jda_segscan_params &P, uint32_t seg, uint32_t i, uint32_t rec, uint32_t g0, uint32_t b0, uint32_t inv, int32_t pr0, int32_t pr1, int32_t pr2,
                               uint32_t rst_from, jda_fin_acc &A)
{
    const uint32_t g = g0 + i;
    if (g > P.n_blocks_total) return;                               // behind the image: padding decoded as blocks
    const uint32_t p_abs = seg * JDA_SEG_BITS + (rec & ((1u << JDA_REC_POS_BITS) - 1u));
    // a stream that ends early has been read on into its zero padding: the serial pre-scan knows what the reference does with it
    // (its test is on the reference's pBuf, at most five bytes behind: the margin makes this one the stricter)
    if ((p_abs >> 3) + 8u > P.scan_len + JDA_SCAN_PAD - 8u) A.bad = 1;
    if (g == P.n_blocks_total) {                                    // behind the last block: the closing entry (an upper bound, see above)
        JDA_G(uint32_t, P.blk_index)[g] = jda_index_canonical(P.restart_pos ? ((p_abs + 7u) & ~7u) : p_abs);
        A.terminal++;
        return;
    }
    const uint32_t x = b0 + i, b = x - jda_umul24(jda_umul24(x, inv) >> 16, P.nblocks), c = b < P.nluma ? 0u : b - P.nluma + 1u;      // (x < 6 + rec_cap)
    const int32_t base = i >= rst_from ? 0 : (c == 0u ? pr0 : (c == 1u ? pr1 : pr2));      // (DC values restart at zero with an interval)
    const int32_t dc = base + ((int32_t)rec >> JDA_REC_POS_BITS);
    if (dc < -32768 || dc > 32767) A.bad = 1;
    const uint32_t a = (uint32_t)(dc < 0 ? -dc : dc);
    A.max_abs_dc = a > A.max_abs_dc ? a : A.max_abs_dc;
    JDA_G(uint32_t, P.blk_index)[g] = jda_index_canonical(p_abs);
    JDA_G(int16_t, P.blk_dc)[g] = (int16_t)dc;
}
JDA_HD void jda_finalize_item(const jda_segscan_params &P, uint32_t seg, uint32_t i, uint32_t g0, uint32_t b0, uint32_t inv, int32_t pr0, int32_t pr1, int32_t pr2, uint32_t rst_from, jda_fin_acc &A)
{
    if (g0 + i > P.n_blocks_total) return;
    jda_finalize_apply(P, seg, i, jda_finalize_load(P, seg, i), g0, b0, inv, pr0, pr1, pr2, rst_from, A);
}
// candidate ci: a magnitude read that some entry lag of its segment truncates.  With the segment's true lag known: does it?  Then
// the block's entry becomes the reference reader's true phase (at the block's first AC symbol) + the flag.  Returns 1 for a
// truncated read (the serial pre-scan's count).
JDA_HD uint32_t jda_resolve_item(const jda_segscan_params &P, uint32_t ci)
{
    const uint32_t JDA_GLOBAL *cd = JDA_G(const uint32_t, P.cands) + (size_t)ci * 4u;
    const uint32_t seg = cd[0], ord = cd[1] & 0xffffu, round = cd[1] >> 16, hit = cd[3];
    const uint32_t JDA_GLOBAL *sum = JDA_G(const uint32_t, P.seg_sum);
    const uint32_t JDA_GLOBAL *st = JDA_G(const uint32_t, P.seg_start);
    if (seg >= P.n_segs || sum[(size_t)seg * JDA_SEG_SUM_WORDS + 7u] != round) return 0;      // the segment was walked again: not its last walk's candidate
    const uint32_t g0 = st[(size_t)seg * JDA_SEG_START_WORDS], j = st[(size_t)seg * JDA_SEG_START_WORDS + 4u];
    if (g0 >= 0xfffffff0u || !((hit >> (4u + 5u * j)) & 1u)) return 0;
    uint32_t t = seg, i = ord - 1u, lagw = cd[2], jt = j, g = g0 + i;
    if (ord == 0u) {                                                // the block was open at the segment's entry: it started in ..
        if (seg == 0u) return 0;
        do { t--; } while (t > 0u && sum[(size_t)t * JDA_SEG_SUM_WORDS] == 0u);              // .. the last segment before that starts a block
        const uint32_t nb = sum[(size_t)t * JDA_SEG_SUM_WORDS];
        if (nb == 0u) return 0;
        i = nb - 1u; lagw = sum[(size_t)t * JDA_SEG_SUM_WORDS + 6u]; jt = st[(size_t)t * JDA_SEG_START_WORDS + 4u]; g = g0 - 1u;
    }
    if (g >= P.n_blocks_total || i >= P.rec_cap) return 0;
    const uint32_t rec = JDA_G(const uint32_t, P.records)[(size_t)t * P.rec_cap + i];
    const uint32_t p_abs = t * JDA_SEG_BITS + (rec & ((1u << JDA_REC_POS_BITS) - 1u));
    const uint32_t u0 = (lagw >> (5u * jt)) & 15u;                  // the window's byte lag at the block's first AC symbol (behind the AC loop's opening refill)
    JDA_G(uint32_t, P.blk_index)[g] = (((p_abs >> 3) - u0) << JDA_INDEX_OFF_BITS) | JDA_INDEX_TRUNC | (8u * u0 + (p_abs & 7u));
    return 1;
}
// interval start nr (1 .. n_intervals - 1): did a settled walk end the interval in front of it, after exactly nr x interval_blocks
// blocks?  (The reference counts MCUs and never looks where the markers were: the two must agree.)  Returns 1 for a mismatch.
JDA_HD uint32_t jda_rst_event_item(const jda_segscan_params &P, uint32_t nr)
{
    const uint32_t JDA_GLOBAL *ev = JDA_G(const uint32_t, P.rst_events) + 2u * (size_t)nr;
    const uint32_t e = ev[0];
    // The reference restarts by MCU count and never looks for the markers.  A marker behind the image's last block by that count
    // is one it never gets to; every other one must stand exactly where the count puts it -- also when a damaged interval has the
    // walk reach the marker only behind the image's last block (found by the pipeline's fuzz: the reference had restarted 2,000 bits
    // earlier, in the middle of what the walk took for one interval).
    const uint64_t want = (uint64_t)nr * P.interval_blocks;
    if (want >= P.n_blocks_total) return 0u;
    if (e == 0u) return 1u;                                         // nobody ended an interval at this marker
    const uint32_t seg = e >> 11, nb = (e & 2047u) - 1u;
    if (seg >= P.n_segs || JDA_G(const uint32_t, P.seg_sum)[(size_t)seg * JDA_SEG_SUM_WORDS + 7u] != ev[1]) return 1u;      // .. not in its segment's last walk
    const uint32_t g0 = JDA_G(const uint32_t, P.seg_start)[(size_t)seg * JDA_SEG_START_WORDS];
    if (g0 >= 0xfffffff0u) return 0u;                               // behind a bad code: the image is rejected for that
    return (uint64_t)g0 + nb == want ? 0u : 1u;
}

// ================================================================================================
// Tile phases.  Every lane of the tile's wavefront runs each phase; a wave-local fence separates
// consecutive phases (the host emulator runs all 64 lanes of a phase, then the next).
//
//   P0  tables -> LDS, the tile's slice of the scan -> LDS window, zero the list counters
//   P1  thread = block: Huffman/RLE expand into the block's int16[64] in LDS (JPEGDecodeMCU,
//       jpeg.inl:2090-2274); classify the block and append its non-empty columns / its row class to
//       work lists.  Scaled 1/4 and 1/8 outputs are finished here (2x2 IDCT or DC fill).
//   P2  thread = (block, non-empty column): dequant + column stage of the IDCT (jpeg.inl:2553-2679).
//       Empty columns cost nothing -- the reference's own shortcut (:2555-2560), made data-parallel
//       by compacting the work items (wave prefix sum / ballots, jda_p1_lists).
//   P3  thread = (block, row): row stage + range limit (jpeg.inl:2680-2797), blocks grouped by the
//       reference's row variant so that a pass never mixes variants.  8 samples -> the MCU's plane.
//   P4  threads tile the output rows: colour conversion and coalesced stores (JPEGPutMCU*).
// ================================================================================================

// component table ids: the descriptor bytes are workgroup-uniform (scalar loads); pick by the
// lane's component with selects instead of a per-lane indexed global load
JDA_HD uint32_t jda_pick3(const uint8_t ids[3], uint32_t c)
{
    const uint32_t a = ids[0], b = ids[1], d = ids[2];
    return c == 0 ? a : (c == 1 ? b : d);
}

struct jda_tile_ctx {                 // wave-uniform facts about the tile, computed once per thread
    uint32_t first_mcu;               // linear MCU index of the tile's first MCU
    uint32_t count;                   // MCUs of the tile that are decoded (<= MCUS, clipped by n_mcus_ok; 0 = padding tile)
    uint32_t first_block;             // linear block index of the tile's first block
    uint32_t win_lo, win_len;         // bytes of the scan staged in LDS
    uint32_t win_need;                // bytes the tile's lanes can touch (> win_len: some reads go to HBM)
};

// same, from index entries already in registers: ix_first = index[first block of the tile],
// ix_end = index[first block after the tile]
template <int MODE>
JDA_HD jda_tile_ctx jda_tile_setup_from(const jda_dev_desc &D, const jda_strip &S, uint32_t ix_first, uint32_t ix_end, uint32_t win_cap = (uint32_t)jda_lds_layout<MODE>::WIN_BYTES)
{
    typedef jda_mode_traits<MODE> T;
    jda_tile_ctx C;
    C.first_mcu = S.mcu_y * D.mcus_x + S.mcu_x0;
    C.count = S.count;
    if (C.first_mcu >= D.n_mcus_ok) C.count = 0;
    else if (C.first_mcu + C.count > D.n_mcus_ok) C.count = D.n_mcus_ok - C.first_mcu;
    C.first_block = C.first_mcu * T::NBLK;
    C.win_lo = 0; C.win_len = 0; C.win_need = 0;
    if (C.count && D.scale_shift != 3 && !(D.pad_[0] & JDA_DESC_DC_ONLY)) {      // (1/8, a progressive file's DC scan: the DC values are all there is, the scan is not read)
        C.win_lo = (ix_first >> JDA_INDEX_OFF_BITS) & ~15u;
        uint32_t hi = ((ix_end >> JDA_INDEX_OFF_BITS) + 8u + 12u + 15u) & ~15u;
        const uint32_t cap = (D.scan_len + JDA_SCAN_PAD) & ~15u;
        if (hi > cap) hi = cap;
        C.win_len = hi > C.win_lo ? hi - C.win_lo : 0;
        // (the slice is asked for by every lane, whatever its length -- jda_window_load --, so an empty one must still start inside the
        // scan: the streamed pipeline launches a decode before the pre-scan's verdict, the entries of a damaged stream may point anywhere)
        if (C.win_len == 0) C.win_lo = 0;
        C.win_need = C.win_len;
        if (C.win_len > win_cap) C.win_len = win_cap;
    }
    return C;
}

template <int MODE>
JDA_HD jda_tile_ctx jda_tile_setup(const jda_dev_desc &D, const jda_strip &S)
{
    typedef jda_mode_traits<MODE> T;
    jda_tile_ctx C;
    C.first_mcu = S.mcu_y * D.mcus_x + S.mcu_x0;
    C.count = S.count;
    if (C.first_mcu >= D.n_mcus_ok) C.count = 0;
    else if (C.first_mcu + C.count > D.n_mcus_ok) C.count = D.n_mcus_ok - C.first_mcu;
    C.first_block = C.first_mcu * T::NBLK;
    C.win_lo = 0; C.win_len = 0; C.win_need = 0;
    if (C.count && D.scale_shift != 3 && !(D.pad_[0] & JDA_DESC_DC_ONLY)) {
        // the tile's blocks are consecutive in the scan: stage one contiguous run of bytes
        C.win_lo = (JDA_G(const uint32_t, D.blk_index)[C.first_block] >> JDA_INDEX_OFF_BITS) & ~15u;
        // a thread may read 12 bytes past (start of the block after the tile) + 8
        uint32_t hi = ((JDA_G(const uint32_t, D.blk_index)[C.first_block + C.count * T::NBLK] >> JDA_INDEX_OFF_BITS) + 8u + 12u + 15u) & ~15u;
        const uint32_t cap = (D.scan_len + JDA_SCAN_PAD) & ~15u;      // never past the padded allocation
        if (hi > cap) hi = cap;
        C.win_len = hi > C.win_lo ? hi - C.win_lo : 0;
        if (C.win_len == 0) C.win_lo = 0;
        C.win_need = C.win_len;
        if (C.win_len > (uint32_t)jda_lds_layout<MODE>::WIN_BYTES) C.win_len = (uint32_t)jda_lds_layout<MODE>::WIN_BYTES;
    }
    return C;
}

// ---- P0 ---------------------------------------------------------------------------------------
// the set bits of the nibble m, lowest first, in 3-bit fields (unused fields 0)
JDA_HD uint32_t jda_nibble_list(uint32_t m)
{
    uint32_t r = 0, n = 0;
    for (uint32_t b = 0; b < 4; b++) if ((m >> b) & 1u) { r |= b << (3u * n); n++; }
    return r;
}
// tables: once per workgroup (tid = thread in workgroup, nthreads = workgroup size)
// with_long: also the long halves of the AC LUTs (JDA_LT_LONG; tab_lds then holds JDA_LT_BYTES + JDA_LT_LONG_BYTES)
JDA_HD void jda_p0_tables_from(const uint8_t *tables, uint32_t tid, uint32_t nthreads, uint8_t *tab_lds, bool with_long = false);
JDA_HD void jda_p0_tables(const jda_dev_desc &D, uint32_t tid, uint32_t nthreads, uint8_t *tab_lds, bool with_long = false) { jda_p0_tables_from(D.tables, tid, nthreads, tab_lds, with_long); }
JDA_HD void jda_p0_tables_from(const uint8_t *tables, uint32_t tid, uint32_t nthreads, uint8_t *tab_lds, bool with_long)
{
    const jda_chunk16_alias JDA_GLOBAL *blob = JDA_G(const jda_chunk16_alias, tables);
    jda_chunk16_alias *tab = (jda_chunk16_alias *)tab_lds;
    // DC LUTs: blob[0, 2048) -> LT_DC ; AC short halves: blob[2048 + k*4096, +2048) -> LT_AC + k*2048 ;
    // quant: blob[10240, 10752) -> the DC LUTs' unused bytes; zigzag: built below
    for (uint32_t j = tid; j < JDA_ZZ_ENTRIES; j += nthreads) {  // zigzag + flag bits of A.2 in one lookup
        uint32_t v = JDA_ZZ_DUMP;
        if (j < 64) {
            const uint32_t n = JDA_G(const uint8_t, tables)[JDA_TB_ZIGZAG + j];
            v = (n << 1) | ((1u << (n & 7u)) << 8);
        }
        ((uint16_t *)(tab_lds + JDA_LT_ZZ))[j] = (uint16_t)v;
    }
    (void)with_long;
    for (uint32_t i = tid; i < JDA_LT_ZZ / 16; i += nthreads) {
        uint32_t src;
        if (i < 128) {                                          // DC LUTs; chunks 16..31 of each (bytes 256..511) take two quantiser tables
            const uint32_t within = i & 63u;
            src = (within >= 16u && within < 32u) ? (JDA_TB_QUANT >> 4) + (i >> 6) * 16u + (within - 16u) : i;
            if (i == (JDA_LT_EOB >> 4)) src = JDA_TB_EOB >> 4;      // (bytes 64..127 of a DC LUT are never read either)
            if (i == (JDA_LT_NIB >> 4) || i == (JDA_LT_NIB >> 4) + 1u) {
                jda_chunk16_alias nb;
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) nb.w[k] = jda_nibble_list((i - (JDA_LT_NIB >> 4)) * 8u + 2u * k) | (jda_nibble_list((i - (JDA_LT_NIB >> 4)) * 8u + 2u * k + 1u) << 16);
                tab[i] = nb;
                continue;
            }
        }
        else src = (JDA_TB_AC >> 4) + (i - 128);                // the AC LUTs, both halves of both tables, in the blob's order
        jda_chunk16_alias c = blob[src];
        if (i >= 128) {                                         // AC entries -> the kernels' layout
#pragma unroll
            for (int k = 0; k < 4; k++) c.w[k] = jda_ac_entry(c.w[k] & 0xffffu) | (jda_ac_entry(c.w[k] >> 16) << 16);
        }
        tab[i] = c;
    }
}

// per wave: zero the list counters, stage the tile's slice of the scan
template <int MODE>
JDA_HD void jda_p0_stage(const jda_dev_desc &D, const jda_tile_ctx &C, uint32_t t, uint8_t *wl, uint32_t win_cap)
{
    typedef jda_lds_layout<MODE> L;
    if (t < 8) ((uint32_t *)(wl + L::CNT_OFF))[t] = 0;
    const uint32_t len = C.win_len < win_cap ? C.win_len : win_cap;
    jda_window_fill(JDA_G(const uint8_t, D.scan), C.win_lo, len, wl + L::WIN_OFF, t);
}

// What a lane of P1 needs that depends only on the image and on the lane -- its block's place in the MCU decides the
// component, hence the Huffman LUTs and the quantiser table -- worked out when a wavefront meets a new image (LDS
// addresses are 32 bits: five registers), not once per tile.
struct jda_lane_pre {          // (offsets, not pointers: a pointer carried around the tile loop loses its address space)
    uint32_t dc_off;          // byte offset in the LDS table copy: DC LUT of the lane's component
    uint32_t ac_off;          // its AC LUT (short half)
    uint32_t ac_long_off;     // byte offset of the AC LUT's long half in the table blob (global)
    uint32_t quant_off;       // byte offset of its quantiser table in the LDS table copy
    uint32_t qsel;            // (offset of the quantiser table / 128) << 10: the column work items carry it
    uint32_t chroma;          // the lane's block is a chroma block
    uint32_t eob_sh, eob_code;   // the next symbol is EOB when (next 32 stream bits >> eob_sh) == eob_code (JDA_TB_EOB)
    uint32_t item_pre;        // qsel | lane << 4: a column work item of the lane's block, less its column (which rides in bits 3:1: a byte offset)
};
template <int MODE>
JDA_HD void jda_lane_prepare(jda_lane_pre &LP, const jda_dev_desc &D, uint32_t lane, const uint8_t *tab)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t b = lane % (uint32_t)T::NBLK;                  // block within the MCU
    const uint32_t c = b < (uint32_t)T::NLUMA ? 0u : b - T::NLUMA + 1u;
    // (jda_pick3 reads the three ids into values first: a select between the array's elements becomes a dynamically
    // indexed load, and that sends the whole descriptor from SGPRs to scratch memory)
    const uint32_t dc_id = jda_pick3(D.dc_id, c), ac_id = jda_pick3(D.ac_id, c), q_id = jda_pick3(D.q_id, c);
    const uint32_t eob = *(const jda_u32_alias *)(tab + JDA_LT_EOB + 4u * ac_id);   // (the image's tables must be staged)
    LP.eob_sh = eob >> 16; LP.eob_code = eob & 0xffffu;
    LP.dc_off = JDA_LT_DC + dc_id * 1024;
    LP.ac_off = JDA_LT_AC + ac_id * 4096;
    LP.ac_long_off = JDA_TB_AC + (ac_id * 2048 + 1024) * 2;
    LP.quant_off = JDA_LT_QUANT_OFF(q_id);
    LP.qsel = (JDA_LT_QUANT_OFF(q_id) >> 7) << 10;                // (the table's offset in units of 128 bytes)
    LP.item_pre = LP.qsel | (lane << 4);
    LP.chroma = b >= (uint32_t)T::NLUMA ? 1u : 0u;
}

// ---- P1 ---------------------------------------------------------------------------------------
// What a thread needs from HBM before it can start decoding its block: issued at kernel entry so the
// two dependent loads (lane schedule -> index entry) overlap P0's table / window staging.
struct jda_p1_inputs { uint32_t lb, ix; int32_t pred; bool active; };

template <int MODE>
JDA_HD jda_p1_inputs jda_p1_prefetch(const jda_dev_desc &D, const jda_tile_ctx &C, uint32_t t)
{
    typedef jda_mode_traits<MODE> T;
    jda_p1_inputs in;
    in.lb = 0; in.ix = 0; in.pred = 0;
    in.active = t < C.count * T::NBLK;
    if (in.active) {
        in.lb = t;
        const uint32_t gb = C.first_block + in.lb;
        in.ix = JDA_G(const uint32_t, D.blk_index)[gb];
        in.pred = JDA_G(const int16_t, D.blk_dc)[gb];
    }
    return in;
}

// Result of a lane's P1: the block's occupancy flags (A.2; 0 = DC-only), or JDA_NO_LIST when the lane has
// nothing for the IDCT work lists (no block, chroma of a luma-only decode, 1/4 and 1/8 scale).
#define JDA_NO_LIST 0xffffffffu

template <int MODE>
JDA_HD uint32_t jda_p1_entropy(const jda_dev_desc &D, const jda_tile_ctx &C, const jda_p1_inputs &in, const jda_lane_pre &LP, const uint8_t *tab, uint8_t *wl,
                               const uint8_t *win, uint32_t win_cap)
{
    typedef jda_lds_layout<MODE> L;
    if (!in.active) return JDA_NO_LIST;
    JDA_P1_TRACE(10);
    const uint32_t lb = in.lb;                                   // (== the lane: LP was made for it)
    if (MODE != JDA_MODE_GRAY && D.gray_from_color && LP.chroma) return JDA_NO_LIST;   // :5225-5233 chroma never decoded
    jda_tables TB;
    TB.dc = tab + LP.dc_off;
    TB.ac_short = (const uint16_t *)(tab + LP.ac_off);
    TB.ac_long = (const uint16_t JDA_GLOBAL *)(JDA_G(const uint8_t, D.tables) + LP.ac_long_off);
    TB.ac_long_lds = TB.ac_short + 1024;
    TB.zz = (const uint16_t *)(tab + JDA_LT_ZZ);
    TB.eob_sh = LP.eob_sh; TB.eob_code = LP.eob_code;
    const int16_t *quant = (const int16_t *)(tab + LP.quant_off);
    int16_t *coef = (int16_t *)(wl + L::COEF_OFF + lb * JDA_COEF_STRIDE);
    uint8_t *plane = (uint8_t *)coef;                            // samples overwrite the block's own slot

    jda_bitreader br;
    br.base = JDA_G(const uint8_t, D.scan);
    br.win = win;
    br.win_lo = C.win_lo;
    br.win_len = C.win_len < win_cap ? C.win_len : win_cap;
    const uint32_t ix = in.ix;
    const bool trunc = (ix & JDA_INDEX_TRUNC) != 0u;             // the entry holds the reference reader's true phase (else maybe a canonical one)
    br.pos = ix >> JDA_INDEX_OFF_BITS;
    br.off = ix & (JDA_INDEX_TRUNC - 1u);
    const uint8_t *wbase = br.win - br.win_lo;
    const int32_t dc = in.pred;                                  // the block's own DC value (index format 2)

    JDA_P1_TRACE(8);
    const int shift = D.scale_shift;
    const bool dc_only = (D.pad_[0] & JDA_DESC_DC_ONLY) != 0;     // wave-uniform: the DC scan of a progressive file -- no AC symbol exists (JPEGDecodeMCU_P with Se = 0)
    if (shift == 3 || (dc_only && shift == 2)) {                 // 1/8: the DC term is the pixel (:5146-5154, bThumbnail) -- the scan is not read at all
        *(jda_u32_alias *)plane = jda_dup8(jda_range_limit5(dc * (int32_t)quant[0]));
        return JDA_NO_LIST;
    }
    if (dc_only) {                                               // (a progressive file asked for at full or half size: DC-only blocks through the IDCT's bypass)
        jda_u64_alias *z = (jda_u64_alias *)coef;
        z[0] = (uint64_t)(uint16_t)dc;
#pragma unroll
        for (int i = 1; i < 16; i++) z[i] = 0;
        return 0;
    }
    // wave-uniform: the whole slice is in LDS (and the tables allow the window-only reader's EOB test)
    const bool win_only = C.win_need <= br.win_len && !(D.pad_[0] & JDA_DESC_GENERAL_P1);
    if (shift == 2) {                                            // 1/4: 2x2 from coefficients 0,1,8,9
        uint32_t flags;
        if (win_only) flags = jda_decode_block_win<5, true, L::LONG_LDS != 0>(br.pos, br.off, wbase, TB, coef, dc, true, trunc);
        else { br.bits = jda_load_be64(br, br.pos); flags = jda_decode_block<5>(br, TB, coef, dc, trunc); }
        const uint32_t px = flags == 0 ? jda_dup8(jda_range_limit5(dc * (int32_t)quant[0]))
                                       : jda_idct_2x2(coef, quant);
        *(jda_u32_alias *)plane = px;
        return JDA_NO_LIST;
    }
    uint32_t flags;
    if (win_only) {
        // the reference's ulBitOff is followed only in a tile that holds a block with a truncated magnitude read (the
        // pre-scan flags those: a fraction of a percent of the blocks of a photograph, none of most synthetic images)
        if (jda_wave_any(trunc)) flags = jda_decode_block_win<64, true, L::LONG_LDS != 0>(br.pos, br.off, wbase, TB, coef, dc, true, trunc);
        else flags = jda_decode_block_win<64, false, L::LONG_LDS != 0>(br.pos, br.off, wbase, TB, coef, dc, true);
    }
    else { br.bits = jda_load_be64(br, br.pos); flags = jda_decode_block<64>(br, TB, coef, dc, trunc); }
    JDA_P1_TRACE(9);
    return flags;
}

// ---- P1 in chunks (images whose index carries continuation entries: photographs, high qualities) -------------------------------
// A wavefront runs P1's symbol loop as long as its longest block, and the blocks of a photograph differ by a factor of ten -- a luma
// block of forty symbols beside chroma blocks of four: 23-41 % of the lanes' trips do work (profiles/r04_p1_lane_balance_estimate.txt).
// With an entry every JDA_CONT_SYMS symbols of a long block (JDA_CONT_*: both pre-scans write them as they pass) the tile's work is
//   pass A   lane = block: the block's first chunk (<= 8 symbols) -- clears the block, stores its DC value;
//   passes B lane = continuation entry e of the tile (they are contiguous in memory, blocks in order: entry C0 + 64 p + lane): the
//            chunk behind it, into ITS block's coefficients; the block's bit position comes from the lane that owns the block
//            (ds_bpermute), the chunk's flag word is ORed into the block's slot (ds_or_b32 on JDA_SLOT_FLAGS);
//   finish   lane = block: own flag word | the slot's.
// A block flagged JDA_INDEX_TRUNC is decoded whole by its own lane in pass A (the reference's ulBitOff has to be followed from the
// block's first symbol); a tile whose slice of the scan does not fit the LDS window takes the general reader, whole blocks.
// cross-lane read (GPU: ds_bpermute, every lane of the wavefront active; host emulator: the array of every lane's value)
JDA_HD uint32_t jda_lane_pull(uint32_t mine, uint32_t src, const uint32_t *all)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)all;
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)mine);
#else
    (void)mine;
    return all[src & 63u];
#endif
}
JDA_HD void jda_lds_or_u32(uint8_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_or((uint32_t *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    *(jda_u32_alias *)p |= v;
#endif
}
#define JDA_P1C_SKIP  0x80000000u    // own.bits: the lane has no block to share (no block, chroma of a luma-only decode, a flagged block, a tile on the general reader)
struct jda_p1c_own { uint32_t bits;  // bit position of the block's first AC symbol | JDA_P1C_SKIP
                     uint32_t fl;    // pass A's flag word (chunk mode: the OR of zigzag entries; whole mode: the block's folded flags)
                     uint32_t whole; // the block was decoded whole in pass A
                     uint32_t listed; };
template <int MODE>
JDA_HD void jda_p1c_tables(jda_tables &TB, const jda_dev_desc &D, uint32_t blk_lane, const uint8_t *tab)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t b = blk_lane % (uint32_t)T::NBLK, c = b < (uint32_t)T::NLUMA ? 0u : b - T::NLUMA + 1u;
    const uint32_t ac_id = jda_pick3(D.ac_id, c);
    const uint32_t eob = *(const jda_u32_alias *)(tab + JDA_LT_EOB + 4u * ac_id);
    TB.dc = tab; TB.ac_short = (const uint16_t *)(tab + JDA_LT_AC + ac_id * 4096u); TB.ac_long = nullptr; TB.ac_long_lds = TB.ac_short + 1024;
    TB.zz = (const uint16_t *)(tab + JDA_LT_ZZ);
    TB.eob_sh = eob >> 16; TB.eob_code = eob & 0xffffu;
}
// pass A.  chunked: the tile takes the chunked path (uniform: its slice is in the window, the tables allow the window reader)
template <int MODE>
JDA_HD jda_p1c_own jda_p1c_block(const jda_dev_desc &D, const jda_tile_ctx &C, const jda_p1_inputs &in, const jda_lane_pre &LP, const uint8_t *tab, uint8_t *wl,
                                 const uint8_t *win, uint32_t win_cap, bool chunked)
{
    typedef jda_lds_layout<MODE> L;
    jda_p1c_own O;
    O.bits = JDA_P1C_SKIP; O.fl = 0; O.whole = 1; O.listed = 0;
    if (!in.active) return O;
    if (MODE != JDA_MODE_GRAY && D.gray_from_color && LP.chroma) return O;
    O.listed = 1;
    jda_tables TB;
    TB.dc = tab + LP.dc_off;
    TB.ac_short = (const uint16_t *)(tab + LP.ac_off);
    TB.ac_long = nullptr;
    TB.ac_long_lds = TB.ac_short + 1024;
    TB.zz = (const uint16_t *)(tab + JDA_LT_ZZ);
    TB.eob_sh = LP.eob_sh; TB.eob_code = LP.eob_code;
    int16_t *coef = (int16_t *)(wl + L::COEF_OFF + in.lb * JDA_COEF_STRIDE);
    const uint32_t ix = in.ix;
    const bool trunc = (ix & JDA_INDEX_TRUNC) != 0u;
    const uint32_t pos = ix >> JDA_INDEX_OFF_BITS, off = ix & (JDA_INDEX_TRUNC - 1u);
    const uint32_t win_len = C.win_len < win_cap ? C.win_len : win_cap;
    const uint8_t *wbase = win - C.win_lo;
    if (!chunked) {                                              // the general reader, whole blocks (as jda_p1_entropy)
        jda_bitreader br;
        br.base = JDA_G(const uint8_t, D.scan); br.win = win; br.win_lo = C.win_lo; br.win_len = win_len; br.pos = pos; br.off = off;
        const bool win_only = C.win_need <= win_len && !(D.pad_[0] & JDA_DESC_GENERAL_P1);
        if (win_only) O.fl = jda_decode_block_win<64, true, true>(pos, off, wbase, TB, coef, in.pred, true, trunc);
        else { br.bits = jda_load_be64(br, br.pos); O.fl = jda_decode_block<64>(br, TB, coef, in.pred, trunc); }
        return O;
    }
    *(jda_u64_alias *)((uint8_t *)coef + JDA_SLOT_FLAGS) = 0;    // the chunks' shared flag word (and the dump bytes behind it)
    if (trunc) {                                                 // (rare) the reference truncates a read of this block: whole, from its exact phase
        O.fl = jda_decode_block_win<64, true, true>(pos, off, wbase, TB, coef, in.pred, true, true);
        return O;
    }
    jda_u64_alias *z = (jda_u64_alias *)coef;
    z[0] = (uint64_t)(uint16_t)in.pred;
#pragma unroll
    for (int i = 1; i < 16; i++) z[i] = 0;
    O.whole = 0;
    O.bits = pos * 8u + off;
    O.fl = jda_decode_chunk_win(O.bits, wbase, TB, coef, 1u, JDA_CONT_SYMS);
    return O;
}
// a pass B item: entry = the continuation entry (valid: this lane has one), owner_bits = the owning lane's jda_p1c_own::bits
template <int MODE>
JDA_HD void jda_p1c_item(const jda_dev_desc &D, const jda_tile_ctx &C, uint32_t entry, uint32_t blk_lane, uint32_t owner_bits, bool valid,
                         const uint8_t *tab, uint8_t *wl, const uint8_t *win)
{
    typedef jda_lds_layout<MODE> L;
    if (!valid || (owner_bits & JDA_P1C_SKIP)) return;
    jda_tables TB;
    jda_p1c_tables<MODE>(TB, D, blk_lane, tab);
    uint8_t *slot = wl + L::COEF_OFF + blk_lane * JDA_COEF_STRIDE;
    const uint32_t fl = jda_decode_chunk_win(owner_bits + JDA_CONT_REL(entry), win - C.win_lo, TB, (int16_t *)slot, JDA_CONT_K(entry), JDA_CONT_SYMS);
    jda_lds_or_u32(slot + JDA_SLOT_FLAGS, fl);
}
// finish: the block's flags for the IDCT work lists (what jda_p1_entropy returns)
template <int MODE>
JDA_HD uint32_t jda_p1c_finish(const jda_p1c_own &O, uint32_t lb, const uint8_t *wl)
{
    typedef jda_lds_layout<MODE> L;
    if (!O.listed) return JDA_NO_LIST;
    if (O.whole) return O.fl;
    return jda_p1c_fold(O.fl | *(const jda_u32_alias *)(wl + L::COEF_OFF + lb * JDA_COEF_STRIDE + JDA_SLOT_FLAGS));
}

// The work lists of the IDCT stages, built by the whole wavefront at once (every lane calls this, with
// its jda_p1_entropy result): the non-empty columns of every block -> two column lists (rows 4-7 empty
// or not, jpeg.inl:2561), every block -> one of the three row-variant lists (:2686-2688) or the DC-only
// list (:5146-5154).  Positions come from a wave prefix sum / ballots; order within a list is irrelevant.
// all_flags: host emulation only (the flags of all 64 lanes).
template <int MODE>
JDA_HD void jda_p1_lists(const jda_dev_desc &D, const jda_lane_pre &LP, uint32_t lane, uint32_t flags, const uint32_t *all_flags, const uint8_t *tab, uint8_t *wl)
{
    typedef jda_lds_layout<MODE> L;
    (void)D;
    uint32_t *cnt = (uint32_t *)(wl + L::CNT_OFF);
    uint8_t *rowlist = wl + L::ROWLIST_OFF;
    uint16_t *collist = (uint16_t *)(wl + L::COLLIST_OFF);
    const bool listed = flags != JDA_NO_LIST;
    const bool has_ac = listed && flags != 0;
    // columns that hold data (column 0 always, :2555); rows 4-7 empty selects the short column stage
    const uint32_t colmask = has_ac ? ((flags & 0xffu) | 1u) : 0u;
    const uint32_t ncols = jda_popcount8(colmask);
    const bool half = (flags & 0x2000u) == 0;
    // one scan for both lists: short-stage columns in the low half of the word, full-stage in the high half
    const uint32_t mine = half ? ncols : (ncols << 16);
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t *all_mine = nullptr, *all_cls = nullptr;
#else
    uint32_t all_mine[JDA_TILE_THREADS], all_cls[JDA_TILE_THREADS];
    for (uint32_t l = 0; l < JDA_TILE_THREADS; l++) {
        const uint32_t f = all_flags[l];
        const bool ac = f != JDA_NO_LIST && f != 0;
        const uint32_t n = ac ? jda_popcount8((f & 0xffu) | 1u) : 0u;
        all_mine[l] = (f & 0x2000u) == 0 ? n : (n << 16);
        all_cls[l] = f == JDA_NO_LIST ? 4u : (f == 0 ? 3u : ((f & 0xf0u) ? 2u : ((f & 0xfcu) ? 1u : 0u)));
    }
#endif
    uint32_t total;
    const uint32_t below = jda_wave_excl_sum(mine, lane, all_mine, total);
    // One array: the short-stage items, then the full-stage items.  A block's columns, lowest first, come out of a
    // 16-entry table as 3-bit fields (low nibble, then high nibble + 4), and the block stores EIGHT items from its
    // place on, whatever it has: what it stores past its own items lands on the places of blocks after it -- stored
    // by a later instruction (the eight stores run from the last item to the first, and a later block's item at the
    // same place has a smaller ordinal) -- or past the end of the list (unused entries, then at most 14 bytes of the
    // row list, which is written below).  No condition per column.  A block without columns stores at the end.
    const uint32_t n_half = total & 0xffffu, n_all = n_half + (total >> 16);
    uint32_t base = half ? (below & 0xffffu) : n_half + (below >> 16);
    if (ncols == 0) base = n_all;
    const uint16_t *nib = (const uint16_t *)(tab + JDA_LT_NIB);
    const uint32_t lo = colmask & 15u, hi = colmask >> 4;
    const uint32_t plist = ((uint32_t)nib[lo] | (((uint32_t)nib[hi] + 0x924u) << (3u * jda_popcount8(lo)))) << 1;      // (<< 1: a column rides in an item as its byte offset)
    uint16_t *dst = collist + base;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
#if !defined(__HIP_DEVICE_COMPILE__)
        if ((uint32_t)k >= ncols) continue;          // (the emulator steps the lanes one after another: no overrun there)
#endif
        dst[k] = (uint16_t)(LP.item_pre | ((plist >> (3 * k)) & 0xeu));
        JDA_STORE_ORDER();                           // the ORDER of the eight stores is what makes the overruns harmless
    }
    const uint32_t cls = !listed ? 4u : (flags == 0 ? 3u : ((flags & 0xf0u) ? 2u : ((flags & 0xfcu) ? 1u : 0u)));
    uint32_t n0, n1, n2, n3;
    const uint32_t r0 = jda_wave_class_rank(cls, 0, lane, all_cls, n0);
    const uint32_t r1 = jda_wave_class_rank(cls, 1, lane, all_cls, n1);
    const uint32_t r2 = jda_wave_class_rank(cls, 2, lane, all_cls, n2);
    const uint32_t r3 = jda_wave_class_rank(cls, 3, lane, all_cls, n3);
    const uint32_t rank = cls == 0 ? r0 : (cls == 1 ? r1 : (cls == 2 ? r2 : r3));
    // one array, classes back to back: 0 | 1 | 2 | DC-only
    const uint32_t cbase = cls == 0 ? 0u : (cls == 1 ? n0 : (cls == 2 ? n0 + n1 : n0 + n1 + n2));
    uint8_t *rdst = listed ? rowlist + cbase + rank : (uint8_t *)&cnt[7];
    *rdst = (uint8_t)lane;
    if (lane == 0) {
        cnt[0] = n_half; cnt[1] = total >> 16;
        // The row variant for columns 0-3 gives what the general variant gives on rows whose columns 4-7 are zero (jpeg.inl:2698-2743:
        // 362 - 256 = 106, and z10 = -z13, z12 = z11 make the odd parts the same products) -- so when the blocks of class 1 that do
        // not fill a pass (eight rows each, eight blocks a pass) fit into the idle lanes of class 2's last pass, they move over: the
        // list is class 0 | 1 | 2 | DC-only, the border between 1 and 2 shifts, and class 1 runs one pass less.  (The other
        // variants round differently: nothing else may move.)
        const uint32_t rem1 = n1 & 7u, slack2 = (8u - (n2 & 7u)) & 7u;
        const uint32_t k = (rem1 != 0u && rem1 <= slack2) ? rem1 : 0u;
        cnt[2] = n0; cnt[3] = n1 - k; cnt[4] = n2 + k; cnt[5] = n3;
    }
}

// ---- P2 ---------------------------------------------------------------------------------------
template <int MODE, bool FAST, bool HALF>
JDA_HD void jda_p2_column_item(const jda_dev_desc &D, uint32_t item, const uint8_t *tab, uint8_t *cbase)
{
    typedef jda_mode_traits<MODE> T;
    // item = (quantiser table's offset / 128) << 10 | block << 4 | column << 1: the column as the byte offset it is in both arrays
    // (six instructions from the item to the two addresses; eight with the column as a number)
    const uint32_t blk = (item >> 4) & 63u, col2 = item & 0xeu;
    (void)D; (void)sizeof(T);
    const int16_t *quant = (const int16_t *)(tab + (((item >> 3) & 0x3f80u) | col2));
    int16_t *coef = (int16_t *)(cbase + col2 + blk * JDA_COEF_STRIDE);
    int32_t cv[8], qv[8], r[8];
#pragma unroll
    for (int row = 0; row < 8; row++) {
        if (HALF && row >= 4) { cv[row] = 0; qv[row] = 0; }
        else { cv[row] = coef[row * 8]; qv[row] = quant[row * 8]; }
    }
    jda_idct_col<FAST, HALF>(cv, qv, r);
#pragma unroll
    for (int row = 0; row < 8; row++) coef[row * 8] = (int16_t)r[row];
}

template <int MODE, bool FAST>
JDA_HD void jda_p2_columns(const jda_dev_desc &D, uint32_t t, const uint8_t *tab, uint8_t *wl)
{
    typedef jda_lds_layout<MODE> L;
    const uint32_t *cnt = (const uint32_t *)(wl + L::CNT_OFF);
    const uint16_t *collist = (const uint16_t *)(wl + L::COLLIST_OFF);
    const uint32_t n_half = cnt[0], n_full = cnt[1];
    uint8_t *const cbase = wl + L::COEF_OFF;
    // (one number walks the list and ends the loop)
    const uint16_t *lp = collist + t;
    for (const uint16_t *const lend = collist + n_half; lp < lend; lp += JDA_TILE_THREADS) jda_p2_column_item<MODE, FAST, true>(D, *lp, tab, cbase);
    lp = collist + n_half + t;
    for (const uint16_t *const lend = collist + n_half + n_full; lp < lend; lp += JDA_TILE_THREADS) jda_p2_column_item<MODE, FAST, false>(D, *lp, tab, cbase);
}

// ---- P3 ---------------------------------------------------------------------------------------
template <int MODE, int RC>
JDA_HD void jda_p3_row_class(uint32_t t, uint8_t *wl, uint32_t first, uint32_t n_blocks)
{
    typedef jda_lds_layout<MODE> L;
    // item i = t + 64 pass is row i & 7 = t & 7 of block list[i >> 3] = list[(t >> 3) + 8 pass]: the row and everything that
    // depends on it alone are the lane's for the whole tile loop, and ONE number walks the list and ends the loop (the loop used to
    // carry i, shift it for the list and add the row's offset to the block's address: seven instructions a pass, four now)
    const uint32_t row = t & 7u;
    const uint8_t *lp = wl + L::ROWLIST_OFF + first + (t >> 3);
    const uint8_t *const lend = wl + L::ROWLIST_OFF + first + n_blocks;
#if defined(__HIP_DEVICE_COMPILE__)
    // (one register the compiler cannot see through: it would keep the constant part of the address apart for the store's offset
    // field and add it back in front of every two-dword read, whose offset fields are too narrow for it)
    uint32_t rb32 = JDA_LDS_A32(wl + L::COEF_OFF + row * 16);
    JDA_OPAQUE(rb32);
    uint8_t *const rowbase = (uint8_t *)(uint8_t __attribute__((address_space(3))) *)rb32;
#else
    uint8_t *const rowbase = wl + L::COEF_OFF + row * 16;
#endif
    for (; lp < lend; lp += JDA_TILE_THREADS / 8) {
        const uint32_t blk = *lp;
        uint8_t *const rp = rowbase + blk * JDA_COEF_STRIDE;
        const jda_u64_alias *src = (const jda_u64_alias *)rp;
        int32_t sv[8];
        const uint64_t a = src[0];
        sv[0] = (int16_t)a; sv[1] = (int16_t)(a >> 16); sv[2] = (int16_t)(a >> 32); sv[3] = (int16_t)(a >> 48);
        if (RC == 2) {
            const uint64_t bq = src[1];
            sv[4] = (int16_t)bq; sv[5] = (int16_t)(bq >> 16); sv[6] = (int16_t)(bq >> 32); sv[7] = (int16_t)(bq >> 48);
        } else { sv[4] = sv[5] = sv[6] = sv[7] = 0; }
        const jda_row8 p = jda_idct_row<RC>(sv);
        // in place (jpeg.inl:2682): row r's 8 bytes land on bytes [8r, 8r+8) of the block, i.e. on row
        // r/2's int16 data -- safe because the 8 rows of a block are handled by 8 adjacent lanes of one
        // wavefront in the same instruction (all reads precede all writes), and on the sequential host
        // emulator rows are visited in ascending order
        jda_u32_alias *dst = (jda_u32_alias *)(rp - row * 8);
        dst[0] = p.lo; dst[1] = p.hi;
    }
}

template <int MODE>
JDA_HD void jda_p3_rows(const jda_dev_desc &D, uint32_t t, const uint8_t *tab, uint8_t *wl)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    const uint32_t *cnt = (const uint32_t *)(wl + L::CNT_OFF);
    const uint32_t n0 = cnt[2], n1 = cnt[3], n2 = cnt[4];
    jda_p3_row_class<MODE, 0>(t, wl, 0, n0);
    jda_p3_row_class<MODE, 1>(t, wl, n0, n1);
    jda_p3_row_class<MODE, 2>(t, wl, n0 + n1, n2);
    // DC-only blocks: all 64 samples = RT((pred * q0) >> 5)  (:5146-5154); one thread per block (rare)
    const uint8_t *list = wl + L::ROWLIST_OFF + n0 + n1 + n2;
    const uint32_t n_dc = cnt[5];
    for (uint32_t i = t; i < n_dc; i += JDA_TILE_THREADS) {
        const uint32_t blk = list[i];
        const uint32_t b = blk % T::NBLK;
        const uint32_t c = b < (uint32_t)T::NLUMA ? 0u : b - T::NLUMA + 1u;
        const int32_t q0 = *(const int16_t *)(tab + JDA_LT_QUANT_OFF(jda_pick3(D.q_id, c)));
        const int32_t dc = *(const int16_t *)(wl + L::COEF_OFF + blk * JDA_COEF_STRIDE);
        const uint32_t v = jda_dup8(jda_range_limit5(dc * q0));
        jda_u32_alias *dst = (jda_u32_alias *)(wl + L::COEF_OFF + blk * JDA_COEF_STRIDE);
#pragma unroll
        for (int k = 0; k < 16; k++) dst[k] = v;
    }
}

// i / d without an integer division per work item: q = (i * ceil(2^22 / d)) >> 22, exact while
// i * d < 2^22 (here i < 16 * d and d <= 384, so i * d < 2.4M) and i * ceil(2^22 / d) < 2^32
JDA_HD uint32_t jda_recip22(uint32_t d) { return ((1u << 22) + d - 1u) / d; }


// ---- P4: colour conversion + coalesced stores ------------------------------------------------------
// four converted pixels -> memory in the requested format.  CLIP: the group may cross the right edge.
// nvalid: how many of the four belong to this tile (a tile's width need not be a multiple of 4, and
// its neighbour -- another wavefront -- owns the pixels right of it).
template <int PT, bool CLIP>
JDA_HD void jda_store4(uint8_t JDA_GLOBAL *row, uint32_t X, uint32_t out_w, const uint32_t v[4], uint32_t nvalid = 4)
{
    uint32_t n = (!CLIP || X + 4 <= out_w) ? 4u : out_w - X;
    if (CLIP && nvalid < n) n = nvalid;
    if (CLIP && (X & 3u)) {                              // tile starts off a 4-pixel boundary: element stores
        for (uint32_t j = 0; j < n; j++) {
            if (PT == JDA_RGB8888) ((jda_u32_alias JDA_GLOBAL *)(row + (size_t)X * 4))[j] = v[j];
            else if (PT == JDA_EIGHT_BIT_GRAYSCALE) row[X + j] = (uint8_t)v[j];
            else ((uint16_t JDA_GLOBAL *)(row + (size_t)X * 2))[j] = (uint16_t)v[j];
        }
        return;
    }
    if (PT == JDA_RGB8888) {
        jda_u32_alias JDA_GLOBAL *d = (jda_u32_alias JDA_GLOBAL *)(row + (size_t)X * 4);
        if (n == 4) { d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3]; }
        else for (uint32_t j = 0; j < n; j++) d[j] = v[j];
    } else if (PT == JDA_EIGHT_BIT_GRAYSCALE) {
        if (n == 4) *(jda_u32_alias JDA_GLOBAL *)(row + X) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        else for (uint32_t j = 0; j < n; j++) row[X + j] = (uint8_t)v[j];
    } else {
        if (n == 4) { jda_u32_alias JDA_GLOBAL *d = (jda_u32_alias JDA_GLOBAL *)(row + (size_t)X * 2); d[0] = v[0] | (v[1] << 16); d[1] = v[2] | (v[3] << 16); }
        else for (uint32_t j = 0; j < n; j++) ((uint16_t JDA_GLOBAL *)(row + (size_t)X * 2))[j] = (uint16_t)v[j];
    }
}

// runtime pixel type -> the templated store (used by the generic path only)
template <bool CLIP>
JDA_HD void jda_store4_rt(uint8_t JDA_GLOBAL *row, uint32_t X, uint32_t out_w, int pt, const uint32_t v[4], uint32_t nvalid)
{
    if (pt == JDA_RGB8888) jda_store4<JDA_RGB8888, CLIP>(row, X, out_w, v, nvalid);
    else if (pt == JDA_EIGHT_BIT_GRAYSCALE) jda_store4<JDA_EIGHT_BIT_GRAYSCALE, CLIP>(row, X, out_w, v, nvalid);
    else jda_store4<JDA_RGB565_LITTLE_ENDIAN, CLIP>(row, X, out_w, v, nvalid);
}

// one chroma sample shared by a 2x2 (or 1x1) group: the products of jpeg.inl:3158-3161, already
// shifted: ((k*c) + (Y << 12)) >> 12 == Y + ((k*c) >> 12) exactly, because Y << 12 is a multiple of 4096
struct jda_chroma { int32_t r, g, b; };
JDA_HD jda_chroma jda_chroma_terms(uint32_t cb8, uint32_t cr8)
{
    // k * (c - 128) == k * c - 128 k : the level shift folds into the multiply-add's constant
    const int32_t cb = (int32_t)cb8, cr = (int32_t)cr8;
    jda_chroma t;
    t.r = (5742 * cr - 5742 * 128) >> 12;
    t.g = (-1409 * cb - 2925 * cr + (1409 + 2925) * 128) >> 12;
    t.b = (7258 * cb - 7258 * 128) >> 12;
    return t;
}
// The same three terms, each duplicated into both 16-bit halves of a word (the operand of the packed
// pixel-pair adds).  x >> 12 == (16 x) >> 16, and the upper half of a word is picked by the byte
// permute that duplicates it: multiply-add + permute per term, no shift.
struct jda_chroma2 { uint32_t r, g, b; };
// un-shifted terms (16 x the products); the wanted value sits in bits 31:16
JDA_HD jda_chroma2 jda_chroma_terms16(uint32_t cb8, uint32_t cr8)
{
    const int32_t cb = (int32_t)cb8, cr = (int32_t)cr8;
    jda_chroma2 t;                                                // (four multiply-adds: left to itself the compiler makes the green term two multiplies and a three-operand add)
    t.r = (uint32_t)jda_mad24(cr, 16 * 5742, -16 * 5742 * 128);
    int32_t g = jda_mad24(cr, -16 * 2925, 16 * (1409 + 2925) * 128);
    JDA_OPAQUE(g);                                                // (.. as it does when it sees both products at once)
    t.g = (uint32_t)jda_mad24(cb, -16 * 1409, g);
    t.b = (uint32_t)jda_mad24(cb, 16 * 7258, -16 * 7258 * 128);
    return t;
}
JDA_HD uint32_t jda_pack_hi16(uint32_t lo, uint32_t hi) { return jda_perm(hi, lo, 0x07060302u); }   // {hi[31:16], lo[31:16]}
// Two horizontally adjacent RGB8888 pixels, red and green of a pixel side by side in a word.  ypair = Y0 | Y1 << 16; trg0 / trg1 = pixel
// 0's / 1's red term in bits 15:0 and green term in bits 31:16 (the same word for both when the pixels share their chroma sample);
// tb: the blue terms where the caller has them -- BHI: one term in bits 31:16 for both pixels, else pixel 0's in 15:0, pixel 1's in 31:16.
// A pixel costs four instructions (add + saturate for R|G, half an add + saturate for B, one permute that also sets alpha) where
// three channel pairs cost four and a half.
template <bool BHI>
JDA_HD void jda_rgba_pair_rg(uint32_t ypair, uint32_t trg0, uint32_t trg1, uint32_t tb, uint32_t &px0, uint32_t &px1)
{
    const uint32_t rg0 = jda_sat_pk_u8(jda_pk_add16_alo(ypair, trg0));                          // [R0, G0, 0, 0]
    const uint32_t rg1 = jda_sat_pk_u8(jda_pk_add16_ahi(ypair, trg1));                          // [R1, G1, 0, 0]
    const uint32_t b2 = jda_sat_pk_u8(BHI ? jda_pk_add16_bhi(ypair, tb) : jda_pk_add16(ypair, tb));   // [B0, B1, 0, 0]
    px0 = jda_perm(b2, rg0, 0x0d040100u);                                                      // [R0, G0, B0, 0xff]
    px1 = jda_perm(b2, rg1, 0x0d050100u);                                                      // [R1, G1, B1, 0xff]
}
template <int PT>
JDA_HD uint32_t jda_rgb_pixel(uint32_t y8, const jda_chroma &t)
{
    const int32_t y = (int32_t)y8;
    if (PT == JDA_RGB8888) {
        const int32_t r = jda_clamp255(t.r + y);
        int32_t g = jda_clamp255(t.g + y);
        const int32_t b = jda_clamp255(t.b + y);
        JDA_OPAQUE(g);
        return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | 0xff000000u;
    }
    // RGB565 goes through the 10-bit wrapping tables
    const int32_t r = jda_clamp255(jda_sext10_at(t.r + y, 0));
    const int32_t g = jda_clamp255(jda_sext10_at(t.g + y, 0));
    const int32_t b = jda_clamp255(jda_sext10_at(t.b + y, 0));
    uint32_t v = (uint32_t)((r >> 3) << 11) | (uint32_t)((g >> 2) << 5) | (uint32_t)(b >> 3);
    if (PT == JDA_RGB565_BIG_ENDIAN) v = ((v & 0xffu) << 8) | (v >> 8);
    return v;
}

// per 16-bit lane: clamp a signed value to 0..255 (v_pk_max_i16, v_pk_min_i16)
JDA_HD uint32_t jda_pk_clamp255(uint32_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short jda_s2 __attribute__((ext_vector_type(2)));
    jda_s2 v = __builtin_bit_cast(jda_s2, a);
    const jda_s2 lo = { 0, 0 }, hi = { 255, 255 };
    v = __builtin_elementwise_min(__builtin_elementwise_max(v, lo), hi);
    return __builtin_bit_cast(uint32_t, v);
#else
    int32_t l = (int16_t)(a & 0xffffu), h = (int16_t)(a >> 16);
    l = l < 0 ? 0 : (l > 255 ? 255 : l); h = h < 0 ? 0 : (h > 255 ? 255 : h);
    return (uint32_t)l | ((uint32_t)h << 16);
#endif
}
// Two horizontally adjacent RGB565 pixels at once (JPEGPixelLE / BE, jpeg.inl:3101-3156): pixel 0 in bits 15:0,
// pixel 1 in bits 31:16.  The reference indexes 10-bit-wrapping tables with (Y + term) & 0x3ff; for 8-bit
// samples Y + term stays inside -227..480, where the wrap is the identity, so the tables reduce to a clamp
// and the field extraction (r >> 3) << 11 | (g >> 2) << 5 | b >> 3 works on both 16-bit lanes of a word.
template <int PT>
JDA_HD uint32_t jda_565_pair(uint32_t ypair, uint32_t tr, uint32_t tg, uint32_t tb)
{
    const uint32_t r2 = jda_pk_clamp255(jda_pk_add16(ypair, tr));
    const uint32_t g2 = jda_pk_clamp255(jda_pk_add16(ypair, tg));
    const uint32_t b2 = jda_pk_clamp255(jda_pk_add16(ypair, tb));
    uint32_t v = ((r2 & 0x00f800f8u) << 8) | ((g2 & 0x00fc00fcu) << 3) | ((b2 >> 3) & 0x001f001fu);
    if (PT == JDA_RGB565_BIG_ENDIAN) v = jda_perm(0, v, 0x02030001u);      // swap the bytes of each pixel (:3149)
    return v;
}

template <int PT>
JDA_HD uint32_t jda_565_pair_t16(uint32_t ypair, const jda_chroma2 &t)
{
    const uint32_t r2 = jda_pk_clamp255(jda_pk_add16_bhi(ypair, t.r));
    const uint32_t g2 = jda_pk_clamp255(jda_pk_add16_bhi(ypair, t.g));
    const uint32_t b2 = jda_pk_clamp255(jda_pk_add16_bhi(ypair, t.b));
    uint32_t v = ((r2 & 0x00f800f8u) << 8) | ((g2 & 0x00fc00fcu) << 3) | ((b2 >> 3) & 0x001f001fu);
    if (PT == JDA_RGB565_BIG_ENDIAN) v = jda_perm(0, v, 0x02030001u);
    return v;
}

// Addresses of the colour stage's work items for a FULL 4:2:0 tile (10 MCUs = 160 x 16 pixels = 320 items of 4x2
// pixels = exactly five passes of the wavefront): item i = lane + 64 * pass always lands on the same LDS offsets and
// on the same offset from the tile's first output pixel, so the index arithmetic (a third of the stage's VALU work)
// is done once per image and kept in registers.  Only the output offset depends on the image (pitch, pixel size).
// The same for a FULL 4:4:4 tile (20 MCUs = 160 x 8 pixels = 320 items of 4 pixels of one row = five passes):
// yo = the luma bytes (Cb, Cr one and two block slots further), rel as above; co is not used.
#define JDA_P4_PASSES 5
#define JDA_P4_PASSES_444 5
struct jda_p4_pre { uint32_t yo[JDA_P4_PASSES_444], co[JDA_P4_PASSES], rel[JDA_P4_PASSES_444]; };
JDA_HD void jda_p4_precompute(jda_p4_pre &P, uint32_t t, uint32_t plane_stride, uint32_t pitch, uint32_t bpp)
{
#pragma unroll
    for (int it = 0; it < JDA_P4_PASSES; it++) {
        const uint32_t i = t + 64u * (uint32_t)it, rp = i / 40u, g = i - rp * 40u;
        const uint32_t po = (g >> 2) * plane_stride;
        P.yo[it] = po + (rp >> 2) * (2 * JDA_COEF_STRIDE) + (rp & 3u) * 16 + ((g >> 1) & 1u) * JDA_COEF_STRIDE + (g & 1u) * 4;
        P.co[it] = po + 4 * JDA_COEF_STRIDE + rp * 8 + (g & 3u) * 2;
        P.rel[it] = rp * 2u * pitch + g * 4u * bpp;
    }
}

JDA_HD void jda_p4_precompute_444(jda_p4_pre &P, uint32_t t, uint32_t plane_stride, uint32_t pitch, uint32_t bpp)
{
#pragma unroll
    for (int it = 0; it < JDA_P4_PASSES_444; it++) {
        const uint32_t i = t + 64u * (uint32_t)it, r = i / 40u, x4 = (i - r * 40u) * 4u;    // 40 groups of 4 pixels per row
        P.yo[it] = (x4 >> 3) * plane_stride + r * 8u + (x4 & 7u);
        P.rel[it] = r * pitch + x4 * bpp;
    }
#pragma unroll
    for (int it = 0; it < JDA_P4_PASSES; it++) P.co[it] = 0;
}

// full-size 4:2:0 colour output (JPEGPutMCU22 scalar body, jpeg.inl:4333-4543): a work item is a 4x2
// pixel group (the two rows share their chroma samples); items are dealt to the threads in row-major
// order so that consecutive threads store consecutive 16-byte groups.
// the eight pixels of one item: ya / yb = four luma samples of the upper / lower row, cb2 / cr2 = two chroma samples each
template <int PT>
JDA_HD void jda_p4_420_item(uint32_t ya, uint32_t yb, uint32_t cb0, uint32_t cb1, uint32_t cr0, uint32_t cr1, uint32_t v0[4], uint32_t v1[4])
{
    // (a chroma sample's three terms serve the two pixels of a pair in both rows: they stay in the upper halves of their words, the
    // packed adds pick them up there; the four chroma samples come as bytes of their own -- ds_read_u8 -- so nothing is spent on
    // taking a 16-bit load apart)
    const jda_chroma2 d0 = jda_chroma_terms16(cb0, cr0);
    const jda_chroma2 d1 = jda_chroma_terms16(cb1, cr1);
    if (PT == JDA_RGB8888) {
        const uint32_t rg0 = jda_pack_hi16(d0.r, d0.g), rg1 = jda_pack_hi16(d1.r, d1.g);
        jda_rgba_pair_rg<true>(jda_perm(0, ya, 0x0c010c00u), rg0, rg0, d0.b, v0[0], v0[1]);
        jda_rgba_pair_rg<true>(jda_perm(0, ya, 0x0c030c02u), rg1, rg1, d1.b, v0[2], v0[3]);
        jda_rgba_pair_rg<true>(jda_perm(0, yb, 0x0c010c00u), rg0, rg0, d0.b, v1[0], v1[1]);
        jda_rgba_pair_rg<true>(jda_perm(0, yb, 0x0c030c02u), rg1, rg1, d1.b, v1[2], v1[3]);
    } else {                                                  // RGB565: v[0], v[1] hold pixel pairs
        v0[0] = jda_565_pair_t16<PT>(jda_perm(0, ya, 0x0c010c00u), d0);
        v0[1] = jda_565_pair_t16<PT>(jda_perm(0, ya, 0x0c030c02u), d1);
        v1[0] = jda_565_pair_t16<PT>(jda_perm(0, yb, 0x0c010c00u), d0);
        v1[1] = jda_565_pair_t16<PT>(jda_perm(0, yb, 0x0c030c02u), d1);
        v0[2] = v0[3] = v1[2] = v1[3] = 0;
    }
}
// item -> memory, whole groups: 16 (RGB8888) or 8 (RGB565) bytes per row
template <int PT>
JDA_HD void jda_p4_420_store(uint8_t JDA_GLOBAL *out, uint32_t off, uint32_t off1, const uint32_t v0[4], const uint32_t v1[4])
{
    if (PT == JDA_RGB8888) {
        jda_chunk16_alias q0, q1;
        q0.w[0] = v0[0]; q0.w[1] = v0[1]; q0.w[2] = v0[2]; q0.w[3] = v0[3];
        q1.w[0] = v1[0]; q1.w[1] = v1[1]; q1.w[2] = v1[2]; q1.w[3] = v1[3];
        *(jda_chunk16_alias JDA_GLOBAL *)(out + off) = q0;
        *(jda_chunk16_alias JDA_GLOBAL *)(out + off1) = q1;
    } else {
        *(jda_u64_alias JDA_GLOBAL *)(out + off) = (uint64_t)v0[0] | ((uint64_t)v0[1] << 32);
        *(jda_u64_alias JDA_GLOBAL *)(out + off1) = (uint64_t)v1[0] | ((uint64_t)v1[1] << 32);
    }
}

// a full, unclipped tile: five passes with the precomputed item addresses
template <int PT>
JDA_HD void jda_p4_420_full10(const jda_dev_desc &D, const jda_p4_pre &P, const uint8_t *plane_base, uint32_t x_base, uint32_t y_base)
{
    const uint32_t bpp = PT == JDA_RGB8888 ? 4u : 2u;
    const uint32_t pitch = D.out_pitch;
    uint8_t JDA_GLOBAL *tile = JDA_G(uint8_t, D.out) + (y_base * pitch + x_base * bpp);      // uniform
#pragma unroll
    for (int it = 0; it < JDA_P4_PASSES; it++) {
        const uint32_t ya = *(const jda_u32_alias *)(plane_base + P.yo[it]), yb = *(const jda_u32_alias *)(plane_base + P.yo[it] + 8);
        const uint8_t *cp = plane_base + P.co[it];
        uint32_t v0[4], v1[4];
        uint32_t cb0, cr0, cb1, cr1;
        jda_lds_bytes_apart(cp, 0, JDA_COEF_STRIDE, cb0, cr0);
        jda_lds_bytes_apart(cp, 1, JDA_COEF_STRIDE, cb1, cr1);
        jda_p4_420_item<PT>(ya, yb, cb0, cb1, cr0, cr1, v0, v1);
        jda_p4_420_store<PT>(tile, P.rel[it], P.rel[it] + pitch, v0, v1);
    }
}

template <int PT, bool CLIP>
JDA_HD void jda_p4_420_full(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                            uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    const uint32_t groups = tile_w >> 2;                          // 4-pixel groups per row (tile_w is a multiple of 16)
    const uint32_t inv = jda_recip22(groups);
    uint8_t JDA_GLOBAL *out = JDA_G(uint8_t, D.out);
    const uint32_t pitch = D.out_pitch;
    // byte offset of the tile's first pixel: 32-bit arithmetic from here on (surfaces are < 4 GiB, checked
    // by jda_batch_create), so an address is the uniform base + one 32-bit lane offset
    const uint32_t bpp = PT == JDA_RGB8888 ? 4u : 2u;
    const uint32_t tile_off = y_base * pitch + x_base * bpp;
    for (uint32_t i = t; i < groups * 8; i += JDA_TILE_THREADS) {
        const uint32_t rp = jda_umul24(i, inv) >> 22, g = i - jda_umul24(rp, groups);   // row pair, 4-pixel group in the row
        const uint32_t x4 = g * 4;
        const uint32_t Y0 = y_base + 2 * rp, X = x_base + x4;
        if (CLIP && (Y0 >= D.out_rows || X >= D.out_w)) continue;
        // LDS byte offsets within the tile's planes: MCU g>>2; luma block (rp>>2)*2 + ((g>>1)&1), row 2rp&7,
        // column (g&1)*4; chroma row rp, column (g&3)*2
        const uint32_t po = jda_umul24(g >> 2, plane_stride);
        const uint32_t yo = po + (rp >> 2) * (2 * JDA_COEF_STRIDE) + (rp & 3u) * 16 + ((g >> 1) & 1u) * JDA_COEF_STRIDE + (g & 1u) * 4;
        const uint32_t co = po + 4 * JDA_COEF_STRIDE + rp * 8 + (g & 3u) * 2;
        const uint32_t ya = *(const jda_u32_alias *)(plane_base + yo), yb = *(const jda_u32_alias *)(plane_base + yo + 8);
        const uint8_t *cp = plane_base + co;
        uint32_t v0[4], v1[4];
        uint32_t cb0, cr0, cb1, cr1;
        jda_lds_bytes_apart(cp, 0, JDA_COEF_STRIDE, cb0, cr0);
        jda_lds_bytes_apart(cp, 1, JDA_COEF_STRIDE, cb1, cr1);
        jda_p4_420_item<PT>(ya, yb, cb0, cb1, cr0, cr1, v0, v1);
        if (!CLIP) {                                              // whole groups, 16 / 8 bytes per row
            const uint32_t off = tile_off + jda_umul24(rp, 2 * pitch) + x4 * bpp;
            jda_p4_420_store<PT>(out, off, off + pitch, v0, v1);
        } else {
            if (PT != JDA_RGB8888) {                              // pixel pairs -> single pixels for the clipped stores
                const uint32_t a01 = v0[0], a23 = v0[1], b01 = v1[0], b23 = v1[1];
                v0[0] = a01 & 0xffffu; v0[1] = a01 >> 16; v0[2] = a23 & 0xffffu; v0[3] = a23 >> 16;
                v1[0] = b01 & 0xffffu; v1[1] = b01 >> 16; v1[2] = b23 & 0xffffu; v1[3] = b23 >> 16;
            }
            uint8_t JDA_GLOBAL *row0 = out + (size_t)Y0 * pitch;
            jda_store4<PT, CLIP>(row0, X, D.out_w, v0);
            if (Y0 + 1 < D.out_rows) jda_store4<PT, CLIP>(row0 + pitch, X, D.out_w, v1);
        }
    }
}

// full-size 4:4:4 colour output (JPEGPutMCU11 scalar body, jpeg.inl:3519-3559)
template <int PT, bool CLIP>
JDA_HD void jda_p4_444_full(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                            uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    const uint32_t groups = tile_w >> 2;
    const uint32_t inv = jda_recip22(groups);
    uint8_t JDA_GLOBAL *out = JDA_G(uint8_t, D.out);
    for (uint32_t i = t; i < groups * 8; i += JDA_TILE_THREADS) {
        const uint32_t r = (i * inv) >> 22, x4 = (i - r * groups) * 4;
        const uint32_t Y = y_base + r, X = x_base + x4;
        if (CLIP && (Y >= D.out_rows || X >= D.out_w)) continue;
        const uint8_t *P = plane_base + (x4 >> 3) * plane_stride + r * 8 + (x4 & 7u);
        const uint32_t y = *(const jda_u32_alias *)P, cb = *(const jda_u32_alias *)(P + JDA_COEF_STRIDE), cr = *(const jda_u32_alias *)(P + 2 * JDA_COEF_STRIDE);
        uint32_t v[4];
        if (PT == JDA_RGB8888) {
            jda_chroma2 c[4];
#pragma unroll
            for (int j = 0; j < 4; j++) c[j] = jda_chroma_terms16((cb >> (8 * j)) & 255u, (cr >> (8 * j)) & 255u);
            jda_rgba_pair_rg<false>(jda_perm(0, y, 0x0c010c00u), jda_pack_hi16(c[0].r, c[0].g), jda_pack_hi16(c[1].r, c[1].g), jda_pack_hi16(c[0].b, c[1].b), v[0], v[1]);
            jda_rgba_pair_rg<false>(jda_perm(0, y, 0x0c030c02u), jda_pack_hi16(c[2].r, c[2].g), jda_pack_hi16(c[3].r, c[3].g), jda_pack_hi16(c[2].b, c[3].b), v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                v[j] = jda_rgb_pixel<PT>((y >> (8 * j)) & 255u, jda_chroma_terms((cb >> (8 * j)) & 255u, (cr >> (8 * j)) & 255u));
        }
        jda_store4<PT, CLIP>(out + (size_t)Y * D.out_pitch, X, D.out_w, v);
    }
}

// a full, unclipped 4:4:4 tile: five passes with the precomputed item addresses
template <int PT>
JDA_HD void jda_p4_444_full21(const jda_dev_desc &D, const jda_p4_pre &P, uint32_t t, const uint8_t *plane_base, uint32_t x_base, uint32_t y_base)
{
    const uint32_t bpp = PT == JDA_RGB8888 ? 4u : 2u;
    uint8_t JDA_GLOBAL *tile = JDA_G(uint8_t, D.out) + (y_base * D.out_pitch + x_base * bpp);      // uniform
#pragma unroll
    for (int it = 0; it < JDA_P4_PASSES_444; it++) {
        const uint8_t *Pp = plane_base + P.yo[it];
        const uint32_t y = *(const jda_u32_alias *)Pp, cb = *(const jda_u32_alias *)(Pp + JDA_COEF_STRIDE), cr = *(const jda_u32_alias *)(Pp + 2 * JDA_COEF_STRIDE);
        uint32_t v[4];
        if (PT == JDA_RGB8888) {
            jda_chroma2 c[4];
#pragma unroll
            for (int j = 0; j < 4; j++) c[j] = jda_chroma_terms16((cb >> (8 * j)) & 255u, (cr >> (8 * j)) & 255u);
            jda_rgba_pair_rg<false>(jda_perm(0, y, 0x0c010c00u), jda_pack_hi16(c[0].r, c[0].g), jda_pack_hi16(c[1].r, c[1].g), jda_pack_hi16(c[0].b, c[1].b), v[0], v[1]);
            jda_rgba_pair_rg<false>(jda_perm(0, y, 0x0c030c02u), jda_pack_hi16(c[2].r, c[2].g), jda_pack_hi16(c[3].r, c[3].g), jda_pack_hi16(c[2].b, c[3].b), v[2], v[3]);
            jda_chunk16_alias q;
            q.w[0] = v[0]; q.w[1] = v[1]; q.w[2] = v[2]; q.w[3] = v[3];
            *(jda_chunk16_alias JDA_GLOBAL *)(tile + P.rel[it]) = q;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                v[j] = jda_rgb_pixel<PT>((y >> (8 * j)) & 255u, jda_chroma_terms((cb >> (8 * j)) & 255u, (cr >> (8 * j)) & 255u));
            *(jda_u64_alias JDA_GLOBAL *)(tile + P.rel[it]) = (uint64_t)(v[0] | (v[1] << 16)) | ((uint64_t)(v[2] | (v[3] << 16)) << 32);
        }
    }
}

// full-size 4:2:2 colour output (JPEGPutMCU21 full-size body, jpeg.inl:4839-4867): a work item is 4 pixels of one
// row; pixels 0-1 share one chroma sample, pixels 2-3 the next
template <int PT, bool CLIP>
JDA_HD void jda_p4_422_full(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                            uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    const uint32_t groups = tile_w >> 2;                          // tile_w is a multiple of 16
    const uint32_t inv = jda_recip22(groups);
    uint8_t JDA_GLOBAL *out = JDA_G(uint8_t, D.out);
    for (uint32_t i = t; i < groups * 8; i += JDA_TILE_THREADS) {
        const uint32_t r = jda_umul24(i, inv) >> 22, g = i - jda_umul24(r, groups);
        const uint32_t x4 = g * 4;
        const uint32_t Y = y_base + r, X = x_base + x4;
        if (CLIP && (Y >= D.out_rows || X >= D.out_w)) continue;
        // MCU g>>2, luma block (g>>1)&1, columns (g&1)*4..; chroma row r, columns ((g>>1)&1)*4 + (g&1)*2 ..
        const uint32_t po = jda_umul24(g >> 2, plane_stride);
        const uint32_t yo = po + ((g >> 1) & 1u) * JDA_COEF_STRIDE + r * 8 + (g & 1u) * 4;
        const uint32_t co = po + 2 * JDA_COEF_STRIDE + r * 8 + (g & 3u) * 2;
        const uint32_t y = *(const jda_u32_alias *)(plane_base + yo);
        const uint32_t cb2 = *(const uint16_t *)(plane_base + co), cr2 = *(const uint16_t *)(plane_base + co + JDA_COEF_STRIDE);
        uint32_t v[4];
        if (PT == JDA_RGB8888) {
            const uint8_t *cp = plane_base + co;
            uint32_t cb0, cr0, cb1, cr1;
            jda_lds_bytes_apart(cp, 0, JDA_COEF_STRIDE, cb0, cr0);
            jda_lds_bytes_apart(cp, 1, JDA_COEF_STRIDE, cb1, cr1);
            const jda_chroma2 d0 = jda_chroma_terms16(cb0, cr0);
            const jda_chroma2 d1 = jda_chroma_terms16(cb1, cr1);
            const uint32_t rg0 = jda_pack_hi16(d0.r, d0.g), rg1 = jda_pack_hi16(d1.r, d1.g);
            jda_rgba_pair_rg<true>(jda_perm(0, y, 0x0c010c00u), rg0, rg0, d0.b, v[0], v[1]);
            jda_rgba_pair_rg<true>(jda_perm(0, y, 0x0c030c02u), rg1, rg1, d1.b, v[2], v[3]);
        } else {
            const jda_chroma2 d0 = jda_chroma_terms16(cb2 & 255u, cr2 & 255u);
            const jda_chroma2 d1 = jda_chroma_terms16(cb2 >> 8, cr2 >> 8);
            const uint32_t a01 = jda_565_pair_t16<PT>(jda_perm(0, y, 0x0c010c00u), d0);
            const uint32_t a23 = jda_565_pair_t16<PT>(jda_perm(0, y, 0x0c030c02u), d1);
            v[0] = a01 & 0xffffu; v[1] = a01 >> 16; v[2] = a23 & 0xffffu; v[3] = a23 >> 16;
        }
        jda_store4<PT, CLIP>(out + (size_t)Y * D.out_pitch, X, D.out_w, v);
    }
}

// full-size 8-bit gray output of any source layout (JPEGPutMCU8BitGray full-size bodies, jpeg.inl:2828-2837,
// :2893-2902, :2943-2952, :3000-3034): the luma samples are the pixels.  A work item is one row of one luma block
// (8 bytes); items are dealt row-major so that consecutive lanes store consecutive 8-byte chunks.
template <int MODE, bool CLIP>
JDA_HD void jda_p4_gray8_full(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                              uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t nbx = (uint32_t)T::MCU_W / 8u;                 // luma blocks across an MCU: 1 or 2
    const uint32_t chunks = tile_w >> 3;                          // 8-pixel chunks per row of the tile
    const uint32_t inv = jda_recip22(chunks);
    uint8_t JDA_GLOBAL *out = JDA_G(uint8_t, D.out);
    const uint32_t pitch = D.out_pitch;
    const uint32_t tile_off = y_base * pitch + x_base;
    if (MODE == JDA_MODE_GRAY && !CLIP && chunks == JDA_TILE_THREADS) {      // a full tile of a gray file: pass = row, lane = block
        const jda_u32_alias *src = (const jda_u32_alias *)(plane_base + jda_umul24(t, plane_stride));
        uint8_t JDA_GLOBAL *dst = out + tile_off + t * 8u;
#pragma unroll
        for (uint32_t r = 0; r < 8; r++)
            *(jda_u64_alias JDA_GLOBAL *)(dst + jda_umul24(r, pitch)) = (uint64_t)src[2 * r] | ((uint64_t)src[2 * r + 1] << 32);
        return;
    }
    for (uint32_t i = t; i < chunks * (uint32_t)T::MCU_H; i += JDA_TILE_THREADS) {
        const uint32_t r = jda_umul24(i, inv) >> 22, c = i - jda_umul24(r, chunks);
        const uint32_t m = nbx == 2 ? (c >> 1) : c, bxq = nbx == 2 ? (c & 1u) : 0u;
        const uint32_t q = (r >> 3) * nbx + bxq;                  // luma block inside the MCU
        const jda_u32_alias *src = (const jda_u32_alias *)(plane_base + jda_umul24(m, plane_stride) + q * JDA_COEF_STRIDE + (r & 7u) * 8);
        const uint32_t lo = src[0], hi = src[1];
        const uint32_t X = x_base + c * 8, Y = y_base + r;
        if (!CLIP) {
            *(jda_u64_alias JDA_GLOBAL *)(out + tile_off + jda_umul24(r, pitch) + c * 8) = (uint64_t)lo | ((uint64_t)hi << 32);
        } else {
            if (Y >= D.out_rows || X >= D.out_w) continue;
            uint8_t JDA_GLOBAL *row = out + (size_t)Y * pitch;
            const uint32_t n = X + 8 <= D.out_w ? 8u : D.out_w - X;
            const uint64_t v = (uint64_t)lo | ((uint64_t)hi << 32);
            if (n == 8) *(jda_u64_alias JDA_GLOBAL *)(row + X) = v;
            else for (uint32_t j = 0; j < n; j++) row[X + j] = (uint8_t)(v >> (8 * j));
        }
    }
}

// half-size 8-bit gray output of any source layout (JPEGPutMCU8BitGray half-size bodies, jpeg.inl:2812-2827, :2857-2873,
// :2907-2923, :2979-2999): a pixel = (the 2x2 luma samples' sum + 2) >> 2.  A work item is one output row of one luma block:
// two source rows (16 bytes) -> 4 pixels, the sums two at a time in the halves of a word; items are dealt row-major so
// that consecutive lanes store consecutive dwords.
JDA_HD uint32_t jda_pair_sums(uint32_t v) { return (v & 0x00ff00ffu) + ((v >> 8) & 0x00ff00ffu); }       // [b0 + b1, b2 + b3] as 16-bit halves
// four output pixels of the half-size gray image from two source rows of eight samples (a0 a1 / b0 b1): (2x2 sum + 2) >> 2 each.
// A 2x2 sum is two byte dot products with ones in two places (the second accumulates onto the first, which starts at 2); the four
// sums are shifted two at a time and their bytes picked by one permute (13 instructions where masks and adds take 21).
JDA_HD uint32_t jda_half_gray4(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1)
{
    const uint32_t lo = 0x00000101u, hi = 0x01010000u;
    const uint32_t s0 = jda_udot4_acc(b0, lo, jda_udot4_acc(a0, lo, 2u)), s1 = jda_udot4_acc(b0, hi, jda_udot4_acc(a0, hi, 2u));
    const uint32_t s2 = jda_udot4_acc(b1, lo, jda_udot4_acc(a1, lo, 2u)), s3 = jda_udot4_acc(b1, hi, jda_udot4_acc(a1, hi, 2u));
    return jda_perm(((s3 << 16) | s2) >> 2, ((s1 << 16) | s0) >> 2, 0x06040200u);      // (sums <= 1022: the shifted halves are the bytes)
}
template <int MODE, bool CLIP>
JDA_HD void jda_p4_gray8_half(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                              uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t nbx = (uint32_t)T::MCU_W / 8u;                 // luma blocks across an MCU: 1 or 2
    const uint32_t chunks = tile_w >> 2;                          // 4-pixel chunks per output row of the tile (tile_w: output pixels)
    const uint32_t inv = jda_recip22(chunks);
    uint8_t JDA_GLOBAL *out = JDA_G(uint8_t, D.out);
    const uint32_t pitch = D.out_pitch;
    const uint32_t tile_off = y_base * pitch + x_base;
    if (MODE == JDA_MODE_GRAY && !CLIP && chunks == JDA_TILE_THREADS) {      // a full tile of a gray file: pass = output row, lane = block
        const jda_u32_alias *src = (const jda_u32_alias *)(plane_base + jda_umul24(t, plane_stride));
        uint8_t JDA_GLOBAL *dst = out + tile_off + t * 4u;
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            *(jda_u32_alias JDA_GLOBAL *)(dst + jda_umul24(r, pitch)) = jda_half_gray4(src[4 * r], src[4 * r + 1], src[4 * r + 2], src[4 * r + 3]);
        }
        return;
    }
    for (uint32_t i = t; i < chunks * ((uint32_t)T::MCU_H >> 1); i += JDA_TILE_THREADS) {
        const uint32_t r = jda_umul24(i, inv) >> 22, c = i - jda_umul24(r, chunks);
        const uint32_t m = nbx == 2 ? (c >> 1) : c, bxq = nbx == 2 ? (c & 1u) : 0u;
        const uint32_t q = (r >> 2) * nbx + bxq;                  // luma block inside the MCU
        const jda_u32_alias *src = (const jda_u32_alias *)(plane_base + jda_umul24(m, plane_stride) + q * JDA_COEF_STRIDE + (r & 3u) * 16);
        const uint32_t v = jda_half_gray4(src[0], src[1], src[2], src[3]);
        const uint32_t X = x_base + c * 4, Y = y_base + r;
        if (!CLIP) *(jda_u32_alias JDA_GLOBAL *)(out + tile_off + jda_umul24(r, pitch) + c * 4) = v;
        else {
            if (Y >= D.out_rows || X >= D.out_w) continue;
            uint8_t JDA_GLOBAL *row = out + (size_t)Y * pitch;
            const uint32_t n = X + 4 <= D.out_w ? 4u : D.out_w - X;
            if (n == 4) *(jda_u32_alias JDA_GLOBAL *)(row + X) = v;
            else for (uint32_t j = 0; j < n; j++) row[X + j] = (uint8_t)(v >> (8 * j));
        }
    }
}

// Half-size RGB8888 output of 4:2:0 (JPEGPutMCU22 half-size body, jpeg.inl:3577-3626): a pixel's luma is the SUM of its 2x2
// samples, << 10, its chroma the one sample at its place (no averaging), and each channel clamp((k . c + (sum << 10)) >> 12)
// = clamp((((k . c) >> 10) + sum) >> 2) -- two pixels per instruction in the halves of a word.  A work item is 4 pixels of
// one output row: two rows of one luma block (16 bytes) and four Cb / Cr samples.
// per 16-bit lane: arithmetic shift right by 2 (v_pk_ashrrev_i16)
JDA_HD uint32_t jda_pk_ashr2(uint32_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short jda_s2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(jda_s2, a) >> 2);
#else
    const int32_t lo = (int16_t)(a & 0xffffu), hi = (int16_t)(a >> 16);
    return ((uint32_t)(lo >> 2) & 0xffffu) | ((uint32_t)(hi >> 2) << 16);
#endif
}
// the three chroma terms x 64 (the wanted (k . c) >> 10 sits in bits 31:16)
JDA_HD jda_chroma2 jda_chroma_terms64(uint32_t cb8, uint32_t cr8)
{
    const int32_t cb = (int32_t)cb8, cr = (int32_t)cr8;
    jda_chroma2 t;
    t.r = (uint32_t)(64 * 5742 * cr - 64 * 5742 * 128);
    t.g = (uint32_t)(-64 * 1409 * cb - 64 * 2925 * cr + 64 * (1409 + 2925) * 128);
    t.b = (uint32_t)(64 * 7258 * cb - 64 * 7258 * 128);
    return t;
}
JDA_HD void jda_rgba_pair_half(uint32_t ysum2, uint32_t tr, uint32_t tg, uint32_t tb, uint32_t &px0, uint32_t &px1)
{
    const uint32_t r2 = jda_sat_pk_u8(jda_pk_ashr2(jda_pk_add16(ysum2, tr)));
    const uint32_t g2 = jda_sat_pk_u8(jda_pk_ashr2(jda_pk_add16(ysum2, tg)));
    const uint32_t b2 = jda_sat_pk_u8(jda_pk_ashr2(jda_pk_add16(ysum2, tb)));
    const uint32_t rg = jda_perm(g2, r2, 0x05010400u);
    px0 = jda_perm(b2, rg, 0x0d040100u);
    px1 = jda_perm(b2, rg, 0x0d050302u);
}
// the same for RGB565 (JPEGPixelLE / BE through the 10-bit wrapping tables: the identity on this value range, as in jda_565_pair)
template <int PT>
JDA_HD uint32_t jda_565_pair_half(uint32_t ysum2, uint32_t tr, uint32_t tg, uint32_t tb)
{
    const uint32_t r2 = jda_pk_clamp255(jda_pk_ashr2(jda_pk_add16(ysum2, tr)));
    const uint32_t g2 = jda_pk_clamp255(jda_pk_ashr2(jda_pk_add16(ysum2, tg)));
    const uint32_t b2 = jda_pk_clamp255(jda_pk_ashr2(jda_pk_add16(ysum2, tb)));
    uint32_t v = ((r2 & 0x00f800f8u) << 8) | ((g2 & 0x00fc00fcu) << 3) | ((b2 >> 3) & 0x001f001fu);
    if (PT == JDA_RGB565_BIG_ENDIAN) v = jda_perm(0, v, 0x02030001u);
    return v;
}
template <int PT, bool CLIP>
JDA_HD void jda_p4_420_half_rgba(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                                 uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    const uint32_t bpp = PT == JDA_RGB8888 ? 4u : 2u;
    const uint32_t groups = tile_w >> 2;                          // tile_w (output pixels) is a multiple of 8
    const uint32_t inv = jda_recip22(groups);
    uint8_t JDA_GLOBAL *out = JDA_G(uint8_t, D.out);
    const uint32_t pitch = D.out_pitch;
    const uint32_t tile_off = y_base * pitch + x_base * bpp;
    for (uint32_t i = t; i < groups * 8; i += JDA_TILE_THREADS) {
        const uint32_t r = jda_umul24(i, inv) >> 22, g = i - jda_umul24(r, groups);     // output row 0..7, group in the row
        const uint32_t X = x_base + g * 4, Y = y_base + r;
        if (CLIP && (Y >= D.out_rows || X >= D.out_w)) continue;
        // MCU g >> 1, luma block (r >> 2) * 2 + (g & 1), its rows 2 (r & 3) and 2 (r & 3) + 1; chroma row r, columns (g & 1) * 4 ..
        const uint32_t po = jda_umul24(g >> 1, plane_stride);
        const jda_u32_alias *ys = (const jda_u32_alias *)(plane_base + po + ((r >> 2) * 2u + (g & 1u)) * JDA_COEF_STRIDE + (r & 3u) * 16);
        const uint32_t co = po + 4 * JDA_COEF_STRIDE + r * 8 + (g & 1u) * 4;
        const uint32_t s01 = jda_pair_sums(ys[0]) + jda_pair_sums(ys[2]), s23 = jda_pair_sums(ys[1]) + jda_pair_sums(ys[3]);
        const uint32_t cb = *(const jda_u32_alias *)(plane_base + co), cr = *(const jda_u32_alias *)(plane_base + co + JDA_COEF_STRIDE);
        jda_chroma2 c[4];
#pragma unroll
        for (int j = 0; j < 4; j++) c[j] = jda_chroma_terms64((cb >> (8 * j)) & 255u, (cr >> (8 * j)) & 255u);
        uint32_t v[4];
        if (PT == JDA_RGB8888) {
            jda_rgba_pair_half(s01, jda_pack_hi16(c[0].r, c[1].r), jda_pack_hi16(c[0].g, c[1].g), jda_pack_hi16(c[0].b, c[1].b), v[0], v[1]);
            jda_rgba_pair_half(s23, jda_pack_hi16(c[2].r, c[3].r), jda_pack_hi16(c[2].g, c[3].g), jda_pack_hi16(c[2].b, c[3].b), v[2], v[3]);
            if (!CLIP) {
                jda_chunk16_alias q;
                q.w[0] = v[0]; q.w[1] = v[1]; q.w[2] = v[2]; q.w[3] = v[3];
                *(jda_chunk16_alias JDA_GLOBAL *)(out + tile_off + jda_umul24(r, pitch) + g * 16u) = q;
            } else jda_store4<PT, true>(out + (size_t)Y * pitch, X, D.out_w, v);
        } else {
            const uint32_t a01 = jda_565_pair_half<PT>(s01, jda_pack_hi16(c[0].r, c[1].r), jda_pack_hi16(c[0].g, c[1].g), jda_pack_hi16(c[0].b, c[1].b));
            const uint32_t a23 = jda_565_pair_half<PT>(s23, jda_pack_hi16(c[2].r, c[3].r), jda_pack_hi16(c[2].g, c[3].g), jda_pack_hi16(c[2].b, c[3].b));
            if (!CLIP) *(jda_u64_alias JDA_GLOBAL *)(out + tile_off + jda_umul24(r, pitch) + g * 8u) = (uint64_t)a01 | ((uint64_t)a23 << 32);
            else {
                v[0] = a01 & 0xffffu; v[1] = a01 >> 16; v[2] = a23 & 0xffffu; v[3] = a23 >> 16;
                jda_store4<PT, true>(out + (size_t)Y * pitch, X, D.out_w, v);
            }
        }
    }
}

// Half-size colour output of 4:4:4 (JPEGPutMCU11 half-size body, jpeg.inl:3297-3322): luma = the 2x2 sum << 10 as above, each
// chroma sample = (its 2x2 sum + 2) >> 2.  A work item is one output row of one MCU (4 pixels): rows 2r, 2r + 1 of its Y, Cb
// and Cr blocks.
template <int PT, bool CLIP>
JDA_HD void jda_p4_444_half(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                            uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    const uint32_t bpp = PT == JDA_RGB8888 ? 4u : 2u;
    const uint32_t groups = tile_w >> 2;                          // = MCUs in the tile
    const uint32_t inv = jda_recip22(groups);
    uint8_t JDA_GLOBAL *out = JDA_G(uint8_t, D.out);
    const uint32_t pitch = D.out_pitch;
    const uint32_t tile_off = y_base * pitch + x_base * bpp;
    for (uint32_t i = t; i < groups * 4; i += JDA_TILE_THREADS) {
        const uint32_t r = jda_umul24(i, inv) >> 22, g = i - jda_umul24(r, groups);     // output row 0..3, MCU
        const uint32_t X = x_base + g * 4, Y = y_base + r;
        if (CLIP && (Y >= D.out_rows || X >= D.out_w)) continue;
        const jda_u32_alias *ys = (const jda_u32_alias *)(plane_base + jda_umul24(g, plane_stride) + r * 16);
        const jda_u32_alias *bs = (const jda_u32_alias *)((const uint8_t *)ys + JDA_COEF_STRIDE), *rs = (const jda_u32_alias *)((const uint8_t *)ys + 2 * JDA_COEF_STRIDE);
        const uint32_t s01 = jda_pair_sums(ys[0]) + jda_pair_sums(ys[2]), s23 = jda_pair_sums(ys[1]) + jda_pair_sums(ys[3]);
        const uint32_t b01 = ((jda_pair_sums(bs[0]) + jda_pair_sums(bs[2]) + 0x00020002u) >> 2) & 0x00ff00ffu, b23 = ((jda_pair_sums(bs[1]) + jda_pair_sums(bs[3]) + 0x00020002u) >> 2) & 0x00ff00ffu;
        const uint32_t r01 = ((jda_pair_sums(rs[0]) + jda_pair_sums(rs[2]) + 0x00020002u) >> 2) & 0x00ff00ffu, r23 = ((jda_pair_sums(rs[1]) + jda_pair_sums(rs[3]) + 0x00020002u) >> 2) & 0x00ff00ffu;
        jda_chroma2 c[4];
        c[0] = jda_chroma_terms64(b01 & 0xffffu, r01 & 0xffffu); c[1] = jda_chroma_terms64(b01 >> 16, r01 >> 16);
        c[2] = jda_chroma_terms64(b23 & 0xffffu, r23 & 0xffffu); c[3] = jda_chroma_terms64(b23 >> 16, r23 >> 16);
        uint32_t v[4];
        if (PT == JDA_RGB8888) {
            jda_rgba_pair_half(s01, jda_pack_hi16(c[0].r, c[1].r), jda_pack_hi16(c[0].g, c[1].g), jda_pack_hi16(c[0].b, c[1].b), v[0], v[1]);
            jda_rgba_pair_half(s23, jda_pack_hi16(c[2].r, c[3].r), jda_pack_hi16(c[2].g, c[3].g), jda_pack_hi16(c[2].b, c[3].b), v[2], v[3]);
            if (!CLIP) {
                jda_chunk16_alias q;
                q.w[0] = v[0]; q.w[1] = v[1]; q.w[2] = v[2]; q.w[3] = v[3];
                *(jda_chunk16_alias JDA_GLOBAL *)(out + tile_off + jda_umul24(r, pitch) + g * 16u) = q;
            } else jda_store4<PT, true>(out + (size_t)Y * pitch, X, D.out_w, v);
        } else {
            const uint32_t a01 = jda_565_pair_half<PT>(s01, jda_pack_hi16(c[0].r, c[1].r), jda_pack_hi16(c[0].g, c[1].g), jda_pack_hi16(c[0].b, c[1].b));
            const uint32_t a23 = jda_565_pair_half<PT>(s23, jda_pack_hi16(c[2].r, c[3].r), jda_pack_hi16(c[2].g, c[3].g), jda_pack_hi16(c[2].b, c[3].b));
            if (!CLIP) *(jda_u64_alias JDA_GLOBAL *)(out + tile_off + jda_umul24(r, pitch) + g * 8u) = (uint64_t)a01 | ((uint64_t)a23 << 32);
            else {
                v[0] = a01 & 0xffffu; v[1] = a01 >> 16; v[2] = a23 & 0xffffu; v[3] = a23 >> 16;
                jda_store4<PT, true>(out + (size_t)Y * pitch, X, D.out_w, v);
            }
        }
    }
}

// pixel type and clipping are decided once per tile (uniform), so the item loops are branch-free
template <int MODE, bool CLIP>
JDA_HD void jda_p4_full_colour(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                               uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    const int pt = D.pixel_type;
    if (MODE == JDA_MODE_420) {
        if (pt == JDA_RGB8888) jda_p4_420_full<JDA_RGB8888, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
        else if (pt == JDA_RGB565_LITTLE_ENDIAN) jda_p4_420_full<JDA_RGB565_LITTLE_ENDIAN, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
        else jda_p4_420_full<JDA_RGB565_BIG_ENDIAN, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
    } else if (MODE == JDA_MODE_422) {
        if (pt == JDA_RGB8888) jda_p4_422_full<JDA_RGB8888, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
        else if (pt == JDA_RGB565_LITTLE_ENDIAN) jda_p4_422_full<JDA_RGB565_LITTLE_ENDIAN, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
        else jda_p4_422_full<JDA_RGB565_BIG_ENDIAN, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
    } else {
        if (pt == JDA_RGB8888) jda_p4_444_full<JDA_RGB8888, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
        else if (pt == JDA_RGB565_LITTLE_ENDIAN) jda_p4_444_full<JDA_RGB565_LITTLE_ENDIAN, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
        else jda_p4_444_full<JDA_RGB565_BIG_ENDIAN, CLIP>(D, t, plane_base, plane_stride, tile_w, x_base, y_base);
    }
}

// everything else (scaled outputs, luma-only, gray JPEGs): generic per-pixel fetch
template <int MODE>
JDA_HD void jda_p4_generic(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                           uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    typedef jda_mode_traits<MODE> T;
    const int shift = D.scale_shift;
    const uint32_t mw_log2 = (uint32_t)T::MCU_W_LOG2 - (uint32_t)shift;       // MCU tile edge in output px = 1 << mw_log2
    const uint32_t mh = (uint32_t)T::MCU_H >> shift;
    const int pt = D.pixel_type;
    const uint32_t groups = (tile_w + 3) >> 2;
    const uint32_t inv = jda_recip22(groups);
    for (uint32_t i = t; i < groups * mh; i += JDA_TILE_THREADS) {
        const uint32_t row = (i * inv) >> 22, x4 = (i - row * groups) * 4;
        const uint32_t Y = y_base + row, X = x_base + x4;
        if (Y >= D.out_rows || X >= D.out_w) continue;
        uint32_t v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t x = x4 + j;
            v[j] = 0;
            if (x < tile_w) {
                const uint32_t m = x >> mw_log2;
                v[j] = jda_output_pixel<MODE>(plane_base + m * plane_stride, x - (m << mw_log2), row, shift, pt);
            }
        }
        jda_store4_rt<true>(JDA_G(uint8_t, D.out) + (size_t)Y * D.out_pitch, X, D.out_w, pt, v, tile_w - x4 < 4u ? tile_w - x4 : 4u);
    }
}

// 1/4 and 1/8 outputs are a few pixels per MCU (a 4:2:0 tile at 1/8: 20 x 2): one pixel per lane instead of the generic
// stage's four -- the wavefront runs a quarter of the per-pixel code --, consecutive lanes store consecutive pixels
template <int MODE>
JDA_HD void jda_p4_thumb(const jda_dev_desc &D, uint32_t t, const uint8_t *plane_base,
                         uint32_t plane_stride, uint32_t tile_w, uint32_t x_base, uint32_t y_base)
{
    typedef jda_mode_traits<MODE> T;
    const int shift = D.scale_shift;
    const uint32_t mw_log2 = (uint32_t)T::MCU_W_LOG2 - (uint32_t)shift;       // MCU tile edge in output px = 1 << mw_log2
    const uint32_t mh = (uint32_t)T::MCU_H >> shift;
    const int pt = D.pixel_type;
    const uint32_t inv = jda_recip22(tile_w);
    for (uint32_t i = t; i < tile_w * mh; i += JDA_TILE_THREADS) {
        const uint32_t row = jda_umul24(i, inv) >> 22, x = i - jda_umul24(row, tile_w);
        const uint32_t Y = y_base + row, X = x_base + x;
        if (Y >= D.out_rows || X >= D.out_w) continue;
        const uint32_t m = x >> mw_log2;
        const uint32_t v = jda_output_pixel<MODE>(plane_base + jda_umul24(m, plane_stride), x - (m << mw_log2), row, shift, pt);
        uint8_t JDA_GLOBAL *rowp = JDA_G(uint8_t, D.out) + (size_t)Y * D.out_pitch;
        if (pt == JDA_RGB8888) ((jda_u32_alias JDA_GLOBAL *)rowp)[X] = v;
        else if (pt == JDA_EIGHT_BIT_GRAYSCALE) rowp[X] = (uint8_t)v;
        else ((uint16_t JDA_GLOBAL *)rowp)[X] = (uint16_t)v;
    }
}

// the precomputed item addresses belong to an image (pitch, pixel size): made when a wavefront meets a new image
template <int MODE>
JDA_HD void jda_p4_prepare(jda_p4_pre &P, const jda_dev_desc &D, uint32_t t)
{
    typedef jda_lds_layout<MODE> L;
    if (MODE == JDA_MODE_420) jda_p4_precompute(P, t, L::PLANE_STRIDE, D.out_pitch, D.pixel_type == JDA_RGB8888 ? 4u : 2u);
    else if (MODE == JDA_MODE_444) jda_p4_precompute_444(P, t, L::PLANE_STRIDE, D.out_pitch, D.pixel_type == JDA_RGB8888 ? 4u : 2u);
    else {
#pragma unroll
        for (int it = 0; it < JDA_P4_PASSES; it++) P.yo[it] = P.co[it] = P.rel[it] = 0;
    }
}

template <int MODE>
JDA_HD void jda_p4_output_at(const jda_dev_desc &D, const jda_strip &S, const jda_tile_ctx &C, uint32_t t, const uint8_t *wl, const jda_p4_pre &P, bool precomputed);
template <int MODE>
JDA_HD void jda_p4_output(const jda_dev_desc &D, const jda_strip &S, const jda_tile_ctx &C, uint32_t t, const uint8_t *wl, const jda_p4_pre &P)
{
    typedef jda_mode_traits<MODE> T;
    if (C.count == 0) return;
    if (D.strip_mcus == 0) { jda_p4_output_at<MODE>(D, S, C, t, wl, P, true); return; }
    // A strip-major surface: the tile lies inside ONE strip (the tile list is cut at strip edges), and inside it the surface is an
    // ordinary one -- base and pitch of the strip, shifted so that the tile's absolute pixel coordinates address it
    const int shift = D.scale_shift;
    const uint32_t mw = (uint32_t)T::MCU_W >> shift, mh = (uint32_t)T::MCU_H >> shift;
    const uint32_t bpp = D.pixel_type == JDA_RGB8888 ? 4u : (D.pixel_type == JDA_EIGHT_BIT_GRAYSCALE ? 1u : 2u);
    const uint32_t n_sx = (D.mcus_x + D.strip_mcus - 1u) / D.strip_mcus, sx = S.mcu_x0 / D.strip_mcus;
    const uint32_t in_strip = D.mcus_x - sx * D.strip_mcus < D.strip_mcus ? D.mcus_x - sx * D.strip_mcus : D.strip_mcus;      // MCUs of this strip (a row's last one may be narrower)
    const uint32_t pitch = in_strip * mw * bpp;
    const size_t strip_bytes = (size_t)D.strip_mcus * mw * mh * bpp;
    jda_dev_desc V = D;
    V.out_pitch = pitch;
    V.out = D.out + ((size_t)S.mcu_y * n_sx + sx) * strip_bytes - ((size_t)S.mcu_y * mh * pitch + (size_t)sx * D.strip_mcus * mw * bpp);
    jda_p4_output_at<MODE>(V, S, C, t, wl, P, false);
}
template <int MODE>
JDA_HD void jda_p4_output_at(const jda_dev_desc &D, const jda_strip &S, const jda_tile_ctx &C, uint32_t t, const uint8_t *wl, const jda_p4_pre &P, bool precomputed)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    if (C.count == 0) return;
    const int shift = D.scale_shift;
    const uint32_t mw = (uint32_t)T::MCU_W >> shift, mh = (uint32_t)T::MCU_H >> shift;   // MCU tile in output px
    const uint32_t tile_w = C.count * mw;                         // output pixels per row of the tile
    const uint32_t x_base = S.mcu_x0 * mw, y_base = S.mcu_y * mh;
    const uint8_t *plane_base = wl + L::PLANE_OFF;
    const bool colour_out = D.pixel_type != JDA_EIGHT_BIT_GRAYSCALE;
    if ((MODE == JDA_MODE_444 || MODE == JDA_MODE_420 || MODE == JDA_MODE_422) && shift == 0 && colour_out) {      // specialised full-size colour paths
        const bool inside = x_base + tile_w <= D.out_w && y_base + mh <= D.out_rows;   // no clipping in this tile
        if (MODE == JDA_MODE_420 && inside && precomputed && C.count == (uint32_t)L::MCUS) {          // the common case: a full tile
            const int pt = D.pixel_type;
            if (pt == JDA_RGB8888) jda_p4_420_full10<JDA_RGB8888>(D, P, plane_base, x_base, y_base);
            else if (pt == JDA_RGB565_LITTLE_ENDIAN) jda_p4_420_full10<JDA_RGB565_LITTLE_ENDIAN>(D, P, plane_base, x_base, y_base);
            else jda_p4_420_full10<JDA_RGB565_BIG_ENDIAN>(D, P, plane_base, x_base, y_base);
            return;
        }
        if (MODE == JDA_MODE_444 && inside && precomputed && C.count == (uint32_t)L::MCUS) {          // a full 4:4:4 tile
            const int pt = D.pixel_type;
            if (pt == JDA_RGB8888) jda_p4_444_full21<JDA_RGB8888>(D, P, t, plane_base, x_base, y_base);
            else if (pt == JDA_RGB565_LITTLE_ENDIAN) jda_p4_444_full21<JDA_RGB565_LITTLE_ENDIAN>(D, P, t, plane_base, x_base, y_base);
            else jda_p4_444_full21<JDA_RGB565_BIG_ENDIAN>(D, P, t, plane_base, x_base, y_base);
            return;
        }
        if (inside) jda_p4_full_colour<MODE, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        else jda_p4_full_colour<MODE, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
    } else if (shift == 0 && !colour_out) {                       // 8-bit gray, full size: the luma samples are the pixels
        const bool inside = x_base + tile_w <= D.out_w && y_base + mh <= D.out_rows;
        if (inside) jda_p4_gray8_full<MODE, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        else jda_p4_gray8_full<MODE, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
    } else if (MODE == JDA_MODE_420 && shift == 1 && colour_out) {      // the most used scaled colour outputs
        const bool inside = x_base + tile_w <= D.out_w && y_base + mh <= D.out_rows;
        const int pt = D.pixel_type;
        if (pt == JDA_RGB8888) {
            if (inside) jda_p4_420_half_rgba<JDA_RGB8888, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
            else jda_p4_420_half_rgba<JDA_RGB8888, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        } else if (pt == JDA_RGB565_LITTLE_ENDIAN) {
            if (inside) jda_p4_420_half_rgba<JDA_RGB565_LITTLE_ENDIAN, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
            else jda_p4_420_half_rgba<JDA_RGB565_LITTLE_ENDIAN, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        } else {
            if (inside) jda_p4_420_half_rgba<JDA_RGB565_BIG_ENDIAN, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
            else jda_p4_420_half_rgba<JDA_RGB565_BIG_ENDIAN, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        }
    } else if (MODE == JDA_MODE_444 && shift == 1 && colour_out) {
        const bool inside = x_base + tile_w <= D.out_w && y_base + mh <= D.out_rows;
        const int pt = D.pixel_type;
        if (pt == JDA_RGB8888) {
            if (inside) jda_p4_444_half<JDA_RGB8888, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
            else jda_p4_444_half<JDA_RGB8888, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        } else if (pt == JDA_RGB565_LITTLE_ENDIAN) {
            if (inside) jda_p4_444_half<JDA_RGB565_LITTLE_ENDIAN, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
            else jda_p4_444_half<JDA_RGB565_LITTLE_ENDIAN, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        } else {
            if (inside) jda_p4_444_half<JDA_RGB565_BIG_ENDIAN, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
            else jda_p4_444_half<JDA_RGB565_BIG_ENDIAN, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        }
    } else if (shift == 1 && !colour_out) {                       // 8-bit gray, half size: 2x2 luma sums
        const bool inside = x_base + tile_w <= D.out_w && y_base + mh <= D.out_rows && (x_base & 3u) == 0;
        if (inside) jda_p4_gray8_half<MODE, false>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
        else jda_p4_gray8_half<MODE, true>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
    } else if (MODE == JDA_MODE_GRAY && shift >= 2 && !colour_out && C.count == (uint32_t)L::MCUS &&
               x_base + tile_w <= D.out_w && y_base + mh <= D.out_rows) {
        // 8-bit gray thumbnails of a gray file (1/4: the block's 2x2 samples, 1/8: its one), a full unclipped tile: lane = block,
        // the 64 lanes of one store instruction cover one contiguous piece of an output row
        const uint8_t *blk = plane_base + jda_umul24(t, (uint32_t)L::PLANE_STRIDE);
        uint8_t JDA_GLOBAL *o = JDA_G(uint8_t, D.out) + (y_base * D.out_pitch + x_base);
        if (shift == 3) o[t] = blk[0];
        else {
            *(uint16_t JDA_GLOBAL *)(o + 2u * t) = *(const uint16_t *)blk;
            *(uint16_t JDA_GLOBAL *)(o + D.out_pitch + 2u * t) = *(const uint16_t *)(blk + 2);
        }
    } else if (shift >= 2)
        jda_p4_thumb<MODE>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
    else
        jda_p4_generic<MODE>(D, t, plane_base, L::PLANE_STRIDE, tile_w, x_base, y_base);
}

// ---- 1/4 scale: a kernel of its own (jda_quarter_tiles in jda_kernels.hip; tests/hostsim steps the same functions) ---------------
// At 1/4 a block is the 2x2 IDCT of coefficients 0, 1, 8, 9 (jpeg.inl:2305-2326) -- zigzag positions 0, 1, 2, 4: the reference's
// JPEGDecodeMCU stores nothing behind position 4 (:2117-2119), and with a per-block index nothing behind it has to be read either.
// So a block is its DC value (index format 2), at most FOUR AC symbols -- they lie in the 104 bits behind its index entry -- and
// sixteen multiplies: no window in LDS, no coefficient slot, no work lists.  lane = block; the five dwords of the scan that hold those bits
// come straight from memory (neighbouring lanes read neighbouring bytes) and the reader slides through them in registers.
struct jda_q4_bits { uint32_t d[5]; };      // scan dwords, big-endian (byte-swapped): d[0] holds the last CONSUMED bit (jda_q4_first_dword)
struct jda_q4_quant { int32_t q0, q1, q8, q9; };
// the dword of the scan that holds the bit in front of the block's first AC symbol
JDA_HD uint32_t jda_q4_first_dword(uint32_t ix)
{
    const uint32_t p = (ix >> JDA_INDEX_OFF_BITS) * 8u + (ix & (JDA_INDEX_TRUNC - 1u));      // (>= 2: a DC symbol lies in front of it)
    return (p - 1u) >> 5;
}
JDA_HD uint32_t jda_bswap32(uint32_t v) { return jda_perm(0, v, 0x00010203u); }
JDA_HD jda_q4_bits jda_q4_load(const uint8_t *scan, uint32_t scan_len, uint32_t ix)
{
    // (the scan section is 16-byte aligned and JDA_SCAN_PAD zero bytes longer than the scan: 20 bytes from a decoded block's dword stay
    // inside.  The streamed pipeline launches the decode before the device pre-scan's verdict is read: an image that fails it is decoded
    // again, but its entries may point anywhere meanwhile -- so the dword is clamped to the section)
    uint32_t a = jda_q4_first_dword(ix);
    const uint32_t a_max = (scan_len + JDA_SCAN_PAD - 20u) >> 2;
    a = a < a_max ? a : a_max;
    const jda_u32_alias JDA_GLOBAL *w = JDA_G(const jda_u32_alias, scan) + a;
    jda_q4_bits B;
#pragma unroll
    for (int i = 0; i < 5; i++) B.d[i] = w[i];
    return B;
}
// the block's four samples: row 0 in bytes 0-1, row 1 in bytes 2-3 (jda_idct_2x2's order).  EXACT / trunc: as jda_decode_block_win
template <bool EXACT>
JDA_HD uint32_t jda_q4_block(uint32_t ix, int32_t dc, jda_q4_bits B, const uint16_t *ac, const jda_q4_quant &Q, bool dc_only, bool trunc)
{
    const uint32_t off = ix & (JDA_INDEX_TRUNC - 1u);
    const uint32_t p = (ix >> JDA_INDEX_OFF_BITS) * 8u + off;
    uint32_t cm = (p - 1u) & 31u;                         // bit of d0 consumed last
    uint32_t d0 = jda_bswap32(B.d[0]), d1 = jda_bswap32(B.d[1]), d2 = jda_bswap32(B.d[2]), d3 = jda_bswap32(B.d[3]), d4 = jda_bswap32(B.d[4]);
    uint32_t roff = EXACT ? jda_ref_refill(off) : 0u;    // the reference's ulBitOff at the block's first AC symbol
    int32_t c1 = 0, c8 = 0, c9 = 0;                      // (:2118)
    // Four trips without a branch: every symbol moves k on by one at least, so four reach the limit of :2117-2119 (k = 5); a lane whose
    // block ended earlier (EOB, or a symbol that went past the limit) keeps looking symbols up -- in bits that are not its block's any more,
    // harmless: k >= 5 stores nothing -- instead of leaving the loop, because every way out of it is an exec-mask region on the dependent
    // chain (peek -> LUT -> position) and the wavefront runs as many trips as its longest block anyway.
    uint32_t k = dc_only ? 8u : 1u;
#pragma unroll
    for (int trip = 0; trip < 4; trip++) {               // (:2223-2265)
        const uint32_t w = jda_alignbit(d0, d1, 31u - cm);
        const uint32_t e = ac[jda_bfe(w, w >= 0xfc000000u ? 16u : 22u, 11u)];
        const uint32_t len = (e >> 12) + 1u, ms = (e >> 8) & 0xfu;
        k = JDA_AC_STOPS(e) ? 8u : k + ((e >> 1) & 0xfu);    // EOB ends the block; else the run
        uint32_t m = w << len;
        const uint32_t n = len + ms;
        if (EXACT) {
            roff += n;                                   // the reference's ulBitOff after its magnitude read (:2249-2252)
            if (roff > 64u && trunc) m &= ~(0xffffffffu >> ((64u + ms - roff) & 31u));      // its window ended inside the magnitude
            roff = jda_ref_refill(roff);
        }
        // a symbol without magnitude bits stores nothing (:2246, "if (.. && usHuff)"): ZRL goes past the limit, but a run of 1 .. 14 with
        // no value -- no encoder writes one, a table may hold one -- lands on k = 2 .. 4, and jda_extend_top(m, 0) is m, not 0
        const int32_t v = ms ? (int32_t)(int16_t)jda_extend_top(m, ms) : 0;
        c1 = k == 1u ? v : c1; c8 = k == 2u ? v : c8; c9 = k == 4u ? v : c9;
        k++;
        if (trip < 3) {
            cm += n;
            if (cm >= 32u) { d0 = d1; d1 = d2; d2 = d3; d3 = d4; cm -= 32u; }      // (a symbol is 26 bits at most: one step)
        }
    }
    const int32_t a = (int32_t)(int16_t)dc * Q.q0, b = c8 * Q.q8, c = c1 * Q.q1, d = c9 * Q.q9;
    const int32_t t0 = a + b, t2 = a - b, t1 = c + d, t3 = c - d;
    return jda_range_limit5(t0 + t1) | (jda_range_limit5(t0 - t1) << 8) | (jda_range_limit5(t2 + t3) << 16) | (jda_range_limit5(t2 - t3) << 24);
}
// what a lane does with a tile's samples: output pixel i of the tile's (count * MCU_W / 4) x (MCU_H / 4) pixels, row-major, in passes
// of 64; a pixel's samples come from the lanes that decoded its blocks (all: every lane's block samples; GPU: ds_bpermute, so every
// lane runs every pass).  Pixels as JPEGPutMCU* make them at iScaleShift 2 (jda_fetch's shift == 2 cases).
template <int MODE>
JDA_HD void jda_q4_store(const jda_dev_desc &D, const jda_strip &S, uint32_t count, uint32_t lane, uint32_t px, const uint32_t *all)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t mw = (uint32_t)T::MCU_W >> 2, mh = (uint32_t)T::MCU_H >> 2;          // an MCU's pixels: 2 x 2, 4 x 4, 4 x 2, 2 x 4
    const uint32_t tile_w = count * mw, n_px = tile_w * mh;
    const uint32_t x_base = S.mcu_x0 * mw, y_base = S.mcu_y * mh;
    const int pt = D.pixel_type;
    if (MODE == JDA_MODE_GRAY && pt == JDA_EIGHT_BIT_GRAYSCALE && count == 64u && (x_base & 3u) == 0u && x_base + tile_w <= D.out_w && y_base + mh <= D.out_rows) {
        // a whole gray tile to 8-bit gray: two lanes share their blocks' rows -- the even one stores row 0 of both, the odd one row 1
        const uint32_t nb = jda_lane_pull(px, lane ^ 1u, all);
        const uint32_t v = (lane & 1u) ? jda_perm(px, nb, 0x07060302u) : jda_perm(nb, px, 0x05040100u);
        uint8_t JDA_GLOBAL *o = JDA_G(uint8_t, D.out) + ((size_t)(y_base + (lane & 1u)) * D.out_pitch + x_base + 2u * (lane & ~1u));
        *(jda_u32_alias JDA_GLOBAL *)o = v;
        return;
    }
    for (uint32_t i0 = 0; i0 < n_px; i0 += JDA_TILE_THREADS) {
        const uint32_t i = i0 + lane;
        uint32_t row = i >= tile_w ? 1u : 0u;
        if (mh == 4u) row += (i >= 2u * tile_w ? 1u : 0u) + (i >= 3u * tile_w ? 1u : 0u);
        const uint32_t x = i - jda_umul24(row, tile_w);
        const uint32_t m = mw == 4u ? x >> 2 : x >> 1, ax = x & (mw - 1u);
        // the luma block of the MCU and the sample in it; where the chroma sample lies in its block
        uint32_t q = 0, ys, cs;
        if (MODE == JDA_MODE_420) { q = (row >> 1) * 2u + (ax >> 1); ys = (row & 1u) * 2u + (ax & 1u); cs = q; }                   // :3664-3748
        else if (MODE == JDA_MODE_422) { q = ax >> 1; ys = row * 2u + (ax & 1u); cs = row * 2u + q; }                               // :4789-4838
        else if (MODE == JDA_MODE_440) { q = row >> 1; ys = (row & 1u) * 2u + ax; cs = q * 2u + ax; }                               // :4610-4682
        else { ys = row * 2u + ax; cs = ys; }
        const uint32_t yl = (m * (uint32_t)T::NBLK + q) & 63u, cl = (m * (uint32_t)T::NBLK + (uint32_t)T::NLUMA) & 63u;
        const uint32_t yw = jda_lane_pull(px, yl, all);
        uint32_t cbw = 0, crw = 0;
        if (MODE != JDA_MODE_GRAY) { cbw = jda_lane_pull(px, cl, all); crw = jda_lane_pull(px, (cl + 1u) & 63u, all); }
        const uint32_t X = x_base + x, Y = y_base + row;
        if (i >= n_px || X >= D.out_w || Y >= D.out_rows) continue;
        const uint32_t y = (yw >> (8u * ys)) & 0xffu;
        uint8_t JDA_GLOBAL *rowp = JDA_G(uint8_t, D.out) + (size_t)Y * D.out_pitch;
        if (pt == JDA_EIGHT_BIT_GRAYSCALE) rowp[X] = (uint8_t)y;
        else if (MODE == JDA_MODE_GRAY) ((uint16_t JDA_GLOBAL *)rowp)[X] = (uint16_t)jda_gray_565(y, pt != JDA_RGB565_LITTLE_ENDIAN);      // JPEGPutMCUGray
        else {
            jda_ycc c;
            c.y = (int32_t)(y << 12); c.cb = (int32_t)((cbw >> (8u * cs)) & 0xffu); c.cr = (int32_t)((crw >> (8u * cs)) & 0xffu);
            if (pt == JDA_RGB8888) ((jda_u32_alias JDA_GLOBAL *)rowp)[X] = jda_pixel_rgba(c);
            else ((uint16_t JDA_GLOBAL *)rowp)[X] = (uint16_t)jda_pixel_565(c, pt == JDA_RGB565_BIG_ENDIAN);
        }
    }
}

// ---- 4 / 2 / 1-bpp error diffusion (JPEGDither, jpeg.inl:4871-4940) ---------------------------------------------------------------
// The reference keeps ONE byte row E[0 .. W + 1] for the whole image: pixel x of a row adds its forward error, clips at 255, keeps the
// top `bits` bits, halves the residue (h) and spreads it as e1 = 7h >> 3 (to pixel x + 1 of the row), e2 = h - e1 (E[x + 2] is SET to
// it), e3 = 5h >> 3 (added to E[x + 1]), e4 = h - e3 (added to E[x]); the next row's pixel p >= 1 starts from e1 of its left
// neighbour plus E[p + 1].  Followed through one row that byte is
//     down(p) = e2(p - 1) + e3(p) + e4(p + 1)          (terms of pixels outside the row drop out; <= 8 + 39 + 24, so the byte never wraps)
// -- a pure function of the row above, which pixel 0 never reads (its forward error is zero and E[1] is write-only).  The first row of
// a strip reads down(1) as zero (E[0..2] are cleared there and nowhere else), every other byte carries over: the image is one chain.
// A row can therefore run two pixels behind the row above it, the value handed down in a register: lanes = rows.
struct jda_dither_lane {
    uint32_t fwd;       // e1 of the pixel before
    uint32_t a, b;      // a = e2(q - 2) + e3(q - 1), b = e2(q - 1): the parts of down(q - 1), down(q) this row's pixels < q have made
};
JDA_HD uint32_t jda_dither_bits(int32_t pixel_type)
{
    return pixel_type == JDA_FOUR_BIT_DITHERED ? 4u : pixel_type == JDA_TWO_BIT_DITHERED ? 2u : pixel_type == JDA_ONE_BIT_DITHERED ? 1u : 0u;
}
JDA_HD uint32_t jda_dither_pitch(uint32_t width, uint32_t bits) { return (width * bits + 7u) >> 3; }      // (W + 1) / 2, (W + 3) / 4, (W + 7) / 8
// One step of a row: pixel q (live: q lies inside the row and the row inside the image; otherwise the lane only moves its sums along, so
// that the step after the row's last pixel hands down(W - 1) on).  `down`: what the row above handed down for pixel q (the caller passes
// zero for q == 1 of a strip's first row and for the image's first row).  Returns down(q - 1) for the row below; px = the pixel's bits.
JDA_HD uint32_t jda_dither_step(jda_dither_lane &L, bool live, int32_t q, uint32_t gray, uint32_t down, uint32_t bits, uint32_t &px)
{
    uint32_t e1 = 0, e2 = 0, e3 = 0, e4 = 0;
    px = 0;
    if (live) {
        uint32_t c = gray + (q > 0 ? L.fwd + down : 0u);
        if (c > 255u) c = 255u;                              // (the only clip: the sum is never negative)
        px = c >> (8u - bits);
        const uint32_t h = (c & (0xffu >> bits)) >> 1;
        e1 = (7u * h) >> 3; e2 = h - e1; e3 = (5u * h) >> 3; e4 = h - e3;
    }
    const uint32_t out = L.a + e4;
    L.a = L.b + e3; L.b = e2; L.fwd = e1;
    return out;
}
// The byte of a row whose width is not a whole number of bytes: the reference packs in place and never stores the unfinished byte, so
// byte (pitch - 1) of packed row y of a strip still holds the strip's gray byte at linear offset y * pitch + pitch - 1 (row pitch W).
// Returns that offset's (row in the strip, column).
JDA_HD void jda_dither_stale_src(uint32_t y_in_strip, uint32_t width, uint32_t pitch, uint32_t &src_row, uint32_t &src_col)
{
    const uint32_t o = y_in_strip * pitch + pitch - 1u;
    src_row = o / width; src_col = o - src_row * width;
}
// A lane's gray bytes.  Every lane of a wavefront loads at the SAME steps -- t % 16 == 0 -- so that the wavefront waits for memory once
// per 16 steps, for loads issued 16 steps before (a lane that loaded when ITS pixel index reached a multiple of 16 made the whole
// wavefront wait for a load issued a step ago on every other step).  At such a step lane r stands at pixel x0 = t - 2 r = 16 m - s with
// s = (2 r) & 15 and m = t / 16 - (r >> 3): its next 16 pixels are the last s bytes of the aligned 16-byte chunk m - 1 and the first
// 16 - s of chunk m.  It keeps p = chunk m - 1, q = chunk m and n = chunk m + 1 (on its way), and cuts its window w out of p:q at
// the byte offset 16 - s, which never changes.
struct jda_dither_feed { uint32_t p[4], q[4], n[4], w[4]; };
JDA_HD void jda_dither_feed_turn(jda_dither_feed &F, uint32_t s)
{
    uint32_t e[9];
#pragma unroll
    for (int j = 0; j < 4; j++) { F.p[j] = F.q[j]; F.q[j] = F.n[j]; e[j] = F.p[j]; e[4 + j] = F.q[j]; }
    e[8] = 0;
    const uint32_t o = 16u - s, d0 = o >> 2, sh = (o & 3u) * 8u;      // (s is even: sh is 0 or 16)
    uint32_t a[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        uint32_t v = e[j];
#pragma unroll
        for (int k = 1; k < 5; k++) v = d0 == (uint32_t)k ? e[j + k < 8 ? j + k : 8] : v;
        a[j] = v;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) F.w[j] = sh ? (a[j] >> sh) | (a[j + 1] << (32u - sh)) : a[j];
}
#define JDA_DITHER_MAX_WAVES 8
#define JDA_DITHER_LAG 2                     // pixels a row runs behind the row above
#define JDA_DITHER_PUBLISH 32                // the last row of a 64-row group tells the next group every so many pixels
#define JDA_DITHER_LDS_HEAD 64               // bytes in front of the hand-over rows: one progress counter per wavefront

// ---- EXIF orientation (JPEG_AUTO_ROTATE): a pure permutation of the pixels of a decoded canvas -------------------------------------
// src = W x H pixels of BPP bytes, dst = W' x H'; dst(y', x') = src(y, x):
//     0, 1: (y', x')    2: (y', W-1-x')    3: (H-1-y', W-1-x')    4: (H-1-y', x')                       W' x H' = W x H
//     5: (x', y')       6: (H-1-x', y')    7: (H-1-x', W-1-y')    8: (x', W-1-y')                       W' x H' = H x W
// i.e. "source x runs against the destination" for 2, 3, 7, 8 and "source y runs against it" for 3, 4, 6, 7, after a transposition for 5-8.
// Tiles are laid on the DESTINATION, JDA_ORIENT_THREADS lanes a tile, every tile on its own:
//   0-4   a tile is 16 vectors of 16 bytes x 64 rows; a lane moves one vector of four rows.  A mirrored row is read backwards: the 16
//         destination bytes at X come from source bytes [Wb - X - 16, Wb - X), which are not 16-byte aligned when Wb % 16 != 0 -- the lane
//         then loads the two aligned vectors around them and cuts its window out (jda_orient_window16; the cut is the same for the
//         whole surface), reverses the pixels inside it (v_perm) and stores ONE aligned vector.
//   5-8   a tile is 32 x 32 BLOCKS of P x P pixels, P = 4 / BPP: a block is one dword of P source rows and one dword of P destination
//         rows.  Stage: lane = (source row r, dword c) reads along source rows -- both mirrors are applied HERE, rows taken in falling order
//         and dwords cut from falling addresses (jda_orient_window4) and reversed -- and writes the dword to LDS.  Emit: lane = (block row
//         bi, block column bj) reads the P dwords of its block, transposes them in registers (v_perm) and stores one dword to each of P
//         destination rows, 32 lanes side by side along a row.  LDS: source row r at line (r % P) * 32 + r / P, JDA_ORIENT_LDS_STRIDE = 33
//         dwords a line: the stage writes 32 consecutive dwords of a line per half wave, the emit reads dwords 33 apart -- every bank once.
// Only the last vector (dword) of a destination row may be stored narrower; nothing behind W' * BPP bytes of a row or behind row H' is
// written.  Source rows are read in whole aligned vectors: up to the next multiple of 16 (of 4 for 5-8) behind W * BPP, inside the pitch.
// Memory goes through an IO policy so that the kernel (jda_kernels.hip) and the lane-by-lane run on the CPU (tests/hostsim/orient_sim.cpp)
// are the same code.
#define JDA_ORIENT_THREADS 256
#define JDA_ORIENT_ROW_VECS 16u              // 0-4: vectors of 16 bytes across a tile
#define JDA_ORIENT_ROW_ROWS 64u              // 0-4: rows of a tile (four per lane)
#define JDA_ORIENT_BLOCKS 32u                // 5-8: blocks across and down a tile
#define JDA_ORIENT_LDS_STRIDE 33u            // 5-8: dwords from one LDS line to the next
#define JDA_ORIENT_LDS_DWORDS(bpp) (JDA_ORIENT_BLOCKS * (4u / (bpp)) * JDA_ORIENT_LDS_STRIDE)
JDA_HD bool jda_orient_transposes(uint32_t o) { return o >= 5u && o <= 8u; }
JDA_HD bool jda_orient_flips_x(uint32_t o) { return o == 2u || o == 3u || o == 7u || o == 8u; }
JDA_HD bool jda_orient_flips_y(uint32_t o) { return o == 3u || o == 4u || o == 6u || o == 7u; }
JDA_HD void jda_orient_dims(uint32_t o, uint32_t w, uint32_t h, uint32_t &dw, uint32_t &dh)
{
    const bool t = jda_orient_transposes(o);
    dw = t ? h : w; dh = t ? w : h;
}
// tiles across and down the destination of a w x h source
JDA_HD void jda_orient_tile_grid(uint32_t o, uint32_t bpp, uint32_t w, uint32_t h, uint32_t &tiles_x, uint32_t &tiles_y)
{
    uint32_t dw, dh;
    jda_orient_dims(o, w, h, dw, dh);
    if (jda_orient_transposes(o)) {
        const uint32_t tp = JDA_ORIENT_BLOCKS * (4u / bpp);
        tiles_x = (dw + tp - 1u) / tp; tiles_y = (dh + tp - 1u) / tp;
    } else {
        tiles_x = (dw * bpp + JDA_ORIENT_ROW_VECS * 16u - 1u) / (JDA_ORIENT_ROW_VECS * 16u); tiles_y = (dh + JDA_ORIENT_ROW_ROWS - 1u) / JDA_ORIENT_ROW_ROWS;
    }
}
// the surface a tile of the flat list belongs to: the last job whose tile0 is not behind it (tile0 rises; n >= 1)
JDA_HD uint32_t jda_orient_find_job(const jda_orient_job *jobs, uint32_t n, uint32_t tile)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (JDA_G(const jda_orient_job, jobs)[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}
// the pixels of a dword in falling order
template <int BPP> JDA_HD uint32_t jda_orient_reverse(uint32_t v)
{
    return BPP == 4 ? v : BPP == 2 ? jda_perm(0u, v, 0x01000302u) : jda_perm(0u, v, 0x00010203u);
}
// P dwords of P pixels each -> pixel m of out[k] = pixel k of in[m]
template <int BPP> JDA_HD void jda_orient_transpose_block(const uint32_t *in, uint32_t *out)
{
    if (BPP == 4) out[0] = in[0];
    else if (BPP == 2) {
        out[0] = jda_perm(in[1], in[0], 0x05040100u);
        out[1] = jda_perm(in[1], in[0], 0x07060302u);
    } else {
        const uint32_t t0 = jda_perm(in[1], in[0], 0x05010400u), t1 = jda_perm(in[1], in[0], 0x07030602u);
        const uint32_t u0 = jda_perm(in[3], in[2], 0x05010400u), u1 = jda_perm(in[3], in[2], 0x07030602u);
        out[0] = jda_perm(u0, t0, 0x05040100u); out[1] = jda_perm(u0, t0, 0x07060302u);
        out[2] = jda_perm(u1, t1, 0x05040100u); out[3] = jda_perm(u1, t1, 0x07060302u);
    }
}
struct jda_orient_geo {                      // a job, wave-uniform
    const uint8_t *src;
    uint8_t *dst;
    uint32_t src_pitch, dst_pitch, w, h, o;
};
// bytes [so, so + 16) of a source row of row_bytes bytes (so < row_bytes, so > -16; what lies outside the aligned vectors that hold a byte
// of the row reads zero): one aligned load when so is a multiple of 16, else two and a cut at so & 15 -- the same for every lane
template <class IO> JDA_HD void jda_orient_window16(IO &io, const uint8_t *row, int32_t so, uint32_t row_bytes, uint32_t *d)
{
    const uint32_t cut = (uint32_t)so & 15u;
    if (cut == 0u) { io.ld128(row + so, d); return; }
    const int32_t a = so - (int32_t)cut;
    uint32_t e[9];
#pragma unroll
    for (int j = 0; j < 9; j++) e[j] = 0u;
    if (a >= 0) io.ld128(row + a, e);
    if ((uint32_t)(a + 16) < row_bytes) io.ld128(row + a + 16, e + 4);
    const uint32_t dw = cut >> 2, by = cut & 3u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t lo = e[j], hi = e[j + 1];
#pragma unroll
        for (int k = 1; k < 4; k++) if (dw == (uint32_t)k) { lo = e[j + k]; hi = e[j + k + 1]; }
        d[j] = jda_alignbyte(hi, lo, by);
    }
}
// bytes [so, so + 4) of a source row (so < row_bytes, so > -4), the same way with dwords
template <class IO> JDA_HD uint32_t jda_orient_window4(IO &io, const uint8_t *row, int32_t so, uint32_t row_bytes)
{
    const uint32_t cut = (uint32_t)so & 3u;
    if (cut == 0u) return io.ld32(row + so);
    const int32_t a = so - (int32_t)cut;
    const uint32_t lo = a >= 0 ? io.ld32(row + a) : 0u;
    const uint32_t hi = (uint32_t)(a + 4) < row_bytes ? io.ld32(row + a + 4) : 0u;
    return jda_alignbyte(hi, lo, cut);
}
// the first n (1-3) bytes of v: the end of a row that is not a whole number of dwords
template <class IO> JDA_HD void jda_orient_store_tail(IO &io, uint8_t *p, uint32_t v, uint32_t n)
{
    if (n & 2u) { io.st16(p, v & 0xffffu); p += 2; v >>= 16; }
    if (n & 1u) io.st8(p, v & 0xffu);
}
// orientations 0-4, tile (tx, ty), lane tid
template <int BPP, class IO> JDA_HD void jda_orient_rows(const jda_orient_geo &G, uint32_t tx, uint32_t ty, uint32_t tid, IO &io)
{
    const uint32_t row_bytes = G.w * (uint32_t)BPP;
    const uint32_t xb = (tx * JDA_ORIENT_ROW_VECS + (tid & (JDA_ORIENT_ROW_VECS - 1u))) * 16u, r0 = ty * JDA_ORIENT_ROW_ROWS + tid / JDA_ORIENT_ROW_VECS;
    if (xb >= row_bytes) return;
    const bool fx = jda_orient_flips_x(G.o), fy = jda_orient_flips_y(G.o);
    const int32_t so = fx ? (int32_t)row_bytes - (int32_t)xb - 16 : (int32_t)xb;
    const uint32_t step = JDA_ORIENT_THREADS / JDA_ORIENT_ROW_VECS, n = row_bytes - xb < 16u ? row_bytes - xb : 16u;
    uint32_t d[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {            // every load of the lane first, then its stores
        const uint32_t y = r0 + (uint32_t)i * step;
        if (y < G.h) jda_orient_window16(io, G.src + (size_t)(fy ? G.h - 1u - y : y) * G.src_pitch, so, row_bytes, d[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t y = r0 + (uint32_t)i * step;
        if (y >= G.h) continue;
        uint32_t q[4];
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = fx ? jda_orient_reverse<BPP>(d[i][3 - j]) : d[i][j];
        uint8_t *p = G.dst + (size_t)y * G.dst_pitch + xb;
        if (n == 16u) { io.st128(p, q); continue; }
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {                      // the row's last, partial vector: whole dwords, then what is left
            if (j < (n >> 2)) io.st32(p + 4u * j, q[j]);
            else if (j == (n >> 2) && (n & 3u)) jda_orient_store_tail(io, p + 4u * j, q[j], n & 3u);
        }
    }
}
// orientations 5-8, first half: the tile's source dwords into LDS, mirrors applied
template <int BPP, class IO> JDA_HD void jda_orient_stage(const jda_orient_geo &G, uint32_t tx, uint32_t ty, uint32_t tid, IO &io)
{
    const uint32_t P = 4u / (uint32_t)BPP, TP = JDA_ORIENT_BLOCKS * P, row_bytes = G.w * (uint32_t)BPP;
    const bool fx = jda_orient_flips_x(G.o), fy = jda_orient_flips_y(G.o);
#pragma unroll
    for (uint32_t i = 0; i < TP * JDA_ORIENT_BLOCKS / JDA_ORIENT_THREADS; i++) {
        const uint32_t idx = i * JDA_ORIENT_THREADS + tid, r = idx / JDA_ORIENT_BLOCKS, c = idx % JDA_ORIENT_BLOCKS;
        const uint32_t dx = tx * TP + r;                         // the destination column this source row becomes
        const uint32_t dy = ty * TP + c * P;                     // the first of the P destination rows this dword's pixels go to
        uint32_t v = 0u;
        if (dx < G.h && dy < G.w) {
            const uint8_t *row = G.src + (size_t)(fy ? G.h - 1u - dx : dx) * G.src_pitch;
            const int32_t so = fx ? (int32_t)row_bytes - (int32_t)(dy * (uint32_t)BPP) - 4 : (int32_t)(dy * (uint32_t)BPP);
            v = jda_orient_window4(io, row, so, row_bytes);
            if (fx) v = jda_orient_reverse<BPP>(v);
        }
        io.lds_wr(((r % P) * JDA_ORIENT_BLOCKS + r / P) * JDA_ORIENT_LDS_STRIDE + c, v);
    }
}
// .. second half (behind a workgroup barrier): blocks out of LDS, transposed, to the destination
template <int BPP, class IO> JDA_HD void jda_orient_emit(const jda_orient_geo &G, uint32_t tx, uint32_t ty, uint32_t tid, IO &io)
{
    const uint32_t P = 4u / (uint32_t)BPP, TP = JDA_ORIENT_BLOCKS * P, dst_row_bytes = G.h * (uint32_t)BPP;
#pragma unroll
    for (uint32_t i = 0; i < JDA_ORIENT_BLOCKS * JDA_ORIENT_BLOCKS / JDA_ORIENT_THREADS; i++) {
        const uint32_t idx = i * JDA_ORIENT_THREADS + tid, bi = idx / JDA_ORIENT_BLOCKS, bj = idx % JDA_ORIENT_BLOCKS;
        uint32_t in[4], out[4];
#pragma unroll
        for (uint32_t m = 0; m < P; m++) in[m] = io.lds_rd((m * JDA_ORIENT_BLOCKS + bj) * JDA_ORIENT_LDS_STRIDE + bi);
        jda_orient_transpose_block<BPP>(in, out);
        const uint32_t xb = (tx * JDA_ORIENT_BLOCKS + bj) * 4u;
        if (xb >= dst_row_bytes) continue;
        const uint32_t n = dst_row_bytes - xb < 4u ? dst_row_bytes - xb : 4u;
#pragma unroll
        for (uint32_t k = 0; k < P; k++) {
            const uint32_t y = ty * TP + bi * P + k;
            if (y >= G.w) continue;
            uint8_t *p = G.dst + (size_t)y * G.dst_pitch + xb;
            if (n == 4u) io.st32(p, out[k]); else jda_orient_store_tail(io, p, out[k], n);
        }
    }
}

// ---- jda_pack_*: decoded surfaces repacked for a GPU-side consumer -------------------------------------------------
// src = a pixel rectangle {x, y, w, h} of a decoded surface: RGB8888 (bytes R, G, B, A: jda_pixel_rgba) or EIGHT_BIT_GRAYSCALE, at src_pitch.
// dst = DENSE: h * w * C elements pixel-major (JDA_PACK_HWC) or C planes of h * w elements (JDA_PACK_CHW); C = 3 (the alpha byte is never
// part of the result; JDA_PACK_BGR: destination channel c is source byte 2 - c) or 1 (gray).  An element is the source byte (ES = 1) or
// table[c][byte], c = the DESTINATION channel, ES = 2 or 4 bytes: a lookup in the LDS copy of the caller's table, no arithmetic.
// The destination is aligned to ES and to nothing else, so the schedule is laid on ADDRESSES: a RUN is a stretch of destination bytes
// whose element index determines the source byte -- the whole HWC image, or one plane; a gray image is one plane -- and vector v of a run
// is the v-th ALIGNED 16 bytes that hold a byte of it.  A tile = JDA_PACK_THREADS consecutive vectors (4 KiB), a lane = one vector: it
// finds the pixel of its first element (one division by w), walks the rectangle from there (x + 1, at w the next row), loads the aligned
// dword of every pixel it touches, cuts the bytes out (v_perm_b32 for HWC bytes: a destination dword is three bytes of one pixel and one of
// the next, in one of three phases) and stores ONE aligned vector.  Only the first and the last vector of a run may be partial: those go
// out as the aligned dwords, halves and bytes that lie inside the run, so that nothing in front of or behind a run is written (in a batch
// tensor those bytes are the neighbouring image's).  A CHW tile does its vectors of ALL planes, one plane after the other, so that the
// three passes over the same source pixels meet in the cache (the planes' vectors are shifted against each other by what h * w * ES
// leaves of 16).  A lane whose vector reaches in front of the run or behind it still loads -- the first / last pixel again: every load is
// unconditional, no branch between them.  Memory goes through an IO policy: the kernel (jda_kernels.hip) and the lane-by-lane run on the
// CPU (tests/hostsim/pack_sim.cpp) are the same code.
#define JDA_PACK_THREADS 256
#define JDA_PACK_TILE_BYTES (JDA_PACK_THREADS * 16u)
#define JDA_PACK_LDS_DWORDS(es) ((es) == 1 ? 4u : 3u * 256u * (uint32_t)(es) / 4u)
struct jda_pack_geo {                        // a job and the launch's format, wave-uniform
    const uint8_t *src;
    uint8_t *dst;
    uint32_t src_pitch, x, y, w, h, bpp, bgr;
};
// bytes of one run and the number of runs of a job
JDA_HD uint32_t jda_pack_run_bytes(bool hwc, uint32_t es, uint32_t w, uint32_t h) { return w * h * es * (hwc ? 3u : 1u); }
JDA_HD uint32_t jda_pack_runs(bool hwc, uint32_t bpp) { return hwc || bpp == 1u ? 1u : 3u; }
// tiles of a job: the vectors of a run begin up to 15 bytes in front of it
JDA_HD uint32_t jda_pack_tiles_of(uint32_t run_bytes) { return (run_bytes + 15u + JDA_PACK_TILE_BYTES - 1u) / JDA_PACK_TILE_BYTES; }
// the job a tile of the flat list belongs to (as jda_orient_find_job)
JDA_HD uint32_t jda_pack_find_job(const jda_pack_job *jobs, uint32_t n, uint32_t tile)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (JDA_G(const jda_pack_job, jobs)[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}
// the caller's table (C * 256 elements of ES bytes, 16-byte aligned) into LDS, a 16-byte vector a lane and pass
template <int ES, class IO> JDA_HD void jda_pack_stage_table(IO &io, const uint8_t *table, uint32_t channels, uint32_t tid)
{
    const uint32_t vecs = channels * 256u * (uint32_t)ES / 16u;
#pragma unroll
    for (uint32_t i = 0; i < 3u * 256u * (uint32_t)ES / 16u / JDA_PACK_THREADS + 1u; i++) {
        const uint32_t v = i * JDA_PACK_THREADS + tid;
        if (v >= vecs) continue;
        uint32_t q[4];
        io.ld_table128(table + 16u * v, q);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) io.lds_wr(4u * v + j, q[j]);
    }
}
// where a lane is in the rectangle: pixel p = y * w + x, held inside [0, w * h)
struct jda_pack_cursor { uint32_t p, x, y; };
JDA_HD void jda_pack_seek(jda_pack_cursor &c, const jda_pack_geo &G, int32_t q)
{
    const uint32_t npx = G.w * G.h;
    c.p = q < 0 ? 0u : (uint32_t)q < npx ? (uint32_t)q : npx - 1u;
    c.y = c.p / G.w; c.x = c.p - c.y * G.w;
}
// from pixel q to q + 1 (q may lie in front of the rectangle or behind it: the cursor stays on the first / last pixel then)
JDA_HD void jda_pack_step(jda_pack_cursor &c, const jda_pack_geo &G, int32_t q)
{
    const uint32_t adv = (q >= 0 && c.p + 1u < G.w * G.h) ? 1u : 0u;
    c.p += adv; c.x += adv;
    if (c.x == G.w) { c.x = 0u; c.y++; }
}
// the aligned dword that holds the cursor's pixel; shift: the bit its first byte begins at (0 for RGB8888)
template <class IO> JDA_HD uint32_t jda_pack_fetch(IO &io, const jda_pack_geo &G, const jda_pack_cursor &c, uint32_t &shift)
{
    const uint32_t off = (G.x + c.x) * G.bpp;
    shift = (off & 3u) * 8u;
    return io.ld32(G.src + (size_t)(G.y + c.y) * G.src_pitch + (off & ~3u));
}
// K = 16 / ES element bytes v[] of destination channels ch[] -> the vector's four dwords
template <int ES, class IO> JDA_HD void jda_pack_elements(IO &io, const uint32_t *v, const uint32_t *ch, uint32_t *out)
{
    if (ES == 1) {
#pragma unroll
        for (int d = 0; d < 4; d++) out[d] = v[4 * d] | (v[4 * d + 1] << 8) | (v[4 * d + 2] << 16) | (v[4 * d + 3] << 24);
    } else if (ES == 2) {
#pragma unroll
        for (int d = 0; d < 4; d++) out[d] = io.lds_rd16(ch[2 * d] * 256u + v[2 * d]) | (io.lds_rd16(ch[2 * d + 1] * 256u + v[2 * d + 1]) << 16);
    } else {
#pragma unroll
        for (int d = 0; d < 4; d++) out[d] = io.lds_rd32(ch[d] * 256u + v[d]);
    }
}
// the vector at p = run + rel (16-byte aligned; rel < 0: the run begins inside it) of a run of run_bytes bytes: one store where the run
// holds all of it, else the aligned dwords, halves and bytes inside the run
template <class IO> JDA_HD void jda_pack_store(IO &io, uint8_t *p, int32_t rel, uint32_t run_bytes, const uint32_t *out)
{
    const uint32_t b0 = rel < 0 ? (uint32_t)-rel : 0u;
    const uint32_t left = run_bytes - (uint32_t)(rel < 0 ? 0 : rel), b1 = rel < 0 ? (run_bytes + b0 < 16u ? run_bytes + b0 : 16u) : (left < 16u ? left : 16u);
    if (b0 == 0u && b1 == 16u) { io.st128(p, out); return; }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        if (4u * j >= b0 && 4u * j + 4u <= b1) { io.st32(p + 4u * j, out[j]); continue; }
#pragma unroll
        for (uint32_t hh = 0; hh < 2u; hh++) {
            const uint32_t s = 4u * j + 2u * hh, half = (out[j] >> (16u * hh)) & 0xffffu;
            if (s >= b0 && s + 2u <= b1) { io.st16(p + s, half); continue; }
            if (s >= b0 && s < b1) io.st8(p + s, half & 0xffu);
            if (s + 1u >= b0 && s + 1u < b1) io.st8(p + s + 1u, half >> 8);
        }
    }
}
// vector `vec` of plane `run` (JDA_PACK_CHW of an RGB8888 surface: run = destination channel; a gray surface: run 0)
template <int ES, class IO> JDA_HD void jda_pack_planar(const jda_pack_geo &G, uint32_t run, uint32_t vec, IO &io)
{
    const uint32_t K = 16u / (uint32_t)ES, run_bytes = jda_pack_run_bytes(false, ES, G.w, G.h);
    uint8_t *start = G.dst + (size_t)run * run_bytes;
    const int32_t rel = (int32_t)(vec * 16u) - (int32_t)((uintptr_t)start & 15u);
    if (rel >= (int32_t)run_bytes) return;
    const int32_t q0 = rel / ES;                               // (rel is a multiple of ES: the run is aligned to it)
    const uint32_t csh = G.bpp == 4u ? 8u * (G.bgr ? 2u - run : run) : 0u;
    jda_pack_cursor c;
    jda_pack_seek(c, G, q0);
    uint32_t v[16], ch[16], out[4];
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        uint32_t sh;
        const uint32_t d = jda_pack_fetch(io, G, c, sh);
        v[k] = (d >> (sh + csh)) & 0xffu; ch[k] = run;
        jda_pack_step(c, G, q0 + (int32_t)k);
    }
    jda_pack_elements<ES>(io, v, ch, out);
    jda_pack_store(io, start + rel, rel, run_bytes, out);
}
// vector `vec` of a JDA_PACK_HWC image (RGB8888 surface).  Element e = 3 * pixel + channel; the vector's first element e0 >= -15, so
// e0 + 15 = 3 * (its pixel + 5) + its channel: no division of a negative number
template <int ES, class IO> JDA_HD void jda_pack_hwc(const jda_pack_geo &G, uint32_t vec, IO &io)
{
    const uint32_t K = 16u / (uint32_t)ES, NP = (K + 1u) / 3u + 1u, run_bytes = jda_pack_run_bytes(true, ES, G.w, G.h);
    const int32_t rel = (int32_t)(vec * 16u) - (int32_t)((uintptr_t)G.dst & 15u);
    if (rel >= (int32_t)run_bytes) return;
    const uint32_t ii = (uint32_t)(rel / ES + 15), c0 = ii % 3u;
    const int32_t q0 = (int32_t)(ii / 3u) - 5;
    jda_pack_cursor c;
    jda_pack_seek(c, G, q0);
    uint32_t px[8], out[4];
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) px[j] = 0u;
#pragma unroll
    for (uint32_t j = 0; j < NP; j++) {
        uint32_t sh;
        px[j] = jda_pack_fetch(io, G, c, sh);
        jda_pack_step(c, G, q0 + (int32_t)j);
    }
    if (ES == 1) {
        // destination dword d = elements c0 + 4 d ..: pixel a = (c0 + 4 d) / 3 from its channel ph = (c0 + 4 d) % 3 on, then pixel a + 1
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) {
            const uint32_t A = 4u * d / 3u, s = c0 + 4u * d % 3u, wrap = s >= 3u ? 1u : 0u, ph = s - 3u * wrap;
            const uint32_t lo = wrap ? px[A + 1u] : px[A], hi = wrap ? px[A + 2u] : px[A + 1u];
            const uint32_t sel = G.bgr ? (ph == 0u ? 0x06000102u : ph == 1u ? 0x05060001u : 0x04050600u)
                                       : (ph == 0u ? 0x04020100u : ph == 1u ? 0x05040201u : 0x06050402u);
            out[d] = jda_perm(hi, lo, sel);
        }
    } else {
        uint32_t v[8], ch[8];
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t s = c0 + k % 3u, wrap = s >= 3u ? 1u : 0u, cd = s - 3u * wrap;
            const uint32_t p = wrap ? px[k / 3u + 1u] : px[k / 3u];
            v[k] = (p >> (8u * (G.bgr ? 2u - cd : cd))) & 0xffu; ch[k] = cd;
        }
        jda_pack_elements<ES>(io, v, ch, out);
    }
    jda_pack_store(io, G.dst + rel, rel, run_bytes, out);
}
// tile `tile` of a job, lane tid (behind the barrier that follows jda_pack_stage_table where ES > 1)
template <int HWC, int ES, class IO> JDA_HD void jda_pack_tile(const jda_pack_geo &G, uint32_t tile, uint32_t tid, IO &io)
{
    const uint32_t vec = tile * JDA_PACK_THREADS + tid;
    if (HWC) { jda_pack_hwc<ES>(G, vec, io); return; }
    const uint32_t runs = jda_pack_runs(false, G.bpp);
    for (uint32_t r = 0; r < runs; r++) jda_pack_planar<ES>(G, r, vec, io);
}

// ---- jda_unpack_*: dense tensors turned back into surfaces, the inverse of jda_pack_*  ---------------------------------
// src = DENSE: h * w * C elements pixel-major (JDA_PACK_HWC) or C planes of h * w elements (JDA_PACK_CHW), aligned to its element and to
// nothing else; C = 3 (tensor channel c is surface byte c, 2 - c with JDA_PACK_BGR) or 1 (gray).  dst = a surface: RGB8888 (bytes R, G, B
// and A = 0xFF) or EIGHT_BIT_GRAYSCALE, 16-byte aligned, at a pitch that is a multiple of 16.  An element is the byte itself (ES = 1) or a
// float16 / float32 x that becomes clamp(rint(x * scale[c] + bias[c]), 0, 255): the product rounded to float32, the sum rounded again
// (never one fused multiply-add), round-half-to-even, NaN -> 0.
// The schedule is laid on the DESTINATION, the aligned side here: a lane makes one aligned 16-byte vector of a surface row (4 RGBX
// pixels or 16 gray ones), a tile = JDA_UNPACK_THREADS consecutive vectors, row-major over the job's ceil(w * bpp / 16) vectors a row.
// A lane finds its (row, vector) with one division, loads the aligned dwords that hold its source elements (12 HWC bytes: at most 4; a
// plane's 4 bytes: at most 2; F32 elements are dwords), realigns them (v_alignbyte), cuts the bytes out (v_perm_b32) or converts, and
// stores once; only the last vector of a row may be partial and goes out as the dwords, the half and the byte inside the row.  Every
// load is unconditional: a dword behind the image is the image's last dword again.  Neighbouring lanes load neighbouring bytes in every
// format.  Memory goes through an IO policy: the kernel (jda_kernels.hip) and the lane-by-lane run on the CPU
// (tests/hostsim/unpack_sim.cpp) are the same code.
#define JDA_UNPACK_THREADS 256
struct jda_unpack_params { float scale[3], bias[3]; };      // per TENSOR channel (kernel arguments)
struct jda_unpack_geo {                      // a job and the launch's format, wave-uniform
    const uint8_t *src;
    uint8_t *dst;
    uint32_t dst_pitch, w, h, bpp, bgr;
    jda_unpack_params p;
};
JDA_HD uint32_t jda_unpack_row_vectors(uint32_t w, uint32_t bpp) { return (w * bpp + 15u) >> 4; }
JDA_HD uint32_t jda_unpack_tiles_of(uint32_t w, uint32_t h, uint32_t bpp) { return (jda_unpack_row_vectors(w, bpp) * h + JDA_UNPACK_THREADS - 1u) / JDA_UNPACK_THREADS; }
// the job a tile of the flat list belongs to (as jda_pack_find_job)
JDA_HD uint32_t jda_unpack_find_job(const jda_unpack_job *jobs, uint32_t n, uint32_t tile)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (JDA_G(const jda_unpack_job, jobs)[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}
// a float16's bits -> float32, exactly (subnormals kept)
JDA_HD float jda_unpack_half(uint32_t h16)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h16);
#else
    const uint32_t sign = (h16 & 0x8000u) << 16, e = (h16 >> 10) & 31u, m = h16 & 0x3ffu;
    uint32_t bits;
    if (e == 31u) bits = sign | 0x7f800000u | (m << 13) | (m ? 0x00400000u : 0u);      // (v_cvt_f32_f16 quiets a signalling NaN)
    else if (e) bits = sign | ((e + 112u) << 23) | (m << 13);
    else if (!m) bits = sign;
    else {
        uint32_t k = 0, mm = m;
        while (!(mm & 0x400u)) { mm <<= 1; k++; }
        bits = sign | ((113u - k) << 23) | ((mm & 0x3ffu) << 13);
    }
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
#endif
}
JDA_HD float jda_unpack_f32(uint32_t bits)
{
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}
// clamp(rint(x * s + b), 0, 255): two roundings (v_mul_f32, v_add_f32), then v_rndne_f32; NaN -> 0
JDA_HD uint32_t jda_unpack_byte(float x, float s, float b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = x * s;
    const float t = p + b;
    float r = __builtin_rintf(t);
    r = r >= 0.f ? r : 0.f;
    r = r > 255.f ? 255.f : r;
    return (uint32_t)r;
}
// K elements from element e0 on of the job's nbytes dense bytes -> the K * ES / 4 dwords that hold them, realigned: the aligned dwords
// from the one that holds e0's first byte on, one more than the elements fill where they may straddle (ES < 4)
template <int ES, int K, class IO> JDA_HD void jda_unpack_gather(IO &io, const jda_unpack_geo &G, uint32_t nbytes, uint32_t e0, uint32_t *r)
{
    const int NW = K * ES / 4, NL = ES == 4 ? NW : NW + 1;
    const uint32_t lead = (uint32_t)((uintptr_t)G.src & 3u);
    const uint8_t *base = G.src - lead;
    const uint32_t last = (lead + nbytes - 1u) & ~3u, o = lead + e0 * (uint32_t)ES, a0 = o & ~3u;
    uint32_t d[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) {
        const uint32_t a = a0 + 4u * (uint32_t)j;
        d[j] = io.ld32(base + (a < last ? a : last));
    }
#pragma unroll
    for (int j = 0; j < NW; j++) r[j] = ES == 4 ? d[j] : jda_alignbyte(d[j + 1 < NL ? j + 1 : j], d[j], o & 3u);
}
// element k of a gathered stream as a surface byte; c: its TENSOR channel
template <int ES> JDA_HD uint32_t jda_unpack_element(const jda_unpack_geo &G, const uint32_t *r, uint32_t k, uint32_t c)
{
    if (ES == 1) return (r[k >> 2] >> (8u * (k & 3u))) & 0xffu;
    const float x = ES == 2 ? jda_unpack_half((r[k >> 1] >> (16u * (k & 1u))) & 0xffffu) : jda_unpack_f32(r[k]);
    return jda_unpack_byte(x, G.p.scale[c], G.p.bias[c]);
}
// the vector at p, `left` bytes of its row from p on: one store where the row holds all of it, else the dwords, the half and the byte inside
template <class IO> JDA_HD void jda_unpack_store(IO &io, uint8_t *p, uint32_t left, const uint32_t *out)
{
    if (left >= 16u) { io.st128(p, out); return; }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        if (4u * j + 4u <= left) { io.st32(p + 4u * j, out[j]); continue; }
        if (4u * j >= left) continue;
        const uint32_t rem = left - 4u * j;                       // 1 .. 3 (gray rows only)
        if (rem & 2u) io.st16(p + 4u * j, out[j] & 0xffffu);
        if (rem & 1u) io.st8(p + 4u * j + (rem & 2u), (out[j] >> (8u * (rem & 2u))) & 0xffu);
    }
}
// vector `vec` of a job.  HWC = 1: a pixel-major source of three channels; HWC = 0: planes -- three (bpp 4) or the one of a gray image
template <int HWC, int ES, class IO> JDA_HD void jda_unpack_vector(const jda_unpack_geo &G, uint32_t vec, IO &io)
{
    const uint32_t vpr = jda_unpack_row_vectors(G.w, G.bpp);
    const uint32_t row = vec / vpr, col = vec - row * vpr;
    if (row >= G.h) return;
    const uint32_t npx = G.w * G.h;
    uint32_t out[4];
    if (HWC) {
        uint32_t r[3 * ES];
        jda_unpack_gather<ES, 12>(io, G, npx * 3u * (uint32_t)ES, (row * G.w + col * 4u) * 3u, r);
        if (ES == 1) {
            // twelve bytes R G B R G B .. in r[0..2]: pixel p is bytes 3 p .. 3 p + 2
            out[0] = jda_perm(r[1], r[0], G.bgr ? 0x0d000102u : 0x0d020100u);
            out[1] = jda_perm(r[1], r[0], G.bgr ? 0x0d030405u : 0x0d050403u);
            out[2] = jda_perm(r[2], r[1], G.bgr ? 0x0d020304u : 0x0d040302u);
            out[3] = jda_perm(r[2], r[2], G.bgr ? 0x0d010203u : 0x0d030201u);
        } else {
#pragma unroll
            for (uint32_t p = 0; p < 4u; p++) {
                out[p] = 0xff000000u;
#pragma unroll
                for (uint32_t c = 0; c < 3u; c++) out[p] |= jda_unpack_element<ES>(G, r, 3u * p + c, c) << (8u * (G.bgr ? 2u - c : c));
            }
        }
    } else if (G.bpp == 4u) {
        uint32_t pl[3][ES];
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) jda_unpack_gather<ES, 4>(io, G, npx * 3u * (uint32_t)ES, c * npx + row * G.w + col * 4u, pl[c]);
        if (ES == 1) {
            const uint32_t rr = G.bgr ? pl[2][0] : pl[0][0], gg = pl[1][0], bb = G.bgr ? pl[0][0] : pl[2][0];
#pragma unroll
            for (uint32_t p = 0; p < 4u; p++) out[p] = jda_perm(bb, jda_perm(gg, rr, 0x0c0c0400u + p * 0x0101u), 0x0d040100u + (p << 16));
        } else {
#pragma unroll
            for (uint32_t p = 0; p < 4u; p++) {
                out[p] = 0xff000000u;
#pragma unroll
                for (uint32_t c = 0; c < 3u; c++) out[p] |= jda_unpack_element<ES>(G, pl[c], p, c) << (8u * (G.bgr ? 2u - c : c));
            }
        }
    } else {
        uint32_t r[4 * ES];
        jda_unpack_gather<ES, 16>(io, G, npx * (uint32_t)ES, row * G.w + col * 16u, r);
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            if (ES == 1) { out[j] = r[j]; continue; }
            out[j] = 0u;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) out[j] |= jda_unpack_element<ES>(G, r, 4u * j + k, 0u) << (8u * k);
        }
    }
    jda_unpack_store(io, G.dst + (size_t)row * G.dst_pitch + (size_t)col * 16u, G.w * G.bpp - col * 16u, out);
}
// tile `tile` of a job, lane tid
template <int HWC, int ES, class IO> JDA_HD void jda_unpack_tile(const jda_unpack_geo &G, uint32_t tile, uint32_t tid, IO &io)
{
    jda_unpack_vector<HWC, ES>(G, tile * JDA_UNPACK_THREADS + tid, io);
}

// ---- jda_rs_*: decoded surfaces resized with one of Pillow's antialiased convolution filters -------------------------
// The result is Pillow's resize(F, box): a horizontal pass into 8-bit intermediates, then a vertical pass, both
//   out = clip8((2^21 + sum_x in[min + x] * k[x]) >> 22)     per byte of a pixel, 32-bit sum, sum(k) ~ 2^22
// BILINEAR, BOX and HAMMING have k >= 0: unsigned 24-bit multiply-adds, unsigned sums, a one-sided clip (SIGNED = false).  BICUBIC and LANCZOS
// have negative taps (SIGNED = true): u8 x signed 24-bit multiply-adds, signed sums, an arithmetic shift and a two-sided clip; the host's
// guard (jda_resize_axis_guard) holds |k| < 2^23 and every sum inside 32 bits.  Schedule, LDS image, loads and stores are the same.
// with the taps {min, cnt, k[ksize]} of every output coordinate made by the HOST in double (jda_resize_plan.h): the kernel is integer.
// An axis table, in dwords: {min, cnt} of coordinate i at [2 i], its ksize coefficients at [2 out_size + i ksize].
// A workgroup owns one output TILE: JDA_RS_TILE_DWORDS dwords of th <= JDA_RS_TILE_ROWS output rows -- a dword is a pixel of RGB8888
// (its four bytes are four channels) or four neighbouring gray pixels; the vertical pass cannot tell them apart.
//   1. horizontal (jda_rs_horizontal): the source rows [row0, row0 + span) that the tile's vertical taps read, resampled at the tile's
//      columns into LDS, one LDS row of JDA_RS_TILE_DWORDS dwords a source row.  A lane = one dword column (tid & 63), a wave =
//      JDA_RS_HROWS source rows at a time: a coefficient is loaded once for the four rows, and the four row loads are independent.
//      Neighbouring lanes load `scale` pixels apart: strided, but tap x + 1 reads the neighbouring dword of the same line.
//   2. the workgroup barrier
//   3. vertical (jda_rs_vertical): a lane = one aligned 16-byte vector (tid & 15) of one output row (tid >> 4): it sums its four
//      dword columns over the row's taps with ds_read_b128 and stores the vector.  An LDS row is exactly the 256-byte bank row, so the
//      sixteen vectors of a row lie on sixteen different slots whatever the row: every lane group of a ds_read_b128 ({0-3, 12-15,
//      20-27}, ..) holds sixteen different tid & 15, i.e. no bank conflict, without padding.  Only a row's last vector may be partial:
//      it goes out as the dwords and bytes in front of out_w * bpp.
// The host picks th per job so that span <= JDA_RS_LDS_ROWS for every tile (one row at the ksize cap).  Memory goes through an IO
// policy: the kernel (jda_kernels.hip) and the lane-by-lane run on the CPU (tests/hostsim/resize_sim.cpp) are the same code.
#define JDA_RS_THREADS 256
#define JDA_RS_TILE_DWORDS 64u
#define JDA_RS_TILE_ROWS 16u
#define JDA_RS_LDS_ROWS 192u                 // 48 KiB: the LDS budget of a tile
#define JDA_RS_HROWS 4u
struct jda_rs_geo {                          // a job, wave-uniform
    const uint8_t *src;
    uint8_t *dst;
    uint32_t src_pitch, dst_pitch, out_w, out_h, htab, vtab, hk, vk, th;
};
// the job a tile of the flat list belongs to (as jda_orient_find_job)
JDA_HD uint32_t jda_rs_find_job(const jda_resize_job *jobs, uint32_t n, uint32_t tile)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (JDA_G(const jda_resize_job, jobs)[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}
JDA_HD uint32_t jda_rs_clip(uint32_t acc)
{
    const uint32_t v = (acc + (1u << 21)) >> 22;
    return v < 255u ? v : 255u;
}
// .. of a signed filter: clip8(t >> 22) with an arithmetic shift, t = acc + 2^21 (inside 32 bits: the host's guard).  Written as both
// sides first (v_med3_i32 between 0 and 2^30 - 1, the largest t that gives 255), then the shift: the same value for every t.  Shift first
// and the compiler packs two results with v_ashr_pk_u8_i32, whose upper 16 bits it takes for zero; on the MI355X they were not (bytes 2
// and 3 of a dword came out wrong), so the kernels must not contain that instruction.
JDA_HD uint32_t jda_rs_clip(int32_t acc)
{
    const int32_t t = acc + (1 << 21);
    return (uint32_t)(t < 0 ? 0 : (t > (1 << 30) - 1 ? (1 << 30) - 1 : t)) >> 22;
}
// sample x tap into the sum: u8 x k >= 0 (v_mad_u32_u24), or u8 x signed k, |k| < 2^23 (v_mad_i32_i24)
JDA_HD uint32_t jda_rs_mul(uint32_t px, uint32_t k) { return jda_umul24(px, k); }
JDA_HD int32_t jda_rs_mul(uint32_t px, int32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24((int32_t)px, k);
#else
    return (int32_t)((uint32_t)jda_sext24((int32_t)px) * (uint32_t)jda_sext24(k));      // (v_mul_i32_i24: bits 23:0 of both, sign-extended)
#endif
}
// the sum's and the tap's type (unsigned with the 24-bit mask as ever, or signed: the host's guard holds every tap inside 24 bits)
template <bool SIGNED> struct jda_rs_acc { typedef uint32_t type; };
template <> struct jda_rs_acc<true> { typedef int32_t type; };
template <bool SIGNED> JDA_HD typename jda_rs_acc<SIGNED>::type jda_rs_tap(uint32_t raw)
{
    typedef typename jda_rs_acc<SIGNED>::type T;
    return SIGNED ? (T)raw : (T)(raw & 0xffffffu);
}
// tile row ty of a job: its first output row, and the source rows [row0, row0 + span) its vertical taps read (min and min + cnt rise
// with the coordinate, so the first and the last row of the tile bound them)
template <class IO> JDA_HD void jda_rs_tile_rows(const jda_rs_geo &G, uint32_t ty, IO &io, uint32_t &oy0, uint32_t &row0, uint32_t &span)
{
    oy0 = ty * G.th;
    const uint32_t last = (oy0 + G.th < G.out_h ? oy0 + G.th : G.out_h) - 1u;
    row0 = io.ld_tap(G.vtab + 2u * oy0);
    span = io.ld_tap(G.vtab + 2u * last) + io.ld_tap(G.vtab + 2u * last + 1u) - row0;
}
template <int BPP, bool SIGNED = false, class IO> JDA_HD void jda_rs_horizontal(const jda_rs_geo &G, uint32_t tx, uint32_t row0, uint32_t span, uint32_t tid, IO &io)
{
    const uint32_t S = BPP == 4 ? 1u : 4u, C = BPP == 4 ? 4u : 1u;          // output pixels of a dword, channels of a pixel
    const uint32_t col = tid & (JDA_RS_TILE_DWORDS - 1u), wave = tid / JDA_RS_TILE_DWORDS;
    const uint32_t dwc = tx * JDA_RS_TILE_DWORDS + col, row_bytes = G.out_w * (uint32_t)BPP;
    if ((dwc & ~3u) * 4u >= row_bytes) return;                             // (no vector of the row holds this column)
    const bool live = dwc * 4u < row_bytes;                                // (else: behind the row in its last vector, zeros)
    for (uint32_t base = wave * JDA_RS_HROWS; base < span; base += JDA_RS_THREADS / JDA_RS_TILE_DWORDS * JDA_RS_HROWS) {
        const uint8_t *rp[JDA_RS_HROWS];
        uint32_t res[JDA_RS_HROWS];
#pragma unroll
        for (uint32_t j = 0; j < JDA_RS_HROWS; j++) {
            const uint32_t r = base + j < span ? base + j : span - 1u;     // (behind the span: the last row again, not stored)
            rp[j] = G.src + (size_t)(row0 + r) * G.src_pitch;
            res[j] = 0u;
        }
        if (live) {
#pragma unroll
            for (uint32_t s = 0; s < S; s++) {
                const uint32_t ox = dwc * S + s;
                if (ox >= G.out_w) continue;
                const uint32_t xmin = io.ld_tap(G.htab + 2u * ox), cnt = io.ld_tap(G.htab + 2u * ox + 1u), kb = G.htab + 2u * G.out_w + ox * G.hk;
                typename jda_rs_acc<SIGNED>::type acc[JDA_RS_HROWS][4];
#pragma unroll
                for (uint32_t j = 0; j < JDA_RS_HROWS; j++)
#pragma unroll
                    for (uint32_t c = 0; c < 4u; c++) acc[j][c] = 0;
                for (uint32_t x = 0; x < cnt; x++) {
                    const typename jda_rs_acc<SIGNED>::type k = jda_rs_tap<SIGNED>(io.ld_tap(kb + x));
                    const uint32_t off = (xmin + x) * (uint32_t)BPP, sh = (off & 3u) * 8u;
#pragma unroll
                    for (uint32_t j = 0; j < JDA_RS_HROWS; j++) {
                        const uint32_t d = io.ld32(rp[j] + (off & ~3u)) >> sh;
#pragma unroll
                        for (uint32_t c = 0; c < C; c++) acc[j][c] += jda_rs_mul((d >> (8u * c)) & 0xffu, k);
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < JDA_RS_HROWS; j++)
#pragma unroll
                    for (uint32_t c = 0; c < C; c++) res[j] |= jda_rs_clip(acc[j][c]) << (8u * (BPP == 4 ? c : s));
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < JDA_RS_HROWS; j++)
            if (base + j < span) io.lds_wr((base + j) * JDA_RS_TILE_DWORDS + col, res[j]);
    }
}
template <int BPP, bool SIGNED = false, class IO> JDA_HD void jda_rs_vertical(const jda_rs_geo &G, uint32_t tx, uint32_t oy0, uint32_t row0, uint32_t tid, IO &io)
{
    const uint32_t vc = tid & 15u, orow = tid >> 4, oy = oy0 + orow, row_bytes = G.out_w * (uint32_t)BPP;
    const uint32_t b0 = (tx * JDA_RS_TILE_DWORDS + vc * 4u) * 4u;           // the vector's first byte in its destination row
    if (orow >= G.th || oy >= G.out_h || b0 >= row_bytes) return;
    const uint32_t ymin = io.ld_tap(G.vtab + 2u * oy), cnt = io.ld_tap(G.vtab + 2u * oy + 1u), kb = G.vtab + 2u * G.out_h + oy * G.vk;
    typename jda_rs_acc<SIGNED>::type acc[16];
    uint32_t out[4];
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) acc[i] = 0;
    for (uint32_t y = 0; y < cnt; y++) {
        const typename jda_rs_acc<SIGNED>::type k = jda_rs_tap<SIGNED>(io.ld_tap(kb + y));
        uint32_t q[4];
        io.lds_rd128((ymin - row0 + y) * JDA_RS_TILE_DWORDS + vc * 4u, q);
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++) acc[i] += jda_rs_mul((q[i >> 2] >> (8u * (i & 3u))) & 0xffu, k);
    }
#pragma unroll
    for (uint32_t d = 0; d < 4u; d++)
        out[d] = jda_rs_clip(acc[4u * d]) | (jda_rs_clip(acc[4u * d + 1u]) << 8) | (jda_rs_clip(acc[4u * d + 2u]) << 16) | (jda_rs_clip(acc[4u * d + 3u]) << 24);
    uint8_t *p = G.dst + (size_t)oy * G.dst_pitch + b0;
    const uint32_t left = row_bytes - b0;
    if (left >= 16u) { io.st128(p, out); return; }
#pragma unroll
    for (uint32_t d = 0; d < 4u; d++) {
        if (4u * d + 4u <= left) { io.st32(p + 4u * d, out[d]); continue; }
#pragma unroll
        for (uint32_t b = 0; b < 4u; b++)
            if (4u * d + b < left) io.st8(p + 4u * d + b, (out[d] >> (8u * b)) & 0xffu);
    }
}

// ---- jda_rd_*: decoded surfaces shrunk by whole factors, Pillow's Image.reduce((fx, fy), box) -------------------------
// An output pixel is the average of its cell of the box: fx x fy source pixels, fewer in the last column and the last row when the box is
// no multiple of the factors.  Per byte of a pixel, with n the pixels of the cell, in unsigned 32-bit arithmetic
//   out = ((sum + n / 2) * floor(2^24 / n)) >> 24          ((255 n + n / 2) * floor(2^24 / n) <= 255.5 * 2^24 < 2^32 for every n)
// which is NOT the rounded mean (sum + n / 2) / n: about a cell in ten differs by one.  The multipliers of the four kinds of cell a box
// has come from the host (jda_reduce_job::mul).
// A workgroup owns one output TILE: JDA_RD_TILE_BYTES bytes (64 RGB8888 pixels, 256 gray ones) of th <= JDA_RD_TILE_ROWS output rows.
//   1. load (jda_rd_load): the source bytes of the tile are, per source row, one run of bytes; a0, the aligned dword its first byte lies
//      in, is column 0.  The items (output row r of the tile, dword column c) are dealt to the lanes in order: neighbouring lanes load
//      neighbouring dwords of one row whatever the factors, a wave-instruction reads 256 contiguous bytes.  A lane adds the <= fy rows of
//      its column in two registers (bytes 0 and 2, bytes 1 and 3, 16 bits each: fy * 255 < 2^16) and writes the four 16-bit column sums
//      as ONE 8-byte LDS entry; entry c of a row lies at c + (c >> 5), see below.
//   2. the workgroup barrier
//   3. store (jda_rd_store): a lane = one aligned 16-byte vector (tid & 15) of one output row (tid >> 4), as in the resize: it adds the
//      <= fx entries of each of its 4 pixels (RGB8888, ds_read_b64) or the <= fx 16-bit sums of each of its 16 bytes (gray), applies the
//      rule and stores the vector; only a row's last vector may be partial, it goes out as the dwords and bytes in front of out_w * bpp.
//      Neighbouring lanes read 4 fx entries apart; the one spare entry behind every 32 moves each group of 32 by one bank pair, so the 32
//      lanes of a ds_read_b64 group lie on 32 different slots for fx = 1, 2, 4, 8 (the bare stride would put them on 8, 4, 2, 1).
// The host picks th per job so that th rows of entries fit JDA_RD_LDS_BYTES.  Memory goes through an IO policy: the kernel
// (jda_kernels.hip) and the lane-by-lane run on the CPU (tests/hostsim/reduce_sim.cpp) are the same code.
#define JDA_RD_THREADS 256
#define JDA_RD_TILE_BYTES 256u
#define JDA_RD_TILE_ROWS 16u
#define JDA_RD_LDS_BYTES (32u << 10)
// LDS entries of one tile row: the dwords that hold fx * JDA_RD_TILE_BYTES bytes beginning anywhere in a dword, spread as above
JDA_HD uint32_t jda_rd_row_entries(uint32_t fx)
{
    const uint32_t cols = fx * (JDA_RD_TILE_BYTES / 4u) + 1u;
    return cols + (cols >> 5) + 1u;
}
struct jda_rd_geo {                          // a job, wave-uniform
    const uint8_t *src;
    uint8_t *dst;
    uint32_t src_pitch, dst_pitch, x0, y0, bw, bh, fx, fy, out_w, out_h, th, row_entries;
    uint32_t mul_whole, mul_right, mul_bottom, mul_corner;      // jda_reduce_job::mul[0 .. 3]
};
// the job a tile of the flat list belongs to (as jda_rs_find_job)
JDA_HD uint32_t jda_rd_find_job(const jda_reduce_job *jobs, uint32_t n, uint32_t tile)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (JDA_G(const jda_reduce_job, jobs)[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}
// a ? b : c of VALUES (of two members of the job, the bare operator is a choice between their addresses and keeps the job in memory)
JDA_HD uint32_t jda_rd_pick(bool a, uint32_t b, uint32_t c) { return a ? b : c; }
// the rule, for one byte's sum over a cell of n pixels
JDA_HD uint32_t jda_rd_mean(uint32_t sum, uint32_t n, uint32_t mul) { return ((sum + (n >> 1)) * mul) >> 24; }
template <int BPP, class IO> JDA_HD void jda_rd_load(const jda_rd_geo &G, uint32_t tx, uint32_t ty, uint32_t tid, IO &io)
{
    const uint32_t tile_px = JDA_RD_TILE_BYTES / (uint32_t)BPP, opx0 = tx * tile_px;
    const uint32_t npx = G.out_w - opx0 < tile_px ? G.out_w - opx0 : tile_px;
    const uint32_t sx0 = G.x0 + opx0 * G.fx, sx1 = opx0 * G.fx + npx * G.fx < G.bw ? sx0 + npx * G.fx : G.x0 + G.bw;
    const uint32_t a0 = (sx0 * (uint32_t)BPP) & ~3u, cols = (sx1 * (uint32_t)BPP - a0 + 3u) >> 2;
    const uint32_t oy0 = ty * G.th, rows = G.out_h - oy0 < G.th ? G.out_h - oy0 : G.th;
    const uint32_t items = rows * cols;
    for (uint32_t w = tid; w < items; w += JDA_RD_THREADS) {
        const uint32_t r = w / cols, c = w - r * cols;
        const uint32_t sy = (oy0 + r) * G.fy, ny = G.bh - sy < G.fy ? G.bh - sy : G.fy;
        const uint8_t *p = G.src + (size_t)(G.y0 + sy) * G.src_pitch + a0 + 4u * c;
        uint32_t lo = 0, hi = 0;
#pragma unroll 4
        for (uint32_t y = 0; y < ny; y++) {
            const uint32_t d = io.ld32(p + (size_t)y * G.src_pitch);
            lo += d & 0x00ff00ffu;
            hi += (d >> 8) & 0x00ff00ffu;
        }
        io.lds_wr64(r * G.row_entries + c + (c >> 5), (lo & 0xffffu) | (hi << 16), (lo >> 16) | (hi & 0xffff0000u));
    }
}
template <int BPP, class IO> JDA_HD void jda_rd_store(const jda_rd_geo &G, uint32_t tx, uint32_t ty, uint32_t tid, IO &io)
{
    const uint32_t PX = 16u / (uint32_t)BPP;                                // pixels of a vector
    const uint32_t vc = tid & 15u, orow = tid >> 4, oy = ty * G.th + orow, row_bytes = G.out_w * (uint32_t)BPP;
    const uint32_t b0 = tx * JDA_RD_TILE_BYTES + vc * 16u;                  // the vector's first byte in its destination row
    if (orow >= G.th || oy >= G.out_h || b0 >= row_bytes) return;
    const uint32_t sy = oy * G.fy, ny = G.bh - sy < G.fy ? G.bh - sy : G.fy;
    const uint32_t opx0 = tx * (JDA_RD_TILE_BYTES / (uint32_t)BPP), shift = ((G.x0 + opx0 * G.fx) * (uint32_t)BPP) & 3u;
    const uint32_t base = orow * G.row_entries;
    uint32_t out[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
    for (uint32_t j = 0; j < PX; j++) {
        const uint32_t px = vc * PX + j, ox = opx0 + px;                    // the pixel in its tile, in its row
        if (ox >= G.out_w) continue;
        const uint32_t sx = ox * G.fx, nx = G.bw - sx < G.fx ? G.bw - sx : G.fx;
        const uint32_t n = nx * ny, mul = jda_rd_pick(nx < G.fx, jda_rd_pick(ny < G.fy, G.mul_corner, G.mul_right), jda_rd_pick(ny < G.fy, G.mul_bottom, G.mul_whole));
        if (BPP == 4) {
            uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            for (uint32_t i = 0; i < nx; i++) {
                const uint32_t e = px * G.fx + i;
                uint32_t q[2];
                io.lds_rd64(base + e + (e >> 5), q);
                s0 += q[0] & 0xffffu; s1 += q[0] >> 16; s2 += q[1] & 0xffffu; s3 += q[1] >> 16;
            }
            out[j & 3u] = jda_rd_mean(s0, n, mul) | (jda_rd_mean(s1, n, mul) << 8) | (jda_rd_mean(s2, n, mul) << 16) | (jda_rd_mean(s3, n, mul) << 24);
        } else {
            uint32_t s = 0;
            for (uint32_t i = 0; i < nx; i++) {
                const uint32_t h = shift + px * G.fx + i, e = h >> 2;
                s += io.lds_rd16((base + e + (e >> 5)) * 4u + (h & 3u));
            }
            out[j >> 2] |= jda_rd_mean(s, n, mul) << (8u * (j & 3u));
        }
    }
    uint8_t *p = G.dst + (size_t)oy * G.dst_pitch + b0;
    const uint32_t left = row_bytes - b0;
    if (left >= 16u) { io.st128(p, out); return; }
#pragma unroll
    for (uint32_t d = 0; d < 4u; d++) {
        if (4u * d + 4u <= left) { io.st32(p + 4u * d, out[d]); continue; }
#pragma unroll
        for (uint32_t b = 0; b < 4u; b++)
            if (4u * d + b < left) io.st8(p + 4u * d + b, (out[d] >> (8u * b)) & 0xffu);
    }
}

// ================================================================================================
// jda_coef_tiles: a tile decoded from COEFFICIENTS (a coefficient image: every scan of a progressive file decoded on the host, or a
// DCT-domain caller's own).  The tile is the decode kernel's -- one wave64, <= 64 consecutive blocks of an MCU row,
// the same LDS slots --, and P1 is replaced by a load phase:
//   load    lane = 16-byte chunk = one row of a block's 8x8 coefficients (natural order, 128 bytes a block in HBM): the tile's
//           blocks are consecutive there, so a pass of 64 lanes is 1 KiB of coalesced 16-byte loads; all eight passes are issued,
//           without a branch between them, before the first one is stored (in the compiled code the waits count down at the
//           stores: read off the ISA, profiles/progressive_code_object.txt, not timed).  A chunk goes into its block's slot (two 8-byte LDS
//           stores: the slots are 136 bytes apart, 8-byte aligned), and while it passes through registers its share of the block's
//           u16MCUFlags is formed as JPEGDecodeMCU would have (jpeg.inl:2207-2208, :2253-2254): for every nonzero AC coefficient
//           at natural index n, (1 << (n & 7)) | (n << 8) -- one uint16 per chunk, parked where the column list will be;
//   flags   lane = block: the OR of its eight chunk words (one 16-byte LDS read).  0 = DC only (:5146-5154).
// (The LDS stores' bank pattern -- 16 bytes a lane, a 136-byte step every eight lanes -- has not been measured nor run through a conflict
// counter: tests/hostsim/coef_sim.cpp checks addresses and values, not banks.)
// In a baseline stream those flags depend only on which positions hold a coded (hence nonzero) coefficient, so equal coefficients
// give equal pixels.  Behind the flags come the decode kernel's own list, column, row and colour stages (jda_p1_lists .. jda_p4_output),
// every multiply in 32 bits.  The table copy in LDS holds what those stages read: the nibble lists and the four quantiser tables.
#define JDA_CT_TAB_BYTES 2048u                               // (JDA_LT_NIB and JDA_LT_QUANT_OFF(0..3) lie below 1,792)
#define JDA_CT_QUANT_BYTES 512u                              // a coefficient image's table blob in HBM: 4 x 64 int16, prescaled, natural order
#define JDA_CT_BLOCK_BYTES 128u
template <int MODE> struct jda_ct_layout {
    enum { WAVE_BYTES = (JDA_CT_TAB_BYTES + jda_lds_layout<MODE>::BASE_BYTES + 15) / 16 * 16 };
};

// io.ld128(base, i, v): the i-th 16-byte vector behind the global pointer `base` (16-byte aligned).  Every load of the load phase is
// UNCONDITIONAL (a lane with nothing to fetch re-reads a vector that is there): no branch between the loads, so they are issued back to
// back (what the compiled code shows; no timing behind it).
template <class IO> JDA_HD void jda_ct_tables(IO &io, const uint8_t *quant, uint32_t lane, uint8_t *tab)
{
    uint32_t v[4];
    io.ld128(quant, lane & (JDA_CT_QUANT_BYTES / 16u - 1u), v);
    if (lane < JDA_CT_QUANT_BYTES / 16u) {
        jda_u32_alias *dst = (jda_u32_alias *)(tab + JDA_LT_QUANT_OFF(lane >> 3) + 16u * (lane & 7u));
        dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
    } else if (lane < JDA_CT_QUANT_BYTES / 16u + 2u) {      // the 16 nibble lists (as jda_p0_tables_from makes them)
        const uint32_t i = lane - JDA_CT_QUANT_BYTES / 16u;
        jda_u32_alias *dst = (jda_u32_alias *)(tab + JDA_LT_NIB + 16u * i);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) dst[k] = jda_nibble_list(i * 8u + 2u * k) | (jda_nibble_list(i * 8u + 2u * k + 1u) << 16);
    }
}

// what the list and column stages need of jda_lane_pre: the lane's quantiser table and its column work item
template <int MODE> JDA_HD void jda_ct_lane_prepare(jda_lane_pre &LP, const jda_dev_desc &D, uint32_t lane)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t b = lane % (uint32_t)T::NBLK;
    const uint32_t c = b < (uint32_t)T::NLUMA ? 0u : b - T::NLUMA + 1u;
    const uint32_t q_id = jda_pick3(D.q_id, c) & 3u;
    LP.dc_off = 0; LP.ac_off = 0; LP.ac_long_off = 0; LP.eob_sh = 0; LP.eob_code = 0;
    LP.quant_off = JDA_LT_QUANT_OFF(q_id);
    LP.qsel = (JDA_LT_QUANT_OFF(q_id) >> 7) << 10;
    LP.item_pre = LP.qsel | (lane << 4);
    LP.chroma = b >= (uint32_t)T::NLUMA ? 1u : 0u;
}

// the flag word of row `row` of a block: v = its eight int16, two to a dword
JDA_HD uint32_t jda_ct_row_flags(const uint32_t v[4], uint32_t row)
{
    uint32_t cols = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (v[j] & 0xffffu) cols |= 1u << (2u * j);
        if (v[j] >> 16) cols |= 2u << (2u * j);
    }
    if (row == 0u) cols &= ~1u;                              // (entry 0 is the DC value: no flag)
    if (cols == 0u) return 0u;
    // OR of n = 8 row + column over the nonzero ones: the row's bits, and bit k of the OR of the columns
    const uint32_t orn = (row << 3) | ((cols & 0xaau) ? 1u : 0u) | ((cols & 0xccu) ? 2u : 0u) | ((cols & 0xf0u) ? 4u : 0u);
    return cols | (orn << 8);
}

// D.scan: the image's coefficients (16-byte aligned).  C: first_block / count of the tile (count >= 1).
template <int MODE, class IO> JDA_HD void jda_ct_load(IO &io, const jda_dev_desc &D, const jda_tile_ctx &C, uint32_t lane, uint8_t *wl)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    const uint32_t n_chunks = C.count * (uint32_t)T::NBLK * 8u;
    const uint32_t c0 = C.first_block * 8u;                  // the tile's first chunk among the image's
    uint32_t v[8][4];
#pragma unroll
    for (uint32_t p = 0; p < 8; p++) {
        const uint32_t c = p * 64u + lane;
        io.ld128(D.scan, c0 + (c < n_chunks ? c : 0u), v[p]);
    }
    uint16_t *cw = (uint16_t *)(wl + L::COLLIST_OFF);
#pragma unroll
    for (uint32_t p = 0; p < 8; p++) {
        const uint32_t c = p * 64u + lane, blk = c >> 3, row = c & 7u;
        if (c >= n_chunks) continue;
        jda_u64_alias *dst = (jda_u64_alias *)(wl + L::COEF_OFF + blk * JDA_COEF_STRIDE + row * 16u);
        dst[0] = (uint64_t)v[p][0] | ((uint64_t)v[p][1] << 32);
        dst[1] = (uint64_t)v[p][2] | ((uint64_t)v[p][3] << 32);
        cw[c] = (uint16_t)jda_ct_row_flags(v[p], row);
    }
}

// lane = block: its u16MCUFlags (0 = DC only), or JDA_NO_LIST (no block, chroma of a luma-only decode)
template <int MODE> JDA_HD uint32_t jda_ct_flags(const jda_dev_desc &D, const jda_tile_ctx &C, const jda_lane_pre &LP, uint32_t lane, const uint8_t *wl)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    if (lane >= C.count * (uint32_t)T::NBLK) return JDA_NO_LIST;
    if (MODE != JDA_MODE_GRAY && D.gray_from_color && LP.chroma) return JDA_NO_LIST;
    const jda_u32_alias *w = (const jda_u32_alias *)(wl + L::COLLIST_OFF + 16u * lane);
    const uint32_t f = w[0] | w[1] | w[2] | w[3];
    return (f | (f >> 16)) & 0xffffu;
}

// ================================================================================================
// jda_sparse_tiles: the same tile from the SPARSE form of a coefficient image: an entry per nonzero coefficient,
//   entry = (g & 1023) << 22 | n << 16 | (uint16_t)value     g: the block's number, n: natural index (0 = DC), ascending within a block
//   first[g] .. first[g + 1]: block g's entries -- a tile's blocks are consecutive, so its entries are ONE contiguous range.
// D.tables: quantisers | first[] (behind JDA_CT_QUANT_BYTES); D.scan: the entries (16-byte aligned).  The load phase that stands in
// for jda_ct_load:
//   zero     the tile's slots (128 bytes of each, 8-byte stores: the slots are 136 bytes apart) and its chunk words;
//   range    first[b0] and first[b0 + nb]: wave-uniform;
//   scatter  lane = 16-byte vector of four entries of the range aligned down to 16 bytes, 64 vectors a pass, JDA_CS_GROUP passes
//            issued back to back without a branch between them (a lane with nothing to fetch re-reads the range's first vector),
//            entries outside [e0, e1) masked.  An entry's slot in the tile is ((e >> 22) - b0) & 1023 -- a tile is <= 64 blocks, so
//            ten bits of g suffice, as for the continuation entries of the baseline index --; its value is one 16-bit LDS store, and
//            for n > 0 its flag word (1 << (n & 7)) | (n << 8) is ORed into the block's chunk word n >> 3 (an LDS atomic OR on the
//            dword that holds the word: several entries of a row, and of the neighbouring row, meet there).
// Behind it the slots and chunk words are those jda_ct_load leaves over the dense form of the same coefficients -- cols = OR of
// 1 << (n & 7), the high byte = OR of n --, so jda_ct_flags and every later stage run unchanged and give equal pixels.
// (Neither the bank pattern of the 2-byte scatter nor the cost of the LDS atomics has been measured on hardware.)
#define JDA_CS_GROUP 4u
// io.ld32u(base, i): the i-th dword behind `base`, the same address in every lane (wave-uniform)
template <int MODE, class IO> JDA_HD void jda_cs_range(IO &io, const jda_dev_desc &D, const jda_tile_ctx &C, uint32_t *e0, uint32_t *e1)
{
    typedef jda_mode_traits<MODE> T;
    const uint8_t *first = D.tables + JDA_CT_QUANT_BYTES;
    *e0 = io.ld32u(first, C.first_block);
    *e1 = io.ld32u(first, C.first_block + C.count * (uint32_t)T::NBLK);
}

template <int MODE> JDA_HD void jda_cs_zero(const jda_tile_ctx &C, uint32_t lane, uint8_t *wl)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    const uint32_t nb = C.count * (uint32_t)T::NBLK;
#pragma unroll
    for (uint32_t p = 0; p < 16; p++) {                      // 16 8-byte stores a block
        const uint32_t i = p * 64u + lane;
        if (i < nb * 16u) *(jda_u64_alias *)(wl + L::COEF_OFF + (i >> 4) * JDA_COEF_STRIDE + (i & 15u) * 8u) = 0;
    }
    if (lane < nb) {                                         // eight chunk words a block
        jda_u64_alias *cw = (jda_u64_alias *)(wl + L::COLLIST_OFF + 16u * lane);
        cw[0] = 0; cw[1] = 0;
    }
}

typedef uint16_t __attribute__((may_alias)) jda_u16_alias;
template <int MODE, class IO> JDA_HD void jda_cs_scatter(IO &io, const jda_dev_desc &D, const jda_tile_ctx &C, uint32_t lane, uint32_t e0, uint32_t e1, uint8_t *wl)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    if (e1 <= e0) return;                                    // (wave-uniform: a tile of empty blocks)
    const uint32_t nb = C.count * (uint32_t)T::NBLK;
    const uint32_t v0 = e0 >> 2, v1 = (e1 + 3u) >> 2;        // the vectors that hold the range
    for (uint32_t base = v0; base < v1; base += 64u * JDA_CS_GROUP) {       // (wave-uniform trip count)
        uint32_t v[JDA_CS_GROUP][4];
#pragma unroll
        for (uint32_t p = 0; p < JDA_CS_GROUP; p++) {
            const uint32_t vi = base + p * 64u + lane;
            io.ld128(D.scan, vi < v1 ? vi : v0, v[p]);
        }
#pragma unroll
        for (uint32_t p = 0; p < JDA_CS_GROUP; p++) {
            const uint32_t vi = base + p * 64u + lane;
            if (vi >= v1) continue;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t ei = vi * 4u + j, e = v[p][j];
                const uint32_t slot = ((e >> 22) - C.first_block) & 1023u, n = (e >> 16) & 63u;
                if (ei < e0 || ei >= e1 || slot >= nb) continue;      // (slot < nb for every entry the host packs: nothing leaves the tile's LDS)
                *(jda_u16_alias *)(wl + L::COEF_OFF + slot * JDA_COEF_STRIDE + 2u * n) = (uint16_t)e;
                if (n) {
                    const uint32_t ci = slot * 8u + (n >> 3);
                    jda_lds_or_u32(wl + L::COLLIST_OFF + (ci >> 1) * 4u, ((1u << (n & 7u)) | (n << 8)) << ((ci & 1u) * 16u));
                }
            }
        }
    }
}

// ================================================================================================
// jda_en_*: decoded surfaces encoded as baseline JPEG files.  The definition is libjpeg's (jcparam.c, jccolor.c,
// jcsample.c, jfdctint.c, jcdctmgr.c, jchuff.c) and is stated once more, in numpy, in tests/encode_util.py.  Six stages, each a
// kernel of jda_kernels.hip, the work of a lane written here behind an IO policy so that tests/hostsim/encode_sim.cpp steps the same code:
//   blocks   lane = one block of the call's flat list (a job's blocks in the order of its scan): the 64 samples of its component
//            -- colour conversion, replication at the rectangle's edges, h2v1 / h2v2 downsampling -- in registers, the islow FDCT rows
//            then columns, quantisation by a host-made reciprocal, 64 x int16 in zig-zag order (128 bytes) to HBM, and beside it the
//            block's DC and the length of its AC code.  A dummy block (luma blocks of the MCU grid that hold no pixel) is zeros.
//   lengths  lane = block: the DC of the block before it of its component (dummies passed over; none at an interval's start) gives
//            the DC difference and the block's whole code length; a dummy takes that DC as its own.
//   scan     a workgroup = a job: positions from lengths.  Every lane sums a run of consecutive elements, then the runs in front of
//            its own, then walks its run again.  An interval starts on a byte, so the sum is of functions p -> (round ? ceil8(p + a)
//            : p) + b, which compose.  The same stage sums the 0xFF counts of the stuffing chunks.
//   emit     lane = block: its code at its bit position in the job's UNSTUFFED scan, dword by dword with an atomic OR into zeroed
//            memory (a dword may hold the ends of two blocks, or many whole ones); an interval's last block adds the 1-bits to the byte.
//   count    lane = a 64-byte chunk of an unstuffed scan: the 0xFF bytes in it.
//   write    lane = chunk: the chunk's bytes at their place in the file -- behind the header, the stuffed zeros of the chunks before
//            and two bytes for every RSTm before --, RSTm in front of an interval's first byte, EOI behind the last byte; the header's
//            chunks are copied.  A job whose file is longer than its capacity is left out as a whole.
#define JDA_EN_THREADS 256
#define JDA_EN_DUMMY 0x80000000u           // in a block's word of the blocks stage: (AC bits << 16) | (DC & 0xffff)
struct jda_en_arrays {                     // the call's scratch, device pointers
    const jda_encode_dev_job *jobs;
    const jda_encode_quant *quant;
    const uint32_t *huff;
    const uint8_t *hdr;
    int16_t *coef;                         // 64 a block
    uint32_t *meta, *code;                 // a block: blocks stage -> lengths stage ((difference << 16) | code bits)
    uint64_t *end;                         // a block: the bit behind its code, from its job's first
    uint64_t *istart;                      // an interval: its first byte in the unstuffed scan
    jda_encode_totals *totals;             // a job
    uint8_t *u;                            // the unstuffed scans (zeros before emit)
    uint32_t *ffcnt;                       // a chunk
    uint64_t *ffend;
    uint32_t n_jobs;
};
template <class IO> JDA_HD uint32_t jda_en_find_block(const jda_encode_dev_job *jobs, uint32_t n, uint32_t b, IO &io)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (io.ld32(&jobs[mid].block0) <= b) lo = mid; else hi = mid;
    }
    return lo;
}
template <class IO> JDA_HD uint32_t jda_en_find_chunk(const jda_encode_dev_job *jobs, uint32_t n, uint32_t c, IO &io)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (io.ld32(&jobs[mid].chunk0) <= c) lo = mid; else hi = mid;
    }
    return lo;
}
JDA_HD uint32_t jda_en_zigzag(uint32_t z)  // natural index of zig-zag position z (folded: every caller's z is a constant of an unrolled loop)
{
    constexpr uint8_t nat[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
    return nat[z];
}
JDA_HD uint32_t jda_en_nbits(uint32_t a) { return a ? 32u - (uint32_t)__builtin_clz(a) : 0u; }
// one pass of jfdctint.c over eight values; FIRST: the row pass (results up by PASS1_BITS), else the column pass (down by it)
template <bool FIRST> JDA_HD void jda_en_fdct8(int32_t &d0, int32_t &d1, int32_t &d2, int32_t &d3, int32_t &d4, int32_t &d5, int32_t &d6, int32_t &d7)
{
    constexpr int N = FIRST ? 11 : 15;
    const int32_t R = 1 << (N - 1);
    const int32_t t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) { d0 = (t10 + t11) << 2; d4 = (t10 - t11) << 2; }
    else { d0 = (t10 + t11 + 2) >> 2; d4 = (t10 - t11 + 2) >> 2; }
    int32_t z1 = (t12 + t13) * 4433;
    d2 = (z1 + t13 * 6270 + R) >> N;
    d6 = (z1 - t12 * 15137 + R) >> N;
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d7 = (u4 + z1 + z3 + R) >> N;
    d5 = (u5 + z2 + z4 + R) >> N;
    d3 = (u6 + z2 + z3 + R) >> N;
    d1 = (u7 + z1 + z4 + R) >> N;
}
// where block s of a job lies: its MCU, its component (0: luma), its block row and column in the component
JDA_HD void jda_en_place(const jda_encode_dev_job &J, uint32_t s, uint32_t &m, uint32_t &c, uint32_t &by, uint32_t &bx)
{
    m = s / J.bpm;
    const uint32_t k = s - m * J.bpm, my = m / J.cx, mx = m - my * J.cx, nl = J.hs * J.vs;
    if (k < nl) { const uint32_t v = k / J.hs; c = 0; by = my * J.vs + v; bx = mx * J.hs + (k - v * J.hs); }
    else { c = 1u + k - nl; by = my; bx = mx; }
}
// component c of a pixel: (kr R + kg G + kb B + add) >> 16, libjpeg's jccolor.c
JDA_HD int32_t jda_en_comp(uint32_t px, int32_t kr, int32_t kg, int32_t kb, int32_t add)
{
    return (kr * (int32_t)(px & 0xffu) + kg * (int32_t)((px >> 8) & 0xffu) + kb * (int32_t)((px >> 16) & 0xffu) + add) >> 16;
}
template <class IO> JDA_HD void jda_en_block(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t b, IO &io)
{
    const uint32_t s = b - J.block0;
    uint32_t m, c, by, bx;
    jda_en_place(J, s, m, c, by, bx);
    uint32_t w[32];
    const uint32_t t = c ? 1u : 0u;
    int16_t *out = A.coef + (size_t)b * 64u;
    if (c == 0u && (bx >= J.wb || by >= J.hb)) {              // a dummy: zeros (the lengths stage gives it its DC), an EOB
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) w[i] = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) io.st128(out + 8u * i, w);
        io.st32(A.meta + b, JDA_EN_DUMMY | ((io.ld32(A.huff) >> 16) << 16));
        return;
    }
    int32_t d[64];
    const uint8_t *base = J.src + (size_t)J.y * J.src_pitch;
    if (J.nc == 1u) {
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++) {
            const uint32_t py = by * 8u + r < J.h ? by * 8u + r : J.h - 1u;
            const uint8_t *row = base + (size_t)py * J.src_pitch + J.x;
#pragma unroll
            for (uint32_t q = 0; q < 8u; q++) {
                const uint32_t px = bx * 8u + q < J.w ? bx * 8u + q : J.w - 1u;
                d[r * 8u + q] = (int32_t)io.ld_px8(row + px) - 128;
            }
        }
    } else {
        const int32_t kr = c == 0u ? 19595 : c == 1u ? -11059 : 32768, kg = c == 0u ? 38470 : c == 1u ? -21709 : -27439;
        const int32_t kb = c == 0u ? 7471 : c == 1u ? 32768 : -5329, add = c == 0u ? 32768 : (128 << 16) + 32767;
        const uint32_t sh = c ? J.hs : 1u, sv = c ? J.vs : 1u;         // source pixels of a sample
        if (sh == 1u) {
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                const uint32_t py = by * 8u + r < J.h ? by * 8u + r : J.h - 1u;
                const uint8_t *row = base + (size_t)py * J.src_pitch + (size_t)J.x * 4u;
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++) {
                    const uint32_t px = bx * 8u + q < J.w ? bx * 8u + q : J.w - 1u;
                    d[r * 8u + q] = jda_en_comp(io.ld_px32(row + px * 4u), kr, kg, kb, add) - 128;
                }
            }
        } else {
            // the plane goes down by replication to a multiple of sv rows only; the DOWNSAMPLED plane's last row is replicated below that
            const uint32_t ch = (J.h + sv - 1u) / sv;
#pragma unroll
            for (uint32_t r = 0; r < 8u; r++) {
                const uint32_t oy = by * 8u + r < ch ? by * 8u + r : ch - 1u;
                const uint32_t y0 = oy * sv, y1 = oy * sv + sv - 1u < J.h ? oy * sv + sv - 1u : J.h - 1u;
                const uint8_t *row0 = base + (size_t)y0 * J.src_pitch + (size_t)J.x * 4u, *row1 = base + (size_t)y1 * J.src_pitch + (size_t)J.x * 4u;
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++) {
                    const uint32_t ox = bx * 8u + q;
                    const uint32_t x0 = 2u * ox < J.w ? 2u * ox : J.w - 1u, x1 = 2u * ox + 1u < J.w ? 2u * ox + 1u : J.w - 1u;
                    int32_t v = jda_en_comp(io.ld_px32(row0 + x0 * 4u), kr, kg, kb, add) + jda_en_comp(io.ld_px32(row0 + x1 * 4u), kr, kg, kb, add);
                    if (sv == 2u) {
                        v += jda_en_comp(io.ld_px32(row1 + x0 * 4u), kr, kg, kb, add) + jda_en_comp(io.ld_px32(row1 + x1 * 4u), kr, kg, kb, add);
                        v = (v + 1 + (int32_t)(q & 1u)) >> 2;          // bias 1, 2, 1, 2 along the row (ox and q have the same parity)
                    } else v = (v + (int32_t)(q & 1u)) >> 1;            // bias 0, 1, 0, 1
                    d[r * 8u + q] = v - 128;
                }
            }
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < 8u; r++) jda_en_fdct8<true>(d[r * 8u], d[r * 8u + 1u], d[r * 8u + 2u], d[r * 8u + 3u], d[r * 8u + 4u], d[r * 8u + 5u], d[r * 8u + 6u], d[r * 8u + 7u]);
#pragma unroll
    for (uint32_t q = 0; q < 8u; q++) jda_en_fdct8<false>(d[q], d[8u + q], d[16u + q], d[24u + q], d[32u + q], d[40u + q], d[48u + q], d[56u + q]);
    // quantise in zig-zag order; the AC code's length on the way
    const jda_encode_quant *Q = A.quant + J.quant;
    const uint32_t *ac = A.huff + t * 256u;
    uint32_t bits = 0, run = 0, dc = 0;
#pragma unroll
    for (uint32_t z = 0; z < 64u; z++) {
        const uint32_t n = jda_en_zigzag(z);
        const int32_t v = d[n];
        const uint32_t a = (uint32_t)(v < 0 ? -v : v) + io.ld32(&Q->half[t][n]);
        const uint32_t r = (uint32_t)(((uint64_t)a * io.ld32(&Q->recip[t][n])) >> 32);       // = a / (8 q): a < 2^17, 8 q <= 2040
        const uint32_t val = (uint32_t)(v < 0 ? -(int32_t)r : (int32_t)r) & 0xffffu;
        if (z & 1u) w[z >> 1] |= val << 16; else w[z >> 1] = val;
        if (z == 0u) dc = val;
        else if (r == 0u) run++;
        else {
            bits += (run >> 4) * (io.ld32(ac + 0xf0u) >> 16) + (io.ld32(ac + (((run & 15u) << 4) | jda_en_nbits(r))) >> 16) + jda_en_nbits(r);
            run = 0;
        }
    }
    if (run) bits += io.ld32(ac) >> 16;
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) io.st128(out + 8u * i, w + 4u * i);
    io.st32(A.meta + b, (bits << 16) | dc);
}
template <class IO> JDA_HD void jda_en_length(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t b, IO &io)
{
    const uint32_t s = b - J.block0, m = s / J.bpm, k = s - m * J.bpm, nl = J.hs * J.vs;
    const uint32_t *meta = A.meta + J.block0;
    const uint32_t me = io.ld32(meta + s);
    const bool fresh = m == 0u || (J.ri && m % J.ri == 0u);          // the MCU opens an interval
    int32_t pred = 0;
    if (k < nl && k > 0u) {
        uint32_t j = s - 1u, v = io.ld32(meta + j);
        while (v & JDA_EN_DUMMY) v = io.ld32(meta + --j);             // (an MCU's first block is never a dummy)
        pred = (int16_t)(v & 0xffffu);
    } else if (!fresh) {
        uint32_t j = k < nl ? (m - 1u) * J.bpm + nl - 1u : s - J.bpm, v = io.ld32(meta + j);
        while (v & JDA_EN_DUMMY) v = io.ld32(meta + --j);
        pred = (int16_t)(v & 0xffffu);
    }
    int32_t diff = 0;
    if (me & JDA_EN_DUMMY) io.st16(A.coef + (size_t)b * 64u, (int16_t)pred);
    else diff = (int32_t)(int16_t)(me & 0xffffu) - pred;
    const uint32_t cat = jda_en_nbits((uint32_t)(diff < 0 ? -diff : diff));
    const uint32_t bits = ((me >> 16) & 0x7fffu) + (io.ld32(A.huff + 512u + (k < nl ? 0u : 16u) + cat) >> 16) + cat;
    io.st32(A.code + b, ((uint32_t)diff << 16) | bits);
}

// ---- scan: position of every element of a job's list from the elements' lengths.  Element i of [first, first + n) has the length
// vals[i] & mask and, with period != 0, starts on a byte where (i - first) % period == 0.  end[i] = the position behind it.
// LDS: 768 x 64 bits: a lane's run as the function p -> (r ? ceil8(p + a) : p) + b: a at [tid], b at [256 + tid], r at [512 + tid].
struct jda_en_fn { uint64_t a, b; uint32_t r; };
JDA_HD uint64_t jda_en_ceil8(uint64_t p) { return (p + 7u) & ~(uint64_t)7u; }
JDA_HD uint64_t jda_en_apply(const jda_en_fn &f, uint64_t p) { return (f.r ? jda_en_ceil8(p + f.a) : p) + f.b; }
JDA_HD void jda_en_then(jda_en_fn &f, bool round, uint64_t len)      // f := (an element of length len, on a byte if round) after f
{
    if (!round) { f.b += len; return; }
    if (f.r) f.b = jda_en_ceil8(f.b) + len;
    else { f.r = 1u; f.a = f.b; f.b = len; }
}
JDA_HD void jda_en_run(uint32_t n, uint32_t tid, uint32_t &i0, uint32_t &i1)
{
    const uint32_t per = (n + JDA_EN_THREADS - 1u) / JDA_EN_THREADS;
    i0 = tid * per < n ? tid * per : n;
    i1 = i0 + per < n ? i0 + per : n;
}
template <class IO> JDA_HD void jda_en_scan_local(const uint32_t *vals, uint32_t mask, uint32_t first, uint32_t n, uint32_t period, uint32_t tid, IO &io)
{
    uint32_t i0, i1;
    jda_en_run(n, tid, i0, i1);
    jda_en_fn f = { 0u, 0u, 0u };
    for (uint32_t i = i0; i < i1; i++) jda_en_then(f, period && i && i % period == 0u, io.ld32(vals + first + i) & mask);
    io.lds_wr64(tid, f.a); io.lds_wr64(256u + tid, f.b); io.lds_wr64(512u + tid, f.r);
}
// behind the barrier.  Returns the position behind the job's last element in the lane that owns it, else ~0
template <class IO> JDA_HD uint64_t jda_en_scan_write(const uint32_t *vals, uint32_t mask, uint32_t first, uint32_t n, uint32_t period, uint64_t *end, uint64_t *istart,
                                                      uint32_t tid, IO &io)
{
    uint32_t i0, i1;
    jda_en_run(n, tid, i0, i1);
    if (i0 >= i1) return ~(uint64_t)0;
    uint64_t p = 0;
    for (uint32_t j = 0; j < tid; j++) {
        jda_en_fn f;
        f.a = io.lds_rd64(j); f.b = io.lds_rd64(256u + j); f.r = (uint32_t)io.lds_rd64(512u + j);
        p = jda_en_apply(f, p);
    }
    for (uint32_t i = i0; i < i1; i++) {
        if (istart && (period ? i % period == 0u : i == 0u)) {
            p = jda_en_ceil8(p);
            io.st64(istart + (period ? i / period : 0u), p >> 3);
        }
        p += io.ld32(vals + first + i) & mask;
        io.st64(end + first + i, p);
    }
    return i1 == n ? p : ~(uint64_t)0;
}

// ---- emit: a block's code into the unstuffed scan
template <class IO> struct jda_en_bits { uint64_t acc; uint32_t n; uint32_t *dw; IO *io; };
template <class IO> JDA_HD void jda_en_flush(jda_en_bits<IO> &W)
{
    const uint32_t v = (uint32_t)(W.acc >> 32);
    if (v) W.io->atomic_or(W.dw, ((v & 0xffu) << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24));
}
template <class IO> JDA_HD void jda_en_put(jda_en_bits<IO> &W, uint32_t v, uint32_t len)      // len <= 16 bits of v, n < 32 on entry
{
    if (!len) return;
    W.acc |= (uint64_t)(v & ((1u << len) - 1u)) << (64u - W.n - len);
    W.n += len;
    if (W.n >= 32u) { jda_en_flush(W); W.acc <<= 32; W.n -= 32u; W.dw++; }
}
template <class IO> JDA_HD void jda_en_emit(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t b, IO &io)
{
    const uint32_t s = b - J.block0, m = s / J.bpm, k = s - m * J.bpm, t = k < J.hs * J.vs ? 0u : 1u;
    const uint32_t code = io.ld32(A.code + b);
    const int32_t diff = (int32_t)(int16_t)(code >> 16);
    const uint64_t start = J.u_off * 8u + io.ld64(A.end + b) - (code & 0xffffu);
    jda_en_bits<IO> W;
    W.acc = 0; W.n = (uint32_t)(start & 31u); W.dw = (uint32_t *)A.u + (start >> 5); W.io = &io;
    const uint32_t *huff = A.huff + J.huff_off, *ac = huff + t * 256u;      // (the job's own words where it is optimised)
    const uint32_t cat = jda_en_nbits((uint32_t)(diff < 0 ? -diff : diff)), hd = io.ld32(huff + 512u + t * 16u + cat);
    jda_en_put(W, hd & 0xffffu, hd >> 16);
    jda_en_put(W, (uint32_t)(diff < 0 ? diff - 1 : diff), cat);
    const uint32_t zrl = io.ld32(ac + 0xf0u);
    uint32_t run = 0;
    for (uint32_t i = 0; i < 8u; i++) {
        uint32_t w[4];
        io.ld128(A.coef + (size_t)b * 64u + 8u * i, w);
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            if (i == 0u && j == 0u) continue;
            const int32_t v = (int32_t)(int16_t)((w[j >> 1] >> (16u * (j & 1u))) & 0xffffu);
            if (v == 0) { run++; continue; }
            for (; run > 15u; run -= 16u) jda_en_put(W, zrl & 0xffffu, zrl >> 16);
            const uint32_t sz = jda_en_nbits((uint32_t)(v < 0 ? -v : v)), h = io.ld32(ac + ((run << 4) | sz));
            jda_en_put(W, h & 0xffffu, h >> 16);
            jda_en_put(W, (uint32_t)(v < 0 ? v - 1 : v), sz);
            run = 0;
        }
    }
    if (run) { const uint32_t h = io.ld32(ac); jda_en_put(W, h & 0xffffu, h >> 16); }
    const uint32_t period = J.ri * J.bpm;
    if (s + 1u == J.n_blocks || (period && (s + 1u) % period == 0u)) jda_en_put(W, 0xffu, (8u - (W.n & 7u)) & 7u);      // the interval's 1-bits to the byte
    if (W.n) jda_en_flush(W);
}

// ---- count and write: the unstuffed scan's chunks
template <class IO> JDA_HD void jda_en_count(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t c, IO &io)
{
    const uint32_t local = c - J.chunk0;
    uint32_t cnt = 0;
    if (local >= J.h_chunks) {
        const uint8_t *p = A.u + J.u_off + (size_t)(local - J.h_chunks) * JDA_EN_CHUNK;
        for (uint32_t i = 0; i < JDA_EN_CHUNK / 16u; i++) {
            uint32_t w[4];
            io.ld128(p + 16u * i, w);
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++) cnt += ((w[j >> 2] >> (8u * (j & 3u))) & 0xffu) == 0xffu ? 1u : 0u;
        }
    }
    io.st32(A.ffcnt + c, cnt);
}
template <class IO> JDA_HD void jda_en_write(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t job, uint32_t c, IO &io)
{
    const uint64_t u_bytes = io.ld64(&A.totals[job].u_bytes);
    if (io.ld64(&A.totals[job].file_bytes) > J.capacity) return;       // the file does not fit: no byte of it is written
    const uint32_t local = c - J.chunk0;
    if (local < J.h_chunks) {
        const uint32_t o = local * JDA_EN_CHUNK, left = J.hdr_len - o < JDA_EN_CHUNK ? J.hdr_len - o : JDA_EN_CHUNK;
        for (uint32_t i = 0; i < left; i++) io.st8(J.dst + o + i, io.ld8(A.hdr + J.hdr_off + o + i));
        return;
    }
    const uint64_t p0 = (uint64_t)(local - J.h_chunks) * JDA_EN_CHUNK;
    const uint64_t *ist = A.istart + J.int0;
    uint32_t lo = 0, hi = J.n_int;                                      // intervals [1, next) start in front of p0: their markers are in front of this chunk
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (io.ld64(ist + mid) < p0) lo = mid; else hi = mid;
    }
    uint32_t next = lo + 1u;
    uint8_t *q = J.dst + J.hdr_len + p0 + (io.ld64(A.ffend + c) - io.ld32(A.ffcnt + c)) + 2u * (uint64_t)lo;
    uint64_t nx = next < J.n_int ? io.ld64(ist + next) : ~(uint64_t)0;
    const uint8_t *src = A.u + J.u_off + p0;
    for (uint32_t i = 0; i < JDA_EN_CHUNK / 16u; i++) {
        if (p0 + 16u * i >= u_bytes) break;
        uint32_t w[4];
        io.ld128(src + 16u * i, w);
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++) {
            const uint64_t p = p0 + 16u * i + j;
            if (p >= u_bytes) continue;
            if (p == nx) {
                io.st8(q++, 0xffu); io.st8(q++, 0xd0u + ((next - 1u) & 7u));
                next++;
                nx = next < J.n_int ? io.ld64(ist + next) : ~(uint64_t)0;
            }
            const uint32_t v = (w[j >> 2] >> (8u * (j & 3u))) & 0xffu;
            io.st8(q++, v);
            if (v == 0xffu) io.st8(q++, 0u);
            if (p + 1u == u_bytes) { io.st8(q++, 0xffu); io.st8(q++, 0xd9u); }
        }
    }
}
// a job's scan, one lane: bytes = the 0xFF counts of its chunks (else its blocks' code lengths), second = behind the barrier
template <class IO> JDA_HD void jda_en_scan_job(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t job, bool bytes, bool second, uint32_t tid, IO &io)
{
    const uint32_t *vals = bytes ? A.ffcnt : A.code;
    const uint32_t mask = bytes ? 0xffffffffu : 0xffffu, first = bytes ? J.chunk0 : J.block0, n = bytes ? J.n_chunks : J.n_blocks, period = bytes ? 0u : J.ri * J.bpm;
    if (!second) { jda_en_scan_local(vals, mask, first, n, period, tid, io); return; }
    const uint64_t p = jda_en_scan_write(vals, mask, first, n, period, bytes ? A.ffend : A.end, bytes ? (uint64_t *)0 : A.istart + J.int0, tid, io);
    if (p == ~(uint64_t)0) return;
    if (!bytes) io.st64(&A.totals[job].u_bytes, jda_en_ceil8(p) >> 3);
    else io.st64(&A.totals[job].file_bytes, (uint64_t)J.hdr_len + io.ld64(&A.totals[job].u_bytes) + p + 2u * (uint64_t)(J.n_int - 1u) + 2u);
}

// ---- jda_ho_*: Huffman tables of a file's own (JDA_ENCODE_OPTIMIZE; DESIGN.md 5.13 rule 9).  Two stages between lengths and scan, each a
// kernel of jda_kernels.hip (jda_huffopt_*), stepped by tests/hostsim/huffopt_sim.cpp:
//   gather   lane = block, a workgroup = 256 consecutive blocks of the flat list.  A workgroup keeps ONE histogram of JDA_EN_HUFF_DWORDS in
//            LDS -- the word tables' index layout: AC symbol rs of table t at [t * 256 + rs], DC category s at [512 + t * 16 + s] -- and
//            takes the jobs that own blocks of its 256 one after the other: clear, barrier, the job's lanes add their symbols (the DC
//            category from the difference of the lengths stage, the AC symbols from the block's 128 bytes of coefficients, a ZRL for
//            every 16 zeros in front of a coefficient, an EOB where the block ends in zeros), barrier, the nonzero bins are added to
//            the job's histogram in HBM, barrier.  Dummy blocks count like any other.  A job that is not optimised is passed over.
//   lengths  lane = block: the same walk once more with the job's own code words: the low 16 bits of the block's word of the lengths
//            stage are written again.  A standard job's blocks are left alone.
template <class IO> JDA_HD void jda_ho_clear(uint32_t tid, IO &io)
{
    for (uint32_t i = tid; i < JDA_EN_HUFF_DWORDS; i += JDA_EN_THREADS) io.lds_st32(i, 0u);
}
template <class IO> JDA_HD void jda_ho_flush(uint32_t *hist, uint32_t tid, IO &io)
{
    for (uint32_t i = tid; i < JDA_EN_HUFF_DWORDS; i += JDA_EN_THREADS) {
        const uint32_t v = io.lds_ld32(i);
        if (v) io.atomic_add(hist + i, v);
    }
}
// a block's symbols, each handed to sym(index in the word tables' layout, extra bits behind its code)
template <class IO, class F> JDA_HD void jda_ho_symbols(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t b, IO &io, F &&sym)
{
    const uint32_t s = b - J.block0, m = s / J.bpm, k = s - m * J.bpm, t = k < J.hs * J.vs ? 0u : 1u;
    const int32_t diff = (int32_t)(int16_t)(io.ld32(A.code + b) >> 16);
    const uint32_t cat = jda_en_nbits((uint32_t)(diff < 0 ? -diff : diff));
    sym(512u + t * 16u + cat, cat);
    uint32_t run = 0;
    for (uint32_t i = 0; i < 8u; i++) {
        uint32_t w[4];
        io.ld128(A.coef + (size_t)b * 64u + 8u * i, w);
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            if (i == 0u && j == 0u) continue;
            const int32_t v = (int32_t)(int16_t)((w[j >> 1] >> (16u * (j & 1u))) & 0xffffu);
            if (v == 0) { run++; continue; }
            for (; run > 15u; run -= 16u) sym(t * 256u + 0xf0u, 0u);
            const uint32_t sz = jda_en_nbits((uint32_t)(v < 0 ? -v : v));
            sym(t * 256u + ((run << 4) | sz), sz);
            run = 0;
        }
    }
    if (run) sym(t * 256u, 0u);
}
template <class IO> JDA_HD void jda_ho_count(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t b, IO &io)
{
    jda_ho_symbols(A, J, b, io, [&io](uint32_t index, uint32_t) { io.lds_add32(index, 1u); });
}
template <class IO> JDA_HD void jda_ho_length(const jda_en_arrays &A, const jda_encode_dev_job &J, uint32_t b, IO &io)
{
    if (J.hist_off == JDA_EN_NO_HIST) return;
    const uint32_t *huff = A.huff + J.huff_off;
    uint32_t bits = 0;
    jda_ho_symbols(A, J, b, io, [&io, &bits, huff](uint32_t index, uint32_t extra) { bits += (io.ld32(huff + index) >> 16) + extra; });
    io.st32(A.code + b, (io.ld32(A.code + b) & 0xffff0000u) | bits);
}

// ================================================================================================
// jda_pe_*: the same coefficients written as a PROGRESSIVE file (DESIGN.md 5.13 rules 10 to 14): libjpeg's default scan script and
// jcphuff.c's four passes.  The work item is a UNIT, one block of one scan; a call's units form one flat list, a job's scans (its
// SEGMENTS, jda_pe_seg) in file order.  Behind blocks and lengths of jda_en_* (the coefficients; a dummy block's DC) nine launches:
//   classify lane = unit of an AC scan: does it emit a symbol of its own (JDA_PE_BREAKER: a pending end-of-band run is flushed in front of
//            it), does its band end in zeros or in correction bits (JDA_PE_JOINS: EOBRUN++), how many correction bits it hands to the
//            run, and -- a refinement scan -- the last newly nonzero position (no ZRL is written behind it).  DC units: 0.
//   resolve  lane = unit.  A unit that joins and is the first of its scan, or a breaker, or follows one that does not join, opens a
//            stretch and walks it (eight records a step) to the unit in front of the next breaker: run after run, each cut at 0x7FFF
//            units or once more than 937 correction bits are buffered (libjpeg's greedy rule; it does not compose as a prefix function,
//            hence the walk).  A run's bits belong to its FIRST unit, behind that unit's own
//            (the units behind it in the run have none): the head's word holds the run's length and its buffered bits, every other
//            unit's the distance to the head and its own offset in the buffered bits.  Every word is written by exactly one lane.
//   gather   a workgroup = 256 consecutive units, one histogram of 256 bins in LDS, the segments it meets taken in turn as
//            jda_huffopt_gather takes jobs: a unit's own symbols and, at a head, the run's EOBn.
//   lengths  lane = unit: its bits under the scan's own code words -- a head's with the run's symbol, extra bits and buffered bits.
//   scan     a workgroup = a segment: positions from lengths (jda_en_scan_* as they stand); every scan starts on a byte of its own.
//            The second launch: a workgroup = a job, the file offsets of its chunks.
//   emit     lane = unit: its own code at its position; its correction bits at their offset in its run's tail; the scan's last unit
//            adds the 1-bits to the byte.
//   count    lane = chunk: a header chunk's bytes, or a data chunk's bytes and 0xFF bytes.
//   write    lane = chunk: header bytes copied, data bytes stuffed; the job's last chunk adds EOI.
#define JDA_PE_BREAKER 1u
#define JDA_PE_JOINS 2u
#define JDA_PE_INRUN 0x80000000u           // a unit's word of the resolve stage: INRUN | (distance to the head << 10) | offset in the buffered bits,
#define JDA_PE_HEAD 0x40000000u            // a head's: INRUN | HEAD | (units of the run << 10) | buffered bits
#define JDA_PE_MAX_RUN 0x7fffu
#define JDA_PE_MAX_BE 937u                 // MAX_CORR_BITS - DCTSIZE2 + 1
#define JDA_PE_NO_SYMBOL 0xffffffffu
struct jda_pe_arrays {
    jda_en_arrays E;                       // jobs, quant, huff (Annex K: blocks and lengths), coef, meta, code, totals, u, ffcnt, ffend
    const jda_pe_seg *segs;
    const jda_pe_job *pjobs;
    const uint32_t *words;                 // the scans' code words (jda_pe_seg.tab)
    const uint8_t *hdr;
    uint32_t *cls, *run, *len;             // a unit
    uint64_t *end;                         // a unit: the bit behind its bits, from its scan's first
    uint64_t *sbytes;                      // a segment: the bytes of its unstuffed data
    uint32_t n_segs;
};
template <class IO> JDA_HD uint32_t jda_pe_find(const jda_pe_seg *segs, uint32_t n, uint32_t x, bool chunk, IO &io)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (io.ld32(chunk ? &segs[mid].chunk0 : &segs[mid].unit0) <= x) lo = mid; else hi = mid;
    }
    return lo;
}
// the block (of the call's flat list) of unit r of a segment: a DC scan walks the job's blocks as they lie, a scan of one component that
// component's own blocks in raster order
JDA_HD uint32_t jda_pe_block(const jda_pe_seg &S, const jda_encode_dev_job &J, uint32_t r)
{
    if (S.comp == JDA_PE_ALL) return J.block0 + r;
    const uint32_t by = r / S.wbc, bx = r - by * S.wbc;
    if (S.comp == 0u) {
        const uint32_t my = by / J.vs, mx = bx / J.hs;
        return J.block0 + (my * J.cx + mx) * J.bpm + (by - my * J.vs) * J.hs + (bx - mx * J.hs);
    }
    return J.block0 + (by * J.cx + bx) * J.bpm + J.hs * J.vs + S.comp - 1u;
}
// f(z, value) for the coefficients ss .. se of a block
template <class IO, class F> JDA_HD void jda_pe_band(const int16_t *blk, uint32_t ss, uint32_t se, IO &io, F &&f)
{
    for (uint32_t i = ss >> 3; i <= (se >> 3); i++) {
        uint32_t w[4];
        io.ld128(blk + 8u * i, w);
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            const uint32_t z = i * 8u + j;
            if (z < ss || z > se) continue;
            f(z, (int32_t)(int16_t)((w[j >> 1] >> (16u * (j & 1u))) & 0xffffu));
        }
    }
}
template <class IO> JDA_HD void jda_pe_classify(const jda_pe_arrays &A, const jda_pe_seg &S, const jda_encode_dev_job &J, uint32_t u, IO &io)
{
    if (S.ss == 0u) { io.st32(A.cls + u, 0u); return; }
    const int16_t *blk = A.E.coef + (size_t)jda_pe_block(S, J, u - S.unit0) * 64u;
    const uint32_t al = S.al;
    uint32_t any = 0, last = 0, eob = 0, br = 0;
    jda_pe_band(blk, S.ss, S.se, io, [&](uint32_t z, int32_t v) {
        const uint32_t t = (uint32_t)(v < 0 ? -v : v) >> al;
        any |= t; last = t;
        if (t == 1u) { eob = z; br = 0u; } else if (t > 1u) br++;
    });
    if (!S.ah) io.st32(A.cls + u, (any ? JDA_PE_BREAKER : 0u) | (last == 0u ? JDA_PE_JOINS : 0u));
    else io.st32(A.cls + u, (eob ? JDA_PE_BREAKER : 0u) | (eob < S.se ? JDA_PE_JOINS : 0u) | (br << 8) | (eob << 16));
}
template <class IO> JDA_HD void jda_pe_resolve(const jda_pe_arrays &A, const jda_pe_seg &S, uint32_t u, IO &io)
{
    const uint32_t c = io.ld32(A.cls + u);
    if (!(c & JDA_PE_JOINS)) { io.st32(A.run + u, 0u); return; }
    if (u > S.unit0 && !(c & JDA_PE_BREAKER) && (io.ld32(A.cls + u - 1u) & JDA_PE_JOINS)) return;      // inside a stretch: its first unit's lane writes this word
    const uint32_t stop = S.unit0 + S.n_units;
    uint32_t a = u, n = 0, be = 0;
    bool open = true;
    for (uint32_t v0 = u; open && v0 < stop; v0 += 8u) {              // eight records a step: their loads are in flight together
        uint32_t cw[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) cw[i] = io.ld32(A.cls + (v0 + i < stop ? v0 + i : stop - 1u));
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) {
            const uint32_t v = v0 + i, cv = cw[i];
            if (!open || v >= stop || (v != u && (cv & JDA_PE_BREAKER))) { open = false; continue; }
            const uint32_t off = be;
            be += (cv >> 8) & 63u; n++;
            if (v != a) io.st32(A.run + v, JDA_PE_INRUN | ((v - a) << 10) | off);
            if (n == JDA_PE_MAX_RUN || be > JDA_PE_MAX_BE) {
                io.st32(A.run + a, JDA_PE_INRUN | JDA_PE_HEAD | (n << 10) | be);
                a = v + 1u; n = 0u; be = 0u;
            }
        }
    }
    if (n) io.st32(A.run + a, JDA_PE_INRUN | JDA_PE_HEAD | (n << 10) | be);
}
// a unit's symbols in the order of the file, handed to k.sym(index in the scan's tables or JDA_PE_NO_SYMBOL, extra bits, their number)
// and k.corr(correction bits, first bit highest, their number); tail: the correction bits it hands to its run
template <class IO, class K> JDA_HD void jda_pe_unit(const jda_pe_arrays &A, const jda_pe_seg &S, const jda_encode_dev_job &J, uint32_t u, IO &io, K &k, uint64_t &tail, uint32_t &ntail)
{
    const uint32_t b = jda_pe_block(S, J, u - S.unit0), al = S.al;
    const int16_t *blk = A.E.coef + (size_t)b * 64u;
    tail = 0; ntail = 0;
    if (S.ss == 0u) {
        const int32_t dc = (int32_t)(int16_t)(io.ld32((const uint32_t *)blk) & 0xffffu);
        if (S.ah) { k.sym(JDA_PE_NO_SYMBOL, (uint32_t)(dc >> al) & 1u, 1u); return; }
        const uint32_t s = b - J.block0, m = s / J.bpm, q = s - m * J.bpm, nl = J.hs * J.vs;
        int32_t pred = 0;                                              // the block before it of its component, dummies included (they carry a DC)
        if (q < nl && q > 0u) pred = (int32_t)(int16_t)(io.ld32((const uint32_t *)(blk - 64)) & 0xffffu);
        else if (m > 0u) pred = (int32_t)(int16_t)(io.ld32((const uint32_t *)(blk - (size_t)(q < nl ? J.bpm - nl + 1u : J.bpm) * 64u)) & 0xffffu);
        const int32_t diff = (dc >> al) - (pred >> al);
        const uint32_t cat = jda_en_nbits((uint32_t)(diff < 0 ? -diff : diff));
        k.sym((q < nl ? 0u : 16u) + cat, (uint32_t)(diff < 0 ? diff - 1 : diff), cat);
        return;
    }
    uint32_t r = 0, nbr = 0;
    uint64_t br = 0;
    if (!S.ah) {
        jda_pe_band(blk, S.ss, S.se, io, [&](uint32_t, int32_t v) {
            const uint32_t t = (uint32_t)(v < 0 ? -v : v) >> al;
            if (!t) { r++; return; }
            for (; r > 15u; r -= 16u) k.sym(0xf0u, 0u, 0u);
            const uint32_t sz = jda_en_nbits(t);
            k.sym((r << 4) | sz, v < 0 ? ~t : t, sz);
            r = 0u;
        });
    } else {
        const uint32_t eob = (io.ld32(A.cls + u) >> 16) & 63u;
        jda_pe_band(blk, S.ss, S.se, io, [&](uint32_t z, int32_t v) {
            const uint32_t t = (uint32_t)(v < 0 ? -v : v) >> al;
            if (!t) { r++; return; }
            while (r > 15u && z <= eob) {
                k.sym(0xf0u, 0u, 0u);
                r -= 16u;
                if (nbr) { k.corr(br, nbr); br = 0; nbr = 0u; }
            }
            if (t > 1u) { br = (br << 1) | (t & 1u); nbr++; return; }
            k.sym((r << 4) | 1u, v < 0 ? 0u : 1u, 1u);
            if (nbr) { k.corr(br, nbr); br = 0; nbr = 0u; }
            r = 0u;
        });
    }
    const uint32_t rn = io.ld32(A.run + u);
    if (rn & JDA_PE_HEAD) {
        const uint32_t len = (rn >> 10) & 0x7fffu, n = jda_en_nbits(len) - 1u;
        k.sym(n << 4, len & ((1u << n) - 1u), n);
    }
    tail = br; ntail = nbr;
}
template <class IO> struct jda_pe_counter {
    IO *io;
    JDA_HD_MEMBER void sym(uint32_t index, uint32_t, uint32_t) { if (index != JDA_PE_NO_SYMBOL) io->lds_add32(index, 1u); }
    JDA_HD_MEMBER void corr(uint64_t, uint32_t) {}
};
template <class IO> struct jda_pe_adder {
    IO *io; const uint32_t *words; uint32_t bits;
    JDA_HD_MEMBER void sym(uint32_t index, uint32_t, uint32_t n) { bits += n + (index != JDA_PE_NO_SYMBOL ? io->ld32(words + index) >> 16 : 0u); }
    JDA_HD_MEMBER void corr(uint64_t, uint32_t n) { bits += n; }
};
template <class IO> JDA_HD void jda_pe_put_long(jda_en_bits<IO> &W, uint64_t bits, uint32_t n)      // n <= 63 bits, the first the highest
{
    while (n) {
        const uint32_t take = n > 16u ? 16u : n;
        jda_en_put(W, (uint32_t)(bits >> (n - take)), take);
        n -= take;
    }
}
template <class IO> struct jda_pe_writer {
    IO *io; const uint32_t *words; jda_en_bits<IO> W;
    JDA_HD_MEMBER void sym(uint32_t index, uint32_t v, uint32_t n)
    {
        if (index != JDA_PE_NO_SYMBOL) { const uint32_t h = io->ld32(words + index); jda_en_put(W, h & 0xffffu, h >> 16); }
        jda_en_put(W, v, n);
    }
    JDA_HD_MEMBER void corr(uint64_t bits, uint32_t n) { jda_pe_put_long(W, bits, n); }
};
template <class IO> JDA_HD void jda_pe_clear(uint32_t tid, IO &io) { for (uint32_t i = tid; i < JDA_PE_TAB_DWORDS; i += JDA_EN_THREADS) io.lds_st32(i, 0u); }
template <class IO> JDA_HD void jda_pe_flush(uint32_t *hist, uint32_t tid, IO &io)
{
    for (uint32_t i = tid; i < JDA_PE_TAB_DWORDS; i += JDA_EN_THREADS) {
        const uint32_t v = io.lds_ld32(i);
        if (v) io.atomic_add(hist + i, v);
    }
}
template <class IO> JDA_HD void jda_pe_count_unit(const jda_pe_arrays &A, const jda_pe_seg &S, const jda_encode_dev_job &J, uint32_t u, IO &io)
{
    jda_pe_counter<IO> k; k.io = &io;
    uint64_t tail; uint32_t ntail;
    jda_pe_unit(A, S, J, u, io, k, tail, ntail);
}
template <class IO> JDA_HD void jda_pe_length(const jda_pe_arrays &A, const jda_pe_seg &S, const jda_encode_dev_job &J, uint32_t u, IO &io)
{
    jda_pe_adder<IO> k; k.io = &io; k.words = A.words + S.tab; k.bits = 0u;
    uint64_t tail; uint32_t ntail;
    jda_pe_unit(A, S, J, u, io, k, tail, ntail);
    const uint32_t rn = S.ss ? io.ld32(A.run + u) : 0u;
    io.st32(A.len + u, k.bits + (rn & JDA_PE_HEAD ? rn & 1023u : 0u));
}
template <class IO> JDA_HD void jda_pe_start(jda_en_bits<IO> &W, const jda_pe_arrays &A, const jda_pe_seg &S, uint64_t bit, IO &io)
{
    const uint64_t p = S.u_off * 8u + bit;
    W.acc = 0; W.n = (uint32_t)(p & 31u); W.dw = (uint32_t *)A.E.u + (p >> 5); W.io = &io;
}
template <class IO> JDA_HD void jda_pe_emit(const jda_pe_arrays &A, const jda_pe_seg &S, const jda_encode_dev_job &J, uint32_t u, IO &io)
{
    jda_pe_writer<IO> k; k.io = &io; k.words = A.words + S.tab;
    const uint64_t end = io.ld64(A.end + u);
    jda_pe_start(k.W, A, S, end - io.ld32(A.len + u), io);
    uint64_t tail; uint32_t ntail;
    jda_pe_unit(A, S, J, u, io, k, tail, ntail);
    if (k.W.n) jda_en_flush(k.W);
    if (ntail) {                                                       // its correction bits, in its run's tail: behind the head's own code and the run's symbol
        const uint32_t rn = io.ld32(A.run + u), a = rn & JDA_PE_HEAD ? u : u - ((rn >> 10) & 0x7fffu);
        const uint32_t off = rn & JDA_PE_HEAD ? 0u : rn & 1023u, be = io.ld32(A.run + a) & 1023u;
        jda_en_bits<IO> T;
        jda_pe_start(T, A, S, io.ld64(A.end + a) - be + off, io);
        jda_pe_put_long(T, tail, ntail);
        if (T.n) jda_en_flush(T);
    }
    if (u + 1u == S.unit0 + S.n_units && (end & 7u)) {                 // the scan's 1-bits to the byte
        jda_en_bits<IO> P;
        jda_pe_start(P, A, S, end, io);
        jda_en_put(P, 0xffu, 8u - (uint32_t)(end & 7u));
        if (P.n) jda_en_flush(P);
    }
}
// a segment's scan of the units' lengths (bytes = false: g = segment) or a job's of its chunks' bytes in the file (g = job)
template <class IO> JDA_HD void jda_pe_scan(const jda_pe_arrays &A, uint32_t g, bool bytes, bool second, uint32_t tid, IO &io)
{
    const uint32_t *vals = bytes ? A.E.ffcnt : A.len;
    const uint32_t first = io.ld32(bytes ? &A.pjobs[g].chunk0 : &A.segs[g].unit0), n = io.ld32(bytes ? &A.pjobs[g].n_chunks : &A.segs[g].n_units);
    if (!second) { jda_en_scan_local(vals, 0xffffffffu, first, n, 0u, tid, io); return; }
    const uint64_t p = jda_en_scan_write(vals, 0xffffffffu, first, n, 0u, bytes ? A.E.ffend : A.end, (uint64_t *)0, tid, io);
    if (p == ~(uint64_t)0) return;
    if (!bytes) io.st64(A.sbytes + g, jda_en_ceil8(p) >> 3);
    else io.st64(&A.E.totals[g].file_bytes, p + 2u);
}
// a chunk's bytes in the file: a header chunk's as they are, a data chunk's and a zero behind every 0xFF
template <class IO> JDA_HD void jda_pe_count(const jda_pe_arrays &A, const jda_pe_seg &S, uint32_t si, uint32_t c, IO &io)
{
    const uint32_t local = c - S.chunk0;
    uint32_t cnt;
    if (local < S.h_chunks) cnt = S.hdr_len - local * JDA_EN_CHUNK < JDA_EN_CHUNK ? S.hdr_len - local * JDA_EN_CHUNK : JDA_EN_CHUNK;
    else {
        const uint64_t p0 = (uint64_t)(local - S.h_chunks) * JDA_EN_CHUNK, left = io.ld64(A.sbytes + si) - p0;
        cnt = left < JDA_EN_CHUNK ? (uint32_t)left : JDA_EN_CHUNK;
        const uint8_t *p = A.E.u + S.u_off + p0;
        for (uint32_t i = 0; i < JDA_EN_CHUNK / 16u; i++) {            // (behind the scan's last byte: zeros)
            uint32_t w[4];
            io.ld128(p + 16u * i, w);
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++) cnt += ((w[j >> 2] >> (8u * (j & 3u))) & 0xffu) == 0xffu ? 1u : 0u;
        }
    }
    io.st32(A.E.ffcnt + c, cnt);
}
template <class IO> JDA_HD void jda_pe_write(const jda_pe_arrays &A, const jda_pe_seg &S, const jda_encode_dev_job &J, uint32_t si, uint32_t c, IO &io)
{
    const uint64_t fb = io.ld64(&A.E.totals[S.job].file_bytes);
    if (fb > J.capacity) return;                                       // the file does not fit: no byte of it is written
    const uint32_t local = c - S.chunk0;
    uint8_t *q = J.dst + (io.ld64(A.E.ffend + c) - io.ld32(A.E.ffcnt + c));
    if (local < S.h_chunks) {
        const uint32_t o = local * JDA_EN_CHUNK, left = S.hdr_len - o < JDA_EN_CHUNK ? S.hdr_len - o : JDA_EN_CHUNK;
        for (uint32_t i = 0; i < left; i++) io.st8(q++, io.ld8(A.hdr + S.hdr_off + o + i));
    } else {
        const uint64_t p0 = (uint64_t)(local - S.h_chunks) * JDA_EN_CHUNK, sb = io.ld64(A.sbytes + si);
        const uint8_t *src = A.E.u + S.u_off + p0;
        for (uint32_t i = 0; i < JDA_EN_CHUNK / 16u; i++) {
            if (p0 + 16u * i >= sb) break;
            uint32_t w[4];
            io.ld128(src + 16u * i, w);
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++) {
                if (p0 + 16u * i + j >= sb) continue;
                const uint32_t v = (w[j >> 2] >> (8u * (j & 3u))) & 0xffu;
                io.st8(q++, v);
                if (v == 0xffu) io.st8(q++, 0u);
            }
        }
    }
    const uint32_t jc0 = io.ld32(&A.pjobs[S.job].chunk0), jcn = io.ld32(&A.pjobs[S.job].n_chunks);
    if (c + 1u == jc0 + jcn) { io.st8(J.dst + fb - 2u, 0xffu); io.st8(J.dst + fb - 1u, 0xd9u); }
}

// ================================================================================================
// jda_rc_*: the coefficients of a compressed file in the place of the blocks stage (lossless recode).  A lane = a block
// of the call's flat list, which is the source's own block order (the order of its scan).  Two stages, a kernel each:
//   extract    the source is a resident baseline image: the lane reads the block's index entry and DC value (index format 2) and walks the
//              AC symbols from the entry's BIT POSITION through the image's AC LUT for the block's component (the table blob's layout in
//              HBM: (length << 8) | RS, found by an 11-bit key) into its slot in LDS: 64 x int16, unscaled, in zig-zag order.  The values
//              are T.81's EXTEND of whole magnitudes -- the reader peeks 32 bits at any bit position, so the reference's un-refilled window
//              (JDA_INDEX_TRUNC) has no part in it and the entry's phase is not looked at.  The wavefront then stores its
//              slots with whole 128-bit stores, 64 lanes 8 consecutive blocks an instruction (jda_rc_store).
//   from_coef  the source is a resident dense coefficient image: natural order -> zig-zag in registers, the indices constants.
// Both leave what jda_en_block leaves: the coefficients and the block's word (AC code bits under the Annex K table of its class << 16 | DC).
// No block of a source is a dummy: every block of the MCU grid carries the source's own coefficients.  A block with an |AC| above 1023 or
// a DC outside -1024 .. 1023 raises its job's word in `bad` (the job is refused) and is clamped, so that the stages behind see legal values.
// A slot is JDA_COEF_STRIDE bytes, the decode kernel's padding: lanes l and l + 32 share a bank where a stride of 128 would put all 64 on one.
#define JDA_RC_SLOT_VALID 128u             // byte offset in a slot: != 0: the lane decoded a block into it
template <class IO> JDA_HD uint32_t jda_rc_peek(const jda_rc_src &S, uint32_t p, IO &io)      // the 32 bits of the scan from bit p on
{
    // (the scan section is scan_len + JDA_SCAN_PAD bytes: both dwords stay inside whatever an entry says)
    const uint32_t a_max = (S.scan_len + JDA_SCAN_PAD - 8u) >> 2;
    uint32_t a = p >> 5;
    a = a < a_max ? a : a_max;
    const uint32_t *w = (const uint32_t *)S.scan + a;
    const uint32_t d0 = __builtin_bswap32(io.ld32(w)), d1 = __builtin_bswap32(io.ld32(w + 1u)), sh = p & 31u;
    return sh ? (d0 << sh) | (d1 >> (32u - sh)) : d0;
}
JDA_HD uint32_t jda_rc_comp(const jda_encode_dev_job &J, uint32_t s)      // the component of block s of a job
{
    const uint32_t k = s % J.bpm, nl = J.hs * J.vs;
    return k < nl ? 0u : 1u + k - nl;
}
// the code bits of an AC value behind `run` zeros, as jda_en_block counts them
template <class IO> JDA_HD uint32_t jda_rc_ac_bits(const uint32_t *ac, uint32_t run, uint32_t a, IO &io)
{
    return (run >> 4) * (io.ld32(ac + 0xf0u) >> 16) + (io.ld32(ac + (((run & 15u) << 4) | jda_en_nbits(a))) >> 16) + jda_en_nbits(a);
}
template <class IO> JDA_HD void jda_rc_extract_block(const jda_en_arrays &A, const jda_encode_dev_job &J, const jda_rc_src &S, uint32_t job, uint32_t b, uint8_t *slot,
                                                     uint32_t *bad, IO &io)
{
    const uint32_t s = b - J.block0, c = jda_rc_comp(J, s), t = c ? 1u : 0u;
    int16_t *coef = (int16_t *)slot;
    jda_u64_alias *z8 = (jda_u64_alias *)slot;
#pragma unroll
    for (int i = 0; i < 16; i++) z8[i] = 0;
    const uint32_t ix = io.ld32(S.blk_index + s);
    const uint32_t dcw = io.ld32((const uint32_t *)S.blk_dc + (s >> 1));
    int32_t dc = (int32_t)(int16_t)((s & 1u) ? dcw >> 16 : dcw & 0xffffu);
    bool wrong = dc < JDA_RC_MIN_DC || dc > JDA_RC_MAX_DC;
    dc = dc < JDA_RC_MIN_DC ? JDA_RC_MIN_DC : dc > JDA_RC_MAX_DC ? JDA_RC_MAX_DC : dc;
    coef[0] = (int16_t)dc;
    uint32_t p = (ix >> JDA_INDEX_OFF_BITS) * 8u + (ix & (JDA_INDEX_TRUNC - 1u));
    const uint32_t *lut = (const uint32_t *)(S.tables + JDA_TB_AC + (S.ac_id[c] & 1u) * 4096u);
    const uint32_t *ac = A.huff + t * 256u;
    uint32_t bits = 0, z = 1, last = 0;
    while (z < 64u) {
        const uint32_t w = jda_rc_peek(S, p, io);
        const uint32_t key = w >= 0xfc000000u ? 1024u + ((w >> 16) & 0x3ffu) : w >> 22;
        const uint32_t pair = io.ld32(lut + (key >> 1)), raw = (key & 1u) ? pair >> 16 : pair & 0xffffu;
        const uint32_t len = raw >> 8, rs = raw & 0xffu, sz = rs & 15u;
        if (len == 0u || rs == 0u) break;                                // no such code, or EOB
        z += rs >> 4;
        if (sz && z < 64u) {
            const uint32_t m = w << len, v = m >> (32u - sz);
            int32_t val = (m & 0x80000000u) ? (int32_t)v : (int32_t)v - (int32_t)((1u << sz) - 1u);       // T.81 F.2.2.1 EXTEND
            uint32_t a = (uint32_t)(val < 0 ? -val : val);
            if (a > (uint32_t)JDA_RC_MAX_AC) { wrong = true; a = JDA_RC_MAX_AC; val = val < 0 ? -JDA_RC_MAX_AC : JDA_RC_MAX_AC; }
            coef[z] = (int16_t)val;
            bits += jda_rc_ac_bits(ac, z - last - 1u, a, io);
            last = z;
        }
        p += len + sz;
        z++;
    }
    if (last < 63u) bits += io.ld32(ac) >> 16;
    io.st32(A.meta + b, (bits << 16) | ((uint32_t)dc & 0xffffu));
    if (wrong) io.atomic_or(bad + job, 1u);
}
// the wavefront's slots (its first block: b0) to the call's coefficients: chunk i * 64 + lane of the 512 16-byte chunks of 64 blocks
template <class IO> JDA_HD void jda_rc_store(const jda_en_arrays &A, uint32_t b0, const uint8_t *slots, uint32_t lane, IO &io)
{
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) {
        const uint32_t ch = i * 64u + lane, blk = ch >> 3, part = ch & 7u;
        const uint8_t *slot = slots + blk * JDA_COEF_STRIDE;
        if (*(const jda_u32_alias *)(slot + JDA_RC_SLOT_VALID) == 0u) continue;
        const jda_u64_alias *q = (const jda_u64_alias *)(slot + part * 16u);
        const uint64_t lo = q[0], hi = q[1];
        const uint32_t w[4] = { (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32) };
        io.st128(A.coef + (size_t)(b0 + blk) * 64u + part * 8u, w);
    }
}
template <class IO> JDA_HD void jda_rc_coef_block(const jda_en_arrays &A, const jda_encode_dev_job &J, const jda_rc_src &S, uint32_t job, uint32_t b, uint32_t *bad, IO &io)
{
    const uint32_t s = b - J.block0, t = jda_rc_comp(J, s) ? 1u : 0u;
    const int16_t *in = S.coef + (size_t)s * 64u;
    uint32_t n[32], w[32];
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) io.ld128(in + 8u * i, n + 4u * i);
    const uint32_t *ac = A.huff + t * 256u;
    uint32_t bits = 0, run = 0, dcw = 0;
    bool wrong = false;
#pragma unroll
    for (uint32_t z = 0; z < 64u; z++) {
        const uint32_t k = jda_en_zigzag(z);
        int32_t v = (int32_t)(int16_t)((k & 1u) ? n[k >> 1] >> 16 : n[k >> 1] & 0xffffu);
        if (z == 0u) {
            if (v < JDA_RC_MIN_DC || v > JDA_RC_MAX_DC) { wrong = true; v = v < JDA_RC_MIN_DC ? JDA_RC_MIN_DC : JDA_RC_MAX_DC; }
            dcw = (uint32_t)v & 0xffffu;
        } else {
            uint32_t a = (uint32_t)(v < 0 ? -v : v);
            if (a > (uint32_t)JDA_RC_MAX_AC) { wrong = true; a = JDA_RC_MAX_AC; v = v < 0 ? -JDA_RC_MAX_AC : JDA_RC_MAX_AC; }
            if (a == 0u) run++;
            else { bits += jda_rc_ac_bits(ac, run, a, io); run = 0; }
        }
        const uint32_t val = (uint32_t)v & 0xffffu;
        if (z & 1u) w[z >> 1] |= val << 16; else w[z >> 1] = val;
    }
    if (run) bits += io.ld32(ac) >> 16;
    int16_t *out = A.coef + (size_t)b * 64u;
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) io.st128(out + 8u * i, w + 4u * i);
    io.st32(A.meta + b, (bits << 16) | dcw);
    if (wrong) io.atomic_or(bad + job, 1u);
}

// ------------------------------------------------------------------------------------------------
// jda_rc_*_xf: the same two stages with every block put at another place, its coefficients permuted and sign-flipped (lossless flip,
// rotate, transpose and MCU crop).  A lane = a block of the job's REGION (jda_rc_xf) in the SOURCE's scan order, so the
// index, DC and scan reads are as local as in jda_rc_extract; the lane works out where its block goes in the target's scan order
// (jda_rc_xf_map) and the block -- 128 bytes, a cache line -- is written there whole.  In zig-zag order a transposition keeps a coefficient
// on its anti-diagonal and reverses its place there (jda_rc_tz); a mirrored target axis negates the coefficients of odd frequency along it,
// which are fixed zig-zag positions of the SOURCE block (JDA_RC_ODD_U / _V: bit z).  DC never changes.
#define JDA_RC_ODD_U 0xB56AAD55554AA952ull  // zig-zag positions of odd horizontal frequency
#define JDA_RC_ODD_V 0xD6AB555AA5552A94ull  // .. of odd vertical frequency: JDA_RC_ODD_U under jda_rc_tz
JDA_HD uint32_t jda_rc_tz(uint32_t z)       // the zig-zag position of the transposed coefficient of zig-zag position z
{
    constexpr uint8_t tz[64] = { 0, 2, 1, 5, 4, 3, 9, 8, 7, 6, 14, 13, 12, 11, 10, 20, 19, 18, 17, 16, 15, 27, 26, 25, 24, 23, 22, 21, 35, 34, 33, 32,
                                 31, 30, 29, 28, 42, 41, 40, 39, 38, 37, 36, 48, 47, 46, 45, 44, 43, 53, 52, 51, 50, 49, 57, 56, 55, 54, 60, 59, 58, 62, 61, 63 };
    return tz[z];
}
// the zig-zag positions of a SOURCE block whose coefficients a job negates
JDA_HD uint64_t jda_rc_xf_neg(uint32_t bits)
{
    const bool t = (bits & JDA_RC_XF_T) != 0u, mx = (bits & JDA_RC_XF_MX) != 0u, my = (bits & JDA_RC_XF_MY) != 0u;
    return ((t ? my : mx) ? JDA_RC_ODD_U : 0ull) ^ ((t ? mx : my) ? JDA_RC_ODD_V : 0ull);       // (transposed: the target's x is the source's y)
}
// block r of a job's region: *s = its index in the source's scan order, the return value its index in the target's
JDA_HD uint32_t jda_rc_xf_map(const jda_encode_dev_job &J, const jda_rc_xf &X, uint32_t r, uint32_t *s)
{
    const uint32_t m = r / J.bpm, k = r - m * J.bpm, nl = J.hs * J.vs;
    const uint32_t my = m / X.rw, mx = m - my * X.rw;
    *s = ((X.y0 + my) * X.scx + X.x0 + mx) * J.bpm + k;
    const bool luma = k < nl;
    uint32_t tx = mx, ty = my, kx = luma ? k % J.hs : 0u, ky = luma ? k / J.hs : 0u;
    if (X.bits & JDA_RC_XF_T) { uint32_t q = tx; tx = ty; ty = q; q = kx; kx = ky; ky = q; }
    if (X.bits & JDA_RC_XF_MX) { tx = J.cx - 1u - tx; if (luma) kx = J.hs - 1u - kx; }
    if (X.bits & JDA_RC_XF_MY) { ty = J.cy - 1u - ty; if (luma) ky = J.vs - 1u - ky; }
    return (ty * J.cx + tx) * J.bpm + (luma ? ky * J.hs + kx : k);
}
// the AC code bits of a finished block in the lane's slot, in the target's zig-zag order, four coefficients a read
template <class IO> JDA_HD uint32_t jda_rc_slot_bits(const uint32_t *ac, const uint8_t *slot, IO &io)
{
    const jda_u64_alias *z8 = (const jda_u64_alias *)slot;
    uint32_t bits = 0, run = 0;
    for (uint32_t q = 0; q < 16u; q++) {
        uint64_t w = z8[q];
        if (q == 0u) w &= ~0xffffull;                                     // (the DC value is no part of a run)
        if (w == 0ull) { run += q ? 4u : 3u; continue; }
        for (uint32_t j = q ? 0u : 1u; j < 4u; j++) {
            const int32_t v = (int32_t)(int16_t)(w >> (16u * j));
            if (v == 0) { run++; continue; }
            bits += jda_rc_ac_bits(ac, run, (uint32_t)(v < 0 ? -v : v), io);
            run = 0;
        }
    }
    if (run) bits += io.ld32(ac) >> 16;
    return bits;
}
// the lane's block into its slot, as jda_rc_extract_block; the return value: the block's index in the call's flat list
template <class IO> JDA_HD uint32_t jda_rc_extract_block_xf(const jda_en_arrays &A, const jda_encode_dev_job &J, const jda_rc_src &S, const jda_rc_xf &X, uint32_t job, uint32_t b,
                                                            uint8_t *slot, uint32_t *bad, IO &io)
{
    uint32_t s;
    const uint32_t d = J.block0 + jda_rc_xf_map(J, X, b - J.block0, &s), c = jda_rc_comp(J, s), t = c ? 1u : 0u;
    const bool tr = (X.bits & JDA_RC_XF_T) != 0u;
    const uint64_t neg = jda_rc_xf_neg(X.bits);
    int16_t *coef = (int16_t *)slot;
    jda_u64_alias *z8 = (jda_u64_alias *)slot;
#pragma unroll
    for (int i = 0; i < 16; i++) z8[i] = 0;
    const uint32_t ix = io.ld32(S.blk_index + s);
    const uint32_t dcw = io.ld32((const uint32_t *)S.blk_dc + (s >> 1));
    int32_t dc = (int32_t)(int16_t)((s & 1u) ? dcw >> 16 : dcw & 0xffffu);
    bool wrong = dc < JDA_RC_MIN_DC || dc > JDA_RC_MAX_DC;
    dc = dc < JDA_RC_MIN_DC ? JDA_RC_MIN_DC : dc > JDA_RC_MAX_DC ? JDA_RC_MAX_DC : dc;
    coef[0] = (int16_t)dc;
    uint32_t p = (ix >> JDA_INDEX_OFF_BITS) * 8u + (ix & (JDA_INDEX_TRUNC - 1u));
    const uint32_t *lut = (const uint32_t *)(S.tables + JDA_TB_AC + (S.ac_id[c] & 1u) * 4096u);
    uint32_t z = 1;
    while (z < 64u) {
        const uint32_t w = jda_rc_peek(S, p, io);
        const uint32_t key = w >= 0xfc000000u ? 1024u + ((w >> 16) & 0x3ffu) : w >> 22;
        const uint32_t pair = io.ld32(lut + (key >> 1)), raw = (key & 1u) ? pair >> 16 : pair & 0xffffu;
        const uint32_t len = raw >> 8, rs = raw & 0xffu, sz = rs & 15u;
        if (len == 0u || rs == 0u) break;                                // no such code, or EOB
        z += rs >> 4;
        if (sz && z < 64u) {
            const uint32_t m = w << len, v = m >> (32u - sz);
            int32_t val = (m & 0x80000000u) ? (int32_t)v : (int32_t)v - (int32_t)((1u << sz) - 1u);       // T.81 F.2.2.1 EXTEND
            if (val > JDA_RC_MAX_AC || val < -JDA_RC_MAX_AC) { wrong = true; val = val < 0 ? -JDA_RC_MAX_AC : JDA_RC_MAX_AC; }
            if ((neg >> z) & 1ull) val = -val;
            coef[tr ? jda_rc_tz(z) : z] = (int16_t)val;
        }
        p += len + sz;
        z++;
    }
    const uint32_t bits = jda_rc_slot_bits(A.huff + t * 256u, slot, io);
    io.st32(A.meta + d, (bits << 16) | ((uint32_t)dc & 0xffffu));
    if (wrong) io.atomic_or(bad + job, 1u);
    return d;
}
// the wavefront's slots to the call's coefficients, as jda_rc_store: a slot's word at JDA_RC_SLOT_VALID is its block's index in the flat
// list + 1 (0: no block), and eight consecutive lanes write the block's line
template <class IO> JDA_HD void jda_rc_store_xf(const jda_en_arrays &A, const uint8_t *slots, uint32_t lane, IO &io)
{
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) {
        const uint32_t ch = i * 64u + lane, blk = ch >> 3, part = ch & 7u;
        const uint8_t *slot = slots + blk * JDA_COEF_STRIDE;
        const uint32_t tag = *(const jda_u32_alias *)(slot + JDA_RC_SLOT_VALID);
        if (tag == 0u) continue;
        const jda_u64_alias *q = (const jda_u64_alias *)(slot + part * 16u);
        const uint64_t lo = q[0], hi = q[1];
        const uint32_t w[4] = { (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32) };
        io.st128(A.coef + (size_t)(tag - 1u) * 64u + part * 8u, w);
    }
}
template <bool TR, class IO> JDA_HD void jda_rc_coef_block_xf_t(const jda_en_arrays &A, const jda_encode_dev_job &J, const jda_rc_src &S, const jda_rc_xf &X, uint32_t job, uint32_t b,
                                                                uint32_t *bad, IO &io)
{
    uint32_t s;
    const uint32_t d = J.block0 + jda_rc_xf_map(J, X, b - J.block0, &s), t = jda_rc_comp(J, s) ? 1u : 0u;
    const bool mx = (X.bits & JDA_RC_XF_MX) != 0u, my = (X.bits & JDA_RC_XF_MY) != 0u;
    const bool su = TR ? my : mx, sv = TR ? mx : my;                      // the SOURCE's odd u / odd v are negated
    const int16_t *in = S.coef + (size_t)s * 64u;
    uint32_t n[32], w[32];
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) io.ld128(in + 8u * i, n + 4u * i);
    const uint32_t *ac = A.huff + t * 256u;
    uint32_t bits = 0, run = 0, dcw = 0;
    bool wrong = false;
#pragma unroll
    for (uint32_t z = 0; z < 64u; z++) {
        const uint32_t kt = jda_en_zigzag(z), k = TR ? ((kt & 7u) << 3) | (kt >> 3) : kt;      // target natural index, source natural index
        int32_t v = (int32_t)(int16_t)((k & 1u) ? n[k >> 1] >> 16 : n[k >> 1] & 0xffffu);
        if (z == 0u) {
            if (v < JDA_RC_MIN_DC || v > JDA_RC_MAX_DC) { wrong = true; v = v < JDA_RC_MIN_DC ? JDA_RC_MIN_DC : JDA_RC_MAX_DC; }
            dcw = (uint32_t)v & 0xffffu;
        } else {
            uint32_t a = (uint32_t)(v < 0 ? -v : v);
            if (a > (uint32_t)JDA_RC_MAX_AC) { wrong = true; a = JDA_RC_MAX_AC; v = v < 0 ? -JDA_RC_MAX_AC : JDA_RC_MAX_AC; }
            if ((k & 1u) && su) v = -v;
            if ((k & 8u) && sv) v = -v;
            if (a == 0u) run++;
            else { bits += jda_rc_ac_bits(ac, run, a, io); run = 0; }
        }
        const uint32_t val = (uint32_t)v & 0xffffu;
        if (z & 1u) w[z >> 1] |= val << 16; else w[z >> 1] = val;
    }
    if (run) bits += io.ld32(ac) >> 16;
    int16_t *out = A.coef + (size_t)d * 64u;
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) io.st128(out + 8u * i, w + 4u * i);
    io.st32(A.meta + d, (bits << 16) | dcw);
    if (wrong) io.atomic_or(bad + job, 1u);
}
template <class IO> JDA_HD void jda_rc_coef_block_xf(const jda_en_arrays &A, const jda_encode_dev_job &J, const jda_rc_src &S, const jda_rc_xf &X, uint32_t job, uint32_t b,
                                                     uint32_t *bad, IO &io)
{
    if (X.bits & JDA_RC_XF_T) jda_rc_coef_block_xf_t<true>(A, J, S, X, job, b, bad, io);
    else jda_rc_coef_block_xf_t<false>(A, J, S, X, job, b, bad, io);
}

// ================================================================================================
// jda_ex_*: the libjpeg-exact decode: the coefficients of a coefficient image through libjpeg's own arithmetic -- the
// RAW DQT entries, jidctint.c's islow IDCT, "fancy" chroma upsampling, jdcolor.c's constants -- so that the pixels are Pillow's, not the
// reference's.  The definition is stated once more in numpy (tests/exact_util.py).  Two stages, a kernel each:
//   planes   the decode's tile (one wave64, <= 64 consecutive blocks of an MCU row) behind a load phase by source: the coefficient kernels'
//            (jda_ct_load, or jda_cs_zero + jda_cs_scatter, as they stand; the chunk words they leave are not looked at), or, for a
//            resident baseline image, jda_ex_load_baseline (below).  lane = block:
//            its 64 coefficients from its LDS slot (sixteen 8-byte reads: a slot is 8-byte aligned), times the raw quantisers of its component (the wavefront's copy
//            in LDS: JDA_EX_QUANT_BYTES), the column pass into a workspace of 64 registers, the row pass, the range limit, eight 8-byte
//            stores into the component's plane in the call's scratch.  Every multiply by an IDCT constant is a full 32-bit one: the
//            arithmetic is defined modulo 2^32 for ANY int16 coefficients (a coefficient image's are the caller's), where a 24-bit
//            multiplier would need a bound on them that nothing checks.  The dequantisation (int16 x uint16) is exact in 24 bits.
//   colour   lane = four output pixels of a row = one 16-byte store (RGB8888; four bytes of a gray surface): the Y bytes and the chroma
//            neighbours the upsampling formulas name, read from the planes in HBM with the indices clamped to the component's OWN extent
//            -- the edge sample replicated, the MCU padding never read --, then the colour conversion.  A tile is a record of the same
//            list as the planes stage's: count MCUs of an MCU row, its rows walked 64 quads at a time.
// IO: ld128 / ld32u as the coefficient kernels'; ld32(base, byte offset), ld8(base, byte offset); st64 / st128 / st32 / st8(base, byte
// offset, ..) -- global memory, the offsets below 2^32 (jda_exact_plan.h checks the planes, jda_fill_launch_desc the surface).
#define JDA_EX_QUANT_BYTES 384u             // 3 x 64 uint16, natural order
template <int MODE> struct jda_ex_layout {
    enum { WAVE_BYTES = (JDA_EX_QUANT_BYTES + jda_lds_layout<MODE>::BASE_BYTES + 15) / 16 * 16,
           HS = (MODE == JDA_MODE_420 || MODE == JDA_MODE_422) ? 2 : 1, VS = (MODE == JDA_MODE_420 || MODE == JDA_MODE_440) ? 2 : 1 };
};

// the wavefront's copy of the image's raw quantisers: 96 dwords
template <class IO> JDA_HD void jda_ex_tables(IO &io, const jda_ex_desc *X, uint32_t lane, uint8_t *qt)
{
    jda_u32_alias *dst = (jda_u32_alias *)qt;
    dst[lane] = io.ld32(&X->quant[0][0], 4u * lane);
    if (lane < JDA_EX_QUANT_BYTES / 4u - 64u) dst[64u + lane] = io.ld32(&X->quant[0][0], 4u * (64u + lane));
}

// one pass of jidctint.c's jpeg_idct_islow over eight values, in place: DESCALE by SHIFT (CONST_BITS - PASS1_BITS = 11 for the columns,
// CONST_BITS + PASS1_BITS + 3 = 18 for the rows); unsigned arithmetic where a sum may wrap, as the definition's 32-bit integers do
template <int SHIFT> JDA_HD void jda_ex_idct8(int32_t &d0, int32_t &d1, int32_t &d2, int32_t &d3, int32_t &d4, int32_t &d5, int32_t &d6, int32_t &d7)
{
    typedef uint32_t U;
    const U R = 1u << (SHIFT - 1);
    const U z1e = ((U)d2 + (U)d6) * 4433u;
    const U t2e = z1e - (U)d6 * 15137u, t3e = z1e + (U)d2 * 6270u;
    const U t0e = ((U)d0 + (U)d4) << 13, t1e = ((U)d0 - (U)d4) << 13;
    const U t10 = t0e + t3e, t13 = t0e - t3e, t11 = t1e + t2e, t12 = t1e - t2e;
    const U z1 = (U)d7 + (U)d1, z2 = (U)d5 + (U)d3, z3 = (U)d7 + (U)d3, z4 = (U)d5 + (U)d1;
    const U z5 = (z3 + z4) * 9633u;
    const U m1 = 0u - z1 * 7373u, m2 = 0u - z2 * 20995u, m3 = z5 - z3 * 16069u, m4 = z5 - z4 * 3196u;
    const U t0 = (U)d7 * 2446u + m1 + m3, t1 = (U)d5 * 16819u + m2 + m4, t2 = (U)d3 * 25172u + m2 + m3, t3 = (U)d1 * 12299u + m1 + m4;
    d0 = (int32_t)(t10 + t3 + R) >> SHIFT; d7 = (int32_t)(t10 - t3 + R) >> SHIFT;
    d1 = (int32_t)(t11 + t2 + R) >> SHIFT; d6 = (int32_t)(t11 - t2 + R) >> SHIFT;
    d2 = (int32_t)(t12 + t1 + R) >> SHIFT; d5 = (int32_t)(t12 - t1 + R) >> SHIFT;
    d3 = (int32_t)(t13 + t0 + R) >> SHIFT; d4 = (int32_t)(t13 - t0 + R) >> SHIFT;
}
// libjpeg's range limit behind the IDCT: the table's index is x & 1023 -- clamp(x + 128) for x in -512 .. 511, wrapping outside
JDA_HD uint32_t jda_ex_limit(int32_t x)
{
    const uint32_t i = (uint32_t)x & 1023u;
    return i < 128u ? i + 128u : i < 512u ? 255u : i < 896u ? 0u : i - 896u;
}

// lane = block of the tile, behind the load phase.  wl: the wavefront's slots, qt: its quantisers
template <int MODE, class IO>
JDA_HD void jda_ex_block(IO &io, const jda_ex_desc &X, const jda_strip &S, const jda_tile_ctx &C, uint32_t lane, const uint8_t *wl, const uint8_t *qt)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    typedef jda_ex_layout<MODE> E;
    if (lane >= C.count * (uint32_t)T::NBLK) return;
    const uint32_t k = lane % (uint32_t)T::NBLK, m = lane / (uint32_t)T::NBLK;
    const uint32_t c = k < (uint32_t)T::NLUMA ? 0u : k - (uint32_t)T::NLUMA + 1u;
    if (c && X.luma_only) return;
    const jda_u64_alias *src = (const jda_u64_alias *)(wl + L::COEF_OFF + lane * JDA_COEF_STRIDE);
    const jda_u64_alias *qs = (const jda_u64_alias *)(qt + c * 128u);
    int32_t ws[64];
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) {                     // four coefficients and their quantisers a step
        const uint64_t v = src[i], q = qs[i];
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++)
            ws[4u * i + j] = jda_mulc<true>((int32_t)(int16_t)(uint16_t)(v >> (16u * j)), (int32_t)(uint16_t)(q >> (16u * j)));
    }
#pragma unroll
    for (uint32_t x = 0; x < 8u; x++)
        jda_ex_idct8<11>(ws[x], ws[8 + x], ws[16 + x], ws[24 + x], ws[32 + x], ws[40 + x], ws[48 + x], ws[56 + x]);
    uint32_t bx, by, pitch;
    if (c == 0u) { bx = (S.mcu_x0 + m) * (uint32_t)E::HS + k % (uint32_t)E::HS; by = S.mcu_y * (uint32_t)E::VS + k / (uint32_t)E::HS; pitch = X.pitch_y; }
    else { bx = S.mcu_x0 + m; by = S.mcu_y; pitch = X.pitch_c; }
    uint8_t *plane = c == 0u ? X.plane[0] : c == 1u ? X.plane[1] : X.plane[2];
    uint32_t off = by * 8u * pitch + bx * 8u;
#pragma unroll
    for (uint32_t y = 0; y < 8u; y++) {
        jda_ex_idct8<18>(ws[8 * y], ws[8 * y + 1], ws[8 * y + 2], ws[8 * y + 3], ws[8 * y + 4], ws[8 * y + 5], ws[8 * y + 6], ws[8 * y + 7]);
        const uint32_t lo = jda_ex_limit(ws[8 * y]) | (jda_ex_limit(ws[8 * y + 1]) << 8) | (jda_ex_limit(ws[8 * y + 2]) << 16) | (jda_ex_limit(ws[8 * y + 3]) << 24);
        const uint32_t hi = jda_ex_limit(ws[8 * y + 4]) | (jda_ex_limit(ws[8 * y + 5]) << 8) | (jda_ex_limit(ws[8 * y + 6]) << 16) | (jda_ex_limit(ws[8 * y + 7]) << 24);
        io.st64(plane, off, lo, hi);
        off += pitch;
    }
}

// jdcolor.c, SCALEBITS 16: the pixel as a dword, R in the lowest byte, A = 0xFF
JDA_HD uint32_t jda_ex_rgba(uint32_t y, uint32_t cbs, uint32_t crs)
{
    const int32_t cb = (int32_t)cbs - 128, cr = (int32_t)crs - 128, Y = (int32_t)y;
    int32_t r = Y + ((91881 * cr + 32768) >> 16);
    int32_t g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    int32_t b = Y + ((116130 * cb + 32768) >> 16);
    r = r < 0 ? 0 : r > 255 ? 255 : r; g = g < 0 ? 0 : g > 255 ? 255 : g; b = b < 0 ? 0 : b > 255 ? 255 : b;
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | 0xff000000u;
}
// the four upsampled samples of a chroma plane under the output pixels x0 .. x0 + 3 (x0 a multiple of 4) of output row y
template <int MODE, class IO> JDA_HD void jda_ex_chroma4(IO &io, const jda_ex_desc &X, const uint8_t *plane, uint32_t x0, uint32_t y, uint32_t *out)
{
    typedef jda_ex_layout<MODE> E;
    const uint32_t j = E::VS == 2 ? y >> 1 : y;
    // the second row of a vertical pair: the one above for an even output row, the one below for an odd one, inside the component's extent
    const uint32_t jn = E::VS == 2 ? ((y & 1u) ? (j + 1u < X.ch ? j + 1u : j) : (j ? j - 1u : 0u)) : j;
    if (E::HS == 1) {
        const uint32_t a = io.ld32(plane, j * X.pitch_c + x0);
        if (E::VS == 1) { for (uint32_t k = 0; k < 4u; k++) out[k] = (a >> (8u * k)) & 255u; return; }
        const uint32_t b = io.ld32(plane, jn * X.pitch_c + x0), bias = 1u + (y & 1u);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) out[k] = (3u * ((a >> (8u * k)) & 255u) + ((b >> (8u * k)) & 255u) + bias) >> 2;
        return;
    }
    const uint32_t i0 = x0 >> 1, last = X.cw - 1u;
    uint32_t t[4];                                           // s[i0 - 1 .. i0 + 2], clamped; for 4:2:0: 3 s[j] + s[jn]
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        uint32_t i = i0 + k;
        i = i ? i - 1u : 0u;
        i = i < last ? i : last;
        const uint32_t a = io.ld8(plane, j * X.pitch_c + i);
        t[k] = E::VS == 2 ? 3u * a + io.ld8(plane, jn * X.pitch_c + i) : a;
    }
    if (E::VS == 2) {
        out[0] = (3u * t[1] + t[0] + 8u) >> 4; out[1] = (3u * t[1] + t[2] + 7u) >> 4;
        out[2] = (3u * t[2] + t[1] + 8u) >> 4; out[3] = (3u * t[2] + t[3] + 7u) >> 4;
    } else {
        out[0] = (3u * t[1] + t[0] + 1u) >> 2; out[1] = (3u * t[1] + t[2] + 2u) >> 2;
        out[2] = (3u * t[2] + t[1] + 1u) >> 2; out[3] = (3u * t[2] + t[3] + 2u) >> 2;
    }
}
// jdsample.c takes the fancy h2v1 / h2v2 upsamplers only for a component MORE than two samples wide (downsampled_width > 2): a narrower one
// -- an image of at most four pixels across -- is replicated, both ways.  What the colour stages of DESIGN.md 5.19 call in the place of
// jda_ex_chroma4 (jda_exact_colour itself keeps calling that one: its instances stay the code they were).
template <int MODE, class IO> JDA_HD void jda_ex_chroma4_any(IO &io, const jda_ex_desc &X, const uint8_t *plane, uint32_t x0, uint32_t y, uint32_t *out)
{
    typedef jda_ex_layout<MODE> E;
    if (E::HS == 2 && X.cw <= 2u) {                          // (wave-uniform)
        const uint32_t row = (E::VS == 2 ? y >> 1 : y) * X.pitch_c, last = X.cw - 1u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t i = (x0 + k) >> 1;
            out[k] = io.ld8(plane, row + (i < last ? i : last));
        }
        return;
    }
    jda_ex_chroma4<MODE>(io, X, plane, x0, y, out);
}
// lane = the output pixels x0 .. x0 + 3 of row y: nothing outside out_w x out_rows is written.  RGB: the file's three
// components ARE R, G, B (jdapimin.c's rule, jda_colour_model): the upsampled samples go out as they stand, no conversion
template <int MODE, bool RGB = false, class IO> JDA_HD void jda_ex_quad(IO &io, const jda_ex_desc &X, uint32_t x0, uint32_t y)
{
    if (y >= X.out_rows || x0 >= X.out_w) return;
    const uint32_t n = X.out_w - x0 < 4u ? X.out_w - x0 : 4u;
    const uint32_t yw = io.ld32(X.plane[0], y * X.pitch_y + x0);
    if (X.gray_out) {
        const uint32_t o = y * X.out_pitch + x0;
        if (n == 4u) io.st32(X.out, o, yw);
        else for (uint32_t k = 0; k < n; k++) io.st8(X.out, o + k, (yw >> (8u * k)) & 255u);
        return;
    }
    uint32_t cb[4] = { 128u, 128u, 128u, 128u }, cr[4] = { 128u, 128u, 128u, 128u }, px[4];
    if (MODE != JDA_MODE_GRAY && RGB) {
        jda_ex_chroma4_any<MODE>(io, X, X.plane[1], x0, y, cb);
        jda_ex_chroma4_any<MODE>(io, X, X.plane[2], x0, y, cr);
    } else if (MODE != JDA_MODE_GRAY) {
        jda_ex_chroma4<MODE>(io, X, X.plane[1], x0, y, cb);
        jda_ex_chroma4<MODE>(io, X, X.plane[2], x0, y, cr);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++)
        px[k] = RGB ? ((yw >> (8u * k)) & 255u) | (cb[k] << 8) | (cr[k] << 16) | 0xff000000u : jda_ex_rgba((yw >> (8u * k)) & 255u, cb[k], cr[k]);
    const uint32_t o = y * X.out_pitch + x0 * 4u;
    if (n == 4u) io.st128(X.out, o, px);
    else for (uint32_t k = 0; k < n; k++) io.st32(X.out, o + 4u * k, px[k]);
}
// a wavefront = a tile record: count MCUs of MCU row mcu_y from MCU mcu_x0
template <int MODE, bool RGB = false, class IO> JDA_HD void jda_ex_colour_tile(IO &io, const jda_ex_desc &X, const jda_strip &S, uint32_t lane)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t quads = (uint32_t)S.count * ((uint32_t)T::MCU_W / 4u), items = quads * (uint32_t)T::MCU_H;
    const uint32_t px0 = (uint32_t)S.mcu_x0 * (uint32_t)T::MCU_W, py0 = (uint32_t)S.mcu_y * (uint32_t)T::MCU_H;
    if (py0 >= X.out_rows || px0 >= X.out_w) return;         // (wave-uniform)
    for (uint32_t it = lane; it < items; it += 64u) {
        const uint32_t r = it / quads, q = it - r * quads;
        jda_ex_quad<MODE, RGB>(io, X, px0 + 4u * q, py0 + r);
    }
}

// jda_ex4_*: the colour stage of a four-component image (CMYK or YCCK).  The planes stage has left four planes: components
// 0..2 as a three-component image of layout MODE, component 3 ("K") decoded as a gray image into X.plane3 -- at component 0's sampling
// (JDA_EX4_K_FULL: pitch_y, w x h) or at 1x1 (a chroma plane's pitch and extent).  lane = four output pixels of a row = one 16-byte store,
// over jda_ex_colour_tile's tile records and clip: component 0 and a full-size K as a dword each, every 1x1 component through
// jda_ex_chroma4_any<MODE> (fancy upsampling over its own extent, the MCU padding never read).  Then the model -- Pillow reads every
// four-component file as "CMYK;I", each byte of libjpeg's output inverted: a CMYK file's samples s give 255 - s; of a YCCK file libjpeg
// makes 255 - R, 255 - G, 255 - B (jdcolor.c's conversion, jda_ex_rgba) and passes K, so the bytes are R, G, B, 255 - s3 -- and the
// pixel type: those four bytes (JDA_CMYK8888), or Pillow's convert("RGB") of them, A = 0xFF.
// Pillow's MULDIV255 (ImagingUtils.h): a * b / 255, rounded
JDA_HD uint32_t jda_ex4_muldiv255(uint32_t a, uint32_t b)
{
    const uint32_t t = a * b + 128u;
    return ((t >> 8) + t) >> 8;
}
// Convert.c's cmyk2rgb on the bytes (C, M, Y, K) packed as a dword, C lowest: nk = 255 - K, clip8(nk - muldiv255(C, nk)), ..
JDA_HD uint32_t jda_ex4_cmyk2rgb(uint32_t cmyk)
{
    const int32_t nk = 255 - (int32_t)(cmyk >> 24);
    uint32_t px = 0xff000000u;
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) {
        int32_t v = nk - (int32_t)jda_ex4_muldiv255((cmyk >> (8u * c)) & 255u, (uint32_t)nk);
        v = v < 0 ? 0 : v > 255 ? 255 : v;
        px |= (uint32_t)v << (8u * c);
    }
    return px;
}
template <int MODE, class IO> JDA_HD void jda_ex4_quad(IO &io, const jda_ex_desc &X, uint32_t x0, uint32_t y)
{
    if (y >= X.out_rows || x0 >= X.out_w) return;
    const uint32_t n = X.out_w - x0 < 4u ? X.out_w - x0 : 4u;
    const uint32_t s0 = io.ld32(X.plane[0], y * X.pitch_y + x0);
    uint32_t s1[4], s2[4], k[4], px[4];
    jda_ex_chroma4_any<MODE>(io, X, X.plane[1], x0, y, s1);
    jda_ex_chroma4_any<MODE>(io, X, X.plane[2], x0, y, s2);
    if (MODE == JDA_MODE_444 || (X.cs4 & JDA_EX4_K_FULL)) {                // (wave-uniform)
        const uint32_t kw = io.ld32(X.plane3, y * X.pitch_y + x0);
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) k[i] = (kw >> (8u * i)) & 255u;
    } else jda_ex_chroma4_any<MODE>(io, X, X.plane3, x0, y, k);
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
        const uint32_t a = (s0 >> (8u * i)) & 255u;
        const uint32_t cmy = (X.cs4 & JDA_EX4_YCCK) ? jda_ex_rgba(a, s1[i], s2[i]) & 0xffffffu : (255u - a) | ((255u - s1[i]) << 8) | ((255u - s2[i]) << 16);
        const uint32_t cmyk = cmy | ((255u - k[i]) << 24);
        px[i] = (X.cs4 & JDA_EX4_CMYK_OUT) ? cmyk : jda_ex4_cmyk2rgb(cmyk);
    }
    const uint32_t o = y * X.out_pitch + x0 * 4u;
    if (n == 4u) io.st128(X.out, o, px);
    else for (uint32_t i = 0; i < n; i++) io.st32(X.out, o + 4u * i, px[i]);
}
// a wavefront = a tile record of the image's components 0..2: count MCUs of MCU row mcu_y from MCU mcu_x0 (jda_ex_colour_tile's walk)
template <int MODE, class IO> JDA_HD void jda_ex4_colour_tile(IO &io, const jda_ex_desc &X, const jda_strip &S, uint32_t lane)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t quads = (uint32_t)S.count * ((uint32_t)T::MCU_W / 4u), items = quads * (uint32_t)T::MCU_H;
    const uint32_t px0 = (uint32_t)S.mcu_x0 * (uint32_t)T::MCU_W, py0 = (uint32_t)S.mcu_y * (uint32_t)T::MCU_H;
    if (py0 >= X.out_rows || px0 >= X.out_w) return;         // (wave-uniform)
    for (uint32_t it = lane; it < items; it += 64u) {
        const uint32_t r = it / quads, q = it - r * quads;
        jda_ex4_quad<MODE>(io, X, px0 + 4u * q, py0 + r);
    }
}

// baseline load phase: a resident BASELINE image as the third source of the planes stage, beside jda_ct_load and jda_cs_zero / _scatter.
// lane = block of the tile: T.81's reader -- a 32-bit peek of the scan at any bit position from the index entry's own, the AC LUT of the
// image's table blob (the layout jda_rc_extract_block reads), EXTEND of WHOLE magnitudes, never the reference's truncated reads -- into the
// lane's LDS slot in NATURAL order (the blob's cZigZag2), the block's DC value from the index.  The slot then holds what the dense load
// phase would have put there for the same coefficients; no coefficient touches HBM.  The reader is written out here a third time (after
// jda_rc_extract_block and its _xf twin): those two store zig-zag order, clamp to the encoder's range and count its code bits as they go,
// and they are kernels of their own features, which this one leaves as they stand.
// what a lane needs of its block's jda_ex_src, field by field (no array: a copy of the whole record, indexed by component, would live in scratch)
struct jda_ex_walk { const uint8_t *scan, *tables; const uint32_t *blk_index; const int16_t *blk_dc; uint32_t scan_len, ac_ids, bpm, nluma; };
template <class IO> JDA_HD jda_ex_walk jda_ex_walk_of(const jda_ex_src *J, IO &io)
{
    jda_ex_walk W;
    W.scan = (const uint8_t *)io.ldptr(&J->S.scan); W.tables = (const uint8_t *)io.ldptr(&J->S.tables);
    W.blk_index = (const uint32_t *)io.ldptr(&J->S.blk_index); W.blk_dc = (const int16_t *)io.ldptr(&J->S.blk_dc);
    W.scan_len = io.ld32(&J->S.scan_len); W.bpm = io.ld32(&J->bpm); W.nluma = io.ld32(&J->nluma);
    W.ac_ids = (io.ld32(&J->S.ac_id[0]) & 1u) | ((io.ld32(&J->S.ac_id[1]) & 1u) << 1) | ((io.ld32(&J->S.ac_id[2]) & 1u) << 2);
    return W;
}
template <class IO> JDA_HD void jda_ex_extract_block(const jda_ex_walk &W, uint32_t s, uint8_t *slot, IO &io)
{
    const uint32_t k = s % W.bpm, c = k < W.nluma ? 0u : 1u + k - W.nluma;
    int16_t *coef = (int16_t *)slot;
    jda_u64_alias *z8 = (jda_u64_alias *)slot;
#pragma unroll
    for (int i = 0; i < 16; i++) z8[i] = 0;
    const uint32_t ix = io.ld32(W.blk_index + s);
    const uint32_t dcw = io.ld32((const uint32_t *)W.blk_dc + (s >> 1));
    coef[0] = (int16_t)((s & 1u) ? dcw >> 16 : dcw & 0xffffu);
    uint32_t p = (ix >> JDA_INDEX_OFF_BITS) * 8u + (ix & (JDA_INDEX_TRUNC - 1u));
    const uint32_t *lut = (const uint32_t *)(W.tables + JDA_TB_AC + ((W.ac_ids >> c) & 1u) * 4096u);
    // (the scan section is scan_len + JDA_SCAN_PAD bytes: both dwords of a peek stay inside whatever an entry says, as jda_rc_peek's)
    const uint32_t a_max = (W.scan_len + JDA_SCAN_PAD - 8u) >> 2;
    uint32_t z = 1;
    while (z < 64u) {
        uint32_t a = p >> 5;
        a = a < a_max ? a : a_max;
        const uint32_t d0 = __builtin_bswap32(io.ld32((const uint32_t *)W.scan + a)), d1 = __builtin_bswap32(io.ld32((const uint32_t *)W.scan + a + 1u)), sh = p & 31u;
        const uint32_t w = sh ? (d0 << sh) | (d1 >> (32u - sh)) : d0;
        const uint32_t key = w >= 0xfc000000u ? 1024u + ((w >> 16) & 0x3ffu) : w >> 22;
        const uint32_t pair = io.ld32(lut + (key >> 1)), raw = (key & 1u) ? pair >> 16 : pair & 0xffffu;
        const uint32_t len = raw >> 8, rs = raw & 0xffu, sz = rs & 15u;
        if (len == 0u || rs == 0u) break;                                // no such code, or EOB
        z += rs >> 4;
        if (sz && z < 64u) {
            const uint32_t m = w << len, v = m >> (32u - sz);
            const int32_t val = (m & 0x80000000u) ? (int32_t)v : (int32_t)v - (int32_t)((1u << sz) - 1u);       // T.81 F.2.2.1 EXTEND
            coef[io.ld8(W.tables, JDA_TB_ZIGZAG + z) & 63u] = (int16_t)val;      // (the blob's cZigZag2: zig-zag position -> natural index)
        }
        p += len + sz;
        z++;
    }
}
// the load phase: lane = block of the tile; src: the image's record
template <int MODE, class IO> JDA_HD void jda_ex_load_baseline(IO &io, const jda_ex_src *src, const jda_tile_ctx &C, uint32_t lane, uint8_t *wl)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    if (lane >= C.count * (uint32_t)T::NBLK) return;
    jda_ex_extract_block(jda_ex_walk_of(src, io), C.first_block + lane, wl + L::COEF_OFF + lane * JDA_COEF_STRIDE, io);
}

// ================================================================================================
// jda_exs_*: the libjpeg-exact decode at 1/2, 1/4 and 1/8: libjpeg's scaled decode as Pillow's draft() drives it, stated
// in numpy in tests/exact_scaled_util.py.  SCALE = 2, 4, 8; MIN = 8 / SCALE.  A component's blocks go through an IDCT of its own size ss
// (jdmaster.c): MIN for luma and for every chroma but 4:2:0's, whose ss is 2 MIN -- at 1/2 the full islow IDCT above -- and which then
// needs no upsampling.  jidctred.c's 4x4 reads 49 coefficients (no row or column 4), its 2x2 reads 25 (frequencies 0, 1, 3, 5, 7), 1x1 the
// DC.  Multiplies by IDCT constants are full 32-bit ones, as at full size.
//   planes   lane = block behind the same three load phases.  A lane takes the coefficients its IDCT reads out of its slot into
//            registers and leaves ss rows of ss bytes packed in px[]; once every lane has read (a wave sync), the slots are free and the
//            tile is assembled over them: per component ROWS rows of the tile's samples, each byte where its plane address says modulo 4
//            (jda_exs_stage).  After another sync the lanes share the rows out dword by dword (jda_exs_store): 4-byte stores wherever
//            all four bytes are the tile's, single bytes at its unaligned ends (a 20-MCU 4:4:4 tile at 1/8 is 20 bytes wide, a 4:2:2 one
//            at 1/8 is 32 luma and 16 chroma bytes).  Neighbouring tiles never write the same byte.
//            A baseline image's 1x1 lanes take the DC value from the index and never touch the scan: jda_exs_load_baseline walks only
//            lanes whose ss is above 1 (4:2:0's chroma at 1/8) -- at 1/8 gray, 4:4:4, 4:2:2 and 4:4:0 have no walk at all.
//   colour   lane = four output pixels at a multiple of 4 (one 16-byte store; single pixels where a tile begins or ends inside the quad),
//            over the tile's own pixels: count x MCU_W / SCALE by MCU_H / SCALE.  X.up names what jdsample.c does at this scale: nothing,
//            h2v1 or h1v2, fancy or replicated; the indices are clamped to the component's own scaled extent (X.cw x X.ch).
#define JDA_EX_UP_NONE 0u
#define JDA_EX_UP_H2V1_FANCY 1u
#define JDA_EX_UP_H2V1_REPLICATE 2u
#define JDA_EX_UP_H1V2_FANCY 3u
#define JDA_EX_UP_H1V2_REPLICATE 4u
template <int MODE, int SCALE> struct jda_exs_layout {
    enum { MIN = 8 / SCALE, SS_Y = MIN, SS_C = MODE == JDA_MODE_420 ? 2 * MIN : MIN,
           HS = jda_ex_layout<MODE>::HS, VS = jda_ex_layout<MODE>::VS, MCUS = jda_lds_layout<MODE>::MCUS,
           // the tile over the slots: a row holds the tile's bytes behind up to three of misalignment, dwords of it up to three more
           PITCH_Y = (MCUS * HS * SS_Y + 6) / 4 * 4, ROWS_Y = VS * SS_Y, PITCH_C = (MCUS * SS_C + 6) / 4 * 4, ROWS_C = SS_C,
           OFF_C = PITCH_Y * ROWS_Y, STAGE_BYTES = OFF_C + 2 * PITCH_C * ROWS_C };
    static_assert(SCALE == 2 || SCALE == 4 || SCALE == 8, "the reduced sizes");
    static_assert(STAGE_BYTES <= jda_lds_layout<MODE>::BLOCKS * JDA_COEF_STRIDE, "the assembled tile fits over the slots");
};

// one pass of jidctred.c's jpeg_idct_4x4 (DESCALE by 12 for the columns, 19 for the rows) and of jpeg_idct_2x2 (13, 20)
template <int SHIFT> JDA_HD void jda_exs_idct4(int32_t d0, int32_t d1, int32_t d2, int32_t d3, int32_t d5, int32_t d6, int32_t d7, int32_t *o, int stride)
{
    typedef uint32_t U;
    const U R = 1u << (SHIFT - 1);
    const U t0 = (U)d0 << 14, t2 = (U)d2 * 15137u - (U)d6 * 6270u;
    const U t10 = t0 + t2, t12 = t0 - t2;
    const U a = (U)d5 * 11893u + (U)d1 * 8697u - (U)d7 * 1730u - (U)d3 * 17799u;
    const U c = (U)d3 * 7373u + (U)d1 * 20995u - (U)d7 * 4176u - (U)d5 * 4926u;
    o[0] = (int32_t)(t10 + c + R) >> SHIFT; o[3 * stride] = (int32_t)(t10 - c + R) >> SHIFT;
    o[stride] = (int32_t)(t12 + a + R) >> SHIFT; o[2 * stride] = (int32_t)(t12 - a + R) >> SHIFT;
}
template <int SHIFT> JDA_HD void jda_exs_idct2(int32_t d0, int32_t d1, int32_t d3, int32_t d5, int32_t d7, int32_t *o, int stride)
{
    typedef uint32_t U;
    const U R = 1u << (SHIFT - 1);
    const U t10 = (U)d0 << 15, t0 = (U)d5 * 6967u + (U)d1 * 29692u - (U)d7 * 5906u - (U)d3 * 10426u;
    o[0] = (int32_t)(t10 + t0 + R) >> SHIFT; o[stride] = (int32_t)(t10 - t0 + R) >> SHIFT;
}
// row r of a slot, dequantised: eight coefficients times the raw quantisers
JDA_HD void jda_exs_row(const jda_u64_alias *src, const jda_u64_alias *qs, uint32_t r, int32_t *d)
{
#pragma unroll
    for (uint32_t h = 0; h < 2u; h++) {
        const uint64_t v = src[2u * r + h], q = qs[2u * r + h];
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) d[4u * h + j] = jda_mulc<true>((int32_t)(int16_t)(uint16_t)(v >> (16u * j)), (int32_t)(uint16_t)(q >> (16u * j)));
    }
}
// the SS x SS samples of one block: row y in px[y * SS / 4 ..] (SS = 8: two dwords a row, 4: one; SS = 2: both rows in px[0], 1: a byte)
template <int SS> JDA_HD void jda_exs_idct(const uint8_t *slot, const uint8_t *q, uint32_t *px)
{
    const jda_u64_alias *src = (const jda_u64_alias *)slot, *qs = (const jda_u64_alias *)q;
    if (SS == 8) {
        int32_t ws[64];
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++) jda_exs_row(src, qs, r, ws + 8u * r);
#pragma unroll
        for (uint32_t x = 0; x < 8u; x++) jda_ex_idct8<11>(ws[x], ws[8 + x], ws[16 + x], ws[24 + x], ws[32 + x], ws[40 + x], ws[48 + x], ws[56 + x]);
#pragma unroll
        for (uint32_t y = 0; y < 8u; y++) {
            jda_ex_idct8<18>(ws[8 * y], ws[8 * y + 1], ws[8 * y + 2], ws[8 * y + 3], ws[8 * y + 4], ws[8 * y + 5], ws[8 * y + 6], ws[8 * y + 7]);
            px[2 * y] = jda_ex_limit(ws[8 * y]) | (jda_ex_limit(ws[8 * y + 1]) << 8) | (jda_ex_limit(ws[8 * y + 2]) << 16) | (jda_ex_limit(ws[8 * y + 3]) << 24);
            px[2 * y + 1] = jda_ex_limit(ws[8 * y + 4]) | (jda_ex_limit(ws[8 * y + 5]) << 8) | (jda_ex_limit(ws[8 * y + 6]) << 16) | (jda_ex_limit(ws[8 * y + 7]) << 24);
        }
    } else if (SS == 4) {
        int32_t d[64], ws[32], o[4];
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++) if (r != 4u) jda_exs_row(src, qs, r, d + 8u * r);
#pragma unroll
        for (uint32_t x = 0; x < 8u; x++) if (x != 4u) jda_exs_idct4<12>(d[x], d[8 + x], d[16 + x], d[24 + x], d[40 + x], d[48 + x], d[56 + x], ws + x, 8);
#pragma unroll
        for (uint32_t y = 0; y < 4u; y++) {
            jda_exs_idct4<19>(ws[8 * y], ws[8 * y + 1], ws[8 * y + 2], ws[8 * y + 3], ws[8 * y + 5], ws[8 * y + 6], ws[8 * y + 7], o, 1);
            px[y] = jda_ex_limit(o[0]) | (jda_ex_limit(o[1]) << 8) | (jda_ex_limit(o[2]) << 16) | (jda_ex_limit(o[3]) << 24);
        }
    } else if (SS == 2) {
        int32_t d[64], ws[16], o[2];
#pragma unroll
        for (uint32_t r = 0; r < 8u; r++) if (r < 2u || (r & 1u)) jda_exs_row(src, qs, r, d + 8u * r);
#pragma unroll
        for (uint32_t x = 0; x < 8u; x++) if (x < 2u || (x & 1u)) jda_exs_idct2<13>(d[x], d[8 + x], d[24 + x], d[40 + x], d[56 + x], ws + x, 8);
        px[0] = 0;
#pragma unroll
        for (uint32_t y = 0; y < 2u; y++) {
            jda_exs_idct2<20>(ws[8 * y], ws[8 * y + 1], ws[8 * y + 3], ws[8 * y + 5], ws[8 * y + 7], o, 1);
            px[0] |= (jda_ex_limit(o[0]) | (jda_ex_limit(o[1]) << 8)) << (16u * y);
        }
    } else {
        const int32_t dc = jda_mulc<true>((int32_t)(int16_t)(uint16_t)src[0], (int32_t)(uint16_t)qs[0]);
        px[0] = jda_ex_limit((int32_t)((uint32_t)dc + 4u) >> 3);                     // DESCALE(d0, 3)
    }
}
// where a lane's block lies: its component, its place in the tile in blocks of the component
template <int MODE> JDA_HD void jda_exs_place(uint32_t lane, uint32_t *c, uint32_t *bx, uint32_t *by)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_ex_layout<MODE> E;
    const uint32_t k = lane % (uint32_t)T::NBLK, m = lane / (uint32_t)T::NBLK;
    *c = k < (uint32_t)T::NLUMA ? 0u : k - (uint32_t)T::NLUMA + 1u;
    *bx = *c ? m : m * (uint32_t)E::HS + k % (uint32_t)E::HS;
    *by = *c ? 0u : k / (uint32_t)E::HS;
}
// the load phase over a resident baseline image: only the lanes whose IDCT reads more than the DC walk the scan
template <int MODE, int SCALE, class IO>
JDA_HD void jda_exs_load_baseline(IO &io, const jda_ex_desc &X, const jda_ex_src *src, const jda_tile_ctx &C, uint32_t lane, uint8_t *wl)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    typedef jda_exs_layout<MODE, SCALE> Z;
    if ((int)Z::SS_Y == 1 && (int)Z::SS_C == 1) return;
    if (lane >= C.count * (uint32_t)T::NBLK) return;
    uint32_t c, bx, by;
    jda_exs_place<MODE>(lane, &c, &bx, &by);
    if ((c ? (int)Z::SS_C : (int)Z::SS_Y) == 1 || (c && X.luma_only)) return;
    jda_ex_extract_block(jda_ex_walk_of(src, io), C.first_block + lane, wl + L::COEF_OFF + lane * JDA_COEF_STRIDE, io);
}
// phase 1, lane = block: the block's samples into px[16] (what the lane's ss needs of it)
template <int MODE, int SCALE, int SOURCE, class IO>
JDA_HD void jda_exs_block(IO &io, const jda_ex_desc &X, const jda_ex_src *src, const jda_tile_ctx &C, uint32_t lane, const uint8_t *wl, const uint8_t *qt, uint32_t *px)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_lds_layout<MODE> L;
    typedef jda_exs_layout<MODE, SCALE> Z;
    if (lane >= C.count * (uint32_t)T::NBLK) return;
    uint32_t c, bx, by;
    jda_exs_place<MODE>(lane, &c, &bx, &by);
    if (c && X.luma_only) return;
    const uint8_t *slot = wl + L::COEF_OFF + lane * JDA_COEF_STRIDE, *q = qt + c * 128u;
    if (c == 0u || (int)Z::SS_C == (int)Z::SS_Y) {
        if ((int)Z::SS_Y == 1 && SOURCE == 2) {                  // the DC value from the index: the slot was never filled
            const uint32_t s = C.first_block + lane;
            const uint32_t dcw = io.ld32((const uint32_t *)io.ldptr(&src->S.blk_dc) + (s >> 1));
            const int32_t dc = jda_mulc<true>((int32_t)(int16_t)(uint16_t)((s & 1u) ? dcw >> 16 : dcw & 0xffffu), (int32_t)(uint16_t)*(const jda_u64_alias *)q);
            px[0] = jda_ex_limit((int32_t)((uint32_t)dc + 4u) >> 3);
        } else jda_exs_idct<(int)Z::SS_Y>(slot, q, px);
    } else jda_exs_idct<(int)Z::SS_C>(slot, q, px);
}
// phase 2, lane = block: its rows into the assembled tile (stage: the wavefront's slots, free by now)
template <int MODE, int SCALE>
JDA_HD void jda_exs_stage(const jda_ex_desc &X, const jda_strip &S, const jda_tile_ctx &C, uint32_t lane, uint8_t *stage, const uint32_t *px)
{
    typedef jda_mode_traits<MODE> T;
    typedef jda_exs_layout<MODE, SCALE> Z;
    if (lane >= C.count * (uint32_t)T::NBLK) return;
    uint32_t c, bx, by;
    jda_exs_place<MODE>(lane, &c, &bx, &by);
    if (c && X.luma_only) return;
    const uint32_t ss = c ? (uint32_t)Z::SS_C : (uint32_t)Z::SS_Y, pitch = c ? (uint32_t)Z::PITCH_C : (uint32_t)Z::PITCH_Y;
    const uint32_t x0 = (uint32_t)S.mcu_x0 * (c ? 1u : (uint32_t)Z::HS) * ss;              // the tile's first sample of a row of the plane
    uint8_t *p = stage + (c ? (uint32_t)Z::OFF_C + (c - 1u) * (uint32_t)(Z::PITCH_C * Z::ROWS_C) : 0u) + by * ss * pitch + (x0 & 3u) + bx * ss;
    if (ss == 8u) {
#pragma unroll
        for (uint32_t y = 0; y < 8u; y++) { ((jda_u32_alias *)(p + y * pitch))[0] = px[2 * y]; ((jda_u32_alias *)(p + y * pitch))[1] = px[2 * y + 1]; }
    } else if (ss == 4u) {
#pragma unroll
        for (uint32_t y = 0; y < 4u; y++) *(jda_u32_alias *)(p + y * pitch) = px[y];
    } else if (ss == 2u) {
        p[0] = (uint8_t)px[0]; p[1] = (uint8_t)(px[0] >> 8); p[pitch] = (uint8_t)(px[0] >> 16); p[pitch + 1u] = (uint8_t)(px[0] >> 24);
    } else p[0] = (uint8_t)px[0];
}
// phase 3: the rows of the assembled tile, shared out dword by dword over the lanes
template <int MODE, int SCALE, class IO>
JDA_HD void jda_exs_store(IO &io, const jda_ex_desc &X, const jda_strip &S, uint32_t lane, const uint8_t *stage)
{
    typedef jda_exs_layout<MODE, SCALE> Z;
    const uint32_t ncomp = (MODE == JDA_MODE_GRAY || X.luma_only) ? 1u : 3u;
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) {                      // (unrolled: the plane pointers stay in registers)
        if (c >= ncomp) break;
        const uint32_t ss = c ? (uint32_t)Z::SS_C : (uint32_t)Z::SS_Y, spitch = c ? (uint32_t)Z::PITCH_C : (uint32_t)Z::PITCH_Y;
        const uint32_t rows = c ? (uint32_t)Z::ROWS_C : (uint32_t)Z::ROWS_Y, hs = c ? 1u : (uint32_t)Z::HS;
        const uint32_t x0 = (uint32_t)S.mcu_x0 * hs * ss, wb = (uint32_t)S.count * hs * ss, a = x0 & 3u, nd = (a + wb + 3u) >> 2;
        const uint32_t pitch = c ? X.pitch_c : X.pitch_y, y0 = (uint32_t)S.mcu_y * rows;
        uint8_t *plane = c == 0u ? X.plane[0] : c == 1u ? X.plane[1] : X.plane[2];
        const uint8_t *st = stage + (c ? (uint32_t)Z::OFF_C + (c - 1u) * (uint32_t)(Z::PITCH_C * Z::ROWS_C) : 0u);
        for (uint32_t it = lane; it < rows * nd; it += 64u) {
            const uint32_t r = it / nd, j = it - r * nd;
            const uint32_t v = *(const jda_u32_alias *)(st + r * spitch + 4u * j);
            const uint32_t lo = j ? 0u : a, hi = a + wb - 4u * j < 4u ? a + wb - 4u * j : 4u;
            const uint32_t off = (y0 + r) * pitch + (x0 - a) + 4u * j;
            if (lo == 0u && hi == 4u) io.st32(plane, off, v);
            else for (uint32_t b = lo; b < hi; b++) io.st8(plane, off + b, (v >> (8u * b)) & 255u);
        }
    }
}

// the four upsampled samples of a chroma plane under the output pixels x0 .. x0 + 3 (x0 a multiple of 4) of output row y
template <class IO> JDA_HD void jda_exs_chroma4(IO &io, const jda_ex_desc &X, const uint8_t *plane, uint32_t x0, uint32_t y, uint32_t *out)
{
    const uint32_t up = X.up;
    if (up == JDA_EX_UP_NONE || up == JDA_EX_UP_H1V2_REPLICATE || up == JDA_EX_UP_H1V2_FANCY) {
        const uint32_t j = up == JDA_EX_UP_NONE ? y : y >> 1;
        const uint32_t a = io.ld32(plane, j * X.pitch_c + x0);
        if (up != JDA_EX_UP_H1V2_FANCY) {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) out[k] = (a >> (8u * k)) & 255u;
            return;
        }
        const uint32_t jn = (y & 1u) ? (j + 1u < X.ch ? j + 1u : j) : (j ? j - 1u : 0u);
        const uint32_t b = io.ld32(plane, jn * X.pitch_c + x0), bias = 1u + (y & 1u);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) out[k] = (3u * ((a >> (8u * k)) & 255u) + ((b >> (8u * k)) & 255u) + bias) >> 2;
        return;
    }
    const uint32_t i0 = x0 >> 1, last = X.cw - 1u, row = y * X.pitch_c;
    if (up == JDA_EX_UP_H2V1_REPLICATE) {
        const uint32_t s0 = io.ld8(plane, row + (i0 < last ? i0 : last)), s1 = io.ld8(plane, row + (i0 + 1u < last ? i0 + 1u : last));
        out[0] = out[1] = s0; out[2] = out[3] = s1;
        return;
    }
    uint32_t t[4];                                           // s[i0 - 1 .. i0 + 2], clamped
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        uint32_t i = i0 + k;
        i = i ? i - 1u : 0u;
        t[k] = io.ld8(plane, row + (i < last ? i : last));
    }
    out[0] = (3u * t[1] + t[0] + 1u) >> 2; out[1] = (3u * t[1] + t[2] + 2u) >> 2;
    out[2] = (3u * t[2] + t[1] + 1u) >> 2; out[3] = (3u * t[2] + t[3] + 2u) >> 2;
}
// lane = the output pixels x0 + lo .. x0 + hi - 1 of row y (x0 a multiple of 4): nothing outside out_w x out_rows is written
// (RGB: as jda_ex_quad's)
template <int MODE, bool RGB = false, class IO> JDA_HD void jda_exs_quad(IO &io, const jda_ex_desc &X, uint32_t x0, uint32_t y, uint32_t lo, uint32_t hi)
{
    if (y >= X.out_rows || x0 + lo >= X.out_w) return;
    if (X.out_w - x0 < hi) hi = X.out_w - x0;
    const uint32_t yw = io.ld32(X.plane[0], y * X.pitch_y + x0);
    if (X.gray_out) {
        const uint32_t o = y * X.out_pitch + x0;
        if (lo == 0u && hi == 4u) io.st32(X.out, o, yw);
        else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) if (k >= lo && k < hi) io.st8(X.out, o + k, (yw >> (8u * k)) & 255u);
        }
        return;
    }
    uint32_t cb[4] = { 128u, 128u, 128u, 128u }, cr[4] = { 128u, 128u, 128u, 128u }, px[4];
    if (MODE != JDA_MODE_GRAY) {
        jda_exs_chroma4(io, X, X.plane[1], x0, y, cb);
        jda_exs_chroma4(io, X, X.plane[2], x0, y, cr);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++)
        px[k] = RGB ? ((yw >> (8u * k)) & 255u) | (cb[k] << 8) | (cr[k] << 16) | 0xff000000u : jda_ex_rgba((yw >> (8u * k)) & 255u, cb[k], cr[k]);
    const uint32_t o = y * X.out_pitch + x0 * 4u;
    if (lo == 0u && hi == 4u) io.st128(X.out, o, px);
    else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) if (k >= lo && k < hi) io.st32(X.out, o + 4u * k, px[k]);
    }
}
// a wavefront = a tile record: the pixels of count MCUs of MCU row mcu_y from MCU mcu_x0 at the record's scale (X.scale: 2, 4, 8)
template <int MODE, bool RGB = false, class IO> JDA_HD void jda_exs_colour_tile(IO &io, const jda_ex_desc &X, const jda_strip &S, uint32_t lane)
{
    typedef jda_mode_traits<MODE> T;
    const uint32_t sh = X.scale == 8u ? 3u : X.scale == 4u ? 2u : 1u;
    const uint32_t mw = (uint32_t)T::MCU_W >> sh, mh = (uint32_t)T::MCU_H >> sh;
    const uint32_t px0 = (uint32_t)S.mcu_x0 * mw, px1 = px0 + (uint32_t)S.count * mw, py0 = (uint32_t)S.mcu_y * mh;
    if (py0 >= X.out_rows || px0 >= X.out_w) return;         // (wave-uniform)
    const uint32_t xa = px0 & ~3u, quads = (px1 - xa + 3u) >> 2, items = quads * mh;
    for (uint32_t it = lane; it < items; it += 64u) {
        const uint32_t r = it / quads, q = it - r * quads, x0 = xa + 4u * q;
        jda_exs_quad<MODE, RGB>(io, X, x0, py0 + r, x0 < px0 ? px0 - x0 : 0u, px1 - x0 < 4u ? px1 - x0 : 4u);
    }
}

// ================================================================================================
// jda_exr_*: the colour stage of a pixel rectangle (jda_exact_colour_rect).  The planes stage has written the MCUs the
// rectangle's formulas read (jda_exact_rect_plan) at the whole image's geometry; a lane makes four DESTINATION pixels dx .. dx + 3 (dx a
// multiple of 4) of destination row dy -- one 16-byte store, or four bytes of a gray surface -- from the source pixels R.x + dx .., row
// R.y + dy: any alignment of the Y bytes, either chroma parity.  The upsampling is named an axis (JDA_EXR_*), from the layout, the record's
// scale and up and libjpeg's rule for a narrow plane, so that one function serves every scale; the formulas, the clamps to the
// component's own extent and the biases are jda_ex_chroma4_any's and jda_exs_chroma4's.  No byte outside the samples the definition
// names for the rectangle's pixels is loaded: a dword only where all four bytes are the rectangle's.
struct jda_exr_rec { uint32_t x, y, w, h; };                 // the rectangle in pixels of the image at its scale; beside jda_ex_desc in the call's blob
#define JDA_EXR_NONE 0u
#define JDA_EXR_REPLICATE 1u
#define JDA_EXR_FANCY 2u
#define JDA_EXR_TILE_QUADS 64u                               // a tile record of the destination: up to 64 quads of a row ..
#define JDA_EXR_TILE_ROWS 32u                                // .. times 32 rows (mcu_x0, mcu_y: the tile's place in units of these; count 1)
#define JDA_EXR_WAVES 4u                                     // wavefronts (tile records) a workgroup of jda_exact_colour_rect
// what each axis of a chroma plane gets: hs, vs the layout's factors, scale / up / cw the record's (scale 0 or 1: full size)
JDA_HD void jda_exr_kinds(uint32_t hs, uint32_t vs, uint32_t scale, uint32_t up, uint32_t cw, uint32_t *kh, uint32_t *kv)
{
    *kh = *kv = JDA_EXR_NONE;
    if (scale <= 1u) {
        const bool narrow = hs == 2u && cw <= 2u;            // jdsample.c: no fancy h2v1 / h2v2 for a component at most two samples wide
        if (hs == 2u) *kh = narrow ? JDA_EXR_REPLICATE : JDA_EXR_FANCY;
        if (vs == 2u) *kv = narrow ? JDA_EXR_REPLICATE : JDA_EXR_FANCY;
        return;
    }
    if (up == JDA_EX_UP_H2V1_FANCY) *kh = JDA_EXR_FANCY;
    else if (up == JDA_EX_UP_H2V1_REPLICATE) *kh = JDA_EXR_REPLICATE;
    else if (up == JDA_EX_UP_H1V2_FANCY) *kv = JDA_EXR_FANCY;
    else if (up == JDA_EX_UP_H1V2_REPLICATE) *kv = JDA_EXR_REPLICATE;
}
// the samples one axis reads for the pixels [p0, p1] (inclusive) of a component `ext` samples long: [*lo, *hi]
JDA_HD void jda_exr_reads(uint32_t kind, uint32_t p0, uint32_t p1, uint32_t ext, uint32_t *lo, uint32_t *hi)
{
    if (kind == JDA_EXR_NONE) { *lo = p0; *hi = p1; return; }
    uint32_t a = p0 >> 1, b = p1 >> 1;
    if (kind == JDA_EXR_FANCY) {
        if (!(p0 & 1u) && a) a--;
        if ((p1 & 1u) && b + 1u < ext) b++;
    }
    *lo = a; *hi = b < ext ? b : ext - 1u;
}
// the bytes sx .. sx + 3 of a plane's row (row: its byte offset) as a dword, of which the first n are asked for; [x_lo, x_hi): the
// samples of the row the rectangle reads -- a dword load only inside them
template <class IO> JDA_HD uint32_t jda_exr_row4(IO &io, const uint8_t *plane, uint32_t row, uint32_t sx, uint32_t n, uint32_t x_lo, uint32_t x_hi)
{
    const uint32_t a = sx & 3u, b = sx - a;
    if (a == 0u) { if (sx + 4u <= x_hi) return io.ld32(plane, row + sx); }
    else if (b >= x_lo && b + 8u <= x_hi) {
        const uint32_t lo = io.ld32(plane, row + b), hi = io.ld32(plane, row + b + 4u);
        return (lo >> (8u * a)) | (hi << (32u - 8u * a));
    }
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) if (k < n) v |= io.ld8(plane, row + sx + k) << (8u * k);
    return v;
}
// the upsampled samples of a chroma plane under the source pixels sx .. sx + n - 1 of source row sy (out[n ..] are not meaningful)
template <class IO>
JDA_HD void jda_exr_chroma4(IO &io, const jda_ex_desc &X, const jda_exr_rec &R, const uint8_t *plane, uint32_t kh, uint32_t kv, uint32_t sx, uint32_t sy, uint32_t n, uint32_t *out)
{
    const uint32_t j = kv == JDA_EXR_NONE ? sy : sy >> 1;
    const uint32_t jn = kv == JDA_EXR_FANCY ? ((sy & 1u) ? (j + 1u < X.ch ? j + 1u : j) : (j ? j - 1u : 0u)) : j;
    const uint32_t row = j * X.pitch_c, rown = jn * X.pitch_c;
    if (kh == JDA_EXR_NONE) {
        const uint32_t a = jda_exr_row4(io, plane, row, sx, n, R.x, R.x + R.w);
        if (kv != JDA_EXR_FANCY) {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) out[k] = (a >> (8u * k)) & 255u;
            return;
        }
        const uint32_t b = jda_exr_row4(io, plane, rown, sx, n, R.x, R.x + R.w), bias = 1u + (sy & 1u);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) out[k] = (3u * ((a >> (8u * k)) & 255u) + ((b >> (8u * k)) & 255u) + bias) >> 2;
        return;
    }
    const uint32_t i0 = sx >> 1, p = sx & 1u, last = X.cw - 1u;
    if (kh == JDA_EXR_REPLICATE) {
        const uint32_t ie = (sx + n - 1u) >> 1;              // the last sample a pixel of the quad lies over
        uint32_t s[3];
#pragma unroll
        for (uint32_t k = 0; k < 3u; k++) {
            const uint32_t i = i0 + k <= ie ? i0 + k : i0;
            s[k] = io.ld8(plane, row + (i < last ? i : last));
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) out[k] = s[(p + k) >> 1];
        return;
    }
    // fancy: s[i0 - 1 .. i0 + 2], clamped, of which a quad that begins on an odd pixel does not read the first, a short one not the last
    uint32_t t[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const bool need = k == 0u ? p == 0u : k == 1u ? true : k == 2u ? n + p >= 2u : n + p >= 4u;
        uint32_t i = need ? i0 + k : i0 + 1u;
        i = i ? i - 1u : 0u;
        i = i < last ? i : last;
        const uint32_t a = io.ld8(plane, row + i);
        t[k] = kv == JDA_EXR_FANCY ? 3u * a + io.ld8(plane, rown + i) : a;
    }
    const uint32_t be = kv == JDA_EXR_FANCY ? 8u : 1u, bo = kv == JDA_EXR_FANCY ? 7u : 2u, sh = kv == JDA_EXR_FANCY ? 4u : 2u;
    if (p == 0u) {
        out[0] = (3u * t[1] + t[0] + be) >> sh; out[1] = (3u * t[1] + t[2] + bo) >> sh;
        out[2] = (3u * t[2] + t[1] + be) >> sh; out[3] = (3u * t[2] + t[3] + bo) >> sh;
    } else {
        out[0] = (3u * t[1] + t[2] + bo) >> sh; out[1] = (3u * t[2] + t[1] + be) >> sh;
        out[2] = (3u * t[2] + t[3] + bo) >> sh; out[3] = (3u * t[3] + t[2] + be) >> sh;
    }
}
// lane = the destination pixels dx .. dx + 3 of destination row dy: nothing outside out_w x out_rows (the clip to the rectangle included)
template <int MODE, bool RGB, class IO>
JDA_HD void jda_exr_quad(IO &io, const jda_ex_desc &X, const jda_exr_rec &R, uint32_t kh, uint32_t kv, uint32_t dx, uint32_t dy)
{
    if (dy >= X.out_rows || dx >= X.out_w) return;
    const uint32_t n = X.out_w - dx < 4u ? X.out_w - dx : 4u, sx = R.x + dx, sy = R.y + dy;
    const uint32_t yw = jda_exr_row4(io, X.plane[0], sy * X.pitch_y, sx, n, R.x, R.x + R.w);
    if (X.gray_out) {
        const uint32_t o = dy * X.out_pitch + dx;
        if (n == 4u) io.st32(X.out, o, yw);
        else for (uint32_t k = 0; k < n; k++) io.st8(X.out, o + k, (yw >> (8u * k)) & 255u);
        return;
    }
    uint32_t cb[4] = { 128u, 128u, 128u, 128u }, cr[4] = { 128u, 128u, 128u, 128u }, px[4];
    if (MODE != JDA_MODE_GRAY) {
        jda_exr_chroma4(io, X, R, X.plane[1], kh, kv, sx, sy, n, cb);
        jda_exr_chroma4(io, X, R, X.plane[2], kh, kv, sx, sy, n, cr);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++)
        px[k] = RGB ? ((yw >> (8u * k)) & 255u) | ((cb[k] & 255u) << 8) | ((cr[k] & 255u) << 16) | 0xff000000u : jda_ex_rgba((yw >> (8u * k)) & 255u, cb[k] & 255u, cr[k] & 255u);
    const uint32_t o = dy * X.out_pitch + dx * 4u;
    if (n == 4u) io.st128(X.out, o, px);
    else for (uint32_t k = 0; k < n; k++) io.st32(X.out, o + 4u * k, px[k]);
}
// a wavefront = a tile record of the destination rectangle: the quads 64 mcu_x0 .. of the rows 32 mcu_y .., inside the clip
template <int MODE, bool RGB, class IO> JDA_HD void jda_exr_colour_tile(IO &io, const jda_ex_desc &X, const jda_exr_rec &R, const jda_strip &S, uint32_t lane)
{
    typedef jda_ex_layout<MODE> E;
    const uint32_t q0 = (uint32_t)S.mcu_x0 * JDA_EXR_TILE_QUADS, dy0 = (uint32_t)S.mcu_y * JDA_EXR_TILE_ROWS, all = (X.out_w + 3u) >> 2;
    if (dy0 >= X.out_rows || q0 >= all) return;                  // (wave-uniform)
    const uint32_t quads = all - q0 < JDA_EXR_TILE_QUADS ? all - q0 : JDA_EXR_TILE_QUADS;
    const uint32_t rows = X.out_rows - dy0 < JDA_EXR_TILE_ROWS ? X.out_rows - dy0 : JDA_EXR_TILE_ROWS, items = quads * rows;
    uint32_t kh, kv;
    jda_exr_kinds((uint32_t)E::HS, (uint32_t)E::VS, X.scale, X.up, X.cw, &kh, &kv);
    for (uint32_t it = lane; it < items; it += 64u) {
        const uint32_t r = it / quads, q = it - r * quads;
        jda_exr_quad<MODE, RGB>(io, X, R, kh, kv, 4u * (q0 + q), dy0 + r);
    }
}

#endif // JDA_DEVICE_CORE_H
