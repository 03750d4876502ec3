// jda_internal.h -- structures shared by the host front end, the device runtime and the kernels.
#ifndef JDA_INTERNAL_H
#define JDA_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/jpegdec_amd.h"

// ---- table blob uploaded per image (16-byte aligned, one contiguous copy into LDS) ----
// layout mirrors what the reference keeps in JPEGIMAGE (src/JPEGDEC.h:235-238) so that the
// kernels index the LUTs exactly like JPEGDecodeMCU does (jpeg.inl:2129-2136, 2231-2236).
#define JDA_TB_DC        0        // 2 x 1024 bytes   (ucHuffDC)
#define JDA_TB_AC        2048     // 2 x 2048 uint16  (usHuffAC)
#define JDA_TB_QUANT     10240    // 4 x 64 int16     (sQuantTable after JPEGFixQuantD)
#define JDA_TB_ZIGZAG    10752    // 64 bytes         (cZigZag2: zigzag position -> natural index)
#define JDA_TB_EOB       10816    // 2 x uint32       (ours: the end-of-block code of each AC table, (32 - length) << 16 | code,
                                  //                   so that P1 recognises EOB by comparing stream bits; JDA_EOB_NONE = no such code)
#define JDA_EOB_NONE     ((31u << 16) | 2u)      // a one-bit field never reads 2
#define JDA_TABLE_BYTES  10832

#define JDA_SCAN_PAD     32       // zero bytes after the filtered scan (window loads overrun)
#define JDA_INDEX_OFF_BITS 7      // index entry (format 2) = (byte position << 7) | flags/bit offset: the reference's bit reader at the block's
                                  // FIRST AC SYMBOL, behind the refill at the top of its AC loop (jpeg.inl:2225-2230; bit offset 0..47 in bits
                                  // 5:0), bit 6 = JDA_INDEX_TRUNC; the block's own DC value rides beside it (blk_dc).  (The closing entry behind
                                  // the last block bounds the scan: the reader as the last block left it, offset 0..64, no flag -- or, from the
                                  // device pre-scan, up to 41 bits further on.)
#define JDA_INDEX_TRUNC 0x40u     // the reference truncates a magnitude read of this block: P1 must follow its ulBitOff
// Continuation entries (optional part of the index): a long block can be entered every JDA_CONT_SYMS AC symbols, so that several lanes
// of P1 share it -- the wavefront runs as long as its longest CHUNK, not its longest block (photographs: luma blocks of 40 symbols beside
// chroma blocks of 4).  blk_cont_first[g] .. blk_cont_first[g + 1] are block g's entries in blk_cont; an entry: the bit position of
// its first symbol relative to the block's first AC symbol (bits 11:0), the zigzag index of its first coefficient (bits 17:12), the low
// seven bits of the block's ordinal (bits 24:18: which lane of a tile owns it).  A block flagged JDA_INDEX_TRUNC is decoded whole.
#define JDA_CONT_SYMS 8u
#define JDA_CONT_ENTRY(rel, k, g) ((uint32_t)(rel) | ((uint32_t)(k) << 12) | (((uint32_t)(g) & 127u) << 18))
#define JDA_CONT_REL(e) ((e) & 0xfffu)
#define JDA_CONT_K(e) (((e) >> 12) & 63u)
#define JDA_CONT_G7(e) (((e) >> 18) & 127u)

// ---- the segment walk's 11-bit table key (jda_device_core.h, JDA_WT_*) and the reference's DC LUT index, shared with the front end
#if defined(__HIPCC__)
#define JDA_HD_INLINE __host__ __device__ static inline
#else
#define JDA_HD_INLINE static inline
#endif
// the reference's DC LUT index for the 12 stream bits code12 (jpeg.inl:2129-2136: short half by the top 6 bits; codes 11111..: 128 + the low 7 bits)
JDA_HD_INLINE uint32_t jda_dc_lut_index(uint32_t code12) { return code12 >= 0xf80u ? (code12 & 0xffu) : (code12 >> 6); }
// the 12 stream bits an 11-bit walk key stands for (low: the two bits a short key does not have)
JDA_HD_INLINE uint32_t jda_walk_key_code12(uint32_t key, uint32_t low) { return key < 1024u ? ((key << 2) | low) : (0xfc0u | ((key - 1024u) >> 4)); }
// Can the walk's DC tables stand for DC LUT t of the blob?  Only a short key of the form 111110xxxx leaves bits the reference
// looks at (it takes 12) undetermined: it must not matter what they are.
static inline int jda_dc_lut_walkable(const uint8_t *tables, uint32_t t)
{
    const uint8_t *dc = tables + JDA_TB_DC + t * 1024u;
    for (uint32_t key = 992u; key < 1008u; key++) {
        const uint32_t i0 = jda_dc_lut_index(jda_walk_key_code12(key, 0u));
        for (uint32_t low = 1; low < 4u; low++) {
            const uint32_t i = jda_dc_lut_index(jda_walk_key_code12(key, low));
            if (dc[i] != dc[i0] || dc[i + 512u] != dc[i0 + 512u]) return 0;
        }
    }
    return 1;
}

// Measuring switches (environment variables that change what a build does) exist only in laboratory builds: make lib EXTRA=-DJDA_LAB.
// The product library reads JPEGDEC_AMD_DEVICE (which GPU the drop-in class uses) and nothing else.
#ifdef JDA_LAB
#include <stdlib.h>
#define JDA_LAB_ENV(name) getenv(name)
#else
#define JDA_LAB_ENV(name) ((const char *)0)
#endif

// kinds of MCU the kernels are specialised for
enum { JDA_MODE_GRAY = 0, JDA_MODE_444 = 1, JDA_MODE_420 = 2, JDA_MODE_422 = 3 /* h2v1, MCU 16x8 */, JDA_MODE_440 = 4 /* h1v2, MCU 8x16 */, JDA_N_MODES = 5 };

// Pointers stored in descriptors are loaded from memory, so the compiler cannot know they point to
// global memory and would emit slow generic (flat_*) accesses; device code casts them with JDA_G().
#if defined(__HIP_DEVICE_COMPILE__)
#define JDA_GLOBAL __attribute__((address_space(1)))
#else
#define JDA_GLOBAL
#endif
#define JDA_G(T, p) ((T JDA_GLOBAL *)(p))

// ---- device-side descriptors ----
struct jda_dev_desc {             // one per image of a batch, 104 bytes
    const uint8_t *scan;          // filtered entropy-coded bytes (4-byte aligned, padded)
    const uint32_t *blk_index;    // n_blocks+1 entries: (byte position << 7) | bit offset at each block's first AC symbol
    const int16_t *blk_dc;        // n_blocks: the block's own DC value
    const uint8_t *tables;        // JDA_TABLE_BYTES
    uint8_t *out;                 // output surface
    const uint32_t *blk_cont_first;   // continuation entries (JDA_CONT_*; NULL: the image has none / is decoded block by block): n_blocks + 1 offsets ..
    const uint32_t *blk_cont;         // .. into the entries
    uint32_t out_pitch;           // bytes
    uint32_t out_w, out_rows;     // clip in output pixels / rows
    uint32_t mcus_x, mcus_y;
    uint32_t n_mcus_ok;           // MCUs the pre-scan validated (others are not decoded)
    uint32_t scan_len;
    uint32_t strip_mcus;          // != 0: the surface is STRIP-MAJOR -- the JPEGDRAW strips of the reference's callback (jpeg.inl:5300-5336), strip_mcus MCUs
                                  // wide and one MCU row high, in raster order, each strip's pixels contiguous (pitch = the strip's own width), a strip
                                  // every strip_mcus x MCU width x MCU height x bytes per pixel; out_pitch then only bounds the surface
    union {                       // 16 bytes of small fields; the kernels carry them as four dwords in SGPRs (cfg)
        struct {
            uint8_t mode;                 // JDA_MODE_*
            uint8_t ncomp;
            uint8_t pixel_type;           // JDA_RGB565_* / RGB8888 / EIGHT_BIT_GRAYSCALE (after LUMA_ONLY folding)
            uint8_t scale_shift;          // 0..3
            uint8_t dc_id[3], ac_id[3], q_id[3];
            uint8_t gray_from_color;      // colour JPEG decoded to GRAY8: chroma blocks are not decoded
            uint8_t fast_mul;             // 1: every IDCT multiply operand fits 24 bits (host-checked bound)
            uint8_t pad_[1];
        };
        uint32_t cfg[4];
    };
};

// descriptor byte pad_[0]: bits 1:0 profiling switches, bit 2 below, bit 3 = the scan holds DC symbols only (the first scan of a
// progressive file, decoded as a thumbnail: jpeg.inl:4964-4966), bits 7:4 = Al, the point transform of those DC differences
#define JDA_DESC_DC_ONLY 8u
// bit 2 = P1 must take its general bit reader: an AC table codes the end-of-block symbol more than once (a malformed but
// decodable DHT), so one compare of stream bits cannot recognise EOB
#define JDA_DESC_GENERAL_P1 4u

struct jda_strip {                // one wavefront's tile: <= 64 consecutive blocks (10/21/64 MCUs) of one MCU row; 16 bytes
    uint32_t image;               // index into the descriptor array
    uint16_t mcu_y;               // (a JPEG has at most 65535 / 8 MCU rows and columns)
    uint16_t mcu_x0;
    uint8_t count;                // MCUs in the tile (0 = padding entry)
    uint8_t first;                // 1: the first tile of its image (the wavefront that draws it restages the tables)
    uint16_t pad_;
    uint32_t ord;                 // which set of tables, counted along this launch's tile list (0, 1, 2, ..): the image's own position in the list unless
                                  // consecutive images share their tables (jda_pipeline: the workgroups then pass from one to the next without restaging)
};

// device marker / stuffing filter (jda_filter_scan), one per image
struct jda_filter_params {
    const uint8_t *raw;          // unfiltered entropy-coded segment (from the first SOS payload byte to the end of the file)
    uint8_t *out;                // filtered scan (zero-initialised by the caller: the padding behind it stays zero)
    uint32_t *restart_pos;       // [0] = 0, then the filtered offset at which each RSTn marker stood (first restart_cap entries)
    uint32_t *result;            // [0] filtered length, [1] number of RSTn markers
    uint32_t raw_len, restart_cap;   // raw_len: bytes from `raw` on, the skipped ones included
    uint32_t *work;              // JDA_FILTER_WORK_BYTES(raw_len): the chunks' transition functions and entry values
    uint32_t raw_skip;           // 0..15 bytes at `raw` that are not the stream's: `raw` is 16-byte aligned, a file that the copy engine took from where the
    uint32_t pad_;               // caller had it (JDA_SUBMIT_PINNED_INPUT) keeps its alignment -- its first byte is raw[raw_skip]
};
#define JDA_FILTER_WORK_BYTES(raw_len) (((size_t)(raw_len) / 16384u + 1u) * 20u)


// The tile list of a whole image, made where it is used (jda_pipeline: the lists of a batch of 64 x 4096x4096 are 6.8 MB -- written by
// the host and carried over the bus they were 6 % of a batch's traffic): one of these per image, the kernel writes the records
struct jda_strips_params {
    jda_strip *dst;              // the image's place in its launch list (n_padded records)
    uint32_t n_padded;           // tiles, padded to whole workgroups with empty records
    uint32_t image, ord;
    uint32_t mcus_x, mcus_y, per;   // per: MCUs in a tile (jda_mcus_per_tile)
};

// Slots a 256-byte segment's block records need (RECORD mode of the device pre-scan, jda_device_core.h): more than its 2,048 bits
// can start blocks.  mcu_min_bits: the fewest bits an MCU of the image can take -- per block the shortest DC code + the shorter of
// the EOB code and four of the shortest AC codes (63 coefficients take at least four symbols) -- from the DHT segments
// (jda_frontend.cpp).  A multiple of four (records are stored in 16-byte groups).
#ifndef JDA_SEG_BYTES
#define JDA_SEG_BYTES 256u           // the device pre-scan's segment: one lane walks one (jda_device_core.h)
#endif
static inline uint32_t jda_record_cap(uint32_t mcu_min_bits, uint32_t nblocks)
{
    if (mcu_min_bits < 2u * nblocks) mcu_min_bits = 2u * nblocks;
    return (((JDA_SEG_BYTES * 8u) / mcu_min_bits + 2u) * nblocks + 4u + 3u) & ~3u;
}

// What the host makes of one file when the GPU does everything else (jda_pipeline): see jda_front_prepare in jda_frontend.cpp
struct jda_front {
    jda_image_info info;
    uint8_t dc_id[3], ac_id[3], q_id[3];
    uint8_t general_p1;          // JDA_DESC_GENERAL_P1
    uint8_t progressive;
    uint8_t device_ok;           // filter + pre-scan can run on the device (else: the serial host path)
    uint8_t fast_provable;       // the 24-bit-multiply bound holds for every legal stream with these quantisers
    uint32_t raw_off, raw_len;   // the entropy-coded segment inside the file (unfiltered)
    uint32_t n_intervals;        // restart intervals (0: no DRI)
    uint32_t rec_cap;            // jda_record_cap of the image's tables
    uint8_t raw_q_id[3], adobe;  // the frame header's quantiser ids as they stand; the file has an Adobe APP14 segment
    uint16_t quant_zz[4][64];    // the DQT entries as the file lists them, by table id (zigzag order)
    uint8_t colour;              // JDA_CS_*: how libjpeg reads the components (jda_colour_model)
};

// jdapimin.c's default_decompress_parms: the colour model libjpeg gives a file.  jfif: an APP0 "JFIF" segment was seen;
// adobe: an APP14 "Adobe" one, transform its flag byte; ids: the frame header's component ids.
static inline int jda_colour_model(int ncomp, int jfif, int adobe, int transform, const int *ids)
{
    if (ncomp == 1) return JDA_CS_GRAY;
    if (ncomp == 3) {
        if (jfif) return JDA_CS_YCBCR;
        if (adobe) return transform == 0 ? JDA_CS_RGB : JDA_CS_YCBCR;
        return ids[0] == 0x52 && ids[1] == 0x47 && ids[2] == 0x42 ? JDA_CS_RGB : JDA_CS_YCBCR;
    }
    if (ncomp == 4) return adobe && transform != 0 ? JDA_CS_YCCK : JDA_CS_CMYK;
    return -1;
}

// One image of a dither launch (device pointers): gray = canvas_w x canvas_h bytes at gray_pitch (16-byte aligned rows), out = packed
// rows at out_pitch (a multiple of 4, >= jda_dither_pitch)
struct jda_dither_job {
    const uint8_t *gray;
    uint8_t *out;
    const uint8_t *seed;   // JDA_DITHER_SEED_BYTES the error row starts from (device), or NULL: zeros
    uint32_t gray_pitch, out_pitch, width, height, strip_rows, bits;
};

// One surface of an orient launch (device pointers): src = the visible rectangle of a decoded canvas, width x height pixels of the
// launch's pixel size at src_pitch; dst = the oriented rectangle (jda_orient_dims) at dst_pitch.  Both 16-byte aligned, both pitches
// multiples of 16.  tile0: the index of the surface's first tile in the launch's flat tile list, tiles_x: tiles across the destination.
struct jda_orient_job {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t src_pitch, dst_pitch, width, height, orientation, tile0, tiles_x, pad_;
};

// One image of a pack launch (device pointers): src = a decoded surface (16-byte aligned, src_pitch a multiple of 16) of the launch's
// pixel size, {x, y, w, h} = the pixel rectangle that is packed; dst = the dense destination, aligned to its element.  tile0: the index
// of the job's first tile in the launch's flat tile list.
struct jda_pack_job {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t src_pitch, x, y, w, h, tile0;
};

// One image of an unpack launch (device pointers): src = the dense image (w * h * C elements, aligned to its element), dst = the surface
// it becomes (16-byte aligned, dst_pitch a multiple of 16) of the launch's pixel size, w x h pixels.  tile0: the index of the job's
// first tile in the launch's flat tile list.
struct jda_unpack_job {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t dst_pitch, w, h, tile0;
};

// One image of a resize launch (device pointers): src = a decoded surface of the launch's pixel size (16-byte aligned, src_pitch a
// multiple of 16), dst = out_w x out_h pixels at dst_pitch, the same.  htab / vtab: where the job's tap tables of the two axes begin in
// the launch's table block, in dwords (the layout of a table: jda_rs_* in jda_device_core.h; the rectangle is in the taps' coordinates,
// so the job carries none); hk / vk: their coefficients per output coordinate.  tile0: the index of the job's first tile in the launch's
// flat tile list, tiles_x: tiles across the destination, th: output rows of a tile.
struct jda_resize_job {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t src_pitch, dst_pitch, out_w, out_h, htab, vtab, hk, vk, tile0, tiles_x, th, pad_;
};

// One image of a reduce launch (device pointers; jda_rd_* in jda_device_core.h): the box {x0, y0, bw, bh} (pixels) of the
// surface at src (16-byte aligned, src_pitch a multiple of 16) averaged over cells of fx x fy pixels into out_w x out_h =
// ceil(bw / fx) x ceil(bh / fy) pixels at dst, the same alignment.  tile0: the index of the job's first tile in the launch's flat tile
// list, tiles_x: tiles across the destination, th: output rows of a tile, row_entries: the LDS entries (8 bytes) of one of them.
// mul[e]: floor(2^24 / n) of a cell of n pixels -- e = 0: a whole cell, 1: the narrower cells of the last column, 2: the lower cells of
// the last row, 3: the corner cell of both (the values of a kind the box has none of are never read).
struct jda_reduce_job {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t src_pitch, dst_pitch, x0, y0, bw, bh, fx, fy, out_w, out_h, tile0, tiles_x, th, row_entries;
    uint32_t mul[4];
};

// One image of an encode call (device pointers; jda_en_* in jda_device_core.h): the rectangle {x, y, w, h} of the surface
// at src becomes a baseline file at dst.  hs x vs: luma blocks of an MCU (1 x 1 with nc = 1: gray); cx x cy MCUs of bpm blocks; wb x hb:
// the luma blocks that hold a pixel (the others of the MCU grid are dummies); ri: the restart interval in MCUs.  The job's blocks are
// [block0, block0 + n_blocks) of the call's flat list, in the order of the scan; its intervals' first bytes lie at istart[int0 ..
// int0 + n_int); quant: its record in the call's quantisers; its header: hdr_len bytes at hdr_off of the header blob.  Known once the
// lengths are (the second upload): u_off, where its unstuffed scan lies in the call's stream buffer (a multiple of 64), and [chunk0,
// chunk0 + n_chunks) of the flat list of 64-byte chunks, the first h_chunks of them the header's.  huff_off: where the job's code words lie
// in the call's word tables, in dwords (0: the Annex K tables every standard job uses); hist_off: where its symbol histogram lies in the
// call's histograms, in dwords (~0u: the job is not optimised and has none).  An optimised job's header is made once its histogram is known.
struct jda_encode_dev_job {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t capacity, u_off;
    uint32_t src_pitch, x, y, w, h, hs, vs, nc, cx, cy, bpm, wb, hb, ri, block0, n_blocks, quant, hdr_off, hdr_len, int0, n_int, chunk0, n_chunks, h_chunks, huff_off, hist_off;
};
struct jda_encode_quant { uint32_t recip[2][64]; uint32_t half[2][64]; };      // natural order, per table: ceil(2^32 / (8 q)) and (8 q) >> 1
struct jda_encode_totals { uint64_t u_bytes, file_bytes; };                    // per job: its unstuffed scan, its whole file
#define JDA_EN_HUFF_DWORDS 544u           // (length << 16) | code: AC symbol rs of table t at [t * 256 + rs], DC category s at [512 + t * 16 + s]
#define JDA_EN_CHUNK 64u                  // bytes of a stuffing chunk
#define JDA_EN_BLOCK_BITS 1665u           // no block's code is longer
#define JDA_EN_NO_HIST 0xffffffffu        // jda_encode_dev_job.hist_off of a job that keeps the Annex K tables
#define JDA_EN_OPT_MAX_BLOCKS 15625000u   // of an optimised job: 64 symbols a block at the most, and no count may pass libjpeg's 10^9
enum { JDA_EN_STAGE_BLOCKS = 0, JDA_EN_STAGE_LENGTHS, JDA_EN_STAGE_SCAN_BITS, JDA_EN_STAGE_EMIT, JDA_EN_STAGE_COUNT, JDA_EN_STAGE_SCAN_BYTES, JDA_EN_STAGE_WRITE, JDA_EN_STAGES };
// the two stages an optimised job adds (jda_huffopt_*): gather runs behind lengths, huffopt_lengths in front of the scan
enum { JDA_EN_STAGE_GATHER = JDA_EN_STAGES, JDA_EN_STAGE_OPT_LENGTHS, JDA_EN_STAGES_OPT };

// The source of one job of a recode call (jda_rc_* in jda_device_core.h; device pointers): a resident baseline image --
// its filtered scan (scan_len bytes and JDA_SCAN_PAD zeros), block index and DC values (index format 2) and table blob, ac_id[c] the AC
// table of component c -- or a resident dense coefficient image (coef: 64 x int16 a block, natural order).  The job's record in the
// call's jda_encode_dev_job list carries the shape; its src is NULL.
enum { JDA_RC_IMAGE = 0, JDA_RC_COEF = 1 };
struct jda_rc_src {
    const uint8_t *scan;
    const uint32_t *blk_index;
    const int16_t *blk_dc;
    const uint8_t *tables;
    const int16_t *coef;
    uint32_t scan_len, kind, ac_id[3], pad_;
};
// The transform of one job of a recode call whose stage is jda_rc_extract_xf / jda_rc_from_coef_xf.  The job's REGION is
// rw x rh MCUs of the source's grid (scx MCUs across) from MCU (x0, y0): what the crop and the trim leave.  bits: JDA_RC_XF_T the blocks and
// their coefficients are transposed, then JDA_RC_XF_MX / _MY the TARGET's x / y axis is mirrored.  The job's record in the call's
// jda_encode_dev_job list carries the target's shape: cx x cy = rw x rh, or rh x rw where transposed (then hs == vs).
#define JDA_RC_XF_T 1u
#define JDA_RC_XF_MX 2u
#define JDA_RC_XF_MY 4u
struct jda_rc_xf { uint32_t bits, scx, x0, y0, rw, rh, pad_[2]; };
#define JDA_RC_MAX_AC 1023                // a recoded block: |AC| <= 1023 and -1024 <= DC <= 1023, else its job is refused
#define JDA_RC_MIN_DC (-1024)
#define JDA_RC_MAX_DC 1023

// One image of a libjpeg-exact decode call (jda_ex_* in jda_device_core.h; device pointers), beside its jda_dev_desc in the
// call's blob.  plane[c]: the 8-bit samples of Y, Cb, Cr in the call's scratch, each padded to the MCU grid, the rows pitch_y / pitch_c
// bytes apart (multiples of 16); w x h: the image, cw x ch: a chroma component's own extent (ceil(w / hs) x ceil(h / vs)).  out: the
// surface, of which out_w x out_rows pixels are written (the clip to the image included); gray_out: it is 8-bit gray (the Y plane), else
// RGB8888.  luma_only: the chroma blocks are not decoded (a gray surface of a colour file).  quant: the RAW DQT entries of Y, Cb, Cr in
// NATURAL order -- not the prescaled quantisers of the coefficient image's own blob.
struct jda_ex_desc {
    uint8_t *plane[3];
    uint8_t *out;
    uint32_t pitch_y, pitch_c, w, h, cw, ch, out_pitch, out_w, out_rows, gray_out, luma_only;
    // a four-component image (jda_exact_colour4; zero in every other record, where the word was padding): JDA_EX4_* bits
    uint32_t cs4;
    uint16_t quant[3][64];
    // a scaled decode (jda_exs_*; zeros in a record of the full-size kernels): scale 2, 4 or 8 -- w x h, cw x ch, the pitches
    // and the clip are then the scaled ones, a plane's blocks ss x ss samples each --, up: what jdsample.c does to the chroma planes (JDA_EX_UP_*)
    uint32_t scale, up;
    // a four-component image: component 3's samples (in the place of eight bytes of padding: a record of the other calls is what it was,
    // byte for byte) -- rows pitch_y apart and w x h samples where JDA_EX4_K_FULL says component 0's sampling, else pitch_c and cw x ch.
    // Its quantisers are in the record of its own gray tiles (the planes stage decodes it as a gray image into this plane).
    uint8_t *plane3;
};
static_assert(sizeof(jda_ex_desc) == 480 && offsetof(jda_ex_desc, plane3) == 472 && offsetof(jda_ex_desc, quant) == 80, "the record the exact kernels read stays as it was");
#define JDA_EX4_YCCK 1u          // components 0..2 are YCbCr (jdcolor.c's conversion in front of the inversion), else C, M, Y as they stand
#define JDA_EX4_K_FULL 2u        // component 3 has component 0's sampling, else 1x1 (a chroma plane's geometry)
#define JDA_EX4_CMYK_OUT 4u      // the surface is JDA_CMYK8888 (Pillow's mode-"CMYK" bytes), else JDA_RGB8888 (its convert("RGB"))
// A resident baseline image as the source of an exact call, beside its jda_dev_desc and jda_ex_desc in the call's blob (a record an image
// of the call; zeros for a coefficient image): what the planes stage's baseline load phase reads -- S as a recode source's; bpm blocks an
// MCU, the first nluma of them luma.
struct jda_ex_src {
    jda_rc_src S;
    uint32_t bpm, nluma, pad_[2];
};

// Progressive encode (jda_pe_* in jda_device_core.h, DESIGN.md 5.13 rules 10 to 14).  A SEGMENT is one scan of one job: its units -- a
// (scan, block) pair each -- are [unit0, unit0 + n_units) of the call's flat unit list, the job's scans in file order.  comp: the scan's
// component (JDA_PE_ALL: every block of the MCU grid in the job's block order, a DC scan); wbc: the blocks in a row of the component's own
// extent; ss, se, ah, al as its SOS states them; tab: where the scan's code words -- and its histogram -- lie in the call's tables, in
// dwords, JDA_PE_TAB_DWORDS a scan ((length << 16) | code: an AC scan's symbol rs at [rs], the first DC scan's category s of table t at
// [t * 16 + s]).  Known once the lengths are: the scan's header (DHTs and SOS; the first scan's: everything from SOI) at hdr_off of the
// header blob, [chunk0, chunk0 + n_chunks) of the flat chunk list, the first h_chunks the header's, and u_off, where its unstuffed data lie.
struct jda_pe_seg {
    uint64_t u_off;
    uint32_t unit0, n_units, job, comp, wbc, ss, se, ah, al, tab, hdr_off, hdr_len, chunk0, n_chunks, h_chunks, pad;
};
struct jda_pe_job { uint32_t seg0, n_segs, chunk0, n_chunks; };                // a job's segments and chunks in the flat lists
#define JDA_PE_ALL 3u
#define JDA_PE_TAB_DWORDS 256u
#define JDA_PE_MAX_SCANS 10u
#define JDA_PE_BLOCK_BITS 3928u           // no block adds more to a file, all its scans together (the derivation: DESIGN.md 5.13 rule 14)
#define JDA_PE_SCAN_HDR 568u              // no scan's DHTs and SOS are longer: two tables of 4 + 17 + 256 bytes, 14 bytes of SOS
#define JDA_PE_FILE_HDR 200u              // SOI, APP0, two DQTs, SOF2: 2 + 18 + 138 + 19 = 177
// the stages of a call, in the order they run (blocks and lengths are jda_encode_blocks and jda_encode_lengths as they stand)
enum { JDA_PE_STAGE_BLOCKS = 0, JDA_PE_STAGE_DC, JDA_PE_STAGE_CLASSIFY, JDA_PE_STAGE_RESOLVE, JDA_PE_STAGE_GATHER, JDA_PE_STAGE_LENGTHS, JDA_PE_STAGE_SCAN_BITS,
       JDA_PE_STAGE_EMIT, JDA_PE_STAGE_COUNT, JDA_PE_STAGE_SCAN_BYTES, JDA_PE_STAGE_WRITE, JDA_PE_STAGES };

#endif
