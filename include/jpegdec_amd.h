/* include/jpegdec_amd.h -- C-ABI of the MI355X-native baseline-JPEG decode path.
 *
 * This is the drop-in boundary for ONE hot path of bitbank2/JPEGDEC: the per-MCU loop of
 * DecodeJPEG (reference src/jpeg.inl:5109-5353: JPEGDecodeMCU -> JPEGIDCT -> JPEGPutMCU*).
 * Plain C types only: no C++, no exceptions, no torch types cross this boundary.  The reference
 * API (openRAM/openFLASH/decode()/JPEG_DRAW_CALLBACK, include/JPEGDEC.h here) is implemented on
 * top of these entry points; INTEGRATION.md shows the binding a maintainer of the reference
 * would add at jpeg.inl:5109.
 *
 * Stages and the reference code each entry point replaces (paths relative to the reference):
 *   jda_parse        host   JPEGParseInfo + JPEGGetSOS + JPEGGetHuffTables   src/jpeg.inl:1572-1785, 1378-1425, 837-873
 *   jda_prepare      host   JPEGMakeHuffTables, JPEGFilter over the whole scan, JPEGFixQuantD and the serial
 *                           entropy pre-scan (JPEGDecodeMCU in skip mode)    src/jpeg.inl:1066-1275, 1431-1540, 1789-1811, 2090-2274
 *   jda_upload       H2D    (no reference equivalent: the reference streams 2 KiB at a time, :1544-1566)
 *   jda_batch_decode GPU    the MCU loops of DecodeJPEG for every image of a batch   src/jpeg.inl:5109-5353
 *                           = JPEGDecodeMCU :2090-2274, JPEGIDCT :2278-2798 (+ DC-only bypass :5146-5154),
 *                             JPEGPutMCU8BitGray/Gray/11/22 :2799-4544, JPEGPixel* :3101-3278
 *
 * Conventions: functions returning int return JDA_SUCCESS (0) or one of the JDA_* error codes,
 * whose values equal the reference's enum (src/JPEGDEC.h:119-126) so getLastError() can pass
 * them through.  Every GPU entry point fails with JDA_ERROR_NO_DEVICE when no HIP device is
 * usable -- there is no CPU fallback in this library.
 */
#ifndef JPEGDEC_AMD_H
#define JPEGDEC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JDA_ABI_VERSION 1

/* error codes: 0..5 are the reference's (src/JPEGDEC.h:119-126) */
enum {
    JDA_SUCCESS = 0,
    JDA_INVALID_PARAMETER = 1,
    JDA_DECODE_ERROR = 2,
    JDA_UNSUPPORTED_FEATURE = 3,
    JDA_INVALID_FILE = 4,
    JDA_ERROR_MEMORY = 5,
    JDA_ERROR_NO_DEVICE = 6,   /* no usable HIP device / runtime error (detail: jda_last_hip_error) */
    JDA_ERROR_HIP = 7
};

/* pixel types: the reference's enum (src/JPEGDEC.h:102-111) */
enum {
    JDA_RGB565_LITTLE_ENDIAN = 0,
    JDA_RGB565_BIG_ENDIAN = 1,
    JDA_RGB8888 = 2,            /* memory order R,G,B,A as the reference's scalar path (jpeg.inl:3162-3175) */
    JDA_EIGHT_BIT_GRAYSCALE = 3,
    /* error-diffused 4 / 2 / 1 bits per pixel (JPEGDither, jpeg.inl:4871-4940): not decode targets of jda_batch_create / jda_decode_to_host
     * (jda_output_geometry refuses them); made from a GRAY8 canvas by jda_dither_surfaces / jda_decode_dither_to_host */
    JDA_FOUR_BIT_DITHERED = 4,
    JDA_TWO_BIT_DITHERED = 5,
    JDA_ONE_BIT_DITHERED = 6
};

/* decode options: the reference's bits (src/JPEGDEC.h:68-75) */
enum {
    JDA_SCALE_HALF = 2,
    JDA_SCALE_QUARTER = 4,
    JDA_SCALE_EIGHTH = 8,
    JDA_LUMA_ONLY = 64,
    /* ours (the reference has nothing like it): decode EVERY scan of a progressive file to a full-size canvas instead of the 1/8
     * thumbnail of its first scan.  No effect on a baseline file.  With a JDA_SCALE_* bit: JDA_UNSUPPORTED_FEATURE.  Taken by
     * jda_decode_to_host / _ex / _flags (whole image); every other decode entry point -- jda_batch_create*, jda_pipeline_submit*,
     * jda_node_submit* (per image, in status[]), jda_decode_to_host_rect / _bands / _strips / _oriented / _packed / _resized, jda_decode_dither_to_host and
     * any call with an MCU rectangle -- answers JDA_UNSUPPORTED_FEATURE for a progressive file asked for with it.  The exceptions stand behind
     * doors of their own: jda_pipeline_submit_ex / jda_node_submit_ex with JDA_SUBMIT_PROGRESSIVE_FULL decode such a file at full size with its
     * batch (without the flag: JDA_UNSUPPORTED_FEATURE in status[], as ever), and jda_coef_decode_surfaces_rect decodes an MCU rectangle of a
     * coefficient image (jda_progressive_prepare + jda_coef_upload_ex). */
    JDA_PROGRESSIVE_FULL = 256
};

/* ------------------------------------------------------------------ host front end */

typedef struct jda_image_info {
    int32_t width, height;        /* SOF0 (jpeg.inl:1684-1685) */
    int32_t ncomp;                /* 1 or 3 */
    int32_t subsample;            /* reference ucSubSample: 0x00 gray, 0x11, 0x12, 0x21, 0x22 (jpeg.inl:1698-1713) */
    int32_t bpp;                  /* bits per sample * ncomp (jpeg.inl:1687) */
    int32_t jpeg_type;            /* 0 baseline, 1 progressive (src/JPEGDEC.h:94-99) */
    int32_t restart_interval;     /* DRI (jpeg.inl:1715-1718) */
    int32_t orientation;          /* EXIF tag 274 if present else 0 */
    int32_t mcu_w, mcu_h;         /* MCU size in source pixels */
    int32_t mcus_x, mcus_y;       /* MCU grid (jpeg.inl:5013-5037) */
    int32_t scan_offset;          /* byte offset of the entropy-coded data */
    int32_t blocks_per_mcu;       /* 1 gray, 3 for 4:4:4, 4 for 4:2:2 / 4:4:0, 6 for 4:2:0 (Y.. Cb Cr in scan order) */
    int32_t has_thumb;            /* EXIF IFD1 present (jpeg.inl:1667-1675) */
    int32_t thumb_w, thumb_h;     /* EXIF tags 256 / 257 (0 when absent, as in the reference) */
    int32_t thumb_offset;         /* file offset of the embedded thumbnail JPEG (tag 513 + TIFF base) */
    int32_t scan_start, scan_end; /* Ss, Se of the first scan (jpeg.inl:1416-1417) */
    int32_t approx;               /* Ah << 4 | Al of the first scan (jpeg.inl:1418-1420) */
} jda_image_info;

/* The option bits an image is really decoded with: a progressive file (jpeg_type 1) is decoded from its first (DC)
 * scan only, as a 1/8 thumbnail -- JPEG_SCALE_EIGHTH is OR-ed in (jpeg.inl:4964-4966) before the HALF / QUARTER /
 * EIGHTH chain (:4978-4990) picks the first bit that is set. */
int32_t jda_effective_options(const jda_image_info *info, int32_t options);
/* .. unless JDA_PROGRESSIVE_FULL is set: on a progressive file the bit is kept and JPEG_SCALE_EIGHTH is not OR-ed in; on a baseline
 * file the bit is cleared.  1 when the effective options carry the bit (the shared refusal check of the paths that lack it). */
int jda_progressive_full_requested(const jda_image_info *info, int32_t options);

/* Header parse only.  Accept/reject rules follow JPEGParseInfo (jpeg.inl:1572-1785). */
int jda_parse(const uint8_t *jpeg, int32_t len, jda_image_info *info);

/* An image made ready for the GPU (host memory): expanded Huffman LUTs, prescaled quant tables,
 * the filtered scan and the per-block index produced by the serial pre-scan. */
typedef struct jda_image jda_image;

/* Parse + table build + filter + pre-scan.  `options` are the JDA_SCALE_* / JDA_LUMA_ONLY bits the
 * image will be decoded with (they do not change the index; they are validated here).
 * Returns NULL on failure with *err set.  The JPEG buffer is not referenced after return. */
jda_image *jda_prepare(const uint8_t *jpeg, int32_t len, int32_t *err);

/* The same with options.  JDA_PREPARE_DEVICE_PRESCAN: skip the serial Huffman pre-scan on the host; the per-block
 * index is then made on the GPU when the image is uploaded (jda_upload / jda_upload_batch) by the segment walk --
 * one lane per 256-byte segment of the filtered scan, with or without restart markers (DRI, jpeg.inl:1715-1718,
 * 5337-5348) -- the same index as the serial pre-scan's in the sense of jda_index_equivalent.  The upload falls back to the host pre-scan by itself
 * when the walk cannot guarantee that (an invalid code, a marker out of place, states that do not settle); files the
 * walk cannot take at all (progressive, one restart interval, table ids 2-3, DC codes its table key cannot tell
 * apart) are pre-scanned here whatever the flag says: jda_image_prescan_pending tells. */
#define JDA_PREPARE_DEVICE_PRESCAN 1
/* Continuation entries (jda_image_block_cont) for every image the serial pre-scan indexes / for none; default: for the images in the
 * window of bits per block in which the decode kernel's chunked entropy phase was measured to pay (56 .. 112). */
#define JDA_PREPARE_CONT_ALWAYS 2
#define JDA_PREPARE_CONT_NEVER 4
/* The host pre-scan of a stream with restart intervals (>= 4 of them, >= 12 KB of scan) decodes its intervals side by side on a few
 * helper threads the library keeps (an interval starts at a marker with predictors zero; the reader's phase across intervals -- the
 * one thing that carries over, SURVEY fact 6 -- is settled afterwards); a stream without them (>= 16 KB of scan) is walked in chunks
 * from a guess, the true path spliced in front of where each walker fell into step.  Either way the same index as the serial
 * pre-scan's in the sense of jda_index_equivalent.  This flag keeps the pre-scan on the calling thread. */
#define JDA_PREPARE_SERIAL_PRESCAN 8
/* .. and this one takes the helper threads for every stream that admits it, whatever its size (the library's own size limits are where
 * the threads were measured to pay; tests use it on small files). */
#define JDA_PREPARE_PARALLEL_PRESCAN 16
jda_image *jda_prepare_ex(const uint8_t *jpeg, int32_t len, int32_t flags, int32_t *err);
/* The helper threads (process-wide): n < 0 as many as the library chooses (the default: up to five, none on fewer than four usable CPUs;
 * made at the first image that takes them, asleep unless one caller decodes image after image within 2 ms of each other), n == 0 none --
 * no thread is made, every pre-scan runs on its caller's thread --, n > 0 at most n in a job.  Returns the setting it replaces.
 * jda_prepare_batch's workers (threads > 1) and the pipeline's workers never use them. */
int jda_set_host_prescan_helpers(int32_t n);
/* jda_prepare_ex for n images on `threads` host threads (<= 0: as many as the process may keep busy -- hardware threads, its affinity mask, a cgroup quota); out[i] / errs[i] per image
 * (errs may be NULL).  Returns JDA_SUCCESS or the first error met. */
int jda_prepare_batch(int32_t n, const uint8_t *const *jpegs, const int32_t *lens, int32_t flags, int32_t threads,
                      jda_image **out, int32_t *errs);
/* 1 while the image's block index has not been made yet (deferred to jda_upload). */
int jda_image_prescan_pending(const jda_image *img);
void jda_image_free(jda_image *img);

const jda_image_info *jda_image_get_info(const jda_image *img);
/* views into the prepared image (owned by img): the filtered scan; the per-BLOCK index, FORMAT 2
 * (n_blocks+1 entries, n_blocks = mcus_x*mcus_y*blocks_per_mcu, scan order): (byte position << 7) | flag << 6 |
 * bit offset = the reference bit reader's state (bb.pBuf, bb.ulBitOff) at the block's FIRST AC SYMBOL, behind the
 * refill at the top of JPEGDecodeMCU's AC loop (jpeg.inl:2225-2230: offset 0..47); and the block's OWN DC value
 * (n_blocks int16: the pre-scan decoded the DC symbol, :2129-2165).  The decode kernel starts every block at
 * coefficient 1; a 1/8 or progressive thumbnail (:5146-5154, :4964-4966) reads the DC values and nothing else.
 * Flag (bit 6): the reference truncates a magnitude read of this block (its window is not refilled between a code and its
 * magnitude, :2249-2252) -- the kernel emulates that from the entry's exact (pBuf, ulBitOff).  The last entry closes
 * the index: a bit position at or behind the last block's last bit (see jda_index_equivalent).
 * *n_mcus_ok < mcus_x*mcus_y means the pre-scan hit an invalid code in that MCU (the reference
 * returns JPEG_DECODE_ERROR there, jpeg.inl:2137, 2237, 5354-5356). */
const uint8_t *jda_image_scan(const jda_image *img, uint32_t *len);
const uint32_t *jda_image_block_index(const jda_image *img, uint32_t *n_mcus_ok);
const int16_t *jda_image_block_dc(const jda_image *img);
/* The optional part of the index: continuation entries, one every 8 AC symbols of a long block, through which several lanes of
 * the decode kernel share it (photographs: luma blocks of forty symbols beside chroma blocks of four -- a wavefront runs as long as
 * its longest CHUNK then, not its longest block).  cont_first[g] .. cont_first[g + 1] (n_blocks + 1 offsets) are block g's entries in
 * the returned array of *n_cont entries: bits 11:0 the bit position of the entry's first symbol relative to the block's first AC
 * symbol, bits 17:12 the zigzag index of its first coefficient, bits 24:18 the low bits of g.  The serial pre-scan writes them for
 * the images JDA_PREPARE_CONT_* names; a decode to RGB8888 of a 4:2:0 or 4:4:4 image that has entries takes them. */
const uint32_t *jda_image_block_cont(const jda_image *img, const uint32_t **cont_first, uint32_t *n_cont);
/* Do two indexes of n_blocks + 1 entries (one from the serial pre-scan, one read back from the device: jda_dev_image_read_index,
 * jda_pipeline_read_index) name the same decode?  The contract between the two pre-scans: every block's entry has the same bit
 * position (byte position * 8 + bit offset) and the same flag; a FLAGGED block's entry is identical (the reference reader's exact
 * phase); an unflagged block's entry from the device is canonical -- (p >> 3) << 7 | (p & 7) for its bit position p -- where the
 * serial pre-scan stores the reader's phase; the closing entries lie within 41 bits of each other (the device's is behind the DC
 * symbol that the stream's padding decodes to, and rounded up to a byte in a stream with restart intervals).  Returns 1 / 0. */
int jda_index_equivalent(const uint32_t *a, const uint32_t *b, uint32_t n_blocks);
/* Which kernels of the library's code object this process has launched, and how often: "<kernel symbol> <launches>\n" per kernel
 * into buf (NUL-terminated, truncated at cap); returns the bytes the whole report needs.  (Diagnostics: the GPU test-suite
 * holds itself to every kernel the library ships.) */
int jda_kernel_launch_counts(char *buf, int cap);
/* Internal (tests, tools): the decode kernel deals the last quads of a launch that fills the GPU at run time ("the
 * pool").  jda_internal_set_decode_pool forces the launches' workgroup cap and the pool's share of the quads in 1/1000 (at most
 * 500), so that a small image runs the pool too -- a forced cap also lifts the rule that a workgroup's run is eight quads and more;
 * 0, 0 restores the defaults (one workgroup per CU, the built-in share).  Process-wide, for the launches made after it.
 * jda_internal_decode_pool_last: of the last launch of the decode kernel, once the caller has synchronised with it: out[0] the
 * quads in its pool (0: it had none), out[1] the claims its workgroups made, out[2] those that found the pool empty (one per
 * workgroup), out[3] the counter slot it used (-1: none).  JDA_ERROR_HIP if the launch did not leave its counters zeroed. */
int jda_internal_set_decode_pool(int32_t grid_cap_override, int32_t pool_permille);
int jda_internal_decode_pool_last(int32_t out[4]);
/* the table blob uploaded to the GPU: DC LUTs 2x1024 B, AC LUTs 2x2048 uint16, quant 4x64 int16, zigzag 64 B,
 * and (ours) the end-of-block code of each AC table, 2 x uint32 = (32 - length) << 16 | code */
const uint8_t *jda_image_tables(const jda_image *img, uint32_t *bytes);
/* number of places where the reference's un-refilled magnitude read drops low bits
 * (SURVEY.md fact 6); informational */
uint32_t jda_image_truncation_events(const jda_image *img);
/* 1: an AC table codes the end-of-block symbol more than once (malformed DHT; jpeg.inl:1066-1275 builds its LUTs per
 * code and decodes it all the same): the kernels then take their general bit reader; informational */
uint32_t jda_image_general_p1(const jda_image *img);

/* Geometry of the decoded surface for (pixel_type, options): bytes per pixel, and the
 * MCU-padded canvas size in output pixels (what the reference's draw callbacks tile). */
int jda_output_geometry(const jda_image_info *info, int32_t pixel_type, int32_t options,
                        int32_t *bytes_per_pixel, int32_t *out_w, int32_t *out_h,
                        int32_t *canvas_w, int32_t *canvas_h);

/* Draw-callback plan (jpeg.inl:5062-5084, 5300-5336): rects[6*i..] = x, y, iWidth, iHeight,
 * iWidthUsed, iBpp of every JPEGDRAW the reference issues.  Returns the count (or -1). */
int jda_draw_plan(const jda_image_info *info, int32_t pixel_type, int32_t options, int32_t max_mcus,
                  int32_t uses_dma, int32_t *rects, int32_t max_rects);

/* The same with a crop rectangle (JPEG_setCropArea, jpeg.inl:682-727; skip logic :5111, :5134-5137).
 * jda_crop_round applies the reference's MCU rounding to a request in place.  crop = {x, y, w, h}
 * already rounded, or NULL.  rects[8*i..] = x, y, iWidth, iHeight, iWidthUsed, iBpp, src_x, src_y with
 * (src_x, src_y) the strip's position in the decoded canvas. */
void jda_crop_round(const jda_image_info *info, int32_t *x, int32_t *y, int32_t *w, int32_t *h);
int jda_draw_plan_ex(const jda_image_info *info, int32_t pixel_type, int32_t options, int32_t max_mcus,
                     int32_t uses_dma, const int32_t *crop, int32_t *rects, int32_t max_rects);
/* The same for decode(xoff, ..): the reference's strip widths of a CROPPED decode depend on the x offset passed to decode()
 * (jpeg.inl:5328 compares jd.x, offset included, with iCropX + iCropCX).  rects as above, x / y relative to the offset. */
int jda_draw_plan_at(const jda_image_info *info, int32_t pixel_type, int32_t options, int32_t max_mcus,
                     int32_t uses_dma, const int32_t *crop, int32_t xoff, int32_t *rects, int32_t max_rects);

/* ------------------------------------------------------------------ device runtime */

typedef struct jda_ctx jda_ctx;        /* one per process per GPU: device, stream, events */
typedef struct jda_dev_image jda_dev_image; /* an image's inputs resident in HBM */
typedef struct jda_batch jda_batch;    /* a launch plan over many resident images */

int jda_device_count(void);
jda_ctx *jda_create(int32_t device, int32_t *err);
void jda_destroy(jda_ctx *ctx);
const char *jda_last_hip_error(const jda_ctx *ctx);
void *jda_stream(jda_ctx *ctx);        /* the hipStream_t every launch of this ctx goes to */

/* device memory helpers (so callers need no HIP binding of their own) */
/* Page-locked HOST memory (hipHostMalloc): a destination the copy back of jda_decode_to_host* reaches at link speed and truly
 * asynchronously -- what lets jda_decode_to_host_bands overlap the copy with the caller's work.  NULL when it cannot be had. */
void *jda_host_alloc(size_t bytes);
void jda_host_free(void *p);
/* page-lock memory the caller already has (a file cache, a receive buffer) for JDA_SUBMIT_PINNED_INPUT; undo before freeing it */
int jda_host_register(void *p, size_t bytes);
int jda_host_unregister(void *p);
void *jda_malloc(jda_ctx *ctx, size_t bytes);
void jda_free(jda_ctx *ctx, void *dptr);
int jda_memset(jda_ctx *ctx, void *dptr, int value, size_t bytes);
int jda_copy_to_host(jda_ctx *ctx, void *host, const void *dptr, size_t bytes);   /* synchronous */
int jda_copy_to_device(jda_ctx *ctx, void *dptr, const void *host, size_t bytes); /* synchronous */

/* H2D: tables + index + filtered scan of one prepared image into one HBM allocation.  For an image prepared
 * with JDA_PREPARE_DEVICE_PRESCAN whose index is still pending, the index is made here on the GPU, equivalent to
 * the serial pre-scan's (jda_index_equivalent; the DC values are equal): one lane per 256 bytes of the scan, whose decoder states settle by
 * self-synchronisation in a few speculative rounds (restart intervals end where the filter found the markers).  A marker that is not where the MCU count puts it, a corrupt or truncated stream, or states that do
 * not settle send the image to the serial host pre-scan instead (the image object is completed in place). */
jda_dev_image *jda_upload(jda_ctx *ctx, jda_image *img, int32_t *err);
/* The same for n images at once: all pending block indexes are made by the same launches (the walk is latency-bound
 * per lane, so throughput comes from the number of segments in flight).  out[i] = device image.
 * Returns JDA_SUCCESS or the first error (then every out[i] is NULL). */
int jda_upload_batch(jda_ctx *ctx, int32_t n, jda_image *const *imgs, jda_dev_image **out);
/* The same, tolerant of holes: imgs[i] == NULL (a file jda_prepare_batch rejected) gives out[i] = NULL and status[i] =
 * JDA_INVALID_PARAMETER; every other image is uploaded (status[i] = JDA_SUCCESS, or the batch's HIP error).  The arrays stay
 * index-aligned with the caller's file list; jda_batch_create accepts the holes and launches nothing for them. */
int jda_upload_batch_ex(jda_ctx *ctx, int32_t n, jda_image *const *imgs, jda_dev_image **out, int32_t *status);
int jda_dev_image_prescan_on_device(const jda_dev_image *dimg);   /* 1: a device pre-scan produced the index */
/* copy the per-block index (n_blocks + 1 entries) and DC values (n_blocks) of a resident image back to the host
 * (either pointer may be NULL); n_blocks = mcus_x * mcus_y * blocks_per_mcu.  Synchronous. */
int jda_dev_image_read_index(jda_ctx *ctx, const jda_dev_image *dimg, uint32_t *index, int16_t *dc);
uint32_t jda_dev_image_mcus_ok(const jda_dev_image *dimg);        /* MCUs the pre-scan validated */
int jda_last_prescan_rounds(const jda_ctx *ctx);                 /* rounds the last device pre-scan on this context took (diagnostics) */
/* The marker / byte-stuffing filter (JPEGFilter, jpeg.inl:1431-1540) run on the GPU over a host buffer, result back on the
 * host: out must hold len bytes; *out_len = filtered length; restart_pos[0] = 0 and restart_pos[k] = filtered offset at
 * which the k-th RSTn marker stood (first restart_cap entries), *n_restarts = markers seen.  A stand-alone entry point
 * (jda_upload_batch still takes the scan filtered by jda_prepare on the host); exposed for callers that want the filtered
 * scan made on the GPU, and for the tests. */
int jda_filter_on_device(jda_ctx *ctx, const uint8_t *raw, int32_t len, uint8_t *out, int32_t *out_len,
                         uint32_t *restart_pos, int32_t restart_cap, int32_t *n_restarts);
void jda_dev_image_free(jda_ctx *ctx, jda_dev_image *dimg);
size_t jda_dev_image_bytes(const jda_dev_image *dimg);

/* where one image of a batch is written */
typedef struct jda_output {
    void *pixels;            /* DEVICE pointer, 16-byte aligned */
    int32_t pitch_bytes;     /* multiple of 16 */
    int32_t width_px;        /* clip: pixels written per row (<= canvas_w) */
    int32_t rows;            /* clip: rows written (<= canvas_h) */
} jda_output;

/* Build the launch plan for n resident images decoded with one (pixel_type, options) each. */
jda_batch *jda_batch_create(jda_ctx *ctx, int32_t n, jda_dev_image *const *images,
                            const jda_output *outputs, const int32_t *pixel_types,
                            const int32_t *options, int32_t *err);
/* The same with a rectangle of MCUs per image: mcu_rects[4 i ..] = {mx0, my0, mx1, my1} (half open, MCU units), or NULL for whole
 * images.  Only the tiles of the rectangle are launched -- the crop-aware decode (the reference skips the MCU rows above the crop
 * and the MCUs left and right of it, jpeg.inl:5111, 5134-5137; here they are not even visited: the per-block index lets a tile start
 * at any MCU).  The surface keeps the whole image's geometry; pixels outside the rectangle are not written.
 * A rectangle is clamped, never refused: a negative mx0 / my0 counts as 0, mx1 / my1 above the image's MCU counts as those counts, a
 * negative mx1 / my1 as 0.  What is left empty -- mx0 >= mx1 or my0 >= my1 after the clamp: an inverted rectangle, one that lies behind
 * the image -- launches no tile and writes nothing; the image keeps its place in the plan and its status is what the stream's is
 * (JDA_SUCCESS for a good file).  The rectangle of a hole (images[i] == NULL) is not looked at.  Each MCU row of a rectangle is cut into
 * tiles from the rectangle's own first MCU, so jda_batch_stats::tiles is, per image, (my1 - my0) * ceil((mx1 - mx0) / MCUs per tile). */
jda_batch *jda_batch_create_rect(jda_ctx *ctx, int32_t n, jda_dev_image *const *images,
                                 const jda_output *outputs, const int32_t *pixel_types,
                                 const int32_t *options, const int32_t *mcu_rects, int32_t *err);
void jda_batch_destroy(jda_ctx *ctx, jda_batch *batch);

/* Enqueue the decode kernels for the whole batch on the ctx stream (asynchronous). */
int jda_batch_decode(jda_ctx *ctx, jda_batch *batch);
/* launch statistics of the plan */
typedef struct jda_batch_stats {
    int64_t source_pixels;      /* sum of width*height */
    int64_t output_bytes;       /* bytes the kernels write */
    int64_t scan_bytes;         /* filtered entropy-coded bytes read */
    int64_t index_bytes;        /* per-block index + DC predictor bytes read */
    int64_t table_bytes;
    int32_t n_launches;         /* kernel launches per jda_batch_decode */
    int32_t n_workgroups;
    int64_t tiles;              /* wavefront tiles with work in the plan */
    int64_t tiles_whole_images; /* ... and what the whole images would have taken (crop-aware plans launch fewer) */
} jda_batch_stats;
int jda_batch_get_stats(const jda_batch *batch, jda_batch_stats *stats);
/* status[i] for every image of the plan: JDA_SUCCESS; JDA_DECODE_ERROR = the stream has a bad MCU (the MCUs before it are decoded,
 * what the reference delivers before it returns the error, jpeg.inl:5354-5356); JDA_INVALID_PARAMETER = a hole (images[i] == NULL) */
int jda_batch_get_status(const jda_batch *batch, int32_t *status);

int jda_sync(jda_ctx *ctx);

/* A position-dependent 64-bit checksum of each of n decoded surfaces (DEVICE pointers; rows x row_bytes[i] at pitch), computed
 * on the GPU: sum over the dwords d at linear index i of (uint64)((d ^ (i * 0x9E3779B1)) * 0x85EBCA6B mod 2^32) * (2 i + 1), mod 2^64,
 * a row's tail bytes zero-extended.  Lets a multi-GPU driver prove "every image decoded exactly once, identically" without moving
 * pixels (the reference has no such notion: its pixels go to a display as they are made).  Synchronous. */
int jda_checksum_surfaces(jda_ctx *ctx, int32_t n, const jda_output *surfaces, const int32_t *row_bytes, uint64_t *checksums);
/* ---- 4 / 2 / 1-bpp Floyd-Steinberg output (the reference's decodeDither: JPEGDither, jpeg.inl:4871-4940, run after every MCU row, :5309-5311)
 * The packed form of a GRAY8 canvas of canvas_w x canvas_h pixels (the canvas of jda_output_geometry for JDA_EIGHT_BIT_GRAYSCALE): rows of
 * *pitch_bytes = (canvas_w * bits + 7) / 8 bytes, most significant bits first, every padded column and row included; *bits = 4 / 2 / 1;
 * *bytes = pitch * canvas_h.  JDA_INVALID_PARAMETER for any other pixel type or an empty canvas. */
int jda_dither_geometry(int32_t canvas_w, int32_t canvas_h, int32_t pixel_type, int32_t *bits, int32_t *pitch_bytes, int64_t *bytes);
/* Dither n GRAY8 canvases resident in HBM in ONE launch on the context's stream (behind whatever decodes them there); synchronous.
 * gray[i]: pixels (16-byte aligned), pitch_bytes (a multiple of 16), width_px x rows = the canvas.  strip_rows[i]: the rows the reference
 * dithers at a time = the height of an MCU row in output pixels (16, 8, 4, 2 or 1): the image is ONE error chain, but the first row of
 * every strip starts with the error under its pixel 1 cleared (jpeg.inl:4882) -- the bytes depend on it; seeds: below.  packed[i]: pixels (4-byte
 * aligned), pitch_bytes (a multiple of 4, >= the pitch of jda_dither_geometry), rows >= gray[i].rows; width_px is not read.  The gray
 * canvases are left as they are.  Where canvas_w * bits is not a whole number of bytes, a row's last byte is what the reference's in-place
 * packing leaves there: the gray byte at offset y * pitch + pitch - 1 of the strip (y: the row within it).  The reference's own error
 * row holds 4,096 pixels; wider canvases are dithered by the same rule (it has no defined behaviour there). */
int jda_dither_surfaces(jda_ctx *ctx, int32_t n, const jda_output *gray, const int32_t *strip_rows, const int32_t *pixel_types,
                        const uint8_t *const *seeds, const jda_output *packed);
/* What the chain starts from.  The reference's error row is NOT clear before the first strip: it lies in the buffer (usPixels) in which the
 * header parse keeps the file's raw DHT contents -- table id t (DC 0-3, AC 4-7) at byte 273 t: 16 code counts, then the symbols
 * (jpeg.inl:837-873, :4881) -- so error byte i of the first row is byte i of that area (bytes 0-2 are cleared, :4882).  jda_dither_seed lays
 * a file's DHT segments out that way: seed[JDA_DITHER_SEED_BYTES]; overlay = 0 starts from zeros (an opened file), overlay = 1 writes over
 * what seed holds (the reference parses an EXIF thumbnail's header over the main image's).  seeds (HOST pointers; the array or an entry
 * may be NULL: zeros) gives jda_dither_surfaces one per canvas. */
#define JDA_DITHER_SEED_BYTES 2184
int jda_dither_seed(const uint8_t *jpeg, int32_t len, int32_t overlay, uint8_t *seed);

/* ---- EXIF orientation applied on the GPU (the class's JPEG_AUTO_ROTATE; the reference defines the bit and never reads it)
 * src = the VISIBLE rectangle of a decoded canvas: W = out_w x H = out_h pixels of bytes_per_pixel bytes (jda_output_geometry), never the MCU
 * padding.  dst = W' x H' pixels, dst(y', x') = src(y, x):
 *     orientation 0, 1: W x H, (y', x')       2: W x H, (y', W-1-x')       3: W x H, (H-1-y', W-1-x')       4: W x H, (H-1-y', x')
 *                 5: H x W, (x', y')          6: H x W, (H-1-x', y')       7: H x W, (H-1-x', W-1-y')       8: H x W, (x', W-1-y')
 * (what Pillow's exif_transpose does: FLIP_LEFT_RIGHT, ROTATE_180, FLIP_TOP_BOTTOM, TRANSPOSE, ROTATE_270, TRANSVERSE, ROTATE_90).  A file's
 * orientation is one byte (EXIF tag 274, jda_image_info.orientation); any value outside 2..8 means "as it is".
 * jda_oriented_geometry: orientation < 0: the file's.  *w, *h = W' x H'; *strip_rows = the source MCU's extent, in output pixels, along the
 * axis that became vertical (mcu_h >> shift for 0-4, mcu_w >> shift for 5-8, at least 1): the height of the strips the class hands to a draw
 * callback.  Refuses what jda_output_geometry refuses, with the same codes. */
int jda_oriented_geometry(const jda_image_info *info, int32_t pixel_type, int32_t options, int32_t orientation,
                          int32_t *bytes_per_pixel, int32_t *w, int32_t *h, int32_t *strip_rows);
/* Orient n surfaces resident in HBM in ONE launch on the context's stream (behind whatever decoded them there); synchronous.
 * src[i]: pixels (16-byte aligned), pitch_bytes (a multiple of 16), width_px x rows = the visible rectangle (rows are read in whole aligned
 * 16-byte vectors: up to the next multiple of 16 behind width_px * bytes_per_pixel, inside the pitch).  dst[i]: the same alignment rules;
 * width_px and rows must equal W' and H'.  Bytes of dst behind W' * bytes_per_pixel in a row, and rows behind H', are not written.
 * orientations[i]: 0..8; 0 or 1 is a copy.  bytes_per_pixel: 1, 2 or 4, of every surface of the call.  JDA_INVALID_PARAMETER: an orientation
 * outside 0..8, another pixel size, a wrong dst size, a null or misaligned pointer, a pitch too small or not a multiple of 16, byte ranges of
 * a dst and of any src or other dst that overlap.  n == 0 succeeds and launches nothing. */
int jda_orient_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *orientations, const jda_output *dst);

/* ---- Decoded surfaces repacked for a GPU-side consumer: three-byte RGB / BGR or planar CHW, tightly packed, as bytes or through a table
 * src[i] = a decoded surface resident in HBM: JDA_RGB8888 (src_bytes_per_pixel 4: bytes R, G, B, A) or JDA_EIGHT_BIT_GRAYSCALE (1); pixels 16-byte
 * aligned, pitch_bytes a multiple of 16 and >= width_px * src_bytes_per_pixel.  rects: {x, y, w, h} in pixels per image, inside width_px x rows;
 * NULL: all of width_px x rows -- pass the visible size (jda_output_geometry's out_w x out_h), not the canvas, and the MCU padding is gone.
 * dst[i] = DENSE, no padding anywhere: JDA_PACK_HWC h * w * C elements pixel-major, JDA_PACK_CHW C planes of h * w elements.  C = 3 for an
 * RGB8888 source (the alpha byte is never read into the result; | JDA_PACK_BGR: destination channel c is source channel 2 - c), C = 1 for a
 * gray source (the layout makes no difference).  dst[i] is aligned to its ELEMENT and to nothing else: image n of a uint8 [N,3,H,W] tensor
 * begins n * 3 * H * W bytes into it.  No byte outside [dst[i], dst[i] + jda_pack_bytes) is written.
 * elem_type JDA_PACK_U8: the source byte, table == NULL.  JDA_PACK_F16 / JDA_PACK_F32: table[c][v], c = the DESTINATION channel -- table =
 * C * 256 elements of the destination type in DEVICE memory, 16-byte aligned, one for the whole call.  The result is a lookup and nothing
 * else: normalisation ((v / 255 - mean) / std), gamma, any transfer is what the caller writes into the table; the kernel does no float
 * arithmetic, so every result is the table's bit pattern.
 * ONE launch on the context's stream (behind whatever decoded the surfaces there), synchronous.  n == 0 succeeds and launches nothing.
 * JDA_INVALID_PARAMETER: a null or misaligned pointer; a pitch too small or not a multiple of 16; a rectangle that is empty or leaves the
 * surface; a pixel size other than 1 or 4; unknown layout bits or element type; a table with U8, none with F16 / F32; JDA_PACK_BGR on a gray
 * source; byte ranges of a destination and of any source (the table included) or other destination that overlap; a job whose dense
 * destination is larger than JDA_PACK_MAX_BYTES (the kernel counts a job's bytes, elements and pixels in 32 bits). */
enum { JDA_PACK_HWC = 0, JDA_PACK_CHW = 1, JDA_PACK_BGR = 2 };          /* layout_flags */
enum { JDA_PACK_U8 = 0, JDA_PACK_F16 = 1, JDA_PACK_F32 = 2 };           /* elem_type */
#define JDA_PACK_MAX_BYTES 0x7fff0000u
/* w * h * channels elements of elem_type in bytes; 0 for arguments that are not positive or an unknown element type */
size_t jda_pack_bytes(int32_t w, int32_t h, int32_t channels, int32_t elem_type);
int jda_pack_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t src_bytes_per_pixel, const int32_t *rects,
                      int32_t layout_flags, int32_t elem_type, const void *table, void *const *dst);

/* ---- The inverse: dense tensors in HBM turned into surfaces the encoders, the resizer and the orienter read
 * src[i] = DENSE, dst[i].width_px x dst[i].rows pixels of C channels: JDA_PACK_HWC pixel-major or JDA_PACK_CHW planes, elements JDA_PACK_U8 /
 * _F16 / _F32, aligned to its ELEMENT and to nothing else (image n of a uint8 [N,3,H,W] tensor begins n * 3 * H * W bytes into it).
 * dst[i] = the surface: JDA_RGB8888 (dst_bytes_per_pixel 4, C = 3: bytes R, G, B, then A = 0xFF) or JDA_EIGHT_BIT_GRAYSCALE (1, C = 1);
 * pixels 16-byte aligned, pitch_bytes a multiple of 16 and >= width_px * dst_bytes_per_pixel.  Tensor channel c is surface channel c, or
 * 2 - c with JDA_PACK_BGR.  Exactly the width_px * dst_bytes_per_pixel bytes of each of the rows are written: not the padding up to the
 * pitch, nothing behind the last row.
 * JDA_PACK_U8: the byte itself, scale_bias == NULL.  JDA_PACK_F16 / _F32: byte = clamp(rint(x * scale[c] + bias[c]), 0, 255), c = the TENSOR
 * channel -- x converted exactly to float32 (subnormals kept), the product rounded to float32, the sum rounded to float32 again (never a
 * fused multiply-add), rint = round half to even, NaN -> 0, +inf -> 255, -inf -> 0: numpy's np.rint(x.astype(np.float32) * s + b) in float32.
 * scale_bias: HOST memory, scale[0..C-1] then bias[0..C-1]; NULL: scale 255, bias 0.  For a tensor normalised as (v / 255 - mean) / std
 * that is scale = 255 * std, bias = 255 * mean.
 * ONE launch on the context's stream, synchronous.  n == 0 succeeds and launches nothing.  The caller makes sure that whatever wrote the
 * tensors (another stream, another library) is done before the call.
 * JDA_INVALID_PARAMETER: a null pointer or array; n < 0; a pixel size other than 1 or 4; unknown layout bits or element type; JDA_PACK_BGR
 * with one channel; scale_bias with U8; a scale or bias that is not finite; a source misaligned for its element; a destination not 16-byte
 * aligned; a pitch too small or not a multiple of 16; a size that is not positive; a dense source larger than JDA_PACK_MAX_BYTES; a
 * destination whose written bytes share a byte with any source or with another destination's. */
int jda_unpack_surfaces(jda_ctx *ctx, int32_t n, const void *const *src, int32_t layout_flags, int32_t elem_type,
                        const float *scale_bias,      /* HOST: scale[0..C-1], bias[0..C-1]; NULL = 255, 0; must be NULL with U8 */
                        const jda_output *dst, int32_t dst_bytes_per_pixel);

/* ---- Decoded surfaces resized on the GPU: Pillow's Image.resize((ow, oh), Image.BILINEAR, box=(x, y, x + w, y + h)), bit for bit
 * src[i] = a decoded surface resident in HBM, JDA_RGB8888 (bytes_per_pixel 4) or JDA_EIGHT_BIT_GRAYSCALE (1); dst[i] = the result,
 * dst[i].width_px x dst[i].rows pixels of the same format: that IS the output size.  Both: pixels 16-byte aligned, pitch_bytes a multiple
 * of 16 and >= width_px * bytes_per_pixel.  rects: {x, y, w, h} in pixels per image, inside width_px x rows; NULL: all of width_px x
 * rows -- pass the visible size (jda_output_geometry's out_w x out_h), not the canvas, and the MCU padding is never sampled.
 * The filter is Pillow's antialiased triangle ("BILINEAR" with reducing_gap unset): per axis scale = box / output size, support =
 * max(scale, 1), 2 * ceil(support) + 1 taps at most per output coordinate, normalised and rounded to 22-bit fixed point on the HOST in
 * double; out = clip8((2^21 + sum in * k) >> 22) per byte, the horizontal pass first into 8-bit intermediates, then the vertical one.
 * All bytes of a pixel are channels: the fourth byte of RGB8888 is resampled like the others (Pillow's mode RGBX).  An axis whose size
 * and box are unchanged comes out as it went in.  No byte of dst[i] outside width_px * bytes_per_pixel x rows is written.
 * ONE launch on the context's stream (behind whatever decoded the surfaces there), synchronous.  n == 0 succeeds and launches nothing.
 * JDA_INVALID_PARAMETER: a null or misaligned pointer; a pitch too small or not a multiple of 16; a rectangle that is empty or leaves the
 * surface; an output size that is not positive; a side above 2^24; a pixel size other than 1 or 4; byte ranges of a destination and of any
 * source, tap table or other destination that overlap.  JDA_UNSUPPORTED_FEATURE: an axis with more than JDA_RESIZE_MAX_KSIZE taps -- a
 * downscale beyond 80 : 1 (every upscale has three) --, or a call whose tap tables ((2 + taps) * 4 bytes per output coordinate and axis;
 * images with equal size, rectangle and output size on an axis share one) pass JDA_RESIZE_MAX_TABLE_BYTES. */
#define JDA_RESIZE_MAX_KSIZE 161
#define JDA_RESIZE_MAX_TABLE_BYTES (64u << 20)
int jda_resize_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst);
/* The same with one of Pillow's five convolution filters for the whole call: Image.resize((ow, oh), F, box), bit for bit.  All share one
 * definition (Pillow's precompute_coeffs + normalize_coeffs_8bpc, then the two integer passes) and differ in the filter function and its
 * support, so in the taps of an axis and in the largest downscale below JDA_RESIZE_MAX_KSIZE:
 *   JDA_RESIZE_BILINEAR  support 1    3 taps in an upscale   downscales to  80 : 1   (jda_resize_surfaces)
 *   JDA_RESIZE_BOX       support 0.5  3                                    160 : 1
 *   JDA_RESIZE_HAMMING   support 1    3                                     80 : 1
 *   JDA_RESIZE_BICUBIC   support 2    5                                     40 : 1
 *   JDA_RESIZE_LANCZOS   support 3    7                                     26.6 : 1
 * BICUBIC and LANCZOS have negative taps and run kernel instances of their own (signed 24-bit multiply-adds, a two-sided clip); the other
 * three run the instances of jda_resize_surfaces.  Everything else as jda_resize_surfaces, which is this call with JDA_RESIZE_BILINEAR.
 * JDA_INVALID_PARAMETER: a filter id that is none of the five.  JDA_UNSUPPORTED_FEATURE also for a tap table that fails the host's guard
 * (a tap of 2^23 or more in size, or an output coordinate whose taps' sum could leave 32 bits: no axis is known that does). */
enum { JDA_RESIZE_BILINEAR = 0, JDA_RESIZE_BOX = 1, JDA_RESIZE_HAMMING = 2, JDA_RESIZE_BICUBIC = 3, JDA_RESIZE_LANCZOS = 4 };
int jda_resize_surfaces_ex(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst,
                           int32_t filter);

/* ---- Decoded surfaces encoded on the GPU as baseline JFIF files: libjpeg's file, byte for byte
 * A job turns the pixel rectangle {x, y, w, h} (1 <= w, h <= 65535, inside width_px x rows) of src[i] -- a surface resident in HBM,
 * JDA_RGB8888 (bytes_per_pixel 4: bytes R, G, B, A; A ignored; pixels and pitch multiples of 4) or JDA_EIGHT_BIT_GRAYSCALE (1) -- into
 * the file libjpeg (Pillow's Image.save(quality=, subsampling=, optimize=False, restart_marker_blocks=)) writes for these pixels, behind
 * its SOS header byte for byte: SOI, JFIF APP0, one 8-bit DQT per table, SOF0 (component ids 1..3), the four Annex K DHTs (two for gray),
 * DRI when restart_interval != 0, SOS, the entropy-coded data, EOI.  quality 1..100 scales the Annex K quantisers as jpeg_set_quality
 * does; colour is jccolor.c's, downsampling jcsample.c's h2v1 / h2v2 with edge replication, the transform jfdctint.c's, the rounding
 * jcdctmgr.c's; restart_interval 0..65535 MCUs (0: none); reserved = 0.  The rules in full: DESIGN.md 5.13.
 * dst[i] = DEVICE memory of dst_capacity[i] bytes, any alignment; dst_bytes[i] and status[i] are HOST arrays: the file's size and
 * JDA_SUCCESS, or -- the file does not fit dst_capacity[i] -- the size it needs and JDA_ERROR_MEMORY, and then NO byte of dst[i] is
 * written; the rest of the call goes on.  jda_encode_bound gives a capacity no file of that shape passes.
 * A fixed number of launches per call on the context's stream (behind whatever made the surfaces there), synchronous; n == 0 succeeds and
 * launches nothing.  JDA_INVALID_PARAMETER, before anything is launched: a null or misaligned pointer, a pitch too small, a rectangle
 * that is empty, too large or leaves the surface, a quality, sampling or pixel size out of range, reserved != 0, a gray surface with a
 * colour sampling or the reverse, a negative capacity, a destination that shares a byte with a source rectangle or another destination.
 * JDA_UNSUPPORTED_FEATURE: a call of more than 2^31 - 1 blocks.  JDA_ERROR_MEMORY from the call: no scratch (144 bytes a block and the
 * coded bytes). */
enum { JDA_ENCODE_GRAY = 0, JDA_ENCODE_444 = 1, JDA_ENCODE_422 = 2, JDA_ENCODE_420 = 3 };
typedef struct jda_encode_job { int32_t x, y, w, h, sampling, quality, restart_interval, reserved; } jda_encode_job;
int jda_encode_bound(int32_t w, int32_t h, int32_t sampling, int32_t restart_interval, int64_t *bytes);
int jda_encode_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs,
                        void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status);
/* jda_encode_surfaces with a word of flags per job: job_flags = NULL (every job as above) or n words.  JDA_ENCODE_OPTIMIZE: the file gets
 * Huffman tables of its own, made from its symbol counts as libjpeg's jpeg_gen_optimal_table makes them -- Pillow's optimize=True, behind
 * the SOS header byte for byte and the same four DHT segments (DC 0, AC 0, and for colour DC 1, AC 1, one segment per table in that order).
 * The symbols are counted and the code lengths summed on the GPU; the tables are made on the host from 2,176 bytes of counts per optimised
 * job, which costs the call one more wait and two more launches (nine whatever n is; a call without an optimised job is jda_encode_surfaces,
 * launch for launch).  jda_encode_bound holds unchanged: the header only shrinks and no code passes 16 bits.  Any other flag bit:
 * JDA_INVALID_PARAMETER before anything is launched.  JDA_UNSUPPORTED_FEATURE: an optimised job of more than 15,625,000 blocks (a symbol
 * count could pass libjpeg's limit of 10^9), or -- after the first launches -- counts for which libjpeg itself gives up (a code of more than
 * 32 bits before the lengths are limited; no picture has been seen to give them). */
enum { JDA_ENCODE_OPTIMIZE = 1 };
int jda_encode_surfaces_ex(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, const uint32_t *job_flags,
                           void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status);
/* jda_encode_surfaces for PROGRESSIVE files: the file Pillow's Image.save(quality=, subsampling=, progressive=True) writes for these pixels,
 * from its SOF2 marker to EOI byte for byte (optimize=True changes nothing in such a file).  SOI, JFIF APP0, one 8-bit DQT per table, SOF2,
 * then libjpeg's default scan script (jpeg_simple_progression: ten scans for colour, six for gray), every scan behind the DHT segment(s) of
 * the table(s) made from its own symbol counts (jpeg_gen_optimal_table) and its SOS, then EOI; no DRI.  The coefficients are those of
 * jda_encode_surfaces; the passes are jcphuff.c's, its two flushes of an end-of-band run -- at 0x7FFF blocks, and once more than 937
 * correction bits are buffered -- included.  The rules in full: DESIGN.md 5.13, rules 10 to 14.
 * Arguments, statuses and refusals as in jda_encode_surfaces, and: restart_interval must be 0 (JDA_INVALID_PARAMETER before anything is
 * launched: restart intervals in progressive scans are not written); a job of more than 15,625,000 blocks is refused
 * (JDA_UNSUPPORTED_FEATURE), as an optimised baseline job is.  Gray and colour jobs may be mixed across calls, not within one.  A file that
 * does not fit its capacity is reported with the size it needs and no byte of it is written.  ELEVEN launches per call whatever n is
 * (blocks and lengths of jda_encode_surfaces, then classify, resolve, gather, lengths, scan, emit, count, scan, write) and three waits: the
 * symbol counts (1 KiB a scan) come back for the host to make the tables, the scans' sizes for it to place them, then the files' sizes.
 * jda_encode_bound_progressive gives a capacity no file of that shape passes (larger than jda_encode_bound: 3,928 bits a block over all
 * scans, and 568 bytes of DHT and SOS a scan).  Scratch: 128 + 8 bytes a block, 20 bytes a unit (a block of a scan), 2 KiB a scan, and
 * the coded bytes. */
int jda_encode_bound_progressive(int32_t w, int32_t h, int32_t sampling, int64_t *bytes);
int jda_encode_surfaces_progressive(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs,
                                    void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status);

/* PCI bus id ("0000:8e:00.0") of the context's GPU, for NUMA placement of the host threads that feed it; buf >= 16 bytes */
int jda_device_pci_bus_id(jda_ctx *ctx, char *buf, int32_t len);
int jda_device_pci_bus_id_of(int32_t device, char *buf, int32_t len);      /* the same by device ordinal, without a context */

/* HIP-event timing on the ctx stream: start/stop record events on that stream; elapsed blocks
 * until stop has happened and returns milliseconds (<0 on error). */
int jda_timer_start(jda_ctx *ctx);
int jda_timer_stop(jda_ctx *ctx);
double jda_timer_elapsed_ms(jda_ctx *ctx);

/* One-call convenience used by the JPEGDEC class: prepare + upload + decode + copy back into a
 * HOST canvas of canvas_w x canvas_h pixels (pitch_bytes per row). */
int jda_decode_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type,
                       int32_t options, void *host_pixels, int32_t pitch_bytes, int32_t rows);
/* The same; *mcus_decoded (may be NULL) = MCUs decoded before the first invalid code, in scan order (all of them on
 * JDA_SUCCESS; fewer with JDA_DECODE_ERROR: the reference stops at that MCU, jpeg.inl:2137, 2237, 5354-5356 -- the
 * canvas holds the MCUs before it, zeros behind). */
int jda_decode_to_host_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type,
                          int32_t options, void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded);
/* jda_decode_to_host_ex for pixel_type JDA_FOUR_BIT_DITHERED / JDA_TWO_BIT_DITHERED / JDA_ONE_BIT_DITHERED: the image is decoded to GRAY8 (luma
 * only) on the device, dithered there MCU row by MCU row as the reference does (jda_dither_surfaces, strip_rows = an MCU row's height) and
 * only the packed rows come back: row r of the canvas at host_packed + r * pitch_bytes, pitch_bytes >= the pitch of jda_dither_geometry.
 * Pre-scan, host fallback, status and *mcus_decoded as jda_decode_to_host_ex for JDA_EIGHT_BIT_GRAYSCALE (JDA_DECODE_ERROR: the MCUs from
 * the bad one on are dithered as zeros).  seed: JDA_DITHER_SEED_BYTES the chain starts from, or NULL: jda_dither_seed of the file. */
int jda_decode_dither_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options,
                              const uint8_t *seed, void *host_packed, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded);
/* jda_decode_to_host_ex followed by jda_pack_surfaces: prepare, upload, decode to a device canvas, pack its visible rectangle and copy back
 * only the dense bytes -- decode, pack and the copy are queued back to back.  The image is decoded as JDA_RGB8888 (C = 3); a gray file, or
 * JDA_LUMA_ONLY, as JDA_EIGHT_BIT_GRAYSCALE (C = 1).  layout_flags, elem_type as jda_pack_surfaces; table: C * 256 elements in HOST memory
 * (any alignment), NULL with JDA_PACK_U8.  host_out: out_bytes >= jda_pack_bytes(*w, *h, C, elem_type) or JDA_INVALID_PARAMETER.  *w, *h (may be
 * NULL): the visible size, jda_output_geometry's out_w x out_h.  The JDA_SCALE_* bits and the default 1/8 thumbnail of a progressive file
 * as in jda_decode_to_host_ex, with the same refusals and codes; JDA_PROGRESSIVE_FULL on a progressive file: JDA_UNSUPPORTED_FEATURE.
 * Pre-scan, host fallback, status and *mcus_decoded as jda_decode_to_host_ex; with JDA_DECODE_ERROR the MCUs from the bad one on are zeros
 * BEFORE the pack (table[c][0] behind it) and the whole result is still delivered. */
int jda_decode_to_host_packed(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, int32_t layout_flags, int32_t elem_type,
                              const void *table, void *host_out, size_t out_bytes, int32_t *w, int32_t *h, int32_t *mcus_decoded);
/* jda_decode_to_host_ex followed by jda_resize_surfaces: prepare, upload, decode to a device canvas, resize rect = {x, y, w, h} (pixels of
 * the visible image, jda_output_geometry's out_w x out_h at the options' scale; NULL: all of it) to out_w x out_h and copy back only those
 * out_w * bpp x out_h bytes: row r at host_pixels + r * pitch_bytes, pitch_bytes >= out_w * bpp (any value), rows >= out_h.  pixel_type:
 * JDA_RGB8888 or JDA_EIGHT_BIT_GRAYSCALE; any other: JDA_INVALID_PARAMETER.  Only the MCUs that hold a pixel the taps read are decoded
 * (jda_batch_create_rect): tiles (may be NULL): [0] wavefront tiles launched, [1] tiles of the whole image.  The rectangle never leaves
 * the visible image, so the MCU padding is never sampled.  Option bits, the default 1/8 thumbnail of a progressive file, refusals and
 * codes as in jda_decode_to_host_ex; JDA_PROGRESSIVE_FULL on a progressive file: JDA_UNSUPPORTED_FEATURE; the limits of
 * jda_resize_surfaces.  With JDA_DECODE_ERROR the MCUs from the bad one on are zeros BEFORE the resize and the whole result is still
 * delivered. */
int jda_decode_to_host_resized(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *rect,
                               int32_t out_w, int32_t out_h, void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded,
                               int32_t *tiles);
/* the same with a filter (JDA_RESIZE_*; 0: jda_decode_to_host_resized).  The MCUs that are decoded are those the CHOSEN filter's taps read: a
 * LANCZOS crop reads up to three times the scale beyond its rectangle on each side -- clipped at the visible image, never at the rectangle. */
int jda_decode_to_host_resized_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *rect,
                                  int32_t out_w, int32_t out_h, int32_t filter, void *host_pixels, int32_t pitch_bytes, int32_t rows,
                                  int32_t *mcus_decoded, int32_t *tiles);
/* jda_decode_to_host_ex, jda_resize_surfaces (only when out_w x out_h differs from the rectangle's size; always the triangle filter,
 * JDA_RESIZE_BILINEAR: the transcode call takes no filter) and jda_encode_surfaces: a JPEG file
 * in, a baseline JPEG file of rect = {x, y, w, h} (pixels of the visible image at the options' scale; NULL: all of it) at out_w x out_h out;
 * only files cross the bus.  The image is decoded as JDA_RGB8888, a gray file as JDA_EIGHT_BIT_GRAYSCALE -- and then sampling must be
 * JDA_ENCODE_GRAY, as it must not be for a colour file (JDA_INVALID_PARAMETER).  Only the MCUs that hold a pixel that is read are decoded.
 * host_file: capacity bytes of HOST memory; *file_bytes = the file's size; a file that does not fit: JDA_ERROR_MEMORY, *file_bytes = the size
 * it needs, host_file untouched.  Option bits, refusals and codes as in jda_decode_to_host_resized and jda_encode_surfaces; with
 * JDA_DECODE_ERROR the MCUs from the bad one on are zeros before the resize and the file is still delivered. */
int jda_transcode_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, const int32_t *rect, int32_t out_w, int32_t out_h,
                          int32_t sampling, int32_t quality, int32_t restart_interval, void *host_file, int64_t capacity, int64_t *file_bytes);
/* the same with the encoder's flags (JDA_ENCODE_OPTIMIZE, as in jda_encode_surfaces_ex; 0: jda_transcode_to_host) */
int jda_transcode_to_host_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, const int32_t *rect, int32_t out_w, int32_t out_h,
                             int32_t sampling, int32_t quality, int32_t restart_interval, uint32_t encode_flags, void *host_file, int64_t capacity,
                             int64_t *file_bytes);
/* jda_transcode_to_host with jda_encode_surfaces_progressive as its encoder: a progressive file out (restart_interval must be 0) */
int jda_transcode_to_host_progressive(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, const int32_t *rect, int32_t out_w, int32_t out_h,
                                      int32_t sampling, int32_t quality, int32_t restart_interval, void *host_file, int64_t capacity, int64_t *file_bytes);
/* A dense image in HOST memory (w x h pixels of channels = 3 or 1; layout_flags, elem_type, scale_bias as jda_unpack_surfaces) to a JPEG file
 * in host memory: the image goes up, jda_unpack_surfaces makes a surface of it, one of the encoders makes the file -- form JDA_RECODE_BASELINE
 * (jda_encode_surfaces), JDA_RECODE_OPTIMIZE (JDA_ENCODE_OPTIMIZE) or JDA_RECODE_PROGRESSIVE (jda_encode_surfaces_progressive; restart_interval
 * must be 0) -- and only the file comes back; the stages are queued back to back on the context's stream.  sampling, quality,
 * restart_interval as jda_encode_job; a gray image (channels 1) takes JDA_ENCODE_GRAY and a colour image must not (JDA_INVALID_PARAMETER).
 * host_file, capacity, *file_bytes and a file that does not fit: as jda_transcode_to_host. */
int jda_encode_dense_to_host(jda_ctx *ctx, const void *host_dense, int32_t w, int32_t h, int32_t channels, int32_t layout_flags, int32_t elem_type,
                             const float *scale_bias, int32_t sampling, int32_t quality, int32_t restart_interval, int32_t form,
                             void *host_file, int64_t capacity, int64_t *file_bytes);
/* jda_decode_to_host_ex followed by the orientation: prepare, upload, decode to a device canvas, orient its visible rectangle into a second
 * device surface (jda_orient_surfaces) and copy back only the W' * bpp x H' bytes of jda_oriented_geometry: row r at host_pixels + r * pitch_bytes,
 * pitch_bytes >= W' * bpp (any value), rows >= H'.  orientation < 0: the file's; 0..8 as given (0, 1: the visible rectangle as it is); above
 * 8: JDA_INVALID_PARAMETER.  Pre-scan, host fallback, status and *mcus_decoded as jda_decode_to_host_ex; with JDA_DECODE_ERROR the MCUs from the
 * bad one on are zeros BEFORE the orientation and the oriented canvas is still delivered.  Decode, orient and the copy are queued back to back.
 * Dithered pixel types: JDA_INVALID_PARAMETER.  (jda_decode_to_host*, jda_batch_* and jda_pipeline_* keep ignoring option bit 1.) */
int jda_decode_to_host_oriented(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, int32_t orientation,
                                void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded);
/* The same, decoding only the MCUs of mcu_rect = {mx0, my0, mx1, my1} (half open; NULL: everything): the canvas keeps its
 * geometry, the rows of the rectangle are written (zeros left and right of it), the others are not touched.  tiles (may be NULL):
 * [0] wavefront tiles launched, [1] tiles of the whole image. */
int jda_decode_to_host_rect(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *mcu_rect,
                            void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded, int32_t *tiles);

/* The same with flags.  JDA_TO_HOST_KEEP_UNDECODED (whole image only, mcu_rect == NULL): when the stream has a bad MCU, copy back
 * only the MCUs in front of it -- whole MCU rows, then the row's MCUs before the bad one -- and leave every other byte of
 * host_pixels as it was: what the reference's early return does to a caller's framebuffer (jpeg.inl:5354-5356). */
#define JDA_TO_HOST_KEEP_UNDECODED 1
int jda_decode_to_host_flags(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *mcu_rect,
                             void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded, int32_t *tiles, int32_t flags);

/* The same, the copy back cut into n_bands (<= 8) bands of whole MCU rows: band_ready(user, row0, row1) is called, in order, as soon as
 * rows [row0, row1) of host_pixels have landed -- what the caller does with them (JPEGDEC::decode replays the reference's JPEGDRAW
 * callbacks, jpeg.inl:5300-5336) overlaps the rest of the copy.  *mcus_decoded is set before the first call.  The copy is NOT cut --
 * one copy, band_ready never called, the caller looks at all rows after the return -- without a callback, with n_bands <= 1, with a
 * rectangle, and with JDA_TO_HOST_KEEP_UNDECODED on a stream that has a bad MCU. */
typedef void(jda_band_callback)(void *user, int32_t row0, int32_t row1);
int jda_decode_to_host_bands(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *mcu_rect,
                             void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded, int32_t *tiles, int32_t flags,
                             int32_t n_bands, jda_band_callback *band_ready, void *user);

/* The whole image STRIP-MAJOR: as the JPEGDRAW strips the reference hands to its draw callback (jpeg.inl:5300-5336) -- strip_mcus MCUs
 * wide (a row's last strip: what is left), one MCU row high, in raster order, every strip's pixels contiguous with the strip's own
 * width as pitch; strip (row y, column s) starts (y * ceil(mcus_x / strip_mcus) + s) * strip_mcus * mcu_w' * mcu_h' * bpp bytes into
 * host_pixels (mcu_w', mcu_h': the MCU in output pixels).  The kernels write the surface in that layout; a consumer hands out
 * pointers instead of copying strips together.  host_bytes >= mcus_y * ceil(mcus_x / strip_mcus) * that strip size.  The copy back
 * in n_bands bands of MCU rows as jda_decode_to_host_bands (band_ready may be NULL). */
int jda_decode_to_host_strips(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, int32_t strip_mcus,
                              void *host_pixels, size_t host_bytes, int32_t *mcus_decoded, int32_t n_bands, jda_band_callback *band_ready, void *user);

/* ------------------------------------------------------------------ the streamed pipeline
 * Files in, pixels resident in HBM out, batch after batch: the host parses headers and builds tables (microseconds per file);
 * the unfiltered entropy-coded bytes go to the GPU, which filters them (JPEGFilter, jpeg.inl:1431-1540), makes the per-block
 * index (equivalent to the serial pre-scan's: jda_index_equivalent) and decodes (jpeg.inl:5109-5353).  Upload + filter + pre-scan of
 * batch n+1 run on streams of their own under the decode of batch n (three batches in flight keep the GPU busy).  Images the device walk cannot take or that fail its checks
 * (progressive, corrupt, truncated, ...) are redone through the serial host pre-scan when the batch is waited for, so every
 * image ends with the status -- and the pixels -- the one-image path (jda_decode_to_host) gives it.
 *   jda_pipeline_create   max_images per batch; depth = batches in flight (1..8); host_threads <= 0: up to 8
 *   jda_pipeline_submit   enqueue one batch; the JPEG buffers and the output surfaces (DEVICE pointers, as jda_output) must
 *                         stay valid until the batch has been waited for.  *ticket identifies the batch.
 *   jda_pipeline_wait     block until the batch is decoded; status[i] = JDA_SUCCESS or the image's error (may be NULL).
 *                         A batch must be waited for before `depth` further batches are submitted.  Returns JDA_SUCCESS unless
 *                         the pipeline itself failed (a bad image is reported in status[], it does not fail its batch). */
typedef struct jda_pipeline jda_pipeline;
typedef struct jda_pipeline_stats {
    int64_t images, device_images, host_path_images, failed_images;
    int64_t source_pixels, compressed_bytes, h2d_bytes;
    int32_t launches, spec_rounds_max;
} jda_pipeline_stats;
jda_pipeline *jda_pipeline_create(jda_ctx *ctx, int32_t max_images, int32_t depth, int32_t host_threads, int32_t *err);
void jda_pipeline_destroy(jda_pipeline *p);
int jda_pipeline_submit(jda_pipeline *p, int32_t n, const uint8_t *const *jpegs, const int32_t *lens, const jda_output *outputs,
                        const int32_t *pixel_types, const int32_t *options, int32_t *ticket);
/* The same with flags.  JDA_SUBMIT_PINNED_INPUT: every jpegs[i] lies in page-locked host memory (jda_host_alloc, or any buffer
 * made known with jda_host_register) -- the copy engine then reads the files' entropy-coded bytes where they are, and no host core
 * copies them into the pipeline's own page-locked mirror first (the host's largest share of a batch; what lets a rank with two or
 * three cores feed its GPU).  Files that lie next to one another in memory (gaps up to 64 KB: a loader's arena, a ring of receive
 * buffers) travel as one copy command; a command that would carry less than 128 KB is not worth what it costs the submitting
 * thread, so isolated small files still go through the mirror. */
#define JDA_SUBMIT_PINNED_INPUT 1
/* JDA_SUBMIT_PROGRESSIVE_FULL: honour JDA_PROGRESSIVE_FULL in options[i] for a progressive file instead of refusing it (without the flag:
 * JDA_UNSUPPORTED_FEATURE in status[i], as ever).  Such a file's scans are walked on the host, on the pipeline's workers next to the other
 * files' header parses, one image a worker; its coefficients travel in whichever form is smaller (JDA_COEF_AUTO) through a page-locked
 * mirror, and all such images of the batch are decoded at full size into outputs[i] by one launch per (form, layout) present, queued behind
 * the batch's decode: jda_pipeline_wait returns when their pixels are in place.  A scale bit beside the option bit: JDA_UNSUPPORTED_FEATURE
 * in status[i] (no DCT-domain scale on this path); a scan error: JDA_DECODE_ERROR in status[i], the surface untouched, the batch goes on.
 * In the statistics these images count in images and host_path_images (their entropy decode ran on the host), in source_pixels and
 * compressed_bytes like any decoded file, their bytes in h2d_bytes, their launches in launches.  Baseline files, and progressive files without the bit, are not affected. */
#define JDA_SUBMIT_PROGRESSIVE_FULL 2
int jda_pipeline_submit_ex(jda_pipeline *p, int32_t n, const uint8_t *const *jpegs, const int32_t *lens, const jda_output *outputs,
                           const int32_t *pixel_types, const int32_t *options, int32_t flags, int32_t *ticket);
int jda_pipeline_wait(jda_pipeline *p, int32_t ticket, int32_t *status);
int jda_pipeline_get_stats(const jda_pipeline *p, jda_pipeline_stats *out);   /* totals over the batches waited for */
/* diagnostics: after jda_pipeline_wait(ticket), before `depth` more batches are submitted -- the per-block index (n_blocks + 1
 * entries) and DC values (n_blocks) the device made for image i, and its filtered scan length (any pointer may be NULL) */
int jda_pipeline_read_index(jda_pipeline *p, int32_t ticket, int32_t i, uint32_t *index, int16_t *dc, uint32_t *filtered_len);

/* ------------------------------------------------------------------ the node: one host process, every GPU
 * Images are independent (the reference zeroes its whole state per image, src/JPEGDEC.cpp:66): a node shards a LIST of files by
 * image.  jda_node owns one context + one streamed pipeline per device and deals a submitted list out in contiguous blocks --
 * device k of K takes images [first, first + count) of jda_node_shard (sizes differ by at most one: the rule the multi-process
 * bench uses).  Every device has ONE PERSISTENT host thread, made with the node and pinned to the CPUs of its GPU's NUMA node
 * (devices on one NUMA node share its CPUs; jda_node_placement tells): it creates the device's context and pipeline -- whose
 * workers inherit the placement -- and runs the device's half of every submit / wait / checksum call, so the calling thread makes
 * no HIP call and keeps its current device.  Pixels never cross between GPUs: outputs[i].pixels must be a
 * DEVICE pointer on the device that owns image i (allocate with jda_malloc(jda_node_context(node, k), ..)).  What comes back
 * is status[i] per image and, for a proof that every image was decoded once and identically wherever it landed, per-image
 * checksums made where the pixels are (jda_node_checksums = jda_checksum_surfaces per device).
 *   jda_node_create   devices == NULL or n_devices <= 0: every visible device (0 .. jda_device_count() - 1); an ordinal may be named more
 *                     than once (each entry is a pipeline, a context and a host thread of its own on that device); max_images_per_device
 *                     bounds a device's block; depth / host_threads_per_device as jda_pipeline_create.  Fails with
 *                     JDA_ERROR_NO_DEVICE when there is no GPU: there is no CPU decode path.
 *   jda_node_submit   n <= devices * max_images_per_device images; buffers and surfaces stay valid until the list is waited for
 *   jda_node_wait     blocks until every device has decoded its block; status may be NULL */
typedef struct jda_node jda_node;
jda_node *jda_node_create(const int32_t *devices, int32_t n_devices, int32_t max_images_per_device, int32_t depth,
                          int32_t host_threads_per_device, int32_t *err);
void jda_node_destroy(jda_node *node);
int32_t jda_node_device_count(const jda_node *node);
int32_t jda_node_device(const jda_node *node, int32_t k);          /* HIP device ordinal of the node's k-th device */
jda_ctx *jda_node_context(jda_node *node, int32_t k);              /* its context (owned by the node) */
void jda_node_shard(const jda_node *node, int32_t n, int32_t k, int32_t *first, int32_t *count);
void jda_node_shard_of(int32_t n_devices, int32_t n, int32_t k, int32_t *first, int32_t *count);     /* the same rule without a node */
int jda_node_submit(jda_node *node, int32_t n, const uint8_t *const *jpegs, const int32_t *lens, const jda_output *outputs,
                    const int32_t *pixel_types, const int32_t *options, int32_t *ticket);
int jda_node_submit_ex(jda_node *node, int32_t n, const uint8_t *const *jpegs, const int32_t *lens, const jda_output *outputs,
                       const int32_t *pixel_types, const int32_t *options, int32_t flags, int32_t *ticket);      /* flags: JDA_SUBMIT_* */
int jda_node_wait(jda_node *node, int32_t ticket, int32_t *status);
/* where device k's host thread runs: its GPU's NUMA node (-1: unknown) and how many CPUs it is pinned to (0: not pinned) */
int jda_node_placement(const jda_node *node, int32_t k, int32_t *numa_node, int32_t *cpus_pinned);
int jda_node_checksums(jda_node *node, int32_t n, const jda_output *surfaces, const int32_t *row_bytes, uint64_t *checksums);
int jda_node_get_stats(const jda_node *node, jda_pipeline_stats *out);   /* sums over the devices' pipelines */

/* ------------------------------------------------------------------ coefficient images (JDA_PROGRESSIVE_FULL, DCT-domain callers)
 * A coefficient image is a file's geometry and prescaled quantisers plus one int16[64] per block: natural (row-major) order, entry 0
 * the DC value, 128 bytes a block, 16-byte aligned, values modulo 2^16; blocks in the order of the per-block index (MCU-interleaved
 * scan order, mcus_x * mcus_y * blocks_per_mcu of them) -- the decode kernel's LDS slot without its padding.
 *   jda_progressive_prepare           every scan of a progressive (SOF2) file decoded on the host (T.81 Annex G): DC and AC, first passes and
 *                                     refinements, EOB runs, spectral selection, restart intervals, DHT and DQT segments in front of and between the
 *                                     scans -- Huffman tables are those in force at each SOS (ids 0-3 of either class; none of the baseline path's
 *                                     table restrictions applies), a component's quantiser is latched at the first scan that names it (a table
 *                                     defined or redefined behind that scan does not reach the component; none defined by then: JDA_DECODE_ERROR)
 *                                     --, non-interleaved scans over the component's own extent -- ceil(w_c / 8) x ceil(h_c / 8) blocks, never the
 *                                     MCU padding, whose blocks keep what the interleaved scans gave them.  The image's quantiser table c is
 *                                     component c's (q_id = 0, 1, 2).  An invalid Huffman code, a scan naming an unknown component or table, a band
 *                                     against the Ss / Se / Ah / Al rules: NULL with JDA_DECODE_ERROR, nothing delivered.  A file that ends (EOI
 *                                     or end of data) behind at least one scan is valid and decodes to what its scans carry; where the data end
 *                                     INSIDE a scan, that scan is read on as if zero bits followed (what libjpeg does with a truncated file).  A
 *                                     first-pass value whose point transform leaves int16 (value << Al, DC or AC: no 8-bit encoder writes one) is
 *                                     kept modulo 2^16, as every coefficient of the image is: defined at coefficient level, no pixels promised.  A
 *                                     baseline file: JDA_INVALID_PARAMETER.
 *   jda_coef_image_from_coefficients  geometry and quantisers from the headers of any supported file, baseline or progressive; coefficients
 *                                     from the caller (copied), n_blocks must match
 *   jda_coef_image_quant              the four prescaled quantiser tables (4 x 64 int16, natural order); q_id (may be NULL): table of Y, Cb, Cr */
typedef struct jda_coef_image jda_coef_image;
jda_coef_image *jda_progressive_prepare(const uint8_t *jpeg, int32_t len, int32_t *err);
jda_coef_image *jda_coef_image_from_coefficients(const uint8_t *jpeg, int32_t len, const int16_t *coefs, uint32_t n_blocks, int32_t *err);
void jda_coef_image_free(jda_coef_image *img);
const jda_image_info *jda_coef_image_get_info(const jda_coef_image *img);
const int16_t *jda_coef_image_coefficients(const jda_coef_image *img, uint32_t *n_blocks);
const int16_t *jda_coef_image_quant(const jda_coef_image *img, uint8_t *q_id);
/* The SPARSE form of a coefficient image: an entry per NONZERO coefficient (mod 2^16), DC included.  Built on first request, owned by the
 * image and cached (thread-safe).  first[n_blocks + 1]: block g's entries are entries[first[g] .. first[g + 1]); *n_entries = first[n_blocks].
 * entry = (g & 1023) << 22 | n << 16 | (uint16_t)value:  n = natural index 0..63 (0 = DC), ascending within a block.  A tile of the kernel is
 * <= 64 consecutive blocks, so ten bits of g place an entry in its tile without a search.  2^31 entries and more: NULL, and
 * jda_coef_image_sparse_status answers JDA_UNSUPPORTED_FEATURE (JDA_SUCCESS otherwise). */
const uint32_t *jda_coef_image_sparse(const jda_coef_image *img, const uint32_t **first, uint32_t *n_entries);
int jda_coef_image_sparse_status(const jda_coef_image *img);
size_t jda_coef_image_sparse_bytes(const jda_coef_image *img);   /* 4 * (n_blocks + 1) + 4 * n_entries, each part rounded up to 16; 0: no sparse form */
/* H2D of one coefficient image (quantisers + coefficients, one allocation), and the decode of n resident ones on the context's stream: ONE
 * launch for the images of one MCU layout -- the kernel is a template over the layout, as the decode kernel is, so a call whose images mix
 * layouts makes one launch per layout present, five at most -- (kernel jda_coef_tiles: dequantise, IDCT with the reference's column / row shortcuts -- driven by the occupancy
 * flags JPEGDecodeMCU would have formed from these coefficients, jpeg.inl:2207-2208 --, colour conversion); synchronous like
 * jda_orient_surfaces.  outputs as jda_batch_create; pixel_types: the four decode targets; options: JDA_LUMA_ONLY (and
 * JDA_PROGRESSIVE_FULL, ignored); a scale bit: JDA_UNSUPPORTED_FEATURE -- full size only. */
typedef struct jda_dev_coef jda_dev_coef;
jda_dev_coef *jda_coef_upload(jda_ctx *ctx, const jda_coef_image *img, int32_t *err);
void jda_dev_coef_free(jda_ctx *ctx, jda_dev_coef *dimg);
int jda_coef_decode_surfaces(jda_ctx *ctx, int32_t n, const jda_dev_coef *const *imgs, const jda_output *outputs, const int32_t *pixel_types,
                             const int32_t *options);
/* Upload with a choice of form.  JDA_COEF_DENSE: 128 bytes a block (jda_coef_upload).  JDA_COEF_SPARSE: quantisers | first[] | entries[] in one
 * allocation, each part 16-byte aligned: 4 bytes a block + 4 a nonzero coefficient -- smaller than dense unless a block holds more than 31
 * nonzero terms (quality-100 noise).  JDA_COEF_AUTO: whichever is fewer bytes for THIS image (dense on a tie, and where the sparse form is
 * refused).  A form outside 0..2 or a NULL image: JDA_INVALID_PARAMETER. */
enum { JDA_COEF_DENSE = 0, JDA_COEF_SPARSE = 1, JDA_COEF_AUTO = 2 };
jda_dev_coef *jda_coef_upload_ex(jda_ctx *ctx, const jda_coef_image *img, int32_t form, int32_t *err);
int jda_dev_coef_form(const jda_dev_coef *d);      /* JDA_COEF_DENSE or JDA_COEF_SPARSE: what is resident */
size_t jda_dev_coef_bytes(const jda_dev_coef *d);  /* of the device allocation, quantisers included */
/* jda_coef_decode_surfaces over images of either form, mixed freely -- sparse ones are decoded by kernel jda_sparse_tiles, whose load phase
 * scatters the entries into the LDS slots the dense load phase fills: equal slots, equal pixels --: one launch per (form, layout) present, ten
 * at most.  mcu_rects (NULL: whole images): {mx0, my0, mx1, my1} per image in MCUs, half open, with the rules of jda_batch_create_rect:
 * clamped to the image, an empty rectangle decodes nothing, tiles are cut from the rectangle's own first MCU; pixels outside are untouched. */
int jda_coef_decode_surfaces_rect(jda_ctx *ctx, int32_t n, const jda_dev_coef *const *imgs, const jda_output *outputs, const int32_t *pixel_types,
                                  const int32_t *options, const int32_t *mcu_rects);

/* ------------------------------------------------------------------ lossless recode
 * A JPEG's own quantised coefficients to a file with another entropy coding -- what jpegtran -optimize / -progressive -copy none do: no
 * IDCT, no colour conversion, no FDCT, no quantisation; every coefficient and every quantiser of the source is in the file that comes out
 * -- with ONE exception, which the format makes: a JDA_RECODE_PROGRESSIVE file holds no AC coefficient of the MCU grid's padding blocks
 * (blocks of a component that lie outside its own extent of ceil(w_c / 8) x ceil(h_c / 8): its AC scans visit that extent only, T.81 A.2.2;
 * jpegtran drops them too).  Their DC values are kept, no pixel inside the image depends on them, and a baseline or optimised target keeps all.
 * The source is resident: a baseline image (jda_upload*, its index from the host pre-scan or from JDA_PREPARE_DEVICE_PRESCAN: the same file
 * either way) or a dense coefficient image (jda_coef_upload, e.g. of jda_progressive_prepare: a progressive file made baseline).  Exactly
 * one of jda_recode_source's two pointers is set.  form: JDA_RECODE_BASELINE (the Annex K tables, as jda_encode_surfaces writes them),
 * JDA_RECODE_OPTIMIZE (tables of the file's own, as JDA_ENCODE_OPTIMIZE), JDA_RECODE_PROGRESSIVE (libjpeg's simple progression, as
 * jda_encode_surfaces_progressive).  restart_interval: -1 the source's own (dropped in a progressive file), 0 none, 1..65535 MCUs.
 * dst, dst_capacity, dst_bytes, status: as in jda_encode_surfaces -- a file that does not fit is reported with the size it needs and
 * JDA_ERROR_MEMORY, and no byte of it is written.  jda_recode_bound: a capacity no recoded file of that source passes (jda_encode_bound /
 * jda_encode_bound_progressive of its shape and what its own DQT segments can add: a third table, 16-bit entries).
 * The file: SOI, JFIF APP0, one DQT segment per distinct table id of the source in the order Y, Cb, Cr first name it, under the source's id,
 * 8-bit unless an entry passes 255 (libjpeg's emit_dqt); the frame header with component ids 1..3; the encoder's Huffman table assignment.
 * No APPn or COM segment of the source is carried over.
 * Launches: one of jda_rc_extract where a job's source is a baseline image and one of jda_rc_from_coef where a job's is a coefficient image,
 * in the place of the blocks stage; then the stages of the form as they stand: 6 more (BASELINE), 8 more (OPTIMIZE), 10 more (PROGRESSIVE).
 * Per job, in status[i], the rest of the call going on: JDA_UNSUPPORTED_FEATURE -- a 4:4:0 source (the encoder has no such sampling), a
 * source file with an Adobe APP14 segment (dropping it would change how the components are read), a sparse coefficient image, a block with
 * an |AC| above 1023 or a DC outside -1024 .. 1023 (stricter than libjpeg, which refuses only a DC DIFFERENCE beyond category 11: the
 * target's restart interval may differ from the source's, and a difference is not local to a block; no byte of such a job's file is
 * written); JDA_DECODE_ERROR -- a baseline source whose pre-scan validated fewer MCUs than the image has.  From the call,
 * JDA_INVALID_PARAMETER: progressive jobs mixed with others, gray and colour mixed in a progressive call, JDA_RECODE_PROGRESSIVE with a
 * positive restart_interval, a source with both or neither pointer set, a destination that overlaps another.
 * jda_recode_to_host: file in, file out -- a baseline file through jda_prepare + jda_upload, a progressive one through
 * jda_progressive_prepare + jda_coef_upload; only files cross the bus. */
enum { JDA_RECODE_BASELINE = 0, JDA_RECODE_OPTIMIZE = 1, JDA_RECODE_PROGRESSIVE = 2 };
typedef struct jda_recode_source { const jda_dev_image *image; const jda_dev_coef *coef; } jda_recode_source;   /* exactly one is set */
typedef struct jda_recode_job { int32_t form, restart_interval, reserved0, reserved1; } jda_recode_job;         /* restart_interval: -1 the source's, 0 none, 1..65535 */
int jda_recode_bound(const jda_image_info *info, int32_t form, int32_t restart_interval, int64_t *bytes);
int jda_recode_images(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_recode_job *jobs,
                      void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status);
int jda_recode_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t form, int32_t restart_interval,
                       void *host_file, int64_t capacity, int64_t *file_bytes);

/* ---- lossless flip, rotate, transpose and MCU crop: the other half of jpegtran.  Per component the coefficients are a
 * grid C[by, bx, v, u] over the whole MCU grid (v: vertical frequency, u: horizontal).  FLIP_H: C[:, ::-1] * (-1)^u.  FLIP_V: C[::-1] *
 * (-1)^v.  TRANSPOSE: C.transpose(1, 0, 3, 2).  ROT_90 (clockwise): TRANSPOSE then FLIP_H.  ROT_270: TRANSPOSE then FLIP_V.  ROT_180:
 * FLIP_H then FLIP_V.  TRANSVERSE: TRANSPOSE then ROT_180.  DC never changes.  The transposing operations swap width and height, transpose
 * every quantiser table, and need a sampling whose transpose the encoder has: gray, 4:4:4, 4:2:0 (a 4:2:2 source: JDA_UNSUPPORTED_FEATURE
 * for the job).  JDA_XF_EXIF: the operation jda_image_info.orientation names (0, 1: none, 2 FLIP_H, 3 ROT_180, 4 FLIP_V, 5 TRANSPOSE,
 * 6 ROT_90, 7 TRANSVERSE, 8 ROT_270 -- the turn JPEG_AUTO_ROTATE makes); no APPn segment is carried over, so the file has no tag.
 * mcu_rect = { x, y, w, h } in source MCUs, applied BEFORE the operation; all zero: the whole image.  The cropped size in pixels on an
 * axis: min(w * mcu_w, width - x * mcu_w), likewise the height.
 * A source axis that is mirrored (x: FLIP_H, ROT_270; y: FLIP_V, ROT_90; both: ROT_180, TRANSVERSE; none: TRANSPOSE) must be a whole
 * number of MCUs after the crop: without JDA_XF_TRIM the job gets JDA_UNSUPPORTED_FEATURE (jpegtran -perfect); with it the partial last
 * MCU column or row is dropped (jpegtran -trim), and a job of which nothing is left is refused.  An unmirrored ragged edge travels with
 * its blocks.  jpegtran's default (an untransformed edge strip) is not offered.
 * jda_recode_geometry: the shape of the file that comes out (width, height, mcus_x, mcus_y, orientation 0; the rest as the source's), or
 * the job's refusal.  jda_recode_bound_ex: jda_recode_bound of that shape.  jda_recode_images_ex: xforms NULL, or every entry NONE (EXIF
 * over orientation 0 or 1 included) with a zero rectangle: jda_recode_images, launch for launch and byte for byte.  As soon as one job has
 * an operation or a rectangle, the stage in the place of the blocks stage is jda_rc_extract_xf and / or jda_rc_from_coef_xf for every job
 * of the call.  JDA_INVALID_PARAMETER from the call: an unknown op or flag, a rectangle with a negative member, one outside the MCU grid,
 * w or h of 0 with another member non-zero.  Everything else is jda_recode_images': range rule, refusals, forms, restart intervals. */
enum { JDA_XF_NONE = 0, JDA_XF_FLIP_H, JDA_XF_FLIP_V, JDA_XF_TRANSPOSE, JDA_XF_TRANSVERSE, JDA_XF_ROT_90, JDA_XF_ROT_180, JDA_XF_ROT_270, JDA_XF_EXIF };
#define JDA_XF_TRIM 1
typedef struct jda_recode_xform { int32_t op, flags, mcu_rect[4]; } jda_recode_xform;
int jda_recode_geometry(const jda_image_info *info, const jda_recode_xform *xform, jda_image_info *out);
int jda_recode_bound_ex(const jda_image_info *info, const jda_recode_xform *xform, int32_t form, int32_t restart_interval, int64_t *bytes);
int jda_recode_images_ex(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_recode_job *jobs, const jda_recode_xform *xforms,
                         void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status);
int jda_recode_to_host_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t form, int32_t restart_interval, const jda_recode_xform *xform,
                          void *host_file, int64_t capacity, int64_t *file_bytes);

/* ------------------------------------------------------------------ libjpeg-exact decode
 * The decode stages above reproduce the reference, an embedded decoder.  These calls decode with libjpeg's own arithmetic instead, so that
 * the pixels are those of Pillow / libjpeg-turbo (Image.open(f).convert("RGB")): T.81's quantised coefficients times the RAW DQT entries,
 * jidctint.c's 8x8 islow IDCT (32-bit integers, the range-limit table's wrap-around included), "fancy" chroma upsampling over each component's
 * own extent with the edge sample replicated, jdcolor.c's 16-bit colour constants.  The definition is stated in numpy in tests/exact_util.py.
 * Where a pre-limit IDCT result leaves -512 .. 511 libjpeg-turbo's SIMD IDCT saturates and the C code wraps: these calls wrap.
 * Sources as in jda_recode_images -- exactly one pointer set (else JDA_INVALID_PARAMETER from the call): a resident baseline image (its
 * index from the host pre-scan or from JDA_PREPARE_DEVICE_PRESCAN) or a resident coefficient image, dense or sparse.  pixel_types (NULL:
 * RGB8888): JDA_RGB8888 (R, G, B, A = 0xFF; a gray file: R = G = B = Y) or JDA_EIGHT_BIT_GRAYSCALE (the Y plane, Image.draft("L")).
 * outputs: base and pitch as jda_batch_create; exactly the min(width, width_px) x min(height, rows) visible pixels are written -- the
 * image's own size, not the MCU grid's -- and no other byte.  Launches, whatever n: one of jda_exact_planes per (layout, dense | sparse |
 * baseline image) present, one of jda_exact_colour per
 * layout present.  Synchronous, like jda_coef_decode_surfaces.  Per image, in status[i], the rest of the call going on:
 * JDA_INVALID_PARAMETER -- another pixel type, a surface jda_batch_create would refuse; JDA_UNSUPPORTED_FEATURE -- a file with an Adobe
 * APP14 segment, a resident image of a progressive file (its first scan only: pass the coefficient image); JDA_DECODE_ERROR -- a baseline
 * source whose pre-scan validated fewer MCUs than the image has.  A call in which every image is refused launches nothing.
 * jda_exact_decode_planes: the first stage alone, libjpeg's raw-data output: planes[3 i + c] (c: Y, Cb, Cr; a gray image: Y only) receives
 * min(width_px, extent) x min(rows, extent) samples of the component's own extent -- width x height for Y, ceil(width / hs) x
 * ceil(height / vs) for Cb and Cr -- at any base and pitch.
 * jda_decode_to_host_exact: file in, pixels out -- a baseline file through jda_prepare + jda_upload, a progressive one (every scan, no
 * option bit) through jda_progressive_prepare + jda_coef_upload_ex(JDA_COEF_AUTO); host_pixels: width x height pixels at pitch_bytes (a pitch
 * below the width's bytes: JDA_INVALID_PARAMETER), of which min(rows, height) rows are written. */
int jda_exact_decode_surfaces(jda_ctx *ctx, int32_t n, const jda_recode_source *sources, const jda_output *outputs, const int32_t *pixel_types,
                              int32_t *status);
int jda_exact_decode_planes(jda_ctx *ctx, int32_t n, const jda_recode_source *sources, const jda_output *planes, int32_t *status);
int jda_decode_to_host_exact(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, void *host_pixels, int32_t pitch_bytes, int32_t rows);

/* ------------------------------------------------------------------ libjpeg-exact decode at 1/2, 1/4, 1/8
 * libjpeg's scaled decode as Pillow's Image.draft() drives it, bit for bit: scale s in {1, 2, 4, 8}, the output ceil(width / s) x
 * ceil(height / s); every component through a reduced IDCT of its own size (jdmaster.c: 8 / s for luma and for every chroma but 4:2:0's,
 * which takes 16 / s and then needs no upsampling; jidctred.c's 4x4, 2x2 and 1x1, jidctint.c's 8x8); fancy upsampling only above 1/8, h2v1
 * fancy only where the component's own width is above 2, replication otherwise; dequantisation, range limit and colour as at full size.
 * The definition is stated in numpy in tests/exact_scaled_util.py; the window rule of the full-size calls carries over.
 * jda_exact_scaled_geometry: the output size and the own extents of Y, Cb, Cr at that scale (comp_w / comp_h: three entries each, zeros for
 * the components a gray file lacks; any pointer may be NULL).  info: a header jda_parse accepted.  JDA_INVALID_PARAMETER for a scale outside
 * {1, 2, 4, 8} or an empty image, JDA_UNSUPPORTED_FEATURE for a header the decode calls refuse by its layout (not one or three components).
 * jda_exact_draft_scale: the scale Pillow's draft(mode, (req_w, req_h)) chooses: the largest of 8, 4, 2, 1 that does not exceed
 * min(width / req_w, height / req_h) (integer divisions); 1 for a request that is not positive.
 * jda_exact_decode_surfaces_scaled: jda_exact_decode_surfaces with a scale per image (scales == NULL: all 1); the surface receives
 * min(ceil(width / s), width_px) x min(ceil(height / s), rows) pixels and no other byte.  Scales may be mixed in one call.  An image at
 * scale 1 goes through jda_exact_decode_surfaces' own kernels and gets its bytes; launches: one of jda_exact_planes[_scaled] per (layout,
 * dense | sparse | baseline image, scale) present, one of jda_exact_colour[_scaled] per (layout, scale) present.  A scale outside {1, 2, 4, 8}:
 * JDA_INVALID_PARAMETER in status[i]; everything jda_exact_decode_surfaces refuses stays refused.  At 1/8 a resident baseline image whose
 * components all decode to one sample a block (every layout but 4:2:0) is decoded from the DC values of its index alone: its scan is not read.
 * jda_exact_decode_planes_scaled: the planes at their own scaled extents (jda_exact_scaled_geometry's).
 * jda_decode_to_host_exact_scaled: the one call at a scale; host_pixels: ceil(width / s) x ceil(height / s) pixels at pitch_bytes. */
int jda_exact_scaled_geometry(const jda_image_info *info, int32_t scale, int32_t *out_w, int32_t *out_h, int32_t *comp_w, int32_t *comp_h);
int jda_exact_draft_scale(const jda_image_info *info, int32_t req_w, int32_t req_h);
int jda_exact_decode_surfaces_scaled(jda_ctx *ctx, int32_t n, const jda_recode_source *sources, const jda_output *outputs, const int32_t *pixel_types,
                                     const int32_t *scales, int32_t *status);
int jda_exact_decode_planes_scaled(jda_ctx *ctx, int32_t n, const jda_recode_source *sources, const jda_output *planes, const int32_t *scales, int32_t *status);
int jda_decode_to_host_exact_scaled(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t scale, void *host_pixels, int32_t pitch_bytes,
                                    int32_t rows);

/* ------------------------------------------------------------------ libjpeg-exact decode: the file's colour model
 * libjpeg does not read every three-component file as YCbCr.  jdapimin.c's rule, as jda_exact_probe resolves it:
 *   1 component                                                   JDA_CS_GRAY
 *   3 components, a JFIF APP0 segment (it beats an Adobe one)     JDA_CS_YCBCR
 *   3, no JFIF, Adobe APP14 with transform 0                      JDA_CS_RGB     the components ARE R, G, B
 *   3, no JFIF, Adobe with transform 1 or anything else           JDA_CS_YCBCR
 *   3, neither marker, component ids 'R', 'G', 'B'                JDA_CS_RGB
 *   3, neither marker, any other ids                              JDA_CS_YCBCR
 *   4, Adobe transform 0, or no Adobe segment                     JDA_CS_CMYK
 *   4, Adobe transform 2 or anything else                         JDA_CS_YCCK
 * jda_exact_probe: header in, the model out -- with the number of components, the layout of components 0..2 (layout: 0 gray, 1 4:4:4,
 * 2 4:2:0, 3 4:2:2, 4 4:4:0, -1 none of them), the sampling byte of component 3 (k_sampling, 0 without one), the size and the SOF
 * type (jpeg_type: 0 sequential, 1 progressive), and what the rule read.  Four components are taken with components 1 and 2 at 1x1,
 * component 0 at 1x1, 2x1, 1x2 or 2x2 and component 3 at 1x1 or at component 0's factors (Pillow's own CMYK files: 22,11,11,11;
 * Photoshop's YCCK: 22,11,11,22).  Returns jda_parse's code for a header it refuses (an SOF1 frame is let through), and
 * JDA_UNSUPPORTED_FEATURE, the fields filled and decodable 0, for a layout the decode calls below do not take.
 * jda_coef_prepare: every scan of a Huffman-coded 8-bit file on the host -- SOF0 / SOF1 (whole blocks) or SOF2 (jda_progressive_prepare's
 * decoder), interleaved scans or one a component, restart intervals -- into a coefficient image.  One or three components: the image
 * jda_progressive_prepare makes of a progressive file.  Four: the handle holds components 0..2 exactly as a three-component image of their
 * layout (jda_coef_image_coefficients, n_blocks) and component 3 as a gray coefficient image over its own MCU-padded block grid, row-major
 * (jda_coef_image_component3: the parent's, freed with it; NULL for every other image); jda_coef_image_get_info says ncomp 4, and every
 * consumer of coefficient images but the calls below answers JDA_UNSUPPORTED_FEATURE for it: jda_coef_decode_surfaces*, the recode calls,
 * the exact calls without the flag; jda_coef_image_sparse gives none (dense only: JDA_COEF_AUTO picks dense, JDA_COEF_SPARSE is refused).
 * jda_exact_decode_surfaces_ex / _planes_ex: jda_exact_decode_surfaces_scaled / _planes_scaled with flags.  flags 0: those calls to the byte,
 * every refusal included.  JDA_EXACT_COLOUR_MODELS: the file's model decides.  A YCbCr file with an Adobe segment (Photoshop's transform 1,
 * JFIF + Adobe) goes through the kernels of the plain calls.  An RGB-coded one through jda_exact_colour_rgb / jda_exact_colour_scaled_rgb,
 * which write the three upsampled planes as R, G, B (fancy upsampling applies to components 1 and 2 as to chroma), A = 0xFF, at every
 * scale.  A four-component one (a dense coefficient image of jda_coef_prepare, scale 1) through jda_exact_colour4: every component through
 * the islow IDCT with its own raw quantiser and fancy upsampling over its own extent, then Pillow's reading of it ("CMYK;I": a CMYK file's
 * samples s as 255 - s; a YCCK file's components 0..2 through jdcolor.c's YCbCr -> RGB, the bytes R, G, B, 255 - s3), written as
 * JDA_CMYK8888 -- those four bytes, np.asarray(Image.open(f)) -- or as JDA_RGB8888 -- Pillow's convert("RGB") of them: nk = 255 - K,
 * clip8(nk - muldiv255(C, nk)), muldiv255(a, b) = ((t >> 8) + t) >> 8 with t = a b + 128; A = 0xFF.  In these stages a component at most
 * two samples wide is replicated, not interpolated, as jdsample.c does.  Per image, JDA_UNSUPPORTED_FEATURE: JDA_EIGHT_BIT_GRAYSCALE of a
 * four-component or RGB-coded source; a four-component source at a scale other than 1, as a sparse or a baseline image, or of another
 * layout; JDA_INVALID_PARAMETER: JDA_CMYK8888 for another source or without the flag.  Launches: as the scaled calls -- one of
 * jda_exact_planes[_scaled] per (layout, source kind, scale) present, a four-component image's K tiles counted under gray --, then one
 * colour launch per (layout, scale) for the gray / YCbCr images, one for the RGB-coded ones, and one of jda_exact_colour4 per layout;
 * a call that refuses everything launches nothing and writes nothing.  The planes call takes planes[4 i + c] with the flag (three entries
 * an image without it): c = 3 a four-component image's K -- libjpeg's raw-data output, un-inverted, each at its own extent.
 * jda_decode_to_host_exact_ex: jda_decode_to_host_exact_scaled with those flags; a four-component file of any SOF type goes through
 * jda_coef_prepare + jda_coef_upload_ex, a progressive file as ever through jda_progressive_prepare, everything else through the resident
 * baseline image. */
enum { JDA_CS_GRAY = 0, JDA_CS_YCBCR = 1, JDA_CS_RGB = 2, JDA_CS_CMYK = 3, JDA_CS_YCCK = 4 };
enum { JDA_EXACT_COLOUR_MODELS = 1 };
enum { JDA_CMYK8888 = 16 };     /* a pixel type of the _ex calls with the flag, for four-component sources: bytes C, M, Y, K as Pillow's mode "CMYK" */
jda_coef_image *jda_coef_prepare(const uint8_t *jpeg, int32_t len, int32_t *err);
const jda_coef_image *jda_coef_image_component3(const jda_coef_image *img);
typedef struct jda_exact_file {
    int32_t colour_model;       /* JDA_CS_* */
    int32_t ncomp;
    int32_t layout;             /* of components 0..2 */
    int32_t k_sampling;         /* component 3's sampling byte (0x11, 0x22, ..), 0 without one */
    int32_t width, height;
    int32_t jpeg_type;          /* 0 baseline, 1 progressive */
    int32_t decodable;          /* the _ex calls take it with JDA_EXACT_COLOUR_MODELS */
    int32_t jfif, adobe, adobe_transform;   /* what the rule read: APP0 JFIF seen, APP14 Adobe seen, its transform byte (-1 without one) */
    int32_t component_id[4];
} jda_exact_file;
int jda_exact_probe(const uint8_t *jpeg, int32_t len, jda_exact_file *out);
int jda_exact_decode_surfaces_ex(jda_ctx *ctx, int32_t n, const jda_recode_source *sources, const jda_output *outputs, const int32_t *pixel_types,
                                 const int32_t *scales, uint32_t flags, int32_t *status);
int jda_exact_decode_planes_ex(jda_ctx *ctx, int32_t n, const jda_recode_source *sources, const jda_output *planes, const int32_t *scales, uint32_t flags,
                               int32_t *status);
int jda_decode_to_host_exact_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t scale, uint32_t flags, void *host_pixels,
                                int32_t pitch_bytes, int32_t rows);

/* The source rectangle {x0, y0, x1, y1} (half open) that resizing rect = {x, y, w, h} of a src_w x src_h image to out_w x out_h reads with
 * `filter` (JDA_RESIZE_*), clipped at the image: what a caller decodes of a file before it resizes a crop.  Host work only. */
int jda_resize_reads(int32_t src_w, int32_t src_h, const int32_t *rect, int32_t out_w, int32_t out_h, int32_t filter, int32_t *reads);

/* ---- libjpeg-exact decode of a pixel rectangle: only the MCUs the rectangle's pixels read are decoded, and the surface
 * holds the rectangle -- its pixels are the whole decode's, cropped (a horizontally subsampled chroma plane at most two samples wide is
 * replicated at full size too, libjpeg's rule: such a rectangle is Pillow's, where jda_exact_decode_surfaces interpolates).
 * rects: {x, y, w, h} per image, pixels of the image at its scale; NULL: jda_exact_decode_surfaces_ex, launch for launch and byte for byte.
 * An all-zero rectangle: that image whole, through the kernels of the _ex call (whole and cropped images mix in one call).
 * status[i]: JDA_INVALID_PARAMETER for an empty rectangle, a negative origin or one that leaves the image; JDA_UNSUPPORTED_FEATURE for a
 * four-component source with a rectangle; everything jda_exact_decode_surfaces_ex refuses stays refused. */
int jda_exact_decode_surfaces_rect(jda_ctx *ctx, int32_t n, const jda_recode_source *sources, const jda_output *outputs, const int32_t *pixel_types,
                                   const int32_t *scales, uint32_t flags, const int32_t *rects, int32_t *status);
/* the MCU rectangle {mx0, my0, mx1, my1} that call decodes for rect (pixel_type decides whether chroma is decoded at all) */
int jda_exact_rect_mcus(const jda_image_info *info, int32_t scale, int32_t pixel_type, const int32_t *rect, int32_t *mcu_rect);
/* file in, the rectangle's pixels out: w x h pixels at pitch_bytes; tiles (may be NULL): [0] planes-stage tiles launched, [1] those of the whole image */
int jda_decode_to_host_exact_rect(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t scale, uint32_t flags, const int32_t *rect,
                                  void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *tiles);

/* ---- Pillow's Image.thumbnail(): draft, reduce, float-box resize
 * im = Image.open(f); im.thumbnail((req_w, req_h), F, reducing_gap) is four steps, each Pillow's bit for bit: (1) the aspect-preserving
 * final size, (2) draft(): the libjpeg-exact decode at 1/1, 1/2, 1/4 or 1/8, chosen from (int(req_w gap), int(req_h gap)), (3) inside
 * resize(reducing_gap=): Image.reduce((fx, fy), box) when a whole factor >= 2 fits an axis, (4) the convolution resize of a FRACTIONAL box.
 *
 * jda_reduce_surfaces: Image.reduce((fx, fy), box) of n surfaces of one pixel size (1 or 4 bytes) in ONE launch of jda_reduce_tiles.
 * factors: {fx, fy} per job, 1 .. JDA_REDUCE_MAX_FACTOR each (beyond: JDA_UNSUPPORTED_FEATURE; below 1: JDA_INVALID_PARAMETER).  boxes:
 * {x0, y0, x1, y1} per job, half open, inside the source, not empty; NULL: every source whole.  An output pixel is the average of its cell
 * of fx x fy source pixels (n of them; fewer in the box's last column and row), per byte ((sum + n / 2) * floor(2^24 / n)) >> 24 in
 * unsigned 32-bit arithmetic -- Pillow's rule, which is not the rounded mean.  All four bytes of an RGB8888 pixel are averaged (A = 0xFF
 * stays 0xFF).  dst[i].width_px x rows must be ceil(box_w / fx) x ceil(box_h / fy) (jda_reduce_geometry), else JDA_INVALID_PARAMETER;
 * exactly those pixels are written.  Pointers and pitches as jda_resize_surfaces: 16-byte aligned, a destination may share no byte with a
 * source or another destination.  fx = fy = 1 copies the box.  n == 0: JDA_SUCCESS, nothing launched.
 *
 * jda_resize_surfaces_box: jda_resize_surfaces_ex with Pillow's resize(size, F, box = (x0, y0, x1, y1)) for FLOAT boxes, four per job (not
 * NULL).  Pillow's conditions, else JDA_INVALID_PARAMETER: 0 <= x0 < x1 <= width_px, 0 <= y0 < y1 <= rows.  The box is held as float32,
 * its length is x1 - x0 rounded to float32, and from there the taps are worked out in double, as Pillow does.  Same kernels, same limits.
 *
 * jda_thumbnail_plan (host only): what Image.thumbnail((req_w, req_h), F, reducing_gap) does to a src_w x src_h JPEG file.  reducing_gap >=
 * 1.0, or 0: Pillow's None (no draft, no reduce).  JDA_INVALID_PARAMETER: 0 < gap < 1 (or not a number), a size that is not positive, a
 * filter id that is none.  JDA_UNSUPPORTED_FEATURE, the plan filled in all the same: a factor beyond JDA_REDUCE_MAX_FACTOR, a resize
 * beyond JDA_RESIZE_MAX_KSIZE, or an image before the final resize more than 100 times as tall as wide whose height shrinks (Pillow
 * then runs the vertical pass first, with other intermediates).
 *
 * jda_decode_to_host_thumbnail: parse, plan, the libjpeg-exact decode at the plan's scale (baseline and progressive files, as
 * jda_decode_to_host_exact_scaled; four-component and RGB-coded files are refused as there), reduce, resize, copy back:
 * np.asarray(im) after im.thumbnail((req_w, req_h), F, reducing_gap).  pixel_type: JDA_RGB8888 (bytes R, G, B, 0xFF) or
 * JDA_EIGHT_BIT_GRAYSCALE (a gray file as Pillow's mode "L"; of a colour file the luma plane through the same steps, which no single
 * Pillow call makes).  host_pixels: pitch_bytes >= out_w * bpp, rows >= out_h
 * of the plan (a caller sizes it with jda_thumbnail_plan), else JDA_INVALID_PARAMETER and nothing launched.  out_w / out_h may be NULL.
 * launches (may be NULL): [0] reduce launches, [1] resize launches of the call (0 or 1 each). */
#define JDA_REDUCE_MAX_FACTOR 32
typedef struct jda_thumbnail_steps {
    int32_t out_w, out_h;           /* the final size (the source's when the request holds it: then no step at all) */
    int32_t scale;                  /* draft(): 1, 2, 4 or 8 */
    int32_t draft_w, draft_h;       /* im.size after draft(): ceil(src / scale) */
    int32_t fx, fy;                 /* the reduce step's factors; 1, 1: there is none */
    int32_t reduce_box[4];          /* its box {x0, y0, x1, y1} in the draft image (_get_safe_box) */
    int32_t reduced_w, reduced_h;   /* the image the resize reads: the reduce step's output, the draft image without one */
    int32_t resize;                 /* 1: a resize of `box` to out_w x out_h follows; 0: the draft image is the result */
    float box[4];                   /* {x0, y0, x1, y1} in the image the resize reads */
} jda_thumbnail_steps;
int jda_reduce_geometry(int32_t box_w, int32_t box_h, int32_t fx, int32_t fy, int32_t *out_w, int32_t *out_h);
int jda_reduce_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *factors, const int32_t *boxes,
                        const jda_output *dst);
int jda_resize_surfaces_box(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const float *boxes, const jda_output *dst,
                            int32_t filter);
int jda_thumbnail_plan(int32_t src_w, int32_t src_h, int32_t req_w, int32_t req_h, int32_t filter, double reducing_gap, jda_thumbnail_steps *plan);
int jda_decode_to_host_thumbnail(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t req_w, int32_t req_h, int32_t filter, double reducing_gap,
                                 int32_t pixel_type, void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *out_w, int32_t *out_h,
                                 int32_t *launches);

const char *jda_version(void);

#ifdef __cplusplus
}
#endif
#endif /* JPEGDEC_AMD_H */
