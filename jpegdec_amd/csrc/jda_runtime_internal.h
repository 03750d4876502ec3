// jda_runtime_internal.h -- what the pieces of the device runtime (jda_runtime.cpp, jda_pipeline.cpp) share.
#ifndef JDA_RUNTIME_INTERNAL_H
#define JDA_RUNTIME_INTERNAL_H

#include <hip/hip_runtime.h>

#include "jda_internal.h"
#include "jda_plan.h"
#include "jda_exact_plan.h"

// launch lists of a batch: one per (mode, fast_mul, kernel variant, window size, P1 in chunks);
// index = (((mode * 2 + fast) * 4 + variant) * 2 + big) * 2 + cont
#define JDA_N_LISTS (32 * JDA_N_MODES)
#define JDA_LIST_MODE(m) ((m) >> 5)
#define JDA_LIST_FAST(m) (((m) >> 4) & 1)
#define JDA_LIST_VARIANT(m) (((m) >> 2) & 3)
#define JDA_LIST_BIG(m) (((m) >> 1) & 1)
#define JDA_LIST_CONT(m) ((m) & 1)

#define JDA_POOL_SLOTS 192
// A tile taken from the decode kernel's pool starts cold when its image is not the one of the wavefront's tile before, and quads claimed one
// by one rarely are of one image when the images are small: the photographs leg (8 quads an image) ran 2.4 % slower with the pool than without,
// 1280x720 images (23 quads) 1.2 % faster (profiles/decode_pool_ab.txt).  So only lists whose images average this many quads run the pool.
#define JDA_POOL_MIN_QUADS_PER_IMAGE 16
#define JDA_POOL_IDLE_MAX ((size_t)2 << 30)      // idle bytes kept at most
#define JDA_MAX_BANDS 8
struct jda_ctx {
    int device;
    hipStream_t stream;
    hipEvent_t ev_start, ev_stop;
    hipEvent_t ev_band[JDA_MAX_BANDS];   // jda_decode_to_host_bands: one per band of the copy back (made on first use)
    uint8_t *pinned;          // page-locked staging for uploads (grow-only, reused)
    size_t pinned_cap;
    int last_segscan_rounds;  // speculative rounds the last marker-less device pre-scan needed (diagnostics)
    char last_error[256];
    // Device blocks the runtime allocated for itself (resident images, launch plans, the one-call path's surface), kept when
    // released and handed out again: hipFree costs ~0.23 ms and synchronises the device, which was most of a small image's
    // time through jda_decode_to_host (the JPEGDEC class).  Everything of a context runs on its one stream, so a block
    // released while work on it is still queued is safe to reuse: the next user's work queues behind it.
    struct { void *p; size_t bytes; bool busy; } pool[JDA_POOL_SLOTS];
    size_t pool_idle;
};

struct jda_dev_image {
    uint8_t *base;            // one allocation: tables | index | dc | scan
    size_t bytes;
    size_t off_tables, off_index, off_dc, off_scan;
    jda_image_info info;
    uint32_t scan_len, n_mcus_ok;
    uint8_t dc_id[3], ac_id[3], q_id[3];
    uint8_t fast_mul;
    uint8_t general_p1;          // JDA_DESC_GENERAL_P1
    uint8_t prescan_on_device;   // the block index was made on the device (jda_segscan_*)
    size_t off_cont_first, off_cont;   // continuation entries (0 / 0: none uploaded)
    uint32_t n_cont;
    uint32_t tiles_total, tiles_over_small;   // host index known: tiles, and those whose scan slice exceeds the 16-wave kernel's window (0 / 0: unknown)
    uint8_t *tables_host;     // a host copy of the tables (JDA_TABLE_BYTES): a launch plan lets consecutive images with equal tables share the first one's copy
    uint16_t quant_zz[4][64]; // the file's DQT entries by table id (zigzag order) and whether it has an Adobe APP14 segment: a recode's header (jda_recode_plan.h)
    uint8_t adobe;
    uint8_t colour;           // JDA_CS_* (jda_colour_model): what the exact decode's _ex calls read the components as
};
extern "C" void jda_image_raw_quant(const jda_image *img, uint16_t *quant_zz, int32_t *adobe);
extern "C" void jda_coef_image_raw_quant(const jda_coef_image *img, uint16_t *quant_zz, uint8_t *q_id, int32_t *adobe);
// JDA_CS_*: how libjpeg reads the file's components (jda_colour_model; the exact decode's _ex calls)
extern "C" int jda_image_colour_model(const jda_image *img);
extern "C" int jda_coef_image_colour_model(const jda_coef_image *img);

struct jda_dev_coef {
    uint8_t *base;            // one allocation: quantisers (JDA_CT_QUANT_BYTES) | coefficients (n_blocks x 128 bytes)  -- JDA_COEF_DENSE
    size_t bytes;             //                 quantisers | first[n_blocks + 1] | entries[n_entries], each part 16-byte aligned -- JDA_COEF_SPARSE
    jda_image_info info;
    uint8_t q_id[3];
    uint32_t n_blocks;
    int form;                 // what is resident
    uint32_t n_entries;
    size_t off_entries;       // the coefficients (dense) / the entries (sparse)
    uint16_t raw_quant[3][64]; // the DQT entries of Y, Cb, Cr as the file lists them, the ids its frame header gives them, its Adobe APP14 flag (a recode's header)
    uint8_t raw_qid[3], adobe;
    uint8_t colour;           // JDA_CS_* (jda_colour_model)
    // a four-component image (jda_coef_prepare; info.ncomp == 4): everything above is components 0..2 as a three-component image, and
    // component 3 is this gray image over its own MCU-padded block grid, uploaded and freed with this one.  NULL otherwise.
    jda_dev_coef *k;
};

// launch plan of a call over coefficient images: descs | tile lists of (form, layout), in one host blob that goes to the device as it is
struct jda_coef_plan {
    std::vector<uint8_t> blob;
    size_t off[2][JDA_N_MODES];
    uint32_t n_tiles[2][JDA_N_MODES];
    int n_launches;           // (form, layout) pairs present
};
// (defined inside jda_runtime.cpp's extern "C" block)
// per_image_err != NULL: an image that cannot be planned (a scale bit, a surface too small) gets its code there and is left out; else the call fails
extern "C" int jda_coef_pick_form(const jda_coef_image *img, int32_t form, int *picked, size_t *payload_bytes);
extern "C" int jda_coef_plan_build(int32_t n, const jda_dev_coef *const *imgs, const jda_output *outputs, const int32_t *pixel_types, const int32_t *options,
                                   const int32_t *mcu_rects, int32_t *per_image_err, jda_coef_plan *plan);
// the launches alone: the blob is in `block` already, or its copy is queued in front
extern "C" hipError_t jda_coef_plan_launch_kernels(const jda_coef_plan &plan, const uint8_t *block, hipStream_t stream);
extern "C" hipError_t jda_coef_plan_launch(const jda_coef_plan &plan, uint8_t *block, hipStream_t stream);

struct jda_batch {
    int32_t n_images;
    jda_dev_desc *d_descs;
    jda_strip *d_strips[JDA_N_LISTS];
    uint32_t n_strips[JDA_N_LISTS];
    jda_batch_stats stats;
    uint32_t flat_max_items;    // JDA_LIST_THUMB_FLAT: the launch's width
    uint8_t pool_ok[JDA_N_LISTS];   // the list's launch may deal its last quads at run time (jda_launch_decode): one table generation, JDA_POOL_MIN_QUADS_PER_IMAGE
    int32_t *status;            // per image: JDA_SUCCESS / JDA_DECODE_ERROR (bad MCU) / JDA_INVALID_PARAMETER (hole)
};


int jda_set_err(jda_ctx *ctx, hipError_t e, const char *what);
hipError_t jda_pool_alloc(jda_ctx *ctx, void **out, size_t bytes);
void jda_pool_free(jda_ctx *ctx, void *p);
extern "C" jda_batch *jda_batch_create_strips(jda_ctx *ctx, int32_t n, jda_dev_image *const *images, const jda_output *outputs, const int32_t *pixel_types,
                                              const int32_t *options, const int32_t *mcu_rects, const int32_t *strip_mcus, int32_t *err);
int jda_plain_variant(const jda_dev_desc &D);
extern "C" int jda_host_range_of(const void *p, size_t len, uintptr_t *base, size_t *bytes);   // the page-locked range (jda_host_alloc / jda_host_register) that holds [p, p + len)
// which launch list an image's tiles go to: ((mode * 2 + fast) * 4 + variant) * 2 + big.  The combination fast = 0, variant = 3 (no
// plain-case kernel exists without the 24-bit multiplies) names the DC thumbnail kernel: 1/8 scale -- also every progressive
// file's DC scan at its default scale --, whose pixels are the blocks' DC values (jpeg.inl:5146-5154): no scan, no index, no IDCT
#define JDA_LIST_THUMB(mode) (((((mode) * 2 + 0) * 4 + 3) * 2 + 0) * 2 + 0)
// .. and the same with big = 1 the 1/4-scale kernel (jda_quarter_tiles): a block is its DC value, <= 4 AC symbols and a 2x2 IDCT
// (jpeg.inl:2305-2326).  (A strip-major surface at 1/4 stays with the decode kernel, whose colour stage knows the layout.)
#define JDA_LIST_QUARTER(mode) (((((mode) * 2 + 0) * 4 + 3) * 2 + 1) * 2 + 0)
// .. and (fast = 0, variant = 3, cont = 1) the flat thumbnail kernels: a WHOLE gray or 4:2:0 image at 1/8 on a row-major surface is a
// pointwise map of its DC array -- the list holds one record per image (jda_dc_thumbnail_flat)
#define JDA_LIST_THUMB_FLAT(mode) (((((mode) * 2 + 0) * 4 + 3) * 2 + 0) * 2 + 1)
#define JDA_LIST_IS_THUMB_FLAT(m) ((m) == JDA_LIST_THUMB_FLAT(JDA_MODE_GRAY) || (m) == JDA_LIST_THUMB_FLAT(JDA_MODE_420))
// whole: every MCU of the image is launched (no crop rectangle)
inline int jda_list_index(const jda_dev_desc &D, int variant, int big, int cont = 0, bool whole = false)
{
    if (D.strip_mcus == 0) {                                      // (a strip-major surface stays with the decode kernel, whose colour stage knows the layout)
        if (D.scale_shift == 3 && whole && (D.mode == JDA_MODE_GRAY || D.mode == JDA_MODE_420)) return JDA_LIST_THUMB_FLAT(D.mode);
        if (D.scale_shift == 3) return JDA_LIST_THUMB(D.mode);
        if (D.scale_shift == 2) return JDA_LIST_QUARTER(D.mode);
    }
    return (((D.mode * 2 + (D.fast_mul ? 1 : 0)) * 4 + variant) * 2 + big) * 2 + cont;
}
int jda_use_cont(const jda_dev_desc &D, int variant, uint32_t n_cont);
int jda_big_window(const jda_dev_desc &D, int variant, uint32_t tiles_total = 0, uint32_t tiles_over_small = 0);
// (jda_fill_launch_desc, the descriptor of one image of a launch plan: jda_plan.h)

extern "C" hipError_t jda_launch_segscan_fused(const jda_segscan_params *params, uint32_t n_images, uint32_t max_segs, uint32_t round, hipStream_t stream);
extern "C" hipError_t jda_launch_checksum(const void *base, uint32_t pitch, uint32_t row_bytes, uint32_t rows, unsigned long long *out, hipStream_t stream);
// n GRAY8 canvases -> packed 4 / 2 / 1-bpp rows, one workgroup an image; *fail (device, zeroed by the caller) is raised if a wavefront gave up waiting
extern "C" hipError_t jda_launch_dither(const jda_dither_job *jobs, uint32_t n, uint32_t max_w, uint32_t max_h, uint32_t *fail, hipStream_t stream);
// n surfaces of one pixel size -> their EXIF orientations, one workgroup a destination tile; n_tiles: the length of the flat tile list
extern "C" hipError_t jda_launch_orient(const jda_orient_job *jobs, uint32_t n, uint32_t n_tiles, uint32_t bytes_per_pixel, hipStream_t stream);
// n jobs of one source pixel size (bpp 1 or 4), layout (hwc: pixel-major, RGB8888 sources only) and element size (es 1: bytes, 2 / 4: through
// `table`, device memory), one workgroup a tile of 4 KiB of destination; n_tiles: the length of the flat tile list
extern "C" hipError_t jda_launch_pack(const jda_pack_job *jobs, uint32_t n, uint32_t n_tiles, int hwc, uint32_t es, const uint8_t *table,
                                      uint32_t bpp, uint32_t bgr, hipStream_t stream);
// n jobs of one destination pixel size (bpp 1 or 4), layout (hwc: pixel-major, RGB8888 destinations only) and element size (es 1: bytes,
// 2 / 4: float16 / float32 through scale_bias = scale[0..2], bias[0..2] per tensor channel, HOST memory: they travel as kernel arguments),
// one workgroup a tile of 256 destination vectors; n_tiles: the length of the flat tile list
extern "C" hipError_t jda_launch_unpack(const jda_unpack_job *jobs, uint32_t n, uint32_t n_tiles, int hwc, uint32_t es, const float *scale_bias,
                                        uint32_t bpp, uint32_t bgr, hipStream_t stream);
// n jobs of one pixel size (1 or 4) resized through the tap tables in `tables` (device memory; the jobs carry where theirs begin), one
// workgroup a tile of 64 output dwords x the job's tile rows; n_tiles: the length of the flat tile list, lds_bytes: the largest tile's LDS;
// signed_taps: the tables of a filter with negative taps (BICUBIC, LANCZOS), run by jda_resize_tiles_signed
extern "C" hipError_t jda_launch_resize(const jda_resize_job *jobs, uint32_t n, uint32_t n_tiles, uint32_t bytes_per_pixel, uint32_t signed_taps, const int32_t *tables,
                                        uint32_t lds_bytes, hipStream_t stream);
// n jobs of one pixel size (1 or 4) shrunk by their whole factors (jda_reduce_tiles; jda_rd_* in jda_device_core.h), one workgroup a tile
// of 256 output bytes x the job's tile rows; n_tiles: the length of the flat tile list, lds_bytes: the largest tile's LDS
extern "C" hipError_t jda_launch_reduce(const jda_reduce_job *jobs, uint32_t n, uint32_t n_tiles, uint32_t bytes_per_pixel, uint32_t lds_bytes, hipStream_t stream);
// one of the seven launches of jda_encode_surfaces (JDA_EN_STAGE_*; jda_en_* in jda_device_core.h); the host sizes the unstuffed scans behind stage 2
extern "C" hipError_t jda_launch_encode_stage(const jda_en_arrays *A, uint32_t stage, uint32_t n_blocks, uint32_t n_chunks, hipStream_t stream);
// the two more of a call with an optimised job (JDA_EN_STAGE_GATHER into the call's zeroed histograms, JDA_EN_STAGE_OPT_LENGTHS; jda_ho_*)
extern "C" hipError_t jda_launch_huffopt_stage(const jda_en_arrays *A, uint32_t stage, uint32_t n_blocks, uint32_t *hist, hipStream_t stream);
// one stage of a progressive call (JDA_PE_STAGE_*; jda_pe_* in jda_device_core.h)
extern "C" hipError_t jda_launch_progenc_stage(const jda_pe_arrays *A, uint32_t stage, uint32_t n_blocks, uint32_t n_units, uint32_t n_jobs, uint32_t n_chunks, uint32_t *hist,
                                               hipStream_t stream);
// the launches of a recode call in the place of the blocks stage (jda_rc_extract and / or jda_rc_from_coef; jda_rc_* in jda_device_core.h)
extern "C" hipError_t jda_launch_recode_blocks(const jda_en_arrays *A, const jda_rc_src *src, uint32_t *bad, uint32_t n_blocks, int any_image, int any_coef,
                                               hipStream_t stream);
// .. and of one in which a job flips, turns, transposes or crops (jda_rc_extract_xf and / or jda_rc_from_coef_xf): a transform record a job
extern "C" hipError_t jda_launch_recode_blocks_xf(const jda_en_arrays *A, const jda_rc_src *src, const jda_rc_xf *xf, uint32_t *bad, uint32_t n_blocks, int any_image,
                                                  int any_coef, hipStream_t stream);
// What a recode call hands the encoder's host code (jda_runtime.cpp, jda_encode_progressive.cpp) in the place of pixels: the source records
// of its jobs; d_src / d_bad: their place, and that of the jobs' range words, in the call's scratch (the encoder's code sets them); bad: the
// words as they came back at the call's first wait -- a job whose word is set gets capacity 0 before the write stage, so no byte of it is written
struct jda_rc_hook {
    std::vector<jda_rc_src> src;
    int any_image, any_coef;
    jda_rc_src *d_src;
    uint32_t *d_bad;
    std::vector<uint32_t> bad;
    std::vector<jda_rc_xf> xf;      // empty: no job of the call has a transform; else a record a job, d_xf their place in the scratch
    jda_rc_xf *d_xf;
};
// the hook's launches in the place of the blocks stage
static inline hipError_t jda_rc_hook_launch(const jda_en_arrays *A, const jda_rc_hook &H, uint32_t n_blocks, hipStream_t stream)
{
    if (!H.xf.empty()) return jda_launch_recode_blocks_xf(A, H.d_src, H.d_xf, H.d_bad, n_blocks, H.any_image, H.any_coef, stream);
    return jda_launch_recode_blocks(A, H.d_src, H.d_bad, n_blocks, H.any_image, H.any_coef, stream);
}
struct jda_pe_plan_out;
// the progressive encoder's three parts over a plan that is made (jda_recode_plan.h), its blocks stage the hook's; totals: a job each
int jda_progenc_recode(jda_ctx *ctx, jda_pe_plan_out &P, jda_rc_hook &hook, std::vector<jda_encode_totals> &totals);
extern "C" hipError_t jda_launch_segscan_tail(const jda_segscan_params *params, uint32_t n_images, uint32_t max_segs, uint32_t first_round, uint32_t max_round, hipStream_t stream);
extern "C" hipError_t jda_launch_filter(const jda_filter_params *params, uint32_t n_images, uint32_t max_raw_len, hipStream_t stream);
extern "C" hipError_t jda_launch_fill_strips(const jda_strips_params *params, uint32_t n_images, uint32_t max_tiles, hipStream_t stream);
extern "C" hipError_t jda_launch_walk_tables(const jda_segscan_params *params, uint32_t n_images, hipStream_t stream);   // before the first walk
extern "C" hipError_t jda_launch_segscan_sums(const jda_segscan_params *params, uint32_t n_images, hipStream_t stream);
extern "C" hipError_t jda_launch_prescan_passes(const jda_segscan_params *params, uint32_t n_images, uint32_t max_segs, uint32_t list_rounds, uint32_t max_round,
                                                int any_record, hipStream_t stream);
// the same, or -- states_first -- the order for a batch too small to fill the GPU: exit states first (SPEC walks), then ONE recording round
extern "C" hipError_t jda_launch_prescan_passes_ex(const jda_segscan_params *params, uint32_t n_images, uint32_t max_segs, uint32_t list_rounds, uint32_t max_round,
                                                   int any_record, int states_first, hipStream_t stream);
// aux: JDA_LIST_THUMB_FLAT: the most items an image of the batch's flat lists has (jda_flat_items); 0 otherwise
// pool_ok: every record of the list has one table generation (jda_strip::ord) and the launches on `stream` run one after the other: the
// persistent kernel may deal the launch's last quads at run time (jda_pool_resolve in jda_kernels.hip); 0: the static split
extern "C" hipError_t jda_launch_decode(int mode, int fast_mul, int variant, int big, int cont, const jda_dev_desc *descs, const jda_strip *strips,
                                        uint32_t n_strips, uint32_t aux, int pool_ok, hipStream_t stream);
// a stream that launched decodes is about to be destroyed: its counter slot of the pool is free again
extern "C" void jda_decode_pool_release(hipStream_t stream);
// tiles of coefficient images of one MCU layout (descs[i].scan: coefficients, .tables: JDA_CT_QUANT_BYTES of quantisers): jda_coef_tiles<mode>
extern "C" hipError_t jda_launch_coef_tiles(int mode, const jda_dev_desc *descs, const jda_strip *tiles, uint32_t n_tiles, hipStream_t stream);
// the same from the sparse form (descs[i].tables: quantisers | first[], .scan: entries): jda_sparse_tiles<mode>
extern "C" hipError_t jda_launch_sparse_tiles(int mode, const jda_dev_desc *descs, const jda_strip *tiles, uint32_t n_tiles, hipStream_t stream);
// one launch of a libjpeg-exact decode call (jda_exact_plan.h): the kernel of L.kind for images of layout L.mode decoded
// at L.scale over the L.n_tiles records at `tiles`; descs, ex, src: the call's records, one an image (descs as for the two launches above, src
// read for baseline images), rects: the rectangle records beside ex (read by the two rectangle kinds alone)
extern "C" hipError_t jda_launch_exact(const jda_exact_launch &L, const jda_dev_desc *descs, const jda_ex_desc *ex, const jda_ex_src *src, const jda_exr_rec *rects,
                                       const jda_strip *tiles, hipStream_t stream);
inline uint32_t jda_flat_items(const jda_dev_desc &D) { return (D.mode == JDA_MODE_GRAY ? (D.mcus_x + 3u) >> 2 : D.mcus_x) * D.mcus_y; }      // quads of blocks (gray) / MCUs

#endif
