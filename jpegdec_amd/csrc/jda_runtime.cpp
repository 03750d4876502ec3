// jda_runtime.cpp -- device runtime behind the C-ABI: context (device, stream, events), resident
// images, batch launch plans.  The reference has no such layer (it is a single-threaded
// streaming decoder); this is the seam that replaces the body of the MCU loops of
// DecodeJPEG (reference src/jpeg.inl:5109-5353) with one kernel launch per batch.
//
// There is NO CPU fallback here: every entry point reports JDA_ERROR_NO_DEVICE / JDA_ERROR_HIP
// when the HIP device or a HIP call is not available.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <vector>

#include <map>
#include <mutex>

#include "jda_runtime_internal.h"
#include "jda_pack_plan.h"
#include "jda_unpack_plan.h"
#include "jda_resize_plan.h"
#include "jda_reduce_plan.h"
#include "jda_thumbnail_plan.h"
#include "jda_encode_plan.h"
#include "jda_recode_plan.h"
#include "jda_prescan_plan.h"

extern "C" uint32_t jda_image_fast_mul(const jda_image *img);
extern "C" uint32_t jda_image_general_p1(const jda_image *img);
extern "C" const uint32_t *jda_image_restart_positions(const jda_image *img, uint32_t *n);
extern "C" void jda_image_run_host_prescan(jda_image *img);
extern "C" int jda_image_index_on_device(const jda_image *img);
extern "C" uint32_t jda_image_record_cap(const jda_image *img);
extern "C" void jda_image_adopt_prescan(jda_image *img, uint32_t n_mcus_ok, uint32_t max_ac_bits, int32_t max_abs_dc, uint32_t trunc_events);
// The plain-case kernel variants (jda_desc_uniform in jda_kernels.hip): full size, every multiply in 24 bits, no stream flags,
// and one of the (layout, output format) pairs a kernel was built for.  0 = the general kernel.
int jda_plain_variant(const jda_dev_desc &D)
{
    if (D.scale_shift != 0 || D.pad_[0] != 0 || !D.fast_mul || D.strip_mcus != 0) return 0;
    const bool colour = D.mode != JDA_MODE_GRAY;
    if (D.pixel_type == JDA_RGB8888 && !D.gray_from_color) return (D.mode == JDA_MODE_444 || D.mode == JDA_MODE_420 || D.mode == JDA_MODE_422) ? 1 : 0;
    if (D.pixel_type == JDA_RGB565_LITTLE_ENDIAN && colour && !D.gray_from_color) return (D.mode == JDA_MODE_444 || D.mode == JDA_MODE_420) ? 2 : 0;
    if (D.pixel_type == JDA_EIGHT_BIT_GRAYSCALE) return (D.mode == JDA_MODE_GRAY || (D.mode == JDA_MODE_420 && D.gray_from_color)) ? 3 : 0;
    return 0;
}

// High-bitrate images go to the kernel variant with one wavefront less per CU and a larger scan window (jda_lds_layout<MODE, 1>):
// a tile whose slice of the scan does not fit the window takes the general bit reader, which goes to HBM at every refill.
// Decided per image from its average bytes of scan per full tile (+ 50 % for the spread between tiles), or from the tiles' slices
// themselves where the host made the index; every decode kernel takes either layout (a launch argument).
int jda_big_window(const jda_dev_desc &D, int variant, uint32_t tiles_total, uint32_t tiles_over_small)
{
    static const int forced = []() { const char *e = JDA_LAB_ENV("JDA_BIG_WINDOW"); return e ? atoi(e) : -1; }();
    if (D.scale_shift == 3) return 0;                             // JDA_LIST_THUMB (or, strip-major, the decode kernel without a window)
    if (D.scale_shift == 2 && D.strip_mcus == 0) return 1;        // JDA_LIST_QUARTER: its lists are padded as the large-window kernels' (no window is staged)
    if (forced >= 0) return forced ? 1 : 0;
    // the index was made on the host: the tiles' slices are known exactly -- the larger window (and the wavefront it costs) only
    // when more than one tile in a hundred does not fit the smaller one
    if (tiles_total) return (uint64_t)tiles_over_small * 100u > tiles_total ? 1 : 0;
    const uint64_t n_mcus = (uint64_t)D.mcus_x * D.mcus_y;
    if (!n_mcus) return 0;
    const uint64_t avg = (uint64_t)D.scan_len * jda_mcus_per_tile(D.mode) / n_mcus;
    return avg + avg / 2 + 48 > jda_window_bytes(D.mode, 0) ? 1 : 0;
}

// P1 in chunks: for an image that HAS continuation entries (the serial pre-scan wrote them: the image lies in the window in which
// the mode was measured to pay, or its caller asked for them: JDA_PREPARE_CONT_*) and whose decode has such a kernel -- the RGB8888
// plain case of 4:2:0 and 4:4:4
int jda_use_cont(const jda_dev_desc &D, int variant, uint32_t n_cont)
{
    if (!n_cont || variant != 1 || (D.mode != JDA_MODE_420 && D.mode != JDA_MODE_444)) return 0;
    return 1;
}

int jda_set_err(jda_ctx *ctx, hipError_t e, const char *what)
{
    if (ctx) snprintf(ctx->last_error, sizeof(ctx->last_error), "%s: %s", what, hipGetErrorString(e));
    return JDA_ERROR_HIP;
}

#define JDA_HIP(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return jda_set_err((ctx), e_, #call); } while (0)

static inline size_t align16(size_t v) { return jda_a16(v); }

hipError_t jda_pool_alloc(jda_ctx *ctx, void **out, size_t bytes)
{
    if (!bytes) bytes = 16;
    int best = -1, empty = -1;
    for (int i = 0; i < JDA_POOL_SLOTS; i++) {
        if (!ctx->pool[i].p) { if (empty < 0) empty = i; continue; }
        if (!ctx->pool[i].busy && ctx->pool[i].bytes >= bytes && ctx->pool[i].bytes <= 2 * bytes + 65536 &&
            (best < 0 || ctx->pool[i].bytes < ctx->pool[best].bytes)) best = i;
    }
    if (best >= 0) { ctx->pool[best].busy = true; ctx->pool_idle -= ctx->pool[best].bytes; *out = ctx->pool[best].p; return hipSuccess; }
    const hipError_t e = hipMalloc(out, bytes);
    if (e == hipSuccess && empty >= 0) { ctx->pool[empty].p = *out; ctx->pool[empty].bytes = bytes; ctx->pool[empty].busy = true; }
    return e;          // (no slot left: the block is not tracked and pool_free hands it to hipFree)
}
void jda_pool_free(jda_ctx *ctx, void *p)
{
    if (!p) return;
    for (int i = 0; i < JDA_POOL_SLOTS; i++)
        if (ctx->pool[i].p == p) {
            ctx->pool[i].busy = false;
            ctx->pool_idle += ctx->pool[i].bytes;
            while (ctx->pool_idle > JDA_POOL_IDLE_MAX) {           // too much idle memory: give the largest idle blocks back
                int big = -1;
                for (int k = 0; k < JDA_POOL_SLOTS; k++)
                    if (ctx->pool[k].p && !ctx->pool[k].busy && (big < 0 || ctx->pool[k].bytes > ctx->pool[big].bytes)) big = k;
                if (big < 0) break;
                (void)hipFree(ctx->pool[big].p);
                ctx->pool_idle -= ctx->pool[big].bytes;
                ctx->pool[big].p = NULL; ctx->pool[big].bytes = 0;
            }
            return;
        }
    (void)hipFree(p);
}

// The measuring hooks' loop (jda_internal_*_time): launch() reps times, each between the context's two timer events on its stream, ms[k]:
// repeat k; then the stream drained, the plan's block (may be NULL) released, and HIP's error under the hook's name.
template <class Launch>
static int timed_launches(jda_ctx *ctx, int32_t reps, float *ms, void *block, const char *who, Launch launch)
{
    int rc = JDA_SUCCESS;
    hipError_t e = hipSuccess;
    for (int k = 0; k < reps && rc == JDA_SUCCESS && e == hipSuccess; k++) {
        e = hipEventRecord(ctx->ev_start, ctx->stream);
        if (e == hipSuccess) rc = launch();
        if (e == hipSuccess) e = hipEventRecord(ctx->ev_stop, ctx->stream);
        if (e == hipSuccess) e = hipEventSynchronize(ctx->ev_stop);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[k], ctx->ev_start, ctx->ev_stop);
    }
    (void)hipStreamSynchronize(ctx->stream);
    jda_pool_free(ctx, block);
    if (rc != JDA_SUCCESS) return rc;
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, who);
}
// The tail of jda_{orient,pack,resize}_surfaces: the launch is queued (launch_rc: what it said); the stream drained, the plan's block
// released, and HIP's error under the entry point's name.
static int finish_surfaces(jda_ctx *ctx, int launch_rc, void *block, const char *who)
{
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    jda_pool_free(ctx, block);
    if (launch_rc != JDA_SUCCESS) return launch_rc;
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, who);
}
// Rows of a device surface to host memory and the wait for them: one piece where neither side has a gap between its rows (and the caller
// allows it), else a 2-D copy.
static int copy_rows_back(jda_ctx *ctx, void *host, size_t host_pitch, const void *from, size_t from_pitch, size_t row_bytes, size_t rows, bool one_piece_ok)
{
    hipError_t e;
    if (one_piece_ok && host_pitch == from_pitch && row_bytes == from_pitch) e = hipMemcpyAsync(host, from, row_bytes * rows, hipMemcpyDeviceToHost, ctx->stream);
    else e = hipMemcpy2DAsync(host, host_pitch, from, from_pitch, row_bytes, rows, hipMemcpyDeviceToHost, ctx->stream);
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }      // (also after an error: the surface goes back to the pool)
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "copy back");
}

extern "C" {

int jda_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

jda_ctx *jda_create(int32_t device, int32_t *err)
{
    int32_t dummy;
    if (!err) err = &dummy;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { *err = JDA_ERROR_NO_DEVICE; return NULL; }
    jda_ctx *ctx = new (std::nothrow) jda_ctx;
    if (!ctx) { *err = JDA_ERROR_MEMORY; return NULL; }
    memset(ctx, 0, sizeof(*ctx));
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev_start) != hipSuccess || hipEventCreate(&ctx->ev_stop) != hipSuccess) {
        delete ctx;
        *err = JDA_ERROR_NO_DEVICE;
        return NULL;
    }
    *err = JDA_SUCCESS;
    return ctx;
}

void jda_destroy(jda_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipEventDestroy(ctx->ev_start);
    (void)hipEventDestroy(ctx->ev_stop);
    for (int i = 0; i < JDA_MAX_BANDS; i++) if (ctx->ev_band[i]) (void)hipEventDestroy(ctx->ev_band[i]);
    jda_decode_pool_release(ctx->stream);
    (void)hipStreamDestroy(ctx->stream);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    for (int i = 0; i < JDA_POOL_SLOTS; i++) if (ctx->pool[i].p) (void)hipFree(ctx->pool[i].p);
    delete ctx;
}

const char *jda_last_hip_error(const jda_ctx *ctx) { return ctx ? ctx->last_error : "no context"; }
void *jda_stream(jda_ctx *ctx) { return ctx ? (void *)ctx->stream : NULL; }

// The page-locked host ranges the library has made or been told of (jda_host_alloc / jda_host_register), by base address:
// jda_pipeline_submit_ex(.., JDA_SUBMIT_PINNED_INPUT) lets the copy engine read a file where it lies only when the file lies
// inside ONE of them, and joins two files into one copy command only inside the same one (a copy that runs over the end of a
// page-locked object, or across the gap between two, is not the caller's memory to read).
namespace {
std::mutex g_host_ranges_mu;
std::map<uintptr_t, size_t> g_host_ranges;
void host_range_add(void *p, size_t bytes) { std::lock_guard<std::mutex> g(g_host_ranges_mu); g_host_ranges[(uintptr_t)p] = bytes; }
void host_range_del(void *p) { std::lock_guard<std::mutex> g(g_host_ranges_mu); g_host_ranges.erase((uintptr_t)p); }
}
// the range [*base, *base + *bytes) that holds [p, p + len); 0 when no single known range does
int jda_host_range_of(const void *p, size_t len, uintptr_t *base, size_t *bytes)
{
    std::lock_guard<std::mutex> g(g_host_ranges_mu);
    auto it = g_host_ranges.upper_bound((uintptr_t)p);
    if (it == g_host_ranges.begin()) return 0;
    --it;
    if ((uintptr_t)p + len > it->first + it->second) return 0;
    *base = it->first; *bytes = it->second;
    return 1;
}
void *jda_host_alloc(size_t bytes)
{
    void *p = NULL;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable) != hipSuccess) return NULL;      // (every GPU of the node may read it: jda_node)
    host_range_add(p, bytes ? bytes : 16);
    return p;
}
void jda_host_free(void *p) { if (p) { host_range_del(p); (void)hipHostFree(p); } }
int jda_host_register(void *p, size_t bytes)
{
    if (!p || !bytes || hipHostRegister(p, bytes, hipHostRegisterPortable) != hipSuccess) return JDA_ERROR_HIP;
    host_range_add(p, bytes);
    return JDA_SUCCESS;
}
int jda_host_unregister(void *p)
{
    if (!p) return JDA_ERROR_HIP;
    host_range_del(p);
    return hipHostUnregister(p) == hipSuccess ? JDA_SUCCESS : JDA_ERROR_HIP;
}

void *jda_malloc(jda_ctx *ctx, size_t bytes)
{
    if (!ctx) return NULL;
    void *p = NULL;
    (void)hipSetDevice(ctx->device);
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc"); return NULL; }
    return p;
}

void jda_free(jda_ctx *ctx, void *dptr)
{
    if (ctx && dptr) { (void)hipSetDevice(ctx->device); (void)hipFree(dptr); }
}

int jda_memset(jda_ctx *ctx, void *dptr, int value, size_t bytes)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    JDA_HIP(ctx, hipMemsetAsync(dptr, value, bytes, ctx->stream));
    JDA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JDA_SUCCESS;
}

int jda_copy_to_host(jda_ctx *ctx, void *host, const void *dptr, size_t bytes)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    JDA_HIP(ctx, hipMemcpyAsync(host, dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    JDA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JDA_SUCCESS;
}

int jda_copy_to_device(jda_ctx *ctx, void *dptr, const void *host, size_t bytes)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    JDA_HIP(ctx, hipMemcpyAsync(dptr, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    JDA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JDA_SUCCESS;
}

// Upload n prepared images.  Images whose block index is still pending (JDA_PREPARE_DEVICE_PRESCAN) get it made on the
// GPU, all of them by the same launches (one grid row per image; the passes of DESIGN.md 5.3) -- the walk is latency-bound per
// lane, so it is the number of segments in flight that makes it fast.  out[i] receives the device image (NULL on failure).
static double now_ms()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

int jda_upload_batch(jda_ctx *ctx, int32_t n, jda_image *const *imgs, jda_dev_image **out)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    const bool trace = JDA_LAB_ENV("JDA_UPLOAD_TRACE") != NULL;          // stage timings on stderr (diagnostics)
    const double t_begin = now_ms();
    double t_mark = t_begin;
#define JDA_UP_MARK(what) do { if (trace) { (void)hipStreamSynchronize(ctx->stream); const double t_ = now_ms(); fprintf(stderr, "jda_upload_batch: %-28s %8.3f ms\n", what, t_ - t_mark); t_mark = t_; } } while (0)
    if (n <= 0 || !imgs || !out) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    struct Item {
        jda_dev_image *d; uint8_t *stage; std::vector<uint8_t> heap; bool on_device; uint32_t n_int;
        size_t alloc, n_blocks; uint32_t tbytes;
        // the index is made on the device (8f N1 / N2): segments of the scan, see jda_seg_walk
        bool seg_mode; uint32_t n_segs; size_t off_ea, off_sum, off_start, off_wl, off_rp, off_wt, off_ev, off_sstats;
        bool record; uint32_t rec_cap, cand_cap; size_t off_recs, off_cands, zero_end;      // RECORD mode of the pre-scan (no restart intervals)
        std::vector<uint32_t> rp;            // restart positions + the sentinel, until their copy has been made
        uint32_t sst[JDA_ST_WORDS];
    };
    std::vector<Item> items((size_t)n);
    int rc = JDA_SUCCESS;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n; i++) out[i] = NULL;
    auto fail_all = [&](int code) {
        for (int i = 0; i < n; i++) { if (items[i].d) { if (items[i].d->base) jda_pool_free(ctx, items[i].d->base); delete items[i].d; items[i].d = NULL; } out[i] = NULL; }
        return code;
    };
    std::vector<jda_segscan_params> seg_params;
    std::vector<int> seg_owner;
    uint32_t max_segs = 0;
    // staging: slices of one page-locked buffer (H2D at link speed, truly asynchronous); when it is full the
    // copies in flight are drained and it is reused from the start
    const size_t kPinnedMax = (size_t)512 << 20;
    size_t pin_off = 0;
    // host copies into the page-locked buffer are the bulk of an upload's host time: they are collected and done by a
    // few threads, and each image's H2D copies are enqueued when its bytes are in place
    struct StageJob { uint8_t *dst; const uint8_t *src; size_t bytes; int image; };
    std::vector<StageJob> stage_jobs;
    hipError_t stage_err = hipSuccess;
    auto flush_stage_jobs = [&]() {
        if (stage_jobs.empty()) return;
        const size_t nj = stage_jobs.size();
        const unsigned hw = std::thread::hardware_concurrency();
        const size_t nt = std::min<size_t>(std::min<size_t>(nj, 8), hw ? hw : 1);
        std::atomic<size_t> next(0);
        auto work = [&]() { for (size_t k; (k = next.fetch_add(1)) < nj;) memcpy(stage_jobs[k].dst, stage_jobs[k].src, stage_jobs[k].bytes); };
        std::vector<std::thread> th;
        for (size_t t = 1; t < nt; t++) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
        for (size_t k = 0; k < nj && stage_err == hipSuccess; k++) {
            Item &it = items[stage_jobs[k].image];
            stage_err = hipMemcpyAsync(it.d->base + it.d->off_tables, it.stage, it.tbytes, hipMemcpyHostToDevice, ctx->stream);
            if (stage_err == hipSuccess) stage_err = hipMemcpyAsync(it.d->base + it.d->off_scan, stage_jobs[k].dst, stage_jobs[k].bytes, hipMemcpyHostToDevice, ctx->stream);
        }
        stage_jobs.clear();
    };
    auto pin_slice = [&](size_t bytes) -> uint8_t * {
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes > kPinnedMax) return NULL;
        if (bytes > ctx->pinned_cap) {
            flush_stage_jobs();
            (void)hipStreamSynchronize(ctx->stream);
            if (ctx->pinned) (void)hipHostFree(ctx->pinned);
            ctx->pinned = NULL; ctx->pinned_cap = 0;
            size_t want = bytes * 8 < kPinnedMax ? bytes * 8 : kPinnedMax;      // room for a few images in flight
            if (want < bytes) want = bytes;
            if (hipHostMalloc((void **)&ctx->pinned, want, hipHostMallocDefault) != hipSuccess) { ctx->pinned = NULL; return NULL; }
            ctx->pinned_cap = want;
            pin_off = 0;
        }
        if (pin_off + bytes > ctx->pinned_cap) { flush_stage_jobs(); (void)hipStreamSynchronize(ctx->stream); pin_off = 0; }
        uint8_t *p = ctx->pinned + pin_off;
        pin_off += bytes;
        return p;
    };
    for (int i = 0; i < n && rc == JDA_SUCCESS; i++) {
        Item &it = items[i];
        jda_image *img = imgs[i];
        if (!img) { rc = JDA_INVALID_PARAMETER; break; }
        const jda_image_info &I = *jda_image_get_info(img);
        uint32_t scan_len = 0, nok = 0;
        const uint8_t *scan = jda_image_scan(img, &scan_len);
        const uint8_t *tables = jda_image_tables(img, &it.tbytes);
        it.n_blocks = (size_t)I.mcus_x * I.mcus_y * I.blocks_per_mcu;
        it.on_device = jda_image_index_on_device(img) != 0;      // index to be made on the device
        if (it.on_device && !jda_prescan_admits(scan_len, jda_image_record_cap(img))) { jda_image_run_host_prescan(img); it.on_device = false; }      // (the record area's bound)
        const uint32_t *rpos = jda_image_restart_positions(img, &it.n_int);
        jda_dev_image *d = new (std::nothrow) jda_dev_image;
        if (!d) { rc = JDA_ERROR_MEMORY; break; }
        memset(d, 0, sizeof(*d));
        it.d = d;
        d->info = I;
        d->scan_len = scan_len;
        jda_image_component_ids(img, d->dc_id, d->ac_id, d->q_id);
        { int32_t adobe = 0; jda_image_raw_quant(img, &d->quant_zz[0][0], &adobe); d->adobe = (uint8_t)adobe; d->colour = (uint8_t)jda_image_colour_model(img); }
        d->general_p1 = (uint8_t)jda_image_general_p1(img);
        d->tables_host = (uint8_t *)malloc(JDA_TABLE_BYTES);
        if (d->tables_host) { uint32_t tb_ = 0; memcpy(d->tables_host, jda_image_tables(img, &tb_), JDA_TABLE_BYTES); }
        d->off_tables = 0;
        d->off_index = align16(it.tbytes);
        d->off_dc = d->off_index + align16((it.n_blocks + 1) * sizeof(uint32_t));
        d->off_scan = d->off_dc + align16(it.n_blocks * sizeof(int16_t));
        d->bytes = d->off_scan + align16((size_t)scan_len + JDA_SCAN_PAD);
        d->off_cont_first = d->off_cont = 0; d->n_cont = 0;
        if (!it.on_device) {                                      // the serial pre-scan's continuation entries travel with its index
            const uint32_t *cf = NULL;
            uint32_t nc = 0;
            (void)jda_image_block_cont(img, &cf, &nc);
            if (nc) {
                d->n_cont = nc;
                d->off_cont_first = d->bytes; d->off_cont = d->off_cont_first + align16((it.n_blocks + 1) * sizeof(uint32_t));
                d->bytes = d->off_cont + align16((size_t)nc * sizeof(uint32_t));
            }
        }
        it.alloc = d->bytes;
        it.seg_mode = it.on_device;
        it.n_segs = 0;
        if (it.seg_mode) {
            // the scan is read in whole 256-byte segments (+ a few bytes): zero padded behind its last byte; then the entry
            // states, the per-segment sums and start values, the two work lists, the restart positions, the result words
            it.rec_cap = jda_image_record_cap(img);
            const jda_prescan_sizes Z = jda_prescan_sizes_of(scan_len, I.restart_interval ? it.n_int : 0u, it.rec_cap);
            it.n_segs = Z.n_segs;
            d->bytes = d->off_scan + Z.scan;
            it.off_ea = d->bytes;
            it.off_sum = it.off_ea + Z.entry;
            it.off_start = it.off_sum + Z.seg_sum;
            it.off_wl = it.off_start + Z.seg_start;
            it.off_rp = it.off_wl + Z.worklist;
            it.off_wt = it.off_rp + Z.restart_pos;
            it.off_ev = it.off_wt + JDA_WT_BYTES;                 // RECORD mode: who ended which restart interval (zeroed)
            it.off_sstats = it.off_ev + Z.rst_events;
            it.alloc = it.off_sstats + 512;
            it.zero_end = it.alloc;                          // (what is memset: everything up to here; records and candidates need none)
            it.record = true;                                 // (a stream the device walks has record slots: front_common)
            if (it.record) {
                it.off_recs = (it.alloc + 255) & ~(size_t)255;
                it.off_cands = it.off_recs + Z.records;
                it.cand_cap = Z.cand_cap;
                it.alloc = it.off_cands + Z.cands;
            }
        }
        e = jda_pool_alloc(ctx, (void **)&d->base, it.alloc);
        if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc(image)"); rc = JDA_ERROR_MEMORY; break; }
        if (it.seg_mode) {
            // only the tables and the scan travel; everything behind the scan's last byte starts as zeros (padding, round-0
            // entry states, counters).  The index is written by the WRITE pass.
            const size_t up = align16(it.tbytes) + align16((size_t)scan_len);
            it.stage = pin_slice(up);
            if (!it.stage) { it.heap.assign(up, 0); it.stage = it.heap.data(); }
            memcpy(it.stage, tables, it.tbytes);
            // the scan's copy into the page-locked slice is left to the staging threads (below): job = (dst, src, bytes, image)
            if (it.heap.empty()) { stage_jobs.push_back({ it.stage + align16(it.tbytes), scan, (size_t)scan_len, i }); }
            else {
                memcpy(it.stage + align16(it.tbytes), scan, scan_len);
                e = hipMemcpyAsync(d->base + d->off_tables, it.stage, it.tbytes, hipMemcpyHostToDevice, ctx->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(d->base + d->off_scan, it.stage + align16(it.tbytes), scan_len, hipMemcpyHostToDevice, ctx->stream);
            }
            if (e == hipSuccess) e = hipMemsetAsync(d->base + d->off_scan + scan_len, 0, it.zero_end - (d->off_scan + scan_len), ctx->stream);
            if (e != hipSuccess) { rc = jda_set_err(ctx, e, "hipMemcpy(image)"); break; }
            jda_segscan_params SP;
            memset(&SP, 0, sizeof(SP));
            SP.scan = d->base + d->off_scan; SP.tables = d->base + d->off_tables;
            SP.entry_cur = (uint32_t *)(d->base + it.off_ea); SP.entry_nxt = SP.entry_cur;
            SP.seg_sum = (uint32_t *)(d->base + it.off_sum); SP.seg_start = (const uint32_t *)(d->base + it.off_start);
            SP.worklist = (uint32_t *)(d->base + it.off_wl); SP.worklist_cap = it.n_segs;
            if (I.restart_interval) {                        // the walk ends intervals where the (host) filter found the markers
                it.rp.assign(rpos, rpos + it.n_int); it.rp.push_back(JDA_RST_SENTINEL);
                e = hipMemcpyAsync(d->base + it.off_rp, it.rp.data(), it.rp.size() * 4, hipMemcpyHostToDevice, ctx->stream);
                if (e != hipSuccess) { rc = jda_set_err(ctx, e, "hipMemcpy(restart positions)"); break; }
                SP.restart_pos = (const uint32_t *)(d->base + it.off_rp);
            }
            SP.blk_index = (uint32_t *)(d->base + d->off_index); SP.blk_dc = (int16_t *)(d->base + d->off_dc);
            SP.stats = (uint32_t *)(d->base + it.off_sstats);
            SP.walk_tables = d->base + it.off_wt;
            if (it.record) {
                SP.records = (uint32_t *)(d->base + it.off_recs); SP.rec_cap = it.rec_cap;
                SP.cands = (uint32_t *)(d->base + it.off_cands); SP.cand_cap = it.cand_cap;
                if (I.restart_interval) SP.rst_events = (uint32_t *)(d->base + it.off_ev);
            }
            jda_prescan_fill_geometry(SP, I, d->dc_id, d->ac_id, scan_len, it.n_segs, I.restart_interval ? it.n_int : 0u);
            seg_params.push_back(SP); seg_owner.push_back(i);
            if (it.n_segs > max_segs) max_segs = it.n_segs;
            continue;
        }
        // stage through one host buffer so it is a single H2D copy
        it.stage = pin_slice(it.alloc);
        if (!it.stage) { it.heap.assign(it.alloc, 0); it.stage = it.heap.data(); }
        memcpy(it.stage + d->off_tables, tables, it.tbytes);
        memcpy(it.stage + d->off_scan, scan, (size_t)scan_len + JDA_SCAN_PAD);
        {
            const uint32_t *index = jda_image_block_index(img, &nok);
            memcpy(it.stage + d->off_index, index, (it.n_blocks + 1) * sizeof(uint32_t));
            memcpy(it.stage + d->off_dc, jda_image_block_dc(img), it.n_blocks * sizeof(int16_t));
            if (d->n_cont) {
                const uint32_t *cf = NULL;
                const uint32_t *ce = jda_image_block_cont(img, &cf, NULL);
                memcpy(it.stage + d->off_cont_first, cf, (it.n_blocks + 1) * sizeof(uint32_t));
                memcpy(it.stage + d->off_cont, ce, (size_t)d->n_cont * sizeof(uint32_t));
            }
            {   // the scan slice of every tile, as jda_tile_setup_from computes it: how many exceed the 16-wave kernel's window
                const int mode = jda_mode_of(I);
                const uint32_t per = jda_mcus_per_tile(mode), win = jda_window_bytes(mode, 0), nb = (uint32_t)I.blocks_per_mcu;
                uint32_t total = 0, over = 0;
                for (uint32_t y = 0; y < (uint32_t)I.mcus_y; y++)
                    for (uint32_t x = 0; x < (uint32_t)I.mcus_x; x += per) {
                        const uint32_t cnt = (uint32_t)I.mcus_x - x < per ? (uint32_t)I.mcus_x - x : per;
                        const size_t b0 = ((size_t)y * I.mcus_x + x) * nb, b1 = b0 + (size_t)cnt * nb;
                        const uint32_t lo = (index[b0] >> JDA_INDEX_OFF_BITS) & ~15u, hi = ((index[b1] >> JDA_INDEX_OFF_BITS) + 8u + 12u + 15u) & ~15u;
                        total++;
                        if (hi - lo > win) over++;
                    }
                d->tiles_total = total; d->tiles_over_small = over;
            }
        }
        e = hipMemcpyAsync(d->base, it.stage, it.alloc, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { rc = jda_set_err(ctx, e, "hipMemcpy(image)"); break; }
    }
    flush_stage_jobs();
    if (rc == JDA_SUCCESS && stage_err != hipSuccess) rc = jda_set_err(ctx, stage_err, "hipMemcpy(image)");
    if (rc != JDA_SUCCESS) { (void)hipStreamSynchronize(ctx->stream); return fail_all(rc); }
    JDA_UP_MARK("alloc + stage + H2D");

    // ---- the index on the device (with or without restart intervals): round 0 and round 1 over every segment, two rounds over the
    // work lists, every further round in one launch, sums, WRITE -- the passes of jda_pipeline, on this context's stream
    jda_segscan_params *d_seg = NULL;
    if (!seg_params.empty() && e == hipSuccess) {
        const uint32_t ns = (uint32_t)seg_params.size();
        e = jda_pool_alloc(ctx, (void **)&d_seg, seg_params.size() * sizeof(jda_segscan_params));
        if (e == hipSuccess) e = hipMemcpyAsync(d_seg, seg_params.data(), seg_params.size() * sizeof(jda_segscan_params), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = jda_launch_walk_tables(d_seg, ns, ctx->stream);
        // round 0, the recording round, two work-list rounds, every further round in one launch, the sums (first block ordinal, DC
        // predictors, window lag per segment), then finalize + candidates (records -> index entries and DC values)
        // A batch that cannot fill the GPU -- one image at a time is the case -- is as slow as its rounds are long, and a round is one
        // wavefront's chain of walk steps: the entry states are settled with the SPEC walk (half a RECORD walk's instructions) and every
        // segment is recorded once, from its settled state (one 4096x4096 image: 0.07 + 3 x 0.15 ms of rounds -> 4 x 0.07 + 0.15).  A batch
        // that does fill it pays per walk, not per round: there the RECORD round right behind round 0 is the cheaper order.
        uint64_t total_segs = 0;
        for (const jda_segscan_params &sp : seg_params) total_segs += sp.n_segs;
        const int states_first = total_segs <= 131072u ? 1 : 0;                 // (two lanes for every SIMD lane of the GPU)
        if (e == hipSuccess) e = jda_launch_prescan_passes_ex(d_seg, ns, max_segs, JDA_PRESCAN_LIST_ROUNDS, JDA_PRESCAN_MAX_ROUND, 1, states_first, ctx->stream);
        for (uint32_t p = 0; p < ns && e == hipSuccess; p++) {
            Item &it = items[seg_owner[p]];
            e = hipMemcpyAsync(it.sst, it.d->base + it.off_sstats, sizeof(it.sst), hipMemcpyDeviceToHost, ctx->stream);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    JDA_UP_MARK("write pass + D2H");
    if (d_seg) jda_pool_free(ctx, d_seg);
    if (e != hipSuccess) return fail_all(jda_set_err(ctx, e, "jda_upload_batch"));

    // a marker that is not where the MCU count puts it, a corrupt or truncated stream, states that did not settle: the serial host
    // pre-scan reproduces what the reference does with such a stream
    bool reupload = false;
    int rounds_max = 0;
    for (size_t p = 0; p < seg_owner.size() && e == hipSuccess; p++) {
        const int i = seg_owner[p];
        Item &it = items[i];
        const jda_image_info &I = *jda_image_get_info(imgs[i]);
        rounds_max = std::max(rounds_max, jda_prescan_rounds_used(it.sst));
        if (jda_prescan_verdict(it.sst, NULL, 0)) {                      // (the host filter placed the markers)
            jda_image_adopt_prescan(imgs[i], (uint32_t)(I.mcus_x * I.mcus_y), it.sst[JDA_ST_MAX_AC], (int32_t)it.sst[JDA_ST_MAX_DC], it.sst[JDA_ST_TRUNC]);
            it.d->prescan_on_device = 1;
        } else {                                                         // corrupt or truncated stream: the serial pre-scan knows what the reference does
            jda_image_run_host_prescan(imgs[i]);
            uint32_t nok = 0;
            const uint32_t *index = jda_image_block_index(imgs[i], &nok);
            e = hipMemcpyAsync(it.d->base + it.d->off_index, index, (it.n_blocks + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(it.d->base + it.d->off_dc, jda_image_block_dc(imgs[i]), it.n_blocks * sizeof(int16_t), hipMemcpyHostToDevice, ctx->stream);
            reupload = true;
        }
    }
    if (!seg_owner.empty()) ctx->last_segscan_rounds = rounds_max;           // rounds that had something to walk
    if (reupload && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail_all(jda_set_err(ctx, e, "jda_upload_batch(re-upload)"));
    for (int i = 0; i < n; i++) {
        uint32_t nok = 0;
        (void)jda_image_block_index(imgs[i], &nok);
        items[i].d->n_mcus_ok = nok;
        items[i].d->fast_mul = (uint8_t)jda_image_fast_mul(imgs[i]);
        out[i] = items[i].d;
    }
    return JDA_SUCCESS;
}

// The same, tolerant of holes: imgs[i] == NULL (a file jda_prepare_batch rejected) gets out[i] = NULL and
// status[i] = JDA_INVALID_PARAMETER, everybody else is uploaded -- a bad image does not cost the batch its place in the arrays.
int jda_upload_batch_ex(jda_ctx *ctx, int32_t n, jda_image *const *imgs, jda_dev_image **out, int32_t *status)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n <= 0 || !imgs || !out) return JDA_INVALID_PARAMETER;
    std::vector<jda_image *> v;
    std::vector<int> ix;
    for (int i = 0; i < n; i++) {
        out[i] = NULL;
        if (status) status[i] = imgs[i] ? JDA_SUCCESS : JDA_INVALID_PARAMETER;
        if (imgs[i]) { v.push_back(imgs[i]); ix.push_back(i); }
    }
    if (v.empty()) return JDA_SUCCESS;
    std::vector<jda_dev_image *> o(v.size(), NULL);
    const int rc = jda_upload_batch(ctx, (int32_t)v.size(), v.data(), o.data());
    for (size_t k = 0; k < v.size(); k++) { out[ix[k]] = o[k]; if (status && rc != JDA_SUCCESS) status[ix[k]] = rc; }
    return rc;
}

jda_dev_image *jda_upload(jda_ctx *ctx, jda_image *img, int32_t *err)
{
    int32_t dummy;
    if (!err) err = &dummy;
    if (!ctx || !img) { *err = ctx ? JDA_INVALID_PARAMETER : JDA_ERROR_NO_DEVICE; return NULL; }
    jda_dev_image *d = NULL;
    *err = jda_upload_batch(ctx, 1, &img, &d);
    return d;
}

int jda_dev_image_prescan_on_device(const jda_dev_image *dimg) { return dimg ? dimg->prescan_on_device : 0; }
int jda_last_prescan_rounds(const jda_ctx *ctx) { return ctx ? ctx->last_segscan_rounds : 0; }
uint32_t jda_dev_image_mcus_ok(const jda_dev_image *dimg) { return dimg ? dimg->n_mcus_ok : 0; }

int jda_filter_on_device(jda_ctx *ctx, const uint8_t *raw, int32_t len, uint8_t *out, int32_t *out_len,
                         uint32_t *restart_pos, int32_t restart_cap, int32_t *n_restarts)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!raw || len < 0 || !out || !out_len) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    const size_t raw_cap = align16((size_t)len) + 16, rcap = restart_cap > 0 ? (size_t)restart_cap : 1;
    const size_t off_out = raw_cap, off_rpos = off_out + align16((size_t)len + 16), off_res = off_rpos + align16(rcap * 4), off_work = off_res + 16;
    const size_t off_par = off_work + align16(JDA_FILTER_WORK_BYTES(len));
    uint8_t *d = NULL;
    hipError_t e = hipMalloc((void **)&d, off_par + sizeof(jda_filter_params));
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(filter)");
    jda_filter_params P;
    P.raw = d; P.out = d + off_out; P.restart_pos = (uint32_t *)(d + off_rpos); P.result = (uint32_t *)(d + off_res);
    P.raw_len = (uint32_t)len; P.restart_cap = (uint32_t)rcap; P.work = (uint32_t *)(d + off_work); P.raw_skip = 0; P.pad_ = 0;
    e = hipMemsetAsync(d, 0, off_par, ctx->stream);
    if (e == hipSuccess && len) e = hipMemcpyAsync(d, raw, (size_t)len, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + off_par, &P, sizeof(P), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = jda_launch_filter((const jda_filter_params *)(d + off_par), 1, (uint32_t)len, ctx->stream);
    uint32_t res[2] = { 0, 0 };
    if (e == hipSuccess) e = hipMemcpyAsync(res, d + off_res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && res[0]) e = hipMemcpy(out, d + off_out, res[0], hipMemcpyDeviceToHost);
    if (e == hipSuccess && restart_pos && restart_cap > 0)
        e = hipMemcpy(restart_pos, d + off_rpos, (size_t)std::min<uint32_t>(res[1] + 1, (uint32_t)restart_cap) * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return jda_set_err(ctx, e, "jda_filter_on_device");
    *out_len = (int32_t)res[0];
    if (n_restarts) *n_restarts = (int32_t)res[1];
    return JDA_SUCCESS;
}
int jda_dev_image_read_index(jda_ctx *ctx, const jda_dev_image *dimg, uint32_t *index, int16_t *dc)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!dimg) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    const size_t nb = (size_t)dimg->info.mcus_x * dimg->info.mcus_y * dimg->info.blocks_per_mcu;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess && index) e = hipMemcpy(index, dimg->base + dimg->off_index, (nb + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && dc) e = hipMemcpy(dc, dimg->base + dimg->off_dc, nb * sizeof(int16_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_dev_image_read_index");
}

void jda_dev_image_free(jda_ctx *ctx, jda_dev_image *dimg)
{
    if (!dimg) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    if (dimg->base) { if (ctx) jda_pool_free(ctx, dimg->base); else (void)hipFree(dimg->base); }
    free(dimg->tables_host);
    delete dimg;
}

size_t jda_dev_image_bytes(const jda_dev_image *dimg) { return dimg ? dimg->bytes : 0; }

jda_batch *jda_batch_create(jda_ctx *ctx, int32_t n, jda_dev_image *const *images,
                            const jda_output *outputs, const int32_t *pixel_types,
                            const int32_t *options, int32_t *err)
{
    return jda_batch_create_rect(ctx, n, images, outputs, pixel_types, options, NULL, err);
}

jda_batch *jda_batch_create_rect(jda_ctx *ctx, int32_t n, jda_dev_image *const *images,
                                 const jda_output *outputs, const int32_t *pixel_types,
                                 const int32_t *options, const int32_t *mcu_rects, int32_t *err)
{
    return jda_batch_create_strips(ctx, n, images, outputs, pixel_types, options, mcu_rects, NULL, err);
}

// strip_mcus[i] != 0: image i's surface is strip-major (jda_dev_desc::strip_mcus; outputs[i] then describes the surface's extent only:
// pitch_bytes x rows >= the strips' bytes)
jda_batch *jda_batch_create_strips(jda_ctx *ctx, int32_t n, jda_dev_image *const *images, const jda_output *outputs, const int32_t *pixel_types,
                                   const int32_t *options, const int32_t *mcu_rects, const int32_t *strip_mcus, int32_t *err)
{
    int32_t dummy;
    if (!err) err = &dummy;
    if (!ctx) { *err = JDA_ERROR_NO_DEVICE; return NULL; }
    if (n <= 0 || !images || !outputs) { *err = JDA_INVALID_PARAMETER; return NULL; }
    std::vector<jda_dev_desc> descs((size_t)n);
    std::vector<jda_strip> strips[JDA_N_LISTS];
    std::vector<int32_t> image_status;
    jda_batch_stats st;
    memset(&st, 0, sizeof(st));
    uint32_t flat_max_items = 0;
    // consecutive images of a list with equal tables and table ids use ONE copy of them (the first one's: it is part of this plan) and are
    // one table generation to the decode kernel -- its workgroups pass from one to the next without restaging (jda_strip::ord)
    int list_owner[JDA_N_LISTS];
    uint32_t list_images[JDA_N_LISTS];
    for (int m = 0; m < JDA_N_LISTS; m++) { list_owner[m] = -1; list_images[m] = 0; }
    for (int i = 0; i < n; i++) {
        const jda_dev_image *im = images[i];
        jda_dev_desc &D = descs[(size_t)i];
        if (!im) { memset(&D, 0, sizeof(D)); image_status.push_back(JDA_INVALID_PARAMETER); continue; }   // a hole (rejected file): nothing is launched for it
        const jda_image_info &I = im->info;
        image_status.push_back(im->n_mcus_ok < (uint32_t)(I.mcus_x * I.mcus_y) ? JDA_DECODE_ERROR : JDA_SUCCESS);   // jpeg.inl:5354-5356
        int bpp = 0;
        const int rc = jda_fill_launch_desc(D, I, im->dc_id, im->ac_id, im->q_id, im->fast_mul, im->general_p1, im->n_mcus_ok, im->scan_len,
                                            outputs[i], pixel_types ? pixel_types[i] : JDA_RGB8888, options ? options[i] : 0, &bpp);
        if (rc != JDA_SUCCESS) { *err = rc; return NULL; }
        D.tables = im->base + im->off_tables;
        D.blk_index = (const uint32_t *)(im->base + im->off_index);
        D.blk_dc = (const int16_t *)(im->base + im->off_dc);
        D.scan = im->base + im->off_scan;
        D.strip_mcus = (strip_mcus && strip_mcus[i] > 0) ? (uint32_t)strip_mcus[i] : 0u;
        // kernel variant 1: the plain case -- full size, RGB8888, every block decoded -- runs a kernel in which these
        // descriptor fields are compile-time constants (jda_desc_uniform<1>)
        const int variant = jda_plain_variant(D);
        const int big = D.scale_shift == 3 ? 0 : jda_big_window(D, variant, im->tiles_total, im->tiles_over_small);
        const int cont = jda_use_cont(D, variant, im->n_cont);
        if (cont) { D.blk_cont_first = (const uint32_t *)(im->base + im->off_cont_first); D.blk_cont = (const uint32_t *)(im->base + im->off_cont); }
        {
            const int li = jda_list_index(D, variant, big, cont, mcu_rects == NULL);
            std::vector<jda_strip> &lst = strips[li];
            list_images[li]++;
            bool same_tables = false;
            if (list_owner[li] >= 0) {
                const jda_dev_image *om = images[list_owner[li]];
                same_tables = om->tables_host && im->tables_host && !memcmp(om->dc_id, im->dc_id, 3) && !memcmp(om->ac_id, im->ac_id, 3) && !memcmp(om->q_id, im->q_id, 3) &&
                              om->info.ncomp == im->info.ncomp && !memcmp(om->tables_host, im->tables_host, JDA_TABLE_BYTES);
            }
            if (same_tables) D.tables = descs[(size_t)list_owner[li]].tables; else list_owner[li] = i;
            const uint32_t per = jda_mcus_per_tile(D.mode);
            if (JDA_LIST_IS_THUMB_FLAT(li)) {                     // a whole gray image at 1/8: one record (jda_dc_thumbnail_flat)
                jda_strip r;
                memset(&r, 0, sizeof(r));
                r.image = (uint32_t)i; r.count = 1; r.first = 1; r.ord = lst.empty() ? 0u : lst.back().ord + (same_tables ? 0u : 1u);
                lst.push_back(r);
                flat_max_items = std::max(flat_max_items, jda_flat_items(D));
                st.tiles += (int64_t)D.mcus_y * ((D.mcus_x + per - 1) / per);
            } else {
                const size_t before = lst.size();
                jda_append_strips(lst, (uint32_t)i, D.mcus_x, D.mcus_y, D.mode, big, mcu_rects ? mcu_rects + 4 * i : NULL, D.strip_mcus, same_tables);
                for (size_t k = before; k < lst.size(); k++) if (lst[k].count) st.tiles++;
            }
            st.tiles_whole_images += (int64_t)D.mcus_y * ((D.mcus_x + per - 1) / per);
        }
        st.source_pixels += (int64_t)I.width * I.height;
        st.output_bytes += (int64_t)D.out_w * D.out_rows * bpp;
        st.scan_bytes += im->scan_len;
        st.index_bytes += (int64_t)I.mcus_x * I.mcus_y * I.blocks_per_mcu * 6;
        st.table_bytes += JDA_TABLE_BYTES;
    }
    jda_batch *b = new (std::nothrow) jda_batch;
    if (!b) { *err = JDA_ERROR_MEMORY; return NULL; }
    memset(b, 0, sizeof(*b));
    b->n_images = n;
    b->flat_max_items = flat_max_items;
    b->status = new (std::nothrow) int32_t[(size_t)n];
    if (b->status) memcpy(b->status, image_status.data(), (size_t)n * sizeof(int32_t));
    (void)hipSetDevice(ctx->device);
    hipError_t e = jda_pool_alloc(ctx, (void **)&b->d_descs, descs.size() * sizeof(jda_dev_desc));
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_descs, descs.data(), descs.size() * sizeof(jda_dev_desc), hipMemcpyHostToDevice, ctx->stream);
    for (int m = 0; m < JDA_N_LISTS && e == hipSuccess; m++) {
        b->n_strips[m] = (uint32_t)strips[m].size();
        if (!b->n_strips[m]) continue;
        if (!JDA_LIST_IS_THUMB_FLAT(m))
            b->pool_ok[m] = strips[m].front().ord == strips[m].back().ord &&
                            strips[m].size() / jda_tiles_per_wg(JDA_LIST_MODE(m), JDA_LIST_BIG(m)) >= (size_t)JDA_POOL_MIN_QUADS_PER_IMAGE * list_images[m];
        e = jda_pool_alloc(ctx, (void **)&b->d_strips[m], strips[m].size() * sizeof(jda_strip));
        if (e == hipSuccess) e = hipMemcpyAsync(b->d_strips[m], strips[m].data(), strips[m].size() * sizeof(jda_strip), hipMemcpyHostToDevice, ctx->stream);
        st.n_launches++;
        st.n_workgroups += JDA_LIST_IS_THUMB_FLAT(m) ? (int32_t)strips[m].size() : (int32_t)(strips[m].size() / jda_tiles_per_wg(JDA_LIST_MODE(m), JDA_LIST_BIG(m)));
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        jda_set_err(ctx, e, "jda_batch_create");
        jda_batch_destroy(ctx, b);
        *err = JDA_ERROR_HIP;
        return NULL;
    }
    b->stats = st;
    *err = JDA_SUCCESS;
    return b;
}

void jda_batch_destroy(jda_ctx *ctx, jda_batch *b)
{
    if (!b) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    if (b->d_descs) { if (ctx) jda_pool_free(ctx, b->d_descs); else (void)hipFree(b->d_descs); }
    for (int m = 0; m < JDA_N_LISTS; m++) if (b->d_strips[m]) { if (ctx) jda_pool_free(ctx, b->d_strips[m]); else (void)hipFree(b->d_strips[m]); }
    delete[] b->status;
    delete b;
}

int jda_batch_decode(jda_ctx *ctx, jda_batch *b)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!b) return JDA_INVALID_PARAMETER;
    for (int m = 0; m < JDA_N_LISTS; m++) {
        if (!b->n_strips[m]) continue;
        JDA_HIP(ctx, jda_launch_decode(JDA_LIST_MODE(m), JDA_LIST_FAST(m), JDA_LIST_VARIANT(m), JDA_LIST_BIG(m), JDA_LIST_CONT(m), b->d_descs, b->d_strips[m], b->n_strips[m],
                                       JDA_LIST_IS_THUMB_FLAT(m) ? b->flat_max_items : 0u, b->pool_ok[m], ctx->stream));
    }
    return JDA_SUCCESS;
}

// status[i] of every image of the plan: JDA_SUCCESS, JDA_DECODE_ERROR (the stream has a bad MCU: the MCUs before it are decoded,
// as the reference leaves them, jpeg.inl:5354-5356) or JDA_INVALID_PARAMETER (a hole in the image array)
int jda_batch_get_status(const jda_batch *b, int32_t *status)
{
    if (!b || !status || !b->status) return JDA_INVALID_PARAMETER;
    memcpy(status, b->status, (size_t)b->n_images * sizeof(int32_t));
    return JDA_SUCCESS;
}

int jda_batch_get_stats(const jda_batch *b, jda_batch_stats *stats)
{
    if (!b || !stats) return JDA_INVALID_PARAMETER;
    *stats = b->stats;
    return JDA_SUCCESS;
}

// checksums[i] of n surfaces (device pointers): see jda_surface_checksum in jda_kernels.hip.  Synchronous.
int jda_checksum_surfaces(jda_ctx *ctx, int32_t n, const jda_output *surfaces, const int32_t *row_bytes, uint64_t *checksums)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n <= 0 || !surfaces || !row_bytes || !checksums) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    unsigned long long *d = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&d, (size_t)n * 8);
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(checksums)");
    e = hipMemsetAsync(d, 0, (size_t)n * 8, ctx->stream);
    for (int i = 0; i < n && e == hipSuccess; i++) {
        if (!surfaces[i].pixels || surfaces[i].pitch_bytes < row_bytes[i] || row_bytes[i] < 0 || surfaces[i].rows < 0) { jda_pool_free(ctx, d); return JDA_INVALID_PARAMETER; }
        e = jda_launch_checksum(surfaces[i].pixels, (uint32_t)surfaces[i].pitch_bytes, (uint32_t)row_bytes[i], (uint32_t)surfaces[i].rows, d + i, ctx->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(checksums, d, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    jda_pool_free(ctx, d);
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_checksum_surfaces");
}

// "0000:8e:00.0" of the context's GPU (for NUMA placement of the host threads that feed it); buf >= 16 bytes
int jda_device_pci_bus_id_of(int32_t device, char *buf, int32_t len)
{
    if (!buf || len < 16) return JDA_INVALID_PARAMETER;
    return hipDeviceGetPCIBusId(buf, len, device) == hipSuccess ? JDA_SUCCESS : JDA_ERROR_HIP;
}
int jda_device_pci_bus_id(jda_ctx *ctx, char *buf, int32_t len)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!buf || len < 16) return JDA_INVALID_PARAMETER;
    return hipDeviceGetPCIBusId(buf, len, ctx->device) == hipSuccess ? JDA_SUCCESS : JDA_ERROR_HIP;
}

int jda_sync(jda_ctx *ctx)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    JDA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JDA_SUCCESS;
}

int jda_timer_start(jda_ctx *ctx)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    JDA_HIP(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    return JDA_SUCCESS;
}

int jda_timer_stop(jda_ctx *ctx)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    JDA_HIP(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    return JDA_SUCCESS;
}

double jda_timer_elapsed_ms(jda_ctx *ctx)
{
    if (!ctx) return -1.0;
    if (hipEventSynchronize(ctx->ev_stop) != hipSuccess) return -1.0;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop) != hipSuccess) return -1.0;
    return (double)ms;
}

int jda_decode_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type,
                       int32_t options, void *host_pixels, int32_t pitch_bytes, int32_t rows)
{
    return jda_decode_to_host_ex(ctx, jpeg, len, pixel_type, options, host_pixels, pitch_bytes, rows, NULL);
}

int jda_decode_to_host_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type,
                          int32_t options, void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded)
{
    return jda_decode_to_host_rect(ctx, jpeg, len, pixel_type, options, NULL, host_pixels, pitch_bytes, rows, mcus_decoded, NULL);
}

int jda_decode_to_host_rect(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *mcu_rect,
                            void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded, int32_t *tiles)
{
    return jda_decode_to_host_flags(ctx, jpeg, len, pixel_type, options, mcu_rect, host_pixels, pitch_bytes, rows, mcus_decoded, tiles, 0);
}

// ---- coefficient images (jda_coef_tiles / jda_sparse_tiles in jda_kernels.hip)
jda_dev_coef *jda_coef_upload(jda_ctx *ctx, const jda_coef_image *img, int32_t *err)
{
    if (!ctx) { if (err) *err = JDA_ERROR_NO_DEVICE; return NULL; }      // (this call's order of checks, as ever)
    return jda_coef_upload_ex(ctx, img, JDA_COEF_DENSE, err);
}

// which form an upload of `form` makes resident, and its bytes behind the quantisers (JDA_COEF_AUTO: the smaller one for THIS image)
int jda_coef_pick_form(const jda_coef_image *img, int32_t form, int *picked, size_t *payload_bytes)
{
    if (!img || form < JDA_COEF_DENSE || form > JDA_COEF_AUTO) return JDA_INVALID_PARAMETER;
    uint32_t n_blocks = 0;
    (void)jda_coef_image_coefficients(img, &n_blocks);
    const size_t dense = align16((size_t)n_blocks * JDA_CT_BLOCK_BYTES);
    if (form == JDA_COEF_DENSE) { *picked = JDA_COEF_DENSE; *payload_bytes = dense; return JDA_SUCCESS; }
    const int st = jda_coef_image_sparse_status(img);
    if (st != JDA_SUCCESS) {
        if (form == JDA_COEF_AUTO && st == JDA_UNSUPPORTED_FEATURE) { *picked = JDA_COEF_DENSE; *payload_bytes = dense; return JDA_SUCCESS; }
        return st;
    }
    const size_t sparse = jda_coef_image_sparse_bytes(img);
    if (form == JDA_COEF_AUTO && sparse >= dense) { *picked = JDA_COEF_DENSE; *payload_bytes = dense; return JDA_SUCCESS; }
    *picked = JDA_COEF_SPARSE; *payload_bytes = sparse;
    return JDA_SUCCESS;
}

jda_dev_coef *jda_coef_upload_ex(jda_ctx *ctx, const jda_coef_image *img, int32_t form, int32_t *err)
{
    int32_t dummy;
    if (!err) err = &dummy;
    if (!img || form < JDA_COEF_DENSE || form > JDA_COEF_AUTO) { *err = JDA_INVALID_PARAMETER; return NULL; }      // (checked on the host, whatever the context)
    if (!ctx) { *err = JDA_ERROR_NO_DEVICE; return NULL; }
    (void)hipSetDevice(ctx->device);
    int picked = JDA_COEF_DENSE;
    size_t payload = 0;
    const int rc = jda_coef_pick_form(img, form, &picked, &payload);
    if (rc != JDA_SUCCESS) { *err = rc; return NULL; }
    jda_dev_coef *d = new (std::nothrow) jda_dev_coef;
    if (!d) { *err = JDA_ERROR_MEMORY; return NULL; }
    memset(d, 0, sizeof(*d));
    d->info = *jda_coef_image_get_info(img);
    const int16_t *coefs = jda_coef_image_coefficients(img, &d->n_blocks);
    const int16_t *quant = jda_coef_image_quant(img, d->q_id);
    { int32_t adobe = 0; jda_coef_image_raw_quant(img, &d->raw_quant[0][0], d->raw_qid, &adobe); d->adobe = (uint8_t)adobe; d->colour = (uint8_t)jda_coef_image_colour_model(img); }
    d->form = picked;
    d->bytes = JDA_CT_QUANT_BYTES + payload;
    hipError_t e = jda_pool_alloc(ctx, (void **)&d->base, d->bytes);
    if (e != hipSuccess) { delete d; jda_set_err(ctx, e, "hipMalloc(coefficient image)"); *err = JDA_ERROR_MEMORY; return NULL; }
    e = hipMemcpyAsync(d->base, quant, JDA_CT_QUANT_BYTES, hipMemcpyHostToDevice, ctx->stream);
    if (picked == JDA_COEF_DENSE) {
        d->off_entries = JDA_CT_QUANT_BYTES;
        if (e == hipSuccess && d->n_blocks) e = hipMemcpyAsync(d->base + JDA_CT_QUANT_BYTES, coefs, (size_t)d->n_blocks * JDA_CT_BLOCK_BYTES, hipMemcpyHostToDevice, ctx->stream);
    } else {                                               // quantisers | first[] | entries[], each part 16-byte aligned (the host arrays are padded alike)
        const uint32_t *first = NULL;
        const uint32_t *entries = jda_coef_image_sparse(img, &first, &d->n_entries);
        const size_t first_bytes = align16(((size_t)d->n_blocks + 1) * 4), entry_bytes = align16((size_t)d->n_entries * 4);
        d->off_entries = JDA_CT_QUANT_BYTES + first_bytes;
        if (e == hipSuccess) e = hipMemcpyAsync(d->base + JDA_CT_QUANT_BYTES, first, first_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && entry_bytes) e = hipMemcpyAsync(d->base + d->off_entries, entries, entry_bytes, hipMemcpyHostToDevice, ctx->stream);
    }
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }      // (the image's host memory is the caller's again)
    if (e != hipSuccess) { jda_pool_free(ctx, d->base); delete d; jda_set_err(ctx, e, "jda_coef_upload"); *err = JDA_ERROR_HIP; return NULL; }
    if (const jda_coef_image *k = jda_coef_image_component3(img)) {      // (a four-component image: component 3 beside it, dense)
        d->k = jda_coef_upload_ex(ctx, k, JDA_COEF_DENSE, err);
        if (!d->k) { jda_pool_free(ctx, d->base); delete d; return NULL; }
    }
    *err = JDA_SUCCESS;
    return d;
}

int jda_dev_coef_form(const jda_dev_coef *d) { return d ? d->form : JDA_COEF_DENSE; }
size_t jda_dev_coef_bytes(const jda_dev_coef *d) { return d ? d->bytes + (d->k ? d->k->bytes : 0) : 0; }

void jda_dev_coef_free(jda_ctx *ctx, jda_dev_coef *d)
{
    if (!d) return;
    if (d->k) jda_dev_coef_free(ctx, d->k);
    if (d->base) { if (ctx) { (void)hipSetDevice(ctx->device); jda_pool_free(ctx, d->base); } else (void)hipFree(d->base); }
    delete d;
}

// descriptors and tile lists of n coefficient images -> one host blob (descs | the lists of the two forms x five layouts); host work only.
// per_image_err != NULL: imgs[i] == NULL is a hole, and an image that cannot be planned gets its code there and is left out, nothing launched
// for either.  mcu_rects: as jda_batch_create_rect (jda_append_strips).
int jda_coef_plan_build(int32_t n, const jda_dev_coef *const *imgs, const jda_output *outputs, const int32_t *pixel_types, const int32_t *options,
                        const int32_t *mcu_rects, int32_t *per_image_err, jda_coef_plan *plan)
{
    plan->blob.clear(); plan->n_launches = 0;
    memset(plan->off, 0, sizeof(plan->off)); memset(plan->n_tiles, 0, sizeof(plan->n_tiles));
    std::vector<jda_dev_desc> descs((size_t)n);
    std::vector<jda_strip> strips[2][JDA_N_MODES];
    for (int i = 0; i < n; i++) {
        const jda_dev_coef *im = imgs[i];
        jda_dev_desc &D = descs[(size_t)i];
        if (per_image_err) per_image_err[i] = JDA_SUCCESS;
        if (!im) { if (!per_image_err) return JDA_INVALID_PARAMETER; memset(&D, 0, sizeof(D)); continue; }
        jda_image_info I = im->info;
        I.jpeg_type = 0;                                   // (coefficients of every scan: geometry and rules of a baseline file of this SOF)
        const int opt = (options ? options[i] : 0) & ~JDA_PROGRESSIVE_FULL;
        const uint8_t no_huff[3] = { 0, 0, 0 };
        int rc = (opt & (JDA_SCALE_HALF | JDA_SCALE_QUARTER | JDA_SCALE_EIGHTH)) ? JDA_UNSUPPORTED_FEATURE : JDA_SUCCESS;      // full size only
        if (I.ncomp != 1 && I.ncomp != 3) rc = JDA_UNSUPPORTED_FEATURE;       // (a four-component image of jda_coef_prepare: the exact decode's _ex calls alone take it)
        if (rc == JDA_SUCCESS) rc = jda_fill_launch_desc(D, I, no_huff, no_huff, im->q_id, 0, 0, (uint32_t)(I.mcus_x * I.mcus_y), 0, outputs[i],
                                                         pixel_types ? pixel_types[i] : JDA_RGB8888, opt, NULL);
        if (rc != JDA_SUCCESS) {
            if (!per_image_err) return rc;
            per_image_err[i] = rc; memset(&D, 0, sizeof(D)); continue;
        }
        D.pad_[0] = 0;
        D.tables = im->base;
        D.scan = im->base + im->off_entries;
        jda_append_strips(strips[im->form == JDA_COEF_SPARSE ? 1 : 0][D.mode], (uint32_t)i, D.mcus_x, D.mcus_y, D.mode, 0, mcu_rects ? mcu_rects + 4 * i : NULL);
    }
    size_t bytes = align16(descs.size() * sizeof(jda_dev_desc));
    for (int f = 0; f < 2; f++)
        for (int m = 0; m < JDA_N_MODES; m++) {
            plan->off[f][m] = bytes; plan->n_tiles[f][m] = (uint32_t)strips[f][m].size();
            bytes += align16(strips[f][m].size() * sizeof(jda_strip));
            if (plan->n_tiles[f][m]) plan->n_launches++;
        }
    plan->blob.assign(bytes, 0);
    memcpy(plan->blob.data(), descs.data(), descs.size() * sizeof(jda_dev_desc));
    for (int f = 0; f < 2; f++)
        for (int m = 0; m < JDA_N_MODES; m++)
            if (!strips[f][m].empty()) memcpy(plan->blob.data() + plan->off[f][m], strips[f][m].data(), strips[f][m].size() * sizeof(jda_strip));
    return JDA_SUCCESS;
}

// the blob's copy into `block` (device, blob.size() bytes) and the launches, one per (form, layout) present, queued on `stream`; the blob is
// read until the copy is done
hipError_t jda_coef_plan_launch(const jda_coef_plan &plan, uint8_t *block, hipStream_t stream)
{
    const hipError_t e = hipMemcpyAsync(block, plan.blob.data(), plan.blob.size(), hipMemcpyHostToDevice, stream);
    return e == hipSuccess ? jda_coef_plan_launch_kernels(plan, block, stream) : e;
}
hipError_t jda_coef_plan_launch_kernels(const jda_coef_plan &plan, const uint8_t *block, hipStream_t stream)
{
    hipError_t e = hipSuccess;
    for (int m = 0; m < JDA_N_MODES && e == hipSuccess; m++)
        if (plan.n_tiles[0][m]) e = jda_launch_coef_tiles(m, (const jda_dev_desc *)block, (const jda_strip *)(block + plan.off[0][m]), plan.n_tiles[0][m], stream);
    for (int m = 0; m < JDA_N_MODES && e == hipSuccess; m++)
        if (plan.n_tiles[1][m]) e = jda_launch_sparse_tiles(m, (const jda_dev_desc *)block, (const jda_strip *)(block + plan.off[1][m]), plan.n_tiles[1][m], stream);
    return e;
}

int jda_coef_decode_surfaces_rect(jda_ctx *ctx, int32_t n, const jda_dev_coef *const *imgs, const jda_output *outputs, const int32_t *pixel_types,
                                  const int32_t *options, const int32_t *mcu_rects)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!imgs || !outputs) return JDA_INVALID_PARAMETER;
    jda_coef_plan plan;
    int rc = jda_coef_plan_build(n, imgs, outputs, pixel_types, options, mcu_rects, NULL, &plan);
    if (rc != JDA_SUCCESS) return rc;
    (void)hipSetDevice(ctx->device);
    uint8_t *blk = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, plan.blob.size());
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(coefficient plan)");
    e = jda_coef_plan_launch(plan, blk, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);     // (the blob leaves pageable memory that goes away with this frame)
    jda_pool_free(ctx, blk);
    if (e != hipSuccess) return jda_set_err(ctx, e, "jda_coef_tiles");
    return es == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, es, "jda_coef_decode_surfaces");
}

int jda_coef_decode_surfaces(jda_ctx *ctx, int32_t n, const jda_dev_coef *const *imgs, const jda_output *outputs, const int32_t *pixel_types,
                             const int32_t *options)
{
    return jda_coef_decode_surfaces_rect(ctx, n, imgs, outputs, pixel_types, options, NULL);
}

// jda_decode_to_host* with JDA_PROGRESSIVE_FULL on a progressive file: every scan on the host, the coefficients to the GPU, the canvas back
static int progressive_full_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options,
                                    void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded)
{
    if (!jpeg || !host_pixels) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    int32_t err = JDA_SUCCESS;
    jda_coef_image *img = jda_progressive_prepare(jpeg, len, &err);
    if (!img) return err;                                 // JDA_DECODE_ERROR: nothing decoded, the canvas untouched
    const jda_image_info I = *jda_coef_image_get_info(img);
    int bpp, ow, oh, cw, ch;
    int rc = jda_output_geometry(&I, pixel_type, options, &bpp, &ow, &oh, &cw, &ch);
    if (rc != JDA_SUCCESS) { jda_coef_image_free(img); return rc; }
    jda_dev_coef *dimg = jda_coef_upload(ctx, img, &err);
    jda_coef_image_free(img);
    if (!dimg) return err;
    const int dpitch = (int)align16((size_t)cw * bpp), drows = rows < ch ? rows : ch;
    void *dout = NULL;
    if (jda_pool_alloc(ctx, &dout, (size_t)dpitch * ch) != hipSuccess) { jda_dev_coef_free(ctx, dimg); return JDA_ERROR_MEMORY; }
    jda_output O;
    O.pixels = dout; O.pitch_bytes = dpitch; O.width_px = cw; O.rows = drows;
    jda_coef_plan plan;
    const jda_dev_coef *one = dimg;
    uint8_t *blk = NULL;
    rc = jda_coef_plan_build(1, &one, &O, &pixel_type, &options, NULL, NULL, &plan);
    if (rc == JDA_SUCCESS && jda_pool_alloc(ctx, (void **)&blk, plan.blob.size()) != hipSuccess) rc = JDA_ERROR_MEMORY;
    if (rc == JDA_SUCCESS) { const hipError_t e = jda_coef_plan_launch(plan, blk, ctx->stream); if (e != hipSuccess) rc = jda_set_err(ctx, e, "jda_coef_tiles"); }
    if (rc == JDA_SUCCESS && drows > 0) {
        const size_t row_bytes = (size_t)cw * bpp < (size_t)pitch_bytes ? (size_t)cw * bpp : (size_t)pitch_bytes;
        rc = copy_rows_back(ctx, host_pixels, (size_t)pitch_bytes, dout, (size_t)dpitch, row_bytes, (size_t)drows, false);
    } else (void)hipStreamSynchronize(ctx->stream);
    if (blk) jda_pool_free(ctx, blk);
    jda_pool_free(ctx, dout);
    jda_dev_coef_free(ctx, dimg);
    if (rc == JDA_SUCCESS && mcus_decoded) *mcus_decoded = I.mcus_x * I.mcus_y;
    return rc;
}

int jda_decode_to_host_flags(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *mcu_rect,
                             void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded, int32_t *tiles, int32_t flags)
{
    if (ctx && !mcu_rect && (options & JDA_PROGRESSIVE_FULL)) {      // (a baseline file: the bit means nothing, the usual path)
        jda_image_info I;
        if (jda_parse(jpeg, len, &I) == JDA_SUCCESS && jda_progressive_full_requested(&I, options)) {
            if (mcus_decoded) *mcus_decoded = 0;
            if (tiles) tiles[0] = tiles[1] = 0;
            return progressive_full_to_host(ctx, jpeg, len, pixel_type, options, host_pixels, pitch_bytes, rows, mcus_decoded);
        }
    }
    return jda_decode_to_host_bands(ctx, jpeg, len, pixel_type, options, mcu_rect, host_pixels, pitch_bytes, rows, mcus_decoded, tiles, flags, 1, NULL, NULL);
}

// Who makes the index of ONE image (jda_decode_to_host*, the class).
static int32_t jda_onecall_prepare_flags(int32_t len)
{
    // One image at a time, the device pre-scan is seven latency-bound launches of ~0.1-0.15 ms each whatever the size (a 640x480 scan
    // is four wavefronts' worth of segments).  The host pre-scan costs 8 us per KB of file on one thread and 2.3 on six around one L3
    // (jda_frontend.cpp, host_prescan_chunks / _intervals): measured end to end on the GPU box (six threads), 1920x1080 (214 KB) 0.65 ms
    // with the host's index against 0.80 with the device's, 2560x1440 (377 KB) 1.08 against 0.90, 4096x4096 4.5 against 1.44 -- the
    // device from 256 KB on; from 128 KB where the host has fewer threads (one: 6.8 us per KB, 1920x1080 1.95 ms).  In batches the
    // device always does it.
    static const int32_t dev_from = []() {
        const char *e = JDA_LAB_ENV("JDA_ONECALL_DEVICE_PRESCAN_BYTES");   // (for measuring the crossover)
        return e ? atoi(e) : ((jda_host_prescan_threads() >= 6 ? 256 : 128) << 10);
    }();
    return len >= dev_from ? JDA_PREPARE_DEVICE_PRESCAN : 0;
}

// ---- the frame of the one calls: ONE file prepared, uploaded, decoded onto a canvas from the pool, released.  What a
// call keeps between those steps is in `onecall`; the entry points call oc_open, oc_geometry, oc_upload, oc_plan, oc_run and oc_close in
// that order, with their own checks, surfaces, uploads and launches between them -- what reaches the context's stream, and in which order,
// is read off each entry point's own body.
struct onecall {
    jda_ctx *ctx; jda_image *img; jda_dev_image *dimg;
    uint8_t *dsurf; jda_batch *b;                // the pool block (the canvas, the caller's surfaces behind it) and the launch plan
    jda_image_info I;                            // (by value: the image is freed as soon as it is uploaded)
    int32_t pixel_type, options;
    int bpp, ow, oh, cw, ch, mw, mh, cpitch;     // mw x mh: the MCU in canvas pixels
    size_t cbytes;
    uint32_t nok; bool complete;
    jda_output C, S;                             // the canvas, and its visible rectangle
    double t_mark;
};
static bool oc_tracing() { static const bool on = JDA_LAB_ENV("JDA_ONECALL_TRACE") != NULL; return on; }       // stage timings on stderr (diagnostics)
#define JDA_OC_MARK(F, what) do { if (oc_tracing()) { const double t_ = now_ms(); fprintf(stderr, "jda_decode_to_host: %-24s %7.3f ms\n", what, t_ - (F).t_mark); (F).t_mark = t_; } } while (0)
// The host's half.  The image stays open: the entry point checks its own parameters against F.I and the geometry and, where it refuses,
// frees F.img and returns -- nothing has been uploaded or launched by then.
static int oc_open(onecall &F, jda_ctx *ctx, const uint8_t *jpeg, int32_t len)
{
    memset(&F, 0, sizeof(F));
    F.ctx = ctx;
    F.t_mark = oc_tracing() ? now_ms() : 0.0;
    (void)hipSetDevice(ctx->device);
    int32_t err = JDA_SUCCESS;
    F.img = jda_prepare_ex(jpeg, len, jda_onecall_prepare_flags(len), &err);
    if (!F.img) return err;
    F.I = *jda_image_get_info(F.img);
    return JDA_SUCCESS;
}
static int oc_geometry(onecall &F, int32_t pixel_type, int32_t options)
{
    F.pixel_type = pixel_type; F.options = options;
    const int rc = jda_output_geometry(&F.I, pixel_type, options, &F.bpp, &F.ow, &F.oh, &F.cw, &F.ch);
    if (rc != JDA_SUCCESS) return rc;
    F.mw = F.cw / (F.I.mcus_x ? F.I.mcus_x : 1); F.mh = F.ch / (F.I.mcus_y ? F.I.mcus_y : 1);
    F.cpitch = (int)align16((size_t)F.cw * F.bpp); F.cbytes = (size_t)F.cpitch * F.ch;
    JDA_OC_MARK(F, "prepare (host)");
    return JDA_SUCCESS;
}
// The file goes up and the host image goes away; a pool block of surf_bytes (F.cbytes and what the caller wants behind the canvas) with the
// canvas C at its head, S the canvas's visible rectangle.  The index is read only AFTER the upload: where the device makes it
// (JDA_PREPARE_DEVICE_PRESCAN) it exists, and a bad MCU is known, only then.  On failure nothing is left to release.
static int oc_upload(onecall &F, size_t surf_bytes, int32_t *mcus_decoded)
{
    int32_t err = JDA_SUCCESS;
    F.dimg = jda_upload(F.ctx, F.img, &err);
    JDA_OC_MARK(F, "upload + device pre-scan");
    jda_image_block_index(F.img, &F.nok);
    F.complete = F.nok == (uint32_t)(F.I.mcus_x * F.I.mcus_y);
    if (mcus_decoded) *mcus_decoded = (int32_t)F.nok;
    jda_image_free(F.img);
    F.img = NULL;
    if (!F.dimg) return err;
    if (jda_pool_alloc(F.ctx, (void **)&F.dsurf, surf_bytes) != hipSuccess) { jda_dev_image_free(F.ctx, F.dimg); return JDA_ERROR_MEMORY; }
    F.C.pixels = F.dsurf; F.C.pitch_bytes = F.cpitch; F.C.width_px = F.cw; F.C.rows = F.ch;
    F.S = F.C; F.S.width_px = F.ow; F.S.rows = F.oh;
    return JDA_SUCCESS;
}
// the MCUs that hold the canvas pixels reads = { x0, y0, x1, y1 } -> mcu_rect; true: every MCU of the image
static bool oc_mcu_rect(const onecall &F, const int32_t *reads, int32_t *mcu_rect)
{
    mcu_rect[0] = reads[0] / F.mw; mcu_rect[1] = reads[1] / F.mh;
    mcu_rect[2] = std::min((reads[2] + F.mw - 1) / F.mw, F.I.mcus_x); mcu_rect[3] = std::min((reads[3] + F.mh - 1) / F.mh, F.I.mcus_y);
    return mcu_rect[0] == 0 && mcu_rect[1] == 0 && mcu_rect[2] == F.I.mcus_x && mcu_rect[3] == F.I.mcus_y;
}
// the launch plan over the canvas C: an MCU rectangle or all of the image (NULL), strip-major (strip_mcus) or row-major (NULL)
static int oc_plan(onecall &F, const int32_t *mcu_rect, const int32_t *strip_mcus, int32_t *tiles)
{
    int32_t err = JDA_SUCCESS;
    F.b = jda_batch_create_strips(F.ctx, 1, &F.dimg, &F.C, &F.pixel_type, &F.options, mcu_rect, strip_mcus, &err);
    if (F.b && tiles) { tiles[0] = (int32_t)F.b->stats.tiles; tiles[1] = (int32_t)F.b->stats.tiles_whole_images; }
    JDA_OC_MARK(F, "surface + launch plan");
    return err;
}
// The decode.  What a bad stream does not reach reads zero: clear_bytes of the block from clear_at on are cleared in front of the decode --
// where the stream has a bad MCU, or (also_complete) whatever it has.
static int oc_run(onecall &F, size_t clear_at, size_t clear_bytes, bool also_complete)
{
    if ((!F.complete || also_complete) && clear_bytes) (void)hipMemsetAsync(F.dsurf + clear_at, 0, clear_bytes, F.ctx->stream);
    return jda_batch_decode(F.ctx, F.b);
}
// The end of every call that got through oc_upload.  A step that failed behind oc_plan may have left work on the stream that reads or
// writes the blocks going back to the pool (plan_block: the post-process's, may be NULL): the stream is drained first.
static int oc_close(onecall &F, int rc, void *plan_block)
{
    if (F.b && rc != JDA_SUCCESS) (void)hipStreamSynchronize(F.ctx->stream);
    JDA_OC_MARK(F, "decode + copy back");
    jda_batch_destroy(F.ctx, F.b);
    jda_pool_free(F.ctx, plan_block);
    jda_pool_free(F.ctx, F.dsurf);
    jda_dev_image_free(F.ctx, F.dimg);
    JDA_OC_MARK(F, "release");
    if (rc == JDA_SUCCESS && !F.complete) rc = JDA_DECODE_ERROR;   // jpeg.inl:5354-5356
    return rc;
}
#undef JDA_OC_MARK

// The whole image as the reference's JPEGDRAW strips (jpeg.inl:5300-5336): strip_mcus MCUs wide, one MCU row high, in raster order, every
// strip's pixels contiguous -- what JPEGDEC::decode hands to the draw callback without touching a pixel (a strip of a row-major canvas is
// a few hundred bytes from each of 16 rows a pitch apart: 8,192 strips of a 4096x4096 image were 1.5 ms of small strided copies).
int jda_decode_to_host_strips(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, int32_t strip_mcus,
                              void *host_pixels, size_t host_bytes, int32_t *mcus_decoded, int32_t n_bands, jda_band_callback *band_ready, void *user)
{
    if (mcus_decoded) *mcus_decoded = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!jpeg || !host_pixels || strip_mcus <= 0) return JDA_INVALID_PARAMETER;
    onecall F;
    int rc = oc_open(F, ctx, jpeg, len);
    if (rc != JDA_SUCCESS) return rc;
    rc = oc_geometry(F, pixel_type, options);
    const jda_image_info &I = F.I;
    const int mh = F.mh, n_sx = (I.mcus_x + strip_mcus - 1) / strip_mcus;
    const size_t strip_bytes = (size_t)strip_mcus * F.mw * mh * F.bpp, row_bytes = (size_t)n_sx * strip_bytes, total = row_bytes * I.mcus_y;
    if (rc == JDA_SUCCESS && host_bytes < total) rc = JDA_INVALID_PARAMETER;
    if (rc != JDA_SUCCESS) { jda_image_free(F.img); return rc; }
    rc = oc_upload(F, std::max(total, F.cbytes) + 256, mcus_decoded);
    if (rc != JDA_SUCCESS) return rc;
    rc = oc_plan(F, NULL, &strip_mcus, NULL);
    if (rc == JDA_SUCCESS) rc = oc_run(F, 0, total, false);                      // (callback mode: what a bad stream does not reach reads zero)
    if (rc == JDA_SUCCESS) {
        int nb = (band_ready && n_bands > 1) ? (n_bands > JDA_MAX_BANDS ? JDA_MAX_BANDS : n_bands) : 1;
        if (nb > I.mcus_y) nb = I.mcus_y;
        const int per = (I.mcus_y + nb - 1) / nb;                                // MCU rows a band
        hipError_t e = hipSuccess;
        int made = 0;
        for (int k = 0; k < nb && e == hipSuccess; k++) {
            const int y0 = k * per, y1 = std::min(I.mcus_y, y0 + per);
            if (y0 >= y1) break;
            if (!ctx->ev_band[k]) e = hipEventCreateWithFlags(&ctx->ev_band[k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipMemcpyAsync((uint8_t *)host_pixels + (size_t)y0 * row_bytes, F.dsurf + (size_t)y0 * row_bytes, (size_t)(y1 - y0) * row_bytes, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(ctx->ev_band[k], ctx->stream);
            if (e == hipSuccess) made++;
        }
        for (int k = 0; k < made && e == hipSuccess; k++) {
            e = hipEventSynchronize(ctx->ev_band[k]);
            if (e == hipSuccess && band_ready) (*band_ready)(user, k * per * mh, std::min(I.mcus_y, (k + 1) * per) * mh);
        }
        { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
        if (e != hipSuccess) rc = jda_set_err(ctx, e, "copy back");
    }
    return oc_close(F, rc, NULL);
}

int jda_decode_to_host_bands(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *mcu_rect,
                             void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded, int32_t *tiles, int32_t flags,
                             int32_t n_bands, jda_band_callback *band_ready, void *user)
{
    if (mcus_decoded) *mcus_decoded = 0;
    if (tiles) tiles[0] = tiles[1] = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    onecall F;
    int rc = oc_open(F, ctx, jpeg, len);
    if (rc != JDA_SUCCESS) return rc;
    rc = oc_geometry(F, pixel_type, options);
    if (rc != JDA_SUCCESS) { jda_image_free(F.img); return rc; }
    rc = oc_upload(F, F.cbytes, mcus_decoded);
    if (rc != JDA_SUCCESS) return rc;
    const jda_image_info &I = F.I;
    const int dpitch = F.cpitch, mh_out = F.mh;
    const int drows = rows < F.ch ? rows : F.ch;
    const size_t row_bytes = (size_t)F.cw * F.bpp < (size_t)pitch_bytes ? (size_t)F.cw * F.bpp : (size_t)pitch_bytes;
    uint8_t *const dout = F.dsurf;
    F.C.rows = drows;
    // only the MCU rows of the rectangle are decoded, zeroed where nothing is written, and copied back
    int r0 = 0, r1 = drows;
    if (mcu_rect) { r0 = std::max(0, std::min(drows, mcu_rect[1] * mh_out)); r1 = std::max(r0, std::min(drows, mcu_rect[3] * mh_out)); }
    rc = oc_plan(F, mcu_rect, NULL, tiles);
    if (rc == JDA_SUCCESS) rc = oc_run(F, (size_t)r0 * dpitch, r1 > r0 ? (size_t)dpitch * (r1 - r0) : 0, mcu_rect != NULL);
    if (rc == JDA_SUCCESS && !F.complete && (flags & JDA_TO_HOST_KEEP_UNDECODED) && !mcu_rect) {
        // the reference returns at the bad MCU and leaves the rest of the caller's buffer alone (jpeg.inl:5354-5356): copy back the
        // whole MCU rows in front of it and, of its own row, the MCUs in front of it -- nothing else of the host buffer is touched
        const int full = (int)(F.nok / (uint32_t)I.mcus_x), part = (int)(F.nok % (uint32_t)I.mcus_x);
        const int rf = std::min(drows, full * mh_out), rp = std::min(drows, (full + 1) * mh_out);
        hipError_t e = hipSuccess;
        if (rf > 0) e = hipMemcpy2DAsync(host_pixels, (size_t)pitch_bytes, dout, (size_t)dpitch, row_bytes, (size_t)rf, hipMemcpyDeviceToHost, ctx->stream);
        const size_t part_bytes = std::min(row_bytes, (size_t)part * F.mw * F.bpp);
        if (e == hipSuccess && part_bytes && rp > rf)
            e = hipMemcpy2DAsync((uint8_t *)host_pixels + (size_t)rf * pitch_bytes, (size_t)pitch_bytes, dout + (size_t)rf * dpitch, (size_t)dpitch, part_bytes, (size_t)(rp - rf), hipMemcpyDeviceToHost, ctx->stream);
        { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
        if (e != hipSuccess) rc = jda_set_err(ctx, e, "copy back");
    } else if (rc == JDA_SUCCESS && r1 > r0 && band_ready && n_bands > 1) {
        // the copy back in bands of whole MCU rows, the caller told as each one lands: what it does with band k (the class replays its
        // draw callbacks) runs while band k + 1 is still on the bus
        int nb = n_bands > JDA_MAX_BANDS ? JDA_MAX_BANDS : n_bands;
        const int mrows = (r1 - r0 + mh_out - 1) / mh_out;
        if (nb > mrows) nb = mrows;
        const int per = ((mrows + nb - 1) / nb) * mh_out;
        hipError_t e = hipSuccess;
        int made = 0;
        for (int k = 0; k < nb && e == hipSuccess; k++) {
            const int b0 = r0 + k * per, b1 = std::min(r1, b0 + per);
            if (b0 >= b1) break;
            if (!ctx->ev_band[k]) e = hipEventCreateWithFlags(&ctx->ev_band[k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipMemcpy2DAsync((uint8_t *)host_pixels + (size_t)b0 * pitch_bytes, (size_t)pitch_bytes, dout + (size_t)b0 * dpitch, (size_t)dpitch, row_bytes, (size_t)(b1 - b0), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(ctx->ev_band[k], ctx->stream);
            if (e == hipSuccess) made++;
        }
        for (int k = 0; k < made && e == hipSuccess; k++) {
            e = hipEventSynchronize(ctx->ev_band[k]);
            if (e == hipSuccess) (*band_ready)(user, r0 + k * per, std::min(r1, r0 + (k + 1) * per));
        }
        // (also after an error: copies queued before it may still be writing the caller's buffer, and the surface goes back to the pool)
        { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
        if (e != hipSuccess) rc = jda_set_err(ctx, e, "copy back");
    } else if (rc == JDA_SUCCESS && r1 > r0)
        rc = copy_rows_back(ctx, (uint8_t *)host_pixels + (size_t)r0 * pitch_bytes, (size_t)pitch_bytes, dout + (size_t)r0 * dpitch, (size_t)dpitch, row_bytes, (size_t)(r1 - r0), false);
    return oc_close(F, rc, NULL);
}

// ---- 4 / 2 / 1-bpp output (jda_dither_rows in jda_kernels.hip)
static inline uint32_t dither_bits_of(int32_t pt) { return pt == JDA_FOUR_BIT_DITHERED ? 4u : pt == JDA_TWO_BIT_DITHERED ? 2u : pt == JDA_ONE_BIT_DITHERED ? 1u : 0u; }
// Upload the job records of n canvases (and wait for them: they leave pageable memory that goes away with this frame); *d_block (pool
// block: jobs, the give-up flag, seeds) is the caller's to release once the stream has drained.  dither_launch then queues the kernel.
struct dither_plan { void *block; uint32_t *d_fail; uint32_t n, max_w, max_h; };
static int dither_upload(jda_ctx *ctx, int32_t n, const jda_output *gray, const int32_t *strip_rows, const int32_t *pixel_types, const uint8_t *const *seeds,
                         const jda_output *packed, dither_plan *plan)
{
    plan->block = NULL;
    std::vector<jda_dither_job> jobs((size_t)n);
    const size_t jobs_bytes = align16(jobs.size() * sizeof(jda_dither_job)), seed_stride = align16(JDA_DITHER_SEED_BYTES);
    std::vector<uint8_t> seed_host;
    for (int i = 0; i < n && seeds; i++) if (seeds[i]) { seed_host.assign((size_t)n * seed_stride, 0); break; }
    uint32_t max_w = 0, max_h = 0;
    for (int i = 0; i < n; i++) {
        const jda_output &G = gray[i], &P = packed[i];
        const uint32_t bits = dither_bits_of(pixel_types[i]);
        if (!bits || !G.pixels || !P.pixels || G.width_px <= 0 || G.width_px > 65535 || G.rows <= 0 || strip_rows[i] <= 0) return JDA_INVALID_PARAMETER;
        if (((uintptr_t)G.pixels & 15u) || (G.pitch_bytes & 15) || G.pitch_bytes < G.width_px) return JDA_INVALID_PARAMETER;
        const int32_t dp = (int32_t)(((uint32_t)G.width_px * bits + 7u) >> 3);
        if (((uintptr_t)P.pixels & 3u) || (P.pitch_bytes & 3) || P.pitch_bytes < dp || P.rows < G.rows) return JDA_INVALID_PARAMETER;
        jda_dither_job &J = jobs[(size_t)i];
        J.gray = (const uint8_t *)G.pixels; J.out = (uint8_t *)P.pixels;
        J.gray_pitch = (uint32_t)G.pitch_bytes; J.out_pitch = (uint32_t)P.pitch_bytes;
        J.width = (uint32_t)G.width_px; J.height = (uint32_t)G.rows; J.strip_rows = (uint32_t)strip_rows[i]; J.bits = bits;
        max_w = std::max(max_w, J.width); max_h = std::max(max_h, J.height);
    }
    uint8_t *blk = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, jobs_bytes + 16 + seed_host.size());
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(dither jobs)");
    plan->block = blk; plan->d_fail = (uint32_t *)(blk + jobs_bytes); plan->n = (uint32_t)n; plan->max_w = max_w; plan->max_h = max_h;
    for (int i = 0; i < n; i++) {
        jobs[(size_t)i].seed = NULL;
        if (seed_host.empty() || !seeds[i]) continue;
        memcpy(&seed_host[(size_t)i * seed_stride], seeds[i], JDA_DITHER_SEED_BYTES);
        jobs[(size_t)i].seed = blk + jobs_bytes + 16 + (size_t)i * seed_stride;
    }
    e = hipMemcpyAsync(blk, jobs.data(), jobs.size() * sizeof(jda_dither_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && !seed_host.empty()) e = hipMemcpyAsync(blk + jobs_bytes + 16, seed_host.data(), seed_host.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(plan->d_fail, 0, 16, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { jda_pool_free(ctx, blk); plan->block = NULL; return jda_set_err(ctx, e, "dither jobs"); }
    return JDA_SUCCESS;
}
static int dither_launch(jda_ctx *ctx, const dither_plan &plan)
{
    const hipError_t e = jda_launch_dither((const jda_dither_job *)plan.block, plan.n, plan.max_w, plan.max_h, plan.d_fail, ctx->stream);
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_dither_rows");
}
// the context's grow-only page-locked block, at least `bytes` of it (whatever used it before has drained: the stream is synchronised before it is replaced)
static uint8_t *ctx_pinned_block(jda_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->pinned_cap) return ctx->pinned;
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = NULL; ctx->pinned_cap = 0;
    if (hipHostMalloc((void **)&ctx->pinned, bytes, hipHostMallocDefault) != hipSuccess) { ctx->pinned = NULL; return NULL; }
    ctx->pinned_cap = bytes;
    return ctx->pinned;
}

int jda_dither_surfaces(jda_ctx *ctx, int32_t n, const jda_output *gray, const int32_t *strip_rows, const int32_t *pixel_types,
                        const uint8_t *const *seeds, const jda_output *packed)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n <= 0 || !gray || !strip_rows || !pixel_types || !packed) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    dither_plan plan;
    uint32_t fail = 0;
    int rc = dither_upload(ctx, n, gray, strip_rows, pixel_types, seeds, packed, &plan);
    if (rc != JDA_SUCCESS) return rc;
    rc = dither_launch(ctx, plan);
    hipError_t e = rc == JDA_SUCCESS ? hipMemcpyAsync(&fail, plan.d_fail, sizeof(fail), hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    jda_pool_free(ctx, plan.block);
    if (rc != JDA_SUCCESS) return rc;
    if (e != hipSuccess) return jda_set_err(ctx, e, "jda_dither_surfaces");
    if (fail) { snprintf(ctx->last_error, sizeof(ctx->last_error), "jda_dither_rows: a wavefront gave up waiting for the rows above it"); return JDA_ERROR_HIP; }
    return JDA_SUCCESS;
}

int jda_decode_dither_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options,
                              const uint8_t *seed, void *host_packed, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded)
{
    uint8_t own_seed[JDA_DITHER_SEED_BYTES];
    if (!seed && jpeg) { (void)jda_dither_seed(jpeg, len, 0, own_seed); seed = own_seed; }
    if (mcus_decoded) *mcus_decoded = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    const uint32_t bits = dither_bits_of(pixel_type);
    if (!bits || !jpeg || !host_packed) return JDA_INVALID_PARAMETER;
    onecall F;
    int rc = oc_open(F, ctx, jpeg, len);
    if (rc != JDA_SUCCESS) return rc;
    rc = oc_geometry(F, JDA_EIGHT_BIT_GRAYSCALE, options);
    const int cw = F.cw, ch = F.ch;
    int32_t dbits = 0, dpitch = 0;
    int64_t dbytes = 0;
    if (rc == JDA_SUCCESS) rc = jda_dither_geometry(cw, ch, pixel_type, &dbits, &dpitch, &dbytes);
    if (rc == JDA_SUCCESS && (pitch_bytes < dpitch || F.I.mcus_y <= 0 || ch % F.I.mcus_y)) rc = JDA_INVALID_PARAMETER;
    if (rc != JDA_SUCCESS) { jda_image_free(F.img); return rc; }
    // (the packed surface at the caller's own pitch where the kernel's dword stores allow it: the copy back then lands where it belongs)
    const int ppitch = (pitch_bytes == dpitch && !(dpitch & 3)) ? dpitch : (int)align16((size_t)dpitch);
    rc = oc_upload(F, F.cbytes + (size_t)ppitch * ch, mcus_decoded);              // the gray canvas, the packed rows behind it
    if (rc != JDA_SUCCESS) return rc;
    jda_output P;
    P.pixels = F.dsurf + F.cbytes; P.pitch_bytes = ppitch; P.width_px = cw; P.rows = ch;
    dither_plan plan;
    plan.block = NULL;
    rc = oc_plan(F, NULL, NULL, NULL);
    if (rc == JDA_SUCCESS) {
        // everything that has to wait for the host -- the job record, the staging block -- first; then decode, dither and the copy back are
        // queued back to back
        uint32_t fail = 0;
        const int32_t strip = F.mh;                     // the rows of one MCU row, as scaled (jpeg.inl:5048-5049, :5310)
        const int drows = rows < ch ? rows : ch;
        rc = dither_upload(ctx, 1, &F.C, &strip, &pixel_type, &seed, &P, &plan);
        // the packed rows come back as ONE copy at the device pitch into page-locked memory and are brought to the caller's pitch here: a
        // 2-D copy of thousands of rows of an odd width into pageable memory goes row by row (3596 x 2840 at 1 bpp: 450-byte rows, +25 ms)
        uint8_t *stage = NULL;
        if (rc == JDA_SUCCESS && drows > 0 && pitch_bytes != ppitch) { stage = ctx_pinned_block(ctx, (size_t)ppitch * drows); if (!stage) rc = JDA_ERROR_MEMORY; }
        if (rc == JDA_SUCCESS) rc = oc_run(F, 0, F.cbytes, false);
        if (rc == JDA_SUCCESS) rc = dither_launch(ctx, plan);
        if (rc == JDA_SUCCESS) {
            hipError_t e = hipSuccess;
            if (drows > 0) e = hipMemcpyAsync(stage ? (void *)stage : host_packed, P.pixels, (size_t)ppitch * drows, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&fail, plan.d_fail, sizeof(fail), hipMemcpyDeviceToHost, ctx->stream);
            { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
            if (e == hipSuccess && stage)
                for (int r = 0; r < drows; r++) memcpy((uint8_t *)host_packed + (size_t)r * pitch_bytes, stage + (size_t)r * ppitch, (size_t)dpitch);
            if (e != hipSuccess) rc = jda_set_err(ctx, e, "copy back");
            else if (fail) { snprintf(ctx->last_error, sizeof(ctx->last_error), "jda_dither_rows: a wavefront gave up waiting for the rows above it"); rc = JDA_ERROR_HIP; }
        }
    }
    return oc_close(F, rc, plan.block);
}

// ---- EXIF orientation (jda_orient_tiles in jda_kernels.hip; the permutation and its tiles: jda_device_core.h)
// Check n surfaces and upload their job records (and wait for them: they leave pageable memory that goes away with this frame); plan->block
// (pool block) is the caller's to release once the stream has drained.  orient_launch then queues the kernel.
struct orient_plan { void *block; uint32_t n, n_tiles, bpp; };
static int orient_upload(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *orientations, const jda_output *dst, orient_plan *plan)
{
    plan->block = NULL; plan->n = (uint32_t)n; plan->n_tiles = 0; plan->bpp = (uint32_t)bytes_per_pixel;
    if (bytes_per_pixel != 1 && bytes_per_pixel != 2 && bytes_per_pixel != 4) return JDA_INVALID_PARAMETER;
    std::vector<jda_orient_job> jobs((size_t)n);
    struct range { uintptr_t a, b; int32_t i; bool is_dst; };
    std::vector<range> ranges;
    ranges.reserve((size_t)n * 2);
    uint64_t tiles = 0;
    for (int i = 0; i < n; i++) {
        const jda_output &S = src[i], &D = dst[i];
        const int32_t o = orientations[i];
        if (o < 0 || o > 8 || !S.pixels || !D.pixels || S.width_px <= 0 || S.rows <= 0 || S.width_px > (1 << 24) || S.rows > (1 << 24)) return JDA_INVALID_PARAMETER;
        uint32_t dw, dh;
        jda_orient_dims((uint32_t)o, (uint32_t)S.width_px, (uint32_t)S.rows, dw, dh);
        if (D.width_px != (int32_t)dw || D.rows != (int32_t)dh) return JDA_INVALID_PARAMETER;
        const int64_t srow = (int64_t)S.width_px * bytes_per_pixel, drow = (int64_t)dw * bytes_per_pixel;
        if (((uintptr_t)S.pixels & 15u) || ((uintptr_t)D.pixels & 15u) || (S.pitch_bytes & 15) || (D.pitch_bytes & 15)) return JDA_INVALID_PARAMETER;
        if (S.pitch_bytes < srow || D.pitch_bytes < drow) return JDA_INVALID_PARAMETER;
        // what the launch reads (whole aligned vectors of every row) and what it writes
        ranges.push_back({ (uintptr_t)S.pixels, (uintptr_t)S.pixels + (size_t)(S.rows - 1) * (size_t)S.pitch_bytes + align16((size_t)srow), i, false });
        ranges.push_back({ (uintptr_t)D.pixels, (uintptr_t)D.pixels + (size_t)(dh - 1) * (size_t)D.pitch_bytes + (size_t)drow, i, true });
        jda_orient_job &J = jobs[(size_t)i];
        J.src = (const uint8_t *)S.pixels; J.dst = (uint8_t *)D.pixels;
        J.src_pitch = (uint32_t)S.pitch_bytes; J.dst_pitch = (uint32_t)D.pitch_bytes;
        J.width = (uint32_t)S.width_px; J.height = (uint32_t)S.rows; J.orientation = (uint32_t)o; J.pad_ = 0;
        uint32_t tx, ty;
        jda_orient_tile_grid((uint32_t)o, (uint32_t)bytes_per_pixel, J.width, J.height, tx, ty);
        J.tile0 = (uint32_t)tiles; J.tiles_x = tx;
        tiles += (uint64_t)tx * ty;
        if (tiles > 0x7fffffffull) return JDA_INVALID_PARAMETER;
    }
    // a destination may share no byte with a source or with another destination: sorted by start, a range that begins inside the union of
    // the ranges before it overlaps one of them -- two sources may, anything with a destination in it may not
    std::sort(ranges.begin(), ranges.end(), [](const range &x, const range &y) { return x.a < y.a; });
    uintptr_t end_any = 0, end_dst = 0;
    for (const range &r : ranges) {
        if (r.is_dst ? r.a < end_any : r.a < end_dst) return JDA_INVALID_PARAMETER;
        end_any = std::max(end_any, r.b);
        if (r.is_dst) end_dst = std::max(end_dst, r.b);
    }
    uint8_t *blk = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, align16(jobs.size() * sizeof(jda_orient_job)));
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(orient jobs)");
    e = hipMemcpyAsync(blk, jobs.data(), jobs.size() * sizeof(jda_orient_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { jda_pool_free(ctx, blk); return jda_set_err(ctx, e, "orient jobs"); }
    plan->block = blk; plan->n_tiles = (uint32_t)tiles;
    return JDA_SUCCESS;
}
static int orient_launch(jda_ctx *ctx, const orient_plan &plan)
{
    const hipError_t e = jda_launch_orient((const jda_orient_job *)plan.block, plan.n, plan.n_tiles, plan.bpp, ctx->stream);
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_orient_tiles");
}

int jda_orient_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *orientations, const jda_output *dst)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0 || (bytes_per_pixel != 1 && bytes_per_pixel != 2 && bytes_per_pixel != 4)) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!src || !orientations || !dst) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    orient_plan plan;
    int rc = orient_upload(ctx, n, src, bytes_per_pixel, orientations, dst, &plan);
    if (rc != JDA_SUCCESS) return rc;
    return finish_surfaces(ctx, orient_launch(ctx, plan), plan.block, "jda_orient_surfaces");
}

int jda_decode_to_host_oriented(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, int32_t orientation,
                                void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded)
{
    if (mcus_decoded) *mcus_decoded = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!jpeg || !host_pixels || orientation > 8 || pixel_type < 0 || pixel_type > JDA_EIGHT_BIT_GRAYSCALE) return JDA_INVALID_PARAMETER;
    onecall F;
    int rc = oc_open(F, ctx, jpeg, len);
    if (rc != JDA_SUCCESS) return rc;
    rc = oc_geometry(F, pixel_type, options);
    int tw = 0, th = 0;
    if (rc == JDA_SUCCESS) rc = jda_oriented_geometry(&F.I, pixel_type, options, orientation, NULL, &tw, &th, NULL);
    if (rc == JDA_SUCCESS && (F.ow > F.cw || F.oh > F.ch || pitch_bytes < tw * F.bpp || rows < th)) rc = JDA_INVALID_PARAMETER;
    if (rc != JDA_SUCCESS) { jda_image_free(F.img); return rc; }
    int32_t o = orientation < 0 ? F.I.orientation : orientation;
    if (o < 2 || o > 8) o = 0;                          // "as it is": the visible rectangle goes back from the canvas itself
    const int opitch = (int)align16((size_t)tw * F.bpp);
    rc = oc_upload(F, F.cbytes + (o ? (size_t)opitch * th : 0), mcus_decoded);    // the decoded canvas, the oriented surface behind it
    if (rc != JDA_SUCCESS) return rc;
    jda_output D;
    D.pixels = F.dsurf + F.cbytes; D.pitch_bytes = opitch; D.width_px = tw; D.rows = th;
    orient_plan plan;
    plan.block = NULL;
    rc = oc_plan(F, NULL, NULL, NULL);
    // what has to wait for the host -- the job record -- first; then decode, orient and the copy back are queued back to back
    if (rc == JDA_SUCCESS && o) rc = orient_upload(ctx, 1, &F.S, F.bpp, &o, &D, &plan);
    if (rc == JDA_SUCCESS) rc = oc_run(F, 0, F.cbytes, false);                    // (the MCUs a bad stream does not reach are zeros before they are turned)
    if (rc == JDA_SUCCESS && o) rc = orient_launch(ctx, plan);
    if (rc == JDA_SUCCESS) rc = copy_rows_back(ctx, host_pixels, (size_t)pitch_bytes, o ? D.pixels : F.dsurf, (size_t)(o ? opitch : F.cpitch), (size_t)tw * F.bpp, (size_t)th, true);
    return oc_close(F, rc, plan.block);
}

// ---- dense RGB / BGR / planar output (jda_pack_tiles in jda_kernels.hip; runs, vectors and the lane's walk: jda_device_core.h)
// Check n jobs (jda_pack_plan.h) and upload their records, and wait for them as orient_upload does; pack_launch then queues the kernel.
struct pack_plan { void *block; uint32_t n, n_tiles, es, hwc, bpp, bgr; const uint8_t *table; };
static int pack_upload(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t src_bytes_per_pixel, const int32_t *rects, int32_t layout_flags, int32_t elem_type,
                       const void *table, void *const *dst, pack_plan *plan)
{
    plan->block = NULL; plan->n = (uint32_t)n; plan->n_tiles = 0;
    jda_pack_plan_out P;
    const int rc = jda_pack_plan_jobs(n, src, src_bytes_per_pixel, rects, layout_flags, elem_type, table, dst, &P);
    if (rc != JDA_SUCCESS) return rc;
    plan->es = P.es; plan->hwc = P.hwc; plan->bpp = (uint32_t)src_bytes_per_pixel; plan->bgr = (layout_flags & JDA_PACK_BGR) ? 1u : 0u;
    plan->table = (const uint8_t *)table;
    uint8_t *blk = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, align16(P.jobs.size() * sizeof(jda_pack_job)));
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(pack jobs)");
    e = hipMemcpyAsync(blk, P.jobs.data(), P.jobs.size() * sizeof(jda_pack_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { jda_pool_free(ctx, blk); return jda_set_err(ctx, e, "pack jobs"); }
    plan->block = blk; plan->n_tiles = P.n_tiles;
    return JDA_SUCCESS;
}
static int pack_launch(jda_ctx *ctx, const pack_plan &plan)
{
    const hipError_t e = jda_launch_pack((const jda_pack_job *)plan.block, plan.n, plan.n_tiles, (int)plan.hwc, plan.es, plan.table, plan.bpp, plan.bgr, ctx->stream);
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_pack_tiles");
}

size_t jda_pack_bytes(int32_t w, int32_t h, int32_t channels, int32_t elem_type)
{
    const uint32_t es = jda_pack_elem_bytes(elem_type);
    if (w <= 0 || h <= 0 || channels <= 0 || !es) return 0;
    return (size_t)w * (size_t)h * (size_t)channels * es;
}

int jda_pack_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t src_bytes_per_pixel, const int32_t *rects,
                      int32_t layout_flags, int32_t elem_type, const void *table, void *const *dst)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0) return JDA_INVALID_PARAMETER;
    { const int frc = jda_pack_check_format(src_bytes_per_pixel, layout_flags, elem_type, table); if (frc != JDA_SUCCESS) return frc; }
    if (n == 0) return JDA_SUCCESS;
    (void)hipSetDevice(ctx->device);
    pack_plan plan;
    int rc = pack_upload(ctx, n, src, src_bytes_per_pixel, rects, layout_flags, elem_type, table, dst, &plan);
    if (rc != JDA_SUCCESS) return rc;
    return finish_surfaces(ctx, pack_launch(ctx, plan), plan.block, "jda_pack_surfaces");
}

int jda_decode_to_host_packed(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, int32_t layout_flags, int32_t elem_type,
                              const void *table, void *host_out, size_t out_bytes, int32_t *w, int32_t *h, int32_t *mcus_decoded)
{
    if (mcus_decoded) *mcus_decoded = 0;
    if (w) *w = 0;
    if (h) *h = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!jpeg || !host_out) return JDA_INVALID_PARAMETER;
    onecall F;
    int rc = oc_open(F, ctx, jpeg, len);
    if (rc != JDA_SUCCESS) return rc;
    const int32_t pixel_type = (F.I.ncomp == 1 || (options & JDA_LUMA_ONLY)) ? JDA_EIGHT_BIT_GRAYSCALE : JDA_RGB8888;
    rc = oc_geometry(F, pixel_type, options);
    const uint32_t es = jda_pack_elem_bytes(elem_type), channels = pixel_type == JDA_RGB8888 ? 3u : 1u;
    // (the table is HOST memory here: its alignment does not matter, the device copy's does)
    if (rc == JDA_SUCCESS) rc = jda_pack_check_format(F.bpp, layout_flags, elem_type, table ? (const void *)16 : NULL);
    const size_t dense = rc == JDA_SUCCESS ? jda_pack_bytes(F.ow, F.oh, (int32_t)channels, elem_type) : 0;
    if (rc == JDA_SUCCESS && (F.ow > F.cw || F.oh > F.ch || out_bytes < dense)) rc = JDA_INVALID_PARAMETER;
    if (rc != JDA_SUCCESS) { jda_image_free(F.img); return rc; }
    if (w) *w = F.ow;
    if (h) *h = F.oh;
    const size_t tbytes = table ? (size_t)channels * 256u * es : 0;
    rc = oc_upload(F, F.cbytes + align16(dense) + tbytes, mcus_decoded);          // the decoded canvas, the dense result and the table behind it
    if (rc != JDA_SUCCESS) return rc;
    uint8_t *ddense = F.dsurf + F.cbytes, *dtable = table ? ddense + align16(dense) : NULL;
    pack_plan plan;
    plan.block = NULL;
    rc = oc_plan(F, NULL, NULL, NULL);
    if (rc == JDA_SUCCESS) {
        // what has to wait for the host -- the table and the job record -- first; then decode, pack and the copy back are queued back to back
        if (table && hipMemcpyAsync(dtable, table, tbytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = JDA_ERROR_HIP;
        void *const dsts[1] = { ddense };
        if (rc == JDA_SUCCESS) rc = pack_upload(ctx, 1, &F.S, F.bpp, NULL, layout_flags, elem_type, dtable, dsts, &plan);
        if (rc == JDA_SUCCESS) rc = oc_run(F, 0, F.cbytes, false);                // (the MCUs a bad stream does not reach are zeros before they are packed)
        if (rc == JDA_SUCCESS) rc = pack_launch(ctx, plan);
        if (rc == JDA_SUCCESS) {
            hipError_t e = hipMemcpyAsync(host_out, ddense, dense, hipMemcpyDeviceToHost, ctx->stream);
            { const hipError_t es2 = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es2; }
            if (e != hipSuccess) rc = jda_set_err(ctx, e, "copy back");
        }
    }
    return oc_close(F, rc, plan.block);
}

// ---- antialiased resize (jda_resize_tiles in jda_kernels.hip; the passes and the tile: jda_device_core.h; checks, taps and tiles: jda_resize_plan.h)
// Check n jobs, build their tap tables and upload both in one block (the job records, the tables behind them), and wait for them as
// orient_upload does; resize_launch then queues the kernel.  reads (may be NULL): per job the source pixels {x0, y0, x1, y1} its taps read.
struct resize_plan { void *block; uint32_t n, n_tiles, bpp, lds_bytes, signed_taps; const int32_t *tables; };
static int resize_upload(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst, resize_plan *plan,
                         int32_t *reads, int32_t filter = JDA_RESIZE_BILINEAR, const float *fboxes = NULL)
{
    plan->signed_taps = jda_resize_filter_signed(filter) ? 1u : 0u;      // (the signed instances: BICUBIC, LANCZOS)
    plan->block = NULL; plan->n = (uint32_t)n; plan->n_tiles = 0; plan->bpp = (uint32_t)bytes_per_pixel; plan->lds_bytes = 0; plan->tables = NULL;
    jda_resize_plan_out P;
    int rc = fboxes ? jda_resize_plan_jobs_box(n, src, bytes_per_pixel, fboxes, dst, &P, filter) : jda_resize_plan_jobs(n, src, bytes_per_pixel, rects, dst, &P, filter);
    if (rc != JDA_SUCCESS) return rc;
    const size_t jbytes = align16(P.jobs.size() * sizeof(jda_resize_job)), tbytes = P.tables.size() * sizeof(int32_t);
    uint8_t *blk = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, jbytes + align16(tbytes));
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(resize jobs)");
    rc = jda_resize_plan_place(&P, blk + jbytes);
    if (rc != JDA_SUCCESS) { jda_pool_free(ctx, blk); return rc; }
    e = hipMemcpyAsync(blk, P.jobs.data(), P.jobs.size() * sizeof(jda_resize_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(blk + jbytes, P.tables.data(), tbytes, hipMemcpyHostToDevice, ctx->stream);
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    if (e != hipSuccess) { jda_pool_free(ctx, blk); return jda_set_err(ctx, e, "resize jobs"); }
    plan->block = blk; plan->n_tiles = P.n_tiles; plan->lds_bytes = P.lds_bytes; plan->tables = (const int32_t *)(blk + jbytes);
    if (reads) memcpy(reads, P.reads.data(), P.reads.size() * sizeof(int32_t));
    return JDA_SUCCESS;
}
static int resize_launch(jda_ctx *ctx, const resize_plan &plan)
{
    const hipError_t e = jda_launch_resize((const jda_resize_job *)plan.block, plan.n, plan.n_tiles, plan.bpp, plan.signed_taps, plan.tables, plan.lds_bytes, ctx->stream);
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_resize_tiles");
}

int jda_resize_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst)
{
    return jda_resize_surfaces_ex(ctx, n, src, bytes_per_pixel, rects, dst, JDA_RESIZE_BILINEAR);
}
int jda_resize_surfaces_ex(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst,
                           int32_t filter)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0 || (bytes_per_pixel != 1 && bytes_per_pixel != 4) || filter < 0 || filter >= JDA_RESIZE_FILTERS) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!src || !dst) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    resize_plan plan;
    int rc = resize_upload(ctx, n, src, bytes_per_pixel, rects, dst, &plan, NULL, filter);
    if (rc != JDA_SUCCESS) return rc;
    return finish_surfaces(ctx, resize_launch(ctx, plan), plan.block, "jda_resize_surfaces");
}

// Pillow's resize(size, F, box = a float box): the same launch over tables made from fractional ends (jda_resize_plan_jobs_box)
int jda_resize_surfaces_box(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const float *boxes, const jda_output *dst, int32_t filter)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0 || (bytes_per_pixel != 1 && bytes_per_pixel != 4) || filter < 0 || filter >= JDA_RESIZE_FILTERS) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!src || !dst || !boxes) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    resize_plan plan;
    int rc = resize_upload(ctx, n, src, bytes_per_pixel, NULL, dst, &plan, NULL, filter, boxes);
    if (rc != JDA_SUCCESS) return rc;
    return finish_surfaces(ctx, resize_launch(ctx, plan), plan.block, "jda_resize_surfaces_box");
}

// ---- Pillow's Image.reduce (jda_reduce_tiles in jda_kernels.hip; the rule and the tile: jda_rd_* in jda_device_core.h; checks and tiles: jda_reduce_plan.h)
// Check n jobs and upload their records, and wait for them as resize_upload does; reduce_launch then queues the kernel.
struct reduce_plan { void *block; uint32_t n, n_tiles, bpp, lds_bytes; };
static int reduce_upload(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *factors, const int32_t *boxes, const jda_output *dst,
                         reduce_plan *plan)
{
    plan->block = NULL; plan->n = (uint32_t)n; plan->n_tiles = 0; plan->bpp = (uint32_t)bytes_per_pixel; plan->lds_bytes = 0;
    jda_reduce_plan_out P;
    const int rc = jda_reduce_plan_jobs(n, src, bytes_per_pixel, factors, boxes, dst, &P);
    if (rc != JDA_SUCCESS) return rc;
    const size_t jbytes = P.jobs.size() * sizeof(jda_reduce_job);
    uint8_t *blk = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, align16(jbytes));
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(reduce jobs)");
    // (the records may share no byte with a destination either: the pool hands out what no surface of the caller's holds)
    e = hipMemcpyAsync(blk, P.jobs.data(), jbytes, hipMemcpyHostToDevice, ctx->stream);
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    if (e != hipSuccess) { jda_pool_free(ctx, blk); return jda_set_err(ctx, e, "reduce jobs"); }
    plan->block = blk; plan->n_tiles = P.n_tiles; plan->lds_bytes = P.lds_bytes;
    return JDA_SUCCESS;
}
static int reduce_launch(jda_ctx *ctx, const reduce_plan &plan)
{
    const hipError_t e = jda_launch_reduce((const jda_reduce_job *)plan.block, plan.n, plan.n_tiles, plan.bpp, plan.lds_bytes, ctx->stream);
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_reduce_tiles");
}
int jda_reduce_geometry(int32_t box_w, int32_t box_h, int32_t fx, int32_t fy, int32_t *out_w, int32_t *out_h)
{
    return jda_reduce_geometry_of(box_w, box_h, fx, fy, out_w, out_h);
}
int jda_reduce_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *factors, const int32_t *boxes, const jda_output *dst)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0 || (bytes_per_pixel != 1 && bytes_per_pixel != 4)) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!src || !dst || !factors) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    reduce_plan plan;
    const int rc = reduce_upload(ctx, n, src, bytes_per_pixel, factors, boxes, dst, &plan);
    if (rc != JDA_SUCCESS) return rc;
    return finish_surfaces(ctx, reduce_launch(ctx, plan), plan.block, "jda_reduce_surfaces");
}
int jda_thumbnail_plan(int32_t src_w, int32_t src_h, int32_t req_w, int32_t req_h, int32_t filter, double reducing_gap, jda_thumbnail_steps *plan)
{
    return jda_thumbnail_plan_of(src_w, src_h, req_w, req_h, filter, reducing_gap, plan);
}

int jda_decode_to_host_resized(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *rect,
                               int32_t out_w, int32_t out_h, void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded,
                               int32_t *tiles)
{
    return jda_decode_to_host_resized_ex(ctx, jpeg, len, pixel_type, options, rect, out_w, out_h, JDA_RESIZE_BILINEAR, host_pixels, pitch_bytes, rows, mcus_decoded, tiles);
}
int jda_decode_to_host_resized_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, const int32_t *rect,
                                  int32_t out_w, int32_t out_h, int32_t filter, void *host_pixels, int32_t pitch_bytes, int32_t rows,
                                  int32_t *mcus_decoded, int32_t *tiles)
{
    if (mcus_decoded) *mcus_decoded = 0;
    if (tiles) tiles[0] = tiles[1] = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!jpeg || !host_pixels || out_w <= 0 || out_h <= 0 || filter < 0 || filter >= JDA_RESIZE_FILTERS) return JDA_INVALID_PARAMETER;
    if (pixel_type != JDA_RGB8888 && pixel_type != JDA_EIGHT_BIT_GRAYSCALE) return JDA_INVALID_PARAMETER;
    onecall F;
    int rc = oc_open(F, ctx, jpeg, len);
    if (rc != JDA_SUCCESS) return rc;
    rc = oc_geometry(F, pixel_type, options);
    const int bpp = F.bpp, ow = F.ow, oh = F.oh;
    if (rc == JDA_SUCCESS && (ow > F.cw || oh > F.ch || (int64_t)pitch_bytes < (int64_t)out_w * bpp || rows < out_h || out_w > (1 << 24) || out_h > (1 << 24))) rc = JDA_INVALID_PARAMETER;
    const int32_t whole[4] = { 0, 0, ow, oh };
    const int32_t *box = rect ? rect : whole;
    if (rc == JDA_SUCCESS && (box[0] < 0 || box[1] < 0 || box[2] <= 0 || box[3] <= 0 || (int64_t)box[0] + box[2] > ow || (int64_t)box[1] + box[3] > oh)) rc = JDA_INVALID_PARAMETER;
    // (the limits of the resize before anything is uploaded)
    { uint32_t k; if (rc == JDA_SUCCESS) rc = jda_resize_axis_ksize(box[0], box[0] + box[2], out_w, &k, filter); if (rc == JDA_SUCCESS) rc = jda_resize_axis_ksize(box[1], box[1] + box[3], out_h, &k, filter); }
    if (rc != JDA_SUCCESS) { jda_image_free(F.img); return rc; }
    const int opitch = (int)align16((size_t)out_w * bpp);
    rc = oc_upload(F, F.cbytes + (size_t)opitch * out_h, mcus_decoded);           // the decoded canvas, the resized surface behind it
    if (rc != JDA_SUCCESS) return rc;
    jda_output D;
    D.pixels = F.dsurf + F.cbytes; D.pitch_bytes = opitch; D.width_px = out_w; D.rows = out_h;
    // what has to wait for the host -- the job record and the taps -- first: the taps say which MCUs have to be decoded at all
    resize_plan plan;
    int32_t reads[4] = { 0, 0, 0, 0 }, mcu_rect[4];
    rc = resize_upload(ctx, 1, &F.S, bpp, box, &D, &plan, reads, filter);        // (reads: what the chosen filter's taps read, clipped at the visible image)
    if (rc == JDA_SUCCESS) {
        const bool all = oc_mcu_rect(F, reads, mcu_rect);
        rc = oc_plan(F, all ? NULL : mcu_rect, NULL, tiles);
        // then decode, resize and the copy back are queued back to back (the MCUs a bad stream does not reach are zeros before they are sampled)
        if (rc == JDA_SUCCESS) rc = oc_run(F, (size_t)mcu_rect[1] * F.mh * F.cpitch, (size_t)(mcu_rect[3] - mcu_rect[1]) * F.mh * F.cpitch, false);
        if (rc == JDA_SUCCESS) rc = resize_launch(ctx, plan);
        if (rc == JDA_SUCCESS) rc = copy_rows_back(ctx, host_pixels, (size_t)pitch_bytes, D.pixels, (size_t)opitch, (size_t)out_w * bpp, (size_t)out_h, true);
    }
    return oc_close(F, rc, plan.block);
}

// ---- baseline encode (jda_encode_* in jda_kernels.hip; the stages: jda_en_* in jda_device_core.h; checks, records and headers: jda_encode_plan.h)
// Two halves with the host between them: the records go up, blocks / lengths / scan run, the per-job sizes of the unstuffed scans come back
// (16 bytes a job), the scans' buffer is taken from the pool and zeroed, the records go up again with every job's place in it, and emit /
// count / scan / write run; then the files' sizes come back.  A call with an optimised job (JDA_ENCODE_OPTIMIZE) has one more step in its first
// half: behind lengths, gather counts the symbols, the histograms come back (2,176 bytes a job) and the host makes the tables, the code words
// and the headers, sends them up, and the second lengths pass writes the code lengths again before the scan sums them.
int jda_encode_bound(int32_t w, int32_t h, int32_t sampling, int32_t restart_interval, int64_t *bytes)
{
    return jda_encode_bound_bytes(w, h, sampling, restart_interval, bytes);
}
struct encode_run {
    uint8_t *a, *b; jda_en_arrays A; jda_encode_plan_out P; std::vector<jda_encode_totals> totals;
    float *stage_ms; uint32_t timed_stages;      // (the measuring hooks: stage_ms[timed_stages], and behind it the host's step between gather and the second lengths pass)
    uint32_t *hist;
    jda_rc_hook *rc;                             // a recode call (jda_recode_images): its sources in the place of the blocks stage; NULL: pixels
};
// stages [s0, s1) queued back to back; with stage_ms (the measuring hook) each between the context's two timer events, its time added to stage_ms[stage]
static hipError_t encode_stages(jda_ctx *ctx, encode_run &R, uint32_t s0, uint32_t s1)
{
    hipError_t e = hipSuccess;
    for (uint32_t s = s0; s < s1 && e == hipSuccess; s++) {
        if (R.stage_ms) e = hipEventRecord(ctx->ev_start, ctx->stream);
        if (e == hipSuccess) {
            if (s == JDA_EN_STAGE_BLOCKS && R.rc) {
                e = jda_rc_hook_launch(&R.A, *R.rc, R.P.n_blocks, ctx->stream);
            } else {
                e = s < JDA_EN_STAGES ? jda_launch_encode_stage(&R.A, s, R.P.n_blocks, R.P.n_chunks, ctx->stream)
                                      : jda_launch_huffopt_stage(&R.A, s, R.P.n_blocks, R.hist, ctx->stream);
            }
        }
        if (R.stage_ms) {
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventRecord(ctx->ev_stop, ctx->stream);
            if (e == hipSuccess) e = hipEventSynchronize(ctx->ev_stop);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop);
            if (s < R.timed_stages) R.stage_ms[s] += ms;
        }
    }
    return e;
}
// an optimised call's step between lengths and scan; rc: the plan's refusal (libjpeg's own limit), e: HIP's
static hipError_t encode_tables(jda_ctx *ctx, encode_run &R, size_t o_huff, size_t o_hdr, int *rc)
{
    jda_encode_plan_out &P = R.P;
    std::vector<uint32_t> hist((size_t)P.n_opt * JDA_EN_HUFF_DWORDS);
    hipError_t e = encode_stages(ctx, R, JDA_EN_STAGE_GATHER, JDA_EN_STAGE_GATHER + 1u);
    const auto t0 = std::chrono::steady_clock::now();
    if (e == hipSuccess) e = hipMemcpyAsync(hist.data(), R.hist, hist.size() * 4, hipMemcpyDeviceToHost, ctx->stream);
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    if (e != hipSuccess) return e;
    *rc = jda_encode_plan_tables(&P, hist.data());
    if (*rc != JDA_SUCCESS) return hipSuccess;
    e = hipMemcpyAsync(R.a + o_huff + (size_t)JDA_EN_HUFF_DWORDS * 4, P.huff.data() + JDA_EN_HUFF_DWORDS, (size_t)P.n_opt * JDA_EN_HUFF_DWORDS * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_hdr, P.hdr.data(), P.hdr.size(), hipMemcpyHostToDevice, ctx->stream);
    if (R.stage_ms && R.timed_stages == JDA_EN_STAGES_OPT) R.stage_ms[JDA_EN_STAGES_OPT] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (e == hipSuccess) e = encode_stages(ctx, R, JDA_EN_STAGE_OPT_LENGTHS, JDA_EN_STAGE_OPT_LENGTHS + 1u);
    return e;
}
static int encode_lengths(jda_ctx *ctx, encode_run &R)
{
    jda_encode_plan_out &P = R.P;
    const size_t n = P.jobs.size(), nb = P.n_blocks;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_jobs = take(n * sizeof(jda_encode_dev_job)), o_quant = take(P.quant.size() * sizeof(jda_encode_quant)), o_huff = take(P.huff.size() * 4), o_hdr = take(P.hdr.size());
    const size_t o_coef = take(nb * 128), o_meta = take(nb * 4), o_code = take(nb * 4), o_end = take(nb * 8), o_ist = take((size_t)P.n_int * 8), o_tot = take(n * sizeof(jda_encode_totals));
    const size_t o_hist = take((size_t)P.n_opt * JDA_EN_HUFF_DWORDS * 4);
    const size_t o_rsrc = take(R.rc ? n * sizeof(jda_rc_src) : 0), o_bad = take(R.rc ? n * 4 : 0), o_xf = take(R.rc ? R.rc->xf.size() * sizeof(jda_rc_xf) : 0);
    hipError_t e = jda_pool_alloc(ctx, (void **)&R.a, off);
    if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc(encode scratch)"); return JDA_ERROR_MEMORY; }
    jda_en_arrays &A = R.A;
    memset(&A, 0, sizeof(A));
    A.jobs = (const jda_encode_dev_job *)(R.a + o_jobs); A.quant = (const jda_encode_quant *)(R.a + o_quant); A.huff = (const uint32_t *)(R.a + o_huff); A.hdr = R.a + o_hdr;
    A.coef = (int16_t *)(R.a + o_coef); A.meta = (uint32_t *)(R.a + o_meta); A.code = (uint32_t *)(R.a + o_code); A.end = (uint64_t *)(R.a + o_end);
    A.istart = (uint64_t *)(R.a + o_ist); A.totals = (jda_encode_totals *)(R.a + o_tot); A.n_jobs = (uint32_t)n;
    R.hist = (uint32_t *)(R.a + o_hist);
    e = hipMemcpyAsync(R.a + o_jobs, P.jobs.data(), n * sizeof(jda_encode_dev_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_quant, P.quant.data(), P.quant.size() * sizeof(jda_encode_quant), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_huff, P.huff.data(), P.huff.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_hdr, P.hdr.data(), P.hdr.size(), hipMemcpyHostToDevice, ctx->stream);
    if (R.rc) {
        R.rc->d_src = (jda_rc_src *)(R.a + o_rsrc); R.rc->d_bad = (uint32_t *)(R.a + o_bad);
        if (e == hipSuccess) e = hipMemcpyAsync(R.rc->d_src, R.rc->src.data(), n * sizeof(jda_rc_src), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(R.rc->d_bad, 0, n * 4, ctx->stream);
        R.rc->d_xf = (jda_rc_xf *)(R.a + o_xf);
        if (e == hipSuccess && !R.rc->xf.empty()) e = hipMemcpyAsync(R.rc->d_xf, R.rc->xf.data(), R.rc->xf.size() * sizeof(jda_rc_xf), hipMemcpyHostToDevice, ctx->stream);
    }
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }      // (the records are on the stack of this call)
    if (P.n_opt) {                                                                                     // (the pool hands out what earlier calls left in it)
        if (e == hipSuccess) e = hipMemsetAsync(R.hist, 0, (size_t)P.n_opt * JDA_EN_HUFF_DWORDS * 4, ctx->stream);
        if (e == hipSuccess) e = encode_stages(ctx, R, JDA_EN_STAGE_BLOCKS, JDA_EN_STAGE_SCAN_BITS);
        int rc = JDA_SUCCESS;
        if (e == hipSuccess) e = encode_tables(ctx, R, o_huff, o_hdr, &rc);
        if (rc != JDA_SUCCESS) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        if (e == hipSuccess) e = encode_stages(ctx, R, JDA_EN_STAGE_SCAN_BITS, JDA_EN_STAGE_EMIT);
    } else if (e == hipSuccess) e = encode_stages(ctx, R, JDA_EN_STAGE_BLOCKS, JDA_EN_STAGE_EMIT);
    R.totals.resize(n);
    if (e == hipSuccess) e = hipMemcpyAsync(R.totals.data(), A.totals, n * sizeof(jda_encode_totals), hipMemcpyDeviceToHost, ctx->stream);
    if (R.rc) { R.rc->bad.assign(n, 0u); if (e == hipSuccess) e = hipMemcpyAsync(R.rc->bad.data(), R.rc->d_bad, n * 4, hipMemcpyDeviceToHost, ctx->stream); }
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    if (R.rc) for (size_t i = 0; i < n; i++) if (R.rc->bad[i]) P.jobs[i].capacity = 0;      // a block out of range: no byte of the job's file is written (encode_files sends the records up again)
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_encode_lengths");
}
static int encode_files(jda_ctx *ctx, encode_run &R)
{
    jda_encode_plan_out &P = R.P;
    const size_t n = P.jobs.size();
    int rc = jda_encode_plan_place(&P, R.totals.data());
    if (rc != JDA_SUCCESS) return rc;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_u = take((size_t)P.u_total), o_cnt = take((size_t)P.n_chunks * 4), o_end = take((size_t)P.n_chunks * 8);
    hipError_t e = jda_pool_alloc(ctx, (void **)&R.b, off);
    if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc(encode streams)"); return JDA_ERROR_MEMORY; }
    R.A.u = R.b + o_u; R.A.ffcnt = (uint32_t *)(R.b + o_cnt); R.A.ffend = (uint64_t *)(R.b + o_end);
    e = hipMemsetAsync(R.A.u, 0, (size_t)P.u_total, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((void *)R.A.jobs, P.jobs.data(), n * sizeof(jda_encode_dev_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = encode_stages(ctx, R, JDA_EN_STAGE_EMIT, JDA_EN_STAGES);
    if (e == hipSuccess) e = hipMemcpyAsync(R.totals.data(), R.A.totals, n * sizeof(jda_encode_totals), hipMemcpyDeviceToHost, ctx->stream);
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_encode_files");
}

static int encode_call(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, const uint32_t *job_flags,
                       void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status, float *stage_ms, uint32_t timed_stages)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0 || (bytes_per_pixel != 1 && bytes_per_pixel != 4)) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!src || !jobs || !dst || !dst_capacity || !dst_bytes || !status) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    encode_run R;
    R.a = R.b = NULL; R.stage_ms = stage_ms; R.timed_stages = timed_stages; R.hist = NULL; R.rc = NULL;
    int rc = jda_encode_plan_jobs_ex(n, src, bytes_per_pixel, jobs, job_flags, dst, dst_capacity, &R.P);
    if (rc != JDA_SUCCESS) return rc;
    rc = encode_lengths(ctx, R);
    if (rc == JDA_SUCCESS) rc = encode_files(ctx, R);
    if (R.b) jda_pool_free(ctx, R.b);
    if (R.a) jda_pool_free(ctx, R.a);
    if (rc != JDA_SUCCESS) return rc;
    for (int i = 0; i < n; i++) {
        dst_bytes[i] = (int64_t)R.totals[(size_t)i].file_bytes;
        status[i] = R.totals[(size_t)i].file_bytes > (uint64_t)dst_capacity[i] ? JDA_ERROR_MEMORY : JDA_SUCCESS;
    }
    return JDA_SUCCESS;
}
int jda_encode_surfaces(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs,
                        void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status)
{
    return encode_call(ctx, n, src, bytes_per_pixel, jobs, NULL, dst, dst_capacity, dst_bytes, status, NULL, 0u);
}
int jda_encode_surfaces_ex(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, const uint32_t *job_flags,
                           void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status)
{
    return encode_call(ctx, n, src, bytes_per_pixel, jobs, job_flags, dst, dst_capacity, dst_bytes, status, NULL, 0u);
}
// Measuring hook of tools/encode_bench.py (not part of the public header): jda_encode_surfaces with every one of its seven launches between
// the context's two timer events on its stream; stage_ms[JDA_EN_STAGES] (order: JDA_EN_STAGE_*) is ADDED to, so the caller zeroes it.
int jda_internal_encode_time(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs,
                             void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status, float *stage_ms)
{
    if (!stage_ms) return JDA_INVALID_PARAMETER;
    return encode_call(ctx, n, src, bytes_per_pixel, jobs, NULL, dst, dst_capacity, dst_bytes, status, stage_ms, JDA_EN_STAGES);
}
// .. and of its --optimize leg: jda_encode_surfaces_ex timed the same way; stage_ms[JDA_EN_STAGES_OPT + 1]: the nine launches (ids 7 and 8: gather and
// the second lengths pass) and, last, the host's wall time between them -- the histograms' copy, the wait, the tables, their upload.
int jda_internal_encode_time_ex(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, const uint32_t *job_flags,
                                void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status, float *stage_ms)
{
    if (!stage_ms) return JDA_INVALID_PARAMETER;
    return encode_call(ctx, n, src, bytes_per_pixel, jobs, job_flags, dst, dst_capacity, dst_bytes, status, stage_ms, JDA_EN_STAGES_OPT);
}

// ---- lossless recode (jda_rc_* in jda_kernels.hip and jda_device_core.h; checks, records and headers: jda_recode_plan.h): the
// encoder's calls as they stand with the sources' own coefficients in the place of the blocks stage.  The jobs' range words come back with
// the totals (a progressive call: with the symbol counts); a job whose word is set is refused and its record sent up again with capacity 0.
int jda_recode_bound(const jda_image_info *info, int32_t form, int32_t restart_interval, int64_t *bytes)
{
    return jda_recode_bound_bytes(info, form, restart_interval, bytes);
}
static void recode_host_of(const jda_recode_source &S, jda_recode_src_host *H)
{
    memset(H, 0, sizeof(*H));
    if (S.image) {
        const jda_dev_image *d = S.image;
        H->kind = JDA_RC_IMAGE; H->info = d->info; H->adobe = d->adobe; H->n_mcus_ok = d->n_mcus_ok;
        for (int c = 0; c < 3; c++) { H->q_id[c] = d->q_id[c]; memcpy(H->quant[c], d->quant_zz[d->q_id[c] & 3], sizeof(H->quant[c])); }
        H->dev.scan = d->base + d->off_scan; H->dev.blk_index = (const uint32_t *)(d->base + d->off_index); H->dev.blk_dc = (const int16_t *)(d->base + d->off_dc);
        H->dev.tables = d->base + d->off_tables; H->dev.scan_len = d->scan_len;
        for (int c = 0; c < 3; c++) H->dev.ac_id[c] = d->ac_id[c];
    } else {
        const jda_dev_coef *d = S.coef;
        H->kind = d->form == JDA_COEF_DENSE ? JDA_RC_COEF : JDA_RC_SPARSE; H->info = d->info; H->adobe = d->adobe;
        memcpy(H->quant, d->raw_quant, sizeof(H->quant)); memcpy(H->q_id, d->raw_qid, 3);
        H->dev.coef = (const int16_t *)(d->base + d->off_entries);
    }
}
static int recode_call(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_recode_job *jobs, const jda_recode_xform *xforms,
                       void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status, float *stage_ms)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!src || !jobs || !dst || !dst_capacity || !dst_bytes || !status) return JDA_INVALID_PARAMETER;
    for (int i = 0; i < n; i++) if ((src[i].image != NULL) == (src[i].coef != NULL)) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    std::vector<jda_recode_src_host> hosts((size_t)n);
    for (int i = 0; i < n; i++) recode_host_of(src[i], &hosts[(size_t)i]);
    jda_recode_plan_out plan;
    for (int i = 0; i < n; i++) dst_bytes[i] = 0;
    int rc = jda_recode_plan_jobs_ex(n, hosts.data(), jobs, xforms, dst, dst_capacity, status, &plan);
    if (rc != JDA_SUCCESS || plan.src.empty()) return rc;
    jda_rc_hook hook;
    hook.xf = plan.xf; hook.d_xf = NULL;
    hook.src = plan.src; hook.any_image = plan.any_image; hook.any_coef = plan.any_coef; hook.d_src = NULL; hook.d_bad = NULL;
    std::vector<jda_encode_totals> totals;
    if (plan.progressive) rc = stage_ms ? JDA_INVALID_PARAMETER : jda_progenc_recode(ctx, plan.P, hook, totals);
    else {
        encode_run R;
        R.a = R.b = NULL; R.stage_ms = stage_ms; R.timed_stages = stage_ms ? JDA_EN_STAGES_OPT : 0u; R.hist = NULL; R.rc = &hook;
        R.P = std::move(plan.P.B);
        rc = encode_lengths(ctx, R);
        if (rc == JDA_SUCCESS) rc = encode_files(ctx, R);
        if (rc != JDA_SUCCESS) (void)hipStreamSynchronize(ctx->stream);
        if (R.b) jda_pool_free(ctx, R.b);
        if (R.a) jda_pool_free(ctx, R.a);
        totals = R.totals;
    }
    if (rc != JDA_SUCCESS) return rc;
    for (size_t k = 0; k < plan.job_of.size(); k++) {
        const int i = plan.job_of[k];
        if (hook.bad[k]) { status[i] = JDA_UNSUPPORTED_FEATURE; continue; }
        dst_bytes[i] = (int64_t)totals[k].file_bytes;
        status[i] = totals[k].file_bytes > (uint64_t)dst_capacity[i] ? JDA_ERROR_MEMORY : JDA_SUCCESS;
    }
    return JDA_SUCCESS;
}
int jda_recode_images(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_recode_job *jobs,
                      void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status)
{
    return recode_call(ctx, n, src, jobs, NULL, dst, dst_capacity, dst_bytes, status, NULL);
}
// ---- .. with a flip, a turn, a transposition or an MCU crop a job: the plan resolves every job's jda_recode_xform into a
// record for jda_rc_extract_xf / jda_rc_from_coef_xf and writes the headers of the turned shape; a call without any runs as above
int jda_recode_geometry(const jda_image_info *info, const jda_recode_xform *xform, jda_image_info *out) { return jda_recode_geometry_of(info, xform, out); }
int jda_recode_bound_ex(const jda_image_info *info, const jda_recode_xform *xform, int32_t form, int32_t restart_interval, int64_t *bytes)
{
    return jda_recode_bound_bytes_ex(info, xform, form, restart_interval, bytes);
}
int jda_recode_images_ex(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_recode_job *jobs, const jda_recode_xform *xforms,
                         void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status)
{
    return recode_call(ctx, n, src, jobs, xforms, dst, dst_capacity, dst_bytes, status, NULL);
}
// Measuring hook of tools/recode_bench.py --transform: jda_internal_recode_time with a jda_recode_xform a job
int jda_internal_recode_time_ex(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_recode_job *jobs, const jda_recode_xform *xforms,
                                void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status, float *stage_ms)
{
    if (!stage_ms) return JDA_INVALID_PARAMETER;
    return recode_call(ctx, n, src, jobs, xforms, dst, dst_capacity, dst_bytes, status, stage_ms);
}
// Measuring hook of tools/recode_bench.py (not part of the public header): a call of baseline or optimised jobs with every one of its launches
// between the context's two timer events; stage_ms[JDA_EN_STAGES_OPT + 1] as jda_internal_encode_time_ex fills it -- entry 0, the blocks stage's,
// is the recode stage's here (jda_rc_extract and / or jda_rc_from_coef) -- is ADDED to, so the caller zeroes it.
int jda_internal_recode_time(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_recode_job *jobs,
                             void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status, float *stage_ms)
{
    if (!stage_ms) return JDA_INVALID_PARAMETER;
    return recode_call(ctx, n, src, jobs, NULL, dst, dst_capacity, dst_bytes, status, stage_ms);
}
// A file made a resident source of the exact road or of a recode for the length of one call: a progressive file (every scan is what libjpeg
// decodes: no option bit) or, with four, a four-component one as a coefficient image in the form `coef_form` makes resident (JDA_COEF_*),
// anything else as a baseline image.  open: JDA_SUCCESS and S set, or the reason; close frees whatever open made.
struct exact_resident {
    jda_image *img; jda_coef_image *cimg; jda_dev_image *dimg; jda_dev_coef *dcoef; jda_recode_source S;
    exact_resident() : img(NULL), cimg(NULL), dimg(NULL), dcoef(NULL) { S.image = NULL; S.coef = NULL; }
    int open(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, bool progressive, bool four, int32_t coef_form)
    {
        int32_t err = JDA_SUCCESS;
        if (progressive || four) {
            cimg = four ? jda_coef_prepare(jpeg, len, &err) : jda_progressive_prepare(jpeg, len, &err);
            if (cimg) dcoef = jda_coef_upload_ex(ctx, cimg, coef_form, &err);
            S.coef = dcoef;
        } else {
            img = jda_prepare(jpeg, len, &err);
            if (img) dimg = jda_upload(ctx, img, &err);
            S.image = dimg;
        }
        return (S.image || S.coef) ? JDA_SUCCESS : (err != JDA_SUCCESS ? err : JDA_DECODE_ERROR);
    }
    void close(jda_ctx *ctx)
    {
        if (dimg) jda_dev_image_free(ctx, dimg);
        if (dcoef) jda_dev_coef_free(ctx, dcoef);
        if (img) jda_image_free(img);
        if (cimg) jda_coef_image_free(cimg);
    }
};
int jda_recode_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t form, int32_t restart_interval, void *host_file, int64_t capacity, int64_t *file_bytes)
{
    return jda_recode_to_host_ex(ctx, jpeg, len, form, restart_interval, NULL, host_file, capacity, file_bytes);
}
int jda_recode_to_host_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t form, int32_t restart_interval, const jda_recode_xform *xform, void *host_file, int64_t capacity,
                          int64_t *file_bytes)
{
    if (file_bytes) *file_bytes = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!jpeg || !host_file || !file_bytes || capacity < 0) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    jda_image_info I;
    int rc = jda_parse(jpeg, len, &I);
    if (rc != JDA_SUCCESS) return rc;
    int64_t bound = 0;
    rc = jda_recode_bound_bytes_ex(&I, xform, form, restart_interval, &bound);
    if (rc != JDA_SUCCESS) return rc;
    exact_resident R;
    rc = R.open(ctx, jpeg, len, I.jpeg_type == 1, false, JDA_COEF_DENSE);
    const int64_t fcap = std::min(capacity, bound);                                        // (no file is longer than the bound)
    void *dfile = NULL;
    if (rc == JDA_SUCCESS) {
        const hipError_t e = jda_pool_alloc(ctx, &dfile, (size_t)fcap + 16);
        if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc(recoded file)"); rc = JDA_ERROR_MEMORY; }
    }
    if (rc == JDA_SUCCESS) {
        const jda_recode_job J = { form, restart_interval, 0, 0 };
        int32_t st = JDA_SUCCESS;
        rc = jda_recode_images_ex(ctx, 1, &R.S, &J, xform, &dfile, &fcap, file_bytes, &st);
        if (rc == JDA_SUCCESS) rc = st;
        if (rc == JDA_SUCCESS) {
            hipError_t e = hipMemcpyAsync(host_file, dfile, (size_t)*file_bytes, hipMemcpyDeviceToHost, ctx->stream);
            { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
            if (e != hipSuccess) rc = jda_set_err(ctx, e, "copy back");
        }
    }
    if (dfile) jda_pool_free(ctx, dfile);
    R.close(ctx);
    return rc;
}

// ---- libjpeg-exact decode (jda_exact_* in jda_kernels.hip, jda_ex_* in jda_device_core.h).  Everything a call
// decides is the plan's (jda_exact_plan.h: jda_exact_plan_build before the call has device memory, jda_exact_plan_place once it knows where
// its block lies): what is refused, the images' planes in the scratch, their records, the tile lists and the launches over them.  Here:
// the sources as the plan reads them, one pool block a call (the plan's blob, behind it the scratch), one copy of the blob, the plan's
// launches in their order, the planes copied out (jda_exact_decode_planes*), the wait.
// scales: NULL: all 1; flags: the _ex calls' (JDA_EXACT_COLOUR_MODELS; planes then has four entries an image, planes[4 i + c], else three);
// rects: jda_exact_decode_surfaces_rect's, NULL: none.
static void exact_view_coef(const jda_dev_coef *d, jda_exact_source *V)
{
    memset(V, 0, sizeof(*V));
    V->kind = d->form == JDA_COEF_SPARSE ? JDA_EXK_PLANES_SPARSE : JDA_EXK_PLANES_DENSE;
    V->info = d->info; V->adobe = d->adobe; V->colour = d->colour;
    memcpy(V->quant, d->raw_quant, sizeof(V->quant));
    V->tables = d->base; V->scan = d->base + d->off_entries;
}
static void exact_view_image(const jda_dev_image *d, jda_exact_source *V)
{
    memset(V, 0, sizeof(*V));
    V->kind = JDA_EXK_PLANES_BASELINE;
    V->info = d->info; V->adobe = d->adobe; V->colour = d->colour; V->n_mcus_ok = d->n_mcus_ok;
    for (int c = 0; c < 3; c++) { memcpy(V->quant[c], d->quant_zz[d->q_id[c] & 3], sizeof(V->quant[c])); V->ac_id[c] = d->ac_id[c]; }
    V->tables = d->base + d->off_tables; V->scan = d->base + d->off_scan; V->scan_len = d->scan_len;
    V->index = (const uint32_t *)(d->base + d->off_index); V->dc = (const int16_t *)(d->base + d->off_dc);
}
// stage_ms (the measuring hook's, else NULL): [0] the planes launches, [1] the colour launches
static int exact_call(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, const jda_output *planes,
                      int32_t *status, float *stage_ms = NULL, const int32_t *scales = NULL, uint32_t flags = 0, const int32_t *rects = NULL)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!src || !status || (!outputs && !planes)) return JDA_INVALID_PARAMETER;
    for (int i = 0; i < n; i++) if ((src[i].image != NULL) == (src[i].coef != NULL)) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    std::vector<jda_exact_source> views(flags ? 2u * (size_t)n : (size_t)n);      // (image i; with flags at n + i component 3 of a four-component one)
    for (int i = 0; i < n; i++) {
        jda_exact_source &V = views[(size_t)i];
        if (src[i].image) { exact_view_image(src[i].image, &V); continue; }
        exact_view_coef(src[i].coef, &V);
        if (flags && src[i].coef->k) { V.k = &views[(size_t)n + (size_t)i]; exact_view_coef(src[i].coef->k, &views[(size_t)n + (size_t)i]); }
    }
    jda_exact_plan plan;
    const int rc = jda_exact_plan_build(n, views.data(), outputs, pixel_types, planes, scales, flags, rects, status, &plan);
    if (rc != JDA_SUCCESS || !plan.n_planned) return rc;
    uint8_t *blk = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, plan.o_scratch + plan.scratch);
    if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc(exact decode)"); return JDA_ERROR_MEMORY; }
    jda_exact_plan_place(&plan, blk);
    e = hipMemcpyAsync(blk, plan.blob.data(), plan.blob.size(), hipMemcpyHostToDevice, ctx->stream);
    hipEvent_t ev[3] = { NULL, NULL, NULL };
    for (int k = 0; k < 3 && stage_ms && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
    if (stage_ms && e == hipSuccess) e = hipEventRecord(ev[0], ctx->stream);
    for (size_t k = 0; k <= plan.launches.size() && e == hipSuccess; k++) {
        if (k == plan.colour_begin && stage_ms) e = hipEventRecord(ev[1], ctx->stream);
        if (k < plan.launches.size() && e == hipSuccess)
            e = jda_launch_exact(plan.launches[k], (const jda_dev_desc *)blk, (const jda_ex_desc *)(blk + plan.o_ex), (const jda_ex_src *)(blk + plan.o_src),
                                 (const jda_exr_rec *)(blk + plan.o_rect), (const jda_strip *)(blk + plan.launches[k].off), ctx->stream);
    }
    if (stage_ms && e == hipSuccess) e = hipEventRecord(ev[2], ctx->stream);
    const int ps = flags ? 4 : 3;                                // entries an image in planes
    for (int i = 0; i < n && e == hipSuccess && planes; i++) {
        const jda_exact_image &M = plan.images[(size_t)i];
        if (M.kind < 0) continue;
        for (int c = 0; c < (M.four ? 4 : M.info.ncomp == 3 ? 3 : 1) && e == hipSuccess; c++) {
            const jda_output &P = planes[ps * i + c];
            const int32_t ew = c == 3 ? (int32_t)M.G.kw : c ? (int32_t)M.G.cw : (int32_t)M.G.w, eh = c == 3 ? (int32_t)M.G.kh : c ? (int32_t)M.G.ch : (int32_t)M.G.h;
            const size_t cw = (size_t)(P.width_px < ew ? P.width_px : ew), crows = (size_t)(P.rows < eh ? P.rows : eh);
            if (cw && crows)
                e = hipMemcpy2DAsync(P.pixels, (size_t)P.pitch_bytes, blk + plan.o_scratch + M.plane_at + (c == 3 ? M.G.off_k : M.G.off[c]), c == 3 ? M.G.pitch_k : c ? M.G.pitch_c : M.G.pitch_y, cw, crows,
                                     hipMemcpyDeviceToDevice, ctx->stream);
        }
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);     // (the blob leaves pageable memory that goes away with this frame)
    for (int k = 0; k < 2 && stage_ms && e == hipSuccess && es == hipSuccess; k++) e = hipEventElapsedTime(&stage_ms[k], ev[k], ev[k + 1]);
    for (int k = 0; k < 3; k++) if (ev[k]) (void)hipEventDestroy(ev[k]);
    jda_pool_free(ctx, blk);
    if (e != hipSuccess) return jda_set_err(ctx, e, "jda_exact_decode");
    return es == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, es, "jda_exact_decode");
}
int jda_exact_decode_surfaces(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, int32_t *status)
{
    if (ctx && n > 0 && !outputs) return JDA_INVALID_PARAMETER;
    return exact_call(ctx, n, src, outputs, pixel_types, NULL, status);
}
// Measuring hook of tools/exact_bench.py (not part of the public header): jda_exact_decode_surfaces with its launches between events of the
// call's own; stage_ms[2]: the jda_exact_planes launches, the jda_exact_colour launches
int jda_internal_exact_time(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, int32_t *status, float *stage_ms)
{
    if (!stage_ms || (ctx && n > 0 && !outputs)) return JDA_INVALID_PARAMETER;
    stage_ms[0] = stage_ms[1] = 0.f;
    return exact_call(ctx, n, src, outputs, pixel_types, NULL, status, stage_ms);
}
int jda_exact_decode_planes(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *planes, int32_t *status)
{
    if (ctx && n > 0 && !planes) return JDA_INVALID_PARAMETER;
    return exact_call(ctx, n, src, NULL, NULL, planes, status);
}
// ---- the same at 1/2, 1/4 and 1/8
int jda_exact_scaled_geometry(const jda_image_info *info, int32_t scale, int32_t *out_w, int32_t *out_h, int32_t *comp_w, int32_t *comp_h)
{
    if (!info) return JDA_INVALID_PARAMETER;
    // (the layout checks of the decode calls: what they refuse has no geometry here either -- four components: JDA_UNSUPPORTED_FEATURE)
    int rc = jda_exact_check(*info, 0, JDA_RGB8888, 0, 0);
    if (rc != JDA_SUCCESS) return rc;
    jda_exact_geo G;
    rc = jda_exact_geometry_scaled(*info, false, scale, &G);
    if (rc != JDA_SUCCESS) return rc;
    if (out_w) *out_w = (int32_t)G.w;
    if (out_h) *out_h = (int32_t)G.h;
    for (int c = 0; c < 3; c++) {
        const bool there = c < info->ncomp;
        if (comp_w) comp_w[c] = there ? (int32_t)(c ? G.cw : G.w) : 0;
        if (comp_h) comp_h[c] = there ? (int32_t)(c ? G.ch : G.h) : 0;
    }
    return JDA_SUCCESS;
}
int jda_exact_draft_scale(const jda_image_info *info, int32_t req_w, int32_t req_h)
{
    return info ? jda_exact_draft(*info, req_w, req_h) : 1;
}
int jda_exact_decode_surfaces_scaled(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, const int32_t *scales,
                                     int32_t *status)
{
    if (ctx && n > 0 && !outputs) return JDA_INVALID_PARAMETER;
    return exact_call(ctx, n, src, outputs, pixel_types, NULL, status, NULL, scales);
}
int jda_exact_decode_planes_scaled(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *planes, const int32_t *scales, int32_t *status)
{
    if (ctx && n > 0 && !planes) return JDA_INVALID_PARAMETER;
    return exact_call(ctx, n, src, NULL, NULL, planes, status, NULL, scales);
}
int jda_exact_decode_surfaces_ex(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, const int32_t *scales,
                                 uint32_t flags, int32_t *status)
{
    if (flags & ~(uint32_t)JDA_EXACT_COLOUR_MODELS) return JDA_INVALID_PARAMETER;
    if (ctx && n > 0 && !outputs) return JDA_INVALID_PARAMETER;
    return exact_call(ctx, n, src, outputs, pixel_types, NULL, status, NULL, scales, flags);
}
int jda_exact_decode_planes_ex(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *planes, const int32_t *scales, uint32_t flags, int32_t *status)
{
    if (flags & ~(uint32_t)JDA_EXACT_COLOUR_MODELS) return JDA_INVALID_PARAMETER;
    if (ctx && n > 0 && !planes) return JDA_INVALID_PARAMETER;
    return exact_call(ctx, n, src, NULL, NULL, planes, status, NULL, scales, flags);
}
// The source rectangle {x0, y0, x1, y1} (half open) the taps of `filter` read when rect = {x, y, w, h} of a src_w x src_h image is resized
// to out_w x out_h, clipped at the image: resize_upload's `reads`, host work only (what decode_to_tensors decodes of a cropped file)
int jda_resize_reads(int32_t src_w, int32_t src_h, const int32_t *rect, int32_t out_w, int32_t out_h, int32_t filter, int32_t *reads)
{
    if (!rect || !reads || src_w <= 0 || src_h <= 0 || out_w <= 0 || out_h <= 0 || out_w > (1 << 24) || out_h > (1 << 24)) return JDA_INVALID_PARAMETER;
    if (rect[0] < 0 || rect[1] < 0 || rect[2] <= 0 || rect[3] <= 0 || (int64_t)rect[0] + rect[2] > src_w || (int64_t)rect[1] + rect[3] > src_h) return JDA_INVALID_PARAMETER;
    for (int a = 0; a < 2; a++) {
        const int32_t in_size = a ? src_h : src_w, in0 = rect[a], in1 = rect[a] + rect[2 + a], out = a ? out_h : out_w;
        uint32_t ksize = 0;
        int rc = jda_resize_axis_ksize(in0, in1, out, &ksize, filter);
        if (rc != JDA_SUCCESS) return rc;
        std::vector<int32_t> tab((size_t)out * (2u + ksize));
        rc = jda_resize_axis_taps(in_size, in0, in1, out, ksize, tab.data(), filter);
        if (rc != JDA_SUCCESS) return rc;
        reads[a] = tab[0]; reads[2 + a] = tab[2 * (size_t)(out - 1)] + tab[2 * (size_t)(out - 1) + 1];
    }
    return JDA_SUCCESS;
}
// ---- a pixel rectangle an image
int jda_exact_decode_surfaces_rect(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, const int32_t *scales,
                                   uint32_t flags, const int32_t *rects, int32_t *status)
{
    if (flags & ~(uint32_t)JDA_EXACT_COLOUR_MODELS) return JDA_INVALID_PARAMETER;
    if (ctx && n > 0 && !outputs) return JDA_INVALID_PARAMETER;
    return exact_call(ctx, n, src, outputs, pixel_types, NULL, status, NULL, scales, flags, rects);
}
// the measuring hook with rectangles (tools/exact_bench.py --rect): stage_ms[1] holds every colour launch, jda_exact_colour_rect among them
int jda_internal_exact_time_rect(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, const int32_t *scales,
                                 uint32_t flags, const int32_t *rects, int32_t *status, float *stage_ms)
{
    if (!stage_ms || (flags & ~(uint32_t)JDA_EXACT_COLOUR_MODELS) || (ctx && n > 0 && !outputs)) return JDA_INVALID_PARAMETER;
    stage_ms[0] = stage_ms[1] = 0.f;
    return exact_call(ctx, n, src, outputs, pixel_types, NULL, status, stage_ms, scales, flags, rects);
}
int jda_exact_rect_mcus(const jda_image_info *info, int32_t scale, int32_t pixel_type, const int32_t *rect, int32_t *mcu_rect)
{
    if (!info || !rect || !mcu_rect) return JDA_INVALID_PARAMETER;
    int rc = jda_exact_check(*info, 0, pixel_type, 0, 0);
    if (rc != JDA_SUCCESS) return rc;
    jda_exact_geo G;
    const bool luma_only = pixel_type == JDA_EIGHT_BIT_GRAYSCALE && info->ncomp == 3;
    rc = jda_exact_geometry_scaled(*info, luma_only, scale, &G);
    if (rc != JDA_SUCCESS) return rc;
    return jda_exact_rect_plan(*info, G, luma_only, rect, mcu_rect);
}
// the measuring hook of the _ex calls (tools/exact_adobe_bench.py): stage_ms[0] the planes launches (K's gray tiles among them), stage_ms[1]
// the colour launches (jda_exact_colour4, the RGB instances)
int jda_internal_exact_time_ex(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, const int32_t *scales,
                               uint32_t flags, int32_t *status, float *stage_ms)
{
    if (!stage_ms || (flags & ~(uint32_t)JDA_EXACT_COLOUR_MODELS) || (ctx && n > 0 && !outputs)) return JDA_INVALID_PARAMETER;
    stage_ms[0] = stage_ms[1] = 0.f;
    return exact_call(ctx, n, src, outputs, pixel_types, NULL, status, stage_ms, scales, flags);
}
// the measuring hook with a scale an image (tools/exact_bench.py --scale)
int jda_internal_exact_time_scaled(jda_ctx *ctx, int32_t n, const jda_recode_source *src, const jda_output *outputs, const int32_t *pixel_types, const int32_t *scales,
                                   int32_t *status, float *stage_ms)
{
    if (!stage_ms || (ctx && n > 0 && !outputs)) return JDA_INVALID_PARAMETER;
    stage_ms[0] = stage_ms[1] = 0.f;
    return exact_call(ctx, n, src, outputs, pixel_types, NULL, status, stage_ms, scales);
}
// rect (NULL or all zero: the whole image): the surface and the host rows hold the rectangle; tiles (may be NULL): [0] the planes-stage tiles
// launched, [1] those of the whole image
static int exact_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t scale, uint32_t flags, const int32_t *rect, void *host_pixels,
                         int32_t pitch_bytes, int32_t rows, int32_t *tiles)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (flags & ~(uint32_t)JDA_EXACT_COLOUR_MODELS) return JDA_INVALID_PARAMETER;
    if (!jpeg || !host_pixels || pitch_bytes < 0 || rows < 0) return JDA_INVALID_PARAMETER;
    if (pixel_type != JDA_RGB8888 && pixel_type != JDA_EIGHT_BIT_GRAYSCALE && !(flags && pixel_type == JDA_CMYK8888)) return JDA_INVALID_PARAMETER;
    if (!jda_exact_scale_ok(scale)) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    jda_image_info I;
    int rc = jda_parse(jpeg, len, &I);
    // with the flag a four-component file of any SOF type goes the progressive files' way, through jda_coef_prepare (which takes SOF1 too)
    bool four = false;
    if (flags) {
        jda_exact_file E;
        const int prc = jda_exact_probe(jpeg, len, &E);
        if (E.ncomp == 4) {
            if (prc != JDA_SUCCESS) return prc;
            four = true;
            if (rc != JDA_SUCCESS) { memset(&I, 0, sizeof(I)); I.width = E.width; I.height = E.height; I.ncomp = 4; rc = JDA_SUCCESS; }
            if (scale != 1) return JDA_UNSUPPORTED_FEATURE;
            if (pixel_type == JDA_EIGHT_BIT_GRAYSCALE) return JDA_UNSUPPORTED_FEATURE;
        }
    }
    if (rc != JDA_SUCCESS) return rc;
    if (pixel_type == JDA_CMYK8888 && !four) return JDA_INVALID_PARAMETER;
    int32_t ow = (I.width + scale - 1) / scale, oh = (I.height + scale - 1) / scale;      // (at scale 1 the file's own size)
    const bool has_rect = rect && (rect[0] || rect[1] || rect[2] || rect[3]);
    if (has_rect) {
        if (four) return JDA_UNSUPPORTED_FEATURE;
        if (rect[0] < 0 || rect[1] < 0 || rect[2] < 1 || rect[3] < 1 || (int64_t)rect[0] + rect[2] > ow || (int64_t)rect[1] + rect[3] > oh) return JDA_INVALID_PARAMETER;
        ow = rect[2]; oh = rect[3];
    }
    if (tiles) {
        tiles[0] = tiles[1] = 0;
        jda_exact_geo G;
        int32_t mcu[4];
        const bool luma_only = pixel_type == JDA_EIGHT_BIT_GRAYSCALE && I.ncomp == 3;
        if (!four && jda_exact_geometry_scaled(I, luma_only, scale, &G) == JDA_SUCCESS && (!has_rect || jda_exact_rect_plan(I, G, luma_only, rect, mcu) == JDA_SUCCESS)) {
            tiles[0] = jda_exact_tile_count(I, has_rect ? mcu : NULL); tiles[1] = jda_exact_tile_count(I, NULL);
        }
    }
    if ((int64_t)pitch_bytes < (int64_t)ow * (pixel_type == JDA_EIGHT_BIT_GRAYSCALE ? 1 : 4)) return JDA_INVALID_PARAMETER;      // (a row holds the image's width, as a surface's does)
    exact_resident R;
    rc = R.open(ctx, jpeg, len, I.jpeg_type == 1, four, JDA_COEF_AUTO);
    const int bpp = pixel_type == JDA_EIGHT_BIT_GRAYSCALE ? 1 : 4;
    const int dpitch = (int)align16((size_t)ow * bpp), drows = rows < oh ? rows : oh;
    void *dout = NULL;
    if (rc == JDA_SUCCESS && jda_pool_alloc(ctx, &dout, (size_t)dpitch * (size_t)oh + 16) != hipSuccess) rc = JDA_ERROR_MEMORY;
    if (rc == JDA_SUCCESS) {
        jda_output O;
        O.pixels = dout; O.pitch_bytes = dpitch; O.width_px = ow; O.rows = drows;
        int32_t st = JDA_SUCCESS;
        rc = exact_call(ctx, 1, &R.S, &O, &pixel_type, NULL, &st, NULL, &scale, flags, has_rect ? rect : NULL);
        if (rc == JDA_SUCCESS) rc = st;
    }
    if (rc == JDA_SUCCESS && drows > 0) {
        rc = copy_rows_back(ctx, host_pixels, (size_t)pitch_bytes, dout, (size_t)dpitch, (size_t)ow * bpp, (size_t)drows, false);
    }
    if (dout) jda_pool_free(ctx, dout);
    R.close(ctx);
    return rc;
}
int jda_decode_to_host_exact(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, void *host_pixels, int32_t pitch_bytes, int32_t rows)
{
    return jda_decode_to_host_exact_scaled(ctx, jpeg, len, pixel_type, 1, host_pixels, pitch_bytes, rows);
}
int jda_decode_to_host_exact_scaled(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t scale, void *host_pixels, int32_t pitch_bytes, int32_t rows)
{
    return jda_decode_to_host_exact_ex(ctx, jpeg, len, pixel_type, scale, 0u, host_pixels, pitch_bytes, rows);
}
int jda_decode_to_host_exact_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t scale, uint32_t flags, void *host_pixels, int32_t pitch_bytes,
                                int32_t rows)
{
    return exact_to_host(ctx, jpeg, len, pixel_type, scale, flags, NULL, host_pixels, pitch_bytes, rows, NULL);
}
int jda_decode_to_host_exact_rect(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t scale, uint32_t flags, const int32_t *rect, void *host_pixels,
                                  int32_t pitch_bytes, int32_t rows, int32_t *tiles)
{
    return exact_to_host(ctx, jpeg, len, pixel_type, scale, flags, rect, host_pixels, pitch_bytes, rows, tiles);
}

// Pillow's Image.open(f).thumbnail((req_w, req_h), F, reducing_gap): the plan, the exact decode at its scale into a device surface, the reduce
// and the resize behind it in the same block (each step's records wait for the host before the step is queued), the result's rows back
int jda_decode_to_host_thumbnail(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t req_w, int32_t req_h, int32_t filter, double reducing_gap,
                                 int32_t pixel_type, void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *out_w, int32_t *out_h, int32_t *launches)
{
    if (out_w) *out_w = 0;
    if (out_h) *out_h = 0;
    if (launches) launches[0] = launches[1] = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!jpeg || !host_pixels || pitch_bytes < 0 || rows < 0) return JDA_INVALID_PARAMETER;
    if (pixel_type != JDA_RGB8888 && pixel_type != JDA_EIGHT_BIT_GRAYSCALE) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    jda_image_info I;
    int rc = jda_parse(jpeg, len, &I);
    if (rc != JDA_SUCCESS) return rc;
    jda_thumbnail_steps T;
    rc = jda_thumbnail_plan_of(I.width, I.height, req_w, req_h, filter, reducing_gap, &T);
    if (rc != JDA_SUCCESS) return rc;
    if (out_w) *out_w = T.out_w;
    if (out_h) *out_h = T.out_h;
    const int bpp = pixel_type == JDA_EIGHT_BIT_GRAYSCALE ? 1 : 4;
    if ((int64_t)pitch_bytes < (int64_t)T.out_w * bpp || rows < T.out_h) return JDA_INVALID_PARAMETER;
    const bool reduces = T.fx > 1 || T.fy > 1;
    exact_resident R;
    rc = R.open(ctx, jpeg, len, I.jpeg_type == 1, false, JDA_COEF_AUTO);
    // one block: the draft image, behind it the reduced image and the result where the plan has those steps (each begins at a multiple of 256)
    jda_output D[3];
    size_t at = 0;
    const int32_t dims[3][2] = { { T.draft_w, T.draft_h }, { T.reduced_w, T.reduced_h }, { T.out_w, T.out_h } };
    const bool used[3] = { true, reduces, T.resize != 0 };
    size_t offs[3];
    for (int i = 0; i < 3; i++) {
        D[i].pitch_bytes = (int32_t)align16((size_t)dims[i][0] * bpp); D[i].width_px = dims[i][0]; D[i].rows = dims[i][1];
        offs[i] = at;
        if (used[i]) at += ((size_t)D[i].pitch_bytes * (size_t)dims[i][1] + 255u) & ~(size_t)255u;
    }
    uint8_t *blk = NULL;
    if (rc == JDA_SUCCESS && jda_pool_alloc(ctx, (void **)&blk, at + 16) != hipSuccess) rc = JDA_ERROR_MEMORY;
    for (int i = 0; i < 3; i++) D[i].pixels = blk && used[i] ? blk + offs[i] : NULL;
    if (rc == JDA_SUCCESS) {
        int32_t st = JDA_SUCCESS;
        rc = exact_call(ctx, 1, &R.S, &D[0], &pixel_type, NULL, &st, NULL, &T.scale);
        if (rc == JDA_SUCCESS) rc = st;
    }
    const jda_output *cur = &D[0];
    reduce_plan rd; rd.block = NULL;
    resize_plan rs; rs.block = NULL;
    if (rc == JDA_SUCCESS && reduces) {
        const int32_t factors[2] = { T.fx, T.fy };
        rc = reduce_upload(ctx, 1, cur, bpp, factors, T.reduce_box, &D[1], &rd);
        if (rc == JDA_SUCCESS) rc = reduce_launch(ctx, rd);
        if (rc == JDA_SUCCESS && launches) launches[0] = 1;
        cur = &D[1];
    }
    if (rc == JDA_SUCCESS && T.resize) {
        rc = resize_upload(ctx, 1, cur, bpp, NULL, &D[2], &rs, NULL, filter, T.box);
        if (rc == JDA_SUCCESS) rc = resize_launch(ctx, rs);
        if (rc == JDA_SUCCESS && launches) launches[1] = 1;
        cur = &D[2];
    }
    if (rc == JDA_SUCCESS) rc = copy_rows_back(ctx, host_pixels, (size_t)pitch_bytes, cur->pixels, (size_t)cur->pitch_bytes, (size_t)T.out_w * bpp, (size_t)T.out_h, false);
    else (void)hipStreamSynchronize(ctx->stream);
    if (rd.block) jda_pool_free(ctx, rd.block);
    if (rs.block) jda_pool_free(ctx, rs.block);
    if (blk) jda_pool_free(ctx, blk);
    R.close(ctx);
    return rc;
}

int jda_transcode_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, const int32_t *rect, int32_t out_w, int32_t out_h,
                          int32_t sampling, int32_t quality, int32_t restart_interval, void *host_file, int64_t capacity, int64_t *file_bytes)
{
    return jda_transcode_to_host_ex(ctx, jpeg, len, options, rect, out_w, out_h, sampling, quality, restart_interval, 0u, host_file, capacity, file_bytes);
}
static int transcode_call(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, const int32_t *rect, int32_t out_w, int32_t out_h,
                          int32_t sampling, int32_t quality, int32_t restart_interval, uint32_t encode_flags, bool progressive, void *host_file, int64_t capacity,
                          int64_t *file_bytes);
int jda_transcode_to_host_ex(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, const int32_t *rect, int32_t out_w, int32_t out_h,
                             int32_t sampling, int32_t quality, int32_t restart_interval, uint32_t encode_flags, void *host_file, int64_t capacity,
                             int64_t *file_bytes)
{
    return transcode_call(ctx, jpeg, len, options, rect, out_w, out_h, sampling, quality, restart_interval, encode_flags, false, host_file, capacity, file_bytes);
}
int jda_transcode_to_host_progressive(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, const int32_t *rect, int32_t out_w, int32_t out_h,
                                      int32_t sampling, int32_t quality, int32_t restart_interval, void *host_file, int64_t capacity, int64_t *file_bytes)
{
    return transcode_call(ctx, jpeg, len, options, rect, out_w, out_h, sampling, quality, restart_interval, 0u, true, host_file, capacity, file_bytes);
}
// the encoder: jda_encode_surfaces_ex, or (progressive) jda_encode_surfaces_progressive
static int transcode_call(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t options, const int32_t *rect, int32_t out_w, int32_t out_h,
                          int32_t sampling, int32_t quality, int32_t restart_interval, uint32_t encode_flags, bool progressive, void *host_file, int64_t capacity,
                          int64_t *file_bytes)
{
    if (file_bytes) *file_bytes = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (encode_flags & ~(uint32_t)JDA_ENCODE_OPTIMIZE) return JDA_INVALID_PARAMETER;
    if (progressive && restart_interval != 0) return JDA_INVALID_PARAMETER;
    if (!jpeg || !host_file || !file_bytes || capacity < 0 || out_w <= 0 || out_h <= 0) return JDA_INVALID_PARAMETER;
    onecall F;
    int rc = oc_open(F, ctx, jpeg, len);
    if (rc != JDA_SUCCESS) return rc;
    rc = oc_geometry(F, F.I.ncomp == 1 ? JDA_EIGHT_BIT_GRAYSCALE : JDA_RGB8888, options);      // a gray file is encoded as it is decoded
    const int bpp = F.bpp, ow = F.ow, oh = F.oh;
    if (rc == JDA_SUCCESS && (ow > F.cw || oh > F.ch)) rc = JDA_INVALID_PARAMETER;
    const int32_t whole[4] = { 0, 0, ow, oh };
    const int32_t *box = rect ? rect : whole;
    if (rc == JDA_SUCCESS && (box[0] < 0 || box[1] < 0 || box[2] <= 0 || box[3] <= 0 || (int64_t)box[0] + box[2] > ow || (int64_t)box[1] + box[3] > oh)) rc = JDA_INVALID_PARAMETER;
    int64_t bound = 0;
    if (rc == JDA_SUCCESS) rc = progressive ? jda_encode_bound_progressive(out_w, out_h, sampling, &bound) : jda_encode_bound_bytes(out_w, out_h, sampling, restart_interval, &bound);
    if (rc == JDA_SUCCESS && (quality < 1 || quality > 100 || (sampling == JDA_ENCODE_GRAY) != (bpp == 1))) rc = JDA_INVALID_PARAMETER;
    const bool resized = rc == JDA_SUCCESS && (out_w != box[2] || out_h != box[3]);
    { uint32_t k; if (resized) rc = jda_resize_axis_ksize(box[0], box[0] + box[2], out_w, &k); if (resized && rc == JDA_SUCCESS) rc = jda_resize_axis_ksize(box[1], box[1] + box[3], out_h, &k); }
    if (rc != JDA_SUCCESS) { jda_image_free(F.img); return rc; }
    const int opitch = (int)align16((size_t)out_w * bpp);
    const size_t rbytes = resized ? (size_t)opitch * out_h : 0;
    const int64_t fcap = std::min(capacity, bound);                                        // (no file is longer than the bound)
    rc = oc_upload(F, F.cbytes + rbytes + (size_t)fcap + 16, NULL);                        // the decoded canvas, the resized surface behind it, the file behind that
    if (rc != JDA_SUCCESS) return rc;
    jda_output D;
    D.pixels = F.dsurf + F.cbytes; D.pitch_bytes = opitch; D.width_px = out_w; D.rows = out_h;
    resize_plan plan;
    plan.block = NULL;
    int32_t reads[4] = { box[0], box[1], box[0] + box[2], box[1] + box[3] }, mcu_rect[4];  // without a resize the encoder reads the rectangle itself
    if (resized) rc = resize_upload(ctx, 1, &F.S, bpp, box, &D, &plan, reads);
    if (rc == JDA_SUCCESS) {
        const bool all = oc_mcu_rect(F, reads, mcu_rect);
        rc = oc_plan(F, all ? NULL : mcu_rect, NULL, NULL);
        if (rc == JDA_SUCCESS) rc = oc_run(F, (size_t)mcu_rect[1] * F.mh * F.cpitch, (size_t)(mcu_rect[3] - mcu_rect[1]) * F.mh * F.cpitch, false);
        if (rc == JDA_SUCCESS && resized) rc = resize_launch(ctx, plan);
        if (rc == JDA_SUCCESS) {
            // the encoder's stages follow on the same stream; its two looks at the sizes are the only waits
            const jda_encode_job E = { resized ? 0 : box[0], resized ? 0 : box[1], out_w, out_h, sampling, quality, restart_interval, 0 };
            void *dfile = F.dsurf + F.cbytes + rbytes;
            int32_t st = JDA_SUCCESS;
            rc = progressive ? jda_encode_surfaces_progressive(ctx, 1, resized ? &D : &F.S, bpp, &E, &dfile, &fcap, file_bytes, &st)
                             : jda_encode_surfaces_ex(ctx, 1, resized ? &D : &F.S, bpp, &E, encode_flags ? &encode_flags : NULL, &dfile, &fcap, file_bytes, &st);
            if (rc == JDA_SUCCESS) rc = st;
            if (rc == JDA_SUCCESS) {
                hipError_t e = hipMemcpyAsync(host_file, dfile, (size_t)*file_bytes, hipMemcpyDeviceToHost, ctx->stream);
                { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
                if (e != hipSuccess) rc = jda_set_err(ctx, e, "copy back");
            }
        }
    }
    return oc_close(F, rc, plan.block);
}

// ---- dense tensors back into surfaces (jda_unpack_tiles in jda_kernels.hip; vectors and the lane's gather: jda_device_core.h)
// Check n jobs (jda_unpack_plan.h) and upload their records, and wait for them as pack_upload does; unpack_launch then queues the kernel.
struct unpack_plan { void *block; uint32_t n, n_tiles, es, hwc, bpp, bgr; float scale_bias[6]; };
static int unpack_upload(jda_ctx *ctx, int32_t n, const void *const *src, int32_t layout_flags, int32_t elem_type, const float *scale_bias,
                         const jda_output *dst, int32_t dst_bytes_per_pixel, unpack_plan *plan)
{
    plan->block = NULL; plan->n = (uint32_t)n; plan->n_tiles = 0;
    jda_unpack_plan_out P;
    const int rc = jda_unpack_plan_jobs(n, src, layout_flags, elem_type, scale_bias, dst, dst_bytes_per_pixel, &P);
    if (rc != JDA_SUCCESS) return rc;
    plan->es = P.es; plan->hwc = P.hwc; plan->bpp = (uint32_t)dst_bytes_per_pixel; plan->bgr = (layout_flags & JDA_PACK_BGR) ? 1u : 0u;
    memcpy(plan->scale_bias, P.scale_bias, sizeof(plan->scale_bias));
    uint8_t *blk = NULL;
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, align16(P.jobs.size() * sizeof(jda_unpack_job)));
    if (e != hipSuccess) return jda_set_err(ctx, e, "hipMalloc(unpack jobs)");
    e = hipMemcpyAsync(blk, P.jobs.data(), P.jobs.size() * sizeof(jda_unpack_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { jda_pool_free(ctx, blk); return jda_set_err(ctx, e, "unpack jobs"); }
    plan->block = blk; plan->n_tiles = P.n_tiles;
    return JDA_SUCCESS;
}
static int unpack_launch(jda_ctx *ctx, const unpack_plan &plan)
{
    const hipError_t e = jda_launch_unpack((const jda_unpack_job *)plan.block, plan.n, plan.n_tiles, (int)plan.hwc, plan.es, plan.scale_bias, plan.bpp, plan.bgr, ctx->stream);
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_unpack_tiles");
}

int jda_unpack_surfaces(jda_ctx *ctx, int32_t n, const void *const *src, int32_t layout_flags, int32_t elem_type, const float *scale_bias,
                        const jda_output *dst, int32_t dst_bytes_per_pixel)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0) return JDA_INVALID_PARAMETER;
    { const int frc = jda_unpack_check_format(dst_bytes_per_pixel, layout_flags, elem_type, scale_bias); if (frc != JDA_SUCCESS) return frc; }
    if (n == 0) return JDA_SUCCESS;
    (void)hipSetDevice(ctx->device);
    unpack_plan plan;
    int rc = unpack_upload(ctx, n, src, layout_flags, elem_type, scale_bias, dst, dst_bytes_per_pixel, &plan);
    if (rc != JDA_SUCCESS) return rc;
    return finish_surfaces(ctx, unpack_launch(ctx, plan), plan.block, "jda_unpack_surfaces");
}

int jda_encode_dense_to_host(jda_ctx *ctx, const void *host_dense, int32_t w, int32_t h, int32_t channels, int32_t layout_flags, int32_t elem_type,
                             const float *scale_bias, int32_t sampling, int32_t quality, int32_t restart_interval, int32_t form,
                             void *host_file, int64_t capacity, int64_t *file_bytes)
{
    if (file_bytes) *file_bytes = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!host_dense || !host_file || !file_bytes || capacity < 0 || w <= 0 || h <= 0 || (channels != 1 && channels != 3)) return JDA_INVALID_PARAMETER;
    if (form != JDA_RECODE_BASELINE && form != JDA_RECODE_OPTIMIZE && form != JDA_RECODE_PROGRESSIVE) return JDA_INVALID_PARAMETER;
    const bool progressive = form == JDA_RECODE_PROGRESSIVE;
    if (progressive && restart_interval != 0) return JDA_INVALID_PARAMETER;
    const int bpp = channels == 3 ? 4 : 1;
    int rc = jda_unpack_check_format(bpp, layout_flags, elem_type, scale_bias);
    if (rc != JDA_SUCCESS) return rc;
    if (quality < 1 || quality > 100 || (sampling == JDA_ENCODE_GRAY) != (bpp == 1)) return JDA_INVALID_PARAMETER;
    const uint64_t dense = (uint64_t)w * (uint64_t)h * (uint64_t)channels * jda_pack_elem_bytes(elem_type);
    if (dense > JDA_PACK_MAX_BYTES) return JDA_INVALID_PARAMETER;
    int64_t bound = 0;
    rc = progressive ? jda_encode_bound_progressive(w, h, sampling, &bound) : jda_encode_bound_bytes(w, h, sampling, restart_interval, &bound);
    if (rc != JDA_SUCCESS) return rc;
    (void)hipSetDevice(ctx->device);
    const size_t pitch = align16((size_t)w * bpp), sbytes = pitch * (size_t)h;
    const int64_t fcap = std::min(capacity, bound);                                        // (no file is longer than the bound)
    uint8_t *blk = NULL;                                                                   // the surface, the dense image behind it, the file behind that
    hipError_t e = jda_pool_alloc(ctx, (void **)&blk, sbytes + align16((size_t)dense) + (size_t)fcap + 16);
    if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc(dense image)"); return JDA_ERROR_MEMORY; }
    uint8_t *ddense = blk + sbytes;
    void *dfile = ddense + align16((size_t)dense);
    jda_output S;
    S.pixels = blk; S.pitch_bytes = (int32_t)pitch; S.width_px = w; S.rows = h;
    unpack_plan plan;
    plan.block = NULL;
    // the image and the job record go up; then unpack and the encoder's stages are queued back to back on the one stream, and its two looks
    // at the sizes are the only waits
    e = hipMemcpyAsync(ddense, host_dense, (size_t)dense, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) rc = jda_set_err(ctx, e, "upload");
    const void *const srcs[1] = { ddense };
    if (rc == JDA_SUCCESS) rc = unpack_upload(ctx, 1, srcs, layout_flags, elem_type, scale_bias, &S, bpp, &plan);
    if (rc == JDA_SUCCESS) rc = unpack_launch(ctx, plan);
    if (rc == JDA_SUCCESS) {
        const jda_encode_job E = { 0, 0, w, h, sampling, quality, restart_interval, 0 };
        const uint32_t flags = form == JDA_RECODE_OPTIMIZE ? (uint32_t)JDA_ENCODE_OPTIMIZE : 0u;
        int32_t st = JDA_SUCCESS;
        rc = progressive ? jda_encode_surfaces_progressive(ctx, 1, &S, bpp, &E, &dfile, &fcap, file_bytes, &st)
                         : jda_encode_surfaces_ex(ctx, 1, &S, bpp, &E, flags ? &flags : NULL, &dfile, &fcap, file_bytes, &st);
        if (rc == JDA_SUCCESS) rc = st;
        if (rc == JDA_SUCCESS) {
            e = hipMemcpyAsync(host_file, dfile, (size_t)*file_bytes, hipMemcpyDeviceToHost, ctx->stream);
            { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
            if (e != hipSuccess) rc = jda_set_err(ctx, e, "copy back");
        }
    }
    (void)hipStreamSynchronize(ctx->stream);
    jda_pool_free(ctx, plan.block);
    jda_pool_free(ctx, blk);
    return rc;
}

// Measuring hook of tools/unpack_bench.py (not part of the public header): the unpack launch between the context's two timer events on
// its stream -- the job records go up before the first event.  ms[k]: repeat k.
int jda_internal_unpack_time(jda_ctx *ctx, int32_t n, const void *const *src, int32_t layout_flags, int32_t elem_type, const float *scale_bias,
                             const jda_output *dst, int32_t dst_bytes_per_pixel, int32_t reps, float *ms)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n <= 0 || reps <= 0 || !ms) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    unpack_plan plan;
    const int rc = unpack_upload(ctx, n, src, layout_flags, elem_type, scale_bias, dst, dst_bytes_per_pixel, &plan);
    if (rc != JDA_SUCCESS) return rc;
    return timed_launches(ctx, reps, ms, plan.block, "jda_internal_unpack_time", [&]() { return unpack_launch(ctx, plan); });
}

// Measuring hook of tools/resize_bench.py (not part of the public header): the resize launch between the context's two timer events on
// its stream -- job records and taps go up before the first event.  ms[k]: repeat k.
int jda_internal_resize_time_ex(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst,
                                int32_t filter, int32_t reps, float *ms);
int jda_internal_resize_time(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst,
                             int32_t reps, float *ms)
{
    return jda_internal_resize_time_ex(ctx, n, src, bytes_per_pixel, rects, dst, JDA_RESIZE_BILINEAR, reps, ms);
}
int jda_internal_resize_time_ex(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *rects, const jda_output *dst,
                                int32_t filter, int32_t reps, float *ms)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n <= 0 || reps <= 0 || !ms || !src || !dst) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    resize_plan plan;
    const int rc = resize_upload(ctx, n, src, bytes_per_pixel, rects, dst, &plan, NULL, filter);
    if (rc != JDA_SUCCESS) return rc;
    return timed_launches(ctx, reps, ms, plan.block, "jda_internal_resize_time", [&]() { return resize_launch(ctx, plan); });
}

// Measuring hook of tools/pack_bench.py (not part of the public header): the pack launch between the context's two timer events on its
// stream -- the job records go up before the first event.  ms[k]: repeat k.
int jda_internal_pack_time(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t src_bytes_per_pixel, const int32_t *rects, int32_t layout_flags,
                           int32_t elem_type, const void *table, void *const *dst, int32_t reps, float *ms)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n <= 0 || reps <= 0 || !ms) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    pack_plan plan;
    const int rc = pack_upload(ctx, n, src, src_bytes_per_pixel, rects, layout_flags, elem_type, table, dst, &plan);
    if (rc != JDA_SUCCESS) return rc;
    return timed_launches(ctx, reps, ms, plan.block, "jda_internal_pack_time", [&]() { return pack_launch(ctx, plan); });
}

// Measuring hooks of tools/orient_bench.py (not part of the public header): the orient launch, and a device-to-device copy to hold it
// against, each between the context's two timer events on its stream -- the job records go up before the first event.  ms[k]: repeat k.
int jda_internal_orient_time(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *orientations, const jda_output *dst,
                             int32_t reps, float *ms)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n <= 0 || !src || !orientations || !dst || reps <= 0 || !ms) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    orient_plan plan;
    const int rc = orient_upload(ctx, n, src, bytes_per_pixel, orientations, dst, &plan);
    if (rc != JDA_SUCCESS) return rc;
    return timed_launches(ctx, reps, ms, plan.block, "jda_internal_orient_time", [&]() { return orient_launch(ctx, plan); });
}
// Measuring hook of tools/thumbnail_bench.py (not part of the public header): the reduce launch between the context's two timer events on
// its stream -- the job records go up before the first event.  ms[k]: repeat k.
int jda_internal_reduce_time(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const int32_t *factors, const int32_t *boxes, const jda_output *dst,
                             int32_t reps, float *ms)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n <= 0 || !src || !factors || !dst || reps <= 0 || !ms) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    reduce_plan plan;
    const int rc = reduce_upload(ctx, n, src, bytes_per_pixel, factors, boxes, dst, &plan);
    if (rc != JDA_SUCCESS) return rc;
    return timed_launches(ctx, reps, ms, plan.block, "jda_internal_reduce_time", [&]() { return reduce_launch(ctx, plan); });
}
int jda_internal_copy_time(jda_ctx *ctx, void *dst, const void *src, size_t bytes, int32_t reps, float *ms)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!dst || !src || !bytes || reps <= 0 || !ms) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    return timed_launches(ctx, reps, ms, NULL, "jda_internal_copy_time", [&]() {
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream);
        return e == hipSuccess ? (int)JDA_SUCCESS : jda_set_err(ctx, e, "jda_internal_copy_time");
    });
}

} // extern "C"
