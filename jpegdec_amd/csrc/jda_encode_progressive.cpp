// jda_encode_progressive.cpp -- jda_encode_surfaces_progressive: the host side of the progressive encoder, a translation unit of its own
// (the baseline encoder's host code in jda_runtime.cpp is compiled as it was).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "jda_runtime_internal.h"
#include "jda_encode_prog_plan.h"

// ---- progressive encode (jda_progenc_* in jda_kernels.hip; the stages: jda_pe_* in jda_device_core.h; checks, records, tables and headers:
// jda_encode_prog_plan.h).  Three parts with the host between them: the records go up, blocks / lengths / classify / resolve / gather run and
// the symbol counts come back (1 KiB a scan); the host makes every scan's table, code words and header, the words go up, lengths / scan run
// and the scans' sizes come back (8 bytes a scan); the host places the scans, the records and headers go up, the zeroed data buffer is
// taken from the pool, and emit / count / scan / write run; then the files' sizes come back.
struct progenc_run {
    uint8_t *a, *b; jda_pe_arrays A; jda_pe_plan_out P; uint32_t *hist; std::vector<jda_encode_totals> totals;
    float *stage_ms;                              // (the measuring hook: stage_ms[JDA_PE_STAGES + 1], the host's two steps last)
    jda_rc_hook *rc;                              // a recode call (jda_recode_images): its sources in the place of the blocks stage; NULL: pixels
};
static hipError_t progenc_stages(jda_ctx *ctx, progenc_run &R, uint32_t s0, uint32_t s1)
{
    hipError_t e = hipSuccess;
    for (uint32_t s = s0; s < s1 && e == hipSuccess; s++) {
        if (R.stage_ms) e = hipEventRecord(ctx->ev_start, ctx->stream);
        if (e == hipSuccess) {
            if (s == JDA_PE_STAGE_BLOCKS && R.rc) {
                e = jda_rc_hook_launch(&R.A.E, *R.rc, R.P.B.n_blocks, ctx->stream);
            } else {
                e = jda_launch_progenc_stage(&R.A, s, R.P.B.n_blocks, R.P.n_units, (uint32_t)R.P.pjobs.size(), R.P.n_chunks, R.hist, ctx->stream);
            }
        }
        if (R.stage_ms) {
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventRecord(ctx->ev_stop, ctx->stream);
            if (e == hipSuccess) e = hipEventSynchronize(ctx->ev_stop);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop);
            R.stage_ms[s] += ms;
        }
    }
    return e;
}
static int progenc_run_call(jda_ctx *ctx, progenc_run &R)
{
    jda_pe_plan_out &P = R.P;
    const size_t n = P.pjobs.size(), nb = P.B.n_blocks, nu = P.n_units, ns = P.segs.size();
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_jobs = take(n * sizeof(jda_encode_dev_job)), o_quant = take(P.B.quant.size() * sizeof(jda_encode_quant)), o_huff = take((size_t)JDA_EN_HUFF_DWORDS * 4);
    const size_t o_coef = take(nb * 128), o_meta = take(nb * 4), o_code = take(nb * 4), o_tot = take(n * sizeof(jda_encode_totals));
    const size_t o_segs = take(ns * sizeof(jda_pe_seg)), o_pjobs = take(n * sizeof(jda_pe_job)), o_words = take(ns * JDA_PE_TAB_DWORDS * 4), o_hist = take(ns * JDA_PE_TAB_DWORDS * 4);
    const size_t o_cls = take(nu * 4), o_run = take(nu * 4), o_len = take(nu * 4), o_end = take(nu * 8), o_sb = take(ns * 8), o_hdr = take(jda_pe_hdr_room(P));
    const size_t o_rsrc = take(R.rc ? n * sizeof(jda_rc_src) : 0), o_bad = take(R.rc ? n * 4 : 0), o_xf = take(R.rc ? R.rc->xf.size() * sizeof(jda_rc_xf) : 0);
    hipError_t e = jda_pool_alloc(ctx, (void **)&R.a, off);
    if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc(progressive encode scratch)"); return JDA_ERROR_MEMORY; }
    jda_pe_arrays &A = R.A;
    memset(&A, 0, sizeof(A));
    A.E.jobs = (const jda_encode_dev_job *)(R.a + o_jobs); A.E.quant = (const jda_encode_quant *)(R.a + o_quant); A.E.huff = (const uint32_t *)(R.a + o_huff);
    A.E.coef = (int16_t *)(R.a + o_coef); A.E.meta = (uint32_t *)(R.a + o_meta); A.E.code = (uint32_t *)(R.a + o_code); A.E.totals = (jda_encode_totals *)(R.a + o_tot);
    A.E.n_jobs = (uint32_t)n;
    A.segs = (const jda_pe_seg *)(R.a + o_segs); A.pjobs = (const jda_pe_job *)(R.a + o_pjobs); A.words = (const uint32_t *)(R.a + o_words); A.hdr = R.a + o_hdr;
    A.cls = (uint32_t *)(R.a + o_cls); A.run = (uint32_t *)(R.a + o_run); A.len = (uint32_t *)(R.a + o_len); A.end = (uint64_t *)(R.a + o_end);
    A.sbytes = (uint64_t *)(R.a + o_sb); A.n_segs = (uint32_t)ns;
    R.hist = (uint32_t *)(R.a + o_hist);
    e = hipMemcpyAsync(R.a + o_jobs, P.B.jobs.data(), n * sizeof(jda_encode_dev_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_quant, P.B.quant.data(), P.B.quant.size() * sizeof(jda_encode_quant), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_huff, P.B.huff.data(), (size_t)JDA_EN_HUFF_DWORDS * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_segs, P.segs.data(), ns * sizeof(jda_pe_seg), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_pjobs, P.pjobs.data(), n * sizeof(jda_pe_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(R.hist, 0, ns * JDA_PE_TAB_DWORDS * 4, ctx->stream);      // (the pool hands out what earlier calls left in it)
    if (R.rc) {
        R.rc->d_src = (jda_rc_src *)(R.a + o_rsrc); R.rc->d_bad = (uint32_t *)(R.a + o_bad);
        if (e == hipSuccess) e = hipMemcpyAsync(R.rc->d_src, R.rc->src.data(), n * sizeof(jda_rc_src), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(R.rc->d_bad, 0, n * 4, ctx->stream);
        R.rc->d_xf = (jda_rc_xf *)(R.a + o_xf);
        if (e == hipSuccess && !R.rc->xf.empty()) e = hipMemcpyAsync(R.rc->d_xf, R.rc->xf.data(), R.rc->xf.size() * sizeof(jda_rc_xf), hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = progenc_stages(ctx, R, JDA_PE_STAGE_BLOCKS, JDA_PE_STAGE_LENGTHS);
    std::vector<uint32_t> hist(ns * JDA_PE_TAB_DWORDS);
    auto t0 = std::chrono::steady_clock::now();
    if (e == hipSuccess) e = hipMemcpyAsync(hist.data(), R.hist, hist.size() * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (R.rc) { R.rc->bad.assign(n, 0u); if (e == hipSuccess) e = hipMemcpyAsync(R.rc->bad.data(), R.rc->d_bad, n * 4, hipMemcpyDeviceToHost, ctx->stream); }
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    if (e != hipSuccess) return jda_set_err(ctx, e, "jda_encode_surfaces_progressive (counts)");
    if (R.rc) {                                   // a job with a block out of range: no byte of its file is written
        bool any = false;
        for (size_t i = 0; i < n; i++) if (R.rc->bad[i]) { P.B.jobs[i].capacity = 0; any = true; }
        if (any) e = hipMemcpyAsync(R.a + o_jobs, P.B.jobs.data(), n * sizeof(jda_encode_dev_job), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return jda_set_err(ctx, e, "jda_recode_images (job records)");
    }
    int rc = jda_pe_plan_tables(&P, hist.data());
    if (rc != JDA_SUCCESS) return rc;
    e = hipMemcpyAsync(R.a + o_words, P.words.data(), P.words.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (R.stage_ms) R.stage_ms[JDA_PE_STAGES] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (e == hipSuccess) e = progenc_stages(ctx, R, JDA_PE_STAGE_LENGTHS, JDA_PE_STAGE_EMIT);
    std::vector<uint64_t> sbytes(ns);
    t0 = std::chrono::steady_clock::now();
    if (e == hipSuccess) e = hipMemcpyAsync(sbytes.data(), A.sbytes, ns * 8, hipMemcpyDeviceToHost, ctx->stream);
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    if (e != hipSuccess) return jda_set_err(ctx, e, "jda_encode_surfaces_progressive (lengths)");
    rc = jda_pe_plan_place(&P, sbytes.data());
    if (rc != JDA_SUCCESS) return rc;
    off = 0;
    const size_t o_u = take((size_t)P.u_total), o_cnt = take((size_t)P.n_chunks * 4), o_ffend = take((size_t)P.n_chunks * 8);
    e = jda_pool_alloc(ctx, (void **)&R.b, off);
    if (e != hipSuccess) { jda_set_err(ctx, e, "hipMalloc(progressive encode streams)"); return JDA_ERROR_MEMORY; }
    A.E.u = R.b + o_u; A.E.ffcnt = (uint32_t *)(R.b + o_cnt); A.E.ffend = (uint64_t *)(R.b + o_ffend);
    e = hipMemsetAsync(A.E.u, 0, (size_t)P.u_total, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_segs, P.segs.data(), ns * sizeof(jda_pe_seg), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_pjobs, P.pjobs.data(), n * sizeof(jda_pe_job), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(R.a + o_hdr, P.hdr.data(), P.hdr.size(), hipMemcpyHostToDevice, ctx->stream);
    if (R.stage_ms) R.stage_ms[JDA_PE_STAGES] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (e == hipSuccess) e = progenc_stages(ctx, R, JDA_PE_STAGE_EMIT, JDA_PE_STAGES);
    R.totals.resize(n);
    if (e == hipSuccess) e = hipMemcpyAsync(R.totals.data(), A.E.totals, n * sizeof(jda_encode_totals), hipMemcpyDeviceToHost, ctx->stream);
    { const hipError_t es = hipStreamSynchronize(ctx->stream); if (e == hipSuccess) e = es; }
    return e == hipSuccess ? JDA_SUCCESS : jda_set_err(ctx, e, "jda_encode_surfaces_progressive (files)");
}
static int progenc_call(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, void *const *dst, const int64_t *dst_capacity,
                        int64_t *dst_bytes, int32_t *status, float *stage_ms)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0 || (bytes_per_pixel != 1 && bytes_per_pixel != 4)) return JDA_INVALID_PARAMETER;
    if (n == 0) return JDA_SUCCESS;
    if (!src || !jobs || !dst || !dst_capacity || !dst_bytes || !status) return JDA_INVALID_PARAMETER;
    (void)hipSetDevice(ctx->device);
    progenc_run R;
    R.a = R.b = NULL; R.hist = NULL; R.stage_ms = stage_ms; R.rc = NULL;
    int rc = jda_pe_plan_jobs(n, src, bytes_per_pixel, jobs, dst, dst_capacity, &R.P);
    if (rc != JDA_SUCCESS) return rc;
    rc = progenc_run_call(ctx, R);
    if (rc != JDA_SUCCESS) (void)hipStreamSynchronize(ctx->stream);
    if (R.b) jda_pool_free(ctx, R.b);
    if (R.a) jda_pool_free(ctx, R.a);
    if (rc != JDA_SUCCESS) return rc;
    for (int i = 0; i < n; i++) {
        dst_bytes[i] = (int64_t)R.totals[(size_t)i].file_bytes;
        status[i] = R.totals[(size_t)i].file_bytes > (uint64_t)dst_capacity[i] ? JDA_ERROR_MEMORY : JDA_SUCCESS;
    }
    return JDA_SUCCESS;
}
// a recode call's progressive jobs (jda_recode_images): the plan is made (jda_recode_plan.h), the hook stands in for the blocks stage
int jda_progenc_recode(jda_ctx *ctx, jda_pe_plan_out &P, jda_rc_hook &hook, std::vector<jda_encode_totals> &totals)
{
    progenc_run R;
    R.a = R.b = NULL; R.hist = NULL; R.stage_ms = NULL; R.rc = &hook;
    R.P = std::move(P);
    int rc = progenc_run_call(ctx, R);
    if (rc != JDA_SUCCESS) (void)hipStreamSynchronize(ctx->stream);
    if (R.b) jda_pool_free(ctx, R.b);
    if (R.a) jda_pool_free(ctx, R.a);
    totals = R.totals;
    P = std::move(R.P);
    return rc;
}
int jda_encode_bound_progressive(int32_t w, int32_t h, int32_t sampling, int64_t *bytes) { return jda_pe_bound_bytes(w, h, sampling, bytes); }
int jda_encode_surfaces_progressive(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs,
                                    void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status)
{
    return progenc_call(ctx, n, src, bytes_per_pixel, jobs, dst, dst_capacity, dst_bytes, status, NULL);
}
// Measuring hook of tools/encode_prog_bench.py (not part of the public header): the call with every one of its eleven launches between the
// context's two timer events; stage_ms[JDA_PE_STAGES + 1] (order: JDA_PE_STAGE_*, then the host's two steps between the parts -- the copies
// back, the waits, the tables, the placement, the uploads) is ADDED to, so the caller zeroes it.
extern "C" int jda_internal_progenc_time(jda_ctx *ctx, int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs,
                              void *const *dst, const int64_t *dst_capacity, int64_t *dst_bytes, int32_t *status, float *stage_ms)
{
    if (!stage_ms) return JDA_INVALID_PARAMETER;
    return progenc_call(ctx, n, src, bytes_per_pixel, jobs, dst, dst_capacity, dst_bytes, status, stage_ms);
}

