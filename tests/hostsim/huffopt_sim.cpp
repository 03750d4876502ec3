// tests/hostsim/huffopt_sim.cpp -- TEST INFRASTRUCTURE: the nine stages of jda_encode_surfaces_ex on the CPU.
//
// huffoptsim_lanes runs a call with per-job flags the way the GPU runs it: blocks and lengths as tests/hostsim/encode_sim.cpp steps them,
// then every lane of jda_huffopt_gather and jda_huffopt_lengths through the kernels' OWN code (jda_ho_* of jda_device_core.h), the host's
// step between them as jda_runtime.cpp takes it (jda_encode_plan_tables of jda_encode_plan.h), then scan, emit, count, scan, write.  The
// memory policy is encode_sim.cpp's -- this file includes it for SimIO, Run, setup and scan, and adds what the two new stages need: a
// workgroup's histogram in LDS is poisoned before every workgroup and a bin of it is read or added to only after this workgroup cleared it
// for the job at hand; the histograms in HBM are zeros and change only by atomic add; an optimised job's code words and header are what
// the host made from the counts the lanes left there.  A workgroup takes its jobs in turn, its lanes in REVERSE order in the adding
// phase: no lane's adds may depend on another's.
// huffoptsim_table is jda_encode_optimal_table alone, huffoptsim_check the argument checks with flags.
#include "encode_sim.cpp"

namespace {
struct OptIO : SimIO {
    std::vector<uint32_t> h; std::vector<uint8_t> h_set;
    void lds_poison() { h.assign(JDA_EN_HUFF_DWORDS, 0xEEEEEEEEu); h_set.assign(JDA_EN_HUFF_DWORDS, 0); }
    void lds_st32(uint32_t i, uint32_t v) { if (i >= h.size()) { fail(-42); return; } h[i] = v; h_set[i] = 1; }
    uint32_t lds_ld32(uint32_t i) { if (i >= h.size() || !h_set[i]) { fail(-43); return 0; } return h[i]; }
    void lds_add32(uint32_t i, uint32_t v) { if (i >= h.size() || !h_set[i]) { fail(-44); return; } h[i] += v; }
    void atomic_add(uint32_t *p, uint32_t v) { if (wr(p, 4, true)) *p += v; }
};
struct OptRun : Run { OptIO oio; std::vector<uint8_t> hist_mem; uint32_t *hist; };

// setup() of encode_sim.cpp fills R.io; the stages here run over a copy that has the histogram's LDS as well
void adopt(OptRun &R) { static_cast<SimIO &>(R.oio) = R.io; }

int gather(OptRun &R)
{
    const uint32_t nb = R.P.n_blocks;
    for (uint32_t first = 0; first < nb; first += JDA_EN_THREADS) {
        R.oio.lds_poison();                                                     // a workgroup finds nothing in LDS
        const uint32_t last = first + JDA_EN_THREADS - 1u < nb ? first + JDA_EN_THREADS - 1u : nb - 1u;
        const uint32_t j0 = jda_en_find_block(R.A.jobs, R.A.n_jobs, first, R.oio), j1 = jda_en_find_block(R.A.jobs, R.A.n_jobs, last, R.oio);
        for (uint32_t j = j0; j <= j1; j++) {
            const uint32_t hoff = R.oio.ld32(&R.A.jobs[j].hist_off);
            if (hoff == JDA_EN_NO_HIST) continue;
            R.oio.cur = &R.jobs[j];
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_ho_clear(tid, R.oio);
            for (uint32_t tid = JDA_EN_THREADS; tid-- > 0u;) {
                const uint32_t b = first + tid;
                if (b < nb && jda_en_find_block(R.A.jobs, R.A.n_jobs, b, R.oio) == j) jda_ho_count(R.A, R.jobs[j], b, R.oio);
            }
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_ho_flush(R.hist + hoff, tid, R.oio);
        }
    }
    return R.oio.err;
}
}

// n jobs over HOST surfaces into HOST files, job_flags = NULL or n words.  0, or the first promise broken (encode_sim.cpp's codes; -42 .. -44:
// the histogram's LDS), or the status of the argument checks or of the table step.  Optional outputs in the call's flat order: coef, code
// (BEHIND the second lengths pass), end; hist: the call's histograms, JDA_EN_HUFF_DWORDS per optimised job in the jobs' order;
// info = {blocks, intervals, chunks, unstuffed bytes, optimised jobs}.
extern "C" int huffoptsim_lanes(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, const uint32_t *job_flags, void *const *dst, const int64_t *cap,
                                int64_t *dst_bytes, int32_t *status, int16_t *coef, uint32_t *code, uint64_t *end, uint32_t *hist, uint64_t *info)
{
    OptRun R;
    int rc = jda_encode_plan_jobs_ex(n, src, bpp, jobs, job_flags, dst, cap, &R.P);
    if (rc != JDA_SUCCESS) return rc;
    setup(R, (uint32_t)bpp);
    jda_encode_plan_out &P = R.P;
    const size_t nj = P.jobs.size(), hist_bytes = (size_t)P.n_opt * JDA_EN_HUFF_DWORDS * 4;
    R.hist = aligned<uint32_t>(R.hist_mem, hist_bytes);                         // (zeroed by the call)
    if (P.n_opt) R.io.add(R.hist, hist_bytes, true, false, true);
    adopt(R);
    OptIO &io = R.oio;
    for (uint32_t b = 0; b < P.n_blocks; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
        if (b < R.jobs[j].block0 || b >= R.jobs[j].block0 + R.jobs[j].n_blocks) return -50;
        io.cur = &R.jobs[j];
        jda_en_block(R.A, R.jobs[j], b, io);
    }
    for (uint32_t b = 0; b < P.n_blocks; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
        io.cur = &R.jobs[j];
        jda_en_length(R.A, R.jobs[j], b, io);
    }
    if (io.err) return io.err;
    if (P.n_opt) {                                                              // a call without an optimised job has none of this
        if (gather(R)) return io.err;
        rc = jda_encode_plan_tables(&P, R.hist);                                // the host between gather and the second lengths pass
        if (rc != JDA_SUCCESS) return rc;
        memcpy(R.huff.data(), P.huff.data(), P.huff.size() * 4);                // (the uploads: the words, the headers)
        memcpy((uint8_t *)R.A.hdr, P.hdr.data(), P.hdr.size());
        for (uint32_t b = 0; b < P.n_blocks; b++) {
            const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
            io.cur = &R.jobs[j];
            jda_ho_length(R.A, R.jobs[j], b, io);
        }
        if (io.err) return io.err;
    }
    // the rest as finish() of encode_sim.cpp runs it, over this call's IO
    auto scan_opt = [&R, &io](bool bytes) {
        for (uint32_t j = 0; j < R.A.n_jobs; j++) {
            std::fill(io.lds.begin(), io.lds.end(), 0xEEEEEEEEEEEEEEEEull);
            std::fill(io.lds_set.begin(), io.lds_set.end(), 0);
            io.cur = &R.jobs[j];
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_en_scan_job(R.A, R.jobs[j], j, bytes, false, tid, io);
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_en_scan_job(R.A, R.jobs[j], j, bytes, true, tid, io);
        }
    };
    scan_opt(false);
    if (io.err) return io.err;
    std::vector<jda_encode_totals> tot(nj);
    for (size_t i = 0; i < nj; i++) { if (!io.rd(&R.A.totals[i].u_bytes, 8)) return -51; tot[i] = R.A.totals[i]; }
    rc = jda_encode_plan_place(&P, tot.data());
    if (rc != JDA_SUCCESS) return rc;
    R.jobs = P.jobs;
    R.A.jobs = R.jobs.data();
    io.allocs[R.jobs_alloc].base = (uint8_t *)R.jobs.data();                  // (the second upload of the records)
    R.A.u = aligned<uint8_t>(R.u, (size_t)P.u_total); io.add(R.A.u, (size_t)P.u_total, true, false, true);
    R.A.ffcnt = aligned<uint32_t>(R.ffcnt, (size_t)P.n_chunks * 4); io.add(R.A.ffcnt, (size_t)P.n_chunks * 4, true, true);
    R.A.ffend = aligned<uint64_t>(R.ffend, (size_t)P.n_chunks * 8); io.add(R.A.ffend, (size_t)P.n_chunks * 8, true, true);
    io.jobs = R.jobs.data(); io.n_jobs = nj;
    io.written.resize(nj);
    for (size_t i = 0; i < nj; i++) io.written[i].assign((size_t)R.jobs[i].capacity, 0);
    for (uint32_t b = 0; b < P.n_blocks; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
        io.cur = &R.jobs[j];
        jda_en_emit(R.A, R.jobs[j], b, io);
    }
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t j = jda_en_find_chunk(R.A.jobs, R.A.n_jobs, c, io);
        if (c < R.jobs[j].chunk0 || c >= R.jobs[j].chunk0 + R.jobs[j].n_chunks) return -52;
        io.cur = &R.jobs[j];
        jda_en_count(R.A, R.jobs[j], c, io);
    }
    scan_opt(true);
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t j = jda_en_find_chunk(R.A.jobs, R.A.n_jobs, c, io);
        io.cur = &R.jobs[j];
        jda_en_write(R.A, R.jobs[j], j, c, io);
    }
    if (io.err) return io.err;
    for (size_t i = 0; i < nj; i++) {
        if (!io.rd(&R.A.totals[i].file_bytes, 8)) return -53;
        const uint64_t fb = R.A.totals[i].file_bytes;
        dst_bytes[i] = (int64_t)fb;
        status[i] = fb > R.jobs[i].capacity ? JDA_ERROR_MEMORY : JDA_SUCCESS;
        for (size_t k = 0; k < io.written[i].size(); k++)
            if ((io.written[i][k] != 0) != (status[i] == JDA_SUCCESS && k < fb)) return -32;
    }
    if (coef) memcpy(coef, R.A.coef, (size_t)P.n_blocks * 128);
    if (code) memcpy(code, R.A.code, (size_t)P.n_blocks * 4);
    if (end) memcpy(end, R.A.end, (size_t)P.n_blocks * 8);
    if (hist && P.n_opt) memcpy(hist, R.hist, hist_bytes);
    if (info) { info[0] = P.n_blocks; info[1] = P.n_int; info[2] = P.n_chunks; info[3] = P.u_total; info[4] = P.n_opt; }
    return 0;
}

// jda_encode_optimal_table: 0, or 1 where libjpeg gives up.  vals: 256 bytes.
extern "C" int huffoptsim_table(const uint32_t *freq, uint8_t *bits, uint8_t *vals, uint32_t *n_vals)
{
    return jda_encode_optimal_table(freq, bits, vals, n_vals) ? 0 : 1;
}
// the argument checks of jda_encode_surfaces_ex (behind its ctx / n == 0 / null-array checks) on pointers that are never followed
extern "C" int huffoptsim_check(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, const uint32_t *job_flags, void *const *dst, const int64_t *cap)
{
    jda_encode_plan_out P;
    return jda_encode_plan_jobs_ex(n, src, bpp, jobs, job_flags, dst, cap, &P);
}
