// tests/hostsim/encode_prog_sim.cpp -- TEST INFRASTRUCTURE: the eleven launches of jda_encode_surfaces_progressive on the CPU.
//
// encodeprogsim_lanes runs a call the way the GPU runs it: blocks and lengths as tests/hostsim/encode_sim.cpp steps them, then every lane of
// classify, resolve, gather, lengths, scan, emit, count, scan and write through the kernels' OWN code (jda_pe_* of jda_device_core.h) over
// the records the host plan makes (jda_encode_prog_plan.h), the host's two steps between them as jda_runtime.cpp takes them.  The memory
// policy is encode_sim.cpp's -- this file includes it for SimIO, Run and setup: an access lies whole inside ONE allocation and is aligned
// to its own width; the unit records, lengths, positions and chunk counts are poisoned, a byte of them is read only after a lane wrote it,
// and every word of them is written -- a resolve word exactly once; the unstuffed data are zeros and change only by atomic OR; a
// workgroup's LDS (the scan's, the histogram's) is poisoned before every workgroup; the histograms in HBM change only by atomic add; no
// byte of a file is written twice, none behind the capacity, and in the end every byte of a file that fits once -- of one that does not,
// none.  resolve, gather's adding phase and emit run their lanes in REVERSE order: no lane may need another's result of the same stage.
// encodeprogsim_resolve runs the run-resolution stage alone over unit records of the caller's; encodeprogsim_check the argument checks;
// encodeprogsim_bound the bound.
#include "encode_sim.cpp"

#include "../../jpegdec_amd/csrc/jda_encode_prog_plan.h"

namespace {
struct ProgIO : SimIO {
    std::vector<uint32_t> h; std::vector<uint8_t> h_set;
    const uint8_t *once_base; size_t once_size;                                  // words that may be stored once only (the resolve stage's)
    void lds_poison() { h.assign(JDA_PE_TAB_DWORDS, 0xEEEEEEEEu); h_set.assign(JDA_PE_TAB_DWORDS, 0); }
    void lds_st32(uint32_t i, uint32_t v) { if (i >= h.size()) { fail(-42); return; } h[i] = v; h_set[i] = 1; }
    uint32_t lds_ld32(uint32_t i) { if (i >= h.size() || !h_set[i]) { fail(-43); return 0; } return h[i]; }
    void lds_add32(uint32_t i, uint32_t v) { if (i >= h.size() || !h_set[i]) { fail(-44); return; } h[i] += v; }
    void atomic_add(uint32_t *p, uint32_t v) { if (wr(p, 4, true)) *p += v; }
    void st32(uint32_t *p, uint32_t v)
    {
        const uint8_t *q = (const uint8_t *)p;
        if (once_base && q >= once_base && q < once_base + once_size) {
            Alloc *a = find(p, 4);
            if (a && !a->init.empty() && a->init[(size_t)(q - a->base)]) { fail(-45); return; }
        }
        SimIO::st32(p, v);
    }
};
bool all_written(ProgIO &io, const void *base)
{
    for (const Alloc &a : io.allocs) if (a.base == (const uint8_t *)base) { for (uint8_t s : a.init) if (!s) return false; return true; }
    return false;
}
void scan_pe(ProgIO &io, const jda_pe_arrays &A, uint32_t groups, bool bytes)
{
    for (uint32_t g = 0; g < groups; g++) {
        std::fill(io.lds.begin(), io.lds.end(), 0xEEEEEEEEEEEEEEEEull);        // a workgroup finds nothing in LDS
        std::fill(io.lds_set.begin(), io.lds_set.end(), 0);
        for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_pe_scan(A, g, bytes, false, tid, io);
        for (uint32_t tid = JDA_EN_THREADS; tid-- > 0u;) jda_pe_scan(A, g, bytes, true, tid, io);
    }
}
}

// n jobs over HOST surfaces into HOST files.  0, or the first promise broken (encode_sim.cpp's codes; -42 .. -44: the histogram's LDS, -45: a
// resolve word stored twice, -7x: a record some lane left unwritten), or the status of the argument checks or of a host step.  Optional
// outputs in the call's flat order: cls, run, len (a unit), end (a unit), hist (256 a segment), seginfo (4 a segment: first unit, units,
// header bytes, unstuffed bytes), hdr (every segment's header bytes back to back, hdr_cap bytes of room), info = {blocks, units, segments,
// chunks, unstuffed bytes rounded to chunks}.
extern "C" int encodeprogsim_lanes(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, void *const *dst, const int64_t *cap, int64_t *dst_bytes, int32_t *status,
                                   uint32_t *cls, uint32_t *run, uint32_t *len, uint64_t *end, uint32_t *hist, uint64_t *seginfo, uint8_t *hdr, int64_t hdr_cap, uint64_t *info)
{
    jda_pe_plan_out P;
    int rc = jda_pe_plan_jobs(n, src, bpp, jobs, dst, cap, &P);
    if (rc != JDA_SUCCESS) return rc;
    Run R;
    R.P = P.B;
    setup(R, (uint32_t)bpp);
    ProgIO io;
    static_cast<SimIO &>(io) = R.io;
    io.once_base = NULL; io.once_size = 0;
    const size_t nj = P.pjobs.size(), ns = P.segs.size(), nu = P.n_units, nb = P.B.n_blocks;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
        io.cur = &R.jobs[j];
        jda_en_block(R.A, R.jobs[j], b, io);
    }
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
        io.cur = &R.jobs[j];
        jda_en_length(R.A, R.jobs[j], b, io);
    }
    if (io.err) return io.err;
    io.cur = NULL;
    // the progressive stages' scratch, every array an allocation of its own
    std::vector<uint8_t> m_cls, m_run, m_len, m_end, m_sb, m_hist, m_words, m_hdr, m_u, m_cnt, m_ffend;
    std::vector<jda_pe_seg> segs = P.segs;
    std::vector<jda_pe_job> pjobs = P.pjobs;
    jda_pe_arrays A;
    memset(&A, 0, sizeof(A));
    A.E = R.A; A.segs = segs.data(); A.pjobs = pjobs.data(); A.n_segs = (uint32_t)ns;
    const size_t segs_alloc = io.add(segs.data(), ns * sizeof(jda_pe_seg), false, false);
    io.add(pjobs.data(), nj * sizeof(jda_pe_job), false, false);
    A.cls = aligned<uint32_t>(m_cls, nu * 4); io.add(A.cls, nu * 4, true, true);
    A.run = aligned<uint32_t>(m_run, nu * 4); io.add(A.run, nu * 4, true, true);
    A.len = aligned<uint32_t>(m_len, nu * 4); io.add(A.len, nu * 4, true, true);
    A.end = aligned<uint64_t>(m_end, nu * 8); io.add(A.end, nu * 8, true, true);
    A.sbytes = aligned<uint64_t>(m_sb, ns * 8); io.add(A.sbytes, ns * 8, true, true);
    uint32_t *H = aligned<uint32_t>(m_hist, ns * JDA_PE_TAB_DWORDS * 4); io.add(H, ns * JDA_PE_TAB_DWORDS * 4, true, false, true);      // (zeroed by the call)
    uint32_t *W = aligned<uint32_t>(m_words, ns * JDA_PE_TAB_DWORDS * 4); io.add(W, ns * JDA_PE_TAB_DWORDS * 4, false, false);
    A.words = W;
    for (uint32_t u = 0; u < nu; u++) {
        const uint32_t s = jda_pe_find(A.segs, A.n_segs, u, false, io);
        if (u < segs[s].unit0 || u >= segs[s].unit0 + segs[s].n_units) return -50;
        jda_pe_classify(A, segs[s], R.jobs[segs[s].job], u, io);
    }
    if (io.err) return io.err;
    if (!all_written(io, A.cls)) return -70;
    io.once_base = (const uint8_t *)A.run; io.once_size = nu * 4;
    for (uint32_t u = (uint32_t)nu; u-- > 0u;) jda_pe_resolve(A, segs[jda_pe_find(A.segs, A.n_segs, u, false, io)], u, io);
    io.once_base = NULL;
    if (io.err) return io.err;
    if (!all_written(io, A.run)) return -71;
    for (uint32_t first = 0; first < nu; first += JDA_EN_THREADS) {              // gather: a workgroup = 256 units, its segments in turn
        io.lds_poison();
        const uint32_t last = first + JDA_EN_THREADS - 1u < nu ? first + JDA_EN_THREADS - 1u : (uint32_t)nu - 1u;
        const uint32_t s0 = jda_pe_find(A.segs, A.n_segs, first, false, io), s1 = jda_pe_find(A.segs, A.n_segs, last, false, io);
        for (uint32_t s = s0; s <= s1; s++) {
            const jda_pe_seg &S = segs[s];
            if (S.ss == 0u && S.ah != 0u) continue;
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_pe_clear(tid, io);
            for (uint32_t tid = JDA_EN_THREADS; tid-- > 0u;) {
                const uint32_t u = first + tid;
                if (u < nu && jda_pe_find(A.segs, A.n_segs, u, false, io) == s) jda_pe_count_unit(A, S, R.jobs[S.job], u, io);
            }
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_pe_flush(H + S.tab, tid, io);
        }
    }
    if (io.err) return io.err;
    rc = jda_pe_plan_tables(&P, H);                                              // the host between gather and lengths
    if (rc != JDA_SUCCESS) return rc;
    memcpy(W, P.words.data(), P.words.size() * 4);                               // (the upload of the words)
    for (uint32_t u = 0; u < nu; u++) {
        const jda_pe_seg &S = segs[jda_pe_find(A.segs, A.n_segs, u, false, io)];
        jda_pe_length(A, S, R.jobs[S.job], u, io);
    }
    if (io.err) return io.err;
    if (!all_written(io, A.len)) return -72;
    scan_pe(io, A, (uint32_t)ns, false);
    if (io.err) return io.err;
    if (!all_written(io, A.end) || !all_written(io, A.sbytes)) return -73;
    rc = jda_pe_plan_place(&P, A.sbytes);                                        // the host between the halves
    if (rc != JDA_SUCCESS) return rc;
    segs = P.segs; pjobs = P.pjobs;                                              // (the second upload of the records: same storage, same size)
    (void)segs_alloc;
    uint8_t *hd = aligned<uint8_t>(m_hdr, P.hdr.size()); memcpy(hd, P.hdr.data(), P.hdr.size()); io.add(hd, P.hdr.size(), false, false);
    A.hdr = hd;
    A.E.u = aligned<uint8_t>(m_u, (size_t)P.u_total); io.add(A.E.u, (size_t)P.u_total, true, false, true);
    A.E.ffcnt = aligned<uint32_t>(m_cnt, (size_t)P.n_chunks * 4); io.add(A.E.ffcnt, (size_t)P.n_chunks * 4, true, true);
    A.E.ffend = aligned<uint64_t>(m_ffend, (size_t)P.n_chunks * 8); io.add(A.E.ffend, (size_t)P.n_chunks * 8, true, true);
    io.jobs = R.jobs.data(); io.n_jobs = nj;
    io.written.resize(nj);
    for (size_t i = 0; i < nj; i++) io.written[i].assign((size_t)R.jobs[i].capacity, 0);
    for (uint32_t u = (uint32_t)nu; u-- > 0u;) {
        const jda_pe_seg &S = segs[jda_pe_find(A.segs, A.n_segs, u, false, io)];
        jda_pe_emit(A, S, R.jobs[S.job], u, io);
    }
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t s = jda_pe_find(A.segs, A.n_segs, c, true, io);
        if (c < segs[s].chunk0 || c >= segs[s].chunk0 + segs[s].n_chunks) return -52;
        jda_pe_count(A, segs[s], s, c, io);
    }
    if (io.err) return io.err;
    if (!all_written(io, A.E.ffcnt)) return -74;
    scan_pe(io, A, (uint32_t)nj, true);
    if (io.err) return io.err;
    if (!all_written(io, A.E.ffend)) return -75;
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t s = jda_pe_find(A.segs, A.n_segs, c, true, io);
        io.cur = &R.jobs[segs[s].job];
        jda_pe_write(A, segs[s], R.jobs[segs[s].job], s, c, io);
    }
    if (io.err) return io.err;
    for (size_t i = 0; i < nj; i++) {
        if (!io.rd(&A.E.totals[i].file_bytes, 8)) return -53;
        const uint64_t fb = A.E.totals[i].file_bytes;
        dst_bytes[i] = (int64_t)fb;
        status[i] = fb > R.jobs[i].capacity ? JDA_ERROR_MEMORY : JDA_SUCCESS;
        for (size_t k = 0; k < io.written[i].size(); k++)
            if ((io.written[i][k] != 0) != (status[i] == JDA_SUCCESS && k < fb)) return -32;
    }
    if (cls) memcpy(cls, A.cls, nu * 4);
    if (run) memcpy(run, A.run, nu * 4);
    if (len) memcpy(len, A.len, nu * 4);
    if (end) memcpy(end, A.end, nu * 8);
    if (hist) memcpy(hist, H, ns * JDA_PE_TAB_DWORDS * 4);
    if (seginfo) for (size_t s = 0; s < ns; s++) { seginfo[4 * s] = segs[s].unit0; seginfo[4 * s + 1] = segs[s].n_units; seginfo[4 * s + 2] = segs[s].hdr_len; seginfo[4 * s + 3] = A.sbytes[s]; }
    if (hdr && (uint64_t)hdr_cap >= P.hdr.size()) memcpy(hdr, P.hdr.data(), P.hdr.size());
    if (info) { info[0] = nb; info[1] = nu; info[2] = ns; info[3] = P.n_chunks; info[4] = P.u_total; }
    return 0;
}

// the run-resolution stage alone over n unit records of one scan (cls as the classify stage leaves them), the lanes in reverse order:
// run[n].  0, or -45 (a word stored twice), -71 (one left unwritten), or an access the policy refuses.
extern "C" int encodeprogsim_resolve(const uint32_t *cls, uint32_t n, uint32_t *run)
{
    if (!n) return -60;
    ProgIO io;
    io.cur = NULL; io.bpp = 0; io.jobs = NULL; io.n_jobs = 0; io.err = 0;
    jda_pe_seg S;
    memset(&S, 0, sizeof(S));
    S.n_units = n; S.ss = 1; S.se = 63; S.ah = 1;
    jda_pe_arrays A;
    memset(&A, 0, sizeof(A));
    A.cls = (uint32_t *)cls; A.run = run; A.n_segs = 1; A.segs = &S;
    io.add((void *)cls, (size_t)n * 4, false, false);
    io.add(run, (size_t)n * 4, true, true);
    io.once_base = (const uint8_t *)run; io.once_size = (size_t)n * 4;
    for (uint32_t u = n; u-- > 0u;) jda_pe_resolve(A, S, u, io);
    if (io.err) return io.err;
    return all_written(io, run) ? 0 : -71;
}
// the argument checks of jda_encode_surfaces_progressive (behind its ctx / n == 0 / null-array checks) on pointers that are never followed
extern "C" int encodeprogsim_check(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, void *const *dst, const int64_t *cap)
{
    jda_pe_plan_out P;
    return jda_pe_plan_jobs(n, src, bpp, jobs, dst, cap, &P);
}
extern "C" int encodeprogsim_bound(int w, int h, int sampling, int64_t *bytes) { return jda_pe_bound_bytes(w, h, sampling, bytes); }
