// tests/hostsim/recode_sim.cpp -- TEST INFRASTRUCTURE: the two recode stages on the CPU (jda_rc_extract and jda_rc_from_coef of
// jpegdec_amd/csrc/jda_kernels.hip), and the host plan of jda_recode_images (jda_recode_plan.h).
//
// recodesim_files prepares every source with the product's own front end (a baseline file: jda_prepare, the host pre-scan's index; a
// progressive file: jda_progressive_prepare, dense coefficients), lays its arrays out as jda_upload / jda_coef_upload do -- every array an
// allocation of its own, of the bytes the device allocation has --, makes the plan, and steps every lane of the stage that stands in for
// the blocks stage through the kernels' OWN code (jda_rc_* of jda_device_core.h) the way the GPU runs it: a workgroup of 256 lanes decodes
// into its slots (poisoned before every workgroup), then -- behind the barrier -- every wavefront's lanes store the slots, the lanes in
// REVERSE order.  Memory goes through encode_sim.cpp's IO policy (this file includes it for SimIO, Run, setup and finish): an access lies
// whole inside one allocation and is aligned to its own width, scratch is read only where a lane wrote it, a job's range word changes only
// by atomic OR.  The call then runs every stage behind into the caller's files: the six of a baseline call as encode_sim.cpp steps them, the
// eight of a call with optimised jobs as huffopt_sim.cpp does (gather, the host's tables and headers with the source's DQT segments, the
// second lengths pass), the ten of a progressive call as encode_prog_sim.cpp does -- the host's steps between them as the runtime takes them.
// Outputs: coef and meta of the call's flat block list, the jobs' range words, the headers, the files.
#include "encode_sim.cpp"

#include "../../jpegdec_amd/csrc/jda_recode_plan.h"

extern "C" void jda_image_raw_quant(const jda_image *img, uint16_t *quant_zz, int32_t *adobe);
extern "C" void jda_coef_image_raw_quant(const jda_coef_image *img, uint16_t *quant_zz, uint8_t *q_id, int32_t *adobe);
extern "C" void jda_image_component_ids(const jda_image *img, uint8_t *dc_id, uint8_t *ac_id, uint8_t *q_id);

namespace {
struct Source {
    jda_image *img; jda_coef_image *cimg;
    std::vector<uint8_t> tables, index, dc, scan, coef;      // the device allocation's parts
    Source() : img(NULL), cimg(NULL) {}
};
size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
template <class T> T *place(std::vector<uint8_t> &v, const void *src, size_t bytes, size_t alloc)
{
    T *p = aligned<T>(v, alloc);
    memset(p, 0xEE, alloc);                                   // (what an upload does not write is whatever the pool left there)
    if (bytes) memcpy(p, src, bytes);
    return p;
}
// the IO policy of the stages behind the recode stage in an optimised or progressive call: encode_sim.cpp's, and what huffopt_sim.cpp and
// encode_prog_sim.cpp add to it -- a workgroup's histogram in LDS, poisoned before every workgroup and read or added to only where this
// workgroup cleared it; the histograms in HBM change only by atomic add; a word of the resolve stage is stored once
struct LaterIO : SimIO {
    std::vector<uint32_t> h; std::vector<uint8_t> h_set;
    const uint8_t *once_base; size_t once_size;
    void lds_poison(size_t words) { h.assign(words, 0xEEEEEEEEu); h_set.assign(words, 0); }
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
// a job's file as the write stage left it: its size and status, every byte of a file that fits written once, of one that does not, none
int collect(LaterIO &io, const jda_en_arrays &A, const std::vector<jda_encode_dev_job> &jobs, int64_t *fb, int32_t *st)
{
    for (size_t i = 0; i < jobs.size(); i++) {
        if (!io.rd(&A.totals[i].file_bytes, 8)) return -53;
        const uint64_t b = A.totals[i].file_bytes;
        fb[i] = (int64_t)b;
        st[i] = b > jobs[i].capacity ? JDA_ERROR_MEMORY : JDA_SUCCESS;
        for (size_t k = 0; k < io.written[i].size(); k++)
            if ((io.written[i][k] != 0) != (st[i] == JDA_SUCCESS && k < b)) return -32;
    }
    return 0;
}
void lengths_stage(Run &R, LaterIO &io)
{
    for (uint32_t b = 0; b < R.P.n_blocks; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
        io.cur = &R.jobs[j];
        jda_en_length(R.A, R.jobs[j], b, io);
    }
}
// the eight launches behind the recode stage of a call with optimised jobs, as huffopt_sim.cpp steps them and jda_runtime.cpp orders them
int finish_optimised(Run &R, LaterIO &io, int64_t *fb, int32_t *st)
{
    jda_encode_plan_out &P = R.P;
    const size_t nj = P.jobs.size(), hist_bytes = (size_t)P.n_opt * JDA_EN_HUFF_DWORDS * 4;
    const uint32_t nb = P.n_blocks;
    std::vector<uint8_t> hist_mem;
    uint32_t *hist = aligned<uint32_t>(hist_mem, hist_bytes);                   // (zeroed by the call)
    io.add(hist, hist_bytes, true, false, true);
    lengths_stage(R, io);
    if (io.err) return io.err;
    for (uint32_t first = 0; first < nb; first += JDA_EN_THREADS) {              // gather: a workgroup = 256 blocks, its jobs in turn
        io.lds_poison(JDA_EN_HUFF_DWORDS);
        const uint32_t last = first + JDA_EN_THREADS - 1u < nb ? first + JDA_EN_THREADS - 1u : nb - 1u;
        const uint32_t j0 = jda_en_find_block(R.A.jobs, R.A.n_jobs, first, io), j1 = jda_en_find_block(R.A.jobs, R.A.n_jobs, last, io);
        for (uint32_t j = j0; j <= j1; j++) {
            const uint32_t hoff = io.ld32(&R.A.jobs[j].hist_off);
            if (hoff == JDA_EN_NO_HIST) continue;
            io.cur = &R.jobs[j];
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_ho_clear(tid, io);
            for (uint32_t tid = JDA_EN_THREADS; tid-- > 0u;) {
                const uint32_t b = first + tid;
                if (b < nb && jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io) == j) jda_ho_count(R.A, R.jobs[j], b, io);
            }
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_ho_flush(hist + hoff, tid, io);
        }
    }
    if (io.err) return io.err;
    int rc = jda_encode_plan_tables(&P, hist);                                   // the host between gather and the second lengths pass: tables, words, headers
    if (rc != JDA_SUCCESS) return rc;
    memcpy(R.huff.data(), P.huff.data(), P.huff.size() * 4);
    memcpy((uint8_t *)R.A.hdr, P.hdr.data(), P.hdr.size());
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
        io.cur = &R.jobs[j];
        jda_ho_length(R.A, R.jobs[j], b, io);
    }
    if (io.err) return io.err;
    auto scan_jobs = [&R, &io](bool bytes) {
        for (uint32_t j = 0; j < R.A.n_jobs; j++) {
            std::fill(io.lds.begin(), io.lds.end(), 0xEEEEEEEEEEEEEEEEull);
            std::fill(io.lds_set.begin(), io.lds_set.end(), 0);
            io.cur = &R.jobs[j];
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_en_scan_job(R.A, R.jobs[j], j, bytes, false, tid, io);
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_en_scan_job(R.A, R.jobs[j], j, bytes, true, tid, io);
        }
    };
    scan_jobs(false);
    if (io.err) return io.err;
    std::vector<jda_encode_totals> tot(nj);
    for (size_t i = 0; i < nj; i++) { if (!io.rd(&R.A.totals[i].u_bytes, 8)) return -51; tot[i] = R.A.totals[i]; }
    for (size_t i = 0; i < nj; i++) P.jobs[i].capacity = R.jobs[i].capacity;      // (a job out of range: capacity 0, as the runtime sends it up again)
    rc = jda_encode_plan_place(&P, tot.data());
    if (rc != JDA_SUCCESS) return rc;
    R.jobs = P.jobs;
    R.A.jobs = R.jobs.data();
    io.allocs[R.jobs_alloc].base = (uint8_t *)R.jobs.data();
    R.A.u = aligned<uint8_t>(R.u, (size_t)P.u_total); io.add(R.A.u, (size_t)P.u_total, true, false, true);
    R.A.ffcnt = aligned<uint32_t>(R.ffcnt, (size_t)P.n_chunks * 4); io.add(R.A.ffcnt, (size_t)P.n_chunks * 4, true, true);
    R.A.ffend = aligned<uint64_t>(R.ffend, (size_t)P.n_chunks * 8); io.add(R.A.ffend, (size_t)P.n_chunks * 8, true, true);
    io.jobs = R.jobs.data(); io.n_jobs = nj;
    io.written.resize(nj);
    for (size_t i = 0; i < nj; i++) io.written[i].assign((size_t)R.jobs[i].capacity, 0);
    for (uint32_t b = 0; b < nb; b++) {
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
    scan_jobs(true);
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t j = jda_en_find_chunk(R.A.jobs, R.A.n_jobs, c, io);
        io.cur = &R.jobs[j];
        jda_en_write(R.A, R.jobs[j], j, c, io);
    }
    if (io.err) return io.err;
    return collect(io, R.A, R.jobs, fb, st);
}
bool all_written(LaterIO &io, const void *base)
{
    for (const Alloc &a : io.allocs) if (a.base == (const uint8_t *)base) { for (uint8_t s : a.init) if (!s) return false; return true; }
    return false;
}
void scan_pe(LaterIO &io, const jda_pe_arrays &A, uint32_t groups, bool bytes)
{
    for (uint32_t g = 0; g < groups; g++) {
        std::fill(io.lds.begin(), io.lds.end(), 0xEEEEEEEEEEEEEEEEull);
        std::fill(io.lds_set.begin(), io.lds_set.end(), 0);
        for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_pe_scan(A, g, bytes, false, tid, io);
        for (uint32_t tid = JDA_EN_THREADS; tid-- > 0u;) jda_pe_scan(A, g, bytes, true, tid, io);
    }
}
// the ten launches behind the recode stage of a progressive call, as encode_prog_sim.cpp steps them and jda_encode_progressive.cpp orders them;
// P: the call's plan (P.B: its job records, DQT segments and table ids), hdr_out: every scan's header bytes back to back
int finish_progressive(Run &R, jda_pe_plan_out &P, LaterIO &io, int64_t *fb, int32_t *st, std::vector<uint8_t> *hdr_out)
{
    const size_t nj = P.pjobs.size(), ns = P.segs.size(), nu = P.n_units;
    lengths_stage(R, io);
    if (io.err) return io.err;
    io.cur = NULL;
    std::vector<uint8_t> m_cls, m_run, m_len, m_end, m_sb, m_hist, m_words, m_hdr, m_u, m_cnt, m_ffend;
    std::vector<jda_pe_seg> segs = P.segs;
    std::vector<jda_pe_job> pjobs = P.pjobs;
    jda_pe_arrays A;
    memset(&A, 0, sizeof(A));
    A.E = R.A; A.segs = segs.data(); A.pjobs = pjobs.data(); A.n_segs = (uint32_t)ns;
    io.add(segs.data(), ns * sizeof(jda_pe_seg), false, false);
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
    if (!all_written(io, A.cls)) return -72;
    io.once_base = (const uint8_t *)A.run; io.once_size = nu * 4;
    for (uint32_t u = (uint32_t)nu; u-- > 0u;) jda_pe_resolve(A, segs[jda_pe_find(A.segs, A.n_segs, u, false, io)], u, io);
    io.once_base = NULL;
    if (io.err) return io.err;
    if (!all_written(io, A.run)) return -73;
    for (uint32_t first = 0; first < nu; first += JDA_EN_THREADS) {              // gather: a workgroup = 256 units, its segments in turn
        io.lds_poison(JDA_PE_TAB_DWORDS);
        const uint32_t last = first + JDA_EN_THREADS - 1u < nu ? first + JDA_EN_THREADS - 1u : (uint32_t)nu - 1u;
        const uint32_t s0 = jda_pe_find(A.segs, A.n_segs, first, false, io), s1 = jda_pe_find(A.segs, A.n_segs, last, false, io);
        for (uint32_t s = s0; s <= s1; s++) {
            const jda_pe_seg &Sg = segs[s];
            if (Sg.ss == 0u && Sg.ah != 0u) continue;
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_pe_clear(tid, io);
            for (uint32_t tid = JDA_EN_THREADS; tid-- > 0u;) {
                const uint32_t u = first + tid;
                if (u < nu && jda_pe_find(A.segs, A.n_segs, u, false, io) == s) jda_pe_count_unit(A, Sg, R.jobs[Sg.job], u, io);
            }
            for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_pe_flush(H + Sg.tab, tid, io);
        }
    }
    if (io.err) return io.err;
    int rc = jda_pe_plan_tables(&P, H);                                          // the host between gather and lengths: tables, words, headers with the source's DQT segments
    if (rc != JDA_SUCCESS) return rc;
    if (P.hdr.size() > jda_pe_hdr_room(P)) return -74;                           // (the room the runtime keeps for them on the device)
    memcpy(W, P.words.data(), P.words.size() * 4);
    for (uint32_t u = 0; u < nu; u++) {
        const jda_pe_seg &Sg = segs[jda_pe_find(A.segs, A.n_segs, u, false, io)];
        jda_pe_length(A, Sg, R.jobs[Sg.job], u, io);
    }
    if (io.err) return io.err;
    if (!all_written(io, A.len)) return -75;
    scan_pe(io, A, (uint32_t)ns, false);
    if (io.err) return io.err;
    if (!all_written(io, A.end) || !all_written(io, A.sbytes)) return -76;
    rc = jda_pe_plan_place(&P, A.sbytes);                                        // the host between the halves
    if (rc != JDA_SUCCESS) return rc;
    segs = P.segs; pjobs = P.pjobs;                                              // (the second upload of the records: same storage, same size)
    uint8_t *hd = aligned<uint8_t>(m_hdr, jda_pe_hdr_room(P)); memcpy(hd, P.hdr.data(), P.hdr.size()); io.add(hd, jda_pe_hdr_room(P), false, false);
    A.hdr = hd;
    A.E.u = aligned<uint8_t>(m_u, (size_t)P.u_total); io.add(A.E.u, (size_t)P.u_total, true, false, true);
    A.E.ffcnt = aligned<uint32_t>(m_cnt, (size_t)P.n_chunks * 4); io.add(A.E.ffcnt, (size_t)P.n_chunks * 4, true, true);
    A.E.ffend = aligned<uint64_t>(m_ffend, (size_t)P.n_chunks * 8); io.add(A.E.ffend, (size_t)P.n_chunks * 8, true, true);
    io.jobs = R.jobs.data(); io.n_jobs = nj;
    io.written.resize(nj);
    for (size_t i = 0; i < nj; i++) io.written[i].assign((size_t)R.jobs[i].capacity, 0);
    for (uint32_t u = (uint32_t)nu; u-- > 0u;) {
        const jda_pe_seg &Sg = segs[jda_pe_find(A.segs, A.n_segs, u, false, io)];
        jda_pe_emit(A, Sg, R.jobs[Sg.job], u, io);
    }
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t s = jda_pe_find(A.segs, A.n_segs, c, true, io);
        if (c < segs[s].chunk0 || c >= segs[s].chunk0 + segs[s].n_chunks) return -52;
        jda_pe_count(A, segs[s], s, c, io);
    }
    if (io.err) return io.err;
    if (!all_written(io, A.E.ffcnt)) return -77;
    scan_pe(io, A, (uint32_t)nj, true);
    if (io.err) return io.err;
    if (!all_written(io, A.E.ffend)) return -78;
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t s = jda_pe_find(A.segs, A.n_segs, c, true, io);
        io.cur = &R.jobs[segs[s].job];
        jda_pe_write(A, segs[s], R.jobs[segs[s].job], s, c, io);
    }
    if (io.err) return io.err;
    if (hdr_out) *hdr_out = P.hdr;
    return collect(io, A.E, R.jobs, fb, st);
}
// the source of one file: its host record, and its arrays added to the IO policy's allocations
int open_source(const uint8_t *jpeg, int32_t len, int sparse, Source &S, jda_recode_src_host &H, SimIO &io)
{
    memset(&H, 0, sizeof(H));
    jda_image_info I;
    int32_t err = jda_parse(jpeg, len, &I);
    if (err != JDA_SUCCESS) return err;
    if (I.jpeg_type == 1) {
        S.cimg = jda_progressive_prepare(jpeg, len, &err);
        if (!S.cimg) return err;
        uint32_t nb = 0;
        const int16_t *c = jda_coef_image_coefficients(S.cimg, &nb);
        int32_t adobe = 0;
        jda_coef_image_raw_quant(S.cimg, &H.quant[0][0], H.q_id, &adobe);
        H.kind = sparse ? (int)JDA_RC_SPARSE : (int)JDA_RC_COEF; H.info = *jda_coef_image_get_info(S.cimg); H.adobe = adobe;
        H.dev.coef = place<int16_t>(S.coef, c, (size_t)nb * 128, align16((size_t)nb * 128));
        io.add((void *)H.dev.coef, align16((size_t)nb * 128), false, false);
        return JDA_SUCCESS;
    }
    S.img = jda_prepare(jpeg, len, &err);
    if (!S.img) return err;
    H.kind = JDA_RC_IMAGE; H.info = *jda_image_get_info(S.img);
    const size_t nb = (size_t)H.info.mcus_x * H.info.mcus_y * H.info.blocks_per_mcu;
    uint32_t scan_len = 0, tb = 0;
    const uint8_t *scan = jda_image_scan(S.img, &scan_len);
    const uint8_t *tables = jda_image_tables(S.img, &tb);
    const uint32_t *index = jda_image_block_index(S.img, &H.n_mcus_ok);
    const int16_t *dc = jda_image_block_dc(S.img);
    uint16_t q[4][64];
    int32_t adobe = 0;
    uint8_t dc_id[3], ac_id[3], q_id[3];
    jda_image_raw_quant(S.img, &q[0][0], &adobe);
    jda_image_component_ids(S.img, dc_id, ac_id, q_id);
    H.adobe = adobe;
    for (int c = 0; c < 3; c++) { H.q_id[c] = q_id[c]; memcpy(H.quant[c], q[q_id[c] & 3], 128); H.dev.ac_id[c] = ac_id[c]; }
    H.dev.tables = place<uint8_t>(S.tables, tables, tb, align16(tb));
    H.dev.blk_index = place<uint32_t>(S.index, index, (nb + 1) * 4, align16((nb + 1) * 4));
    H.dev.blk_dc = place<int16_t>(S.dc, dc, nb * 2, align16(nb * 2));
    H.dev.scan = place<uint8_t>(S.scan, scan, (size_t)scan_len + JDA_SCAN_PAD, align16((size_t)scan_len + JDA_SCAN_PAD));
    H.dev.scan_len = scan_len;
    io.add((void *)H.dev.tables, align16(tb), false, false);
    io.add((void *)H.dev.blk_index, align16((nb + 1) * 4), false, false);
    io.add((void *)H.dev.blk_dc, align16(nb * 2), false, false);
    io.add((void *)H.dev.scan, align16((size_t)scan_len + JDA_SCAN_PAD), false, false);
    return JDA_SUCCESS;
}
}

// n files recoded into HOST files.  form / ri: a job each (ri: -1 the source's); sparse: NULL, or != 0 where a progressive source is to count
// as a sparse coefficient image.  0, or the first promise broken (encode_sim.cpp's codes; -71: a block of the list that no lane
// stored), or what the call's checks give.  status: a job each, as jda_recode_images sets it.
// Optional outputs in the flat order of the jobs that run: coef (64 a block), meta (a block); bad: a word a job of the CALL (0 where it
// did not run); hdr / hdr_len: the headers of the jobs that run, back to back (baseline jobs; hdr_cap bytes of room); info = {blocks, jobs
// that run, launches of extract, launches of from_coef}.
extern "C" int recodesim_files(int n, const uint8_t *const *jpegs, const int32_t *lens, const int32_t *form, const int32_t *ri, const int32_t *sparse, void *const *dst,
                               const int64_t *cap, int64_t *dst_bytes, int32_t *status, int16_t *coef, uint32_t *meta, uint32_t *bad, uint8_t *hdr, int64_t hdr_cap,
                               int64_t *hdr_len, uint64_t *info)
{
    Run R;
    R.io.err = 0;
    std::vector<Source> S((size_t)n);
    std::vector<jda_recode_src_host> hosts((size_t)n);
    std::vector<jda_recode_job> jobs((size_t)n);
    SimIO sources;                                            // (setup() clears the run's allocations: the sources' are added behind it)
    sources.err = 0;
    int rc = JDA_SUCCESS;
    for (int i = 0; i < n && rc == JDA_SUCCESS; i++) {
        rc = open_source(jpegs[i], lens[i], sparse ? sparse[i] : 0, S[(size_t)i], hosts[(size_t)i], sources);
        const jda_recode_job J = { form[i], ri[i], 0, 0 };
        jobs[(size_t)i] = J;
        dst_bytes[i] = 0;
    }
    jda_recode_plan_out plan;
    if (rc == JDA_SUCCESS) rc = jda_recode_plan_jobs(n, hosts.data(), jobs.data(), dst, cap, status, &plan);
    int out = rc;
    if (rc == JDA_SUCCESS && !plan.src.empty()) {
        R.P = plan.P.B;
        if (R.P.hdr.empty()) R.P.hdr.push_back(0);                                  // (a progressive call's headers are made behind its gather stage: setup() copies from a vector that has storage)
        setup(R, 0u);
        for (const Alloc &a : sources.allocs) R.io.allocs.push_back(a);
        const size_t nj = plan.src.size(), nb = R.P.n_blocks;
        std::vector<uint8_t> src_mem, bad_mem, slot_mem;
        jda_rc_src *d_src = place<jda_rc_src>(src_mem, plan.src.data(), nj * sizeof(jda_rc_src), nj * sizeof(jda_rc_src));
        uint32_t *d_bad = aligned<uint32_t>(bad_mem, nj * 4);                      // (zeroed by the call)
        R.io.add(d_src, nj * sizeof(jda_rc_src), false, false);
        R.io.add(d_bad, nj * 4, true, false, true);
        uint8_t *slots = aligned<uint8_t>(slot_mem, (size_t)JDA_EN_THREADS * JDA_COEF_STRIDE);
        SimIO &io = R.io;
        uint64_t n_extract = 0, n_coef = 0;
        if (plan.any_image) {
            n_extract = 1;
            for (uint32_t first = 0; first < nb; first += JDA_EN_THREADS) {
                memset(slots, 0xEE, (size_t)JDA_EN_THREADS * JDA_COEF_STRIDE);      // a workgroup finds nothing in LDS
                for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) {
                    const uint32_t b = first + tid;
                    uint8_t *slot = slots + tid * JDA_COEF_STRIDE;
                    uint32_t valid = 0;
                    if (b < nb) {
                        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
                        if (b < R.jobs[j].block0 || b >= R.jobs[j].block0 + R.jobs[j].n_blocks) return -50;
                        if (io.ld32(&d_src[j].kind) == JDA_RC_IMAGE) { jda_rc_extract_block(R.A, R.jobs[j], d_src[j], j, b, slot, d_bad, io); valid = 1; }
                    }
                    memcpy(slot + JDA_RC_SLOT_VALID, &valid, 4);
                }
                for (uint32_t wave = 0; wave < JDA_EN_THREADS / 64u; wave++)
                    for (uint32_t lane = 64u; lane-- > 0u;) jda_rc_store(R.A, first + wave * 64u, slots + wave * 64u * JDA_COEF_STRIDE, lane, io);
            }
        }
        if (plan.any_coef) {
            n_coef = 1;
            for (uint32_t b = 0; b < nb; b++) {
                const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
                if (io.ld32(&d_src[j].kind) == JDA_RC_COEF) jda_rc_coef_block(R.A, R.jobs[j], d_src[j], j, b, d_bad, io);
            }
        }
        if (io.err) return io.err;
        for (size_t k = 0; k < nb * 128; k++) if (!io.allocs[3].init[k]) return -71;      // (3 = coef, 4 = meta: setup()'s order)
        for (size_t k = 0; k < nb * 4; k++) if (!io.allocs[4].init[k]) return -71;
        if (coef) memcpy(coef, R.A.coef, nb * 128);
        if (meta) memcpy(meta, R.A.meta, nb * 4);
        for (int i = 0; i < n; i++) bad[i] = 0;
        for (size_t k = 0; k < nj; k++) {
            bad[plan.job_of[k]] = d_bad[k];
            if (d_bad[k]) { status[plan.job_of[k]] = JDA_UNSUPPORTED_FEATURE; R.P.jobs[k].capacity = 0; R.jobs[k].capacity = 0; }
        }
        if (info) { info[0] = nb; info[1] = nj; info[2] = n_extract; info[3] = n_coef; }
        std::vector<int64_t> fb(nj);
        std::vector<int32_t> st(nj);
        std::vector<uint8_t> headers;
        if (!plan.progressive && R.P.n_opt == 0) {
            out = finish(R, fb.data(), st.data(), NULL, NULL, NULL, NULL, 0);
            headers = R.P.hdr;
        } else {
            LaterIO later;
            static_cast<SimIO &>(later) = R.io;
            later.once_base = NULL; later.once_size = 0;
            if (plan.progressive) out = finish_progressive(R, plan.P, later, fb.data(), st.data(), &headers);
            else { out = finish_optimised(R, later, fb.data(), st.data()); headers = R.P.hdr; }
        }
        if (out == 0)
            for (size_t k = 0; k < nj; k++) {
                const int i = plan.job_of[k];
                if (d_bad[k]) continue;
                dst_bytes[i] = fb[k]; status[i] = st[k];
            }
        if (hdr_len) *hdr_len = (int64_t)headers.size();
        if (hdr && (int64_t)headers.size() <= hdr_cap && !headers.empty()) memcpy(hdr, headers.data(), headers.size());
    } else if (info) { info[0] = info[1] = info[2] = info[3] = 0; }
    for (Source &s : S) { if (s.img) jda_image_free(s.img); if (s.cimg) jda_coef_image_free(s.cimg); }
    return out;
}

// the checks of jda_recode_images on sources described by hand (pointers that are never followed): kind, info, quant, q_id, adobe, n_mcus_ok
extern "C" int recodesim_check(int n, const jda_recode_src_host *hosts, const jda_recode_job *jobs, void *const *dst, const int64_t *cap, int32_t *status)
{
    jda_recode_plan_out plan;
    return jda_recode_plan_jobs(n, hosts, jobs, dst, cap, status, &plan);
}
extern "C" int recodesim_bound(const jda_image_info *info, int form, int ri, int64_t *bytes) { return jda_recode_bound_bytes(info, form, ri, bytes); }
// the DQT segments of a source; returns their length, or -1 where the plan refuses the tables
extern "C" int recodesim_dqt(int nc, const uint16_t *quant, const uint8_t *q_id, uint8_t *out, int cap)
{
    std::vector<uint8_t> o;
    if (!jda_recode_dqt(nc, (const uint16_t(*)[64])quant, q_id, o)) return -1;
    if ((int)o.size() <= cap) memcpy(out, o.data(), o.size());
    return (int)o.size();
}
// the encoder's own headers through the generalised builders: what they were before (tests/test_recode_cpu.py holds them to encodesim_header)
extern "C" int recodesim_quality_header(int w, int h, int sampling, int quality, int ri, uint8_t *out, int cap)
{
    std::vector<uint8_t> o;
    jda_encode_header(w, h, sampling, quality, ri, o);
    if ((int)o.size() <= cap) memcpy(out, o.data(), o.size());
    return (int)o.size();
}
