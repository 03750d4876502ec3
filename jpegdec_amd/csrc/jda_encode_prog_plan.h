// jda_encode_prog_plan.h -- HOST: jda_encode_surfaces_progressive's arguments checked and turned into the segment records (one scan of one
// job each) on top of the baseline plan's job and quantiser records (jda_encode_plan.h), and -- once the device has counted the symbols --
// every scan's Huffman table, code words and header bytes, and -- once it has summed the lengths -- the place of every scan's unstuffed
// data and chunks.  No HIP in here: the runtime (jda_runtime.cpp) and the CPU tests (tests/hostsim/encode_prog_sim.cpp) run the same code.
// The definition: DESIGN.md 5.13 rules 10 to 14; the stages: jda_pe_* in jda_device_core.h.
#ifndef JDA_ENCODE_PROG_PLAN_H
#define JDA_ENCODE_PROG_PLAN_H

#include "jda_encode_plan.h"

// libjpeg's jpeg_simple_progression (jcparam.c): component (JDA_PE_ALL: every component, interleaved), Ss, Se, Ah, Al
struct jda_pe_scan_def { uint8_t comp, ss, se, ah, al; };
static const jda_pe_scan_def jda_pe_script_colour[10] = { { JDA_PE_ALL, 0, 0, 0, 1 }, { 0, 1, 5, 0, 2 }, { 2, 1, 63, 0, 1 }, { 1, 1, 63, 0, 1 }, { 0, 6, 63, 0, 2 },
                                                          { 0, 1, 63, 2, 1 }, { JDA_PE_ALL, 0, 0, 1, 0 }, { 2, 1, 63, 1, 0 }, { 1, 1, 63, 1, 0 }, { 0, 1, 63, 1, 0 } };
static const jda_pe_scan_def jda_pe_script_gray[6] = { { JDA_PE_ALL, 0, 0, 0, 1 }, { 0, 1, 5, 0, 2 }, { 0, 6, 63, 0, 2 }, { 0, 1, 63, 2, 1 }, { JDA_PE_ALL, 0, 0, 1, 0 }, { 0, 1, 63, 1, 0 } };

struct jda_pe_plan_out {
    jda_encode_plan_out B;                   // jobs, quant, the Annex K words (blocks and lengths run as in a baseline call)
    std::vector<jda_pe_seg> segs;
    std::vector<jda_pe_job> pjobs;
    std::vector<uint32_t> words;             // JDA_PE_TAB_DWORDS a segment (zeros until jda_pe_plan_tables)
    std::vector<uint8_t> hdr;                // every segment's header bytes, back to back (jda_pe_plan_tables)
    uint32_t n_units, n_chunks;              // n_chunks: after jda_pe_plan_place
    uint64_t u_total;
    std::vector<uint32_t> hdr_grow;          // a job (empty in a call over pixels): the bytes its own DQT segments add to JDA_PE_FILE_HDR (jda_recode_plan.h)
};
static inline uint32_t jda_pe_scans(int32_t sampling) { return sampling == JDA_ENCODE_GRAY ? 6u : 10u; }
// the room the headers of a call can take
static inline size_t jda_pe_hdr_room(const jda_pe_plan_out &P)
{
    size_t grow = 0;
    for (uint32_t g : P.hdr_grow) grow += g;
    return P.segs.size() * JDA_PE_SCAN_HDR + P.pjobs.size() * JDA_PE_FILE_HDR + grow;
}

// The largest file the image can become (DESIGN.md 5.13 rule 14): every block at JDA_PE_BLOCK_BITS over all its scans, every byte
// stuffed, every scan padded to a byte, every scan's header at JDA_PE_SCAN_HDR.
static inline int jda_pe_bound_bytes(int32_t w, int32_t h, int32_t sampling, int64_t *bytes)
{
    uint32_t cx, cy, bpm;
    uint64_t blocks, ints;
    if (!bytes) return JDA_INVALID_PARAMETER;
    *bytes = 0;
    if (!jda_encode_counts(w, h, sampling, 0, &cx, &cy, &bpm, &blocks, &ints)) return JDA_INVALID_PARAMETER;
    const uint64_t ns = jda_pe_scans(sampling);
    *bytes = (int64_t)(JDA_PE_FILE_HDR + ns * JDA_PE_SCAN_HDR + 2u * ((blocks * JDA_PE_BLOCK_BITS + 7u) / 8u + ns) + 2u);
    return JDA_SUCCESS;
}

static inline int jda_pe_plan_segments(jda_pe_plan_out *plan);
// n >= 1 jobs: the baseline plan's checks and records, then a segment per scan.  A restart interval is refused (JDA_INVALID_PARAMETER), a
// job of more than JDA_EN_OPT_MAX_BLOCKS blocks too (JDA_UNSUPPORTED_FEATURE: a symbol count could pass libjpeg's 10^9).
static inline int jda_pe_plan_jobs(int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, void *const *dst, const int64_t *dst_capacity,
                                   jda_pe_plan_out *plan)
{
    plan->segs.clear(); plan->pjobs.clear(); plan->words.clear(); plan->hdr.clear(); plan->n_units = plan->n_chunks = 0; plan->u_total = 0; plan->hdr_grow.clear();
    if (n > 0 && jobs) for (int i = 0; i < n; i++) if (jobs[i].restart_interval != 0) return JDA_INVALID_PARAMETER;
    const int rc = jda_encode_plan_jobs_ex(n, src, bytes_per_pixel, jobs, NULL, dst, dst_capacity, &plan->B);
    if (rc != JDA_SUCCESS) return rc;
    return jda_pe_plan_segments(plan);
}
// a segment per scan of every job of plan->B (the job records are made: by jda_encode_plan_jobs_ex, or by a recode's plan)
static inline int jda_pe_plan_segments(jda_pe_plan_out *plan)
{
    plan->segs.clear(); plan->pjobs.clear(); plan->words.clear(); plan->hdr.clear(); plan->n_units = plan->n_chunks = 0; plan->u_total = 0;
    uint64_t units = 0;
    for (size_t i = 0; i < plan->B.jobs.size(); i++) {
        const jda_encode_dev_job &J = plan->B.jobs[i];
        if (J.n_blocks > JDA_EN_OPT_MAX_BLOCKS) return JDA_UNSUPPORTED_FEATURE;
        const uint32_t ns = J.nc == 1u ? 6u : 10u;
        const jda_pe_scan_def *script = J.nc == 1u ? jda_pe_script_gray : jda_pe_script_colour;
        jda_pe_job pj = { (uint32_t)plan->segs.size(), ns, 0u, 0u };
        plan->pjobs.push_back(pj);
        for (uint32_t k = 0; k < ns; k++) {
            jda_pe_seg S;
            memset(&S, 0, sizeof(S));
            S.job = (uint32_t)i; S.comp = script[k].comp; S.ss = script[k].ss; S.se = script[k].se; S.ah = script[k].ah; S.al = script[k].al;
            S.wbc = S.comp == 0u ? J.wb : J.cx;                              // (a chroma component's own extent is the MCU grid)
            S.n_units = S.comp == JDA_PE_ALL ? J.n_blocks : S.comp == 0u ? J.wb * J.hb : J.cx * J.cy;
            if (units + S.n_units > 0x7fffffffull) return JDA_UNSUPPORTED_FEATURE;   // (the flat unit list is indexed by 32 bits)
            S.unit0 = (uint32_t)units; units += S.n_units;
            S.tab = (uint32_t)plan->segs.size() * JDA_PE_TAB_DWORDS;
            plan->segs.push_back(S);
        }
    }
    if (plan->segs.size() * (size_t)JDA_PE_TAB_DWORDS > 0x7fffffffull) return JDA_UNSUPPORTED_FEATURE;
    plan->words.assign(plan->segs.size() * (size_t)JDA_PE_TAB_DWORDS, 0u);
    plan->n_units = (uint32_t)units;
    return JDA_SUCCESS;
}
static inline void jda_pe_put_dht(std::vector<uint8_t> &o, uint32_t tc_th, const jda_encode_table &T)
{
    std::vector<uint8_t> p;
    p.push_back((uint8_t)tc_th);
    p.insert(p.end(), T.bits, T.bits + 16);
    p.insert(p.end(), T.vals, T.vals + T.n_vals);
    jda_encode_put_seg(o, 0xc4, p);
}
// code words of one table at w[vals]
static inline void jda_pe_table_words(const jda_encode_table &T, uint32_t *w)
{
    uint32_t code = 0, k = 0;
    for (uint32_t len = 1; len <= 16u; len++, code <<= 1)
        for (uint32_t i = 0; i < T.bits[len - 1u]; i++, k++, code++) w[T.vals[k]] = (len << 16) | code;
}
// everything in front of the first scan's DHTs: SOI, JFIF APP0, a DQT per table, SOF2
static inline void jda_pe_file_header(int32_t w, int32_t h, const jda_encode_dev_job &J, int32_t quality, std::vector<uint8_t> &o)
{
    const uint8_t tq[3] = { 0, 1, 1 };
    std::vector<uint8_t> dqt;
    jda_encode_quality_dqt(quality, (int)J.nc, dqt);
    jda_encode_header_front(w, h, (int)J.nc, (int)J.hs, (int)J.vs, dqt.data(), dqt.size(), tq, 0xc2, o);
}
// between gather and lengths: hist = the call's histograms as the device counted them (the word tables' layout).  Every scan gets the
// table(s) of its own counts (libjpeg's jpeg_gen_optimal_table), its code words and its header: a DHT segment per table, then its SOS.
// JDA_UNSUPPORTED_FEATURE: a histogram that libjpeg itself refuses.
static inline int jda_pe_plan_tables(jda_pe_plan_out *plan, const uint32_t *hist)
{
    plan->hdr.clear();
    std::fill(plan->words.begin(), plan->words.end(), 0u);
    for (size_t si = 0; si < plan->segs.size(); si++) {
        jda_pe_seg &S = plan->segs[si];
        const jda_encode_dev_job &J = plan->B.jobs[S.job];
        const uint32_t *H = hist + S.tab;
        uint32_t *W = plan->words.data() + S.tab;
        std::vector<uint8_t> o;
        const bool first = si == plan->pjobs[S.job].seg0;
        if (first && plan->B.dqt.empty()) jda_pe_file_header((int32_t)J.w, (int32_t)J.h, J, plan->B.quality[S.job], o);
        else if (first) jda_encode_header_front((int32_t)J.w, (int32_t)J.h, (int)J.nc, (int)J.hs, (int)J.vs, plan->B.dqt[S.job].data(), plan->B.dqt[S.job].size(),
                                                plan->B.tq.data() + 3 * S.job, 0xc2, o);
        if (S.ss == 0u && S.ah == 0u) {
            for (uint32_t t = 0; t < (J.nc == 1u ? 1u : 2u); t++) {
                uint32_t freq[256];
                memset(freq, 0, sizeof(freq));
                memcpy(freq, H + t * 16u, 16 * sizeof(uint32_t));
                jda_encode_table T;
                if (!jda_encode_optimal_table(freq, T.bits, T.vals, &T.n_vals)) return JDA_UNSUPPORTED_FEATURE;
                jda_pe_table_words(T, W + t * 16u);
                jda_pe_put_dht(o, t, T);
            }
        } else if (S.ss != 0u) {
            jda_encode_table T;
            if (!jda_encode_optimal_table(H, T.bits, T.vals, &T.n_vals)) return JDA_UNSUPPORTED_FEATURE;
            jda_pe_table_words(T, W);
            jda_pe_put_dht(o, 0x10u | (S.comp == 0u ? 0u : 1u), T);
        }
        std::vector<uint8_t> sos;
        if (S.comp == JDA_PE_ALL) {
            sos.push_back((uint8_t)J.nc);
            for (uint32_t c = 0; c < J.nc; c++) { sos.push_back((uint8_t)(1u + c)); sos.push_back((uint8_t)(c && !S.ah ? 0x10 : 0x00)); }
        } else { sos.push_back(1); sos.push_back((uint8_t)(1u + S.comp)); sos.push_back((uint8_t)(S.comp ? 0x01 : 0x00)); }
        sos.push_back((uint8_t)S.ss); sos.push_back((uint8_t)S.se); sos.push_back((uint8_t)((S.ah << 4) | S.al));
        jda_encode_put_seg(o, 0xda, sos);
        if (o.size() > JDA_PE_SCAN_HDR + (first ? JDA_PE_FILE_HDR + (plan->hdr_grow.empty() ? 0u : plan->hdr_grow[S.job]) : 0u)) return JDA_ERROR_MEMORY;      // (never: at most 256 symbols a table)
        S.hdr_off = (uint32_t)plan->hdr.size(); S.hdr_len = (uint32_t)o.size();
        plan->hdr.insert(plan->hdr.end(), o.begin(), o.end());
    }
    return JDA_SUCCESS;
}
// sbytes[s] = the bytes of segment s's unstuffed data (the device's sums).  JDA_UNSUPPORTED_FEATURE past 2^31 chunks.
static inline int jda_pe_plan_place(jda_pe_plan_out *plan, const uint64_t *sbytes)
{
    uint64_t chunks = 0, u = 0;
    for (size_t j = 0; j < plan->pjobs.size(); j++) {
        jda_pe_job &pj = plan->pjobs[j];
        pj.chunk0 = (uint32_t)chunks;
        for (uint32_t k = 0; k < pj.n_segs; k++) {
            jda_pe_seg &S = plan->segs[pj.seg0 + k];
            const uint64_t uc = (sbytes[pj.seg0 + k] + JDA_EN_CHUNK - 1u) / JDA_EN_CHUNK;
            S.h_chunks = (S.hdr_len + JDA_EN_CHUNK - 1u) / JDA_EN_CHUNK;
            if (chunks + S.h_chunks + uc > 0x7fffffffull) return JDA_UNSUPPORTED_FEATURE;
            S.chunk0 = (uint32_t)chunks; S.n_chunks = S.h_chunks + (uint32_t)uc; S.u_off = u;
            chunks += S.n_chunks; u += uc * JDA_EN_CHUNK;
        }
        pj.n_chunks = (uint32_t)chunks - pj.chunk0;
    }
    plan->n_chunks = (uint32_t)chunks; plan->u_total = u;
    return JDA_SUCCESS;
}

#endif
