// jda_encode_plan.h -- HOST: the arguments of jda_encode_surfaces checked and turned into the job records, the quantiser records, the
// Huffman code words and the file headers of one call, and -- once the device has summed the code lengths -- the place of every job's
// unstuffed scan and stuffing chunks.  No HIP in here: the runtime (jda_runtime.cpp) and the CPU tests (tests/hostsim/encode_sim.cpp)
// run the same checks and build the same records.  The definition: DESIGN.md 5.13; the stages: jda_en_* in jda_device_core.h.
#ifndef JDA_ENCODE_PLAN_H
#define JDA_ENCODE_PLAN_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "jda_device_core.h"

// ITU-T T.81 Annex K: the two quantisers (natural order) and the four Huffman tables
static const uint8_t jda_en_k_quant[2][64] = {
    { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
    { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 } };
static const uint8_t jda_en_k_dc_bits[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
static const uint8_t jda_en_k_dc_vals[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
static const uint8_t jda_en_k_ac_bits[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125 }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119 } };
static const uint8_t jda_en_k_ac_vals[2][162] = {
    { 1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23,
      24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106,
      115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169,
      170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229,
      230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250 },
    { 0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37,
      241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106,
      115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168,
      169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229,
      230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250 } };
struct jda_encode_plan_out {
    std::vector<jda_encode_dev_job> jobs;
    std::vector<jda_encode_quant> quant;     // one per quality of the call
    std::vector<uint32_t> huff;              // JDA_EN_HUFF_DWORDS (Annex K), then as many for every optimised job (zeros until jda_encode_plan_tables)
    std::vector<uint8_t> hdr;                // every job's header, back to back
    uint32_t n_blocks, n_int, n_chunks;      // n_chunks: after jda_encode_plan_place
    uint64_t u_total;                        // bytes of all unstuffed scans, each rounded up to a chunk (after jda_encode_plan_place)
    std::vector<int32_t> quality;            // a job (its header is written twice where it is optimised)
    uint32_t n_opt;                          // optimised jobs: JDA_EN_HUFF_DWORDS of histogram each
    // a call whose jobs bring quantisers of their own (jda_recode_plan.h; empty in a call over pixels): a job's DQT segments as they go into
    // its file, the table ids of Y, Cb, Cr, and the room kept for an optimised job's header
    std::vector<std::vector<uint8_t>> dqt;
    std::vector<uint8_t> tq;                 // 3 a job
    std::vector<uint32_t> hdr_room;
};
// one Huffman table as a DHT segment lists it
struct jda_encode_table { uint8_t bits[16]; uint8_t vals[256]; uint32_t n_vals; };

// libjpeg's jpeg_set_quality: table t (0 luma, 1 chroma) at quality q, natural order
static inline void jda_encode_quantiser(int32_t q, int t, uint8_t *out)
{
    const int32_t s = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; i++) {
        const int32_t v = ((int32_t)jda_en_k_quant[t][i] * s + 50) / 100;
        out[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}
// (|c| + half) / d == ((|c| + half) * recip) >> 32 for d = 8 q, q <= 255, and every numerator below 2^17: recip = ceil(2^32 / d) is off
// by less than d / 2^32 of the quotient's unit, and numerator * d < 2^32 (tests/test_encode_cpu.py tries all of them)
static inline uint32_t jda_encode_recip(uint32_t d) { return (uint32_t)(((1ull << 32) + d - 1u) / d); }
static inline void jda_encode_quant_record(int32_t q, jda_encode_quant *Q)
{
    for (int t = 0; t < 2; t++) {
        uint8_t tab[64];
        jda_encode_quantiser(q, t, tab);
        for (int i = 0; i < 64; i++) { const uint32_t d = (uint32_t)tab[i] << 3; Q->recip[t][i] = jda_encode_recip(d); Q->half[t][i] = d >> 1; }
    }
}
// the code words of four tables, (bits, vals) as a DHT lists them, in the order DC 0, AC 0, DC 1, AC 1 (a NULL bits: that table stays zeros)
static inline void jda_encode_huff_words_from(const uint8_t *const bits4[4], const uint8_t *const vals4[4], uint32_t *w)
{
    memset(w, 0, JDA_EN_HUFF_DWORDS * sizeof(uint32_t));
    for (int t = 0; t < 2; t++) {
        for (int cls = 0; cls < 2; cls++) {
            const uint8_t *bits = bits4[t * 2 + cls], *vals = vals4[t * 2 + cls];
            if (!bits) continue;
            uint32_t code = 0, k = 0;
            for (uint32_t len = 1; len <= 16u; len++, code <<= 1)
                for (uint32_t i = 0; i < bits[len - 1u]; i++, k++, code++) w[cls ? (uint32_t)t * 256u + vals[k] : 512u + (uint32_t)t * 16u + vals[k]] = (len << 16) | code;
        }
    }
}
static inline void jda_encode_huff_words(uint32_t *w)
{
    const uint8_t *const bits4[4] = { jda_en_k_dc_bits[0], jda_en_k_ac_bits[0], jda_en_k_dc_bits[1], jda_en_k_ac_bits[1] };
    const uint8_t *const vals4[4] = { jda_en_k_dc_vals, jda_en_k_ac_vals[0], jda_en_k_dc_vals, jda_en_k_ac_vals[1] };
    jda_encode_huff_words_from(bits4, vals4, w);
}
// libjpeg's jpeg_gen_optimal_table (jchuff.c): the table of a symbol histogram.  The pseudo-symbol 256 of count 1 keeps the all-ones code
// free; the two least frequent symbols are merged until one is left, a tie going to the LARGER symbol (<= in both searches); the lengths
// come from the others[] chains; the counts of lengths 32 .. 17 are folded back; one code leaves the longest length in use; vals lists the
// symbols by length, then by value.  No count may pass 10^9, the value the searches start from (JDA_EN_OPT_MAX_BLOCKS sees to it), so every
// merged count fits 32 bits.  false: a code of more than 32 bits, where libjpeg gives up (JERR_HUFF_CLEN_OVERFLOW).
static inline bool jda_encode_optimal_table(const uint32_t freq_in[256], uint8_t bits_out[16], uint8_t *vals, uint32_t *n_vals)
{
    uint32_t freq[257], bits[33];
    int32_t codesize[257], others[257], live[257], syms[257], n_live = 0;
    memcpy(freq, freq_in, 256 * sizeof(uint32_t));
    freq[256] = 1u;
    memset(bits, 0, sizeof(bits)); memset(codesize, 0, sizeof(codesize));
    for (int i = 0; i < 257; i++) { others[i] = -1; if (freq[i]) live[n_live++] = i; }
    const int32_t n_syms = n_live;
    memcpy(syms, live, (size_t)n_live * sizeof(int32_t));
    // (libjpeg searches all 257 entries for every merge; the symbols that still have a count, kept in ascending order, give the same two)
    while (n_live > 1) {
        int k1 = -1, k2 = -1;
        uint32_t v = 1000000000u;
        for (int k = 0; k < n_live; k++) if (freq[live[k]] <= v) { v = freq[live[k]]; k1 = k; }
        v = 1000000000u;
        for (int k = 0; k < n_live; k++) if (freq[live[k]] <= v && k != k1) { v = freq[live[k]]; k2 = k; }
        if (k1 < 0 || k2 < 0) break;                                       // (a count above 10^9: the plan lets none through)
        int c1 = live[k1], c2 = live[k2];
        freq[c1] += freq[c2]; freq[c2] = 0;
        memmove(live + k2, live + k2 + 1, (size_t)(n_live - k2 - 1) * sizeof(int32_t)); n_live--;
        for (codesize[c1]++; others[c1] >= 0;) { c1 = others[c1]; codesize[c1]++; }
        others[c1] = c2;
        for (codesize[c2]++; others[c2] >= 0;) { c2 = others[c2]; codesize[c2]++; }
    }
    memset(bits_out, 0, 16); *n_vals = 0;
    for (int k = 0; k < n_syms; k++) if (codesize[syms[k]]) { if (codesize[syms[k]] > 32) return false; bits[codesize[syms[k]]]++; }
    int i = 32;
    for (; i > 16; i--)
        while (bits[i] > 0) {
            int j = i - 2;
            while (bits[j] == 0) j--;
            bits[i] -= 2; bits[i - 1]++; bits[j + 1] += 2; bits[j]--;
        }
    while (i > 0 && bits[i] == 0) i--;
    if (i == 0) return true;                                             // (no symbol but the pseudo one: an empty table)
    bits[i]--;
    for (int k = 0; k < 16; k++) bits_out[k] = (uint8_t)bits[k + 1];
    uint32_t p = 0;
    for (int len = 1; len <= 32; len++)
        for (int k = 0; k < n_syms; k++) if (syms[k] <= 255 && codesize[syms[k]] == len) vals[p++] = (uint8_t)syms[k];
    *n_vals = p;
    return true;
}
static inline void jda_encode_put_seg(std::vector<uint8_t> &o, uint8_t marker, const std::vector<uint8_t> &payload)
{
    o.push_back(0xff); o.push_back(marker);
    o.push_back((uint8_t)((payload.size() + 2u) >> 8)); o.push_back((uint8_t)(payload.size() + 2u));
    o.insert(o.end(), payload.begin(), payload.end());
}
// SOI, JFIF APP0, DQT per table, SOF0, the DHTs, DRI (ri != 0), SOS: everything in front of the entropy-coded data.  tables == NULL: the
// Annex K DHTs, DC 0, DC 1, AC 0, AC 1 as libjpeg writes the standard ones; else the job's own (DC 0, AC 0, DC 1, AC 1 in tables[], the
// last two unused for gray), a segment per table in that order, as libjpeg writes them behind its statistics pass.
// the DQT segments of a file at `quality`: table 0, and table 1 where there is chroma
static inline void jda_encode_quality_dqt(int32_t quality, int nc, std::vector<uint8_t> &o)
{
    for (int t = 0; t < (nc == 1 ? 1 : 2); t++) {
        uint8_t nat[64];
        jda_encode_quantiser(quality, t, nat);
        std::vector<uint8_t> p(65);
        p[0] = (uint8_t)t;
        for (int z = 0; z < 64; z++) p[1 + z] = nat[jda_en_zigzag((uint32_t)z)];
        jda_encode_put_seg(o, 0xdb, p);
    }
}
// SOI, JFIF APP0, the DQT segments as handed in, the frame header (marker: 0xc0 or 0xc2) with tq[c] the quantiser of component c
static inline void jda_encode_header_front(int32_t w, int32_t h, int nc, int hs, int vs, const uint8_t *dqt, size_t dqt_bytes, const uint8_t tq[3], uint8_t marker, std::vector<uint8_t> &o)
{
    o.push_back(0xff); o.push_back(0xd8);
    jda_encode_put_seg(o, 0xe0, { 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 });
    o.insert(o.end(), dqt, dqt + dqt_bytes);
    std::vector<uint8_t> sof = { 8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, (uint8_t)nc, 1, (uint8_t)((hs << 4) | vs), tq[0] };
    for (int c = 1; c < nc; c++) { sof.push_back((uint8_t)(1 + c)); sof.push_back(0x11); sof.push_back(tq[c]); }
    jda_encode_put_seg(o, marker, sof);
}
// the same with explicit quantisers (a recode: the source's own): dqt = its DQT segments, tq[c] = the table id of component c
static inline void jda_encode_header_explicit(int32_t w, int32_t h, int32_t sampling, const uint8_t *dqt, size_t dqt_bytes, const uint8_t tq[3], int32_t ri,
                                              const jda_encode_table *tables, std::vector<uint8_t> &o)
{
    const int nc = sampling == JDA_ENCODE_GRAY ? 1 : 3, hs = sampling >= JDA_ENCODE_422 ? 2 : 1, vs = sampling == JDA_ENCODE_420 ? 2 : 1;
    jda_encode_header_front(w, h, nc, hs, vs, dqt, dqt_bytes, tq, 0xc0, o);
    for (int k = 0; k < (nc == 1 ? 2 : 4); k++) {
        const int cls = tables ? k & 1 : (nc == 1 ? k : k >> 1), t = tables ? k >> 1 : (nc == 1 ? 0 : k & 1);
        const uint8_t *bits = tables ? tables[k].bits : cls ? jda_en_k_ac_bits[t] : jda_en_k_dc_bits[t];
        const uint8_t *vals = tables ? tables[k].vals : cls ? jda_en_k_ac_vals[t] : jda_en_k_dc_vals;
        std::vector<uint8_t> p;
        p.push_back((uint8_t)((cls << 4) | t));
        p.insert(p.end(), bits, bits + 16);
        p.insert(p.end(), vals, vals + (tables ? tables[k].n_vals : cls ? 162u : 12u));
        jda_encode_put_seg(o, 0xc4, p);
    }
    if (ri) jda_encode_put_seg(o, 0xdd, { (uint8_t)(ri >> 8), (uint8_t)ri });
    std::vector<uint8_t> sos = { (uint8_t)nc, 1, 0x00 };
    for (int c = 1; c < nc; c++) { sos.push_back((uint8_t)(1 + c)); sos.push_back(0x11); }
    sos.push_back(0); sos.push_back(63); sos.push_back(0);
    jda_encode_put_seg(o, 0xda, sos);
}
static inline void jda_encode_header_tables(int32_t w, int32_t h, int32_t sampling, int32_t quality, int32_t ri, const jda_encode_table *tables, std::vector<uint8_t> &o)
{
    const uint8_t tq[3] = { 0, 1, 1 };
    std::vector<uint8_t> dqt;
    jda_encode_quality_dqt(quality, sampling == JDA_ENCODE_GRAY ? 1 : 3, dqt);
    jda_encode_header_explicit(w, h, sampling, dqt.data(), dqt.size(), tq, ri, tables, o);
}
static inline void jda_encode_header(int32_t w, int32_t h, int32_t sampling, int32_t quality, int32_t ri, std::vector<uint8_t> &o)
{
    jda_encode_header_tables(w, h, sampling, quality, ri, NULL, o);
}
// blocks and intervals of a w x h image; false: not an image the encoder takes
static inline bool jda_encode_counts(int64_t w, int64_t h, int32_t sampling, int32_t ri, uint32_t *cx, uint32_t *cy, uint32_t *bpm, uint64_t *blocks, uint64_t *intervals)
{
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || sampling < JDA_ENCODE_GRAY || sampling > JDA_ENCODE_420 || ri < 0 || ri > 65535) return false;
    const uint32_t hs = sampling >= JDA_ENCODE_422 ? 2u : 1u, vs = sampling == JDA_ENCODE_420 ? 2u : 1u;
    *cx = ((uint32_t)w + 8u * hs - 1u) / (8u * hs); *cy = ((uint32_t)h + 8u * vs - 1u) / (8u * vs);
    *bpm = sampling == JDA_ENCODE_GRAY ? 1u : hs * vs + 2u;
    const uint64_t mcus = (uint64_t)*cx * *cy;
    *blocks = mcus * *bpm;
    *intervals = ri ? (mcus + (uint32_t)ri - 1u) / (uint32_t)ri : 1u;
    return true;
}
static inline uint32_t jda_encode_header_bytes(int32_t sampling, int32_t ri)          // (its length depends on nothing else)
{
    std::vector<uint8_t> o;
    jda_encode_header(1, 1, sampling, 50, ri, o);
    return (uint32_t)o.size();
}
// the largest file the image can become: every block at JDA_EN_BLOCK_BITS, every byte stuffed, every interval padded and marked.
// It holds for an optimised job (JDA_ENCODE_OPTIMIZE) as it stands: its DHTs list at most 12 DC and 162 AC symbols -- the only ones a
// block can hold -- so its header is no longer than the Annex K one counted here; and no code of jda_encode_optimal_table is longer than
// 16 bits, the longest of Annex K, so a block stays within 16 + 11 bits of DC and 63 x (16 + 10) of AC = JDA_EN_BLOCK_BITS.
static inline int jda_encode_bound_bytes(int32_t w, int32_t h, int32_t sampling, int32_t ri, int64_t *bytes)
{
    uint32_t cx, cy, bpm;
    uint64_t blocks, ints;
    if (!bytes) return JDA_INVALID_PARAMETER;
    *bytes = 0;
    if (!jda_encode_counts(w, h, sampling, ri, &cx, &cy, &bpm, &blocks, &ints)) return JDA_INVALID_PARAMETER;
    *bytes = (int64_t)(jda_encode_header_bytes(sampling, ri) + 2u * ((blocks * JDA_EN_BLOCK_BITS + 7u) / 8u + ints) + 2u * ints + 2u);
    return JDA_SUCCESS;
}

// n >= 1 jobs.  The records of the first half of the call; chunk0 / n_chunks / h_chunks / u_off are jda_encode_plan_place's.  job_flags:
// NULL or n words of JDA_ENCODE_*.  An optimised job gets JDA_EN_HUFF_DWORDS of the word tables and of the histograms, and room for its
// header (no longer than the Annex K one); the words and the header are jda_encode_plan_tables'.
static inline int jda_encode_plan_jobs_ex(int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, const uint32_t *job_flags, void *const *dst,
                                          const int64_t *dst_capacity, jda_encode_plan_out *plan)
{
    plan->jobs.clear(); plan->quant.clear(); plan->huff.clear(); plan->hdr.clear(); plan->n_blocks = plan->n_int = plan->n_chunks = 0; plan->u_total = 0;
    plan->quality.clear(); plan->n_opt = 0; plan->dqt.clear(); plan->tq.clear(); plan->hdr_room.clear();
    if (bytes_per_pixel != 1 && bytes_per_pixel != 4) return JDA_INVALID_PARAMETER;
    if (n <= 0 || !src || !jobs || !dst || !dst_capacity) return JDA_INVALID_PARAMETER;
    const uint32_t bpp = (uint32_t)bytes_per_pixel;
    struct range { uintptr_t a, b; bool is_dst; };
    std::vector<range> ranges;
    std::map<int32_t, uint32_t> quals;
    uint64_t blocks = 0, ints = 0;
    plan->jobs.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const jda_output &S = src[i];
        const jda_encode_job &E = jobs[i];
        if (!S.pixels || !dst[i] || S.width_px <= 0 || S.rows <= 0 || dst_capacity[i] < 0) return JDA_INVALID_PARAMETER;
        if (job_flags && (job_flags[i] & ~(uint32_t)JDA_ENCODE_OPTIMIZE)) return JDA_INVALID_PARAMETER;
        const bool opt = job_flags && (job_flags[i] & JDA_ENCODE_OPTIMIZE);
        if (((uintptr_t)S.pixels & (bpp - 1u)) || (S.pitch_bytes & (int32_t)(bpp - 1u)) || (int64_t)S.pitch_bytes < (int64_t)S.width_px * bpp) return JDA_INVALID_PARAMETER;
        if (E.x < 0 || E.y < 0 || E.w < 1 || E.h < 1 || (int64_t)E.x + E.w > S.width_px || (int64_t)E.y + E.h > S.rows) return JDA_INVALID_PARAMETER;
        if (E.quality < 1 || E.quality > 100 || E.reserved != 0) return JDA_INVALID_PARAMETER;
        if ((E.sampling == JDA_ENCODE_GRAY) != (bpp == 1u)) return JDA_INVALID_PARAMETER;          // a gray surface takes the gray sampling and no other
        jda_encode_dev_job &J = plan->jobs[(size_t)i];
        memset(&J, 0, sizeof(J));
        uint64_t jb, ji;
        if (!jda_encode_counts(E.w, E.h, E.sampling, E.restart_interval, &J.cx, &J.cy, &J.bpm, &jb, &ji)) return JDA_INVALID_PARAMETER;
        if (blocks + jb > 0x7fffffffull) return JDA_UNSUPPORTED_FEATURE;                       // (the flat block list is indexed by 32 bits)
        if (opt && jb > JDA_EN_OPT_MAX_BLOCKS) return JDA_UNSUPPORTED_FEATURE;                  // (a symbol count could pass 10^9)
        J.src = (const uint8_t *)S.pixels; J.dst = (uint8_t *)dst[i]; J.capacity = (uint64_t)dst_capacity[i];
        J.src_pitch = (uint32_t)S.pitch_bytes; J.x = (uint32_t)E.x; J.y = (uint32_t)E.y; J.w = (uint32_t)E.w; J.h = (uint32_t)E.h;
        J.hs = E.sampling >= JDA_ENCODE_422 ? 2u : 1u; J.vs = E.sampling == JDA_ENCODE_420 ? 2u : 1u; J.nc = E.sampling == JDA_ENCODE_GRAY ? 1u : 3u;
        J.wb = (J.w + 7u) / 8u; J.hb = (J.h + 7u) / 8u; J.ri = (uint32_t)E.restart_interval;
        J.block0 = (uint32_t)blocks; J.n_blocks = (uint32_t)jb; J.int0 = (uint32_t)ints; J.n_int = (uint32_t)ji;
        blocks += jb; ints += ji;
        auto it = quals.find(E.quality);
        if (it == quals.end()) {
            it = quals.emplace(E.quality, (uint32_t)plan->quant.size()).first;
            plan->quant.emplace_back();
            jda_encode_quant_record(E.quality, &plan->quant.back());
        }
        J.quant = it->second;
        J.hdr_off = (uint32_t)plan->hdr.size();
        plan->quality.push_back(E.quality);
        if (opt) {
            plan->n_opt++;
            J.huff_off = plan->n_opt * JDA_EN_HUFF_DWORDS; J.hist_off = (plan->n_opt - 1u) * JDA_EN_HUFF_DWORDS;
            plan->hdr.resize(plan->hdr.size() + jda_encode_header_bytes(E.sampling, E.restart_interval));      // (hdr_len: 0 until the tables are made)
        } else {
            J.hist_off = JDA_EN_NO_HIST;
            jda_encode_header(E.w, E.h, E.sampling, E.quality, E.restart_interval, plan->hdr);
            J.hdr_len = (uint32_t)plan->hdr.size() - J.hdr_off;
        }
        const uintptr_t s0 = (uintptr_t)S.pixels + (size_t)E.y * (size_t)S.pitch_bytes + (size_t)E.x * bpp;
        ranges.push_back({ s0, s0 + (size_t)(E.h - 1) * (size_t)S.pitch_bytes + (size_t)E.w * bpp, false });
        ranges.push_back({ (uintptr_t)dst[i], (uintptr_t)dst[i] + (size_t)dst_capacity[i], true });
    }
    // a destination may share no byte with a source or with another destination (as jda_resize_surfaces checks it)
    std::sort(ranges.begin(), ranges.end(), [](const range &p, const range &q) { return p.a < q.a; });
    uintptr_t end_any = 0, end_dst = 0;
    for (const range &r : ranges) {
        if (r.a == r.b) continue;
        if (r.is_dst ? r.a < end_any : r.a < end_dst) return JDA_INVALID_PARAMETER;
        end_any = std::max(end_any, r.b);
        if (r.is_dst) end_dst = std::max(end_dst, r.b);
    }
    plan->huff.assign((size_t)JDA_EN_HUFF_DWORDS * (1u + plan->n_opt), 0u);
    jda_encode_huff_words(plan->huff.data());
    plan->n_blocks = (uint32_t)blocks; plan->n_int = (uint32_t)ints;
    return JDA_SUCCESS;
}
static inline int jda_encode_plan_jobs(int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, void *const *dst, const int64_t *dst_capacity,
                                       jda_encode_plan_out *plan)
{
    return jda_encode_plan_jobs_ex(n, src, bytes_per_pixel, jobs, NULL, dst, dst_capacity, plan);
}
// between gather and the second lengths pass: hist = the call's histograms as the device counted them (n_opt x JDA_EN_HUFF_DWORDS, the word
// tables' index layout).  Every optimised job gets its tables, its code words at huff_off and its header (hdr_len) in the room kept for it.
// JDA_UNSUPPORTED_FEATURE: a histogram that libjpeg itself refuses (a code of more than 32 bits before the lengths are limited).
static inline int jda_encode_plan_tables(jda_encode_plan_out *plan, const uint32_t *hist)
{
    for (size_t i = 0; i < plan->jobs.size(); i++) {
        jda_encode_dev_job &J = plan->jobs[i];
        if (J.hist_off == JDA_EN_NO_HIST) continue;
        const uint32_t *H = hist + J.hist_off;
        const int nt = J.nc == 1u ? 1 : 2;
        jda_encode_table T[4];
        const uint8_t *bits4[4] = { NULL, NULL, NULL, NULL }, *vals4[4] = { NULL, NULL, NULL, NULL };
        for (int t = 0; t < nt; t++)
            for (int cls = 0; cls < 2; cls++) {
                uint32_t freq[256];
                memset(freq, 0, sizeof(freq));
                if (cls) memcpy(freq, H + t * 256, 256 * sizeof(uint32_t)); else memcpy(freq, H + 512 + t * 16, 16 * sizeof(uint32_t));
                jda_encode_table &tab = T[t * 2 + cls];
                if (!jda_encode_optimal_table(freq, tab.bits, tab.vals, &tab.n_vals)) return JDA_UNSUPPORTED_FEATURE;
                bits4[t * 2 + cls] = tab.bits; vals4[t * 2 + cls] = tab.vals;
            }
        jda_encode_huff_words_from(bits4, vals4, plan->huff.data() + J.huff_off);
        const int32_t sampling = J.nc == 1u ? JDA_ENCODE_GRAY : J.vs == 2u ? JDA_ENCODE_420 : J.hs == 2u ? JDA_ENCODE_422 : JDA_ENCODE_444;
        std::vector<uint8_t> h;
        if (plan->dqt.empty()) jda_encode_header_tables((int32_t)J.w, (int32_t)J.h, sampling, plan->quality[i], (int32_t)J.ri, T, h);
        else jda_encode_header_explicit((int32_t)J.w, (int32_t)J.h, sampling, plan->dqt[i].data(), plan->dqt[i].size(), plan->tq.data() + 3 * i, (int32_t)J.ri, T, h);
        if (h.size() > (plan->hdr_room.empty() ? jda_encode_header_bytes(sampling, (int32_t)J.ri) : plan->hdr_room[i])) return JDA_ERROR_MEMORY;      // (never: at most 12 + 162 symbols)
        memcpy(plan->hdr.data() + J.hdr_off, h.data(), h.size());
        J.hdr_len = (uint32_t)h.size();
    }
    return JDA_SUCCESS;
}
// the second half: u_bytes[i] = the bytes of job i's unstuffed scan (the device's sums).  JDA_UNSUPPORTED_FEATURE past 2^31 chunks.
static inline int jda_encode_plan_place(jda_encode_plan_out *plan, const jda_encode_totals *totals)
{
    uint64_t chunks = 0, u = 0;
    for (size_t i = 0; i < plan->jobs.size(); i++) {
        jda_encode_dev_job &J = plan->jobs[i];
        const uint64_t uc = (totals[i].u_bytes + JDA_EN_CHUNK - 1u) / JDA_EN_CHUNK;
        J.h_chunks = (J.hdr_len + JDA_EN_CHUNK - 1u) / JDA_EN_CHUNK;
        if (chunks + J.h_chunks + uc > 0x7fffffffull) return JDA_UNSUPPORTED_FEATURE;
        J.chunk0 = (uint32_t)chunks; J.n_chunks = J.h_chunks + (uint32_t)uc; J.u_off = u;
        chunks += J.n_chunks; u += uc * JDA_EN_CHUNK;
    }
    plan->n_chunks = (uint32_t)chunks; plan->u_total = u;
    return JDA_SUCCESS;
}

#endif
