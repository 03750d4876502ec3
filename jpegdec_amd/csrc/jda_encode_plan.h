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
    std::vector<uint32_t> huff;              // JDA_EN_HUFF_DWORDS
    std::vector<uint8_t> hdr;                // every job's header, back to back
    uint32_t n_blocks, n_int, n_chunks;      // n_chunks: after jda_encode_plan_place
    uint64_t u_total;                        // bytes of all unstuffed scans, each rounded up to a chunk (after jda_encode_plan_place)
};

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
static inline void jda_encode_huff_words(uint32_t *w)
{
    memset(w, 0, JDA_EN_HUFF_DWORDS * sizeof(uint32_t));
    for (int t = 0; t < 2; t++) {
        for (int cls = 0; cls < 2; cls++) {
            const uint8_t *bits = cls ? jda_en_k_ac_bits[t] : jda_en_k_dc_bits[t], *vals = cls ? jda_en_k_ac_vals[t] : jda_en_k_dc_vals;
            uint32_t code = 0, k = 0;
            for (uint32_t len = 1; len <= 16u; len++, code <<= 1)
                for (uint32_t i = 0; i < bits[len - 1u]; i++, k++, code++) w[cls ? (uint32_t)t * 256u + vals[k] : 512u + (uint32_t)t * 16u + vals[k]] = (len << 16) | code;
        }
    }
}
static inline void jda_encode_put_seg(std::vector<uint8_t> &o, uint8_t marker, const std::vector<uint8_t> &payload)
{
    o.push_back(0xff); o.push_back(marker);
    o.push_back((uint8_t)((payload.size() + 2u) >> 8)); o.push_back((uint8_t)(payload.size() + 2u));
    o.insert(o.end(), payload.begin(), payload.end());
}
// SOI, JFIF APP0, DQT per table, SOF0, the Annex K DHTs, DRI (ri != 0), SOS: everything in front of the entropy-coded data
static inline void jda_encode_header(int32_t w, int32_t h, int32_t sampling, int32_t quality, int32_t ri, std::vector<uint8_t> &o)
{
    const int nc = sampling == JDA_ENCODE_GRAY ? 1 : 3, hs = sampling >= JDA_ENCODE_422 ? 2 : 1, vs = sampling == JDA_ENCODE_420 ? 2 : 1;
    o.push_back(0xff); o.push_back(0xd8);
    jda_encode_put_seg(o, 0xe0, { 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 });
    for (int t = 0; t < (nc == 1 ? 1 : 2); t++) {
        uint8_t nat[64];
        jda_encode_quantiser(quality, t, nat);
        std::vector<uint8_t> p(65);
        p[0] = (uint8_t)t;
        for (int z = 0; z < 64; z++) p[1 + z] = nat[jda_en_zigzag((uint32_t)z)];
        jda_encode_put_seg(o, 0xdb, p);
    }
    std::vector<uint8_t> sof = { 8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, (uint8_t)nc, 1, (uint8_t)((hs << 4) | vs), 0 };
    for (int c = 1; c < nc; c++) { sof.push_back((uint8_t)(1 + c)); sof.push_back(0x11); sof.push_back(1); }
    jda_encode_put_seg(o, 0xc0, sof);
    for (int cls = 0; cls < 2; cls++)
        for (int t = 0; t < (nc == 1 ? 1 : 2); t++) {
            const uint8_t *bits = cls ? jda_en_k_ac_bits[t] : jda_en_k_dc_bits[t], *vals = cls ? jda_en_k_ac_vals[t] : jda_en_k_dc_vals;
            std::vector<uint8_t> p;
            p.push_back((uint8_t)((cls << 4) | t));
            p.insert(p.end(), bits, bits + 16);
            p.insert(p.end(), vals, vals + (cls ? 162 : 12));
            jda_encode_put_seg(o, 0xc4, p);
        }
    if (ri) jda_encode_put_seg(o, 0xdd, { (uint8_t)(ri >> 8), (uint8_t)ri });
    std::vector<uint8_t> sos = { (uint8_t)nc, 1, 0x00 };
    for (int c = 1; c < nc; c++) { sos.push_back((uint8_t)(1 + c)); sos.push_back(0x11); }
    sos.push_back(0); sos.push_back(63); sos.push_back(0);
    jda_encode_put_seg(o, 0xda, sos);
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
// the largest file the image can become: every block at JDA_EN_BLOCK_BITS, every byte stuffed, every interval padded and marked
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

// n >= 1 jobs.  The records of the first half of the call; chunk0 / n_chunks / h_chunks / u_off are jda_encode_plan_place's.
static inline int jda_encode_plan_jobs(int32_t n, const jda_output *src, int32_t bytes_per_pixel, const jda_encode_job *jobs, void *const *dst, const int64_t *dst_capacity,
                                       jda_encode_plan_out *plan)
{
    plan->jobs.clear(); plan->quant.clear(); plan->huff.clear(); plan->hdr.clear(); plan->n_blocks = plan->n_int = plan->n_chunks = 0; plan->u_total = 0;
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
        if (((uintptr_t)S.pixels & (bpp - 1u)) || (S.pitch_bytes & (int32_t)(bpp - 1u)) || (int64_t)S.pitch_bytes < (int64_t)S.width_px * bpp) return JDA_INVALID_PARAMETER;
        if (E.x < 0 || E.y < 0 || E.w < 1 || E.h < 1 || (int64_t)E.x + E.w > S.width_px || (int64_t)E.y + E.h > S.rows) return JDA_INVALID_PARAMETER;
        if (E.quality < 1 || E.quality > 100 || E.reserved != 0) return JDA_INVALID_PARAMETER;
        if ((E.sampling == JDA_ENCODE_GRAY) != (bpp == 1u)) return JDA_INVALID_PARAMETER;          // a gray surface takes the gray sampling and no other
        jda_encode_dev_job &J = plan->jobs[(size_t)i];
        memset(&J, 0, sizeof(J));
        uint64_t jb, ji;
        if (!jda_encode_counts(E.w, E.h, E.sampling, E.restart_interval, &J.cx, &J.cy, &J.bpm, &jb, &ji)) return JDA_INVALID_PARAMETER;
        if (blocks + jb > 0x7fffffffull) return JDA_UNSUPPORTED_FEATURE;                       // (the flat block list is indexed by 32 bits)
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
        jda_encode_header(E.w, E.h, E.sampling, E.quality, E.restart_interval, plan->hdr);
        J.hdr_len = (uint32_t)plan->hdr.size() - J.hdr_off;
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
    plan->huff.resize(JDA_EN_HUFF_DWORDS);
    jda_encode_huff_words(plan->huff.data());
    plan->n_blocks = (uint32_t)blocks; plan->n_int = (uint32_t)ints;
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
