// tests/hostsim/encode_sim.cpp -- TEST INFRASTRUCTURE: the encode kernels' schedule on the CPU.
//
// encodesim_lanes runs the six stages of jda_encode_surfaces (jda_encode_* of jpegdec_amd/csrc/jda_kernels.hip) the way the GPU runs them:
// every lane of every stage one after the other through the kernels' OWN code (jda_en_* of jda_device_core.h) over the records the host
// plan makes (jda_encode_plan.h), the two halves of a workgroup's scan either side of its barrier, the host's step between the halves of
// the call as jda_runtime.cpp takes it.  Memory goes through an IO policy that holds every access to what the kernels promise: an access
// lies whole inside ONE allocation of the call and is aligned to its own width; a pixel load reads a pixel of its job's rectangle; scratch
// is poisoned and a byte of it is read only after a lane wrote it; the unstuffed scans are zeros and change only by atomic OR; the scan's
// LDS is poisoned before every workgroup and read only where this workgroup wrote it; no byte of a file is written twice, none behind the
// capacity, and in the end every byte of a file that fits once -- of one that does not, none.
// encodesim_coefs runs the stages behind the first over coefficients the caller chose (what no picture gives); encodesim_scan runs the scan
// stage alone over lengths the caller chose, the second half's lanes in reverse order; encodesim_check runs the argument checks alone;
// encodesim_divide tries the reciprocal of every divisor on every numerator.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../jpegdec_amd/csrc/jda_encode_plan.h"

namespace {
struct Alloc { uint8_t *base; size_t size; bool writable, atomic_only; std::vector<uint8_t> init; };      // init empty: all of it may be read
struct SimIO {
    std::vector<Alloc> allocs;
    const jda_encode_dev_job *cur; uint32_t bpp;
    std::vector<std::vector<uint8_t>> written;      // per job: its file's bytes
    const jda_encode_dev_job *jobs; size_t n_jobs;
    std::vector<uint64_t> lds; std::vector<uint8_t> lds_set;
    int err;
    void fail(int e) { if (!err) err = e; }
    size_t add(void *p, size_t size, bool writable, bool poisoned, bool atomic_only = false)
    {
        Alloc a; a.base = (uint8_t *)p; a.size = size; a.writable = writable; a.atomic_only = atomic_only;
        if (poisoned) { memset(p, 0xEE, size); a.init.assign(size, 0); }
        allocs.push_back(a);
        return allocs.size() - 1;
    }
    Alloc *find(const void *p, size_t n)
    {
        const uint8_t *q = (const uint8_t *)p;
        if ((uintptr_t)q % n) { fail(-10); return NULL; }
        for (Alloc &a : allocs) if (q >= a.base && q + n <= a.base + a.size) return &a;
        fail(-11);
        return NULL;
    }
    bool rd(const void *p, size_t n)
    {
        Alloc *a = find(p, n);
        if (!a) return false;
        if (!a->init.empty()) for (size_t i = 0; i < n; i++) if (!a->init[(size_t)((const uint8_t *)p - a->base) + i]) { fail(-12); return false; }
        return true;
    }
    bool wr(void *p, size_t n, bool atomic = false)
    {
        Alloc *a = find(p, n);
        if (!a) return false;
        if (!a->writable || (a->atomic_only && !atomic)) { fail(-13); return false; }
        if (!a->init.empty()) for (size_t i = 0; i < n; i++) a->init[(size_t)((uint8_t *)p - a->base) + i] = 1;
        return true;
    }
    uint32_t px(const uint8_t *p, uint32_t n)
    {
        if (!cur || (uintptr_t)p % n || p < cur->src) { fail(-20); return 0; }
        const size_t off = (size_t)(p - cur->src), row = off / cur->src_pitch, col = off % cur->src_pitch;
        if (row < cur->y || row >= cur->y + cur->h || col < (size_t)cur->x * bpp || col + n > (size_t)(cur->x + cur->w) * bpp || n != bpp) { fail(-21); return 0; }
        uint32_t v = 0;
        memcpy(&v, p, n);
        return v;
    }
    uint32_t ld_px32(const uint8_t *p) { return px(p, 4); }
    uint32_t ld_px8(const uint8_t *p) { return px(p, 1); }
    uint32_t ld8(const uint8_t *p) { return rd(p, 1) ? *p : 0u; }
    uint32_t ld32(const uint32_t *p) { uint32_t v = 0; if (rd(p, 4)) memcpy(&v, p, 4); return v; }
    uint64_t ld64(const uint64_t *p) { uint64_t v = 0; if (rd(p, 8)) memcpy(&v, p, 8); return v; }
    void ld128(const void *p, uint32_t *v) { memset(v, 0, 16); if (rd(p, 16)) memcpy(v, p, 16); }
    void st16(int16_t *p, int16_t v) { if (wr(p, 2)) memcpy(p, &v, 2); }
    void st32(uint32_t *p, uint32_t v) { if (wr(p, 4)) memcpy(p, &v, 4); }
    void st64(uint64_t *p, uint64_t v) { if (wr(p, 8)) memcpy(p, &v, 8); }
    void st128(void *p, const uint32_t *v) { if (wr(p, 16)) memcpy(p, v, 16); }
    void atomic_or(uint32_t *p, uint32_t v) { if (wr(p, 4, true)) *p |= v; }
    void st8(uint8_t *p, uint32_t v)                 // only files are written by the byte
    {
        for (size_t j = 0; j < n_jobs; j++) {
            const jda_encode_dev_job &J = jobs[j];
            if (p >= J.dst && p < J.dst + J.capacity) {
                uint8_t &w = written[j][(size_t)(p - J.dst)];
                if (w || &J != cur) { fail(-30); return; }
                w = 1; *p = (uint8_t)v;
                return;
            }
        }
        fail(-31);
    }
    void lds_wr64(uint32_t i, uint64_t v) { if (i >= lds.size()) { fail(-40); return; } lds[i] = v; lds_set[i] = 1; }
    uint64_t lds_rd64(uint32_t i) { if (i >= lds.size() || !lds_set[i]) { fail(-41); return 0; } return lds[i]; }
};

struct Run {
    jda_encode_plan_out P;
    jda_en_arrays A;
    SimIO io;
    std::vector<uint8_t> quant, hdr, coef, meta, code, end, ist, tot, u, ffcnt, ffend;
    std::vector<uint32_t> huff;
    std::vector<jda_encode_dev_job> jobs;
    size_t jobs_alloc;
};
template <class T> T *aligned(std::vector<uint8_t> &v, size_t bytes) { v.assign(bytes + 64, 0); return (T *)(((uintptr_t)v.data() + 63) & ~(uintptr_t)63); }

void scan(Run &R, bool bytes)
{
    for (uint32_t j = 0; j < R.A.n_jobs; j++) {
        std::fill(R.io.lds.begin(), R.io.lds.end(), 0xEEEEEEEEEEEEEEEEull);      // a workgroup finds nothing in LDS
        std::fill(R.io.lds_set.begin(), R.io.lds_set.end(), 0);
        R.io.cur = &R.jobs[j];
        for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_en_scan_job(R.A, R.jobs[j], j, bytes, false, tid, R.io);
        for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_en_scan_job(R.A, R.jobs[j], j, bytes, true, tid, R.io);
    }
}
// the first half's scratch, as encode_lengths of jda_runtime.cpp lays it out (every array an allocation of its own here: an access may not
// stray from one into its neighbour)
void setup(Run &R, uint32_t bpp)
{
    jda_encode_plan_out &P = R.P;
    const size_t n = P.jobs.size(), nb = P.n_blocks;
    memset(&R.A, 0, sizeof(R.A));
    R.jobs = P.jobs;
    R.io.allocs.clear(); R.io.err = 0; R.io.bpp = bpp; R.io.cur = NULL;
    R.io.lds.assign(3 * JDA_EN_THREADS, 0); R.io.lds_set.assign(3 * JDA_EN_THREADS, 0);
    jda_encode_quant *q = aligned<jda_encode_quant>(R.quant, P.quant.size() * sizeof(jda_encode_quant));
    memcpy(q, P.quant.data(), P.quant.size() * sizeof(jda_encode_quant));
    R.huff = P.huff;
    uint8_t *h = aligned<uint8_t>(R.hdr, P.hdr.size());
    memcpy(h, P.hdr.data(), P.hdr.size());
    R.A.jobs = R.jobs.data(); R.A.quant = q; R.A.huff = R.huff.data(); R.A.hdr = h; R.A.n_jobs = (uint32_t)n;
    R.io.add(q, P.quant.size() * sizeof(jda_encode_quant), false, false);      // (the order matters to encodesim_coefs: 3 = coef, 4 = meta)
    R.io.add(R.huff.data(), R.huff.size() * 4, false, false);
    R.io.add(h, P.hdr.size(), false, false);
    R.A.coef = aligned<int16_t>(R.coef, nb * 128); R.io.add(R.A.coef, nb * 128, true, true);
    R.A.meta = aligned<uint32_t>(R.meta, nb * 4); R.io.add(R.A.meta, nb * 4, true, true);
    R.A.code = aligned<uint32_t>(R.code, nb * 4); R.io.add(R.A.code, nb * 4, true, true);
    R.A.end = aligned<uint64_t>(R.end, nb * 8); R.io.add(R.A.end, nb * 8, true, true);
    R.A.istart = aligned<uint64_t>(R.ist, (size_t)P.n_int * 8); R.io.add(R.A.istart, (size_t)P.n_int * 8, true, true);
    R.A.totals = aligned<jda_encode_totals>(R.tot, n * sizeof(jda_encode_totals)); R.io.add(R.A.totals, n * sizeof(jda_encode_totals), true, true);
    R.jobs_alloc = R.io.add(R.jobs.data(), n * sizeof(jda_encode_dev_job), false, false);
}
// everything behind the blocks stage; 0 or the first promise broken
int finish(Run &R, int64_t *dst_bytes, int32_t *status, uint32_t *code, uint64_t *end, uint64_t *istart, uint8_t *unstuffed, int64_t unstuffed_cap)
{
    jda_encode_plan_out &P = R.P;
    const size_t n = P.jobs.size();
    for (uint32_t b = 0; b < P.n_blocks; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, R.io);
        if (b < R.jobs[j].block0 || b >= R.jobs[j].block0 + R.jobs[j].n_blocks) return -50;
        R.io.cur = &R.jobs[j];
        jda_en_length(R.A, R.jobs[j], b, R.io);
    }
    scan(R, false);
    if (R.io.err) return R.io.err;
    // the host between the halves
    std::vector<jda_encode_totals> tot(n);
    for (size_t i = 0; i < n; i++) { if (!R.io.rd(&R.A.totals[i].u_bytes, 8)) return -51; tot[i] = R.A.totals[i]; }
    const int rc = jda_encode_plan_place(&P, tot.data());
    if (rc != JDA_SUCCESS) return rc;
    R.jobs = P.jobs;
    R.A.jobs = R.jobs.data();
    R.io.allocs[R.jobs_alloc].base = (uint8_t *)R.jobs.data();      // (the second upload of the records)
    R.A.u = aligned<uint8_t>(R.u, (size_t)P.u_total); R.io.add(R.A.u, (size_t)P.u_total, true, false, true);
    R.A.ffcnt = aligned<uint32_t>(R.ffcnt, (size_t)P.n_chunks * 4); R.io.add(R.A.ffcnt, (size_t)P.n_chunks * 4, true, true);
    R.A.ffend = aligned<uint64_t>(R.ffend, (size_t)P.n_chunks * 8); R.io.add(R.A.ffend, (size_t)P.n_chunks * 8, true, true);
    R.io.jobs = R.jobs.data(); R.io.n_jobs = n;
    R.io.written.resize(n);
    for (size_t i = 0; i < n; i++) R.io.written[i].assign((size_t)R.jobs[i].capacity, 0);
    for (uint32_t b = 0; b < P.n_blocks; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, R.io);
        R.io.cur = &R.jobs[j];
        jda_en_emit(R.A, R.jobs[j], b, R.io);
    }
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t j = jda_en_find_chunk(R.A.jobs, R.A.n_jobs, c, R.io);
        if (c < R.jobs[j].chunk0 || c >= R.jobs[j].chunk0 + R.jobs[j].n_chunks) return -52;
        R.io.cur = &R.jobs[j];
        jda_en_count(R.A, R.jobs[j], c, R.io);
    }
    scan(R, true);
    for (uint32_t c = 0; c < P.n_chunks; c++) {
        const uint32_t j = jda_en_find_chunk(R.A.jobs, R.A.n_jobs, c, R.io);
        R.io.cur = &R.jobs[j];
        jda_en_write(R.A, R.jobs[j], j, c, R.io);
    }
    if (R.io.err) return R.io.err;
    for (size_t i = 0; i < n; i++) {
        if (!R.io.rd(&R.A.totals[i].file_bytes, 8)) return -53;
        const uint64_t fb = R.A.totals[i].file_bytes;
        dst_bytes[i] = (int64_t)fb;
        status[i] = fb > R.jobs[i].capacity ? JDA_ERROR_MEMORY : JDA_SUCCESS;
        for (size_t k = 0; k < R.io.written[i].size(); k++)
            if ((R.io.written[i][k] != 0) != (status[i] == JDA_SUCCESS && k < fb)) return -32;      // a byte of the file missing, or one written that is not the file's
    }
    if (code) memcpy(code, R.A.code, (size_t)P.n_blocks * 4);
    if (end) memcpy(end, R.A.end, (size_t)P.n_blocks * 8);
    if (istart) memcpy(istart, R.A.istart, (size_t)P.n_int * 8);
    if (unstuffed && (uint64_t)unstuffed_cap >= P.u_total) memcpy(unstuffed, R.A.u, (size_t)P.u_total);
    return 0;
}
}

// n jobs over HOST surfaces into HOST files.  0, or the first promise broken (-1x an access outside its allocation / misaligned / of poisoned
// scratch / a plain store into the unstuffed scans, -2x a pixel load outside the job's rectangle, -3x the files' bytes, -4x LDS, -5x the
// lists), or the status the argument checks of jda_encode_surfaces give.  Optional outputs, all in the call's flat order: coef (64 a block),
// code ((DC difference << 16) | code bits, a block), end (the bit behind a block's code), istart (an interval's first byte), unstuffed
// (the unstuffed scans, a job's at a multiple of 64 bytes), info = {blocks, intervals, chunks, unstuffed bytes}.
extern "C" int encodesim_lanes(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, void *const *dst, const int64_t *cap, int64_t *dst_bytes, int32_t *status,
                               int16_t *coef, uint32_t *code, uint64_t *end, uint64_t *istart, uint8_t *unstuffed, int64_t unstuffed_cap, uint64_t *info)
{
    Run R;
    const int rc = jda_encode_plan_jobs(n, src, bpp, jobs, dst, cap, &R.P);
    if (rc != JDA_SUCCESS) return rc;
    setup(R, (uint32_t)bpp);
    for (uint32_t b = 0; b < R.P.n_blocks; b++) {
        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, R.io);
        R.io.cur = &R.jobs[j];
        jda_en_block(R.A, R.jobs[j], b, R.io);
    }
    if (R.io.err) return R.io.err;
    const int e = finish(R, dst_bytes, status, code, end, istart, unstuffed, unstuffed_cap);
    if (e) return e;
    if (coef) memcpy(coef, R.A.coef, (size_t)R.P.n_blocks * 128);
    if (info) { info[0] = R.P.n_blocks; info[1] = R.P.n_int; info[2] = R.P.n_chunks; info[3] = R.P.u_total; }
    return 0;
}

// one w x h job whose blocks' coefficients are the caller's (64 a block, zig-zag order, the order of the scan; DC = the block's value): the
// blocks stage's two outputs are made here, the other five stages run as above
extern "C" int encodesim_coefs(int w, int h, int sampling, int quality, int ri, const int16_t *coefs, void *dst, int64_t cap, int64_t *dst_bytes, int32_t *status,
                               uint32_t *code, uint64_t *end, uint64_t *info)
{
    Run R;
    std::vector<uint8_t> pixels((size_t)w * h * 4);
    jda_output S;
    S.pixels = pixels.data(); S.pitch_bytes = w * (sampling == JDA_ENCODE_GRAY ? 1 : 4); S.width_px = w; S.rows = h;
    const jda_encode_job E = { 0, 0, w, h, sampling, quality, ri, 0 };
    const int rc = jda_encode_plan_jobs(1, &S, sampling == JDA_ENCODE_GRAY ? 1 : 4, &E, &dst, &cap, &R.P);
    if (rc != JDA_SUCCESS) return rc;
    setup(R, sampling == JDA_ENCODE_GRAY ? 1u : 4u);
    const jda_encode_dev_job &J = R.jobs[0];
    for (uint32_t b = 0; b < J.n_blocks; b++) {
        const uint32_t t = b % J.bpm < J.hs * J.vs ? 0u : 1u;
        uint32_t bits = 0, run = 0;
        for (uint32_t z = 1; z < 64u; z++) {
            const int v = coefs[(size_t)b * 64 + z];
            if (!v) { run++; continue; }
            const uint32_t sz = jda_en_nbits((uint32_t)abs(v));
            bits += (run >> 4) * (R.huff[t * 256u + 0xf0u] >> 16) + (R.huff[t * 256u + (((run & 15u) << 4) | sz)] >> 16) + sz;
            run = 0;
        }
        if (run) bits += R.huff[t * 256u] >> 16;
        memcpy(R.A.coef + (size_t)b * 64, coefs + (size_t)b * 64, 128);
        R.A.meta[b] = (bits << 16) | (uint16_t)coefs[(size_t)b * 64];
    }
    R.io.allocs[3].init.assign(R.io.allocs[3].size, 1); R.io.allocs[4].init.assign(R.io.allocs[4].size, 1);      // (coef and meta: written above)
    const int e = finish(R, dst_bytes, status, code, end, NULL, NULL, 0);
    if (e) return e;
    if (info) { info[0] = R.P.n_blocks; info[1] = R.P.n_int; info[2] = R.P.n_chunks; info[3] = R.P.u_total; }
    return 0;
}

// the scan stage alone over n lengths of the caller's (bytes_mode: the chunks' 0xFF counts, all bits of a value and no interval; else the
// blocks' code lengths, the low 16 bits, an interval every `period` elements): a workgroup's first half lane 0 .. 255 into poisoned LDS,
// its second half lane 255 DOWN TO 0 -- no lane's second half may need another's.  end: n, istart: an interval (unused in bytes_mode),
// total: the unstuffed bytes (bytes_mode: the sum), as jda_en_scan_job takes it from the one lane that owns the last element.
extern "C" int encodesim_scan(const uint32_t *vals, uint32_t n, int bytes_mode, uint32_t period, uint64_t *end, uint64_t *istart, uint64_t *total)
{
    SimIO io;
    io.cur = NULL; io.bpp = 0; io.jobs = NULL; io.n_jobs = 0; io.err = 0;
    if (!n || (bytes_mode && period)) return -60;                              // (-6x: this entry's own)
    const uint32_t mask = bytes_mode ? 0xffffffffu : 0xffffu, n_int = period ? (n + period - 1u) / period : 1u;
    io.add((void *)vals, (size_t)n * 4, false, false);
    io.add(end, (size_t)n * 8, true, true);
    if (!bytes_mode) io.add(istart, (size_t)n_int * 8, true, true);
    io.lds.assign(3 * JDA_EN_THREADS, 0xEEEEEEEEEEEEEEEEull); io.lds_set.assign(3 * JDA_EN_THREADS, 0);
    for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) jda_en_scan_local(vals, mask, 0u, n, period, tid, io);
    uint32_t owners = 0;
    for (uint32_t tid = JDA_EN_THREADS; tid-- > 0u;) {
        const uint64_t p = jda_en_scan_write(vals, mask, 0u, n, period, end, bytes_mode ? (uint64_t *)0 : istart, tid, io);
        if (p == ~(uint64_t)0) continue;
        owners++;
        *total = bytes_mode ? p : jda_en_ceil8(p) >> 3;
    }
    if (io.err) return io.err;
    if (owners != 1u) return -61;
    for (const Alloc &a : io.allocs) for (uint8_t s : a.init) if (!s) return -62;      // an element or an interval that no lane wrote
    return 0;
}

// the argument checks of jda_encode_surfaces (behind its ctx / n == 0 / null-array checks) on pointers that are never followed
extern "C" int encodesim_check(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, void *const *dst, const int64_t *cap)
{
    jda_encode_plan_out P;
    return jda_encode_plan_jobs(n, src, bpp, jobs, dst, cap, &P);
}
extern "C" int encodesim_bound(int w, int h, int sampling, int ri, int64_t *bytes) { return jda_encode_bound_bytes(w, h, sampling, ri, bytes); }
// the header of a job's file; returns its length (cap too small: nothing copied)
extern "C" int encodesim_header(int w, int h, int sampling, int quality, int ri, uint8_t *out, int cap)
{
    std::vector<uint8_t> o;
    jda_encode_header(w, h, sampling, quality, ri, o);
    if ((int)o.size() <= cap) memcpy(out, o.data(), o.size());
    return (int)o.size();
}
// every divisor 8 q, q = 1..255, against every numerator below 2^17: the number of quotients the reciprocal gets wrong
extern "C" int64_t encodesim_divide(void)
{
    int64_t bad = 0;
    for (uint32_t q = 1; q <= 255u; q++) {
        const uint32_t d = q << 3, r = jda_encode_recip(d);
        for (uint32_t a = 0; a < (1u << 17); a++) bad += (uint32_t)(((uint64_t)a * r) >> 32) != a / d;
    }
    return bad;
}
