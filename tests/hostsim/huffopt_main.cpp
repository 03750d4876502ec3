// tests/hostsim/huffopt_main.cpp -- TEST INFRASTRUCTURE: the optimised encode's plan, table builder and lane simulator (huffopt_sim.cpp) as a
// program of its own, built under AddressSanitizer + UBSan (make huffoptasan): nothing is loaded into an interpreter.  It encodes batches of
// rectangles of every sampling, optimised and standard jobs alternating, 1 x 1 jobs between larger ones, out of exactly sized surfaces into
// exactly sized heap blocks -- once at the bound, once at the exact size with one job a byte short --, checks that an optimised file is no
// longer than the standard one, runs the table builder over histograms of its own (one symbol, all 256, Fibonacci-like counts that pass 16 bits
// before the lengths are limited) and the refusals.  Exit status 0 and "huffopt_asan ok" when every call answers as it must.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int huffoptsim_lanes(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, const uint32_t *job_flags, void *const *dst, const int64_t *cap,
                                int64_t *dst_bytes, int32_t *status, int16_t *coef, uint32_t *code, uint64_t *end, uint32_t *hist, uint64_t *info);
extern "C" int huffoptsim_table(const uint32_t *freq, uint8_t *bits, uint8_t *vals, uint32_t *n_vals);
extern "C" int huffoptsim_check(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, const uint32_t *job_flags, void *const *dst, const int64_t *cap);
extern "C" int encodesim_bound(int w, int h, int sampling, int ri, int64_t *bytes);

#define CHECK(c) do { if (!(c)) { printf("huffopt_asan: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// Kraft's sum of a table in units of 2^-16: at most 2^16 - 1 (the all-ones code stays free), and n_vals symbols
static bool sound(const uint8_t *bits, uint32_t n_vals)
{
    uint32_t k = 0, n = 0;
    for (int len = 1; len <= 16; len++) { k += (uint32_t)bits[len - 1] << (16 - len); n += bits[len - 1]; }
    return n == n_vals && k < 65536u;
}

int main()
{
    uint32_t seed = 54321u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
    const int sizes[][2] = { { 1, 1 }, { 17, 9 }, { 1, 1 }, { 25, 16 }, { 264, 240 }, { 1, 1 }, { 40, 40 } };
    for (int sampling = 0; sampling < 4; sampling++) {
        const int bpp = sampling == 0 ? 1 : 4, n = 7;
        std::vector<std::vector<uint8_t>> surf(n);
        std::vector<jda_output> src(n);
        std::vector<jda_encode_job> jobs(n);
        std::vector<uint32_t> flags(n);
        std::vector<int64_t> cap(n), bytes(n), plain(n);
        std::vector<int32_t> status(n);
        for (int i = 0; i < n; i++) {
            const int w = sizes[i][0], h = sizes[i][1], pitch = (w + 5) * bpp, ri = i == 3 ? 1 : i == 4 ? 7 : 0;
            surf[i].resize((size_t)pitch * (h + 3));                       // exactly the surface: a load behind it is the sanitizer's
            for (uint8_t &b : surf[i]) b = (uint8_t)(i == 6 ? 200 : rnd());
            src[i].pixels = surf[i].data(); src[i].pitch_bytes = pitch; src[i].width_px = w + 5; src[i].rows = h + 3;
            jobs[i] = { 3, 2, w, h, sampling, i == 3 ? 100 : 75, ri, 0 };
            CHECK(encodesim_bound(w, h, sampling, ri, &cap[i]) == 0);
        }
        // pass 0: no flags, the bound; 1: the even jobs optimised; 2: the odd ones; 3: the odd ones at the exact sizes, job 1 a byte short
        for (int pass = 0; pass < 4; pass++) {
            for (int i = 0; i < n; i++) flags[i] = pass == 0 ? 0u : (uint32_t)(pass == 1 ? (i & 1) ^ 1 : i & 1);
            std::vector<std::vector<uint8_t>> file(n);
            std::vector<void *> dst(n);
            for (int i = 0; i < n; i++) { file[i].assign((size_t)cap[i], 0x5a); dst[i] = file[i].data(); }
            std::vector<uint32_t> hist((size_t)n * 544u);
            uint64_t info[5] = { 0, 0, 0, 0, 0 };
            CHECK(huffoptsim_lanes(n, src.data(), bpp, jobs.data(), pass == 0 ? NULL : flags.data(), dst.data(), cap.data(), bytes.data(), status.data(), NULL, NULL, NULL,
                                   hist.data(), info) == 0);
            CHECK(info[4] == (pass == 0 ? 0u : pass == 1 ? 4u : 3u));
            for (int i = 0; i < n; i++) {
                if (pass == 3 && i == 1) { CHECK(status[i] == JDA_ERROR_MEMORY && bytes[i] == cap[i] + 1 && file[i][0] == 0x5a); continue; }
                CHECK(status[i] == 0 && bytes[i] <= cap[i] && file[i][0] == 0xff && file[i][1] == 0xd8 && file[i][(size_t)bytes[i] - 1] == 0xd9);
                if (pass == 0) plain[i] = bytes[i];
                else if (flags[i]) CHECK(bytes[i] < plain[i]);             // (these pictures: the file shrinks)
                else CHECK(bytes[i] == plain[i]);
            }
            if (pass == 1) {                                               // the first histogram is job 0's, 1 x 1: one MCU, every block in a DC bin
                uint32_t dc = 0;
                for (size_t k = 512; k < 544; k++) dc += hist[k];
                CHECK(dc == (sampling == 0 ? 1u : sampling == 1 ? 3u : sampling == 2 ? 4u : 6u));
            }
            if (pass == 2) for (int i = 0; i < n; i++) cap[i] = bytes[i] - (i == 1 ? 1 : 0);
        }
        // the refusals: a flag bit that is not one, and the block cap (the pointers are never followed)
        std::vector<uint8_t> f((size_t)cap[0] + 1);
        void *d0 = f.data();
        uint32_t bad = 2u, opt = JDA_ENCODE_OPTIMIZE;
        CHECK(huffoptsim_check(1, src.data(), bpp, jobs.data(), &opt, &d0, cap.data()) == 0);
        CHECK(huffoptsim_check(1, src.data(), bpp, jobs.data(), &bad, &d0, cap.data()) == JDA_INVALID_PARAMETER);
        bad = 0x80000001u;
        CHECK(huffoptsim_check(1, src.data(), bpp, jobs.data(), &bad, &d0, cap.data()) == JDA_INVALID_PARAMETER);
        CHECK(huffoptsim_check(0, src.data(), bpp, jobs.data(), &opt, &d0, cap.data()) == JDA_INVALID_PARAMETER);
    }
    {
        static uint8_t wide[8];
        jda_output S;
        S.pixels = wide; S.pitch_bytes = 65536; S.width_px = 65535; S.rows = 65535;
        uint8_t file[8];
        void *d0 = file;
        int64_t cap = 8;
        uint32_t opt = JDA_ENCODE_OPTIMIZE;
        jda_encode_job E = { 0, 0, 25000, 40000, 0, 75, 0, 0 };           // 3125 x 5000 = 15,625,000 blocks: the most
        CHECK(huffoptsim_check(1, &S, 1, &E, &opt, &d0, &cap) == 0);
        E.h = 40001;
        CHECK(huffoptsim_check(1, &S, 1, &E, &opt, &d0, &cap) == JDA_UNSUPPORTED_FEATURE);
        CHECK(huffoptsim_check(1, &S, 1, &E, NULL, &d0, &cap) == 0);
    }
    // the table builder over histograms of its own
    {
        uint32_t freq[256];
        uint8_t bits[16], vals[256];
        uint32_t nv = 0;
        memset(freq, 0, sizeof(freq));
        freq[0x21] = 7u;                                                   // one symbol: a code of one bit
        CHECK(huffoptsim_table(freq, bits, vals, &nv) == 0 && nv == 1u && bits[0] == 1 && vals[0] == 0x21 && sound(bits, nv));
        for (int i = 0; i < 256; i++) freq[i] = 1u + (uint32_t)rnd();     // all 256
        CHECK(huffoptsim_table(freq, bits, vals, &nv) == 0 && nv == 256u && sound(bits, nv));
        memset(freq, 0, sizeof(freq));
        uint32_t a = 1, b = 2;
        for (int i = 0; i < 30; i++) { freq[i * 5] = a; const uint32_t c = a + b + 1u; a = b; b = c; }      // a(n) = a(n-1) + a(n-2) + 1, no ties: lengths up to 30 before the limit
        CHECK(huffoptsim_table(freq, bits, vals, &nv) == 0 && nv == 30u && sound(bits, nv) && bits[15] > 0);
        for (int i = 0; i < 256; i++) freq[i] = 1000000000u / 256u;        // counts that sum to 10^9
        CHECK(huffoptsim_table(freq, bits, vals, &nv) == 0 && nv == 256u && sound(bits, nv));
        memset(freq, 0, sizeof(freq));
        a = 1; b = 2;
        for (int i = 0; i < 40; i++) { freq[i] = a; const uint32_t c = a + b + 1u; a = b; b = c; }         // 40 of them (7 x 10^8 in all): a code of more than 32 bits, libjpeg gives up
        CHECK(huffoptsim_table(freq, bits, vals, &nv) == 1);
    }
    printf("huffopt_asan ok\n");
    return 0;
}
