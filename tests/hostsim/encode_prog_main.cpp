// tests/hostsim/encode_prog_main.cpp -- TEST INFRASTRUCTURE: the progressive encode's plan and lane simulator (encode_prog_sim.cpp) as a
// program of its own, built under AddressSanitizer + UBSan (make encodeprogasan): nothing is loaded into an interpreter.  It encodes batches
// of rectangles of every sampling, 1 x 1 jobs between larger ones, out of exactly sized surfaces into exactly sized heap blocks -- once at
// the bound, once at the exact sizes with one job a byte short --, a repeated block at quality 100 (runs cut by the 937 rule), the
// run-resolution stage alone at its limits, and the refusals.  Exit status 0 and "encode_prog_asan ok" when every call answers as it must.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int encodeprogsim_lanes(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, void *const *dst, const int64_t *cap, int64_t *dst_bytes, int32_t *status,
                                   uint32_t *cls, uint32_t *run, uint32_t *len, uint64_t *end, uint32_t *hist, uint64_t *seginfo, uint8_t *hdr, int64_t hdr_cap, uint64_t *info);
extern "C" int encodeprogsim_resolve(const uint32_t *cls, uint32_t n, uint32_t *run);
extern "C" int encodeprogsim_check(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, void *const *dst, const int64_t *cap);
extern "C" int encodeprogsim_bound(int w, int h, int sampling, int64_t *bytes);

#define CHECK(c) do { if (!(c)) { printf("encode_prog_asan: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    uint32_t seed = 97531u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
    const int sizes[][2] = { { 1, 1 }, { 17, 9 }, { 1, 1 }, { 25, 16 }, { 160, 16 }, { 1, 1 }, { 264, 24 } };
    for (int sampling = 0; sampling < 4; sampling++) {
        const int bpp = sampling == 0 ? 1 : 4, n = 7;
        std::vector<std::vector<uint8_t>> surf(n);
        std::vector<jda_output> src(n);
        std::vector<jda_encode_job> jobs(n);
        std::vector<int64_t> cap(n), bytes(n), exact(n);
        std::vector<int32_t> status(n);
        uint8_t tile[64];
        for (uint8_t &b : tile) b = (uint8_t)rnd();
        for (int i = 0; i < n; i++) {
            const int w = sizes[i][0], h = sizes[i][1], pitch = (w + 5) * bpp;
            surf[i].resize((size_t)pitch * (h + 3));                       // exactly the surface: a load behind it is the sanitizer's
            for (size_t k = 0; k < surf[i].size(); k++) {
                const size_t y = k / (size_t)pitch, x = (k % (size_t)pitch) / (size_t)bpp;
                surf[i][k] = i == 4 ? tile[((y + 6) % 8) * 8 + (x + 5) % 8] : i == 6 ? 200 : (uint8_t)rnd();      // job 4: one block repeated, job 6: flat
            }
            src[i].pixels = surf[i].data(); src[i].pitch_bytes = pitch; src[i].width_px = w + 5; src[i].rows = h + 3;
            jobs[i] = { 3, 2, w, h, sampling, i == 4 || i == 3 ? 100 : 75, 0, 0 };
            CHECK(encodeprogsim_bound(w, h, sampling, &cap[i]) == 0);
        }
        for (int pass = 0; pass < 2; pass++) {                             // 0: the bound; 1: the exact sizes, job 1 a byte short
            std::vector<std::vector<uint8_t>> file(n);
            std::vector<void *> dst(n);
            for (int i = 0; i < n; i++) { file[i].assign((size_t)cap[i], 0x5a); dst[i] = file[i].data(); }
            uint64_t info[5] = { 0, 0, 0, 0, 0 };
            CHECK(encodeprogsim_lanes(n, src.data(), bpp, jobs.data(), dst.data(), cap.data(), bytes.data(), status.data(), NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, info) == 0);
            CHECK(info[2] == (uint64_t)n * (sampling == 0 ? 6u : 10u));
            for (int i = 0; i < n; i++) {
                if (pass == 1 && i == 1) { CHECK(status[i] == JDA_ERROR_MEMORY && bytes[i] == cap[i] + 1 && file[i][0] == 0x5a); continue; }
                CHECK(status[i] == 0 && bytes[i] <= cap[i] && file[i][0] == 0xff && file[i][1] == 0xd8 && file[i][(size_t)bytes[i] - 2] == 0xff && file[i][(size_t)bytes[i] - 1] == 0xd9);
                if (pass == 0) exact[i] = bytes[i]; else CHECK(bytes[i] == exact[i]);
            }
            if (pass == 0) for (int i = 0; i < n; i++) cap[i] = bytes[i] - (i == 1 ? 1 : 0);
        }
        std::vector<uint8_t> f(4096);
        void *d0 = f.data();
        int64_t c0 = 4096;
        CHECK(encodeprogsim_check(1, src.data(), bpp, jobs.data(), &d0, &c0) == 0);
        jda_encode_job bad = jobs[0];
        bad.restart_interval = 1;
        CHECK(encodeprogsim_check(1, src.data(), bpp, &bad, &d0, &c0) == JDA_INVALID_PARAMETER);
        CHECK(encodeprogsim_check(0, src.data(), bpp, jobs.data(), &d0, &c0) == JDA_INVALID_PARAMETER);
    }
    {   // the run-resolution stage alone: 937 and 938 buffered bits, runs of 0x7FFF and one more, stretches of one
        std::vector<uint32_t> cls, run;
        auto joins = [](uint32_t bits) { return 2u | (bits << 8); };
        cls.assign(14, joins(63)); cls.push_back(joins(55)); cls.push_back(joins(1)); cls.push_back(joins(1));
        run.assign(cls.size(), 0);
        CHECK(encodeprogsim_resolve(cls.data(), (uint32_t)cls.size(), run.data()) == 0);
        CHECK(run[0] == (0xC0000000u | (16u << 10) | 938u) && run[16] == (0xC0000000u | (1u << 10) | 1u));
        cls[14] = joins(56);
        CHECK(encodeprogsim_resolve(cls.data(), (uint32_t)cls.size(), run.data()) == 0);
        CHECK(run[0] == (0xC0000000u | (15u << 10) | 938u) && run[15] == (0xC0000000u | (2u << 10) | 2u));
        cls.assign(32768, 2u); run.assign(32768, 0);
        CHECK(encodeprogsim_resolve(cls.data(), 32768u, run.data()) == 0);
        CHECK(run[0] == (0xC0000000u | (32767u << 10)) && run[32766] == (0x80000000u | (32766u << 10)) && run[32767] == (0xC0000000u | (1u << 10)));
        CHECK(encodeprogsim_resolve(cls.data(), 32767u, run.data()) == 0);
        const uint32_t ones[6] = { 2u, 1u, 3u, 3u, 1u, 2u };
        CHECK(encodeprogsim_resolve(ones, 6u, run.data()) == 0);
        CHECK(run[0] == (0xC0000000u | (1u << 10)) && run[1] == 0u && run[2] == run[0] && run[3] == run[0] && run[4] == 0u && run[5] == run[0]);
    }
    printf("encode_prog_asan ok\n");
    return 0;
}
