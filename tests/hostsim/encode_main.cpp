// tests/hostsim/encode_main.cpp -- TEST INFRASTRUCTURE: the encode plan, header builder and lane simulator (encode_sim.cpp) as a program of
// its own, built under AddressSanitizer + UBSan (make encodeasan): nothing is loaded into an interpreter.  It encodes a batch of rectangles of
// every sampling out of guard-surrounded surfaces into exactly sized heap blocks, once more one byte short -- among them two long jobs (gray
// 264 x 240 and 4:2:0 352 x 352, an interval an MCU: a lane of the scan stage walks a run of blocks with several interval starts, and one of
// chunks) --, a worst-case tile from chosen coefficients, and runs the refusals.  Exit status 0 and "encode_asan ok" when every call answers as it must.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int encodesim_lanes(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, void *const *dst, const int64_t *cap, int64_t *dst_bytes, int32_t *status,
                               int16_t *coef, uint32_t *code, uint64_t *end, uint64_t *istart, uint8_t *unstuffed, int64_t unstuffed_cap, uint64_t *info);
extern "C" int encodesim_coefs(int w, int h, int sampling, int quality, int ri, const int16_t *coefs, void *dst, int64_t cap, int64_t *dst_bytes, int32_t *status,
                               uint32_t *code, uint64_t *end, uint64_t *info);
extern "C" int encodesim_scan(const uint32_t *vals, uint32_t n, int bytes_mode, uint32_t period, uint64_t *end, uint64_t *istart, uint64_t *total);
extern "C" int encodesim_check(int n, const jda_output *src, int bpp, const jda_encode_job *jobs, void *const *dst, const int64_t *cap);
extern "C" int encodesim_bound(int w, int h, int sampling, int ri, int64_t *bytes);

#define CHECK(c) do { if (!(c)) { printf("encode_asan: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    uint32_t seed = 12345u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
    const int sizes[][2] = { { 1, 1 }, { 17, 9 }, { 40, 40 }, { 129, 65 }, { 7, 64 }, { 264, 240 }, { 352, 352 } };
    for (int sampling = 0; sampling < 4; sampling++) {
        const int bpp = sampling == 0 ? 1 : 4, n = sampling == 0 || sampling == 3 ? 6 : 5, big = sampling == 0 ? 5 : 6;      // (the long job: the last)
        std::vector<std::vector<uint8_t>> surf(n);
        std::vector<jda_output> src(n);
        std::vector<jda_encode_job> jobs(n);
        std::vector<int64_t> cap(n), bytes(n);
        std::vector<int32_t> status(n);
        for (int i = 0; i < n; i++) {
            const int k = i < 5 ? i : big, ri = i < 5 ? i : 1, w = sizes[k][0], h = sizes[k][1], pitch = (w + 5) * bpp;
            surf[i].resize((size_t)pitch * (h + 3));                       // exactly the surface: a load behind it is the sanitizer's
            for (uint8_t &b : surf[i]) b = (uint8_t)rnd();
            src[i].pixels = surf[i].data(); src[i].pitch_bytes = pitch; src[i].width_px = w + 5; src[i].rows = h + 3;
            jobs[i] = { 3, 2, w, h, sampling, i == 2 ? 100 : 75, ri, 0 };
            CHECK(encodesim_bound(w, h, sampling, ri, &cap[i]) == 0);
        }
        for (int pass = 0; pass < 2; pass++) {                             // the bound, then the exact size with one job a byte short
            std::vector<std::vector<uint8_t>> file(n);
            std::vector<void *> dst(n);
            for (int i = 0; i < n; i++) { file[i].assign((size_t)cap[i], 0x5a); dst[i] = file[i].data(); }
            CHECK(encodesim_lanes(n, src.data(), bpp, jobs.data(), dst.data(), cap.data(), bytes.data(), status.data(), NULL, NULL, NULL, NULL, NULL, 0, NULL) == 0);
            for (int i = 0; i < n; i++) {
                if (pass == 1 && i == 1) { CHECK(status[i] == JDA_ERROR_MEMORY && bytes[i] == cap[i] + 1 && file[i][0] == 0x5a); continue; }
                CHECK(status[i] == 0 && bytes[i] <= cap[i] && file[i][0] == 0xff && file[i][1] == 0xd8 && file[i][(size_t)bytes[i] - 1] == 0xd9);
                cap[i] = bytes[i] - (i == 1 ? 1 : 0);
            }
        }
        void *d0 = surf[0].data();
        CHECK(encodesim_check(1, src.data(), bpp, jobs.data(), &d0, cap.data()) == JDA_INVALID_PARAMETER);      // a file over its own source
        jobs[0].quality = 0;
        std::vector<uint8_t> f((size_t)cap[0] + 1);
        d0 = f.data();
        CHECK(encodesim_check(1, src.data(), bpp, jobs.data(), &d0, cap.data()) == JDA_INVALID_PARAMETER);
    }
    // a tile of 64 4:4:4 blocks at the longest code a block can have: every AC +-1023 .. (category 10), DC differences of category 11
    {
        const int w = 8 * 22, h = 8;                                        // 66 blocks: 22 MCUs of three
        std::vector<int16_t> coefs(66 * 64);
        for (int b = 0; b < 66; b++) {
            coefs[(size_t)b * 64] = (int16_t)(((b / 3) & 1) ? 1023 : -1024);
            for (int z = 1; z < 64; z++) coefs[(size_t)b * 64 + z] = (int16_t)((z & 1) ? 1023 : -1023);
        }
        int64_t cap = 0, bytes = 0;
        int32_t status = -1;
        CHECK(encodesim_bound(w, h, 1, 0, &cap) == 0);
        std::vector<uint8_t> file((size_t)cap);
        CHECK(encodesim_coefs(w, h, 1, 100, 0, coefs.data(), file.data(), cap, &bytes, &status, NULL, NULL, NULL) == 0);
        CHECK(status == 0 && bytes <= cap);
    }
    // the scan stage alone over exactly sized arrays: 1000 blocks of the longest code, an interval every 3 (four a lane, several starts a run),
    // and 513 chunks (three a lane, the last lanes empty)
    {
        std::vector<uint32_t> vals(1000, 1665u);
        std::vector<uint64_t> end(1000), istart(334);
        uint64_t total = 0;
        CHECK(encodesim_scan(vals.data(), 1000, 0, 3, end.data(), istart.data(), &total) == 0);
        CHECK(istart[333] == 333u * 625u && end[999] == 333u * 5000u + 1665u && total == 333u * 625u + 209u);      // ceil8(3 x 1665) = 5000 bits
        vals.assign(513, 64u); end.assign(513, 0);
        CHECK(encodesim_scan(vals.data(), 513, 1, 0, end.data(), NULL, &total) == 0);
        CHECK(end[512] == 513u * 64u && total == 513u * 64u);
    }
    printf("encode_asan ok\n");
    return 0;
}
