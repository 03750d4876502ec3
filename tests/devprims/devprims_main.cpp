// devprims_main.cpp -- the host dispatchers of devprims_ops.h as a program of their own under AddressSanitizer + UBSan
// (make devprimsasan): nothing is loaded into an interpreter.  tests/test_devprims_cpu.py writes the inputs of every family into a
// file, this program runs the host loops over them and over the whole pixel cube and prints one checksum a record; the test holds
// the checksums against those of the library's host side, which it has compared with the numpy definitions element for element.
//
// file: records of { u32 family, op, n, maxsteps } + the family's arrays as the host loops take them (uint32 words; a walk's steps
// as bytes, padded to a multiple of four).  family 1 val: a b c; 2 wave: a b; 3 window reader: win[64] start[n] steps[n * maxsteps];
// 4 cube: nothing (elements 0 .. n - 1); 5 LDS: win[64] a b.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "devprims_ops.h"

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static uint64_t checksum(const std::vector<uint32_t> &v)
{
    uint64_t s = 0;
    for (size_t i = 0; i < v.size(); i++) s += (uint64_t)v[i] * (uint64_t)(i + 1);
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: devprims_asan <records>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t h[4];
    int rec = 0;
    while (fread(h, 4, 4, f) == 4) {
        const uint32_t family = h[0], n = h[2], ms = h[3];
        const int op = (int)h[1];
        if (n > (1u << 24) || ms > 4096u) { fprintf(stderr, "record %d: sizes\n", rec); return 1; }
        std::vector<uint32_t> a(n), b(n), c(n), out, win(DP_WIN_BYTES / 4u);
        bool ok = true;
        if (family == 1) {
            ok = rd(f, a.data(), 4u * n) && rd(f, b.data(), 4u * n) && rd(f, c.data(), 4u * n);
            out.assign(n, 0u);
            if (ok) dp_host_val(op, a.data(), b.data(), c.data(), out.data(), (int)n);
        } else if (family == 2) {
            ok = n % 64u == 0 && rd(f, a.data(), 4u * n) && rd(f, b.data(), 4u * n);
            out.assign(2u * (size_t)n, 0u);
            if (ok) dp_host_wave(op, a.data(), b.data(), out.data(), (int)n);
        } else if (family == 3) {
            const size_t sb = ((size_t)n * ms + 3u) & ~(size_t)3u;
            std::vector<uint8_t> steps(sb);
            ok = rd(f, win.data(), DP_WIN_BYTES) && rd(f, a.data(), 4u * n) && rd(f, steps.data(), sb);
            out.assign((size_t)n * ms, 0u);
            if (ok) dp_host_wr(win.data(), a.data(), steps.data(), out.data(), (int)n, (int)ms);
        } else if (family == 4) {
            out.assign(n, 0u);
            dp_host_cube(op, out.data(), 0u, (int)n);
        } else if (family == 5) {
            ok = n % 64u == 0 && rd(f, win.data(), DP_WIN_BYTES) && rd(f, a.data(), 4u * n) && rd(f, b.data(), 4u * n);
            out.assign(n, 0u);
            if (ok) dp_host_lds(op, win.data(), a.data(), b.data(), out.data(), (int)n);
        } else ok = false;
        if (!ok) { fprintf(stderr, "record %d: malformed\n", rec); return 1; }
        printf("rec %d %u %d %016llx\n", rec, family, op, (unsigned long long)checksum(out));
        rec++;
    }
    fclose(f);
    printf("devprims_asan ok %d\n", rec);
    return 0;
}
