// tests/hostsim/exact_adobe_main.cpp -- TEST INFRASTRUCTURE: exact_adobe_sim.cpp with a main of its own, built under AddressSanitizer + UBSan
// (make exactadobeasan): the plan, the host scan decoder (jda_coef_prepare) and every lane of the colour-model decode over the files named
// on the command line -- whole and clipped, a four-component file to RGB8888 and CMYK8888, a one- or three-component one at 1, 1/2, 1/4
// and 1/8 --, the full-size results held to the row-major twin.  A program: nothing is loaded into an interpreter.  Prints "exact_adobe_asan ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int exactadobesim_plan(int width, int height, int ncomp, int subsample, int k_hv, int colour, int pixel_type, int scale, int baseline_image, int64_t *out);
extern "C" int exactadobesim_run(const uint8_t *jpeg, int len, int pixel_type, int scale, uint8_t *out, int pitch, int width_px, int rows, uint8_t *twin_out,
                                 uint8_t *planes_out, int32_t *info);

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: exact_adobe_asan file.jpg ..\n"); return 2; }
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint8_t> jpeg;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) jpeg.insert(jpeg.end(), buf, buf + n);
        fclose(f);
        jda_exact_file E;
        if (jda_exact_probe(jpeg.data(), (int32_t)jpeg.size(), &E) != JDA_SUCCESS) { fprintf(stderr, "%s: not probed\n", argv[a]); return 1; }
        const bool four = E.ncomp == 4;
        const int sub[5] = { 0, 0x11, 0x22, 0x21, 0x12 };
        int64_t plan[16];
        if (exactadobesim_plan(E.width, E.height, E.ncomp, sub[E.layout], E.k_sampling, E.colour_model, JDA_RGB8888, 1, 0, plan) != JDA_SUCCESS || plan[15] <= 0) {
            fprintf(stderr, "%s: plan\n", argv[a]); return 1;
        }
        if (four && exactadobesim_plan(E.width, E.height, 4, sub[E.layout], E.k_sampling, E.colour_model, JDA_RGB8888, 2, 0, plan) != JDA_UNSUPPORTED_FEATURE) {
            fprintf(stderr, "%s: a scaled four-component plan\n", argv[a]); return 1;
        }
        for (int pt = 0; pt < (four ? 2 : 1); pt++)
            for (int scale = 1; scale <= (four ? 1 : 8); scale *= 2)
                for (int clip = 0; clip < 2; clip++) {
                    const int pixel_type = pt ? (int)JDA_CMYK8888 : (int)JDA_RGB8888;
                    const int w = (E.width + scale - 1) / scale, h = (E.height + scale - 1) / scale;
                    const int cw = clip ? (w > 1 ? w - 1 : w) : w, ch = clip ? (h + 1) / 2 : h, pitch = (w * 4 + 15) & ~15;
                    uint8_t *out = NULL;
                    if (posix_memalign((void **)&out, 16, (size_t)pitch * h) != 0) return 2;
                    memset(out, 0x5A, (size_t)pitch * h);
                    std::vector<uint8_t> twin((size_t)w * h * 4), planes((size_t)E.width * E.height * 4 + 64);
                    int32_t info[8];
                    const int rc = exactadobesim_run(jpeg.data(), (int)jpeg.size(), pixel_type, scale, out, pitch, cw, ch, twin.data(), planes.data(), info);
                    bool ok = rc == 0 && info[0] > 0 && info[3] == 0 && info[4] == 0 && info[6] == 0 && (scale > 1 || info[7] == 1);
                    for (int y = 0; ok && scale == 1 && y < ch; y++) ok = memcmp(out + (size_t)y * pitch, twin.data() + (size_t)y * w * 4, (size_t)cw * 4) == 0;
                    free(out);
                    if (!ok) { fprintf(stderr, "%s: pixel type %d scale %d clip %d: rc %d, twice %d, outside %d, planes %d\n", argv[a], pixel_type, scale, clip, rc, info[3], info[4], info[6]); return 1; }
                }
    }
    printf("exact_adobe_asan ok\n");
    return 0;
}
