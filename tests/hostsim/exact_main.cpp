// tests/hostsim/exact_main.cpp -- TEST INFRASTRUCTURE: exact_sim.cpp with a main of its own, built under AddressSanitizer + UBSan (make
// exactasan): the plan and every lane of the exact decode over the files named on the command line -- a baseline file as a resident
// baseline image, a progressive one as a dense and as a sparse coefficient image --, RGB8888 and gray, each held to the row-major twin.
// A program: nothing is loaded into an interpreter.  Prints "exact_asan ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int exactsim_plan(int width, int height, int ncomp, int subsample, int adobe, int pixel_type, int luma_only, int baseline_image, int jpeg_type, int n_mcus_ok,
                             int64_t *out);
extern "C" int exactsim_run(const uint8_t *jpeg, int len, const int16_t *coefs, uint32_t n_blocks, int source, int pixel_type, uint8_t *out, int pitch, int width_px,
                            int rows, uint8_t *twin_out, uint8_t *planes_out, uint8_t *twin_planes, int32_t *info);

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: exact_asan file.jpg ..\n"); return 2; }
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint8_t> jpeg;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) jpeg.insert(jpeg.end(), buf, buf + n);
        fclose(f);
        jda_image_info I;
        if (jda_parse(jpeg.data(), (int32_t)jpeg.size(), &I) != JDA_SUCCESS) { fprintf(stderr, "%s: not parsed\n", argv[a]); return 1; }
        int64_t plan[12];
        if (exactsim_plan(I.width, I.height, I.ncomp, I.subsample, 0, JDA_RGB8888, 0, 0, 0, -1, plan) != JDA_SUCCESS || plan[11] <= 0) { fprintf(stderr, "%s: plan\n", argv[a]); return 1; }
        if (exactsim_plan(I.width, I.height, I.ncomp, I.subsample, 0, JDA_RGB565_LITTLE_ENDIAN, 0, 0, 0, -1, plan) != JDA_INVALID_PARAMETER) { fprintf(stderr, "%s: pixel type\n", argv[a]); return 1; }
        if (exactsim_plan(I.width, I.height, I.ncomp, I.subsample, 0, JDA_RGB8888, 0, 1, 0, I.mcus_x * I.mcus_y - 1, plan) != JDA_DECODE_ERROR) { fprintf(stderr, "%s: bad MCU\n", argv[a]); return 1; }
        for (int source = (I.jpeg_type == 1 ? 0 : 2); source <= (I.jpeg_type == 1 ? 1 : 2); source++)
            for (int pt = JDA_RGB8888; pt <= JDA_EIGHT_BIT_GRAYSCALE; pt++) {
                const int bpp = pt == JDA_RGB8888 ? 4 : 1, pitch = (I.width * bpp + 15) & ~15;
                uint8_t *out = NULL;
                if (posix_memalign((void **)&out, 16, (size_t)pitch * I.height) != 0) return 2;
                memset(out, 0x5A, (size_t)pitch * I.height);
                std::vector<uint8_t> twin((size_t)I.width * bpp * I.height), planes((size_t)I.width * I.height * 3, 0), tplanes((size_t)I.width * I.height * 3, 0);
                int32_t info[5];
                // (a gray surface of a colour file decodes no chroma: its planes are not asked for)
                const bool want_planes = !(pt == JDA_EIGHT_BIT_GRAYSCALE && I.ncomp == 3);
                const int rc = exactsim_run(jpeg.data(), (int)jpeg.size(), NULL, 0, source, pt, out, pitch, I.width, I.height, twin.data(), want_planes ? planes.data() : NULL,
                                            want_planes ? tplanes.data() : NULL, info);
                bool ok = rc == 0 && info[0] > 0 && info[3] == 0 && info[4] == 0 && planes == tplanes;
                for (int y = 0; ok && y < I.height; y++) ok = memcmp(out + (size_t)y * pitch, twin.data() + (size_t)y * I.width * bpp, (size_t)I.width * bpp) == 0;
                free(out);
                if (!ok) { fprintf(stderr, "%s: source %d pixel type %d: rc %d, twice %d, outside %d\n", argv[a], source, pt, rc, info[3], info[4]); return 1; }
            }
    }
    printf("exact_asan ok\n");
    return 0;
}
