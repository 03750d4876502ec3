// tests/hostsim/exact_scaled_main.cpp -- TEST INFRASTRUCTURE: exact_scaled_sim.cpp with a main of its own, built under AddressSanitizer +
// UBSan (make exactscaledasan): the plan and every lane of the scaled exact decode over the files named on the command line -- a baseline
// file as a resident baseline image, a progressive one as a dense and as a sparse coefficient image --, at 1/2, 1/4 and 1/8, RGB8888 and
// gray, whole and clipped, each held to the row-major twin.  A program: nothing is loaded into an interpreter.  Prints "exact_scaled_asan ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int exactscaledsim_plan(int width, int height, int ncomp, int subsample, int adobe, int pixel_type, int luma_only, int scale, int64_t *out);
extern "C" int exactscaledsim_run(const uint8_t *jpeg, int len, const int16_t *coefs, uint32_t n_blocks, int source, int pixel_type, int scale, uint8_t *out, int pitch,
                                  int width_px, int rows, uint8_t *twin_out, uint8_t *planes_out, uint8_t *twin_planes, int32_t *info);

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: exact_scaled_asan file.jpg ..\n"); return 2; }
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint8_t> jpeg;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) jpeg.insert(jpeg.end(), buf, buf + n);
        fclose(f);
        jda_image_info I;
        if (jda_parse(jpeg.data(), (int32_t)jpeg.size(), &I) != JDA_SUCCESS) { fprintf(stderr, "%s: not parsed\n", argv[a]); return 1; }
        int64_t plan[16];
        if (exactscaledsim_plan(I.width, I.height, I.ncomp, I.subsample, 0, JDA_RGB8888, 0, 3, plan) != JDA_INVALID_PARAMETER) { fprintf(stderr, "%s: scale 3\n", argv[a]); return 1; }
        for (int scale = 2; scale <= 8; scale *= 2) {
            if (exactscaledsim_plan(I.width, I.height, I.ncomp, I.subsample, 0, JDA_RGB8888, 0, scale, plan) != JDA_SUCCESS || plan[15] <= 0) { fprintf(stderr, "%s: plan\n", argv[a]); return 1; }
            const int ow = (int)plan[3], oh = (int)plan[4];
            for (int source = (I.jpeg_type == 1 ? 0 : 2); source <= (I.jpeg_type == 1 ? 1 : 2); source++)
                for (int pt = JDA_RGB8888; pt <= JDA_EIGHT_BIT_GRAYSCALE; pt++)
                    for (int clip = 0; clip < 2; clip++) {
                        const int bpp = pt == JDA_RGB8888 ? 4 : 1, pitch = (ow * bpp + 15) & ~15;
                        const int cw = clip ? (ow > 1 ? ow - 1 : ow) : ow, ch = clip ? (oh + 1) / 2 : oh;
                        uint8_t *out = NULL;
                        if (posix_memalign((void **)&out, 16, (size_t)pitch * oh) != 0) return 2;
                        memset(out, 0x5A, (size_t)pitch * oh);
                        std::vector<uint8_t> twin((size_t)ow * bpp * oh), planes((size_t)ow * oh * 3 + 64, 0), tplanes((size_t)ow * oh * 3 + 64, 0);
                        int32_t info[8];
                        // (a gray surface of a colour file decodes no chroma: its planes are not asked for)
                        const bool want_planes = !(pt == JDA_EIGHT_BIT_GRAYSCALE && I.ncomp == 3);
                        const int rc = exactscaledsim_run(jpeg.data(), (int)jpeg.size(), NULL, 0, source, pt, scale, out, pitch, cw, ch, twin.data(),
                                                          want_planes ? planes.data() : NULL, want_planes ? tplanes.data() : NULL, info);
                        bool ok = rc == 0 && info[0] > 0 && info[3] == 0 && info[4] == 0 && info[6] == 0 && info[7] == 0 && planes == tplanes;
                        for (int y = 0; ok && y < oh; y++)
                            for (int x = 0; ok && x < pitch; x++) {
                                const bool visible = y < ch && x < cw * bpp;
                                ok = out[(size_t)y * pitch + x] == (visible ? twin[(size_t)y * ow * bpp + x] : 0x5A);
                            }
                        free(out);
                        if (!ok) {
                            fprintf(stderr, "%s: scale %d source %d pixel type %d clip %d: rc %d, twice %d, outside %d, planes twice %d, unwritten %d\n", argv[a], scale, source, pt,
                                    clip, rc, info[3], info[4], info[6], info[7]);
                            return 1;
                        }
                    }
        }
    }
    printf("exact_scaled_asan ok\n");
    return 0;
}
