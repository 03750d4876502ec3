// tests/hostsim/exact_rect_main.cpp -- TEST INFRASTRUCTURE: exact_rect_sim.cpp with a main of its own, built under AddressSanitizer + UBSan
// (make exactrectasan): the rectangle plan and every lane of the planes and colour stages over the files named on the command line -- a
// baseline file as a resident baseline image, a progressive one as a dense and as a sparse coefficient image --, at every scale, RGB8888
// and gray, whole, at every alignment and parity, at the image's edges and clipped; each rectangle's pixels are held to the crop of the
// whole-image rectangle's.  In front of the files the plan of a whole call (jda_exact_plan_build / _place) over a mixed batch made of header
// numbers.  A program: nothing is loaded into an interpreter.  Prints "exact_rect_asan ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int exactrectsim_plan(int width, int height, int ncomp, int subsample, int pixel_type, int scale, const int32_t *rect, int32_t *mcu);
extern "C" int exactrectsim_run(const uint8_t *jpeg, int len, const int16_t *coefs, uint32_t n_blocks, int source, int pixel_type, int scale, int n_rects,
                                const int32_t *rects, const int32_t *clips, uint8_t *out, uint8_t *twin_out, int32_t *status, int32_t *info);

extern "C" int exactrectsim_call_plan(int n, const int32_t *hdr, uint32_t flags, int with_rects, int32_t *status, int64_t *launches, int cap, int32_t *n_launches,
                                      uint8_t *blob, int64_t blob_cap, int64_t *layout, int64_t *image);

// the plan of one call over every layout, source kind and scale, a rectangle, an RGB-coded and a four-component image and, in the middle, an
// image that is refused; with the colour stage's own lists and with the shared ones; and calls with nothing to launch
static bool call_plans()
{
    // width, height, ncomp, subsample, source, colour model, pixel type, scale, rectangle, surface
    static const int32_t hdr[10][14] = {
        { 517, 11, 1, 0x00, 0, JDA_CS_GRAY, JDA_RGB8888, 1, 0, 0, 0, 0, 517, 11 },  { 165, 11, 3, 0x11, 1, JDA_CS_YCBCR, JDA_RGB8888, 2, 0, 0, 0, 0, 83, 6 },
        { 173, 27, 3, 0x22, 2, JDA_CS_YCBCR, JDA_RGB8888, 1, 0, 0, 0, 0, 173, 27 }, { 269, 11, 3, 0x21, 0, JDA_CS_YCBCR, JDA_RGB8888, 8, 0, 0, 0, 0, 34, 2 },
        { 173, 27, 3, 0x22, 2, JDA_CS_YCBCR, JDA_RGB8888, 3, 0, 0, 0, 0, 173, 27 }, { 133, 27, 3, 0x12, 2, JDA_CS_YCBCR, JDA_RGB8888, 1, 0, 0, 0, 0, 133, 27 },
        { 173, 27, 3, 0x22, 0, JDA_CS_YCBCR, JDA_RGB8888, 1, 21, 3, 97, 20, 97, 20 }, { 165, 11, 3, 0x11, 1, JDA_CS_RGB, JDA_RGB8888, 2, 0, 0, 0, 0, 83, 6 },
        { 165, 11, 4, 0x11, 0, JDA_CS_CMYK, JDA_RGB8888, 1, 0, 0, 0, 0, 165, 11 },  { 173, 27, 3, 0x22, 1, JDA_CS_YCBCR, JDA_EIGHT_BIT_GRAYSCALE, 1, 0, 0, 0, 0, 173, 27 } };
    std::vector<uint8_t> blob(1 << 16);
    int64_t launches[64 * 5], layout[10], image[10 * 10];
    int32_t status[10], nl = -1;
    for (int own = 1; own >= 0; own--) {
        for (int i = 0; i < 10; i++) status[i] = 99;
        if (exactrectsim_call_plan(10, &hdr[0][0], own ? JDA_EXACT_COLOUR_MODELS : 0u, own, status, launches, 64, &nl, blob.data(), (int64_t)blob.size(), layout, image) != JDA_SUCCESS) return false;
        // (without the flag the RGB-coded file is read as YCbCr and the four-component one refused)
        for (int i = 0; i < 10; i++) if (status[i] != (i == 4 ? JDA_INVALID_PARAMETER : i == 8 && !own ? JDA_UNSUPPORTED_FEATURE : JDA_SUCCESS)) return false;
        if (nl != (own ? 16 : 12) || layout[6] != (own ? 8 : 7) || layout[8] != (own ? 9 : 8)) return false;      // launches, the first colour launch, images planned
        for (int k = 0; k < nl; k++)
            if (launches[5 * k + 3] + 16 * launches[5 * k + 4] > layout[0] || (launches[5 * k + 3] & 15)) return false;
    }
    if (exactrectsim_call_plan(0, NULL, 0u, 0, status, launches, 64, &nl, blob.data(), (int64_t)blob.size(), layout, image) != JDA_SUCCESS || nl != 0) return false;
    if (exactrectsim_call_plan(1, &hdr[4][0], 0u, 1, status, launches, 64, &nl, blob.data(), (int64_t)blob.size(), layout, image) != JDA_SUCCESS || nl != 0 || layout[0] != 0 ||
        status[0] != JDA_INVALID_PARAMETER) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: exact_rect_asan file.jpg ..\n"); return 2; }
    if (!call_plans()) { fprintf(stderr, "the plan of a call\n"); return 1; }
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint8_t> jpeg;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) jpeg.insert(jpeg.end(), buf, buf + n);
        fclose(f);
        jda_image_info I;
        if (jda_parse(jpeg.data(), (int32_t)jpeg.size(), &I) != JDA_SUCCESS) { fprintf(stderr, "%s: not parsed\n", argv[a]); return 1; }
        for (int scale = 1; scale <= 8; scale *= 2) {
            const int ow = (I.width + scale - 1) / scale, oh = (I.height + scale - 1) / scale;
            int32_t mcu[4];
            const int32_t outside[4] = { ow - 1, 0, 2, 1 }, empty[4] = { 0, 0, 0, 1 }, neg[4] = { -1, 0, 1, 1 };
            if (exactrectsim_plan(I.width, I.height, I.ncomp, I.subsample, JDA_RGB8888, scale, outside, mcu) != JDA_INVALID_PARAMETER ||
                exactrectsim_plan(I.width, I.height, I.ncomp, I.subsample, JDA_RGB8888, scale, empty, mcu) != JDA_INVALID_PARAMETER ||
                exactrectsim_plan(I.width, I.height, I.ncomp, I.subsample, JDA_RGB8888, scale, neg, mcu) != JDA_INVALID_PARAMETER) { fprintf(stderr, "%s: refusals\n", argv[a]); return 1; }
            std::vector<int32_t> rects = { 0, 0, ow, oh }, clips = { ow, oh };
            for (int x = 0; x < 9 && x < ow; x++)
                for (int y = 0; y < 3 && y < oh; y++) {
                    const int w = 1 + (x * 5 + y * 3) % 19, h = 1 + (x + 2 * y) % 6;
                    if (x + w > ow || y + h > oh) continue;
                    rects.insert(rects.end(), { x, y, w, h }); clips.insert(clips.end(), { w - (x % 3 == 2 ? 1 : 0), h + 1 });
                }
            for (int n = 1; n <= 9 && n <= ow && n <= oh; n++) { rects.insert(rects.end(), { ow - n, oh - 1 - (n < oh ? n % 2 : 0), n, 1 }); clips.insert(clips.end(), { n, 1 }); }
            rects.insert(rects.end(), { ow / 2, 0, 1, oh }); clips.insert(clips.end(), { 1, oh });
            rects.insert(rects.end(), { 0, oh / 2, ow, 1 }); clips.insert(clips.end(), { ow - 1, 1 });
            const int n = (int)rects.size() / 4;
            for (int source = (I.jpeg_type == 1 ? 0 : 2); source <= (I.jpeg_type == 1 ? 1 : 2); source++)
                for (int pt = JDA_RGB8888; pt <= JDA_EIGHT_BIT_GRAYSCALE; pt++) {
                    const int bpp = pt == JDA_RGB8888 ? 4 : 1;
                    size_t total = 0;
                    for (int k = 0; k < n; k++) total += (size_t)rects[4 * k + 2] * bpp * rects[4 * k + 3];
                    std::vector<uint8_t> out(total + 1, 0x77);
                    std::vector<int32_t> status((size_t)n, 99);
                    int32_t info[2];
                    const int rc = exactrectsim_run(jpeg.data(), (int)jpeg.size(), NULL, 0, source, pt, scale, n, rects.data(), clips.data(), out.data(), NULL, status.data(), info);
                    bool ok = rc == 0 && info[0] > 0 && info[1] > 0;
                    size_t at = (size_t)ow * bpp * oh;                                      // rectangle 0 is the whole image
                    for (int k = 1; ok && k < n; k++) {
                        const int x = rects[4 * k], y = rects[4 * k + 1], cw = clips[2 * k] < rects[4 * k + 2] ? clips[2 * k] : rects[4 * k + 2];
                        const int ch = clips[2 * k + 1] < rects[4 * k + 3] ? clips[2 * k + 1] : rects[4 * k + 3];
                        for (int r = 0; ok && r < ch; r++, at += (size_t)cw * bpp)
                            ok = memcmp(out.data() + at, out.data() + ((size_t)(y + r) * ow + x) * bpp, (size_t)cw * bpp) == 0;
                    }
                    for (int k = 0; k < n; k++) ok = ok && status[(size_t)k] == 0;
                    ok = ok && out[total] == 0x77;
                    if (!ok) { fprintf(stderr, "%s: scale %d source %d pixel type %d: rc %d\n", argv[a], scale, source, pt, rc); return 1; }
                }
        }
    }
    printf("exact_rect_asan ok\n");
    return 0;
}
