// tests/hostsim/recode_xf_main.cpp -- TEST INFRASTRUCTURE: recode_xf_sim.cpp's entry point as a program of its own, built with
// -fsanitize=address,undefined (make recodexfasan): the plan of jda_recode_images_ex and every lane of its two transforming stages over the
// files named on the command line (fixtures of tests/golden: baseline files of every layout and progressive ones), each under every
// operation with JDA_XF_TRIM to every form, then cropped to its second MCU column and row on, then all of them in one baseline call with a
// different operation each.  A job may be refused (a 4:2:2 file transposed, a one-MCU axis trimmed away); nothing else may go wrong.
// Prints "recode_xf_asan ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"

extern "C" int recodexfsim_files(int n, const uint8_t *const *jpegs, const int32_t *lens, const int32_t *form, const int32_t *ri, const int32_t *sparse,
                                 const jda_recode_xform *xforms, void *const *dst, const int64_t *cap, int64_t *dst_bytes, int32_t *status, int16_t *coef, uint32_t *meta,
                                 uint32_t *bad, uint8_t *hdr, int64_t hdr_cap, int64_t *hdr_len, uint64_t *info);

int main(int argc, char **argv)
{
    std::vector<std::vector<uint8_t>> files;
    for (int i = 1; i < argc; i++) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) { printf("cannot open %s\n", argv[i]); return 2; }
        std::vector<uint8_t> b;
        uint8_t chunk[4096];
        for (size_t k; (k = fread(chunk, 1, sizeof(chunk), f)) > 0;) b.insert(b.end(), chunk, chunk + k);
        fclose(f);
        files.push_back(b);
    }
    if (files.empty()) { printf("no files\n"); return 2; }
    const size_t n = files.size();
    const int64_t cap1 = 1 << 20;
    std::vector<uint8_t> out(n * (size_t)cap1);
    std::vector<const uint8_t *> ptr(n);
    std::vector<int32_t> len(n), form(n), ri(n), status(n);
    std::vector<void *> dst(n);
    std::vector<int64_t> cap(n, cap1), nbytes(n);
    std::vector<uint32_t> bad(n);
    std::vector<jda_recode_xform> xf(n);
    uint64_t info[6];
    int64_t hdr_len = 0;
    for (size_t i = 0; i < n; i++) { ptr[i] = files[i].data(); len[i] = (int32_t)files[i].size(); dst[i] = out.data() + i * (size_t)cap1; }
    int runs = 0, written = 0;
    for (size_t i = 0; i < n; i++) {
        jda_image_info I;
        if (jda_parse(ptr[i], len[i], &I) != JDA_SUCCESS) { printf("%s: not parsed\n", argv[1 + i]); return 1; }
        for (int crop = 0; crop < 2; crop++) {
            if (crop && (I.mcus_x < 2 || I.mcus_y < 2)) continue;
            for (int op = JDA_XF_NONE; op <= JDA_XF_EXIF; op++)
                for (int f = 0; f < 3; f++) {
                    const int32_t fo = f, rr = f == 1 ? 2 : -1 + f / 2;
                    jda_recode_xform X = { op, JDA_XF_TRIM, { 0, 0, 0, 0 } };
                    if (crop) { X.mcu_rect[0] = 1; X.mcu_rect[1] = 1; X.mcu_rect[2] = I.mcus_x - 1; X.mcu_rect[3] = I.mcus_y - 1; }
                    const int rc = recodexfsim_files(1, &ptr[i], &len[i], &fo, &rr, NULL, &X, &dst[i], &cap[i], &nbytes[i], &status[i], NULL, NULL, &bad[i], NULL, 0, &hdr_len, info);
                    if (rc != 0 || (status[i] != JDA_SUCCESS && status[i] != JDA_UNSUPPORTED_FEATURE)) { printf("%s op %d form %d crop %d: rc %d status %d\n", argv[1 + i], op, f, crop, rc, status[i]); return 1; }
                    runs++;
                    if (status[i] == JDA_SUCCESS && (nbytes[i] < 4 || ((uint8_t *)dst[i])[0] != 0xff || ((uint8_t *)dst[i])[nbytes[i] - 1] != 0xd9)) { printf("%s op %d form %d: no file\n", argv[1 + i], op, f); return 1; }
                    written += status[i] == JDA_SUCCESS;
                }
        }
    }
    for (size_t i = 0; i < n; i++) { form[i] = 0; ri[i] = -1; const jda_recode_xform X = { (int32_t)(i % 8), JDA_XF_TRIM, { 0, 0, 0, 0 } }; xf[i] = X; }
    const int rc = recodexfsim_files((int)n, ptr.data(), len.data(), form.data(), ri.data(), NULL, xf.data(), dst.data(), cap.data(), nbytes.data(), status.data(), NULL, NULL,
                                     bad.data(), NULL, 0, &hdr_len, info);
    if (rc != 0) { printf("the call over all files: rc %d\n", rc); return 1; }
    for (size_t i = 0; i < n; i++) if (status[i] == JDA_SUCCESS && (nbytes[i] < 4 || out[i * (size_t)cap1] != 0xff || out[i * (size_t)cap1 + (size_t)nbytes[i] - 1] != 0xd9)) { printf("file %zu\n", i); return 1; }
    printf("recode_xf_asan ok: %d calls, %d files written, %llu blocks in the last\n", runs + 1, written, (unsigned long long)info[0]);
    return 0;
}
