// tests/class_cpu/stub_dither.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// The CPU stand-in for jda_decode_dither_to_host, beside stub_runtime.cpp's stand-ins for the other device entry points the drop-in
// class calls: the oracle's GRAY8 canvas, dithered by the row-major twin of the kernel (tests/hostsim/dither_twin.h).  It lets
// JPEGDEC::decodeDither's host logic -- refusals, the draw sequence, what reaches the caller's buffer -- run without a GPU against
// what the unmodified reference recorded (tests/golden/dither).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"
#include "../hostsim/dither_twin.h"

extern "C" int jda_decode_dither_to_host(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options,
                                         const uint8_t *seed, void *host_packed, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded)
{
    if (mcus_decoded) *mcus_decoded = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    int32_t bits = 0, dpitch = 0;
    jda_image_info I;
    int rc = jda_parse(jpeg, len, &I);
    if (rc != JDA_SUCCESS) return rc;
    int bpp, ow, oh, cw, ch;
    rc = jda_output_geometry(&I, JDA_EIGHT_BIT_GRAYSCALE, options, &bpp, &ow, &oh, &cw, &ch);
    if (rc == JDA_SUCCESS) rc = jda_dither_geometry(cw, ch, pixel_type, &bits, &dpitch, NULL);
    if (rc != JDA_SUCCESS) return rc;
    if (!host_packed || pitch_bytes < dpitch || I.mcus_y <= 0) return JDA_INVALID_PARAMETER;
    std::vector<uint8_t> gray((size_t)cw * ch, 0), packed((size_t)dpitch * ch, 0);
    rc = jda_decode_to_host_ex(ctx, jpeg, len, JDA_EIGHT_BIT_GRAYSCALE, options, gray.data(), cw, ch, mcus_decoded);      // (the stand-in of stub_runtime.cpp)
    if (rc != JDA_SUCCESS && rc != JDA_DECODE_ERROR) return rc;
    uint8_t own[JDA_DITHER_SEED_BYTES];
    if (!seed) { (void)jda_dither_seed(jpeg, len, 0, own); seed = own; }
    if (dither_twin_rowmajor(gray.data(), cw, cw, ch, ch / I.mcus_y, bits, seed, packed.data(), dpitch) != 0) return JDA_INVALID_PARAMETER;
    for (int r = 0; r < ch && r < rows; r++) memcpy((uint8_t *)host_packed + (size_t)r * pitch_bytes, &packed[(size_t)r * dpitch], (size_t)dpitch);
    return rc;
}
