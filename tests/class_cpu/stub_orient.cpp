// tests/class_cpu/stub_orient.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// The CPU stand-in for jda_decode_to_host_oriented, beside stub_runtime.cpp's stand-ins for the other device entry points the drop-in
// class calls: the oracle's canvas (zeros from a bad MCU on, as the device leaves it), its visible rectangle turned by the row-major
// twin of the kernel (tests/hostsim/orient_twin.h).  It lets JPEGDEC::decode's JPEG_AUTO_ROTATE path -- refusals, the strip sequence,
// what reaches the caller's buffer -- run without a GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"
#include "../hostsim/orient_twin.h"

extern "C" int jda_decode_to_host_oriented(jda_ctx *ctx, const uint8_t *jpeg, int32_t len, int32_t pixel_type, int32_t options, int32_t orientation,
                                           void *host_pixels, int32_t pitch_bytes, int32_t rows, int32_t *mcus_decoded)
{
    if (mcus_decoded) *mcus_decoded = 0;
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (!jpeg || !host_pixels || orientation > 8 || pixel_type < 0 || pixel_type > JDA_EIGHT_BIT_GRAYSCALE) return JDA_INVALID_PARAMETER;
    jda_image_info I;
    int rc = jda_parse(jpeg, len, &I);
    if (rc != JDA_SUCCESS) return rc;
    int bpp, ow, oh, cw, ch, tw = 0, th = 0;
    rc = jda_output_geometry(&I, pixel_type, options, &bpp, &ow, &oh, &cw, &ch);
    if (rc == JDA_SUCCESS) rc = jda_oriented_geometry(&I, pixel_type, options, orientation, NULL, &tw, &th, NULL);
    if (rc != JDA_SUCCESS) return rc;
    if (pitch_bytes < tw * bpp || rows < th) return JDA_INVALID_PARAMETER;
    std::vector<uint8_t> canvas((size_t)cw * bpp * ch, 0), turned((size_t)tw * bpp * th, 0);
    rc = jda_decode_to_host_ex(ctx, jpeg, len, pixel_type, options, canvas.data(), cw * bpp, ch, mcus_decoded);      // (the stand-in of stub_runtime.cpp)
    if (rc != JDA_SUCCESS && rc != JDA_DECODE_ERROR) return rc;
    if (orient_twin_rowmajor(canvas.data(), cw * bpp, ow, oh, bpp, orientation < 0 ? I.orientation : orientation, turned.data(), tw * bpp) != 0) return JDA_INVALID_PARAMETER;
    for (int r = 0; r < th; r++) memcpy((uint8_t *)host_pixels + (size_t)r * pitch_bytes, &turned[(size_t)r * tw * bpp], (size_t)tw * bpp);
    return rc;
}
