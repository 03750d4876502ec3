// tests/class_cpu/stub_coef.cpp -- TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// The CPU stand-in of the device calls behind decode(JPEG_PROGRESSIVE_FULL): "device" memory is host memory, a resident coefficient
// image is a copy of the host one, and jda_coef_decode_surfaces is the row-major twin of the jda_coef_tiles kernel
// (tests/hostsim/coef_twin.h: the kernel's own arithmetic, none of its schedule).  The scans are decoded by the real host code
// (jda_progressive.cpp), so the class's CPU build runs the whole option from the file to the draw callbacks without a GPU.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jpegdec_amd.h"
#include "../hostsim/coef_twin.h"
#include "../../jpegdec_amd/csrc/jda_plan.h"

struct jda_ctx { int device; };
struct jda_dev_coef {
    jda_image_info info;
    uint8_t q_id[3];
    std::vector<int16_t> quant, coefs;
};

extern "C" {

void *jda_malloc(jda_ctx *ctx, size_t bytes) { void *p = NULL; return (ctx && posix_memalign(&p, 64, bytes ? bytes : 64) == 0) ? p : NULL; }
void jda_free(jda_ctx *, void *p) { free(p); }
int jda_copy_to_host(jda_ctx *ctx, void *host, const void *dptr, size_t bytes) { if (!ctx) return JDA_ERROR_NO_DEVICE; memcpy(host, dptr, bytes); return JDA_SUCCESS; }

jda_dev_coef *jda_coef_upload(jda_ctx *ctx, const jda_coef_image *img, int32_t *err)
{
    int32_t dummy;
    if (!err) err = &dummy;
    if (!ctx) { *err = JDA_ERROR_NO_DEVICE; return NULL; }
    if (!img) { *err = JDA_INVALID_PARAMETER; return NULL; }
    jda_dev_coef *d = new jda_dev_coef;
    d->info = *jda_coef_image_get_info(img);
    uint32_t n = 0;
    const int16_t *c = jda_coef_image_coefficients(img, &n);
    const int16_t *q = jda_coef_image_quant(img, d->q_id);
    d->coefs.assign(c, c + (size_t)n * 64);
    d->quant.assign(q, q + 256);
    *err = JDA_SUCCESS;
    return d;
}
void jda_dev_coef_free(jda_ctx *, jda_dev_coef *d) { delete d; }

int jda_coef_decode_surfaces(jda_ctx *ctx, int32_t n, const jda_dev_coef *const *imgs, const jda_output *outputs, const int32_t *pixel_types, const int32_t *options)
{
    if (!ctx) return JDA_ERROR_NO_DEVICE;
    if (n < 0 || (n > 0 && (!imgs || !outputs))) return JDA_INVALID_PARAMETER;
    for (int i = 0; i < n; i++) {
        const jda_dev_coef *d = imgs[i];
        if (!d) return JDA_INVALID_PARAMETER;
        jda_image_info I = d->info;
        I.jpeg_type = 0;
        const int opt = (options ? options[i] : 0) & ~JDA_PROGRESSIVE_FULL;
        int pt = pixel_types ? pixel_types[i] : JDA_RGB8888;
        if (pt < 0 || pt > JDA_EIGHT_BIT_GRAYSCALE) return JDA_INVALID_PARAMETER;
        if (opt & (JDA_SCALE_HALF | JDA_SCALE_QUARTER | JDA_SCALE_EIGHTH)) return JDA_UNSUPPORTED_FEATURE;
        if ((opt & JDA_LUMA_ONLY) && pt < JDA_EIGHT_BIT_GRAYSCALE) pt = JDA_EIGHT_BIT_GRAYSCALE;
        int bpp, ow, oh, cw, ch;
        const int rc = jda_output_geometry(&I, pt, opt, &bpp, &ow, &oh, &cw, &ch);
        if (rc != JDA_SUCCESS) return rc;
        const jda_output &O = outputs[i];
        const int mode = jda_mode_of(I);
        if (mode == JDA_MODE_GRAY && pt == JDA_RGB8888) pt = JDA_RGB565_BIG_ENDIAN;
        const uint32_t w = (uint32_t)(O.width_px < cw ? O.width_px : cw), rows = (uint32_t)(O.rows < ch ? O.rows : ch);
        if (!O.pixels || O.pitch_bytes < (int)w * bpp) return JDA_INVALID_PARAMETER;
        if (coef_twin_decode(mode, (uint32_t)I.mcus_x, (uint32_t)I.mcus_y, d->q_id, d->quant.data(), d->coefs.data(), pt, (uint8_t *)O.pixels, (uint32_t)O.pitch_bytes, w, rows) != 0)
            return JDA_INVALID_PARAMETER;
    }
    return JDA_SUCCESS;
}

} // extern "C"
