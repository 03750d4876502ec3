/* A plain C program on the C flavour of the API decoding with a caller-chosen option word (JPEG_PROGRESSIVE_FULL among them) --
 * tests/test_gpu_progressive_full.py.  Usage:
 *     prog_user file.jpg pixel_type options framebuffer(0|1) canvas_w canvas_h bytes_per_pixel max_mcus out.bin log.txt
 * Callback mode: the strips are assembled into a canvas_w x canvas_h canvas (pixels of bytes_per_pixel bytes) written to out.bin, and
 * every JPEGDRAW goes to log.txt as "x y iWidth iHeight iWidthUsed iBpp".  Framebuffer mode: a buffer of that size, filled with 0x5a,
 * is the framebuffer and is written as it stands.  Exit code: 0, or getLastError() (102: failure without a code). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "JPEGDEC.h"

static uint8_t *g_canvas;
static int g_w, g_h, g_bpp;
static FILE *g_log;

static int draw(JPEGDRAW *d)
{
    fprintf(g_log, "%d %d %d %d %d %d\n", d->x, d->y, d->iWidth, d->iHeight, d->iWidthUsed, d->iBpp);
    for (int r = 0; r < d->iHeight; r++) {
        int y = d->y + r, n = d->iWidth;
        if (y >= g_h) break;
        if (d->x + n > g_w) n = g_w - d->x;
        if (n > 0) memcpy(g_canvas + ((size_t)y * g_w + d->x) * g_bpp, (uint8_t *)d->pPixels + (size_t)r * d->iWidth * g_bpp, (size_t)n * g_bpp);
    }
    return 1;
}

int main(int argc, char **argv)
{
    JPEGIMAGE jpg;
    if (argc < 11) return 100;
    const int pt = atoi(argv[2]), options = atoi(argv[3]), fb = atoi(argv[4]), max_mcus = atoi(argv[8]);
    g_w = atoi(argv[5]); g_h = atoi(argv[6]); g_bpp = atoi(argv[7]);
    if (!JPEG_openFile(&jpg, argv[1], draw)) return 101;
    g_canvas = (uint8_t *)malloc((size_t)g_w * g_h * g_bpp + 64);
    memset(g_canvas, fb ? 0x5a : 0, (size_t)g_w * g_h * g_bpp + 64);
    g_log = fopen(argv[10], "w");
    if (!g_canvas || !g_log) return 103;
    JPEG_setPixelType(&jpg, pt);
    if (max_mcus > 0) JPEG_setMaxOutputSize(&jpg, max_mcus);
    if (fb) JPEG_setFramebuffer(&jpg, g_canvas);
    const int ok = JPEG_decode(&jpg, 0, 0, options);
    const int err = JPEG_getLastError(&jpg);
    fclose(g_log);
    FILE *f = fopen(argv[9], "wb");
    if (!f) return 103;
    fwrite(g_canvas, 1, (size_t)g_w * g_h * g_bpp, f);
    fclose(f);
    JPEG_close(&jpg);
    free(g_canvas);
    return ok ? 0 : (err ? err : 102);
}
