// jda_progressive.cpp -- every scan of a progressive (SOF2) file decoded on the host into coefficient planes (ITU-T T.81 Annex G),
// and the coefficient image that carries them -- or a caller's own coefficients -- to the GPU (jda_coef_upload, jda_coef_tiles).
//
// The reference decodes the first (DC) scan of such a file and nothing else (jpeg.inl:4964-4966); this is the opt-in extension
// behind JDA_PROGRESSIVE_FULL.  Geometry, component ids and the prescaled quantisers come from the same header
// walk as everything else (jda_parse); the segments are walked here: DHT and DQT segments in front of and between the scans are
// honoured -- Huffman tables are those in force at each SOS (ids 0-3 of either class: canonical codes, none of the reference's LUT
// shapes), and a component's quantiser is latched, and prescaled, at the first scan that names the component (as libjpeg does: a
// table defined or redefined behind that scan no longer reaches it).  jda_coef_image_from_coefficients, which serves baseline files
// too, takes the header's quantisers as the baseline path builds them (jda_front_prepare).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>

#include "jda_internal.h"

extern "C" int jda_front_prepare(const uint8_t *jpeg, int32_t len, uint8_t *tables, jda_front *out);
extern "C" void jda_front_prescale_quant(const uint16_t *zz, int convert, int16_t *out);
extern "C" int jda_parse_coef(const uint8_t *jpeg, int32_t len, jda_image_info *info, int32_t *comp_hv, int32_t *colour, int32_t *adobe);

struct jda_coef_image {
    jda_image_info info;
    uint8_t q_id[3];
    uint8_t raw_qid[3], adobe;               // the frame header's table id of component c; the file has an Adobe APP14 segment
    uint8_t colour;                          // JDA_CS_*: how libjpeg reads the components (jda_colour_model)
    uint16_t raw_quant[3][64];               // component c's DQT entries as the file lists them (zigzag order): a recode writes them back
    alignas(16) int16_t quant[4 * 64];      // prescaled (JPEGFixQuantD, jpeg.inl:1789-1811), natural order: JDA_TB_QUANT of the table blob
    int16_t *coefs;                          // n_blocks x int16[64], natural order, MCU-interleaved scan order; 16-byte aligned
    uint32_t n_blocks;
    // the sparse form (jda_coef_image_sparse): made on first request, kept; coefs is constant once the image is handed out
    std::once_flag sparse_once;
    uint32_t *sp_first, *sp_entries;        // first[n_blocks + 1] and entries[n_entries], each padded with zeros to 16 bytes
    uint32_t sp_n_entries;
    int sp_status;                           // JDA_SUCCESS / JDA_UNSUPPORTED_FEATURE (2^31 entries and more) / JDA_ERROR_MEMORY
    // a four-component file (jda_coef_prepare): info.ncomp is 4, everything above is components 0..2 stored exactly as a
    // three-component image of their layout (blocks_per_mcu and n_blocks count those), and component 3 is this gray coefficient image over
    // its own MCU-padded block grid, row-major, owned by this one.  NULL in every other image.
    jda_coef_image *k;
};

namespace {

const uint8_t kZigZag[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

// a canonical Huffman code (T.81 F.2.2.3): the codes of length l are mincode[l] .. maxcode[l], their symbols from valptr[l] on
struct Huff {
    bool defined;
    int32_t maxcode[18], mincode[17], valptr[17];
    uint8_t symbols[256];
    int total;
};

bool huff_build(Huff &h, const uint8_t *counts, const uint8_t *symbols, int total)
{
    int32_t code = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        h.valptr[l] = k; h.mincode[l] = code;
        code += counts[l - 1]; k += counts[l - 1];
        if (code > (1 << l)) return false;             // over-subscribed
        h.maxcode[l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    memcpy(h.symbols, symbols, (size_t)total);
    h.total = total; h.defined = true;
    return true;
}

// the entropy-coded segment of one scan: byte stuffing removed as it is read; a marker ends the data (zero bits behind it, as
// every decoder feeds them), RSTn markers are stepped over by restart()
struct Bits {
    const uint8_t *d;
    int len, pos;
    uint32_t acc;
    int n;
    bool fill()
    {
        while (n <= 24) {
            uint32_t b = 0;
            if (pos < len) {
                b = d[pos];
                if (b == 0xff) {
                    if (pos + 1 < len && d[pos + 1] == 0) pos += 2;
                    else b = 0;                        // a marker (or the file's last byte): stay in front of it
                } else pos++;
            }
            acc |= b << (24 - n);
            n += 8;
        }
        return true;
    }
    uint32_t peek(int k) { if (n < k) fill(); return acc >> (32 - k); }
    void drop(int k) { acc <<= k; n -= k; }
    uint32_t get(int k) { if (k == 0) return 0; const uint32_t v = peek(k); drop(k); return v; }
    // byte-align and step over the RSTn marker that follows (fill bytes and stray data in front of it are skipped)
    void restart()
    {
        acc = 0; n = 0;
        while (pos + 1 < len) {
            if (d[pos] == 0xff && d[pos + 1] >= 0xd0 && d[pos + 1] <= 0xd7) { pos += 2; return; }
            if (d[pos] == 0xff && d[pos + 1] != 0 && d[pos + 1] != 0xff) return;       // another marker: the scan ends here
            pos++;
        }
    }
};

inline int decode_symbol(Bits &B, const Huff &h)
{
    uint32_t w = B.peek(16);
    int32_t code = 0;
    for (int l = 1; l <= 16; l++) {
        code = (int32_t)(w >> (16 - l));
        if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) {
            const int i = h.valptr[l] + code - h.mincode[l];
            if (i >= h.total) return -1;
            B.drop(l);
            return h.symbols[i];
        }
    }
    return -1;                                         // no code of the table starts like this
}

inline int32_t extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v; }

// rm: the component's blocks lie row-major from there, rm_w a row (component 3 of a four-component image), else in the MCUs of coefs
struct Comp { int id, h, v, blocks_w, blocks_h, mcu_off; int16_t *rm; int rm_w; };

struct Decoder {
    const uint8_t *d;
    int len;
    jda_image_info I;
    Comp comp[4];
    int hmax, vmax;
    bool sequential;                         // SOF0 / SOF1: every scan codes whole blocks (T.81 F.2.2), else Annex G
    Huff dc[4], ac[4];
    int restart_interval;
    int16_t *coefs;
    // quantisers: the DQT contents in force (zigzag order), and per component the table id of the frame header and whether its
    // table has been latched into quant_out[64 c ..] (the coefficient image's table c: q_id = {0, 1, 2})
    uint16_t quant_zz[4][64];
    bool quant_defined[4], latched[4];
    int tq[4];
    int16_t *quant_out[4];                   // per component: where its prescaled table and its DQT entries go
    uint16_t *raw_out[4];

    bool read_dqt(int at, int seglen)
    {
        int q = at + 2, end = at + seglen;
        if (end > len) return false;
        while (q < end) {
            const int pq = d[q] >> 4, t = d[q] & 15;
            if (t > 3 || pq > 1 || q + 1 + (pq ? 128 : 64) > end) return false;
            for (int i = 0; i < 64; i++) quant_zz[t][i] = pq ? (uint16_t)((d[q + 1 + 2 * i] << 8) | d[q + 2 + 2 * i]) : d[q + 1 + i];
            quant_defined[t] = true;
            q += 1 + (pq ? 128 : 64);
        }
        return true;
    }
    bool latch(int c)
    {
        if (latched[c]) return true;
        if (!quant_defined[tq[c]]) return false;
        jda_front_prescale_quant(quant_zz[tq[c]], tq[c] < I.ncomp, quant_out[c]);      // (the conversion rule of the baseline path)
        memcpy(raw_out[c], quant_zz[tq[c]], sizeof(quant_zz[0]));
        latched[c] = true;
        return true;
    }

    int16_t *block(const Comp &c, int bx, int by) const
    {
        if (c.rm) return c.rm + ((size_t)by * (size_t)c.rm_w + (size_t)bx) * 64;
        const int mcu = (by / c.v) * I.mcus_x + bx / c.h;
        const int within = (by % c.v) * c.h + bx % c.h;
        return coefs + ((size_t)mcu * I.blocks_per_mcu + c.mcu_off + within) * 64;
    }

    bool read_dht(int at, int seglen)
    {
        int q = at + 2, end = at + seglen;
        if (end > len) return false;
        while (q < end) {
            if (q + 17 > end) return false;
            const int tc = d[q] >> 4, th = d[q] & 15;
            if (tc > 1 || th > 3) return false;
            int total = 0;
            for (int i = 0; i < 16; i++) total += d[q + 1 + i];
            if (total > 256 || q + 17 + total > end) return false;
            if (!huff_build(tc ? ac[th] : dc[th], d + q + 1, d + q + 17, total)) return false;
            q += 17 + total;
        }
        return true;
    }

    // one scan; *pos_io: in = the first entropy-coded byte, out = where the reader stopped
    int scan(int ns, const int *ci, const int *td, const int *ta, int Ss, int Se, int Ah, int Al, int *pos_io)
    {
        Bits B;
        B.d = d; B.len = len; B.pos = *pos_io; B.acc = 0; B.n = 0;
        int32_t pred[4] = { 0, 0, 0, 0 };
        uint32_t eobrun = 0;
        int until_restart = restart_interval;
        const bool interleaved = ns > 1;
        const Comp &c0 = comp[ci[0]];
        const int units_x = interleaved ? I.mcus_x : c0.blocks_w, units_y = interleaved ? I.mcus_y : c0.blocks_h;
        const int16_t p1 = (int16_t)(1 << Al), m1 = (int16_t)(-(1 << Al));
        for (int uy = 0; uy < units_y; uy++)
            for (int ux = 0; ux < units_x; ux++) {
                if (restart_interval && until_restart == 0) {
                    B.restart();
                    pred[0] = pred[1] = pred[2] = pred[3] = 0; eobrun = 0;
                    until_restart = restart_interval;
                }
                until_restart--;
                for (int k = 0; k < ns; k++) {
                    const Comp &c = comp[ci[k]];
                    const int nh = interleaved ? c.h : 1, nv = interleaved ? c.v : 1;
                    for (int by = 0; by < nv; by++)
                        for (int bx = 0; bx < nh; bx++) {
                            int16_t *blk = interleaved ? block(c, ux * c.h + bx, uy * c.v + by) : block(c, ux, uy);
                            if (sequential) {                                    // a whole block (F.2.2.1, F.2.2.2)
                                const int t = decode_symbol(B, dc[td[k]]);
                                if (t < 0 || t > 16) return JDA_DECODE_ERROR;
                                if (t) pred[ci[k]] += extend(B.get(t), t);
                                blk[0] = (int16_t)(uint16_t)(uint32_t)pred[ci[k]];
                                for (int z = 1; z <= 63; z++) {
                                    const int rs = decode_symbol(B, ac[ta[k]]);
                                    if (rs < 0) return JDA_DECODE_ERROR;
                                    const int r = rs >> 4, s = rs & 15;
                                    if (s) {
                                        z += r;
                                        if (z > 63) return JDA_DECODE_ERROR;
                                        blk[kZigZag[z]] = (int16_t)(uint16_t)(uint32_t)extend(B.get(s), s);
                                    } else if (r == 15) z += 15;
                                    else break;
                                }
                                continue;
                            }
                            if (Ss == 0) {
                                if (Ah == 0) {                                   // DC, first pass (G.1.2.1)
                                    const int s = decode_symbol(B, dc[td[k]]);
                                    if (s < 0 || s > 16) return JDA_DECODE_ERROR;
                                    if (s) pred[ci[k]] += extend(B.get(s), s);
                                    blk[0] = (int16_t)(uint16_t)((uint32_t)pred[ci[k]] << Al);
                                } else if (B.get(1)) blk[0] = (int16_t)(blk[0] | p1);   // DC refinement (G.1.2.1.1)
                            } else if (Ah == 0) {                                // AC, first pass (G.1.2.2)
                                if (eobrun) { eobrun--; continue; }
                                for (int z = Ss; z <= Se; z++) {
                                    const int rs = decode_symbol(B, ac[ta[k]]);
                                    if (rs < 0) return JDA_DECODE_ERROR;
                                    const int r = rs >> 4, s = rs & 15;
                                    if (s) {
                                        z += r;
                                        if (z > Se) return JDA_DECODE_ERROR;
                                        blk[kZigZag[z]] = (int16_t)(uint16_t)((uint32_t)extend(B.get(s), s) << Al);
                                    } else if (r == 15) z += 15;
                                    else { eobrun = (1u << r) + B.get(r) - 1u; break; }
                                }
                            } else {                                             // AC refinement (G.1.2.3)
                                int z = Ss;
                                if (eobrun == 0) {
                                    for (; z <= Se; z++) {
                                        const int rs = decode_symbol(B, ac[ta[k]]);
                                        if (rs < 0) return JDA_DECODE_ERROR;
                                        int r = rs >> 4;
                                        int16_t val = 0;
                                        if (rs & 15) {
                                            if ((rs & 15) != 1) return JDA_DECODE_ERROR;
                                            val = B.get(1) ? p1 : m1;
                                        } else if (r != 15) { eobrun = (1u << r) + B.get(r); break; }
                                        // correction bits of the nonzero coefficients passed, until r zero ones have been
                                        for (; z <= Se; z++) {
                                            int16_t &cf = blk[kZigZag[z]];
                                            if (cf != 0) {
                                                if (B.get(1) && !(cf & p1)) cf = (int16_t)(cf + (cf >= 0 ? p1 : m1));
                                            } else if (--r < 0) break;
                                        }
                                        if (val) {
                                            if (z > Se) return JDA_DECODE_ERROR;
                                            blk[kZigZag[z]] = val;
                                        }
                                    }
                                }
                                if (eobrun) {                                    // the rest of the band: correction bits only
                                    for (; z <= Se; z++) {
                                        int16_t &cf = blk[kZigZag[z]];
                                        if (cf != 0 && B.get(1) && !(cf & p1)) cf = (int16_t)(cf + (cf >= 0 ? p1 : m1));
                                    }
                                    eobrun--;
                                }
                            }
                        }
                }
            }
        *pos_io = B.pos;
        return JDA_SUCCESS;
    }

    int run(int first_sos)
    {
        int at = first_sos, scans = 0;                 // at: a marker
        while (at + 4 <= len) {
            if (d[at] != 0xff) { at++; continue; }
            const int m = d[at + 1];
            if (m == 0xff) { at++; continue; }
            if (m == 0xd9) break;                      // EOI
            if (m == 0 || (m >= 0xd0 && m <= 0xd7) || m == 0x01) { at += 2; continue; }
            const int seglen = (d[at + 2] << 8) | d[at + 3];
            if (seglen < 2) return JDA_DECODE_ERROR;
            if (m == 0xc4) { if (!read_dht(at + 2, seglen)) return JDA_DECODE_ERROR; }
            else if (m == 0xdb) { if (!read_dqt(at + 2, seglen)) return JDA_DECODE_ERROR; }
            else if (m == 0xdd) { if (seglen == 4 && at + 6 <= len) restart_interval = (d[at + 4] << 8) | d[at + 5]; }
            else if (m == 0xda) {
                const int q = at + 4;
                if (q >= len) break;
                const int ns = d[q];
                if (ns < 1 || ns > I.ncomp || seglen != 6 + 2 * ns || at + 2 + seglen > len) return JDA_DECODE_ERROR;
                int ci[4], td[4], ta[4];
                for (int k = 0; k < ns; k++) {
                    int j;
                    for (j = 0; j < I.ncomp; j++) if (comp[j].id == d[q + 1 + 2 * k]) break;
                    if (j == I.ncomp) return JDA_DECODE_ERROR;                 // a component the frame does not have
                    for (int e = 0; e < k; e++) if (ci[e] >= j) return JDA_DECODE_ERROR;    // (frame order, each once)
                    ci[k] = j; td[k] = d[q + 2 + 2 * k] >> 4; ta[k] = d[q + 2 + 2 * k] & 15;
                    if (td[k] > 3 || ta[k] > 3) return JDA_DECODE_ERROR;
                }
                const int Ss = d[q + 1 + 2 * ns], Se = d[q + 2 + 2 * ns], Ah = d[q + 3 + 2 * ns] >> 4, Al = d[q + 3 + 2 * ns] & 15;
                // G.1.1.1.1: a DC band is 0..0, an AC band lies in 1..63 and belongs to one component; a refinement moves one bit
                if (sequential) { if (Ss != 0 || Se != 63 || Ah != 0 || Al != 0) return JDA_DECODE_ERROR; }      // (B.2.3: what a sequential scan states)
                else if (Ss > Se || Se > 63 || (Ss == 0 && Se != 0) || (Ss > 0 && ns != 1) || Al > 13 || (Ah != 0 && Al != Ah - 1)) return JDA_DECODE_ERROR;
                for (int k = 0; k < ns; k++) {
                    if (sequential && (!dc[td[k]].defined || !ac[ta[k]].defined)) return JDA_DECODE_ERROR;
                    if (Ss == 0 && Ah == 0 && !dc[td[k]].defined) return JDA_DECODE_ERROR;
                    if (Ss > 0 && !ac[ta[k]].defined) return JDA_DECODE_ERROR;
                    if (!latch(ci[k])) return JDA_DECODE_ERROR;                  // a scan of a component whose quantiser no DQT has defined yet
                }
                int pos = at + 2 + seglen;
                const int rc = scan(ns, ci, td, ta, Ss, Se, Ah, Al, &pos);
                if (rc != JDA_SUCCESS) return rc;
                scans++;
                at = pos;
                while (at + 1 < len && !(d[at] == 0xff && d[at + 1] != 0 && d[at + 1] != 0xff && !(d[at + 1] >= 0xd0 && d[at + 1] <= 0xd7))) at++;
                continue;
            }
            at += 2 + seglen;
        }
        for (int c = 0; c < I.ncomp; c++) (void)latch(c);   // (a component no scan named: its coefficients are zero, its table whatever is there)
        return scans ? JDA_SUCCESS : JDA_DECODE_ERROR;
    }
};

// want_progressive: the header walk alone (jda_parse) -- the scan decoder brings its own Huffman tables and latches the quantisers, so
// none of the baseline path's table restrictions (DC ids 0-1, codes its LUT shapes hold) applies; else the header's tables as the
// baseline path builds them
jda_coef_image *coef_image_new(const uint8_t *jpeg, int32_t len, int want_progressive, int32_t *err)
{
    alignas(16) uint8_t tables[JDA_TABLE_BYTES];
    jda_front F;
    memset(&F, 0, sizeof(F));
    memset(tables, 0, sizeof(tables));
    int rc;
    if (want_progressive) {
        rc = jda_parse(jpeg, len, &F.info);
        const jda_image_info &I = F.info;
        if (rc == JDA_SUCCESS && I.jpeg_type != 1) rc = JDA_INVALID_PARAMETER;
        if (rc == JDA_SUCCESS && !((I.ncomp == 1 || I.ncomp == 3) && I.width > 0 && I.height > 0 && I.mcu_w > 0 &&
                                   (I.subsample == 0x00 || I.subsample == 0x11 || I.subsample == 0x22 || I.subsample == 0x21 || I.subsample == 0x12)))
            rc = JDA_UNSUPPORTED_FEATURE;
        F.q_id[0] = 0; F.q_id[1] = 1; F.q_id[2] = 2;       // table c = component c's, latched by the scan decoder
    } else rc = jda_front_prepare(jpeg, len, tables, &F);
    if (rc != JDA_SUCCESS) { *err = rc; return NULL; }
    jda_coef_image *img = new (std::nothrow) jda_coef_image;
    if (!img) { *err = JDA_ERROR_MEMORY; return NULL; }
    img->info = F.info;
    memcpy(img->q_id, F.q_id, 3);
    memcpy(img->quant, tables + JDA_TB_QUANT, sizeof(img->quant));
    memset(img->raw_quant, 0, sizeof(img->raw_quant));
    for (int c = 0; c < 3; c++) { img->raw_qid[c] = F.raw_q_id[c]; memcpy(img->raw_quant[c], F.quant_zz[F.raw_q_id[c] & 3], sizeof(img->raw_quant[0])); }
    img->adobe = F.adobe;
    if (want_progressive) {                  // (jda_parse hands the header fields alone)
        jda_exact_file E;
        img->colour = jda_exact_probe(jpeg, len, &E) == JDA_SUCCESS && E.colour_model >= 0 ? (uint8_t)E.colour_model : (uint8_t)(F.info.ncomp == 1 ? JDA_CS_GRAY : JDA_CS_YCBCR);
    } else img->colour = F.colour;
    img->n_blocks = (uint32_t)(F.info.mcus_x * F.info.mcus_y * F.info.blocks_per_mcu);
    img->coefs = NULL;
    img->k = NULL;
    img->sp_first = img->sp_entries = NULL; img->sp_n_entries = 0; img->sp_status = JDA_SUCCESS;
    const size_t bytes = ((size_t)img->n_blocks * 128 + 15) & ~(size_t)15;
    if (posix_memalign((void **)&img->coefs, 64, bytes ? bytes : 64) != 0) { delete img; *err = JDA_ERROR_MEMORY; return NULL; }
    memset(img->coefs, 0, bytes);
    *err = JDA_SUCCESS;
    return img;
}

// the sparse form: an entry per nonzero coefficient (DC included), blocks in order, natural index ascending within a block
void sparse_pack(jda_coef_image *img)
{
    const uint32_t nb = img->n_blocks;
    const size_t first_bytes = (((size_t)nb + 1) * 4 + 15) & ~(size_t)15;
    uint32_t *first = NULL;
    if (posix_memalign((void **)&first, 64, first_bytes) != 0) { img->sp_status = JDA_ERROR_MEMORY; return; }
    memset(first, 0, first_bytes);
    uint64_t total = 0;
    for (uint32_t g = 0; g < nb; g++) {
        const int16_t *b = img->coefs + (size_t)g * 64;
        first[g] = (uint32_t)total;
        uint32_t k = 0;
        for (int q = 0; q < 16; q++) {
            uint64_t w;
            memcpy(&w, b + 4 * q, 8);
            if (w) for (int j = 0; j < 4; j++) k += b[4 * q + j] != 0;
        }
        total += k;
        if (total >= ((uint64_t)1 << 31)) { free(first); img->sp_status = JDA_UNSUPPORTED_FEATURE; return; }
    }
    first[nb] = (uint32_t)total;
    const size_t entry_bytes = ((size_t)total * 4 + 15) & ~(size_t)15;
    uint32_t *entries = NULL;
    if (posix_memalign((void **)&entries, 64, entry_bytes ? entry_bytes : 64) != 0) { free(first); img->sp_status = JDA_ERROR_MEMORY; return; }
    memset(entries, 0, entry_bytes ? entry_bytes : 64);
    uint32_t *e = entries;
    for (uint32_t g = 0; g < nb; g++) {
        const int16_t *b = img->coefs + (size_t)g * 64;
        const uint32_t hi = (g & 1023u) << 22;
        for (int q = 0; q < 16; q++) {
            uint64_t w;
            memcpy(&w, b + 4 * q, 8);
            if (!w) continue;
            for (int j = 0; j < 4; j++)
                if (b[4 * q + j] != 0) *e++ = hi | ((uint32_t)(4 * q + j) << 16) | (uint16_t)b[4 * q + j];
        }
    }
    img->sp_first = first; img->sp_entries = entries; img->sp_n_entries = (uint32_t)total;
}

} // namespace

extern "C" {

jda_coef_image *jda_progressive_prepare(const uint8_t *jpeg, int32_t len, int32_t *err)
{
    int32_t dummy;
    if (!err) err = &dummy;
    jda_coef_image *img = coef_image_new(jpeg, len, 1, err);
    if (!img) return NULL;
    const jda_image_info &I = img->info;
    Decoder *D = new (std::nothrow) Decoder;
    if (!D) { jda_coef_image_free(img); *err = JDA_ERROR_MEMORY; return NULL; }
    memset(D, 0, sizeof(*D));
    D->d = jpeg; D->len = len; D->I = I; D->coefs = img->coefs;
    for (int c = 0; c < 3; c++) { D->quant_out[c] = img->quant + 64 * c; D->raw_out[c] = img->raw_quant[c]; }
    D->restart_interval = 0;
    const int lh = (I.subsample == 0x22 || I.subsample == 0x21) ? 2 : 1, lv = (I.subsample == 0x22 || I.subsample == 0x12) ? 2 : 1;
    D->hmax = lh; D->vmax = lv;
    // the frame's component ids, and the first SOS: a second walk over the segments (the header parse keeps neither)
    int at = 2, first_sos = -1, rc = JDA_SUCCESS;
    while (at + 4 <= len) {
        if (jpeg[at] != 0xff) { at++; continue; }
        const int m = jpeg[at + 1];
        if (m == 0xff) { at++; continue; }
        if (m < 0xc0) { at += 2; continue; }
        const int seglen = (jpeg[at + 2] << 8) | jpeg[at + 3];
        if (m == 0xc2) {
            if (at + 2 + seglen > len || seglen < 8 + 3 * I.ncomp) { rc = JDA_DECODE_ERROR; break; }
            for (int c = 0; c < I.ncomp; c++) {
                Comp &C = D->comp[c];
                C.id = jpeg[at + 10 + 3 * c];
                D->tq[c] = jpeg[at + 12 + 3 * c] & 3;
                img->raw_qid[c] = (uint8_t)D->tq[c];
                C.h = c == 0 ? lh : 1; C.v = c == 0 ? lv : 1;
                const int wc = (I.width * C.h + lh - 1) / lh, hc = (I.height * C.v + lv - 1) / lv;      // the component's own extent (A.1.1)
                C.blocks_w = (wc + 7) / 8; C.blocks_h = (hc + 7) / 8;
                C.mcu_off = c == 0 ? 0 : lh * lv + c - 1;
            }
        } else if (m == 0xc4) { if (!D->read_dht(at + 2, seglen)) { rc = JDA_DECODE_ERROR; break; } }
        else if (m == 0xdb) { if (!D->read_dqt(at + 2, seglen)) { rc = JDA_DECODE_ERROR; break; } }
        else if (m == 0xee) { if (seglen >= 7 && at + 9 <= len && !memcmp(jpeg + at + 4, "Adobe", 5)) img->adobe = 1; }
        else if (m == 0xdd) { if (seglen == 4 && at + 6 <= len) D->restart_interval = (jpeg[at + 4] << 8) | jpeg[at + 5]; }
        else if (m == 0xda) { first_sos = at; break; }
        at += 2 + seglen;
    }
    if (rc == JDA_SUCCESS && first_sos < 0) rc = JDA_DECODE_ERROR;
    if (rc == JDA_SUCCESS) rc = D->run(first_sos);
    delete D;
    if (rc != JDA_SUCCESS) { jda_coef_image_free(img); *err = rc; return NULL; }      // nothing is delivered: no partial image
    *err = JDA_SUCCESS;
    return img;
}

// Every scan of a Huffman-coded 8-bit file of one, three or four components, sequential (SOF0, SOF1: whole blocks, F.2.2) or progressive
// (SOF2: the Annex G decoder above), interleaved or a scan per component: the coefficient image the exact decode's _ex calls take
// (DESIGN.md 5.19).  One and three components: the image jda_progressive_prepare makes of a progressive file, in every field.  Four:
// components 1 and 2 at 1x1, component 0 at 1x1, 2x1, 1x2 or 2x2, component 3 at 1x1 or at component 0's factors -- components 0..2 as a
// three-component image, component 3 as the gray child (jda_coef_image::k); anything else: JDA_UNSUPPORTED_FEATURE.
jda_coef_image *jda_coef_prepare(const uint8_t *jpeg, int32_t len, int32_t *err)
{
    int32_t dummy;
    if (!err) err = &dummy;
    jda_image_info I;
    int32_t hv[4] = { 0, 0, 0, 0 }, colour = -1, adobe = 0;
    int rc = jda_parse_coef(jpeg, len, &I, hv, &colour, &adobe);
    if (rc == JDA_SUCCESS && !((I.ncomp == 1 || I.ncomp == 3 || I.ncomp == 4) && I.bpp == 8 * I.ncomp && I.width > 0 && I.height > 0 && I.mcu_w > 0 &&
                               (I.subsample == 0x00 || I.subsample == 0x11 || I.subsample == 0x22 || I.subsample == 0x21 || I.subsample == 0x12)))
        rc = JDA_UNSUPPORTED_FEATURE;
    if (rc == JDA_SUCCESS && I.ncomp >= 3 && (hv[1] != 0x11 || hv[2] != 0x11)) rc = JDA_UNSUPPORTED_FEATURE;
    if (rc == JDA_SUCCESS && I.ncomp == 4 && hv[3] != 0x11 && hv[3] != hv[0]) rc = JDA_UNSUPPORTED_FEATURE;
    if (rc != JDA_SUCCESS) { *err = rc; return NULL; }
    const int lh = (I.subsample == 0x22 || I.subsample == 0x21) ? 2 : 1, lv = (I.subsample == 0x22 || I.subsample == 0x12) ? 2 : 1;
    const bool k_full = I.ncomp == 4 && hv[3] == hv[0];
    I.blocks_per_mcu = (I.ncomp >= 3 ? 2 : 0) + lh * lv;          // (of components 0..2: the header walk counts a three-component file's chroma only)
    auto make = [&](const jda_image_info &info, int col) -> jda_coef_image * {
        jda_coef_image *m = new (std::nothrow) jda_coef_image;
        if (!m) return NULL;
        m->info = info;
        m->q_id[0] = 0; m->q_id[1] = 1; m->q_id[2] = 2;
        memset(m->quant, 0, sizeof(m->quant)); memset(m->raw_quant, 0, sizeof(m->raw_quant)); memset(m->raw_qid, 0, sizeof(m->raw_qid));
        m->adobe = (uint8_t)adobe; m->colour = (uint8_t)col;
        m->n_blocks = (uint32_t)(info.mcus_x * info.mcus_y * info.blocks_per_mcu);
        m->coefs = NULL; m->k = NULL;
        m->sp_first = m->sp_entries = NULL; m->sp_n_entries = 0; m->sp_status = JDA_SUCCESS;
        const size_t bytes = ((size_t)m->n_blocks * 128 + 15) & ~(size_t)15;
        if (posix_memalign((void **)&m->coefs, 64, bytes ? bytes : 64) != 0) { m->coefs = NULL; delete m; return NULL; }
        memset(m->coefs, 0, bytes);
        return m;
    };
    jda_coef_image *img = make(I, colour);
    if (!img) { *err = JDA_ERROR_MEMORY; return NULL; }
    if (I.ncomp == 4) {
        jda_image_info K = I;                                  // component 3 as a gray image over its MCU-padded block grid
        const int kh = k_full ? lh : 1, kv = k_full ? lv : 1;
        K.ncomp = 1; K.bpp = 8; K.subsample = 0; K.mcu_w = K.mcu_h = 8; K.blocks_per_mcu = 1;
        K.width = (I.width * kh + lh - 1) / lh; K.height = (I.height * kv + lv - 1) / lv;
        K.mcus_x = I.mcus_x * kh; K.mcus_y = I.mcus_y * kv;
        img->k = make(K, JDA_CS_GRAY);
        if (!img->k) { jda_coef_image_free(img); *err = JDA_ERROR_MEMORY; return NULL; }
        img->sp_status = JDA_UNSUPPORTED_FEATURE;              // (dense only)
    }
    Decoder *D = new (std::nothrow) Decoder;
    if (!D) { jda_coef_image_free(img); *err = JDA_ERROR_MEMORY; return NULL; }
    memset(D, 0, sizeof(*D));
    D->d = jpeg; D->len = len; D->I = I; D->coefs = img->coefs;
    D->sequential = I.jpeg_type != 1;
    for (int c = 0; c < 3; c++) { D->quant_out[c] = img->quant + 64 * c; D->raw_out[c] = img->raw_quant[c]; }
    if (img->k) { D->quant_out[3] = img->k->quant; D->raw_out[3] = img->k->raw_quant[0]; }
    D->hmax = lh; D->vmax = lv;
    int at = 2, first_sos = -1;
    while (at + 4 <= len) {                                    // (the walk of jda_progressive_prepare, four components and any SOF let in)
        if (jpeg[at] != 0xff) { at++; continue; }
        const int m = jpeg[at + 1];
        if (m == 0xff) { at++; continue; }
        if (m < 0xc0) { at += 2; continue; }
        const int seglen = (jpeg[at + 2] << 8) | jpeg[at + 3];
        if (m == 0xc0 || m == 0xc1 || m == 0xc2) {
            if (at + 2 + seglen > len || seglen < 8 + 3 * I.ncomp) { rc = JDA_DECODE_ERROR; break; }
            for (int c = 0; c < I.ncomp; c++) {
                Comp &C = D->comp[c];
                C.id = jpeg[at + 10 + 3 * c];
                D->tq[c] = jpeg[at + 12 + 3 * c] & 3;
                if (c < 3) img->raw_qid[c] = (uint8_t)D->tq[c]; else img->k->raw_qid[0] = (uint8_t)D->tq[c];
                const bool full = c == 0 || (c == 3 && k_full);
                C.h = full ? lh : 1; C.v = full ? lv : 1;
                const int wc = (I.width * C.h + lh - 1) / lh, hc = (I.height * C.v + lv - 1) / lv;      // the component's own extent (A.1.1)
                C.blocks_w = (wc + 7) / 8; C.blocks_h = (hc + 7) / 8;
                C.mcu_off = c == 0 ? 0 : lh * lv + c - 1;
                if (c == 3) { C.rm = img->k->coefs; C.rm_w = img->k->info.mcus_x; }
            }
        } else if (m == 0xc4) { if (!D->read_dht(at + 2, seglen)) { rc = JDA_DECODE_ERROR; break; } }
        else if (m == 0xdb) { if (!D->read_dqt(at + 2, seglen)) { rc = JDA_DECODE_ERROR; break; } }
        else if (m == 0xdd) { if (seglen == 4 && at + 6 <= len) D->restart_interval = (jpeg[at + 4] << 8) | jpeg[at + 5]; }
        else if (m == 0xda) { first_sos = at; break; }
        at += 2 + seglen;
    }
    if (rc == JDA_SUCCESS && first_sos < 0) rc = JDA_DECODE_ERROR;
    if (rc == JDA_SUCCESS) rc = D->run(first_sos);
    delete D;
    if (rc != JDA_SUCCESS) { jda_coef_image_free(img); *err = rc; return NULL; }      // nothing is delivered: no partial image
    *err = JDA_SUCCESS;
    return img;
}

// component 3 of a four-component image (jda_coef_prepare) as the gray coefficient image it is stored as -- the parent's, freed with it --,
// NULL for every other image
const jda_coef_image *jda_coef_image_component3(const jda_coef_image *img) { return img ? img->k : NULL; }

jda_coef_image *jda_coef_image_from_coefficients(const uint8_t *jpeg, int32_t len, const int16_t *coefs, uint32_t n_blocks, int32_t *err)
{
    int32_t dummy;
    if (!err) err = &dummy;
    if (!coefs) { *err = JDA_INVALID_PARAMETER; return NULL; }
    jda_coef_image *img = coef_image_new(jpeg, len, 0, err);
    if (!img) return NULL;
    if (n_blocks != img->n_blocks) { jda_coef_image_free(img); *err = JDA_INVALID_PARAMETER; return NULL; }
    memcpy(img->coefs, coefs, (size_t)n_blocks * 128);
    return img;
}

void jda_coef_image_free(jda_coef_image *img)
{
    if (!img) return;
    if (img->k) jda_coef_image_free(img->k);
    free(img->coefs);
    free(img->sp_first);
    free(img->sp_entries);
    delete img;
}

const jda_image_info *jda_coef_image_get_info(const jda_coef_image *img) { return img ? &img->info : NULL; }

const int16_t *jda_coef_image_coefficients(const jda_coef_image *img, uint32_t *n_blocks)
{
    if (n_blocks) *n_blocks = img ? img->n_blocks : 0;
    return img ? img->coefs : NULL;
}

const int16_t *jda_coef_image_quant(const jda_coef_image *img, uint8_t *q_id)
{
    if (!img) return NULL;
    if (q_id) memcpy(q_id, img->q_id, 3);
    return img->quant;
}

// the quantisers of Y, Cb, Cr as the file's DQT segments list them (3 x 64, zigzag order), the table ids its frame header gives them, and
// whether it carries an Adobe APP14 segment: what a lossless recode writes back, and what it refuses (jda_recode_plan.h)
int jda_coef_image_colour_model(const jda_coef_image *img) { return img ? img->colour : -1; }
void jda_coef_image_raw_quant(const jda_coef_image *img, uint16_t *quant_zz, uint8_t *q_id, int32_t *adobe)
{
    if (quant_zz) memcpy(quant_zz, img->raw_quant, sizeof(img->raw_quant));
    if (q_id) memcpy(q_id, img->raw_qid, 3);
    if (adobe) *adobe = img->adobe;
}

const uint32_t *jda_coef_image_sparse(const jda_coef_image *img, const uint32_t **first, uint32_t *n_entries)
{
    if (first) *first = NULL;
    if (n_entries) *n_entries = 0;
    if (!img) return NULL;
    if (img->k) return NULL;                                      // (a four-component image: dense only, sp_status says so)
    jda_coef_image *m = const_cast<jda_coef_image *>(img);        // (the cache is the image's own)
    std::call_once(m->sparse_once, sparse_pack, m);
    if (!img->sp_first) return NULL;
    if (first) *first = img->sp_first;
    if (n_entries) *n_entries = img->sp_n_entries;
    return img->sp_entries;
}

int jda_coef_image_sparse_status(const jda_coef_image *img)
{
    if (!img) return JDA_INVALID_PARAMETER;
    (void)jda_coef_image_sparse(img, NULL, NULL);
    return img->sp_status;
}

size_t jda_coef_image_sparse_bytes(const jda_coef_image *img)
{
    if (!img || !jda_coef_image_sparse(img, NULL, NULL)) return 0;
    return ((((size_t)img->n_blocks + 1) * 4 + 15) & ~(size_t)15) + (((size_t)img->sp_n_entries * 4 + 15) & ~(size_t)15);
}

} // extern "C"
