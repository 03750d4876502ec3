// jda_recode_plan.h -- HOST: the arguments of jda_recode_images checked and turned into the encoder's own job records (jda_encode_plan.h,
// jda_encode_prog_plan.h) with a source record each in the place of a pixel pointer, and the files' headers with the SOURCE's quantisers in
// the place of a quality.  No HIP in here: the runtime and the CPU tests (tests/hostsim/recode_sim.cpp) run the same checks and build the
// same records.  The definition: DESIGN.md 5.14; the stages: jda_rc_* in jda_device_core.h.
// jda_recode_images_ex (a flip, a turn, a transposition or an MCU crop a job) is the same plan with a jda_recode_xform a job
// resolved into a jda_rc_xf record: the job records, DQT segments and headers are then the TURNED region's.
//
// The range rule (|AC| <= 1023, -1024 <= DC <= 1023 for every block, checked by the stages, per block) is stricter than libjpeg's, which
// refuses only a DC DIFFERENCE beyond category 11: the target's restart interval may differ from the source's, so the differences of the
// target are not the source's, and a difference is not local to a block.  A source inside the rule can be written with any interval.
#ifndef JDA_RECODE_PLAN_H
#define JDA_RECODE_PLAN_H

#include "jda_encode_prog_plan.h"

// what the host knows of one source: a resident baseline image or a resident coefficient image
struct jda_recode_src_host {
    int kind;                        // JDA_RC_IMAGE, JDA_RC_COEF, or JDA_RC_SPARSE: a coefficient image whose sparse form is resident (refused)
    jda_image_info info;
    uint16_t quant[3][64];           // the DQT entries of Y, Cb, Cr as the source file lists them (zigzag order)
    uint8_t q_id[3];                 // .. and the table id its frame header gives each
    int adobe;                       // the source file has an Adobe APP14 segment
    uint32_t n_mcus_ok;              // a baseline image: the MCUs its pre-scan validated
    jda_rc_src dev;                  // the device pointers of the job's record
};
enum { JDA_RC_SPARSE = 2 };

struct jda_recode_plan_out {
    bool progressive;
    jda_pe_plan_out P;               // P.B: the job records, words and headers of the ACTIVE jobs; segments where progressive
    std::vector<jda_rc_src> src;     // an active job each
    std::vector<int32_t> job_of;     // an active job's index in the call
    int any_image, any_coef;
    std::vector<jda_rc_xf> xf;       // empty: no job of the call has an operation or a rectangle; else an active job each
};

static inline int32_t jda_recode_sampling(const jda_image_info &I);

// ---- flip, rotate, transpose and MCU crop ----
// one job's jda_recode_xform resolved against its source: EXIF, crop, trim and the sampling check
struct jda_recode_xf_host {
    jda_rc_xf dev;                   // the op bits, the source grid's width, the region's origin and size in MCUs
    int32_t w, h;                    // the target's size in pixels
    uint32_t tcx, tcy;               // .. and its MCU grid
    bool plain;                      // no operation and no rectangle: the job as jda_recode_images runs it
};
// JDA_SUCCESS; JDA_INVALID_PARAMETER: an argument the CALL refuses; JDA_UNSUPPORTED_FEATURE: the job is refused.  x NULL: none.
static inline int jda_recode_xf_resolve(const jda_image_info &I, const jda_recode_xform *x, jda_recode_xf_host *o)
{
    static const jda_recode_xform none = { JDA_XF_NONE, 0, { 0, 0, 0, 0 } };
    if (!x) x = &none;
    memset(o, 0, sizeof(*o));
    if (x->op < JDA_XF_NONE || x->op > JDA_XF_EXIF || (x->flags & ~JDA_XF_TRIM) != 0) return JDA_INVALID_PARAMETER;
    const int32_t *r = x->mcu_rect;
    if (r[0] < 0 || r[1] < 0 || r[2] < 0 || r[3] < 0) return JDA_INVALID_PARAMETER;
    const bool whole = (r[0] | r[1] | r[2] | r[3]) == 0;
    int32_t op = x->op;
    if (op == JDA_XF_EXIF) {
        static const int32_t of[9] = { JDA_XF_NONE, JDA_XF_NONE, JDA_XF_FLIP_H, JDA_XF_ROT_180, JDA_XF_FLIP_V, JDA_XF_TRANSPOSE, JDA_XF_ROT_90, JDA_XF_TRANSVERSE, JDA_XF_ROT_270 };
        op = I.orientation >= 0 && I.orientation <= 8 ? of[I.orientation] : JDA_XF_NONE;
    }
    static const uint32_t bits_of[8] = { 0u, JDA_RC_XF_MX, JDA_RC_XF_MY, JDA_RC_XF_T, JDA_RC_XF_T | JDA_RC_XF_MX | JDA_RC_XF_MY, JDA_RC_XF_T | JDA_RC_XF_MX,
                                         JDA_RC_XF_MX | JDA_RC_XF_MY, JDA_RC_XF_T | JDA_RC_XF_MY };
    const uint32_t bits = bits_of[op];
    if (bits == 0u && whole) {                                                                 // the job as jda_recode_images runs it: its shape is the plan's to judge
        o->dev.scx = (uint32_t)I.mcus_x; o->dev.rw = (uint32_t)I.mcus_x; o->dev.rh = (uint32_t)I.mcus_y;
        o->w = I.width; o->h = I.height; o->tcx = (uint32_t)I.mcus_x; o->tcy = (uint32_t)I.mcus_y; o->plain = true;
        return JDA_SUCCESS;
    }
    if (I.mcus_x <= 0 || I.mcus_y <= 0 || I.mcu_w <= 0 || I.mcu_h <= 0) return JDA_INVALID_PARAMETER;
    if (!whole && (r[2] == 0 || r[3] == 0 || (int64_t)r[0] + r[2] > I.mcus_x || (int64_t)r[1] + r[3] > I.mcus_y)) return JDA_INVALID_PARAMETER;
    const bool t = (bits & JDA_RC_XF_T) != 0u;
    // the SOURCE's axes that are mirrored: transposed, the target's x is the source's y
    const bool src_mx = (bits & (t ? JDA_RC_XF_MY : JDA_RC_XF_MX)) != 0u, src_my = (bits & (t ? JDA_RC_XF_MX : JDA_RC_XF_MY)) != 0u;
    int32_t x0 = whole ? 0 : r[0], y0 = whole ? 0 : r[1], rw = whole ? I.mcus_x : r[2], rh = whole ? I.mcus_y : r[3];
    int64_t pw = std::min<int64_t>((int64_t)rw * I.mcu_w, (int64_t)I.width - (int64_t)x0 * I.mcu_w), ph = std::min<int64_t>((int64_t)rh * I.mcu_h, (int64_t)I.height - (int64_t)y0 * I.mcu_h);
    if (pw <= 0 || ph <= 0) return JDA_INVALID_PARAMETER;
    if (t && I.mcu_w != I.mcu_h) return JDA_UNSUPPORTED_FEATURE;                               // 4:2:2 would become 4:4:0
    if (src_mx && pw % I.mcu_w) {
        if (!(x->flags & JDA_XF_TRIM) || --rw == 0) return JDA_UNSUPPORTED_FEATURE;
        pw = (int64_t)rw * I.mcu_w;
    }
    if (src_my && ph % I.mcu_h) {
        if (!(x->flags & JDA_XF_TRIM) || --rh == 0) return JDA_UNSUPPORTED_FEATURE;
        ph = (int64_t)rh * I.mcu_h;
    }
    o->dev.bits = bits; o->dev.scx = (uint32_t)I.mcus_x; o->dev.x0 = (uint32_t)x0; o->dev.y0 = (uint32_t)y0; o->dev.rw = (uint32_t)rw; o->dev.rh = (uint32_t)rh;
    o->w = (int32_t)(t ? ph : pw); o->h = (int32_t)(t ? pw : ph);
    o->tcx = (uint32_t)(t ? rh : rw); o->tcy = (uint32_t)(t ? rw : rh);
    return JDA_SUCCESS;
}
// the shape of the file a job writes (the source's record with the target's size and grid, no orientation), or its refusal
static inline int jda_recode_geometry_of(const jda_image_info *info, const jda_recode_xform *x, jda_image_info *out)
{
    if (!info || !out) return JDA_INVALID_PARAMETER;
    jda_recode_xf_host X;
    const int rc = jda_recode_xf_resolve(*info, x, &X);
    if (rc != JDA_SUCCESS) return rc;
    if (jda_recode_sampling(*info) < 0) return JDA_UNSUPPORTED_FEATURE;
    *out = *info;
    out->width = X.w; out->height = X.h; out->mcus_x = (int32_t)X.tcx; out->mcus_y = (int32_t)X.tcy; out->orientation = 0;
    return JDA_SUCCESS;
}
// the quantisers of a job: the source's, every table transposed where the job transposes -- q'[z] = q[T[z]]
static inline void jda_recode_xf_quant(const uint16_t quant[3][64], uint32_t bits, uint16_t out[3][64])
{
    for (int c = 0; c < 3; c++) for (uint32_t z = 0; z < 64u; z++) out[c][z] = quant[c][(bits & JDA_RC_XF_T) ? jda_rc_tz(z) : z];
}

// the encoder's sampling of a source, or -1 (4:4:0, or a shape the front end would not have let through)
static inline int32_t jda_recode_sampling(const jda_image_info &I)
{
    if (I.ncomp == 1) return JDA_ENCODE_GRAY;
    if (I.ncomp != 3) return -1;
    return I.subsample == 0x11 ? JDA_ENCODE_444 : I.subsample == 0x21 ? JDA_ENCODE_422 : I.subsample == 0x22 ? JDA_ENCODE_420 : -1;
}
// the restart interval of the target: -1 = the source's (none in a progressive file); false: not a value the call takes
static inline bool jda_recode_interval(const jda_image_info &I, int32_t form, int32_t restart_interval, int32_t *ri)
{
    if (form < JDA_RECODE_BASELINE || form > JDA_RECODE_PROGRESSIVE || restart_interval < -1 || restart_interval > 65535) return false;
    if (form == JDA_RECODE_PROGRESSIVE) { *ri = 0; return restart_interval <= 0; }
    *ri = restart_interval < 0 ? (I.restart_interval > 0 && I.restart_interval <= 65535 ? I.restart_interval : 0) : restart_interval;
    return true;
}
// One DQT segment per distinct table id, in the order Y, Cb, Cr first name it, under the source's id; 8-bit entries unless one passes 255
// (libjpeg's emit_dqt).  false: an entry of zero (no DQT defined the table), or one id with two contents (a table redefined between the
// scans of a progressive source).
static inline bool jda_recode_dqt(int nc, const uint16_t quant[3][64], const uint8_t q_id[3], std::vector<uint8_t> &o)
{
    for (int c = 0; c < nc; c++) {
        if (q_id[c] > 3) return false;
        int first = c;
        for (int k = 0; k < c; k++) if (q_id[k] == q_id[c]) { first = k; break; }
        if (first != c) { if (memcmp(quant[first], quant[c], 128) != 0) return false; continue; }
        bool wide = false;
        for (int z = 0; z < 64; z++) { if (quant[c][z] == 0) return false; if (quant[c][z] > 255) wide = true; }
        std::vector<uint8_t> p;
        p.push_back((uint8_t)((wide ? 0x10 : 0x00) | q_id[c]));
        for (int z = 0; z < 64; z++) { if (wide) p.push_back((uint8_t)(quant[c][z] >> 8)); p.push_back((uint8_t)quant[c][z]); }
        jda_encode_put_seg(o, 0xdb, p);
    }
    return true;
}
// the bytes of the DQT segments the encoder's bounds and header rooms count: a table of 8-bit entries for luma, and one for chroma
static inline uint32_t jda_recode_std_dqt(int nc) { return nc == 1 ? 69u : 138u; }
// .. and the most a source's own can take: a table of 16-bit entries a component
static inline uint32_t jda_recode_max_dqt(int nc) { return (uint32_t)nc * 133u; }

static inline int jda_recode_bound_bytes(const jda_image_info *info, int32_t form, int32_t restart_interval, int64_t *bytes)
{
    if (!bytes) return JDA_INVALID_PARAMETER;
    *bytes = 0;
    if (!info) return JDA_INVALID_PARAMETER;
    int32_t ri = 0;
    if (!jda_recode_interval(*info, form, restart_interval, &ri)) return JDA_INVALID_PARAMETER;
    const int32_t sampling = jda_recode_sampling(*info);
    if (sampling < 0) return JDA_UNSUPPORTED_FEATURE;
    int64_t b = 0;
    const int rc = form == JDA_RECODE_PROGRESSIVE ? jda_pe_bound_bytes(info->width, info->height, sampling, &b) : jda_encode_bound_bytes(info->width, info->height, sampling, ri, &b);
    if (rc != JDA_SUCCESS) return rc;
    *bytes = b + (int64_t)(jda_recode_max_dqt(info->ncomp) - jda_recode_std_dqt(info->ncomp));
    return JDA_SUCCESS;
}

// n >= 1 jobs.  status[i]: JDA_SUCCESS for a job that runs, else why it does not (the call goes on without it).  The return value is the
// call's: JDA_INVALID_PARAMETER for arguments no job can be made of.  plan->src.empty(): nothing to run.
// xforms: NULL, or a jda_recode_xform a job
static inline int jda_recode_plan_jobs_ex(int32_t n, const jda_recode_src_host *hosts, const jda_recode_job *jobs, const jda_recode_xform *xforms, void *const *dst,
                                          const int64_t *dst_capacity, int32_t *status, jda_recode_plan_out *plan)
{
    jda_encode_plan_out &B = plan->P.B;
    B.jobs.clear(); B.quant.clear(); B.huff.clear(); B.hdr.clear(); B.n_blocks = B.n_int = B.n_chunks = 0; B.u_total = 0; B.quality.clear(); B.n_opt = 0;
    B.dqt.clear(); B.tq.clear(); B.hdr_room.clear();
    plan->P.segs.clear(); plan->P.pjobs.clear(); plan->P.words.clear(); plan->P.hdr.clear(); plan->P.hdr_grow.clear(); plan->P.n_units = plan->P.n_chunks = 0; plan->P.u_total = 0;
    plan->src.clear(); plan->job_of.clear(); plan->any_image = plan->any_coef = 0; plan->progressive = false; plan->xf.clear();
    if (n <= 0 || !hosts || !jobs || !dst || !dst_capacity || !status) return JDA_INVALID_PARAMETER;
    int n_prog = 0;
    for (int i = 0; i < n; i++) {
        int32_t ri;
        if (jobs[i].reserved0 != 0 || jobs[i].reserved1 != 0 || !dst[i] || dst_capacity[i] < 0) return JDA_INVALID_PARAMETER;
        if (hosts[i].kind != JDA_RC_IMAGE && hosts[i].kind != JDA_RC_COEF && hosts[i].kind != JDA_RC_SPARSE) return JDA_INVALID_PARAMETER;
        if (!jda_recode_interval(hosts[i].info, jobs[i].form, jobs[i].restart_interval, &ri)) return JDA_INVALID_PARAMETER;
        n_prog += jobs[i].form == JDA_RECODE_PROGRESSIVE ? 1 : 0;
    }
    std::vector<jda_recode_xf_host> X((size_t)n);
    std::vector<int> xrc((size_t)n, JDA_SUCCESS);
    bool any_xf = false;
    for (int i = 0; i < n; i++) {
        xrc[(size_t)i] = jda_recode_xf_resolve(hosts[i].info, xforms ? &xforms[i] : NULL, &X[(size_t)i]);
        if (xrc[(size_t)i] == JDA_INVALID_PARAMETER) return JDA_INVALID_PARAMETER;
        if (xrc[(size_t)i] != JDA_SUCCESS || !X[(size_t)i].plain) any_xf = true;
    }
    if (n_prog != 0 && n_prog != n) return JDA_INVALID_PARAMETER;                          // all jobs of a call are progressive, or none is
    plan->progressive = n_prog != 0;
    if (plan->progressive) for (int i = 1; i < n; i++) if ((hosts[i].info.ncomp == 1) != (hosts[0].info.ncomp == 1)) return JDA_INVALID_PARAMETER;
    // no destination may share a byte with another
    {
        std::vector<std::pair<uintptr_t, uintptr_t>> r;
        for (int i = 0; i < n; i++) if (dst_capacity[i] > 0) r.push_back({ (uintptr_t)dst[i], (uintptr_t)dst[i] + (size_t)dst_capacity[i] });
        std::sort(r.begin(), r.end());
        for (size_t k = 1; k < r.size(); k++) if (r[k].first < r[k - 1].second) return JDA_INVALID_PARAMETER;
    }
    uint64_t blocks = 0, ints = 0;
    for (int i = 0; i < n; i++) {
        const jda_recode_src_host &H = hosts[i];
        const jda_image_info &I = H.info;
        const int32_t sampling = jda_recode_sampling(I);
        status[i] = JDA_SUCCESS;
        if (sampling < 0 || H.adobe || H.kind == JDA_RC_SPARSE || xrc[(size_t)i] != JDA_SUCCESS) { status[i] = JDA_UNSUPPORTED_FEATURE; continue; }
        const jda_recode_xf_host &T = X[(size_t)i];
        int32_t ri = 0;
        (void)jda_recode_interval(I, jobs[i].form, jobs[i].restart_interval, &ri);
        jda_encode_dev_job J;
        memset(&J, 0, sizeof(J));
        uint64_t jb, ji;
        if (!jda_encode_counts(I.width, I.height, sampling, ri, &J.cx, &J.cy, &J.bpm, &jb, &ji)) { status[i] = JDA_UNSUPPORTED_FEATURE; continue; }
        if ((int32_t)J.cx != I.mcus_x || (int32_t)J.cy != I.mcus_y || (int32_t)J.bpm != I.blocks_per_mcu) { status[i] = JDA_UNSUPPORTED_FEATURE; continue; }
        if (H.kind == JDA_RC_IMAGE && H.n_mcus_ok < J.cx * J.cy) { status[i] = JDA_DECODE_ERROR; continue; }      // a bad MCU: nothing behind it is known (the WHOLE source, whatever the region)
        // the target's shape: the region, turned
        if (!jda_encode_counts(T.w, T.h, sampling, ri, &J.cx, &J.cy, &J.bpm, &jb, &ji) || J.cx != T.tcx || J.cy != T.tcy) { status[i] = JDA_UNSUPPORTED_FEATURE; continue; }
        const bool opt = jobs[i].form == JDA_RECODE_OPTIMIZE;
        if ((opt || plan->progressive) && jb > JDA_EN_OPT_MAX_BLOCKS) { status[i] = JDA_UNSUPPORTED_FEATURE; continue; }
        if (blocks + jb > 0x7fffffffull) { status[i] = JDA_UNSUPPORTED_FEATURE; continue; }                      // (the flat block list is indexed by 32 bits)
        std::vector<uint8_t> dqt;
        uint16_t quant[3][64];
        jda_recode_xf_quant(H.quant, T.dev.bits, quant);
        if (!jda_recode_dqt(I.ncomp, quant, H.q_id, dqt)) { status[i] = JDA_UNSUPPORTED_FEATURE; continue; }
        J.dst = (uint8_t *)dst[i]; J.capacity = (uint64_t)dst_capacity[i];
        J.w = (uint32_t)T.w; J.h = (uint32_t)T.h;
        J.hs = sampling >= JDA_ENCODE_422 ? 2u : 1u; J.vs = sampling == JDA_ENCODE_420 ? 2u : 1u; J.nc = sampling == JDA_ENCODE_GRAY ? 1u : 3u;
        J.wb = (J.w + 7u) / 8u; J.hb = (J.h + 7u) / 8u; J.ri = (uint32_t)ri;
        J.block0 = (uint32_t)blocks; J.n_blocks = (uint32_t)jb; J.int0 = (uint32_t)ints; J.n_int = (uint32_t)ji;
        blocks += jb; ints += ji;
        J.hdr_off = (uint32_t)B.hdr.size();
        const uint8_t tq[3] = { H.q_id[0], H.q_id[I.ncomp == 3 ? 1 : 0], H.q_id[I.ncomp == 3 ? 2 : 0] };
        const uint32_t room = jda_encode_header_bytes(sampling, ri) - jda_recode_std_dqt(I.ncomp) + (uint32_t)dqt.size();
        if (opt) {
            B.n_opt++;
            J.huff_off = B.n_opt * JDA_EN_HUFF_DWORDS; J.hist_off = (B.n_opt - 1u) * JDA_EN_HUFF_DWORDS;
            B.hdr.resize(B.hdr.size() + room);                                             // (hdr_len: 0 until the tables are made)
        } else {
            J.hist_off = JDA_EN_NO_HIST;
            if (!plan->progressive) {
                jda_encode_header_explicit(T.w, T.h, sampling, dqt.data(), dqt.size(), tq, ri, NULL, B.hdr);
                J.hdr_len = (uint32_t)B.hdr.size() - J.hdr_off;
            }
        }
        B.jobs.push_back(J);
        B.quality.push_back(0);
        B.tq.insert(B.tq.end(), tq, tq + 3);
        B.hdr_room.push_back(room);
        plan->P.hdr_grow.push_back(dqt.size() > jda_recode_std_dqt(I.ncomp) ? (uint32_t)dqt.size() - jda_recode_std_dqt(I.ncomp) : 0u);
        B.dqt.push_back(std::move(dqt));
        plan->src.push_back(H.dev);
        plan->src.back().kind = (uint32_t)H.kind;
        plan->job_of.push_back(i);
        if (any_xf) plan->xf.push_back(T.dev);
        if (H.kind == JDA_RC_IMAGE) plan->any_image = 1; else plan->any_coef = 1;
    }
    if (plan->src.empty()) return JDA_SUCCESS;
    B.quant.resize(1);                                                                     // (no stage of a recode reads a quantiser record)
    memset(&B.quant[0], 0, sizeof(B.quant[0]));
    B.huff.assign((size_t)JDA_EN_HUFF_DWORDS * (1u + B.n_opt), 0u);
    jda_encode_huff_words(B.huff.data());
    B.n_blocks = (uint32_t)blocks; B.n_int = (uint32_t)ints;
    if (plan->progressive) return jda_pe_plan_segments(&plan->P);
    return JDA_SUCCESS;
}
static inline int jda_recode_plan_jobs(int32_t n, const jda_recode_src_host *hosts, const jda_recode_job *jobs, void *const *dst, const int64_t *dst_capacity, int32_t *status,
                                       jda_recode_plan_out *plan)
{
    return jda_recode_plan_jobs_ex(n, hosts, jobs, NULL, dst, dst_capacity, status, plan);
}
static inline int jda_recode_bound_bytes_ex(const jda_image_info *info, const jda_recode_xform *x, int32_t form, int32_t restart_interval, int64_t *bytes)
{
    if (!bytes) return JDA_INVALID_PARAMETER;
    *bytes = 0;
    jda_image_info out;
    const int rc = jda_recode_geometry_of(info, x, &out);
    if (rc != JDA_SUCCESS) return rc;
    out.restart_interval = info->restart_interval;
    return jda_recode_bound_bytes(&out, form, restart_interval, bytes);
}

#endif
