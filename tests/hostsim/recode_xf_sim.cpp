// tests/hostsim/recode_xf_sim.cpp -- TEST INFRASTRUCTURE: the two transforming recode stages on the CPU (jda_rc_extract_xf and
// jda_rc_from_coef_xf of jpegdec_amd/csrc/jda_kernels.hip), and the host plan of jda_recode_images_ex (jda_recode_plan.h).
//
// recodexfsim_files is recode_sim.cpp's recodesim_files with a jda_recode_xform a job: the sources are prepared and laid out the same way
// (this file includes recode_sim.cpp for that, for its IO policies and for the stages behind), the plan is jda_recode_plan_jobs_ex's, and
// where the plan says so the stage in the place of the blocks stage is the _xf pair, stepped lane by lane through the kernels' OWN code the
// way the GPU runs it: a workgroup of 256 lanes decodes into its slots (poisoned before every workgroup) and tags each with its block's place
// in the target's order; behind the barrier every wavefront's lanes store the slots, the lanes in REVERSE order.  On top of encode_sim.cpp's
// policy (an access lies whole inside one allocation and is aligned to its own width) a byte of the call's coefficients and block words is
// stored ONCE: a second store to it is an error (-46), one that no lane stored is too (-71).  A call in which no job has an operation or a
// rectangle runs the plain pair, as the runtime does; info tells which ran.
#include "recode_sim.cpp"

namespace {
struct OnceIO : SimIO {
    void once(void *p, size_t n)
    {
        Alloc *a = find(p, n);
        if (!a || a->init.empty()) return;
        for (size_t i = 0; i < n; i++) if (a->init[(size_t)((uint8_t *)p - a->base) + i]) { fail(-46); return; }
    }
    void st32(uint32_t *p, uint32_t v) { once(p, 4); SimIO::st32(p, v); }
    void st128(void *p, const uint32_t *v) { once(p, 16); SimIO::st128(p, v); }
};
}

// As recodesim_files (recode_sim.cpp), with xforms: NULL, or a jda_recode_xform a job.  info = {blocks, jobs that run, launches of extract,
// of from_coef, of extract_xf, of from_coef_xf}.
extern "C" int recodexfsim_files(int n, const uint8_t *const *jpegs, const int32_t *lens, const int32_t *form, const int32_t *ri, const int32_t *sparse,
                                 const jda_recode_xform *xforms, void *const *dst, const int64_t *cap, int64_t *dst_bytes, int32_t *status, int16_t *coef, uint32_t *meta,
                                 uint32_t *bad, uint8_t *hdr, int64_t hdr_cap, int64_t *hdr_len, uint64_t *info)
{
    Run R;
    R.io.err = 0;
    std::vector<Source> S((size_t)n);
    std::vector<jda_recode_src_host> hosts((size_t)n);
    std::vector<jda_recode_job> jobs((size_t)n);
    SimIO sources;
    sources.err = 0;
    int rc = JDA_SUCCESS;
    for (int i = 0; i < n && rc == JDA_SUCCESS; i++) {
        rc = open_source(jpegs[i], lens[i], sparse ? sparse[i] : 0, S[(size_t)i], hosts[(size_t)i], sources);
        const jda_recode_job J = { form[i], ri[i], 0, 0 };
        jobs[(size_t)i] = J;
        dst_bytes[i] = 0;
    }
    jda_recode_plan_out plan;
    if (rc == JDA_SUCCESS) rc = jda_recode_plan_jobs_ex(n, hosts.data(), jobs.data(), xforms, dst, cap, status, &plan);
    int out = rc;
    if (info) for (int k = 0; k < 6; k++) info[k] = 0;
    if (rc == JDA_SUCCESS && !plan.src.empty()) {
        R.P = plan.P.B;
        if (R.P.hdr.empty()) R.P.hdr.push_back(0);
        setup(R, 0u);
        for (const Alloc &a : sources.allocs) R.io.allocs.push_back(a);
        const size_t nj = plan.src.size(), nb = R.P.n_blocks;
        const bool xf = !plan.xf.empty();
        if (xf && plan.xf.size() != nj) return -60;
        std::vector<uint8_t> src_mem, bad_mem, slot_mem, xf_mem;
        jda_rc_src *d_src = place<jda_rc_src>(src_mem, plan.src.data(), nj * sizeof(jda_rc_src), nj * sizeof(jda_rc_src));
        jda_rc_xf *d_xf = place<jda_rc_xf>(xf_mem, plan.xf.data(), plan.xf.size() * sizeof(jda_rc_xf), nj * sizeof(jda_rc_xf));
        uint32_t *d_bad = aligned<uint32_t>(bad_mem, nj * 4);
        R.io.add(d_src, nj * sizeof(jda_rc_src), false, false);
        if (xf) R.io.add(d_xf, nj * sizeof(jda_rc_xf), false, false);
        R.io.add(d_bad, nj * 4, true, false, true);
        uint8_t *slots = aligned<uint8_t>(slot_mem, (size_t)JDA_EN_THREADS * JDA_COEF_STRIDE);
        OnceIO io;
        static_cast<SimIO &>(io) = R.io;
        if (plan.any_image) {
            for (uint32_t first = 0; first < nb; first += JDA_EN_THREADS) {
                memset(slots, 0xEE, (size_t)JDA_EN_THREADS * JDA_COEF_STRIDE);
                for (uint32_t tid = 0; tid < JDA_EN_THREADS; tid++) {
                    const uint32_t b = first + tid;
                    uint8_t *slot = slots + tid * JDA_COEF_STRIDE;
                    uint32_t tag = 0;
                    if (b < nb) {
                        const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
                        if (b < R.jobs[j].block0 || b >= R.jobs[j].block0 + R.jobs[j].n_blocks) return -50;
                        if (io.ld32(&d_src[j].kind) == JDA_RC_IMAGE) {
                            if (xf) {
                                if (!io.rd(&d_xf[j], sizeof(jda_rc_xf))) return -61;
                                tag = 1u + jda_rc_extract_block_xf(R.A, R.jobs[j], d_src[j], d_xf[j], j, b, slot, d_bad, io);
                                if (tag - 1u < R.jobs[j].block0 || tag - 1u >= R.jobs[j].block0 + R.jobs[j].n_blocks) return -62;      // a block lands in its own job
                            } else { jda_rc_extract_block(R.A, R.jobs[j], d_src[j], j, b, slot, d_bad, io); tag = 1; }
                        }
                    }
                    memcpy(slot + JDA_RC_SLOT_VALID, &tag, 4);
                }
                for (uint32_t wave = 0; wave < JDA_EN_THREADS / 64u; wave++)
                    for (uint32_t lane = 64u; lane-- > 0u;) {
                        if (xf) jda_rc_store_xf(R.A, slots + wave * 64u * JDA_COEF_STRIDE, lane, io);
                        else jda_rc_store(R.A, first + wave * 64u, slots + wave * 64u * JDA_COEF_STRIDE, lane, io);
                    }
            }
            if (info) info[xf ? 4 : 2] = 1;
        }
        if (plan.any_coef) {
            for (uint32_t b = nb; b-- > 0u;) {
                const uint32_t j = jda_en_find_block(R.A.jobs, R.A.n_jobs, b, io);
                if (io.ld32(&d_src[j].kind) != JDA_RC_COEF) continue;
                if (xf) jda_rc_coef_block_xf(R.A, R.jobs[j], d_src[j], d_xf[j], j, b, d_bad, io);
                else jda_rc_coef_block(R.A, R.jobs[j], d_src[j], j, b, d_bad, io);
            }
            if (info) info[xf ? 5 : 3] = 1;
        }
        if (io.err) return io.err;
        R.io = static_cast<SimIO &>(io);
        for (size_t k = 0; k < nb * 128; k++) if (!R.io.allocs[3].init[k]) return -71;      // (3 = coef, 4 = meta: setup()'s order)
        for (size_t k = 0; k < nb * 4; k++) if (!R.io.allocs[4].init[k]) return -71;
        if (coef) memcpy(coef, R.A.coef, nb * 128);
        if (meta) memcpy(meta, R.A.meta, nb * 4);
        for (int i = 0; i < n; i++) bad[i] = 0;
        for (size_t k = 0; k < nj; k++) {
            bad[plan.job_of[k]] = d_bad[k];
            if (d_bad[k]) { status[plan.job_of[k]] = JDA_UNSUPPORTED_FEATURE; R.P.jobs[k].capacity = 0; R.jobs[k].capacity = 0; }
        }
        if (info) { info[0] = nb; info[1] = nj; }
        std::vector<int64_t> fb(nj);
        std::vector<int32_t> st(nj);
        std::vector<uint8_t> headers;
        if (!plan.progressive && R.P.n_opt == 0) {
            out = finish(R, fb.data(), st.data(), NULL, NULL, NULL, NULL, 0);
            headers = R.P.hdr;
        } else {
            LaterIO later;
            static_cast<SimIO &>(later) = R.io;
            later.once_base = NULL; later.once_size = 0;
            if (plan.progressive) out = finish_progressive(R, plan.P, later, fb.data(), st.data(), &headers);
            else { out = finish_optimised(R, later, fb.data(), st.data()); headers = R.P.hdr; }
        }
        if (out == 0)
            for (size_t k = 0; k < nj; k++) {
                const int i = plan.job_of[k];
                if (d_bad[k]) continue;
                dst_bytes[i] = fb[k]; status[i] = st[k];
            }
        if (hdr_len) *hdr_len = (int64_t)headers.size();
        if (hdr && (int64_t)headers.size() <= hdr_cap && !headers.empty()) memcpy(hdr, headers.data(), headers.size());
    }
    for (Source &s : S) { if (s.img) jda_image_free(s.img); if (s.cimg) jda_coef_image_free(s.cimg); }
    return out;
}

// the plan's own answers: the shape of the file a job writes, and the bound of its size
extern "C" int recodexfsim_geometry(const jda_image_info *info, const jda_recode_xform *x, jda_image_info *out) { return jda_recode_geometry_of(info, x, out); }
extern "C" int recodexfsim_bound(const jda_image_info *info, const jda_recode_xform *x, int form, int ri, int64_t *bytes) { return jda_recode_bound_bytes_ex(info, x, form, ri, bytes); }
