// tests/hostsim/resize_filters_sim.cpp -- TEST INFRASTRUCTURE: the resize kernels' schedule on the CPU for Pillow's five filters.
//
// resize_sim.cpp (included for its IO policy, which holds every access to what the kernel promises: DESIGN.md 5.12) runs the unsigned
// instances over the triangle's tables; this file runs the plan of jda_resize_surfaces_ex for any filter and the instance the runtime would
// launch for it -- jda_rs_horizontal / jda_rs_vertical <BPP, false> for BILINEAR, BOX and HAMMING, <BPP, true> for BICUBIC and LANCZOS --
// lane by lane, the horizontal pass of all lanes before the vertical pass of any.  resizefsim_taps gives the host's table of one axis,
// resizefsim_guard the guard's answer on a table the caller made, resizefsim_check the argument checks without a GPU.
#include "resize_sim.cpp"

namespace {
template <int BPP, bool SIGNED> int run_filter(SimIO &io, const jda_resize_job &J, uint32_t n_tiles)
{
    jda_rs_geo G;
    G.src = J.src; G.dst = J.dst; G.src_pitch = J.src_pitch; G.dst_pitch = J.dst_pitch; G.out_w = J.out_w; G.out_h = J.out_h;
    G.htab = J.htab; G.vtab = J.vtab; G.hk = J.hk; G.vk = J.vk; G.th = J.th;
    for (uint32_t tile = 0; tile < n_tiles; tile++) {
        const uint32_t ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
        std::fill(io.lds_set.begin(), io.lds_set.end(), 0);      // a workgroup finds nothing in LDS
        uint32_t oy0, row0, span;
        io.tile_row0 = 0; io.tile_span = 0;
        jda_rs_tile_rows(G, ty, io, oy0, row0, span);
        if (span == 0u || span > JDA_RS_LDS_ROWS || span * JDA_RS_TILE_DWORDS > io.lds.size()) return -41;
        io.tile_row0 = row0; io.tile_span = span;
        for (uint32_t tid = 0; tid < JDA_RS_THREADS; tid++) jda_rs_horizontal<BPP, SIGNED>(G, tx, row0, span, tid, io);
        for (uint32_t tid = 0; tid < JDA_RS_THREADS; tid++) jda_rs_vertical<BPP, SIGNED>(G, tx, oy0, row0, tid, io);
    }
    return io.err;
}
}

// the host's table of one axis for a filter (the layout: resizesim_taps); returns ksize, or minus the status the plan gives (the guard's
// among them), or -100 when cap (dwords) is too small
extern "C" int resizefsim_taps(int filter, int in_size, int in0, int in1, int out_size, int32_t *out, int cap)
{
    uint32_t ksize;
    int rc = jda_resize_axis_ksize(in0, in1, out_size, &ksize, filter);
    if (rc != JDA_SUCCESS) return -rc;
    if ((int64_t)out_size * (2 + (int64_t)ksize) > cap) return -100;
    rc = jda_resize_axis_taps(in_size, in0, in1, out_size, ksize, out, filter);
    return rc != JDA_SUCCESS ? -rc : (int)ksize;
}

// the triangle's table through the entry the code had before the filters: the defaults of the same functions
extern "C" int resizefsim_taps_old(int in_size, int in0, int in1, int out_size, int32_t *out, int cap)
{
    return resizesim_taps(in_size, in0, in1, out_size, out, cap);
}

// the guard on a table of the caller's (the layout of an axis table): the status jda_resize_axis_taps would give for it
extern "C" int resizefsim_guard(int filter, const int32_t *tab, int out_size, int ksize)
{
    return jda_resize_axis_guard(filter, tab, out_size, (uint32_t)ksize);
}

// as resizesim_lanes, for a filter.  info (may be NULL): {tiles, tile rows, lds bytes, horizontal ksize, vertical ksize, signed instance}
extern "C" int resizefsim_lanes(int filter, const uint8_t *src, int pitch, int width_px, int rows, int bpp, int x, int y, int w, int h, uint8_t *dst,
                                int dst_pitch, int out_w, int out_h, uint32_t *info)
{
    jda_output S, D;
    S.pixels = (void *)src; S.pitch_bytes = pitch; S.width_px = width_px; S.rows = rows;
    D.pixels = dst; D.pitch_bytes = dst_pitch; D.width_px = out_w; D.rows = out_h;
    const int32_t rect[4] = { x, y, w, h };
    jda_resize_plan_out plan;
    const int rc = jda_resize_plan_jobs(1, &S, bpp, rect, &D, &plan, filter);
    if (rc != JDA_SUCCESS) return rc;
    const jda_resize_job &J = plan.jobs[0];
    const bool sgn = jda_resize_filter_signed(filter);
    if (info) { info[0] = plan.n_tiles; info[1] = J.th; info[2] = plan.lds_bytes; info[3] = J.hk; info[4] = J.vk; info[5] = sgn ? 1u : 0u; }
    if (J.th == 0u || J.th > JDA_RS_TILE_ROWS || plan.n_tiles != J.tiles_x * ((J.out_h + J.th - 1u) / J.th)) return -42;
    SimIO io;
    io.src = src; io.src_pitch = (uint32_t)pitch; io.src_rows = (uint32_t)rows; io.bpp = (uint32_t)bpp;
    memcpy(io.rd, plan.reads.data(), sizeof(io.rd));
    io.tables = plan.tables.data();
    io.htab0 = J.htab; io.htab1 = J.htab + J.out_w * (2u + J.hk); io.vtab0 = J.vtab; io.vtab1 = J.vtab + J.out_h * (2u + J.vk);
    if (io.htab1 > plan.tables.size() || io.vtab1 > plan.tables.size()) return -43;
    io.dst = dst; io.dst_pitch = (uint32_t)dst_pitch; io.out_w = J.out_w; io.out_h = J.out_h;
    io.written.assign((size_t)J.out_h * J.out_w * (uint32_t)bpp, 0);
    io.lds.assign(plan.lds_bytes / 4u, 0xEEEEEEEEu); io.lds_set.assign(io.lds.size(), 0);
    io.err = 0;
    const int e = sgn ? (bpp == 4 ? run_filter<4, true>(io, J, plan.n_tiles) : run_filter<1, true>(io, J, plan.n_tiles))
                      : (bpp == 4 ? run_filter<4, false>(io, J, plan.n_tiles) : run_filter<1, false>(io, J, plan.n_tiles));
    if (e) return e;
    for (uint8_t b : io.written) if (!b) return -24;
    return 0;
}

// as resizesim_check, for a filter.  info (may be NULL): {tiles, lds bytes, table bytes, then the first job's source pixels {x0, y0, x1, y1}}
extern "C" int resizefsim_check(int filter, int n, const jda_output *src, int bpp, const int32_t *rects, const jda_output *dst, const void *tables_at, uint32_t *info)
{
    jda_resize_plan_out plan;
    int rc = jda_resize_plan_jobs(n, src, bpp, rects, dst, &plan, filter);
    if (rc == JDA_SUCCESS && tables_at) rc = jda_resize_plan_place(&plan, tables_at);
    if (info) {
        info[0] = plan.n_tiles; info[1] = plan.lds_bytes; info[2] = (uint32_t)(plan.tables.size() * 4u);
        for (int i = 0; i < 4; i++) info[3 + i] = rc == JDA_SUCCESS && plan.reads.size() >= 4u ? (uint32_t)plan.reads[(size_t)i] : 0u;
    }
    return rc;
}
