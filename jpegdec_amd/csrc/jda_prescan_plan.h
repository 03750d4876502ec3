// jda_prescan_plan.h -- HOST: what a launch of the device pre-scan (jda_segscan_* in jda_kernels.hip, jda_seg_walk in jda_device_core.h)
// asks of its caller: the bytes of every per-image array, which scans are admitted, the fields of jda_segscan_params that follow from
// the image alone, and what the result words say.  No HIP in here and no allocation: jda_upload_batch (jda_runtime.cpp), the streamed
// pipeline (jda_pipeline.cpp) and the CPU emulator (tests/hostsim/hostsim.cpp) lay the arrays out each in its own order, and all three
// size them, fill the parameters and read the verdict here.
#ifndef JDA_PRESCAN_PLAN_H
#define JDA_PRESCAN_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "jda_device_core.h"

static inline size_t jda_a16(size_t v) { return (v + 15) & ~(size_t)15; }

// Bytes of the arrays of one image, each rounded up to 16 (what they hold: jda_segscan_params).  len: the caller's bound of the
// filtered scan's length (jda_upload_batch has the filtered scan; the pipeline has the unfiltered one, which is no shorter);
// n_intervals: restart intervals, 0 for a stream without DRI; rec_cap: jda_record_cap of the image's tables.
struct jda_prescan_sizes {
    uint32_t n_segs, cand_cap;       // segments of JDA_SEG_BYTES (the last one may be empty); candidates the list holds
    size_t scan;                     // the scan, zero padded: whole segments + 16 bytes (a lane reads 12 bytes of the next), JDA_SCAN_PAD at least
    size_t entry;                    // n_segs + 1 entry states (zeroed)
    size_t seg_sum, seg_start;       // JDA_SEG_SUM_WORDS / JDA_SEG_START_WORDS words per segment
    size_t worklist;                 // two lists of n_segs segment numbers
    size_t restart_pos;              // n_intervals positions + the sentinel; 0 without intervals
    size_t rst_events;               // two words per interval (zeroed); 0 without intervals
    size_t records;                  // rec_cap slots per segment
    size_t cands;                    // cand_cap candidates of 16 bytes
};
static inline jda_prescan_sizes jda_prescan_sizes_of(uint32_t len, uint32_t n_intervals, uint32_t rec_cap)
{
    jda_prescan_sizes S;
    const size_t n = S.n_segs = len / JDA_SEG_BYTES + 1u;
    S.scan = jda_a16(std::max((size_t)len + JDA_SCAN_PAD, n * JDA_SEG_BYTES + 16));
    S.entry = jda_a16((n + 1) * 4);
    S.seg_sum = jda_a16(n * 4 * JDA_SEG_SUM_WORDS);
    S.seg_start = jda_a16(n * 4 * JDA_SEG_START_WORDS);
    S.worklist = jda_a16(n * 8);
    S.restart_pos = n_intervals ? jda_a16(((size_t)n_intervals + 1) * 4) : 0;
    S.rst_events = n_intervals ? jda_a16((size_t)n_intervals * 8) : 0;
    S.cand_cap = std::max<uint32_t>(1024u, S.n_segs * 16u);      // (a high-quality photograph: five candidates per segment, most of them of walks that were redone)
    S.records = jda_a16(n * rec_cap * 4);
    S.cands = (size_t)S.cand_cap * 16;
    return S;
}

// The block records are rec_cap slots per 256-byte segment: 6 x the scan with the usual tables, up to 16 x with a DHT whose shortest
// codes are one or two bits.  Past 8 x (+ 16 MB of grace) the image takes the serial host pre-scan: a batch of such files must not ask
// for an arena several times what the same files needed before the records existed.
static inline bool jda_prescan_admits(uint32_t len, uint32_t rec_cap)
{
    return (uint64_t)(len / JDA_SEG_BYTES + 1u) * rec_cap * 4u <= 8ull * len + (16ull << 20);
}

// The fields of P that are a function of the image alone.  The pointers, walk_tables_shared and filter_result stay with the caller.
static inline void jda_prescan_fill_geometry(jda_segscan_params &P, const jda_image_info &I, const uint8_t *dc_id, const uint8_t *ac_id,
                                             uint32_t len, uint32_t n_segs, uint32_t n_intervals)
{
    P.scan_len = len; P.n_segs = n_segs; P.n_blocks_total = (uint32_t)((size_t)I.mcus_x * I.mcus_y * I.blocks_per_mcu);
    P.nblocks = (uint8_t)I.blocks_per_mcu; P.nluma = (uint8_t)(I.blocks_per_mcu - (I.ncomp == 3 ? 2 : 0));
    for (int c = 0; c < 3; c++) { P.dc_id[c] = dc_id[c]; P.ac_id[c] = ac_id[c]; }
    if (n_intervals) {
        P.n_intervals = n_intervals;
        P.interval_blocks = (uint32_t)I.restart_interval * (uint32_t)I.blocks_per_mcu;
        P.round_last = ((uint32_t)(I.mcus_x * I.mcus_y) % (uint32_t)I.restart_interval) == 0 ? 1u : 0u;
    }
}

// Rounds that had something to walk: rounds 0 and 1 walk every segment, round r >= 2 the list whose length lies at JDA_ST_ROUND0 + r.
static inline int jda_prescan_rounds_used(const uint32_t *stats)
{
    int r = 2;
    while (r <= (int)JDA_PRESCAN_MAX_ROUND + 1 && stats[JDA_ST_ROUND0 + r]) r++;
    return r;
}

// May the device's index be adopted?  The last round left nothing to walk; enough blocks and no bad code before the end; the closing
// entry written once; every marker where the MCU count puts it; the states-first order's recording round (round JDA_PRESCAN_MAX_ROUND)
// found every exit state as the SPEC rounds had left it.  Anything else -- a corrupt or truncated stream, states that did not settle --
// goes to the serial host pre-scan, which reproduces what the reference does with such a stream.
// The last two hold by themselves where a caller's passes cannot break them (jda_kernels.hip): JDA_ST_RST_MISMATCH is written by
// jda_segscan_resolve_cands alone and under `if (P.restart_pos)` only, so it stays 0 for a stream without intervals; the list length
// of round r + 1 is written by round r (jda_fused_item), and without states_first jda_segscan_tail stops before round
// JDA_PRESCAN_MAX_ROUND (the pipeline's max_round is no larger: a static_assert there), so the word behind that round's stays 0.
// filter_result: the device filter's {length, markers} where it ran (the pipeline), else NULL -- the host filter placed the markers.
// A stream with intervals must then have shown the filter as many markers as the MCU count asks for (jda_segscan_resolve: nothing
// walks otherwise).
static inline bool jda_prescan_verdict(const uint32_t *stats, const uint32_t *filter_result, uint32_t n_intervals)
{
    if (filter_result && n_intervals && filter_result[1] + 1u != n_intervals) return false;
    return stats[JDA_ST_SETTLED] == 1 && stats[JDA_ST_INDEX_OK] == 1 && stats[JDA_ST_BAD] == 0 && stats[JDA_ST_TERMINAL] == 1 &&
           stats[JDA_ST_RST_MISMATCH] == 0 && stats[JDA_ST_ROUND0 + JDA_PRESCAN_MAX_ROUND + 1u] == 0;
}

#endif
