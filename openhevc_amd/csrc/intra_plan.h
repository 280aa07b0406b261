/*
 * intra_plan.h — what the intra pass of a batch decides before it launches (engine.hip: intra_pass), as functions of plain values:
 * which form a picture takes, and the staged form's launch — waves, phases, whether the residual spans are staged, and the carve-up
 * of the dynamic LDS block that intra.hip's intra_ctu_body follows without a check of its own.  Pure host code: no HIP runtime
 * call, no engine, no allocation — tests/intra_plan_check.cpp runs all of it on the CPU.
 */
#ifndef OHEVC_INTRA_PLAN_H
#define OHEVC_INTRA_PLAN_H

#include "dev_frame.h"
#include "engine_tuning.h"
#include "handover_layout.h"            /* align_up */

/* The two forms (intra.hip), one launch each:
 *   direct  a wave per CTU working on the picture in HBM — pictures whose intra blocks cover less than half of their samples
 *           (B / P pictures);
 *   dag     a workgroup per CTU with the CTU staged in LDS — the others (I pictures).
 * intra_area64: the samples of the picture's intra blocks / 64, all planes (DevSummary) */
static inline bool intra_plan_direct(const OhPicParams *p, uint32_t intra_area64, const OhTuning &t)
{
    if (t.intra_mode != OH_INTRA_AUTO)
        return t.intra_mode == OH_INTRA_DIRECT;
    const uint64_t pic_samples64 = ((uint64_t)p->width * p->height * (p->chroma_format_idc == 0 ? 2 : p->chroma_format_idc == 1 ? 3 : p->chroma_format_idc == 2 ? 4 : 6) / 2) >> 6;
    return (uint64_t)intra_area64 * 2 < pic_samples64;
}

/* what intra_pass gathers over the pictures of a batch that take the staged form */
struct OhIntraFigures {
    int      batch = 0;                                /* pictures of the batch, of either form */
    uint32_t max_items = 1, max_sub = 1, max_res = 0;  /* over their schedule entries: blocks, sub-levels, int16 of the residual span */
    uint64_t sum_items = 0, sum_sub = 0, total_entries = 0;
    bool     contiguous = true;                        /* no entry's residual span is scattered over the pool */
};

static inline OhIntraLaunch intra_plan_launch(int log2_ctb_size, int chroma_format_idc, const OhIntraFigures &f, int n_cu, const OhTuning &t)
{
    OhIntraLaunch L;
    /* the CTUs' residual spans staged in LDS, or every block fetching its own from the pool one sub-level ahead (intra.hip:
     * slots_prepare)?  Staging costs ~11 KB of LDS per workgroup in a launch that holds one all-intra CTU.  A launch of at most a
     * workgroup per CU is latency-bound: stage (a 4K I picture alone 6.6 ms against 7.0); any wider one runs at workgroups-per-CU x
     * latency: keep the LDS small (all-intra batches 39.8 against 37.6 Gpix/s, the mixed bench +0.6 %) */
    L.staged = f.contiguous && (t.intra_res_lds >= 0 ? t.intra_res_lds != 0 : f.total_entries / 8 <= (uint64_t)n_cu);
    /* waves per CTU: as many as blocks run side by side in a sub-level (more only hold LDS and wave slots); a small batch cannot
     * fill the chip anyway: spend the waves on the single picture's latency */
    const double par = f.sum_sub ? (double)f.sum_items / (double)f.sum_sub : 1.0;
    L.waves = t.intra_waves ? t.intra_waves : par > (f.batch < 8 ? 2.5 : 4.5) ? 8 : par > 1.25 ? 4 : 2;
    /* sub-levels go round-robin to `phases` groups of waves (intra.hip): a group prepares its next sub-level while another
     * finishes its own, so at least two */
    L.phases = t.intra_phases;
    if (L.phases < 2 || L.phases > L.waves || L.waves % L.phases) L.phases = 2;
    const OhCtuAreas areas = oh_ctu_areas(log2_ctb_size, chroma_format_idc);
    size_t off = align_up((size_t)areas.total * sizeof(uint16_t), 16);
    L.off_items = (uint32_t)off; off += (size_t)f.max_items * sizeof(DevIntra);
    L.off_sub = (uint32_t)off;   off += ((size_t)f.max_sub + 1) * sizeof(uint32_t);
    L.off_small = (uint32_t)off; off = align_up(off + (size_t)f.max_sub * sizeof(uint32_t), 16);
    L.off_res = (uint32_t)off;   off = align_up(off + (size_t)(L.staged ? f.max_res : 0) * sizeof(int16_t), 16);
    L.off_wave = (uint32_t)off;  off += (size_t)L.waves * OH_INTRA_WAVE_LDS;
    L.lds_bytes = (uint32_t)off;                       /* <= OH_INTRA_MAX_LDS for everything the preparation lets through */
    return L;
}

#endif
