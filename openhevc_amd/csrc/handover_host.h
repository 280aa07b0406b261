/*
 * handover_host.h — the host work of the hand-over that more than one thread does: the check-and-count of one work list
 * (handover_check_list) and the pool of helper threads that shares it, and the staging copy behind it, with the calling thread
 * (CopyPool).  Pure host code like handover_layout.h: no HIP runtime call, no engine — tests/handover_parallel_check.cpp runs all of
 * it on the CPU under AddressSanitizer, UBSan and ThreadSanitizer.
 *
 * The order of events in a chunk (engine_handover.hip: upload_chunk), n lists, one submitting thread and its h helpers:
 *   1. the submitter alone: parameters, the current picture and the mask of usable reference slots of every list (engine state);
 *   2. handover_check_chunk: submitter and min(h, n - 1) helpers CLAIM lists from a shared cursor, one thread per list; every list
 *      gets its HostSide, its PU block offsets and its error slot; the submitter reports the failing list of lowest index;
 *   3. the submitter alone: layouts, arena, headers, staging buffer;
 *   4. CopyPool::run over the copy jobs of a group: the pieces are CLAIMED from a cursor in the same way;
 *   5. the submitter alone: everything that is enqueued.
 * A helper sees nothing of the engine: no error string, no timer, no HIP call.
 */
#ifndef OHEVC_HANDOVER_HOST_H
#define OHEVC_HANDOVER_HOST_H

#include <stdarg.h>
#include <stdio.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/ohevc_hip.h"
#include "handover_layout.h"

/* what the check of one list leaves: OH_OK, or the code and the message the engine reports */
struct HandoverCheck { int rc; char msg[200]; };

static inline int hc_fail(HandoverCheck *r, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
static inline int hc_fail(HandoverCheck *r, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r->msg, sizeof(r->msg), fmt, ap);
    va_end(ap);
    return r->rc = code;
}

/* The host's check and count of one work list: what sizes the device arena — blocks per PU, transform blocks per size: two light
 * loops over arrays nobody has touched since they were recorded — and the few consistency rules the preparation kernels rely on
 * (everything else is validated on the GPU).  ref_ok: bit i set when slot i of f->ref_pics holds a picture of this geometry other
 * than the current one; the caller knows the pictures, this function only the list.  Touches nothing but its arguments. */
static inline int handover_check_list(const OhFrame *f, uint32_t ref_ok, HostSide *h, std::vector<uint32_t> &pu_off, HandoverCheck *r)
{
    const OhPicParams &p = f->p;
    r->rc = OH_OK; r->msg[0] = 0;
    h->ref_ok = ref_ok; h->ref_used = 0; h->n_cross = 0; h->any_dense = false;
    if ((f->n_pu && !f->pu) || (f->n_wp && !f->wp) || (f->n_tu && !f->tu) || (f->n_intra && !f->intra))
        return hc_fail(r, OH_E_ARG, "a non-zero item count comes with a NULL array (pu / wp / tu / intra)");
    /* blocks per PU: sizes the MC block lists (prep_pu_scan repeats the sums on the GPU and validates every PU) */
    uint64_t nl = 0, nc = 0;
    const int hs = oh_hshift(&p, 1), vs = oh_vshift(&p, 1), two = p.chroma_format_idc ? 2 : 0;
    if ((uint64_t)f->n_pu * 2048 >= (1ull << 31))
        return hc_fail(r, OH_E_ARG, "PU list too long");
    pu_off.resize(2 * ((size_t)f->n_pu + 1));
    uint32_t *ol = pu_off.data(), *oc = ol + f->n_pu + 1;       /* running sums: where every PU's blocks start in the two lists */
    h->pu_off = ol;
    uint32_t ref_used = 0;
    for (uint32_t i = 0; i < f->n_pu; i++) {
        const OhPu &pu = f->pu[i];
        ol[i] = (uint32_t)nl; oc[i] = (uint32_t)nc;
        nl += (uint64_t)(((pu.w + 7) >> 3) * ((pu.h + 7) >> 3));
        nc += (uint64_t)(two * ((((pu.w >> hs) + 7) >> 3) * (((pu.h >> vs) + 7) >> 3)));
        for (int l = 0; l < 2; l++)
            if (pu.ref[l] < OH_MAX_REFS) ref_used |= 1u << pu.ref[l];
    }
    h->ref_used = (uint16_t)ref_used;
    ol[f->n_pu] = (uint32_t)nl; oc[f->n_pu] = (uint32_t)nc;
    for (uint32_t i = 0; i < f->n_wp; i++)
        if (f->wp[i].log2_denom[0] > 7 || f->wp[i].log2_denom[1] > 7)
            return hc_fail(r, OH_E_ARG, "weights %u: log2 denominator out of range", i);
    uint32_t tu_cnt[4] = { 0, 0, 0, 0 }, n_cross = 0, all_flags = OH_TUF_SPARSE;
    for (uint32_t i = 0; i < f->n_tu; i++) {                  /* launch sizes of the residual pass; is any block dense? */
        const OhTu &t = f->tu[i];
        tu_cnt[(t.log2_size - 2) & 3]++;
        n_cross += (t.flags & OH_TUF_CROSS) != 0;
        all_flags &= t.flags;
    }
    for (int k = 0; k < 4; k++) h->tu_cnt[k] = tu_cnt[k];
    h->n_cross = n_cross;
    h->any_dense = f->n_tu && !(all_flags & OH_TUF_SPARSE);
    if (h->any_dense && f->n_coeff && !f->coeffs)
        return hc_fail(r, OH_E_ARG, "dense transform blocks but coeffs[] is NULL");
    if (h->n_cross && !f->tu_cross)
        return hc_fail(r, OH_E_ARG, "cross-component blocks without tu_cross[]");
    if (f->n_intra && p.constrained_intra_pred && !f->is_intra)
        return hc_fail(r, OH_E_ARG, "constrained_intra_pred without the is_intra map");
    if (f->n_intra) {
        /* the level table is the contract behind the waits between CTUs (prep_intra_wait: a CTU waits only for lower levels), and
         * prep_intra_ctu looks every entry's level up in it: checked here; everything below it on the GPU */
        if (!f->level_start || !f->n_levels || !f->ictu || !f->n_ictu || !f->sub_start || !f->n_sub ||
            f->level_start[0] != 0 || f->level_start[f->n_levels] != f->n_ictu)
            return hc_fail(r, OH_E_ARG, "intra wavefront tables inconsistent");
        for (uint32_t l = 0; l < f->n_levels; l++)
            if (f->level_start[l] > f->level_start[l + 1])
                return hc_fail(r, OH_E_ARG, "intra level table not monotonic");
    }
    if (p.deblock_enabled) {
        const OhBsInputs *bi = f->bs_in;                      /* boundary strengths derived on the GPU instead of handed over */
        if (bi && (!bi->mvf || !bi->cbf_luma || !bi->call_log2 || !bi->ctb_flags))
            return hc_fail(r, OH_E_ARG, "bs_in: all four maps are required");
        if (bi && (p.log2_min_pu_size < 2 || p.log2_min_tb_size < 2))
            return hc_fail(r, OH_E_ARG, "bs_in: min PU / TB size below 4");
        if (bi) {
            const size_t n_cells = (size_t)(p.width >> p.log2_min_tb_size) * (p.height >> p.log2_min_tb_size);
            for (size_t i = 0; i < n_cells; i++)
                if (bi->call_log2[i] && (bi->call_log2[i] < p.log2_min_tb_size || bi->call_log2[i] > p.log2_ctb_size))
                    return hc_fail(r, OH_E_ARG, "bs_in: call_log2[%zu] = %d is not a block size of this picture", i, bi->call_log2[i]);
        }
        if ((!bi && (!f->vertical_bs || !f->horizontal_bs || f->bs_size < oh_bs_size(&p))) || !f->qp_y_tab || !f->deblock)
            return hc_fail(r, OH_E_ARG, "deblock side arrays missing or too small");
    }
    if ((p.pcm_loop_filter_disable || p.transquant_bypass_enable) && !f->is_pcm)
        return hc_fail(r, OH_E_ARG, "is_pcm map required when pcm loop-filter disable / transquant bypass is on");
    OhPrepCounts *cnt = &h->cnt;
    cnt->n_pu = f->n_pu; cnt->n_mc_luma = (uint32_t)nl; cnt->n_mc_chroma = (uint32_t)nc; cnt->n_tu = f->n_tu;
    cnt->n_intra = f->n_intra; cnt->n_sub = f->n_intra ? f->n_sub : 0; cnt->n_ictu = f->n_intra ? f->n_ictu : 0;
    return OH_OK;
}

/* The helper threads of one engine's hand-over, and of its output fetch: run(n, fn) calls fn(i) once for every i in [0, n) and
 * returns when all calls have returned.  The items are CLAIMED, not dealt: the calling thread and the helpers that have woken up take
 * the next index from one atomic cursor, so a thread that loses its CPU delays the item it holds and nothing else, and a helper that
 * has not woken up by the time the last item is taken is not waited for at all.  One run at a time (an engine has one submitter). */
struct CopyPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv, done_cv;
    /* the run in progress; written and read under mu, but for the cursor */
    void (*call)(void *ctx, size_t i) = nullptr;
    void *ctx = nullptr;
    size_t n_items = 0;
    std::atomic<size_t> next{ 0 };
    uint64_t gen = 0;
    bool open = false;               /* helpers may still join the run */
    int joined = 0, finished = 0;
    bool stop = false;

    void worker()
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return stop || (open && gen != seen); });
            if (stop) return;
            seen = gen;
            joined++;
            void (*const c)(void *, size_t) = call;
            void *const x = ctx;
            const size_t n = n_items;
            lk.unlock();
            for (size_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < n; )
                c(x, i);
            lk.lock();
            if (++finished == joined && !open) done_cv.notify_one();
        }
    }
    void start(int n) { for (int k = 0; k < n; k++) th.emplace_back(&CopyPool::worker, this); }
    int helpers() const { return (int)th.size(); }

    /* fn(i) for every i in [0, n), on the calling thread and at most max_helpers helpers (fewer items than threads wake fewer) */
    template <class Fn> void run(size_t n, Fn &&fn, int max_helpers = 1 << 30)
    {
        const size_t k = std::min({ th.size(), (size_t)std::max(max_helpers, 0), n ? n - 1 : 0 });
        if (!k) {                                              /* no helpers, or one item: the same loop, one thread */
            for (size_t i = 0; i < n; i++) fn(i);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            ctx = (void *)&fn;
            call = [](void *x, size_t i) { (*(typename std::remove_reference<Fn>::type *)x)(i); };
            n_items = n;
            next.store(0, std::memory_order_relaxed);
            joined = finished = 0;
            open = true; gen++;
        }
        if (k == th.size()) cv.notify_all();
        else for (size_t i = 0; i < k; i++) cv.notify_one();
        for (size_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < n; )
            fn(i);
        std::unique_lock<std::mutex> lk(mu);
        open = false;                                          /* who has not joined by now stays asleep */
        done_cv.wait(lk, [&] { return finished == joined; });
    }
    static void copy_one(const CopyJob &j)
    {
        if (j.pack) pack_bs((uint8_t *)j.dst, (const uint8_t *)j.src, j.n);
        else memcpy(j.dst, j.src, j.n);
    }
    void run(const std::vector<CopyJob> &jobs)                 /* returns when every job has been copied */
    {
        const CopyJob *j = jobs.data();
        run(jobs.size(), [j](size_t i) { copy_one(j[i]); });
    }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
};

/* The check-and-count phase of a chunk: list i of fs[0 .. n) into h[i], pu_off[i] and res[i], every list by exactly one thread of
 * the pool (at most n - 1 helpers are woken; one list is the caller's own).  Returns the index of the failing list with the lowest
 * index — the one a loop over the lists in order would have stopped at — or -1. */
static inline int handover_check_chunk(CopyPool *pool, const OhFrame *const *fs, const uint32_t *ref_ok, int n, HostSide *h,
                                       std::vector<uint32_t> *pu_off, HandoverCheck *res)
{
    auto one = [=](size_t i) { (void)handover_check_list(fs[i], ref_ok[i], &h[i], pu_off[i], &res[i]); };
    if (pool) pool->run((size_t)n, one);
    else for (int i = 0; i < n; i++) one((size_t)i);
    for (int i = 0; i < n; i++)
        if (res[i].rc != OH_OK)
            return i;
    return -1;
}

#endif
