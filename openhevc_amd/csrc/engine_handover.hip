/*
 * engine_handover.hip — hand-over of work lists to the engine, a chunk (the lists of one call, at most OH_MAX_BATCH) at a time:
 * host-side checks and counts, ONE device arena for the chunk (laid out by handover_layout.h, taken from the engine's pool), the
 * headers, the staging copies (one per group of OH_STAGE_GROUP lists) or the pull out of pinned memory, and the preparation kernels
 * behind them on the copy stream.  oh_frames_upload / oh_frame_upload of the C ABI (include/ohevc_hip.h).
 * Order of events for a chunk: (1) parameters, current picture and usable references of every list, on the submitting thread;
 * (2) the lists checked and counted list-parallel by the submitter and the engine's helper threads (handover_host.h), the failing list
 * of lowest index reported; (3) layouts, arena, summary block, headers; (4) per group a staging buffer, the staging copy with its
 * pieces claimed by the same threads, and ONE H2D copy; (5) the preparation launches and `ready`.  Nothing is taken from a pool or
 * enqueued before (2) is through, and no helper touches the caller's arrays once oh_frames_upload has returned.
 */
#include <memory>

#include "engine_impl.h"

hipEvent_t sync_event_get(OhEngine *e)
{
    hipEvent_t ev = nullptr;
    if (!e->sync_events.empty()) { ev = e->sync_events.back(); e->sync_events.pop_back(); return ev; }
    return hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess ? ev : nullptr;
}
void sync_event_put(OhEngine *e, hipEvent_t ev)
{
    if (!ev) return;
    if (e->sync_events.size() < 4096) e->sync_events.push_back(ev); else (void)hipEventDestroy(ev);
}

/* ---------------- device arenas ---------------- */
/* the two places that allocate and free an arena: what oh_engine_memory reports as alive (pooled or holding a work list) is counted here */
static void *arena_new(OhEngine *e, size_t bytes)
{
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess)
        return nullptr;
    e->arenas_alive++; e->arena_bytes_alive += bytes;
    return p;
}
static void arena_delete(OhEngine *e, void *p, size_t bytes)
{
    (void)hipFree(p);
    if (e) { e->arenas_alive--; e->arena_bytes_alive -= bytes; }
}

/* an arena of at least `total` bytes for a chunk: a pooled one that fits (within 2x), else a new one rounded up to 1 MiB */
static int arena_take(OhEngine *e, size_t total, OhChunk *ck)
{
    /* oldest first (the pool is in release order): an arena released long ago has no pass left that reads it, so the copy
     * need not wait for the engine stream; the most recently released one would stall the copy stream behind the passes
     * of the batch that just let go of it */
    int best = -1;
    for (size_t i = 0; i < e->arenas.size() && best < 0; i++)
        if (e->arenas[i].bytes >= total && e->arenas[i].bytes <= 2 * total + (1u << 20))
            best = (int)i;
    if (best >= 0 && e->arenas[best].free_ev && hipEventQuery(e->arenas[best].free_ev) != hipSuccess && e->arenas.size() < 512)
        best = -1;                                      /* even the oldest fit is still in flight: a new arena beats a stall */
    if (best >= 0) {
        ck->arena = e->arenas[best].p; ck->arena_bytes = e->arenas[best].bytes;
        if (e->arenas[best].free_ev) {                  /* released while passes were in flight: the copies must stay behind them */
            (void)hipStreamWaitEvent(e->copy_stream, e->arenas[best].free_ev, 0);
            sync_event_put(e, e->arenas[best].free_ev);
        }
        e->arenas.erase(e->arenas.begin() + best);
        return OH_OK;
    }
    ck->arena_bytes = align_up(total, (size_t)1 << 20);
    if ((ck->arena = arena_new(e, ck->arena_bytes)) == nullptr) {
        (void)hipStreamSynchronize(e->stream);
        for (auto &a : e->arenas) { sync_event_put(e, a.free_ev); arena_delete(e, a.p, a.bytes); }      /* the pool may be what is in the way */
        e->arenas.clear();
        if ((ck->arena = arena_new(e, ck->arena_bytes)) == nullptr)
            FAIL(e, OH_E_NOMEM, "hipMalloc(%zu) for the work lists failed", total);
    }
    return OH_OK;
}

/* the last list of a chunk is gone: event and summary block go back to their pools, the arena to the engine's.  in_flight: kernels
 * enqueued on the engine stream may still read the arena — an event recorded there now (the stream is in order: it covers the lists
 * released earlier as well) tells the copy stream when the next chunk may overwrite it. */
static void chunk_free(OhEngine *e, OhChunk *ck, bool in_flight)
{
    if (e && ck->ready)
        sync_event_put(e, ck->ready);
    if (ck->sum_host) {
        if (e && e->sum_pool.size() < 4096) e->sum_pool.push_back(ck->sum_host);
        else (void)hipHostFree(ck->sum_host);
    }
    if (ck->arena) {
        if (e && e->arenas.size() < 1024) {
            hipEvent_t fe = nullptr;
            if (in_flight && (fe = sync_event_get(e)) != nullptr && hipEventRecord(fe, e->stream) != hipSuccess) {
                sync_event_put(e, fe);
                fe = nullptr;
            }
            if (in_flight && !fe)
                (void)hipStreamSynchronize(e->stream);           /* no event to be had: wait instead */
            e->arenas.push_back({ ck->arena, ck->arena_bytes, fe });
        } else {
            if (in_flight && e) (void)hipStreamSynchronize(e->stream);
            arena_delete(e, ck->arena, ck->arena_bytes);
        }
    }
    delete ck;
}

/* a list lets go of its chunk.  in_flight: passes of THIS list may still be running (oh_frame_release); remembered until the last
 * list of the chunk goes, whichever way that one goes */
void free_dev_frame(OhEngine *e, OhDevFrame *df, bool in_flight)
{
    if (!df)
        return;
    OhChunk *ck = df->chunk;
    delete df;
    if (!ck)
        return;
    ck->in_flight = ck->in_flight || in_flight;
    if (--ck->refs <= 0)
        chunk_free(e, ck, ck->in_flight);
}

/* ---------------- work lists ---------------- */
static bool same_geometry(const OhPicParams &a, const OhPicParams &b)
{
    return a.width == b.width && a.height == b.height && a.bit_depth == b.bit_depth && a.chroma_format_idc == b.chroma_format_idc;
}

/* ---------------------------------------------------------------------------------------------------------------------
 * Hand-over of a work list.  The host copies the RAW lists (include/ohevc_frame.h, exactly as recorded) into one pinned
 * buffer, counts what sizes the device arena — blocks per PU, transform blocks per size: two light loops — and enqueues on the
 * copy stream:   H2D copy  ->  preparation kernels (prep.hip: validation of every index a pass kernel will follow, the
 * <= 8x8 MC block lists, the transform-size buckets, the intra block descriptors, schedule and statistics)  ->
 * boundary strengths from the motion field when the list carries bs_in (bs.hip)  ->  the summary back to pinned memory  ->
 * `ready`.  Nothing of it touches samples, so it overlaps the passes of the pictures before.  A malformed list is
 * reported by the first oh_frame(s)_execute that includes it (OH_E_ARG, before any of its passes is launched).
 * The counting (handover_host.h: handover_check_list) and the staging copy are shared with the engine's helper threads, lists and
 * pieces claimed from a cursor; what knows the engine — pictures, pools, streams, the error string, the timers — stays on the
 * submitting thread.
 * ------------------------------------------------------------------------------------------------------------------- */
/* the engine's helper threads, started with the first hand-over and before anything of it that they share */
static CopyPool *copiers_get(OhEngine *e)
{
    if (!e->copiers) {
        e->copiers = new CopyPool();
        e->copiers->start(e->tuning.copy_threads);
    }
    return e->copiers;
}

/* bit i: slot i of the list's references holds a picture of its geometry that is not the picture being reconstructed */
static uint32_t usable_refs(OhEngine *e, const OhFrame *f, const Pic *cur)
{
    uint32_t ok = 0;
    for (int i = 0; i < OH_MAX_REFS; i++) {
        Pic *r = get_pic(e, f->ref_pics[i]);
        if (r && same_geometry(r->p, f->p) && r != cur)
            ok |= 1u << i;
    }
    return ok;
}

/* pinned block the summaries of one chunk's work lists land in */
static void *summary_block_get(OhEngine *e)
{
    void *p = nullptr;
    if (!e->sum_pool.empty()) { p = e->sum_pool.back(); e->sum_pool.pop_back(); return p; }
    return hipHostMalloc(&p, OH_MAX_BATCH * sizeof(DevSummary), hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

/* everything of the header but summary_host: pictures, pointers into the two parts of the list in its chunk's arena, counts; and which
 * references df was uploaded with */
static void fill_header(OhEngine *e, const OhFrame *f, const Pic *cur, const HostSide &h, const HandoverLayout &L, char *copied_base, char *rest_base,
                        OhDevFrame *df, HandoverHeader *H)
{
    DevFrame &hd = H->d;
    hd.pp = f->p;
    fill_planes(&hd.cur, cur, false);
    fill_planes(&hd.out, cur, f->p.sao_enabled && f->sao);
    for (int i = 0; i < OH_MAX_REFS; i++) {
        Pic *r = get_pic(e, f->ref_pics[i]);
        df->ref_id[i] = -1; df->ref_gen[i] = 0; df->ref_half[i] = 0;
        if (h.ref_ok >> i & 1) {
            fill_planes(&hd.refs[i], r, r->final_b);
            df->ref_id[i] = f->ref_pics[i]; df->ref_gen[i] = r->gen; df->ref_half[i] = r->final_b ? 1 : 0;
        }
    }
    df->ref_used = h.ref_used;
    df->cur_gen = cur->gen;
    handover_bind_split(L, copied_base, rest_base, H);
    hd.coeffs_present = f->coeffs != nullptr;
    hd.err_word = e->kerr; hd.cur_pic_id = f->cur_pic;
    hd.n_pu = f->n_pu; hd.n_mc_luma = h.cnt.n_mc_luma; hd.n_mc_chroma = h.cnt.n_mc_chroma; hd.n_tu = f->n_tu; hd.n_intra = f->n_intra;
    hd.n_ictu = h.cnt.n_ictu; hd.n_sub = h.cnt.n_sub; hd.n_levels = f->n_intra ? f->n_levels : 0; hd.n_wp = f->n_wp; hd.n_sparse = f->sparse ? f->n_sparse : 0;
    hd.ref_ok = h.ref_ok; hd.n_coeff = f->n_coeff;
    hd.n_cross = h.n_cross;
    for (int k = 0, first = 0; k < 4; k++) { hd.tu_first[k] = (uint32_t)first; hd.tu_cnt[k] = h.tu_cnt[k]; first += (int)h.tu_cnt[k]; }
    hd.dbg = e->dbg;
}

/* The two forms of the copy.  A list that lies in pinned memory (OH_FRAME_PINNED) is pulled by the GPU: the segments made here (the
 * header, the PU block offsets) and the table of segments stand in the staging buffer, every other segment is read from the caller's
 * pinned memory where it lies — ONE kernel launch (prep_pull), no host copy of the lists and no DMA request per array (fifteen of
 * those per picture cost the host as much as the copy they replaced). */
enum { PULL_TABLE = 64 };
static_assert(HL_N_SEGS <= PULL_TABLE, "a table entry per copied segment");
static size_t pulled_stage_bytes(const HandoverLayout &L) { return L.own_bytes + PULL_TABLE * sizeof(OhPullSeg); }
static hipError_t stage_pulled(OhEngine *e, const HandoverLayout &L, char *arena, OhEngine::Stage *sg)     /* arena: the list's copied part */
{
    char *sp = (char *)sg->p;
    OhPullSeg *tab = (OhPullSeg *)(sp + L.own_bytes);
    int nt = 0;
    size_t pulled = 0;
    { HostTimer t(e, OH_HT_UPLOAD_MEMCPY);
    for (int i = 0; i < L.ns; i++)
        if (L.seg[i].own && L.seg[i].bytes) {
            memcpy(sp, L.seg[i].src, L.seg[i].bytes);
            tab[nt++] = OhPullSeg{ sp, arena + L.seg[i].off, L.seg[i].bytes };
            sp += align_up(L.seg[i].bytes, 256);
        }
    for (int i = 0; i < L.ns; i++)
        if (!L.seg[i].own && L.copied(L.seg[i])) {
            tab[nt++] = OhPullSeg{ L.seg[i].src, arena + L.seg[i].off, L.seg[i].bytes };
            pulled += L.seg[i].bytes;
        }
    }
    HostTimer t_enq(e, OH_HT_UPLOAD_ENQUEUE);
    ohk_pull(tab, nt, pulled, e->copy_stream);
    return hipGetLastError();
}

/* Any other list is staged.  A group of consecutive lists goes into ONE pinned buffer, each laid out as in the arena (their copied
 * parts are neighbours there), by ONE run of the copy helpers over the jobs of all of them -> ONE H2D copy of `bytes` */
static hipError_t stage_copied(OhEngine *e, const HandoverLayout *L, const size_t *copied_off, int n, char *arena, size_t bytes, OhEngine::Stage *sg)
{
    { HostTimer t(e, OH_HT_UPLOAD_MEMCPY);
    e->copy_jobs.clear();
    for (int i = 0; i < n; i++)
        handover_copy_jobs_add(L[i], (char *)sg->p + (copied_off[i] - copied_off[0]), e->copy_jobs);
    copiers_get(e)->run(e->copy_jobs);                      /* claimed piece by piece by the calling thread and the helpers */
    }
    /* asynchronous: the caller's arrays are already copied out; the pinned buffer stays busy until `done` */
    HostTimer t_enq(e, OH_HT_UPLOAD_ENQUEUE);
    return hipMemcpyAsync(arena + copied_off[0], sg->p, bytes, hipMemcpyHostToDevice, e->copy_stream);
}

/* with bs_in, behind the copy: both grids from the maps — once per work list, the maps never change */
static hipError_t enqueue_bs_derive(const OhFrame *f, const HandoverHeader &H, hipStream_t cs)
{
    const size_t bs_packed = (oh_bs_size(&f->p) + 3) / 4;
    hipError_t hrc = hipMemsetAsync((void *)H.d.vbs, 0, align_up(bs_packed, 4), cs);     /* bs_kernel ORs the non-zero strengths in; the padded tail is read by the deblock pass */
    if (hrc == hipSuccess) hrc = hipMemsetAsync((void *)H.d.hbs, 0, align_up(bs_packed, 4), cs);
    if (hrc == hipSuccess)
        ohk_bs_derive(&f->p, H.mvf, H.cbf_luma, H.call_log2, H.ctb_flags, f->bs_in->loop_filter_across_tiles, (void *)H.d.vbs, (void *)H.d.hbs, cs);
    return hrc;
}

/* what the hand-over of a chunk keeps per list between its steps (per host thread: engines of several threads hand over at once) */
struct ChunkScratch {
    HostSide h[OH_MAX_BATCH];
    std::vector<uint32_t> pu_off[OH_MAX_BATCH];
    HandoverHeader H[OH_MAX_BATCH];
    HandoverLayout L[OH_MAX_BATCH];
    Pic *cur[OH_MAX_BATCH];
    uint32_t ref_ok[OH_MAX_BATCH];
    HandoverCheck chk[OH_MAX_BATCH];  /* the error slot of every list: written by whichever thread checked it */
};

/* The hand-over of one chunk, n <= OH_MAX_BATCH lists: every list checked and counted; ONE arena; the lists staged and copied in
 * groups of OH_STAGE_GROUP (a pulled list is a group of its own); one set of preparation launches (the kernels pick the list with a
 * grid dimension, like the passes); ONE `ready` event.  On the copy stream that is at most one wait, a copy and an event per group,
 * the preparation launches and one event.  On an error out[] holds the lists made so far (or nulls): the caller frees them. */
static int upload_chunk(OhEngine *e, const OhFrame *const *fs, int n, OhDevFrame **out)
{
    static thread_local std::unique_ptr<ChunkScratch> scratch;
    if (!scratch) scratch.reset(new ChunkScratch());
    ChunkScratch &S = *scratch;
    HostTimer t_all(e, OH_HT_UPLOAD);
    CopyPool *pool = copiers_get(e);
    /* what needs the engine, list by list on this thread: it stops at the first list it refuses (n_ok of them passed; the error
     * stands in e->err), and that list is the one reported unless a list before it fails its own check below */
    int n_ok = 0, rc_engine = OH_OK;
    auto engine_side = [&](int i) -> int {
        const OhFrame *f = fs[i];
        if (!f)
            return OH_E_ARG;
        if (const int rc = check_params(e, &f->p))
            return rc;
        S.cur[i] = get_pic(e, f->cur_pic);
        if (!S.cur[i] || !same_geometry(S.cur[i]->p, f->p))
            FAIL(e, OH_E_ARG, "cur_pic %d is not an allocated picture of this geometry", f->cur_pic);
        S.ref_ok[i] = usable_refs(e, f, S.cur[i]);
        return OH_OK;
    };
    while (n_ok < n && (rc_engine = engine_side(n_ok)) == OH_OK)
        n_ok++;
    /* check and count, list-parallel: every list is taken by one thread (this one or a helper) and all of them are through before
     * anything is taken from a pool or enqueued, so a refused chunk leaves the engine as it was */
    int bad;
    { HostTimer t(e, OH_HT_UPLOAD_COUNT);
    bad = handover_check_chunk(pool, fs, S.ref_ok, n_ok, S.h, S.pu_off, S.chk);
    }
    if (bad >= 0) {
        e->err = S.chk[bad].msg;
        return S.chk[bad].rc;
    }
    if (rc_engine != OH_OK)
        return rc_engine;
    for (int i = 0; i < n; i++) {
        memset(&S.H[i], 0, sizeof(S.H[i]));
        S.L[i] = handover_layout(fs[i], S.h[i], &S.H[i].d);
    }
    HIPCHK(e, hipSetDevice(e->device));
    const HandoverChunk C = handover_chunk_place(S.L, n);
    OhChunk *ck = new OhChunk();
    int rc;
    { HostTimer t(e, OH_HT_UPLOAD_ARENA);
    rc = arena_take(e, C.total, ck);
    }
    if (rc) {
        delete ck;
        return rc;
    }
    if ((ck->sum_host = summary_block_get(e)) == nullptr) {
        chunk_free(e, ck, false);
        FAIL(e, OH_E_NOMEM, "hipHostMalloc(%zu) for the summaries failed", OH_MAX_BATCH * sizeof(DevSummary));
    }
    char *arena = (char *)ck->arena;
    ck->refs = n;
    for (int i = 0; i < n; i++) {
        const OhFrame *f = fs[i];
        const HostSide &h = S.h[i];
        OhDevFrame *df = new OhDevFrame();
        df->chunk = ck;
        fill_header(e, f, S.cur[i], h, S.L[i], arena + C.copied_off[i], arena + C.rest_off[i], df, &S.H[i]);
        df->sum_host = (DevSummary *)ck->sum_host + i;
        S.H[i].d.summary_host = df->sum_host;              /* pinned, device-accessible: prep_finish stores the summary there */
        df->sum_dev = S.H[i].d.summary;
        df->cnt = h.cnt;
        df->d = (DevFrame *)(arena + C.copied_off[i]);
        df->p = f->p;
        for (int k = 0; k < 4; k++) df->tu_cnt[k] = h.tu_cnt[k];
        df->n_cross = h.n_cross;
        df->has_sao = f->p.sao_enabled && f->sao;
        df->cur_pic = f->cur_pic;              /* which half of cur_pic is final changes when the list is EXECUTED, not here */
        df->owner = e;
        out[i] = df;
    }

    hipStream_t cs = e->copy_stream;
    /* byte grids still have to be packed on the way: such a list is staged even when it lies in pinned memory */
    auto pulled = [&](int i) { return (fs[i]->flags & OH_FRAME_PINNED) != 0 && !S.L[i].packs; };
    for (int g0 = 0, g1; g0 < n; g0 = g1) {
        const bool pull = pulled(g0);
        for (g1 = g0 + 1; !pull && g1 < n && g1 - g0 < OH_STAGE_GROUP && !pulled(g1); g1++)
            ;
        const size_t bytes = C.copied_off[g1] - C.copied_off[g0];
        OhEngine::Stage *sg;
        { HostTimer t(e, OH_HT_UPLOAD_STAGE_WAIT);
        sg = stage_acquire(e, pull ? pulled_stage_bytes(S.L[g0]) : bytes);   /* a pinned buffer whose previous copy has completed */
        }
        if (!sg)
            FAIL(e, OH_E_NOMEM, "hipHostMalloc(%zu) failed", bytes);
        hipError_t hrc = pull ? stage_pulled(e, S.L[g0], arena + C.copied_off[g0], sg)
                              : stage_copied(e, &S.L[g0], &C.copied_off[g0], g1 - g0, arena, bytes, sg);
        HostTimer t_enq(e, OH_HT_UPLOAD_ENQUEUE);
        if (hrc == hipSuccess && stage_in_use(e, sg, cs) != OH_OK)
            hrc = hipGetLastError();
        for (int i = g0; i < g1; i++) {
            e->up_bytes += S.L[i].copy_bytes;
            if (hrc == hipSuccess && S.H[i].mvf)
                hrc = enqueue_bs_derive(fs[i], S.H[i], cs);
        }
        if (hrc != hipSuccess)
            FAIL(e, OH_E_HIP, "work-list upload failed: %s", hipGetErrorString(hrc));
    }

    HostTimer t_enq(e, OH_HT_UPLOAD_ENQUEUE);
    OhBatch B;
    memset(&B, 0, sizeof(B));
    OhPrepCounts mx;
    memset(&mx, 0, sizeof(mx));
    uint32_t max_cross = 0, max_runs = 0;
    for (int i = 0; i < n; i++) {
        const OhDevFrame *df = out[i];
        B.f[i] = df->d;
        mx.n_pu = std::max(mx.n_pu, df->cnt.n_pu); mx.n_tu = std::max(mx.n_tu, df->cnt.n_tu);
        mx.n_intra = std::max(mx.n_intra, df->cnt.n_intra); mx.n_sub = std::max(mx.n_sub, df->cnt.n_sub);
        mx.n_ictu = std::max(mx.n_ictu, df->cnt.n_ictu);
        max_runs = std::max(max_runs, ((df->cnt.n_mc_luma + 63) >> 6) + ((df->cnt.n_mc_chroma + 63) >> 6));
        max_cross = std::max(max_cross, df->n_cross);
    }
    ohk_prepare(&B, n, &mx, max_runs, max_cross, cs);
    HIPCHK(e, hipGetLastError());
    /* one point in the copy stream makes all of them ready */
    if ((ck->ready = sync_event_get(e)) == nullptr)
        FAIL(e, OH_E_NOMEM, "no event for the work lists");
    HIPCHK(e, hipEventRecord(ck->ready, cs));
    return OH_OK;
}

extern "C" int oh_frames_upload(OhEngine *e, const OhFrame *const *fs, int n, OhDevFrame **out)
{
    if (!e || n < 0 || (n && (!fs || !out)))
        return OH_E_ARG;
    for (int i = 0; i < n; i++) out[i] = nullptr;
    int rc = OH_OK;
    for (int c0 = 0; c0 < n && rc == OH_OK; c0 += OH_MAX_BATCH)
        rc = upload_chunk(e, fs + c0, n - c0 < OH_MAX_BATCH ? n - c0 : OH_MAX_BATCH, out + c0);
    if (rc != OH_OK) {                                     /* all or nothing */
        bool any = false;
        for (int i = 0; i < n; i++) any = any || out[i];
        if (any) (void)hipStreamSynchronize(e->copy_stream);
        for (int i = 0; i < n; i++) { free_dev_frame(e, out[i]); out[i] = nullptr; }
    }
    return rc;
}

extern "C" int oh_frame_upload(OhEngine *e, const OhFrame *f, OhDevFrame **out)
{
    if (!e || !f || !out)
        return OH_E_ARG;
    return oh_frames_upload(e, &f, 1, out);
}
