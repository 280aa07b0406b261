/*
 * engine.hip — host side of the MI355X engine: device-resident pictures (the DPB lives in HBM), staging buffers,
 * pass scheduling on one HIP stream, release of executed work lists, per-pass event timing.  Work lists are handed over
 * in engine_handover.hip; what runs on finished pictures beside that path is in engine_pics.hip (its engine-free arithmetic in
 * pics_math.hip) and engine_shvc.hip; engine_impl.h is what they share.
 * C ABI in include/ohevc_hip.h.  No CPU fallback exists: without a usable device every entry
 * point returns OH_E_HIP.
 */
#include "engine_impl.h"

/* after a wait on the engine's stream: did a kernel latch a failure (intra.hip: dag_latch_error)?  Reported once, then cleared. */
int kernel_error(OhEngine *e)
{
    if (!e->kerr || !e->kerr[0])
        return OH_OK;
    const uint32_t pic = e->kerr[1], where = e->kerr[2];     /* kerr[0] = OH_KE_DAG_TIMEOUT, the only code */
    e->kerr[0] = 0;
    FAIL(e, OH_E_HIP, "intra pass (one launch per picture): picture %u, schedule entry %u gave up waiting for a neighbour CTU; the picture's samples are not valid",
         pic, where);
}

HostTimer::HostTimer(OhEngine *e_, int slot_) : e(e_), slot(slot_), t0(std::chrono::steady_clock::now()) {}
HostTimer::~HostTimer()
{
    e->host_ms[slot] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    e->host_calls[slot]++;
}

extern "C" uint64_t oh_engine_upload_bytes(OhEngine *e, int reset)
{
    if (!e)
        return 0;
    const uint64_t v = e->up_bytes;
    if (reset) e->up_bytes = 0;
    return v;
}

extern "C" int oh_engine_host_times(OhEngine *e, double *ms, uint64_t *calls, int n, int reset)
{
    if (!e || n < 0)
        return OH_E_ARG;
    for (int i = 0; i < n && i < OH_N_HOST_TIMES; i++) {
        if (ms) ms[i] = e->host_ms[i];
        if (calls) calls[i] = e->host_calls[i];
    }
    if (reset)
        for (int i = 0; i < OH_N_HOST_TIMES; i++) { e->host_ms[i] = 0; e->host_calls[i] = 0; }
    return OH_OK;
}

static int engine_create(OhEngine **out, int device, hipStream_t ext, bool use_ext)
{
    if (!out)
        return OH_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        fprintf(stderr, "ohevc_hip: no usable HIP device (count=%d, requested %d); there is no CPU fallback\n", n, device);
        return OH_E_HIP;
    }
    OhEngine *e = new OhEngine();
    e->device = device;
    bool ok = hipSetDevice(device) == hipSuccess;
    if (ok && use_ext) {
        e->stream = ext;
        e->own_stream = false;
    } else if (ok) {
        ok = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) == hipSuccess;
    }
    /* default priority.  With the highest stream priority (hipStreamCreateWithPriority) the 4K Main 10 decode bench, four hardware
     * queues, four alternating pairs of runs, gave 82.6-82.8 Gpixels/s against 79.3-87.9 (median 87.3) without, and arena_take's share
     * of the host time rose from 0.0001 to 0.03 ms per picture (profiles/r10_chunk_handover.txt); at 12 queues it made no difference */
    if (ok)
        ok = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok || ohk_init() != 0) {
        fprintf(stderr, "ohevc_hip: device %d initialisation failed\n", device);
        delete e;
        return OH_E_HIP;
    }
    if (hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || e->n_cu <= 0)
        e->n_cu = 256;
    if (hipHostMalloc((void **)&e->kerr, 4 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
        fprintf(stderr, "ohevc_hip: no pinned memory for the kernels' error word\n");
        delete e;
        return OH_E_HIP;
    }
    memset(e->kerr, 0, 4 * sizeof(uint32_t));
    if (hipMalloc((void **)&e->tickets, (size_t)OhEngine::TICKET_WORDS * OhEngine::TICKET_RING * sizeof(uint32_t)) != hipSuccess) {
        fprintf(stderr, "ohevc_hip: no device memory for the ticket counters\n");
        delete e;
        return OH_E_HIP;
    }
    e->tuning = tuning_from_env();
    if (e->tuning.stamps) {
        const size_t bytes = (16 + 4000 * 16) * sizeof(uint64_t);
        if (hipMalloc((void **)&e->dbg, bytes) == hipSuccess)
            (void)hipMemset(e->dbg, 0, bytes);
    }
    *out = e;
    return OH_OK;
}

/* diagnostics: copies the in-kernel stamp records (see intra.hip, OH_STAMPS) and clears them */
extern "C" int oh_debug_read(OhEngine *e, uint64_t *out, size_t n_u64)
{
    if (!e || !e->dbg || !out)
        return OH_E_ARG;
    const size_t total = 16 + 4000 * 16;
    if (n_u64 > total) n_u64 = total;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(out, e->dbg, n_u64 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemset(e->dbg, 0, total * sizeof(uint64_t)));
    return OH_OK;
}

/* page-locked host memory for work lists handed over with OH_FRAME_PINNED (the GPU reads them by DMA where they lie) */
extern "C" void *oh_host_alloc(size_t bytes)
{
    void *p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
extern "C" void oh_host_free(void *p) { if (p) (void)hipHostFree(p); }

extern "C" int oh_engine_create(OhEngine **out, int device) { return engine_create(out, device, nullptr, false); }
extern "C" int oh_engine_create_on_stream(OhEngine **out, int device, void *hip_stream)
{
    return engine_create(out, device, (hipStream_t)hip_stream, true);
}

extern "C" int oh_engine_memory(OhEngine *e, uint64_t out[6])
{
    if (!e || !out)
        return OH_E_ARG;
    uint64_t sb = 0;
    for (auto &c : e->stages) sb += c.bytes;
    out[0] = e->arenas_alive; out[1] = e->arena_bytes_alive; out[2] = e->arenas.size();
    out[3] = e->stages.size(); out[4] = sb; out[5] = e->deferred.size();
    return OH_OK;
}

extern "C" const char *oh_engine_last_error(const OhEngine *e) { return e ? e->err.c_str() : "no engine"; }
extern "C" void *oh_engine_stream(OhEngine *e) { return e ? (void *)e->stream : nullptr; }

extern "C" int oh_engine_sync(OhEngine *e)
{
    if (!e)
        return OH_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (OhDevFrame *df : e->deferred)
        free_dev_frame(e, df);
    e->deferred.clear();
    return kernel_error(e);
}

extern "C" void oh_engine_destroy(OhEngine *e)
{
    if (!e)
        return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
    for (OhDevFrame *df : e->deferred)
        free_dev_frame(e, df);
    for (Pic &p : e->pics)
        if (p.used && p.base && p.owned)
            (void)hipFree(p.base);
    for (auto &s : e->ev_pool)
        for (auto &ev : s.ev) (void)hipEventDestroy(ev);
    for (auto &ev : e->lev_pool) (void)hipEventDestroy(ev);
    for (auto &ev : e->lev_pending) (void)hipEventDestroy(ev);
    for (auto &s : e->ev_pending)
        for (auto &ev : s.ev) (void)hipEventDestroy(ev);
    for (auto &c : e->stages) { (void)hipEventDestroy(c.done); (void)hipHostFree(c.p); }
    for (auto &a : e->arenas) { if (a.free_ev) (void)hipEventDestroy(a.free_ev); (void)hipFree(a.p); }
    for (auto &ev : e->sync_events) (void)hipEventDestroy(ev);
    for (void *b : e->sum_pool) (void)hipHostFree(b);
    if (e->dl_count && e->tuning.fetch_timing)
        fprintf(stderr, "ohevc engine: %llu output fetches, per fetch %.2f ms waiting for the picture's passes and its device-to-host copy, %.2f ms moving the rows into the caller's planes\n",
                (unsigned long long)e->dl_count, e->dl_wait_ms / e->dl_count, e->dl_copy_ms / e->dl_count);
    delete e->copiers;
    delete e->dl_copiers;
    for (auto *c : e->dl_stages) { (void)hipEventDestroy(c->done); (void)hipHostFree(c->p); delete c; }
    if (e->kerr) (void)hipHostFree(e->kerr);
    if (e->tickets) (void)hipFree(e->tickets);
    for (const OhEngine::Scratch *s : { &e->hash_dev, &e->resize_dev, &e->colour_tabs.dev, &e->light_tabs.dev, &e->light_res, &e->compare_res,
                                        &e->compose_dev, &e->hist_res, &e->lut_tabs, &e->grain_tabs, &e->grain_patterns, &e->remap_tabs, &e->motion_res, &e->motion_centres, &e->motion_field })
        if (s->p) (void)hipFree(s->p);
    for (auto &ev : e->batch_ev) if (ev) (void)hipEventDestroy(ev);
    if (e->dl_stream) { (void)hipStreamSynchronize(e->dl_stream); (void)hipStreamDestroy(e->dl_stream); }
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    if (e->own_stream)
        (void)hipStreamDestroy(e->stream);
    delete e;
}

/* ---------------- pictures ---------------- */
int check_params(OhEngine *e, const OhPicParams *p)
{
    if (!p || p->width <= 0 || p->height <= 0 || p->width > 16384 || p->height > 16384)
        FAIL(e, OH_E_ARG, "bad picture size");
    if (p->bit_depth != 8 && p->bit_depth != 9 && p->bit_depth != 10 && p->bit_depth != 12)
        FAIL(e, OH_E_UNSUPPORTED, "bit depth %d not supported (8/9/10/12: what the reference's wrapper can hand out, openHevcWrapper.c)", p->bit_depth);
    if (p->chroma_format_idc < 0 || p->chroma_format_idc > 3)
        FAIL(e, OH_E_ARG, "chroma_format_idc %d out of range", p->chroma_format_idc);
    if (p->log2_ctb_size < 4 || p->log2_ctb_size > 6 || p->log2_min_cb_size < 3 || p->log2_min_cb_size > p->log2_ctb_size ||
        p->log2_min_tb_size < 2 || p->log2_min_tb_size > 5 || p->log2_min_pu_size != p->log2_min_cb_size - 1)
        FAIL(e, OH_E_ARG, "bad block size parameters");
    if ((uint64_t)oh_ctb_width(p) * (uint64_t)oh_ctb_height(p) > 65535u)
        FAIL(e, OH_E_UNSUPPORTED, "%d x %d picture with %d x %d CTBs has more than 65535 CTBs: the intra schedule (OhIntraCtu.ctu) counts them in 16 bits; use larger CTBs",
             p->width, p->height, 1 << p->log2_ctb_size, 1 << p->log2_ctb_size);
    if (p->width % (1 << p->log2_min_cb_size) || p->height % (1 << p->log2_min_cb_size))
        FAIL(e, OH_E_ARG, "picture size must be a multiple of the minimum CB size");
    return OH_OK;
}

/* layout of one picture allocation: half 0 = planes A, half 1 = planes B */
static size_t pic_layout(const OhPicParams *p, Pic *pic, size_t off[6])
{
    uint64_t o[3] = { 0, 0, 0 };
    const size_t half = (size_t)oh_pic_half_layout(p, pic->stride, o);
    for (int c = 0; c < (p->chroma_format_idc ? 3 : 1); c++) {
        pic->w[c] = p->width >> oh_hshift(p, c);
        pic->h[c] = p->height >> oh_vshift(p, c);
        off[c] = (size_t)o[c];
        off[3 + c] = half + (size_t)o[c];
    }
    return 2 * half;
}

extern "C" size_t oh_pic_bytes(const OhPicParams *p)
{
    Pic tmp;
    size_t off[6];
    return p ? pic_layout(p, &tmp, off) : 0;
}

static int pic_install(OhEngine *e, const OhPicParams *p, void *half0, void *half1, bool owned, int *pic_id)
{
    Pic pic;
    size_t off[6];
    pic.used = true;
    pic.p = *p;
    pic.owned = owned;
    pic.gen = ++e->pic_gen;
    size_t half = pic_layout(p, &pic, off) / 2;
    pic.base = half0;
    for (int c = 0; c < (p->chroma_format_idc ? 3 : 1); c++) {
        pic.a[c] = (char *)half0 + off[c];
        pic.b[c] = (char *)half1 + (off[3 + c] - half);
    }
    size_t id = 0;
    while (id < e->pics.size() && e->pics[id].used)
        id++;
    if (id == e->pics.size())
        e->pics.push_back(pic);
    else
        e->pics[id] = pic;
    *pic_id = (int)id;
    return OH_OK;
}

extern "C" int oh_pic_alloc(OhEngine *e, const OhPicParams *p, int *pic_id)
{
    if (!e || !pic_id)
        return OH_E_ARG;
    int rc = check_params(e, p);
    if (rc)
        return rc;
    HIPCHK(e, hipSetDevice(e->device));
    void *mem = nullptr;
    HIPCHK(e, hipMalloc(&mem, oh_pic_bytes(p)));
    return pic_install(e, p, mem, (char *)mem + oh_pic_bytes(p) / 2, true, pic_id);
}

extern "C" int oh_pic_wrap(OhEngine *e, const OhPicParams *p, void *half0, void *half1, size_t half_bytes, int *pic_id)
{
    if (!e || !pic_id || !half0 || !half1)
        return OH_E_ARG;
    int rc = check_params(e, p);
    if (rc)
        return rc;
    if (half_bytes < oh_pic_bytes(p) / 2 || ((uintptr_t)half0 & 255) || ((uintptr_t)half1 & 255))
        FAIL(e, OH_E_ARG, "oh_pic_wrap: each half needs %zu bytes, 256-byte aligned", oh_pic_bytes(p) / 2);
    return pic_install(e, p, half0, half1, false, pic_id);
}

Pic *get_pic(OhEngine *e, int id)
{
    if (id < 0 || (size_t)id >= e->pics.size() || !e->pics[id].used)
        return nullptr;
    return &e->pics[id];
}

int check_pics(OhEngine *e, const int *pic_ids, int n, const char *who)
{
    for (int i = 0; i < n; i++)
        if (!get_pic(e, pic_ids[i]))
            FAIL(e, OH_E_ARG, "%s: unknown picture %d", who, pic_ids[i]);
    return OH_OK;
}

extern "C" int oh_pic_free(OhEngine *e, int pic_id)
{
    if (!e)
        return OH_E_ARG;
    Pic *p = get_pic(e, pic_id);
    if (!p)
        FAIL(e, OH_E_ARG, "oh_pic_free: unknown picture %d", pic_id);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (p->owned)
        HIPCHK(e, hipFree(p->base));
    *p = Pic();
    return OH_OK;
}

extern "C" int oh_pic_final_half(OhEngine *e, int pic_id)
{
    if (!e)
        return OH_E_ARG;
    Pic *p = get_pic(e, pic_id);
    return p ? (p->final_b ? 1 : 0) : OH_E_ARG;
}

extern "C" int oh_pic_set_final_half(OhEngine *e, int pic_id, int half)
{
    if (!e)
        return OH_E_ARG;
    Pic *p = get_pic(e, pic_id);
    if (!p || (half != 0 && half != 1))
        FAIL(e, OH_E_ARG, "oh_pic_set_final_half: bad picture or half");
    p->final_b = half == 1;
    p->done_seq = 0;                      /* filled from outside (an exchange): a download stays behind the whole engine stream */
    return OH_OK;
}

/* a new pinned buffer of at least `bytes` (4 MiB steps) with its event, not busy; false: nothing was allocated */
bool stage_create(OhEngine::Stage *c, size_t bytes)
{
    c->bytes = align_up(bytes, (size_t)4 << 20); c->busy = false; c->p = nullptr; c->done = nullptr;
    if (hipHostMalloc(&c->p, c->bytes, hipHostMallocDefault) == hipSuccess && hipEventCreateWithFlags(&c->done, hipEventDisableTiming) == hipSuccess)
        return true;
    if (c->p) (void)hipHostFree(c->p);
    return false;
}

/* a pinned buffer of at least `bytes` whose previous copy has completed (uploads and downloads share the pool) */
OhEngine::Stage *stage_acquire(OhEngine *e, size_t bytes)
{
    OhEngine::Stage *sg = nullptr;
    for (auto &c : e->stages) {
        if (c.busy && hipEventQuery(c.done) == hipSuccess)
            c.busy = false;
        if (!c.busy && c.bytes >= bytes && (!sg || c.bytes < sg->bytes))
            sg = &c;
    }
    if (sg)
        return sg;
    /* every buffer that fits is busy: beyond OH_STAGE_POOL_BYTES wait for the one whose copy is furthest along instead of pinning more
     * host memory (this is what throttles a host that hands pictures over faster than PCIe and the passes take them) */
    size_t alive = 0;
    for (auto &c : e->stages) alive += c.bytes;
    const size_t want = align_up(bytes, (size_t)4 << 20);
    if (alive + want > OH_STAGE_POOL_BYTES) {
        for (auto &c : e->stages)
            if (c.busy && c.bytes >= bytes) {
                if (hipEventSynchronize(c.done) != hipSuccess)
                    return nullptr;
                c.busy = false;
                return &c;
            }
        /* the pool holds smaller buffers only (lists that came alone before a chunk did): idle ones make room */
        for (size_t i = e->stages.size(); i-- > 0 && alive + want > OH_STAGE_POOL_BYTES; )
            if (!e->stages[i].busy) {
                alive -= e->stages[i].bytes;
                (void)hipEventDestroy(e->stages[i].done); (void)hipHostFree(e->stages[i].p);
                e->stages.erase(e->stages.begin() + (long)i);
            }
    }
    OhEngine::Stage c;
    if (!stage_create(&c, bytes))
        return nullptr;
    e->stages.push_back(c);
    return &e->stages.back();
}

/* a host list where the kernels read it: copied into a pinned buffer of the pool (pinned host memory is mapped) */
OhEngine::Stage *stage_list(OhEngine *e, const void *list, size_t bytes)
{
    OhEngine::Stage *sg = stage_acquire(e, bytes);
    if (sg) memcpy(sg->p, list, bytes);
    return sg;
}

/* what is enqueued on `st` so far reads the buffer: it is busy until the stream has passed this point */
int stage_in_use(OhEngine *e, OhEngine::Stage *sg, hipStream_t st)
{
    HIPCHK(e, hipEventRecord(sg->done, st));
    sg->busy = true;
    return OH_OK;
}

/* the summary the preparation kernels left (prep.hip): waits for the list's `ready` event the first time */
static int read_summary(OhEngine *e, OhDevFrame *df, int index)
{
    if (df->summary_read)
        return df->prep_err ? OH_E_ARG : OH_OK;
    { HostTimer t(e, OH_HT_EXECUTE_WAIT_PREP);
    HIPCHK(e, hipEventSynchronize(df->chunk->ready));
    }
    const DevSummary *s = (const DevSummary *)df->sum_host;
    df->summary_read = true;
    df->prep_err = s->err;
    if (s->err) {
        static const char *what[] = { "", "prediction unit", "transform block", "intra block", "intra schedule entry" };
        FAIL(e, OH_E_ARG, "work list %d: %s %u is malformed (rectangle / reference / index out of range); nothing of it was executed",
             index, what[s->err <= 4 ? s->err : 0], s->err_item);
    }
    for (int k = 0; k < 4; k++)
        if (s->tu_cnt[k] != df->tu_cnt[k])
            FAIL(e, OH_E_ARG, "work list %d: transform block counts changed between hand-over and preparation", index);
    df->intra_area64 = s->intra_area64; df->max_passes = s->max_passes;
    df->max_items = s->max_items; df->max_sub = s->max_sub; df->max_res = s->max_res; df->res_scattered = s->res_scattered != 0;
    df->sum_items = s->sum_items; df->sum_sub = s->sum_sub;
    return OH_OK;
}

/* The intra pass of a batch (intra.hip), one launch per form; which form a picture takes and the staged launch's numbers are
 * intra_plan.h's.  A CTU takes the schedule entry of the ticket it draws when it starts and waits only for lower tickets, so the
 * launch drains whatever the dispatch order; a wait that gives up anyway (bounded by OhTuning::spin_limit) is reported by kernel_error. */
static int intra_pass(OhEngine *e, OhDevFrame *const *fr, int nb, const OhBatch *all, hipStream_t st)
{
    const OhPicParams *p = &fr[0]->p;
    OhBatch bd, bs;                                  /* direct / staged dag */
    memset(&bd, 0, sizeof(bd)); memset(&bs, 0, sizeof(bs));
    int nd = 0, ns = 0;
    uint32_t max_ictu_d = 0, max_ictu_s = 0, max_ictu_all = 0;
    OhIntraFigures fig;
    fig.batch = nb;
    for (int i = 0; i < nb; i++) {
        if (!fr[i]->cnt.n_ictu)
            continue;
        max_ictu_all = std::max(max_ictu_all, fr[i]->cnt.n_ictu);
        if (intra_plan_direct(p, fr[i]->intra_area64, e->tuning)) {
            bd.f[nd++] = fr[i]->d;
            max_ictu_d = std::max(max_ictu_d, fr[i]->cnt.n_ictu);
            continue;
        }
        bs.f[ns++] = fr[i]->d;
        max_ictu_s = std::max(max_ictu_s, fr[i]->cnt.n_ictu);
        fig.total_entries += fr[i]->cnt.n_ictu;
        const OhDevFrame &d = *fr[i];
        fig.max_items = std::max(fig.max_items, d.max_items); fig.max_sub = std::max(fig.max_sub, d.max_sub); fig.max_res = std::max(fig.max_res, d.max_res);
        fig.sum_items += d.sum_items; fig.sum_sub += d.sum_sub;
        fig.contiguous = fig.contiguous && !d.res_scattered;
    }
    if (!nd && !ns)
        return OH_OK;
    /* the pass's launches as one bracket (they overlap nothing else on this stream); per-launch events are a sample, not a log:
     * stop bracketing once 100 k launches are pending collection */
    hipEvent_t a = nullptr, b = nullptr;
    if (e->profile > 1 && e->lev_pending.size() < 200000) {
        for (hipEvent_t *pe : { &a, &b }) {
            if (!e->lev_pool.empty()) { *pe = e->lev_pool.back(); e->lev_pool.pop_back(); }
            else HIPCHK(e, hipEventCreate(pe));
        }
    }
    uint32_t *tk = e->tickets + (size_t)OhEngine::TICKET_WORDS * (e->ticket_seq++ % OhEngine::TICKET_RING);
    ohk_intra_dag_reset(all, nb, max_ictu_all, tk, st);
    if (a) HIPCHK(e, hipEventRecord(a, st));
    if (nd)
        ohk_intra_direct(&bd, nd, p, max_ictu_d, tk, e->tuning.spin_limit, st);
    if (ns) {
        const OhIntraLaunch IL = intra_plan_launch(p->log2_ctb_size, p->chroma_format_idc, fig, e->n_cu, e->tuning);
        ohk_intra_dag(&bs, ns, p, &IL, max_ictu_s, tk + OH_MAX_BATCH * 32, e->tuning.spin_limit, st);
    }
    if (b) {
        HIPCHK(e, hipEventRecord(b, st));
        e->lev_pending.push_back(a);
        e->lev_pending.push_back(b);
    }
    return OH_OK;
}

/* Execute n mutually independent pictures: every pass is one launch over all of them (chunks of
 * OH_MAX_BATCH).  Nothing orders the pictures of a batch against each other, so none of them may be a
 * reference of another one. */
extern "C" int oh_frames_execute(OhEngine *e, OhDevFrame *const *dfs, int n)
{
    if (!e || n < 0 || (n && !dfs))
        return OH_E_ARG;
    if (n == 0)
        return OH_OK;                                       /* an empty batch is a no-op */
    HostTimer t_all(e, OH_HT_EXECUTE);
    HIPCHK(e, hipSetDevice(e->device));
    for (int i = 0; i < n; i++) {
        if (!dfs[i])
            return OH_E_ARG;
        if (dfs[i]->owner != e)
            FAIL(e, OH_E_ARG, "batch: picture %d was uploaded to another engine", i);
        int src = read_summary(e, dfs[i], i);               /* a malformed list stops the batch before anything is launched */
        if (src)
            return src;
        const OhPicParams &a = dfs[0]->p, &b = dfs[i]->p;
        if (memcmp(&a, &b, sizeof(a)) != 0)
            FAIL(e, OH_E_ARG, "batch: picture %d has other parameters than picture 0", i);
    }
    hipStream_t st = e->stream;
    {
        /* Pictures are looked up NOW, not at upload: the work list may have been uploaded before its references were decoded or
         * received (multi-GPU exchange: oh_pic_set_final_half after the upload), and ids may have been freed and reused since.
         * A reference whose finished half differs from the one DevFrame.refs[] points at is patched in HBM, in stream order. */
        std::vector<uint8_t> role(e->pics.size(), 0);             /* 1: written by this batch, 2: read by this batch */
        struct Patch { DevPlanes *dst; DevPlanes v; };
        std::vector<Patch> patches;
        for (int i = 0; i < n; i++) {
            OhDevFrame *df = dfs[i];
            if (!df->chunk->waited) {                       /* the chunk's copies run on the copy stream: one wait covers its lists */
                HIPCHK(e, hipStreamWaitEvent(st, df->chunk->ready, 0));
                df->chunk->waited = true;
            }
            Pic *c = get_pic(e, df->cur_pic);
            if (!c || c->gen != df->cur_gen)
                FAIL(e, OH_E_ARG, "batch: picture %d's cur_pic %d was freed after the upload", i, df->cur_pic);
            if (role[df->cur_pic] & 1)
                FAIL(e, OH_E_ARG, "batch: two work lists reconstruct picture %d", df->cur_pic);
            role[df->cur_pic] |= 1;
        }
        for (int i = 0; i < n; i++) {
            OhDevFrame *df = dfs[i];
            for (int s = 0; s < OH_MAX_REFS; s++) {
                if (!(df->ref_used >> s & 1))
                    continue;
                Pic *r = get_pic(e, df->ref_id[s]);
                if (!r || r->gen != df->ref_gen[s])
                    FAIL(e, OH_E_ARG, "batch: picture %d references picture %d, which was freed after the upload", i, df->ref_id[s]);
                if (role[df->ref_id[s]] & 1)
                    FAIL(e, OH_E_ARG, "batch: picture %d is a reference of picture %d of the same batch (nothing orders them)", df->ref_id[s], i);
                const uint8_t half = r->final_b ? 1 : 0;
                if (half != df->ref_half[s]) {
                    Patch pt;
                    pt.dst = &df->d->refs[s];
                    fill_planes(&pt.v, r, r->final_b);
                    patches.push_back(pt);
                    df->ref_half[s] = half;
                }
            }
        }
        if (!patches.empty()) {
            OhEngine::Stage *sg = stage_acquire(e, patches.size() * sizeof(DevPlanes));
            if (!sg)
                FAIL(e, OH_E_NOMEM, "hipHostMalloc for %zu reference patches failed", patches.size());
            DevPlanes *hp = (DevPlanes *)sg->p;
            for (size_t k = 0; k < patches.size(); k++) {
                hp[k] = patches[k].v;
                HIPCHK(e, hipMemcpyAsync(patches[k].dst, &hp[k], sizeof(DevPlanes), hipMemcpyHostToDevice, st));
            }
            if (const int rc = stage_in_use(e, sg, st))
                return rc;
        }
    }
    const bool prof = e->profile > 0;
    for (int c0 = 0; c0 < n; c0 += OH_MAX_BATCH) {
        const int nb = n - c0 < OH_MAX_BATCH ? n - c0 : OH_MAX_BATCH;
        OhDevFrame *const *fr = dfs + c0;
        const OhPicParams *p = &fr[0]->p;
        EventSet es;
        if (prof) {
            if (!e->ev_pool.empty()) {
                es = e->ev_pool.back();
                e->ev_pool.pop_back();
            } else {
                for (auto &ev : es.ev)
                    HIPCHK(e, hipEventCreate(&ev));
            }
            es.n_frames = nb;
            HIPCHK(e, hipEventRecord(es.ev[0], st));
        }
#define MARK(k) do { if (prof) HIPCHK(e, hipEventRecord(es.ev[(k) + 1], st)); } while (0)
        for (int i = 0; i < nb; i++)                       /* which half holds the finished picture once this has run */
            if (Pic *c = get_pic(e, fr[i]->cur_pic))
                c->final_b = fr[i]->has_sao;
        OhBatch all;
        memset(&all, 0, sizeof(all));
        uint32_t max_luma = 0, max_chroma = 0, max_tu[4] = { 0, 0, 0, 0 };
        for (int i = 0; i < nb; i++) {
            all.f[i] = fr[i]->d;
            max_luma = std::max(max_luma, fr[i]->cnt.n_mc_luma); max_chroma = std::max(max_chroma, fr[i]->cnt.n_mc_chroma);
            for (int k = 0; k < 4; k++) max_tu[k] = std::max(max_tu[k], fr[i]->tu_cnt[k]);
        }
        ohk_inter(&all, nb, p, max_luma, max_chroma, st);
        MARK(OH_PASS_INTER);
        ohk_residual(&all, nb, p, max_tu, st);
        {
            uint32_t max_cross = 0;
            for (int i = 0; i < nb; i++) max_cross = std::max(max_cross, fr[i]->n_cross);
            ohk_cross(&all, nb, p, max_cross, st);
        }
        MARK(OH_PASS_RESIDUAL);
        if (const int rc = intra_pass(e, fr, nb, &all, st))
            return rc;
        MARK(OH_PASS_INTRA);
        if (p->deblock_enabled)
            ohk_deblock(&all, nb, p, 0, st);
        MARK(OH_PASS_DEBLOCK_V);
        if (p->deblock_enabled)
            ohk_deblock(&all, nb, p, 1, st);
        MARK(OH_PASS_DEBLOCK_H);
        {
            OhBatch sub;
            memset(&sub, 0, sizeof(sub));
            int ns = 0;
            for (int i = 0; i < nb; i++)
                if (fr[i]->has_sao)
                    sub.f[ns++] = fr[i]->d;
            if (ns)
                ohk_sao(&sub, ns, p, st);
        }
        MARK(OH_PASS_SAO);
#undef MARK
        HIPCHK(e, hipGetLastError());
        if (prof)
            e->ev_pending.push_back(es);
        {   /* the batch's pictures are finished behind this point of the stream */
            const uint64_t seq = ++e->batch_seq;
            hipEvent_t &bev = e->batch_ev[seq % OhEngine::BATCH_RING];
            if (!bev) HIPCHK(e, hipEventCreateWithFlags(&bev, hipEventDisableTiming));
            HIPCHK(e, hipEventRecord(bev, st));
            for (int i = 0; i < nb; i++)
                if (Pic *c = get_pic(e, fr[i]->cur_pic))
                    c->done_seq = seq;
        }
    }
    return OH_OK;
}

extern "C" int oh_frame_execute(OhEngine *e, OhDevFrame *df)
{
    return oh_frames_execute(e, &df, 1);
}

extern "C" int oh_frame_free(OhEngine *e, OhDevFrame *df)
{
    if (!e || !df)
        return OH_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (df->chunk && df->chunk->ready)
        HIPCHK(e, hipEventSynchronize(df->chunk->ready));   /* never executed: its copy may still be running */
    free_dev_frame(e, df);
    return OH_OK;
}

/* stream-ordered release: the arena returns to the pool at once; whoever reuses it fills it with a copy enqueued on the engine
 * stream, i.e. behind every pass that still reads it.  No host wait (oh_frame_free waits for the stream first). */
extern "C" int oh_frame_release(OhEngine *e, OhDevFrame *df)
{
    if (!e || !df)
        return OH_E_ARG;
    if (df->owner != e)
        FAIL(e, OH_E_ARG, "oh_frame_release: work list of another engine");
    HostTimer t_all(e, OH_HT_RELEASE);
    HIPCHK(e, hipSetDevice(e->device));
    if (df->chunk && !df->chunk->waited && df->chunk->ready) {
        HIPCHK(e, hipStreamWaitEvent(e->stream, df->chunk->ready, 0));      /* never executed: the release still has to stay behind its copy */
        df->chunk->waited = true;
    }
    free_dev_frame(e, df, true);
    return OH_OK;
}

extern "C" int oh_frame_submit(OhEngine *e, const OhFrame *f)
{
    OhDevFrame *df = nullptr;
    int rc = oh_frame_upload(e, f, &df);
    if (rc)
        return rc;
    rc = oh_frame_execute(e, df);
    /* stream-ordered release: the arena returns to the pool behind the passes that read it.  (Rounds 1-2 parked the list until
     * oh_engine_sync: a decoder that submits a long stream and syncs once at the end kept one arena per picture in HBM.) */
    const int rr = oh_frame_release(e, df);
    return rc ? rc : rr;
}

/* the two boundary-strength grids of an uploaded work list as the deblock pass reads them (handed over or derived from bs_in) */
extern "C" int oh_frame_download_bs(OhEngine *e, OhDevFrame *df, uint8_t *vbs, uint8_t *hbs, size_t bytes)
{
    if (!e || !df || !vbs || !hbs)
        return OH_E_ARG;
    if (df->owner != e || !df->p.deblock_enabled)
        FAIL(e, OH_E_ARG, "oh_frame_download_bs: work list of another engine / without deblocking");
    HIPCHK(e, hipSetDevice(e->device));
    if (df->chunk && df->chunk->ready)
        HIPCHK(e, hipEventSynchronize(df->chunk->ready));   /* the list arrives on the copy stream */
    DevFrame hd;
    HIPCHK(e, hipMemcpyAsync(&hd, df->d, sizeof(hd), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const size_t n = bytes < oh_bs_size(&df->p) ? bytes : oh_bs_size(&df->p), np = (n + 3) / 4;
    std::vector<uint8_t> pk(2 * np);
    HIPCHK(e, hipMemcpyAsync(pk.data(), hd.vbs, np, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(pk.data() + np, hd.hbs, np, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < n; i++) {                          /* back to one strength per byte, the reference's layout */
        vbs[i] = (pk[i >> 2] >> ((i & 3) * 2)) & 3;
        hbs[i] = (pk[np + (i >> 2)] >> ((i & 3) * 2)) & 3;
    }
    return OH_OK;
}

/* ---------------- profiling ---------------- */
extern "C" int oh_engine_profile(OhEngine *e, int enable)
{
    if (!e)
        return OH_E_ARG;
    e->profile = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return OH_OK;
}

extern "C" int oh_engine_pass_times(OhEngine *e, double *ms, uint64_t *executes, int reset)
{
    if (!e)
        return OH_E_ARG;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (EventSet &s : e->ev_pending) {
        for (int k = 0; k < OH_N_PASSES; k++) {
            float t = 0;
            HIPCHK(e, hipEventElapsedTime(&t, s.ev[k], s.ev[k + 1]));
            e->pass_ms[k] += t;
        }
        e->executes += (uint64_t)s.n_frames;
        e->ev_pool.push_back(s);
    }
    e->ev_pending.clear();
    for (size_t i = 0; i + 1 < e->lev_pending.size(); i += 2) {
        float t = 0;
        HIPCHK(e, hipEventElapsedTime(&t, e->lev_pending[i], e->lev_pending[i + 1]));
        e->intra_launch_ms += t;
        e->intra_launches++;
        e->lev_pool.push_back(e->lev_pending[i]);
        e->lev_pool.push_back(e->lev_pending[i + 1]);
    }
    e->lev_pending.clear();
    if (ms)
        for (int k = 0; k < OH_N_PASSES; k++) ms[k] = e->pass_ms[k];
    if (executes)
        *executes = e->executes;
    if (reset) {
        for (double &v : e->pass_ms) v = 0;
        e->executes = 0;
    }
    return OH_OK;
}

/* per-LAUNCH device time of the intra pass (sum over launches, count); call after oh_engine_pass_times */
extern "C" int oh_engine_intra_launch_times(OhEngine *e, double *ms, uint64_t *launches, int reset)
{
    if (!e)
        return OH_E_ARG;
    if (ms) *ms = e->intra_launch_ms;
    if (launches) *launches = e->intra_launches;
    if (reset) { e->intra_launch_ms = 0; e->intra_launches = 0; }
    return OH_OK;
}
