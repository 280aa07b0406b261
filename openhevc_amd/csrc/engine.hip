/*
 * engine.hip — host side of the MI355X engine: device-resident pictures (the DPB lives in HBM),
 * work-list upload, pass scheduling on one HIP stream, per-pass event timing.  What runs on finished
 * pictures beside that path is in engine_pics.hip and engine_shvc.hip; engine_impl.h is what they share.
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
    if (ok)
        ok = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking) == hipSuccess;     /* (highest priority for this stream: measured, no difference) */
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
    if (const char *sl = getenv("OHEVC_SPIN_LIMIT"))          /* tests: make a waiting workgroup give up at once */
        e->spin_limit = (uint32_t)std::max(1l, atol(sl));
    if (getenv("OHEVC_STAMPS")) {
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

static hipEvent_t sync_event_get(OhEngine *e)
{
    hipEvent_t ev = nullptr;
    if (!e->sync_events.empty()) { ev = e->sync_events.back(); e->sync_events.pop_back(); return ev; }
    return hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess ? ev : nullptr;
}
static void sync_event_put(OhEngine *e, hipEvent_t ev)
{
    if (!ev) return;
    if (e->sync_events.size() < 4096) e->sync_events.push_back(ev); else (void)hipEventDestroy(ev);
}

/* arenas go back to the engine's pool.  in_flight: kernels enqueued on the engine stream may still read the arena — an event
 * recorded there now tells the copy stream when the next work list may overwrite it. */
static void free_dev_frame(OhEngine *e, OhDevFrame *df, bool in_flight = false)
{
    if (!df)
        return;
    if (e && df->ready)
        sync_event_put(e, df->ready);
    if (df->sum_host) {
        if (e && e->sum_pool.size() < 4096) e->sum_pool.push_back(df->sum_host);
        else (void)hipHostFree(df->sum_host);
    }
    if (df->arena) {
        if (e && e->arenas.size() < 1024) {
            hipEvent_t fe = nullptr;
            if (in_flight && (fe = sync_event_get(e)) != nullptr && hipEventRecord(fe, e->stream) != hipSuccess) {
                sync_event_put(e, fe);
                fe = nullptr;
            }
            if (in_flight && !fe)
                (void)hipStreamSynchronize(e->stream);           /* no event to be had: wait instead */
            e->arenas.push_back({ df->arena, df->arena_bytes, fe });
        } else {
            if (in_flight) (void)hipStreamSynchronize(e->stream);
            (void)hipFree(df->arena);
            if (e) { e->arenas_alive--; e->arena_bytes_alive -= df->arena_bytes; }
        }
    }
    delete df;
}

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
    if (e->dl_count && getenv("OHEVC_FETCH_TIMING"))
        fprintf(stderr, "ohevc engine: %llu output fetches, per fetch %.2f ms waiting for the picture's passes and its device-to-host copy, %.2f ms moving the rows into the caller's planes\n",
                (unsigned long long)e->dl_count, e->dl_wait_ms / e->dl_count, e->dl_copy_ms / e->dl_count);
    delete e->copiers;
    delete e->dl_copiers;
    for (auto *c : e->dl_stages) { (void)hipEventDestroy(c->done); (void)hipHostFree(c->p); delete c; }
    if (e->kerr) (void)hipHostFree(e->kerr);
    if (e->tickets) (void)hipFree(e->tickets);
    if (e->hash_dev.p) (void)hipFree(e->hash_dev.p);
    if (e->resize_dev.p) (void)hipFree(e->resize_dev.p);
    if (e->colour_dev.p) (void)hipFree(e->colour_dev.p);
    for (auto &ev : e->batch_ev) if (ev) (void)hipEventDestroy(ev);
    if (e->dl_stream) { (void)hipStreamSynchronize(e->dl_stream); (void)hipStreamDestroy(e->dl_stream); }
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    if (e->own_stream)
        (void)hipStreamDestroy(e->stream);
    delete e;
}

/* ---------------- pictures ---------------- */
static int check_params(OhEngine *e, const OhPicParams *p)
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

/* n boundary strengths (0..2, one per byte: hevc_filter.c's vertical_bs / horizontal_bs) -> (n + 3) / 4 bytes, entry i in bits
 * 2 (i & 3) of byte i >> 2 — the form the deblock pass reads.  Four bytes per multiply: the 2-bit fields land in the top byte. */
void pack_bs(uint8_t *dst, const uint8_t *src, size_t n)
{
    size_t i = 0;
    for (; i + 4 <= n; i += 4) {
        uint32_t x;
        memcpy(&x, src + i, 4);
        dst[i >> 2] = (uint8_t)(((x & 0x03030303u) * 0x01041040u) >> 24);
    }
    if (i < n) {
        uint32_t v = 0;
        for (size_t k = i; k < n; k++) v |= (uint32_t)(src[k] & 3) << ((k & 3) * 2);
        dst[i >> 2] = (uint8_t)v;
    }
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
    /* every buffer is busy: beyond OH_MAX_STAGES wait for one whose copy is furthest along instead of pinning more host memory
     * (this is what throttles a host that hands pictures over faster than PCIe and the passes take them) */
    if (e->stages.size() >= OH_MAX_STAGES) {
        for (auto &c : e->stages)
            if (c.busy && c.bytes >= bytes) {
                if (hipEventSynchronize(c.done) != hipSuccess)
                    return nullptr;
                c.busy = false;
                return &c;
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

/* ---------------- work lists ---------------- */
static void fill_planes(DevPlanes *dp, const Pic *p, bool use_b)
{
    for (int c = 0; c < 3; c++) {
        dp->p[c] = use_b ? p->b[c] : p->a[c];
        dp->stride[c] = p->stride[c];
        dp->w[c] = p->w[c];
        dp->h[c] = p->h[c];
    }
}

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
 * ------------------------------------------------------------------------------------------------------------------- */
static int check_host_side(OhEngine *e, const OhFrame *f, const Pic *cur, OhPrepCounts *cnt, uint32_t tu_cnt[4], uint32_t *n_cross,
                           bool *any_dense, uint16_t *ref_used, uint32_t *ref_ok, std::vector<uint32_t> &pu_off)
{
    const OhPicParams &p = f->p;
    *ref_ok = 0; *ref_used = 0; *n_cross = 0; *any_dense = false;
    for (int i = 0; i < OH_MAX_REFS; i++) {
        Pic *r = get_pic(e, f->ref_pics[i]);
        if (r && same_geometry(r->p, p) && r != cur)
            *ref_ok |= 1u << i;
    }
    if ((f->n_pu && !f->pu) || (f->n_wp && !f->wp) || (f->n_tu && !f->tu) || (f->n_intra && !f->intra))
        FAIL(e, OH_E_ARG, "a non-zero item count comes with a NULL array (pu / wp / tu / intra)");
    /* blocks per PU: sizes the MC block lists (prep_pu_scan repeats the sums on the GPU and validates every PU) */
    uint64_t nl = 0, nc = 0;
    const int hs = oh_hshift(&p, 1), vs = oh_vshift(&p, 1), two = p.chroma_format_idc ? 2 : 0;
    if ((uint64_t)f->n_pu * 2048 >= (1ull << 31))
        FAIL(e, OH_E_ARG, "PU list too long");
    pu_off.resize(2 * ((size_t)f->n_pu + 1));
    uint32_t *ol = pu_off.data(), *oc = ol + f->n_pu + 1;       /* running sums: where every PU's blocks start in the two lists */
    for (uint32_t i = 0; i < f->n_pu; i++) {
        const OhPu &pu = f->pu[i];
        ol[i] = (uint32_t)nl; oc[i] = (uint32_t)nc;
        nl += (uint64_t)(((pu.w + 7) >> 3) * ((pu.h + 7) >> 3));
        nc += (uint64_t)(two * ((((pu.w >> hs) + 7) >> 3) * (((pu.h >> vs) + 7) >> 3)));
        for (int l = 0; l < 2; l++)
            if (pu.ref[l] < OH_MAX_REFS) *ref_used |= (uint16_t)(1u << pu.ref[l]);
    }
    ol[f->n_pu] = (uint32_t)nl; oc[f->n_pu] = (uint32_t)nc;
    for (uint32_t i = 0; i < f->n_wp; i++)
        if (f->wp[i].log2_denom[0] > 7 || f->wp[i].log2_denom[1] > 7)
            FAIL(e, OH_E_ARG, "weights %u: log2 denominator out of range", i);
    tu_cnt[0] = tu_cnt[1] = tu_cnt[2] = tu_cnt[3] = 0;
    for (uint32_t i = 0; i < f->n_tu; i++) {                  /* launch sizes of the residual pass; is any block dense? */
        const OhTu &t = f->tu[i];
        tu_cnt[(t.log2_size - 2) & 3]++;
        *n_cross += (t.flags & OH_TUF_CROSS) != 0;
        *any_dense = *any_dense || !(t.flags & OH_TUF_SPARSE);
    }
    if (*any_dense && f->n_coeff && !f->coeffs)
        FAIL(e, OH_E_ARG, "dense transform blocks but coeffs[] is NULL");
    if (*n_cross && !f->tu_cross)
        FAIL(e, OH_E_ARG, "cross-component blocks without tu_cross[]");
    if (f->n_intra && p.constrained_intra_pred && !f->is_intra)
        FAIL(e, OH_E_ARG, "constrained_intra_pred without the is_intra map");
    if (f->n_intra) {
        /* the level table is the contract behind the waits between CTUs (prep_intra_wait: a CTU waits only for lower levels), and
         * prep_intra_ctu looks every entry's level up in it: checked here; everything below it on the GPU */
        if (!f->level_start || !f->n_levels || !f->ictu || !f->n_ictu || !f->sub_start || !f->n_sub ||
            f->level_start[0] != 0 || f->level_start[f->n_levels] != f->n_ictu)
            FAIL(e, OH_E_ARG, "intra wavefront tables inconsistent");
        for (uint32_t l = 0; l < f->n_levels; l++)
            if (f->level_start[l] > f->level_start[l + 1])
                FAIL(e, OH_E_ARG, "intra level table not monotonic");
    }
    if (p.deblock_enabled) {
        const OhBsInputs *bi = f->bs_in;                      /* boundary strengths derived on the GPU instead of handed over */
        if (bi && (!bi->mvf || !bi->cbf_luma || !bi->call_log2 || !bi->ctb_flags))
            FAIL(e, OH_E_ARG, "bs_in: all four maps are required");
        if (bi && (p.log2_min_pu_size < 2 || p.log2_min_tb_size < 2))
            FAIL(e, OH_E_ARG, "bs_in: min PU / TB size below 4");
        if (bi) {
            const size_t n_cells = (size_t)(p.width >> p.log2_min_tb_size) * (p.height >> p.log2_min_tb_size);
            for (size_t i = 0; i < n_cells; i++)
                if (bi->call_log2[i] && (bi->call_log2[i] < p.log2_min_tb_size || bi->call_log2[i] > p.log2_ctb_size))
                    FAIL(e, OH_E_ARG, "bs_in: call_log2[%zu] = %d is not a block size of this picture", i, bi->call_log2[i]);
        }
        if ((!bi && (!f->vertical_bs || !f->horizontal_bs || f->bs_size < oh_bs_size(&p))) || !f->qp_y_tab || !f->deblock)
            FAIL(e, OH_E_ARG, "deblock side arrays missing or too small");
    }
    if ((p.pcm_loop_filter_disable || p.transquant_bypass_enable) && !f->is_pcm)
        FAIL(e, OH_E_ARG, "is_pcm map required when pcm loop-filter disable / transquant bypass is on");
    cnt->n_pu = f->n_pu; cnt->n_mc_luma = (uint32_t)nl; cnt->n_mc_chroma = (uint32_t)nc; cnt->n_tu = f->n_tu;
    cnt->n_intra = f->n_intra; cnt->n_sub = f->n_intra ? f->n_sub : 0; cnt->n_ictu = f->n_intra ? f->n_ictu : 0;
    return OH_OK;
}

/* pinned block the summary of one work list lands in */
static void *summary_block_get(OhEngine *e)
{
    void *p = nullptr;
    if (!e->sum_pool.empty()) { p = e->sum_pool.back(); e->sum_pool.pop_back(); return p; }
    return hipHostMalloc(&p, sizeof(DevSummary), hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

/* the host part of one hand-over and its H2D copy; finish_uploads() enqueues the preparation kernels behind it */
static int upload_one(OhEngine *e, const OhFrame *f, OhDevFrame **out)
{
    *out = nullptr;
    int rc = check_params(e, &f->p);
    if (rc)
        return rc;
    Pic *cur = get_pic(e, f->cur_pic);
    if (!cur || !same_geometry(cur->p, f->p))
        FAIL(e, OH_E_ARG, "cur_pic %d is not an allocated picture of this geometry", f->cur_pic);
    static const bool timing = getenv("OHEVC_UPLOAD_TIMING") != nullptr;      /* diagnostic: where the host time of an upload goes */
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto t_begin = tnow();
    OhPrepCounts cnt;
    uint32_t tu_cnt[4], n_cross = 0, ref_ok = 0;
    uint16_t ref_used = 0;
    bool any_dense = false;
    static thread_local std::vector<uint32_t> pu_off;
    HostTimer t_all(e, OH_HT_UPLOAD);
    { HostTimer t(e, OH_HT_UPLOAD_COUNT);
    rc = check_host_side(e, f, cur, &cnt, tu_cnt, &n_cross, &any_dense, &ref_used, &ref_ok, pu_off);
    }
    if (rc)
        return rc;
    auto t_valid = tnow();
    HIPCHK(e, hipSetDevice(e->device));

    const OhPicParams &p = f->p;
    const size_t n_ctb = (size_t)oh_ctb_width(&p) * oh_ctb_height(&p);
    const size_t n_pcm = (size_t)oh_min_pu_width(&p) * oh_min_pu_height(&p);
    const bool has_sao = p.sao_enabled && f->sao;
    const bool has_db = p.deblock_enabled != 0;

    /* arena: [copied: header, raw lists, side arrays, coefficient pool] [device only: prepared lists, scratch, residual pool] */
    struct Seg { const void *src; size_t bytes, off; size_t pack_n; };     /* pack_n != 0: src holds pack_n boundary strengths, one per byte */
    Seg seg[56];
    int ns = 0;
    size_t total = 0;
    auto add = [&](const void *src, size_t bytes) {
        if (ns >= 56) abort();                                  /* a segment was added without growing seg[] */
        seg[ns].src = src; seg[ns].bytes = bytes; seg[ns].off = total; seg[ns].pack_n = 0;
        total += align_up(bytes ? bytes : 1, 256);
        return ns++;
    };
    DevFrame hd;
    memset(&hd, 0, sizeof(hd));
    int s_hdr = add(&hd, sizeof(DevFrame));
    int s_pu = add(f->pu, (size_t)f->n_pu * sizeof(OhPu));
    int s_puoff = add(pu_off.data(), 2 * ((size_t)f->n_pu + 1) * sizeof(uint32_t));
    int s_wp = add(f->wp, (size_t)f->n_wp * sizeof(OhWeights));
    int s_tur = add(f->tu, (size_t)f->n_tu * sizeof(OhTu));
    int s_tusp = add(f->tu_sparse, f->tu_sparse ? (size_t)f->n_tu * sizeof(uint32_t) : 0);
    int s_tucr = add(f->tu_cross, f->tu_cross ? (size_t)f->n_tu * sizeof(uint32_t) : 0);
    int s_sparse = add(f->sparse, (size_t)(f->sparse ? f->n_sparse : 0) * sizeof(uint32_t));
    int s_scaling = add(f->scaling, f->scaling ? sizeof(OhScalingList) : 0);
    int s_inr = add(f->intra, (size_t)f->n_intra * sizeof(OhIntra));
    int s_ictur = add(cnt.n_ictu ? f->ictu : nullptr, (size_t)cnt.n_ictu * sizeof(OhIntraCtu));
    const uint32_t n_levels = f->n_intra ? f->n_levels : 0;
    int s_lvl = add(n_levels ? f->level_start : nullptr, n_levels ? ((size_t)n_levels + 1) * sizeof(uint32_t) : 0);
    int s_sub = add(cnt.n_sub ? f->sub_start : nullptr, cnt.n_sub ? ((size_t)cnt.n_sub + 1) * sizeof(uint32_t) : 0);
    const bool cip = p.constrained_intra_pred && f->is_intra;
    int s_isin = add(cip ? f->is_intra : nullptr, cip ? n_pcm : 0);
    const OhBsInputs *bsi = has_db ? f->bs_in : nullptr;
    const size_t bs_bytes = bsi ? oh_bs_size(&p) : f->bs_size;
    /* the grids cross PCIe and live in HBM four strengths to the byte (0..2 each: 2 bits) — a megabyte less per 4K picture */
    const size_t bs_packed = (bs_bytes + 3) / 4;
    int s_vbs = add(has_db && !bsi ? f->vertical_bs : nullptr, has_db ? bs_packed : 0);    /* with bs_in: written by bs_kernel after the copy */
    int s_hbs = add(has_db && !bsi ? f->horizontal_bs : nullptr, has_db ? bs_packed : 0);
    const bool bs_packed_in = (f->flags & OH_FRAME_BS_PACKED) != 0;          /* the grids come four to the byte already */
    if (has_db && !bsi && !bs_packed_in) seg[s_vbs].pack_n = seg[s_hbs].pack_n = bs_bytes;
    const size_t n_mtb = (size_t)(p.width >> p.log2_min_tb_size) * (p.height >> p.log2_min_tb_size);
    int s_mvf = add(bsi ? bsi->mvf : nullptr, bsi ? n_pcm * sizeof(OhMvField) : 0);
    int s_cbf = add(bsi ? bsi->cbf_luma : nullptr, bsi ? n_mtb : 0);
    int s_call = add(bsi ? bsi->call_log2 : nullptr, bsi ? n_mtb : 0);
    int s_bsf = add(bsi ? bsi->ctb_flags : nullptr, bsi ? n_ctb : 0);
    int s_qp = add(has_db ? f->qp_y_tab : nullptr, has_db ? oh_qp_tab_size(&p) : 0);
    /* the PCM / bypass map is read by the deblock and SAO passes only under these two flags (hevc_filter.c:180, 337; deblock.hip, sao.hip):
     * without them its half megabyte per 4K picture stays on the host */
    const bool need_pcm = f->is_pcm && (p.pcm_loop_filter_disable || p.transquant_bypass_enable);
    int s_pcm = add(need_pcm ? f->is_pcm : nullptr, need_pcm ? n_pcm : 0);
    int s_db = add(has_db ? f->deblock : nullptr, has_db ? n_ctb * sizeof(OhDeblockCtb) : 0);
    int s_sao = add(has_sao ? f->sao : nullptr, has_sao ? n_ctb * sizeof(OhSaoCtb) : 0);
    const bool has_pend = has_sao && f->sao_pending && oh_sao_stale_config(&p);     /* tiled pictures: the driver order as bits per CTB */
    int s_pend = add(has_pend ? f->sao_pending : nullptr, has_pend ? n_ctb : 0);
    int s_coef = add(f->coeffs, (size_t)f->n_coeff * sizeof(int16_t));
    /* the dense pool is the last copied segment: when every block came as levels nothing of it crosses PCIe */
    const size_t copy_bytes = any_dense || !f->n_tu ? total : seg[s_coef].off;
    /* device only.  The first four are cleared before the preparation kernels run. */
    const size_t zero_off = total;
    int s_cursor = add(nullptr, 16 * sizeof(uint32_t));
    int s_sum = add(nullptr, sizeof(DevSummary));
    int s_seen = add(nullptr, cnt.n_intra ? n_ctb * sizeof(uint32_t) : 0);
    int s_keep = add(nullptr, f->n_tu);
    const size_t zero_bytes = total - zero_off;
    int s_mcl = add(nullptr, (size_t)cnt.n_mc_luma * sizeof(DevMcJob));
    int s_mcc = add(nullptr, (size_t)cnt.n_mc_chroma * sizeof(DevMcJob));
    int s_aux = add(nullptr, (size_t)cnt.n_ictu * sizeof(uint32_t));
    int s_tu = add(nullptr, (size_t)f->n_tu * sizeof(DevTu));
    int s_cross = add(nullptr, (size_t)n_cross * sizeof(DevCross));
    int s_intra = add(nullptr, (size_t)f->n_intra * sizeof(DevIntra));
    int s_ictu = add(nullptr, (size_t)cnt.n_ictu * sizeof(DevIntraCtu));
    int s_small = add(nullptr, (size_t)cnt.n_sub * sizeof(uint32_t));
    int s_perm = add(nullptr, (size_t)f->n_intra * sizeof(uint32_t));
    int s_wait = add(nullptr, (size_t)cnt.n_ictu * 4 * sizeof(uint32_t));
    int s_done = add(nullptr, (size_t)cnt.n_ictu * sizeof(uint32_t));
    int s_clvl = add(nullptr, (size_t)cnt.n_ictu * sizeof(uint32_t));
    int s_cord = add(nullptr, (size_t)cnt.n_ictu * sizeof(uint32_t));
    const size_t res_off = total;
    total += align_up((size_t)(f->n_coeff ? f->n_coeff : 1) * sizeof(int16_t), 256);
    const bool stale_cfg = has_db && has_sao && oh_sao_stale_config(&p);       /* see DevFrame.sao_stale */
    const size_t stale_off = total;
    if (stale_cfg)
        total += align_up(oh_sao_stale_index(&p, 3, 0, 0) * sizeof(uint16_t), 256);

    auto t_lists = tnow();
    bool best_was_new = false;
    OhDevFrame *df = new OhDevFrame();
    {   /* a pooled arena that fits (within 2x), else a new one rounded up to 1 MiB */
        HostTimer t(e, OH_HT_UPLOAD_ARENA);
        /* oldest first (the pool is in release order): an arena released long ago has no pass left that reads it, so the copy
         * need not wait for the engine stream; the most recently released one would stall the copy stream behind the passes
         * of the batch that just let go of it */
        int best = -1;
        best_was_new = false;
        for (size_t i = 0; i < e->arenas.size() && best < 0; i++)
            if (e->arenas[i].bytes >= total && e->arenas[i].bytes <= 2 * total + (1u << 20))
                best = (int)i;
        if (best >= 0 && e->arenas[best].free_ev && hipEventQuery(e->arenas[best].free_ev) != hipSuccess && e->arenas.size() < 512)
            best = -1;                                      /* even the oldest fit is still in flight: a new arena beats a stall */
        if (best >= 0) {
            df->arena = e->arenas[best].p; df->arena_bytes = e->arenas[best].bytes;
            if (e->arenas[best].free_ev) {                  /* released while passes were in flight: the copy must stay behind them */
                (void)hipStreamWaitEvent(e->copy_stream, e->arenas[best].free_ev, 0);
                sync_event_put(e, e->arenas[best].free_ev);
            }
            e->arenas.erase(e->arenas.begin() + best);
        } else {
            best_was_new = true;
            df->arena_bytes = align_up(total, (size_t)1 << 20);
            if (hipMalloc(&df->arena, df->arena_bytes) != hipSuccess) {
                (void)hipStreamSynchronize(e->stream);
                for (auto &a : e->arenas) { sync_event_put(e, a.free_ev); (void)hipFree(a.p); e->arenas_alive--; e->arena_bytes_alive -= a.bytes; }      /* the pool may be what is in the way */
                e->arenas.clear();
                if (hipMalloc(&df->arena, df->arena_bytes) != hipSuccess) {
                    df->arena = nullptr;
                    delete df;
                    FAIL(e, OH_E_NOMEM, "hipMalloc(%zu) for the work list failed", total);
                }
            }
        }
    }
    if (best_was_new) { e->arenas_alive++; e->arena_bytes_alive += df->arena_bytes; }
    char *base = (char *)df->arena;
    hd.pp = p;
    fill_planes(&hd.cur, cur, false);
    fill_planes(&hd.out, cur, has_sao);
    for (int i = 0; i < OH_MAX_REFS; i++) {
        Pic *r = get_pic(e, f->ref_pics[i]);
        df->ref_id[i] = -1; df->ref_gen[i] = 0; df->ref_half[i] = 0;
        if (ref_ok >> i & 1) {
            fill_planes(&hd.refs[i], r, r->final_b);
            df->ref_id[i] = f->ref_pics[i]; df->ref_gen[i] = r->gen; df->ref_half[i] = r->final_b ? 1 : 0;
        }
    }
    df->ref_used = ref_used;
    df->cur_gen = cur->gen;
#define AT(T, s) ((T)(base + seg[s].off))
    hd.pu = AT(const OhPu *, s_pu);
    hd.mc_luma = AT(const DevMcJob *, s_mcl); hd.mc_chroma = AT(const DevMcJob *, s_mcc);
    hd.wp = AT(const OhWeights *, s_wp);
    hd.tu = AT(const DevTu *, s_tu); hd.tu_raw = AT(const OhTu *, s_tur);
    hd.tu_sparse = f->tu_sparse ? AT(const uint32_t *, s_tusp) : nullptr;
    hd.tu_cross = f->tu_cross ? AT(const uint32_t *, s_tucr) : nullptr;
    hd.sparse = f->sparse ? AT(const uint32_t *, s_sparse) : nullptr;
    hd.cross = AT(const DevCross *, s_cross);
    hd.scaling = f->scaling ? AT(const OhScalingList *, s_scaling) : nullptr;
    hd.coeffs = AT(const int16_t *, s_coef);
    hd.coeffs_present = f->coeffs != nullptr;
    hd.res = (int16_t *)(base + res_off);
    hd.sao_stale = stale_cfg ? (uint16_t *)(base + stale_off) : nullptr;
    hd.intra = AT(const DevIntra *, s_intra); hd.intra_raw = AT(const OhIntra *, s_inr);
    hd.ictu = AT(const DevIntraCtu *, s_ictu); hd.ictu_raw = AT(const OhIntraCtu *, s_ictur);
    hd.sub_start = AT(const uint32_t *, s_sub);
    hd.sub_small = AT(const uint32_t *, s_small); hd.sub_small_w = AT(uint32_t *, s_small);
    hd.lvl_start = AT(const uint32_t *, s_lvl);
    hd.is_intra = cip ? AT(const uint8_t *, s_isin) : nullptr;
    hd.vbs = AT(const uint8_t *, s_vbs); hd.hbs = AT(const uint8_t *, s_hbs);
    hd.qp = AT(const int8_t *, s_qp);
    hd.is_pcm = need_pcm ? AT(const uint8_t *, s_pcm) : nullptr;
    hd.db = AT(const OhDeblockCtb *, s_db);
    hd.sao = has_sao ? AT(const OhSaoCtb *, s_sao) : nullptr;
    hd.sao_pending = has_pend ? AT(const uint8_t *, s_pend) : nullptr;
    hd.pu_off = AT(const uint32_t *, s_puoff); hd.ctu_aux = AT(uint32_t *, s_aux); hd.tu_keep = AT(uint8_t *, s_keep); hd.tu_cursor = AT(uint32_t *, s_cursor);
    hd.intra_perm = AT(uint32_t *, s_perm); hd.ctu_seen = AT(uint32_t *, s_seen); hd.summary = AT(void *, s_sum);
    hd.ctu_wait = AT(uint32_t *, s_wait); hd.ctu_done = AT(uint32_t *, s_done); hd.ctu_lvl = AT(uint32_t *, s_clvl); hd.ctu_order = AT(uint32_t *, s_cord);
    hd.err_word = e->kerr; hd.cur_pic_id = f->cur_pic;
#undef AT
    hd.n_pu = f->n_pu; hd.n_mc_luma = cnt.n_mc_luma; hd.n_mc_chroma = cnt.n_mc_chroma; hd.n_tu = f->n_tu; hd.n_intra = f->n_intra;
    hd.n_ictu = cnt.n_ictu; hd.n_sub = cnt.n_sub; hd.n_levels = n_levels; hd.n_wp = f->n_wp; hd.n_sparse = f->sparse ? f->n_sparse : 0;
    hd.ref_ok = ref_ok; hd.n_coeff = f->n_coeff;
    hd.n_cross = n_cross;
    hd.zero_ptr = (uint32_t *)(base + zero_off); hd.zero_words = (uint32_t)(zero_bytes / 4);
    for (int k = 0, first = 0; k < 4; k++) { hd.tu_first[k] = (uint32_t)first; hd.tu_cnt[k] = tu_cnt[k]; first += (int)tu_cnt[k]; }
    hd.dbg = e->dbg;
    (void)s_hdr;

    /* stage everything in one host buffer -> one H2D copy; a list that lies in pinned memory (OH_FRAME_PINNED) is copied by DMA from
     * where it lies, segment by segment: only what this function made itself (the header, the PU block offsets) is staged */
    auto t_alloc = tnow();
    const bool direct = (f->flags & OH_FRAME_PINNED) != 0 && !(has_db && !bsi && !bs_packed_in);     /* byte grids still have to be packed on the way */
    const size_t own_bytes = align_up(sizeof(DevFrame), 256) + align_up(2 * ((size_t)f->n_pu + 1) * sizeof(uint32_t), 256) + 64 * sizeof(OhPullSeg);
    OhEngine::Stage *sg;
    { HostTimer t(e, OH_HT_UPLOAD_STAGE_WAIT);
    sg = stage_acquire(e, direct ? own_bytes : copy_bytes);   /* a pinned buffer whose previous copy has completed */
    }
    df->sum_host = summary_block_get(e);
    hd.summary_host = df->sum_host;                        /* pinned, device-accessible: prep_finish stores the summary there */
    if (!sg || !df->sum_host) {
        free_dev_frame(e, df);
        FAIL(e, OH_E_NOMEM, "hipHostMalloc(%zu) failed", copy_bytes);
    }
    void *stage = sg->p;
    hipStream_t cs = e->copy_stream;
    hipError_t hrc = hipSuccess;
    if (direct) {
        /* the GPU pulls the list: the two segments made here (header, PU block offsets) and the table of segments stand in the staging
         * buffer, every other segment is read from the caller's pinned memory where it lies — ONE kernel launch (prep_pull), no host
         * copy of the lists and no DMA request per array (fifteen of those per picture cost the host as much as the copy they replaced) */
        OhPullSeg *tab;
        int nt = 0;
        size_t pulled = 0;
        { HostTimer t(e, OH_HT_UPLOAD_MEMCPY);
        char *sp = (char *)stage;
        memcpy(sp, seg[s_hdr].src, seg[s_hdr].bytes);
        char *po = sp + align_up(sizeof(DevFrame), 256);
        if (seg[s_puoff].bytes) memcpy(po, seg[s_puoff].src, seg[s_puoff].bytes);
        tab = (OhPullSeg *)(po + align_up(seg[s_puoff].bytes, 256));
        tab[nt++] = OhPullSeg{ sp, (char *)df->arena, seg[s_hdr].bytes };
        if (seg[s_puoff].bytes) tab[nt++] = OhPullSeg{ po, (char *)df->arena + seg[s_puoff].off, seg[s_puoff].bytes };
        for (int i = 0; i < ns; i++)
            if (i != s_hdr && i != s_puoff && seg[i].bytes && seg[i].src && seg[i].off + seg[i].bytes <= copy_bytes) {
                tab[nt++] = OhPullSeg{ seg[i].src, (char *)df->arena + seg[i].off, seg[i].bytes };
                pulled += seg[i].bytes;
            }
        }
        HostTimer t_enq(e, OH_HT_UPLOAD_ENQUEUE);
        ohk_pull(tab, nt, pulled, cs);
        hrc = hipGetLastError();
    } else {
        { HostTimer t(e, OH_HT_UPLOAD_MEMCPY);
        if (!e->copiers) {
            static const char *cenv = getenv("OHEVC_COPY_THREADS");
            e->copiers = new CopyPool();
            e->copiers->start(cenv ? std::max(0, std::min(atoi(cenv), 8)) : 2);
        }
        /* pieces of at most 128 KB, dealt round-robin to the calling thread and the helpers */
        std::vector<CopyJob> &jobs = e->copy_jobs;
        jobs.clear();
        const size_t piece = 128 * 1024;
        for (int i = 0; i < ns; i++)
            if (seg[i].bytes && seg[i].src && seg[i].off + seg[i].bytes <= copy_bytes) {
                if (seg[i].pack_n) {                                      /* four source bytes per byte: pieces of 4 x 128 KB strengths */
                    for (size_t o = 0; o < seg[i].pack_n; o += 4 * piece)
                        jobs.push_back({ (char *)stage + seg[i].off + o / 4, (const char *)seg[i].src + o, std::min(4 * piece, seg[i].pack_n - o), true });
                } else {
                    for (size_t o = 0; o < seg[i].bytes; o += piece)
                        jobs.push_back({ (char *)stage + seg[i].off + o, (const char *)seg[i].src + o, std::min(piece, seg[i].bytes - o), false });
                }
            }
        e->copiers->run(jobs);
        }
        /* asynchronous: the caller's arrays are already copied out; the pinned buffer stays busy until `done` */
        HostTimer t_enq(e, OH_HT_UPLOAD_ENQUEUE);
        hrc = hipMemcpyAsync(df->arena, stage, copy_bytes, hipMemcpyHostToDevice, cs);
    }
    HostTimer t_enq(e, OH_HT_UPLOAD_ENQUEUE);
    if (hrc == hipSuccess)
        hrc = hipEventRecord(sg->done, cs);
    sg->busy = hrc == hipSuccess;
    e->up_bytes += copy_bytes;
    if (hrc == hipSuccess && bsi) {                        /* both grids from the maps: once per work list, the maps never change */
        hrc = hipMemsetAsync(base + seg[s_vbs].off, 0, align_up(bs_packed, 4), cs);          /* bs_kernel ORs the non-zero strengths in; the padded tail is read by the deblock pass */
        if (hrc == hipSuccess) hrc = hipMemsetAsync(base + seg[s_hbs].off, 0, align_up(bs_packed, 4), cs);
        if (hrc == hipSuccess)
            ohk_bs_derive(&p, base + seg[s_mvf].off, base + seg[s_cbf].off, base + seg[s_call].off, base + seg[s_bsf].off, bsi->loop_filter_across_tiles,
                          base + seg[s_vbs].off, base + seg[s_hbs].off, cs);
    }
    df->sum_dev = base + seg[s_sum].off;
    df->cnt = cnt;
    if (hrc != hipSuccess) {
        (void)hipStreamSynchronize(cs);
        free_dev_frame(e, df);
        FAIL(e, OH_E_HIP, "work-list upload failed: %s", hipGetErrorString(hrc));
    }
    if (timing) {
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        auto t_end = tnow();
        fprintf(stderr, "oh_frame_upload: host checks + counting %.3f ms, layout %.3f ms, arena %.3f ms, staging copy + enqueue %.3f ms (%zu bytes)\n",
                ms(t_begin, t_valid), ms(t_valid, t_lists), ms(t_lists, t_alloc), ms(t_alloc, t_end), copy_bytes);
    }
    df->d = (DevFrame *)base;
    df->p = p;
    for (int k = 0; k < 4; k++) df->tu_cnt[k] = tu_cnt[k];
    df->n_cross = n_cross;
    df->has_sao = has_sao;
    df->cur_pic = f->cur_pic;                  /* which half of cur_pic is final changes when the list is EXECUTED, not here */
    df->owner = e;
    *out = df;
    return OH_OK;
}

/* preparation kernels of n freshly copied work lists (one set of launches per 32 of them: the kernels pick the list with a grid
 * dimension, like the passes), their summaries back to pinned memory, their `ready` events */
static int finish_uploads(OhEngine *e, OhDevFrame *const *dfs, int n)
{
    HostTimer t_enq(e, OH_HT_UPLOAD_ENQUEUE);
    hipStream_t cs = e->copy_stream;
    for (int c0 = 0; c0 < n; c0 += OH_MAX_BATCH) {
        const int nb = n - c0 < OH_MAX_BATCH ? n - c0 : OH_MAX_BATCH;
        OhBatch B;
        memset(&B, 0, sizeof(B));
        OhPrepCounts mx;
        memset(&mx, 0, sizeof(mx));
        uint32_t max_cross = 0, max_runs = 0;
        for (int i = 0; i < nb; i++) {
            const OhDevFrame *df = dfs[c0 + i];
            B.f[i] = df->d;
            mx.n_pu = std::max(mx.n_pu, df->cnt.n_pu); mx.n_tu = std::max(mx.n_tu, df->cnt.n_tu);
            mx.n_intra = std::max(mx.n_intra, df->cnt.n_intra); mx.n_sub = std::max(mx.n_sub, df->cnt.n_sub);
            mx.n_ictu = std::max(mx.n_ictu, df->cnt.n_ictu);
            max_runs = std::max(max_runs, ((df->cnt.n_mc_luma + 63) >> 6) + ((df->cnt.n_mc_chroma + 63) >> 6));
            max_cross = std::max(max_cross, df->n_cross);
        }
        ohk_prepare(&B, nb, &mx, max_runs, max_cross, cs);
        HIPCHK(e, hipGetLastError());
    }
    /* one point in the copy stream makes all of them ready: an event per list, recorded back to back */
    for (int i = 0; i < n; i++) {
        OhDevFrame *df = dfs[i];
        if ((df->ready = sync_event_get(e)) == nullptr)
            FAIL(e, OH_E_NOMEM, "no event for the work list");
        HIPCHK(e, hipEventRecord(df->ready, cs));
    }
    return OH_OK;
}

extern "C" int oh_frames_upload(OhEngine *e, const OhFrame *const *fs, int n, OhDevFrame **out)
{
    if (!e || n < 0 || (n && (!fs || !out)))
        return OH_E_ARG;
    for (int i = 0; i < n; i++) out[i] = nullptr;
    int rc = OH_OK;
    int done = 0;
    for (; done < n && rc == OH_OK; done++)
        rc = fs[done] ? upload_one(e, fs[done], &out[done]) : OH_E_ARG;
    if (rc == OH_OK)
        rc = finish_uploads(e, out, n);
    if (rc != OH_OK) {                                     /* all or nothing */
        (void)hipStreamSynchronize(e->copy_stream);
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

/* the summary the preparation kernels left (prep.hip): waits for the list's `ready` event the first time */
static int read_summary(OhEngine *e, OhDevFrame *df, int index)
{
    if (df->summary_read)
        return df->prep_err ? OH_E_ARG : OH_OK;
    { HostTimer t(e, OH_HT_EXECUTE_WAIT_PREP);
    HIPCHK(e, hipEventSynchronize(df->ready));
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

/* the CTUs' residual spans staged in LDS, or every block fetching its own from the pool one sub-level ahead (intra.hip: slots_prepare)?
 * Staging costs ~11 KB of LDS per workgroup in a launch that holds one all-intra CTU, i.e. workgroups per CU (OHEVC_INTRA_RES_LDS=0 / 1
 * forces one way: experiments) */
static bool res_in_lds(const OhEngine *e, uint64_t workgroups)
{
    static const char *env = getenv("OHEVC_INTRA_RES_LDS");
    if (env) return atoi(env) != 0;
    /* a launch of at most a workgroup per CU is latency-bound: stage (a 4K I picture alone 6.6 ms against 7.0); any wider one runs at
     * workgroups-per-CU x latency: keep the LDS small (all-intra batches 39.8 against 37.6 Gpix/s, the mixed bench +0.6 %) */
    return workgroups <= (uint64_t)e->n_cu;
}

/* The intra pass of a batch (intra.hip), one launch per form:
 *   direct  a wave per CTU working on the picture in HBM — pictures whose intra blocks cover less than half of their samples
 *           (B / P pictures);
 *   dag     a workgroup per CTU with the CTU staged in LDS — the others (I pictures).
 * OHEVC_INTRA_MODE=dag / direct forces one form for every picture.  A CTU takes the schedule entry of the ticket it draws when it
 * starts and waits only for lower tickets, so the launch drains whatever the dispatch order; a wait that gives up anyway (bounded by
 * OHEVC_SPIN_LIMIT) is reported by kernel_error. */
static int intra_pass(OhEngine *e, OhDevFrame *const *fr, int nb, const OhBatch *all, hipStream_t st)
{
    const OhPicParams *p = &fr[0]->p;
    static const char *menv = getenv("OHEVC_INTRA_MODE");
    const bool force_dag = menv && !strcmp(menv, "dag"), force_direct = menv && !strcmp(menv, "direct");
    OhBatch bd, bs;                                  /* direct / staged dag */
    memset(&bd, 0, sizeof(bd)); memset(&bs, 0, sizeof(bs));
    int nd = 0, ns = 0;
    uint32_t max_ictu_d = 0, max_ictu_s = 0, max_ictu_all = 0, max_items = 1, max_sub = 1, max_res = 0;
    uint64_t sum_items = 0, sum_sub = 0, total_entries = 0;
    bool staged = true;
    const uint64_t pic_samples64 = ((uint64_t)p->width * p->height * (p->chroma_format_idc == 0 ? 2 : p->chroma_format_idc == 1 ? 3 : p->chroma_format_idc == 2 ? 4 : 6) / 2) >> 6;
    for (int i = 0; i < nb; i++) {
        if (!fr[i]->cnt.n_ictu)
            continue;
        max_ictu_all = std::max(max_ictu_all, fr[i]->cnt.n_ictu);
        const bool sparse = force_direct || (!force_dag && (uint64_t)fr[i]->intra_area64 * 2 < pic_samples64);
        if (sparse) {
            bd.f[nd++] = fr[i]->d;
            max_ictu_d = std::max(max_ictu_d, fr[i]->cnt.n_ictu);
            continue;
        }
        bs.f[ns++] = fr[i]->d;
        max_ictu_s = std::max(max_ictu_s, fr[i]->cnt.n_ictu);
        total_entries += fr[i]->cnt.n_ictu;
        const OhDevFrame &d = *fr[i];
        max_items = std::max(max_items, d.max_items); max_sub = std::max(max_sub, d.max_sub); max_res = std::max(max_res, d.max_res);
        sum_items += d.sum_items; sum_sub += d.sum_sub;
        staged = staged && !d.res_scattered;
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
        ohk_intra_direct(&bd, nd, p, max_ictu_d, tk, e->spin_limit, st);
    if (ns) {
        OhIntraLaunch IL;
        /* residual spans in LDS only while the chip holds the whole launch (a picture alone); else the blocks fetch theirs a sub-level ahead */
        IL.staged = staged && res_in_lds(e, total_entries / 8);
        /* waves per CTU: as many as blocks run side by side in a sub-level (more only hold LDS and wave slots); a small batch cannot
         * fill the chip anyway: spend the waves on the single picture's latency (OHEVC_INTRA_WAVES forces them: experiments) */
        static const char *wenv = getenv("OHEVC_INTRA_WAVES");
        const double par = sum_sub ? (double)sum_items / (double)sum_sub : 1.0;
        IL.waves = wenv ? (uint32_t)atoi(wenv) : par > (nb < 8 ? 2.5 : 4.5) ? 8 : par > 1.25 ? 4 : 2;
        if (IL.waves != 2 && IL.waves != 4 && IL.waves != 8) IL.waves = 8;
        /* sub-levels go round-robin to `phases` groups of waves (intra.hip): a group prepares its next sub-level while another
         * finishes its own, so at least two */
        static const char *penv = getenv("OHEVC_INTRA_PHASES");
        IL.phases = penv ? (uint32_t)atoi(penv) : 2u;
        if (IL.phases < 2 || IL.phases > IL.waves || IL.waves % IL.phases) IL.phases = 2;
        const OhCtuAreas areas = oh_ctu_areas(p->log2_ctb_size, p->chroma_format_idc);
        size_t off = align_up((size_t)areas.total * sizeof(uint16_t), 16);
        IL.off_items = (uint32_t)off; off += (size_t)max_items * sizeof(DevIntra);
        IL.off_sub = (uint32_t)off;   off += ((size_t)max_sub + 1) * sizeof(uint32_t);
        IL.off_small = (uint32_t)off; off = align_up(off + (size_t)max_sub * sizeof(uint32_t), 16);
        IL.off_res = (uint32_t)off;   off = align_up(off + (size_t)(IL.staged ? max_res : 0) * sizeof(int16_t), 16);
        IL.off_wave = (uint32_t)off;  off += (size_t)IL.waves * OH_INTRA_WAVE_LDS;
        IL.lds_bytes = (uint32_t)off;
        ohk_intra_dag(&bs, ns, p, &IL, max_ictu_s, tk + OH_MAX_BATCH * 32, e->spin_limit, st);
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
    HIPCHK(e, hipSetDevice(e->device));
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
            if (!df->waited) {                              /* the list's copy runs on the copy stream */
                HIPCHK(e, hipStreamWaitEvent(st, df->ready, 0));
                df->waited = true;
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
            HIPCHK(e, hipEventRecord(sg->done, st));
            sg->busy = true;
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
    if (df->ready)
        HIPCHK(e, hipEventSynchronize(df->ready));          /* never executed: its copy may still be running */
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
    if (!df->waited && df->ready)
        HIPCHK(e, hipStreamWaitEvent(e->stream, df->ready, 0));      /* never executed: the release still has to stay behind its copy */
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
    if (df->ready)
        HIPCHK(e, hipEventSynchronize(df->ready));          /* the list arrives on the copy stream */
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
