/*
 * engine_pics.hip — the host side of what the engine does with finished pictures beside the reconstruction path: plane upload and
 * download, the two-phase window fetch, and the picture services, one section each below with its kernel file and its part of DESIGN.md.
 * Their arithmetic, which needs neither an engine nor a device, is pics_math.hip; the helpers at the top are what the services share.
 */
#include <cmath>
#include "engine_impl.h"
#include "pics_math.h"
#include "grain_common.h"

/* at least `bytes` of device scratch, grow-only in 1 MiB steps.  Growing frees the old block: the caller has made sure that nothing
 * enqueued still uses it. */
static int scratch_reserve(OhEngine *e, OhEngine::Scratch *s, size_t bytes)
{
    if (bytes <= s->bytes)
        return OH_OK;
    if (s->p) (void)hipFree(s->p);
    s->p = nullptr; s->bytes = 0;
    const size_t want = align_up(bytes, (size_t)1 << 20);
    HIPCHK(e, hipMalloc(&s->p, want));
    s->bytes = want;
    return OH_OK;
}

/* the first of n pictures (ids checked) whose params differ from those of the first; n: all are equal */
static int first_other_params(OhEngine *e, const int *pic_ids, int n)
{
    for (int i = 1; i < n; i++)
        if (memcmp(&get_pic(e, pic_ids[i])->p, &get_pic(e, pic_ids[0])->p, sizeof(OhPicParams)))
            return i;
    return n;
}

/* ---------------- what the services share ---------------- */
/* a check of pics_math.hip that said `why`: rc, OH_OK included, with the message set where it is a refusal */
static int refuse(OhEngine *e, int rc, const char *who, const char *why)
{
    if (rc)
        FAIL(e, rc, "%s: %s", who, why);
    return OH_OK;
}
static int refuse(OhEngine *e, int rc, const char *who, const std::string &why) { return refuse(e, rc, who, why.c_str()); }

/* the n pictures of a call in launch sets of at most per_set: set(i0, m) fills in the m pictures from i0 on and launches */
template <typename Set> static int launch_sets(OhEngine *e, int n, Set set, int per_set = OH_CONV_MAX_PICS)
{
    for (int i0 = 0; i0 < n; i0 += per_set) {
        set(i0, std::min(n - i0, per_set));
        HIPCHK(e, hipGetLastError());
    }
    return OH_OK;
}

/* `bytes` that fill(pinned block) writes, in device scratch s in front of the launches that follow: staged in a pinned buffer of the pool
 * and copied on the engine stream, behind the launches of an earlier call that read the device copy.  Growing the scratch frees the old
 * block: a caller whose earlier launches may still use it has waited for them.  what: the block, for the refusal */
template <typename Fill> static int upload(OhEngine *e, const char *who, const char *what, OhEngine::Scratch *s, size_t bytes, Fill fill)
{
    OH_TRY(scratch_reserve(e, s, bytes));
    OhEngine::Stage *sg = stage_acquire(e, bytes);
    if (!sg)
        FAIL(e, OH_E_NOMEM, "%s: no staging buffer for %zu bytes of %s", who, bytes, what);
    fill(sg->p);
    HIPCHK(e, hipMemcpyAsync(s->p, sg->p, bytes, hipMemcpyHostToDevice, e->stream));
    return stage_in_use(e, sg, e->stream);
}

static int upload_copy(OhEngine *e, const char *who, const char *what, OhEngine::Scratch *s, size_t bytes, const void *block)
{
    return upload(e, who, what, s, bytes, [=](void *h) { memcpy(h, block, bytes); });
}

/* the first of n pictures that are known and all have its params; nullptr: they are not (OH_E_ARG, the message set) */
static const Pic *alike_pics(OhEngine *e, const char *who, const int *pic_ids, int n)
{
    if (check_pics(e, pic_ids, n, who))
        return nullptr;
    const int other = first_other_params(e, pic_ids, n);
    if (other < n)
        FAIL(e, nullptr, "%s: picture %d has other params than picture %d", who, pic_ids[other], pic_ids[0]);
    return get_pic(e, pic_ids[0]);
}

/* the destinations of a call in rising order (what its search for a picture that is also a source takes); none may be listed twice */
static int distinct_dsts(OhEngine *e, const char *who, const int *dst_ids, int n, std::vector<int> *sorted)
{
    *sorted = std::vector<int>(dst_ids, dst_ids + n);
    std::sort(sorted->begin(), sorted->end());
    if (std::adjacent_find(sorted->begin(), sorted->end()) != sorted->end())
        FAIL(e, OH_E_ARG, "%s: a destination is listed twice", who);
    return OH_OK;
}

/* no destination is listed twice and none is among the sources */
static int dsts_apart(OhEngine *e, const char *who, const int *dst_ids, int nd, const int *src_ids, int ns)
{
    int both = 0;
    switch (ids_apart(dst_ids, nd, src_ids, ns, &both)) {
    case 1: FAIL(e, OH_E_ARG, "%s: a destination is listed twice", who);
    case 2: FAIL(e, OH_E_ARG, "%s: picture %d is both source and destination", who, both);
    }
    return OH_OK;
}

/* the pictures of index i in time: around[0][i] before and around[1][i] after own_ids[i] (`own`: what the call names it), where a null
 * array or an entry of -1 stands for the picture itself; srcs: every source of the call.  used: the mode reads them at all */
struct Neighbours { std::vector<int> around[2], srcs; };
static int neighbours(OhEngine *e, const char *who, const char *own, const int *prev_ids, const int *own_ids, const int *next_ids, int n,
                      bool used, Neighbours *nb)
{
    const int *const ids[2] = { prev_ids, next_ids };
    int side = 0;
    const int bad = neighbours_resolve(ids, own_ids, n, used, nb->around, &nb->srcs, &side);
    if (bad >= 0)
        FAIL(e, OH_E_ARG, "%s: %s picture %d (-1 stands for the %s picture)", who, side ? "next" : "prev", ids[side][bad], own);
    return OH_OK;
}

/* sources and n destinations of one kind: all known and alike, the destinations apart.  The first source, or nullptr (OH_E_ARG) */
static const Pic *alike_apart(OhEngine *e, const char *who, const std::vector<int> &srcs, const int *dst_ids, int n)
{
    std::vector<int> all(srcs);
    all.insert(all.end(), dst_ids, dst_ids + n);
    const Pic *p0 = alike_pics(e, who, all.data(), (int)all.size());
    if (!p0 || dsts_apart(e, who, dst_ids, n, srcs.data(), (int)srcs.size()))
        return nullptr;
    return p0;
}

/* ns sources and nd destinations whose params may differ: the sources known and alike, then the destinations, then the destinations
 * apart.  *s0, *d0: the first of each side.  The engine's device is the current one from here on */
static int srcs_dsts(OhEngine *e, const char *who, const int *src_ids, int ns, const int *dst_ids, int nd, const Pic **s0, const Pic **d0)
{
    if (!(*s0 = alike_pics(e, who, src_ids, ns)) || !(*d0 = alike_pics(e, who, dst_ids, nd)))
        return OH_E_ARG;
    OH_TRY(dsts_apart(e, who, dst_ids, nd, src_ids, ns));
    HIPCHK(e, hipSetDevice(e->device));
    return OH_OK;
}

/* pictures `as` of params a and `bs` of params b (the nouns of the refusal) that a call takes only in one bit depth and chroma format */
static int same_format(OhEngine *e, const char *who, const char *as, const OhPicParams &a, const char *bs, const OhPicParams &b)
{
    if (a.bit_depth != b.bit_depth || a.chroma_format_idc != b.chroma_format_idc)
        FAIL(e, OH_E_UNSUPPORTED, "%s: %s of %d bit, chroma format %d; %s of %d bit, chroma format %d (oh_pics_reformat first)", who, as,
             a.bit_depth, a.chroma_format_idc, bs, b.bit_depth, b.chroma_format_idc);
    return OH_OK;
}

/* a picture's geometry as the kernels take it: planes (1 or 3), bytes between the rows of the first np planes, and the coded size of
 * the plane classes (0 luma, 1 chroma) that np planes have.  What a helper does not set stays as the caller cleared it */
static int n_planes(const OhPicParams &p) { return p.chroma_format_idc ? 3 : 1; }

static void row_pitches(const Pic *p, int np, int32_t pitch[3])
{
    for (int c = 0; c < np; c++) pitch[c] = p->stride[c] * sample_bytes(p->p.bit_depth);
}

static void class_sizes(const Pic *p, int np, int32_t w[2], int32_t h[2])
{
    for (int q = 0; q < (np > 1 ? 2 : 1); q++) { w[q] = p->w[q]; h[q] = p->h[q]; }
}

/* the planes of a picture that a launch reads: its finished half, null from plane np on */
template <typename P> static void read_planes(const Pic *p, int np, P planes[3])
{
    for (int c = 0; c < 3; c++) planes[c] = c < np ? final_planes(p)[c] : nullptr;
}

/* the planes of a picture that a launch writes: half 0, which holds the finished picture from here on, and no reconstruction batch
 * made it: a download stays behind the engine stream.  Called per launch set, after every check of the call, in front of the launch */
static void write_planes(Pic *p, int np, void *planes[3])
{
    for (int c = 0; c < 3; c++) planes[c] = c < np ? p->a[c] : nullptr;
    p->final_b = false;
    p->done_seq = 0;
}

/* the bytes from ptr to the end of its allocation; ROOM_NONE: ptr is not device memory of the engine's device (the current one);
 * ROOM_UNKNOWN: it is, but the runtime cannot tell its extent — callers let such memory pass */
enum : size_t { ROOM_NONE = 0, ROOM_UNKNOWN = ~(size_t)0 };
static size_t device_room(OhEngine *e, const void *ptr)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != e->device) {
        (void)hipGetLastError();
        return ROOM_NONE;
    }
    void *base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ptr)) == hipSuccess)
        return (size_t)((const char *)base + size - (const char *)ptr);
    (void)hipGetLastError();
    return ROOM_UNKNOWN;
}

/* the caller's images (`what`: "dst" or "src"): n of ib bytes, image_stride apart, of sb-byte samples, in `bytes` bytes of device memory at p */
static int image_run_check(OhEngine *e, const char *who, const char *what, const void *p, int n, size_t ib, size_t sb, size_t image_stride, size_t bytes)
{
    if (image_stride < ib || image_stride % sb || (uintptr_t)p % sb)
        FAIL(e, OH_E_ARG, "%s: image_stride %zu (an image takes %zu bytes) or %s not a multiple of the %zu-byte sample", who, image_stride, ib, what, sb);
    if (!p || ib > bytes || (size_t)(n - 1) > (bytes - ib) / image_stride)
        FAIL(e, OH_E_ARG, "%s: %d images of %zu bytes, %zu apart, do not fit %zu bytes", who, n, ib, image_stride, bytes);
    const size_t total = (size_t)(n - 1) * image_stride + ib;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t room = device_room(e, p);
    if (room == ROOM_NONE)
        FAIL(e, OH_E_ARG, "%s: %s is not device memory of device %d", who, what, e->device);
    if (room != ROOM_UNKNOWN && total > room)
        FAIL(e, OH_E_ARG, "%s: %zu bytes at %s run past the end of its allocation", who, total, what);
    return OH_OK;
}

/* what a conversion kernel takes of the pictures' layout (all alike: p0) and of the OhConvert's window and chroma filter */
static void conv_args(OhConvArgs *a, const Pic *p0, const OhConvert *cv)
{
    const OhPicParams &p = p0->p;
    row_pitches(p0, 3, a->pitch);
    a->cw = p0->w[1]; a->ch = p0->h[1];
    a->left = cv->win.left; a->top = cv->win.top;
    window_size(&p, cv->win, &a->W, &a->H);
    a->cf = p.chroma_format_idc; a->bd = p.bit_depth; a->filter = cv->chroma_filter;
}

/* the first n_entries table entries of col in tc's device copy, in front of the launches that follow: built on the host unless col is the
 * cache's last, then staged in a pinned buffer and copied on the engine stream — behind earlier launches that read the device copy */
static int table_stage(OhEngine *e, OhEngine::TableCache *tc, const OhColour *col, int n_entries, const char *who)
{
    if (!tc->cached || memcmp(&tc->last, col, sizeof(*col))) {
        tc->cached = false;
        tc->tab.resize((size_t)OH_COLT_N);
        std::string why;
        OH_TRY(refuse(e, colour_build(col, tc->tab.data(), tc->misc, &why), who, why));
        tc->last = *col; tc->cached = true; tc->on_dev = false;
    }
    if (!tc->on_dev)                                            /* a cache always asks for as many entries: the device copy never grows */
        OH_TRY(upload_copy(e, who, n_entries == OH_COLT_N ? "tables" : "table", &tc->dev, (size_t)n_entries * sizeof(int32_t), tc->tab.data()));
    tc->on_dev = true;
    return OH_OK;
}

/* the results of a call that ends with a wait.  begin: `bytes` of device scratch in s (the old buffer is idle), cleared on the engine stream
 * in front of the launches, and a pinned buffer; fetch: the copy into it, the one stream wait, and what a kernel that gave up has latched */
static int results_begin(OhEngine *e, const char *who, OhEngine::Scratch *s, size_t bytes, int n, OhEngine::Stage **sg)
{
    OH_TRY(scratch_reserve(e, s, bytes));
    *sg = stage_acquire(e, bytes);
    if (!*sg)
        FAIL(e, OH_E_NOMEM, "%s: no staging buffer for %d results", who, n);
    HIPCHK(e, hipMemsetAsync(s->p, 0, bytes, e->stream));
    return OH_OK;
}

static int results_fetch(OhEngine *e, const OhEngine::Scratch *s, size_t bytes, OhEngine::Stage *sg)
{
    HIPCHK(e, hipMemcpyAsync(sg->p, s->p, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return kernel_error(e);
}

extern "C" int oh_pic_upload(OhEngine *e, int pic_id, const uint8_t *const planes[3], const ptrdiff_t strides[3])
{
    if (!e || !planes || !strides)
        return OH_E_ARG;
    Pic *p = get_pic(e, pic_id);
    if (!p)
        FAIL(e, OH_E_ARG, "oh_pic_upload: unknown picture %d", pic_id);
    HIPCHK(e, hipSetDevice(e->device));
    const size_t bpp = sample_bytes(p->p.bit_depth);
    for (int c = 0; c < (p->p.chroma_format_idc ? 3 : 1); c++)
        HIPCHK(e, hipMemcpy2DAsync(p->a[c], (size_t)p->stride[c] * bpp, planes[c], (size_t)strides[c], (size_t)p->w[c] * bpp,
                                   (size_t)p->h[c], hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    p->final_b = false;
    p->done_seq = 0;
    return OH_OK;
}

extern "C" int oh_pic_download(OhEngine *e, int pic_id, uint8_t *const planes[3], const ptrdiff_t strides[3])
{
    if (!e || !planes || !strides)
        return OH_E_ARG;
    Pic *p = get_pic(e, pic_id);
    if (!p)
        FAIL(e, OH_E_ARG, "oh_pic_download: unknown picture %d", pic_id);
    HIPCHK(e, hipSetDevice(e->device));
    const size_t bpp = sample_bytes(p->p.bit_depth);
    for (int c = 0; c < (p->p.chroma_format_idc ? 3 : 1); c++)
        HIPCHK(e, hipMemcpy2DAsync(planes[c], (size_t)strides[c], final_planes(p)[c], (size_t)p->stride[c] * bpp,
                                   (size_t)p->w[c] * bpp, (size_t)p->h[c], hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    OH_TRY(kernel_error(e));     /* a kernel that gave up: these samples are not the picture */
    return OH_OK;
}

/* Output side of the path: the conformance-window crop of ff_hevc_output_frame (hevc_refs.c:248-254:
 * plane pointers advanced by (left >> hshift, top >> vshift)) followed by libOpenHevcGetOutputCpy's packed row copies
 * (openHevcWrapper.c:353-398: `height >> vshift` rows of `(width >> hshift) << pixel_shift` bytes, width / height = the cropped
 * size).  One strided device-to-pinned copy per plane, one wait, then the rows go to the caller's pitches. */
/* The output fetch in two halves, for a decoder whose threads share ONE engine behind a lock (the drop-in library: frame-thread
 * workers hand pictures over while the application's thread fetches the one that was released):
 *   oh_pic_download_start   (under the caller's engine lock, microseconds) validates, takes a pinned DOWNLOAD staging buffer — a list
 *                           of its own, guarded by its own mutex — and enqueues the strided device-to-host copies behind the batch
 *                           that finished the picture (download stream), then records an event;
 *   oh_download_finish      (NO engine lock needed, any thread) waits for that event, copies the rows into the caller's planes with
 *                           the download copy helpers, and gives the staging buffer back.
 * oh_pic_download_window is the two in a row. */
struct OhDownload {
    OhEngine::Stage *sg;
    size_t row[3], rows[3], off[3];
    int np;
};

extern "C" int oh_pic_download_start(OhEngine *e, int pic_id, const OhWindow *win, OhDownload **out)
{
    if (!e || !win || !out)
        return OH_E_ARG;
    *out = nullptr;
    Pic *p = get_pic(e, pic_id);
    if (!p)
        FAIL(e, OH_E_ARG, "oh_pic_download_window: unknown picture %d", pic_id);
    std::string why;
    if (!crop_window_ok(&p->p, *win, false, &why))
        FAIL(e, OH_E_ARG, "oh_pic_download_window: %s", why.c_str());
    int W, H;
    window_size(&p->p, *win, &W, &H);
    HIPCHK(e, hipSetDevice(e->device));
    const size_t bpp = sample_bytes(p->p.bit_depth);
    OhDownload d;
    d.np = n_planes(p->p);
    size_t total = 0;
    for (int c = 0; c < d.np; c++) {
        const int hs = oh_hshift(&p->p, c), vs = oh_vshift(&p->p, c);
        d.row[c] = (size_t)(W >> hs) * bpp; d.rows[c] = (size_t)(H >> vs);
        d.off[c] = total; total += align_up(d.row[c] * d.rows[c], 256);
    }
    {   /* a free download buffer that fits, else a new one (a decoder has one or two fetches in flight) */
        std::lock_guard<std::mutex> lk(e->dl_mu);
        d.sg = nullptr;
        for (auto *c : e->dl_stages)
            if (!c->busy && c->bytes >= total && (!d.sg || c->bytes < d.sg->bytes)) d.sg = c;
        if (!d.sg) {
            OhEngine::Stage *c = new OhEngine::Stage();
            if (!stage_create(c, total)) {
                delete c;
                FAIL(e, OH_E_NOMEM, "hipHostMalloc(%zu) failed", total);
            }
            e->dl_stages.push_back(c);
            d.sg = c;
        }
        d.sg->busy = true;
    }
    /* a picture a batch of this engine finished, and whose event is still in the ring: the copies run on the download stream behind
     * THAT batch; anything else (uploaded, up-sampled, received from another GPU, long ago): behind everything on the engine stream */
    hipStream_t dl = e->stream;
    if (p->done_seq && e->batch_seq - p->done_seq < OhEngine::BATCH_RING - 1) {
        if (!e->dl_stream) HIPCHK(e, hipStreamCreateWithFlags(&e->dl_stream, hipStreamNonBlocking));
        HIPCHK(e, hipStreamWaitEvent(e->dl_stream, e->batch_ev[p->done_seq % OhEngine::BATCH_RING], 0));
        dl = e->dl_stream;
    }
    hipError_t he = hipSuccess;
    for (int c = 0; c < d.np && he == hipSuccess; c++) {
        const int hs = oh_hshift(&p->p, c), vs = oh_vshift(&p->p, c);
        const uint8_t *src = (const uint8_t *)final_planes(p)[c] + ((size_t)(win->top >> vs) * p->stride[c] + (size_t)(win->left >> hs)) * bpp;
        he = hipMemcpy2DAsync((char *)d.sg->p + d.off[c], d.row[c], src, (size_t)p->stride[c] * bpp, d.row[c], d.rows[c], hipMemcpyDeviceToHost, dl);
    }
    if (he == hipSuccess) he = hipEventRecord(d.sg->done, dl);
    if (he != hipSuccess) {
        std::lock_guard<std::mutex> lk(e->dl_mu);
        d.sg->busy = false;
        FAIL(e, OH_E_HIP, "oh_pic_download_window: %s", hipGetErrorString(he));
    }
    *out = new OhDownload(d);
    return OH_OK;
}

extern "C" int oh_download_finish(OhEngine *e, OhDownload *d, uint8_t *const planes[3], const ptrdiff_t strides[3])
{
    if (!e || !d)
        return OH_E_ARG;
    int rc = OH_OK;
    if (!planes || !strides)
        rc = OH_E_ARG;
    for (int c = 0; c < d->np && !rc; c++)
        if (!planes[c] || (ptrdiff_t)d->row[c] > strides[c])
            rc = OH_E_ARG;
    const auto t_w0 = std::chrono::steady_clock::now();
    const hipError_t he = hipEventSynchronize(d->sg->done);    /* also when the arguments are bad: the buffer goes back only after its copy */
    const auto t_w1 = std::chrono::steady_clock::now();
    if (!rc && he != hipSuccess) rc = OH_E_HIP;
    if (!rc) rc = kernel_error(e);                             /* a kernel that gave up: these samples are not the picture */
    if (!rc) {
        std::lock_guard<std::mutex> lk(e->dl_copy_mu);         /* one fetch at a time uses the helpers */
        if (!e->dl_copiers) {
            e->dl_copiers = new CopyPool();
            e->dl_copiers->start(e->tuning.fetch_threads);
        }
        /* pieces of at most 1 MiB (packed planes) or single rows (pitched planes), dealt round-robin to the helpers and this thread */
        std::vector<CopyJob> &jobs = e->dl_jobs;
        jobs.clear();
        for (int c = 0; c < d->np; c++) {
            const char *src = (const char *)d->sg->p + d->off[c];
            if ((size_t)strides[c] == d->row[c]) {
                const size_t n = d->row[c] * d->rows[c], piece = (size_t)1 << 20;
                for (size_t o = 0; o < n; o += piece) jobs.push_back(CopyJob{ (char *)planes[c] + o, src + o, n - o < piece ? n - o : piece, false });
            } else {
                for (size_t y = 0; y < d->rows[c]; y++) jobs.push_back(CopyJob{ (char *)planes[c] + (ptrdiff_t)y * strides[c], src + y * d->row[c], d->row[c], false });
            }
        }
        e->dl_copiers->run(jobs);
        e->dl_wait_ms += std::chrono::duration<double, std::milli>(t_w1 - t_w0).count();
        e->dl_copy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_w1).count();
        e->dl_count++;
    }
    {
        std::lock_guard<std::mutex> lk(e->dl_mu);
        d->sg->busy = false;
    }
    delete d;
    return rc;
}

extern "C" int oh_pic_download_window(OhEngine *e, int pic_id, const OhWindow *win, uint8_t *const planes[3], const ptrdiff_t strides[3])
{
    if (!e || !win || !planes || !strides)
        return OH_E_ARG;
    OhDownload *d = nullptr;
    const int rc = oh_pic_download_start(e, pic_id, win, &d);
    if (rc)
        return rc;
    const int rc2 = oh_download_finish(e, d, planes, strides);
    if (rc2 == OH_E_ARG)
        FAIL(e, OH_E_ARG, "oh_pic_download_window: a destination plane is missing or its pitch is smaller than a row");
    if (rc2 == OH_E_HIP)
        FAIL(e, OH_E_HIP, "oh_pic_download_window: the device-to-host copy failed");
    return rc2;
}

/* the planes of n pictures (ids checked) as hash jobs, the half that holds the final samples; slot[i * 3 + c]: the job of plane c of
 * picture i, -1 for the planes a monochrome picture lacks.  Returns the number of jobs. */
static int plane_jobs(OhEngine *e, const int *pic_ids, int n, OhMd5Job *jobs, int *slot)
{
    int nj = 0;
    for (int i = 0; i < n; i++) {
        const Pic *p = get_pic(e, pic_ids[i]);
        const uint32_t bpp = sample_bytes(p->p.bit_depth);
        for (int c = 0; c < 3; c++) {
            slot[i * 3 + c] = -1;
            if (c && !p->p.chroma_format_idc)
                continue;
            OhMd5Job &j = jobs[nj];
            j.base = final_planes(p)[c];
            j.pitch = (uint32_t)p->stride[c] * bpp; j.row_bytes = (uint32_t)p->w[c] * bpp; j.rows = (uint32_t)p->h[c]; j.bps = bpp;
            slot[i * 3 + c] = nj++;
        }
    }
    return nj;
}

/* Picture hash on the GPU: the three plane digests of the reference's SEI check (hevc.c:4146-4162 over calc_md5,
 * hevc.c:4623-4638: the whole coded planes, sps->width x sps->height and the chroma sizes, packed rows) for n finished pictures in one
 * launch of one chain per (picture, plane) — md5.hip.  48 bytes per picture come back instead of the picture.  Waits for the engine
 * stream.  digests: n x 3 x 16 bytes (monochrome: planes 1, 2 zero).  pic_ids checked. */
static int pics_md5(OhEngine *e, const int *pic_ids, int n, uint8_t *digests)
{
    HIPCHK(e, hipSetDevice(e->device));
    const size_t jobs_bytes = align_up((size_t)n * 3 * sizeof(OhMd5Job), 256);
    OhEngine::Stage *sg = stage_acquire(e, jobs_bytes + (size_t)n * 48);
    if (!sg)
        FAIL(e, OH_E_NOMEM, "hipHostMalloc for %d picture hashes failed", n);
    OhMd5Job *jobs = (OhMd5Job *)sg->p;
    uint8_t *out = (uint8_t *)sg->p + jobs_bytes;
    std::vector<int> slot((size_t)n * 3);
    const int nj = plane_jobs(e, pic_ids, n, jobs, slot.data());
    ohk_md5(jobs, nj, out, e->stream);                        /* pinned host memory is mapped: the kernel reads the jobs and writes the digests there */
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    OH_TRY(kernel_error(e));     /* a kernel that gave up: these samples are not the picture */
    for (size_t k = 0; k < slot.size(); k++) {
        if (slot[k] >= 0) memcpy(digests + k * 16, out + (size_t)slot[k] * 16, 16);
        else memset(digests + k * 16, 0, 16);
    }
    return OH_OK;
}

extern "C" int oh_pics_md5(OhEngine *e, const int *pic_ids, int n, uint8_t *digests)
{
    if (!e || n < 0 || (n && (!pic_ids || !digests)))
        return OH_E_ARG;
    if (!n)
        return OH_OK;
    OH_TRY(check_pics(e, pic_ids, n, "oh_pics_md5"));
    return pics_md5(e, pic_ids, n, digests);
}

/* CRC (kind 1) or checksum (kind 2) of every plane of n pictures (ids checked): vals[i * 3 + c], 0 for planes a monochrome picture
 * lacks.  hash.hip: one workgroup per OH_HASH_TASK bytes of every plane in one launch, then one per plane to combine.  The job table
 * and the task list are staged in pinned memory and copied to HBM in one piece; the values come back through the pinned buffer. */
static int pics_crc_checksum(OhEngine *e, const int *pic_ids, int n, int kind, uint32_t *vals)
{
    HIPCHK(e, hipSetDevice(e->device));
    std::vector<int> slot((size_t)n * 3);
    std::vector<OhMd5Job> jv((size_t)n * 3);
    const int nj = plane_jobs(e, pic_ids, n, jv.data(), slot.data());
    std::vector<uint32_t> first((size_t)nj + 1, 0);
    for (int k = 0; k < nj; k++) {
        const uint64_t bytes = (uint64_t)jv[k].row_bytes * jv[k].rows;
        first[k + 1] = first[k] + (uint32_t)((bytes + OH_HASH_TASK - 1) / OH_HASH_TASK);
    }
    const uint32_t nt = first[nj];
    const size_t o_first = align_up((size_t)nj * sizeof(OhMd5Job), 256), o_map = o_first + align_up(((size_t)nj + 1) * 4, 256),
                 o_part = o_map + align_up((size_t)nt * 8, 256), dev_bytes = o_part + align_up((size_t)nt * 4, 256);
    OH_TRY(scratch_reserve(e, &e->hash_dev, dev_bytes));    /* every call ends with a wait: the old buffer is idle */
    OhEngine::Stage *sg = stage_acquire(e, o_part + (size_t)nj * 4);
    if (!sg)
        FAIL(e, OH_E_NOMEM, "hipHostMalloc for %d picture hashes failed", n);
    char *h = (char *)sg->p, *d = (char *)e->hash_dev.p;
    memcpy(h, jv.data(), (size_t)nj * sizeof(OhMd5Job));
    memcpy(h + o_first, first.data(), ((size_t)nj + 1) * 4);
    uint32_t *map = (uint32_t *)(h + o_map);
    for (int k = 0; k < nj; k++)
        for (uint32_t t = first[k]; t < first[k + 1]; t++) { map[2 * t] = (uint32_t)k; map[2 * t + 1] = t - first[k]; }
    uint32_t *out = (uint32_t *)(h + o_part);                 /* pinned and mapped: the combine kernel writes the plane values there */
    HIPCHK(e, hipMemcpyAsync(d, h, o_part, hipMemcpyHostToDevice, e->stream));
    ohk_hash(kind, (const OhMd5Job *)d, (const uint32_t *)(d + o_first), (const uint32_t *)(d + o_map), nj, (int)nt, (uint32_t *)(d + o_part), out,
             e->stream);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    OH_TRY(kernel_error(e));
    for (size_t k = 0; k < slot.size(); k++)
        vals[k] = slot[k] >= 0 ? out[slot[k]] : 0;
    return OH_OK;
}

extern "C" int oh_pics_hash(OhEngine *e, const int *pic_ids, int n, int hash_type, OhPictureHash *out)
{
    if (!e || n < 0 || (n && (!pic_ids || !out)))
        return OH_E_ARG;
    if (hash_type < 0 || hash_type > 2)
        FAIL(e, OH_E_ARG, "oh_pics_hash: hash_type %d (0 MD5, 1 CRC, 2 checksum)", hash_type);
    if (!n)
        return OH_OK;
    OH_TRY(check_pics(e, pic_ids, n, "oh_pics_hash"));
    std::vector<uint32_t> v((size_t)n * 12);                  /* per picture: MD5 three 16-byte digests, else three values */
    uint8_t *dg = (uint8_t *)v.data();
    OH_TRY(hash_type == 0 ? pics_md5(e, pic_ids, n, dg) : pics_crc_checksum(e, pic_ids, n, hash_type, v.data()));
    for (int i = 0; i < n; i++) {
        memset(&out[i], 0, sizeof(out[i]));
        out[i].present = 1; out[i].hash_type = hash_type;
        if (hash_type == 0) memcpy(out[i].md5, dg + (size_t)i * 48, 48);
        else memcpy(hash_type == 1 ? out[i].crc : out[i].checksum, &v[(size_t)i * 3], 3 * sizeof(uint32_t));
    }
    return OH_OK;
}

/* ---------------- conversion to standard images (convert.hip) ---------------- */
/* oh_pics_convert and oh_pics_convert_colour (col set: its tables are staged in front of the launches, which are colour.hip's) */
static int pics_convert(OhEngine *e, const char *who, const int *pic_ids, int n, const OhConvert *cv, const OhColour *col, void *dst,
                        size_t image_stride, size_t dst_bytes)
{
    const Pic *p0 = alike_pics(e, who, pic_ids, n);
    if (!p0) return OH_E_ARG;
    size_t ib = 0;
    std::string why;
    OH_TRY(refuse(e, conv_check(&p0->p, cv, &ib, &why), who, why));
    OH_TRY(image_run_check(e, who, "dst", dst, n, ib, (size_t)conv_sample_bytes(cv, p0->p.bit_depth), image_stride, dst_bytes));
    OhColArgs ca;
    OhConvArgs &a = ca.c;
    memset(&ca, 0, sizeof(ca));
    conv_args(&a, p0, cv);
    a.nc = cv->format == OH_CONV_RGBA ? 4 : 3;
    a.image_stride = image_stride;
    if (cv->format >= OH_CONV_RGB_PLANAR) {
        OhConvert k16 = *cv;
        if (col) k16.sample = OH_CONV_U16;                      /* the colour stages start from the 16-bit R'G'B' */
        OH_TRY(refuse(e, oh_convert_coeffs(&k16, a.bd, a.k, OH_CONV_NCOEFFS), who, "no coefficients for this conversion"));
    }
    if (col) {
        OH_TRY(table_stage(e, &e->colour_tabs, col, OH_COLT_N, who));
        ca.tab = (const int32_t *)e->colour_tabs.dev.p;
        memcpy(ca.misc, e->colour_tabs.misc, sizeof(ca.misc));
    }
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) read_planes(get_pic(e, pic_ids[i0 + i]), n_planes(p0->p), a.src[i]);
        a.dst = (char *)dst + (size_t)i0 * image_stride;
        if (col) ohk_colour(&ca, cv->format, cv->sample, m, e->stream);
        else     ohk_convert(&a, cv->format, cv->sample, m, e->stream);
    });
}

extern "C" int oh_pics_convert(OhEngine *e, const int *pic_ids, int n, const OhConvert *cv, void *dst, size_t image_stride, size_t dst_bytes)
{
    if (!e || n < 0 || !cv || (n && !pic_ids))
        return OH_E_ARG;
    if (!n)
        return OH_OK;
    return pics_convert(e, "oh_pics_convert", pic_ids, n, cv, nullptr, dst, image_stride, dst_bytes);
}

/* ---------------- import of standard images (import.hip) ---------------- */
extern "C" int oh_pics_import(OhEngine *e, const int *pic_ids, int n, const OhConvert *cv, const void *src, size_t image_stride, size_t src_bytes)
{
    const char *who = "oh_pics_import";
    if (!e || n < 0 || !cv || (n && !pic_ids))
        return OH_E_ARG;
    if (!n)
        return OH_OK;
    const Pic *p0 = alike_pics(e, who, pic_ids, n);
    if (!p0) return OH_E_ARG;
    OH_TRY(dsts_apart(e, who, pic_ids, n, nullptr, 0));
    size_t ib = 0;
    std::string why;
    OH_TRY(refuse(e, conv_check(&p0->p, cv, &ib, &why), who, why));
    OH_TRY(image_run_check(e, who, "src", src, n, ib, (size_t)conv_sample_bytes(cv, p0->p.bit_depth), image_stride, src_bytes));
    OhImpArgs a;
    memset(&a, 0, sizeof(a));
    const OhPicParams &p = p0->p;
    const int np = n_planes(p);
    row_pitches(p0, np, a.pitch);
    class_sizes(p0, np, a.pw, a.ph);
    a.left = cv->win.left; a.top = cv->win.top;
    window_size(&p, cv->win, &a.W, &a.H);
    a.cf = p.chroma_format_idc; a.bd = p.bit_depth; a.filter = cv->chroma_filter;
    a.nc = cv->format == OH_CONV_RGBA ? 4 : 3;
    a.image_stride = image_stride;
    if (cv->format >= OH_CONV_RGB_PLANAR)
        OH_TRY(refuse(e, oh_import_coeffs(cv, p.bit_depth, a.k, OH_IMPORT_NCOEFFS), who, "no coefficients for this conversion"));
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) write_planes(get_pic(e, pic_ids[i0 + i]), np, a.dst[i]);
        a.src = (const char *)src + (size_t)i0 * image_stride;
        ohk_import(&a, cv->format, cv->sample, m, e->stream);
    });
}

/* ---------------- colour conversion (colour.hip) ---------------- */
extern "C" int oh_pics_convert_colour(OhEngine *e, const int *pic_ids, int n, const OhConvert *cv, const OhColour *col, void *dst,
                                      size_t image_stride, size_t dst_bytes)
{
    if (!e || n < 0 || !cv || !col || (n && !pic_ids))
        return OH_E_ARG;
    std::string why;
    OH_TRY(refuse(e, colour_check(col, &why), "oh_pics_convert_colour", why));
    if (cv->format >= OH_CONV_PLANAR && cv->format <= OH_CONV_SEMIPLANAR)
        FAIL(e, OH_E_UNSUPPORTED, "oh_pics_convert_colour: format %d is a YUV format", cv->format);
    if (col->out_transfer == OH_COL_LINEAR && (cv->sample == OH_CONV_U8 || cv->sample == OH_CONV_U16))
        FAIL(e, OH_E_UNSUPPORTED, "oh_pics_convert_colour: OH_COL_LINEAR takes F16 or F32 samples");
    if (!n)
        return OH_OK;
    return pics_convert(e, "oh_pics_convert_colour", pic_ids, n, cv, col, dst, image_stride, dst_bytes);
}

/* ---------------- light-level statistics (light.hip) ---------------- */
/* the OhColour whose table A and luminance weights the light-level pass uses.  Neither depends on src_peak; HLG is built with 1000
 * nits so that a peak outside what oh_pics_convert_colour takes for its OOTF passes colour_check */
static OhColour light_colour(const OhLightSpec *sp)
{
    OhColour c;
    memset(&c, 0, sizeof(c));
    c.in_transfer = sp->in_transfer;
    c.in_primaries = c.out_primaries = sp->in_primaries;
    c.out_transfer = OH_COL_LINEAR; c.tone = OH_TONE_NONE; c.norm = OH_NORM_LUMA;
    c.src_peak = c.white = sp->in_transfer == 18 ? 1000.0f : sp->src_peak;
    c.dst_peak = 100.0f;
    return c;
}

extern "C" int oh_pics_light_level(OhEngine *e, const int *pic_ids, int n, const OhConvert *cv, const OhLightSpec *sp, OhLightLevel *out)
{
    const char *who = "oh_pics_light_level";
    if (!e || n < 0 || !cv || !sp || !out || (n && !pic_ids))
        return OH_E_ARG;
    if (sp->norm < OH_NORM_MAXRGB || sp->norm > OH_NORM_LUMA)
        FAIL(e, OH_E_ARG, "%s: norm %d outside its list", who, sp->norm);
    if (!std::isfinite(sp->src_peak) || !(sp->src_peak > 0))
        FAIL(e, OH_E_ARG, "%s: src_peak is finite and positive", who);
    const OhColour col = light_colour(sp);
    std::string why;
    OH_TRY(refuse(e, colour_check(&col, &why) ? OH_E_UNSUPPORTED : OH_OK, who, why));
    if (!n)
        return OH_OK;
    const Pic *p0 = alike_pics(e, who, pic_ids, n);
    if (!p0) return OH_E_ARG;
    OhConvert k16 = *cv;                                        /* format and sample are not the caller's to set: the 16-bit R'G'B' */
    k16.format = OH_CONV_RGB; k16.sample = OH_CONV_U16;
    size_t ib = 0;
    OH_TRY(refuse(e, conv_check(&p0->p, &k16, &ib, &why), who, why));
    HIPCHK(e, hipSetDevice(e->device));
    OhLightArgs la;
    OhConvArgs &a = la.c;
    memset(&la, 0, sizeof(la));
    conv_args(&a, p0, cv);
    OH_TRY(refuse(e, oh_convert_coeffs(&k16, a.bd, a.k, OH_CONV_NCOEFFS), who, "no coefficients for this conversion"));
    la.luma = sp->norm == OH_NORM_LUMA;
    /* table A alone, in a cache of its own; the call ends with a wait, so no launch reads the device copy while it changes */
    { const int rc = table_stage(e, &e->light_tabs, &col, OH_COLT_G, who); if (rc) return rc == OH_E_ARG ? OH_E_UNSUPPORTED : rc; }
    la.tab = (const int32_t *)e->light_tabs.dev.p;
    for (int j = 0; j < 3; j++) la.w[j] = e->light_tabs.misc[9 + j];
    const size_t bytes = (size_t)n * sizeof(OhLightDev);
    OhEngine::Stage *sg = nullptr;
    OH_TRY(results_begin(e, who, &e->light_res, bytes, n, &sg));
    OH_TRY(launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) read_planes(get_pic(e, pic_ids[i0 + i]), n_planes(p0->p), a.src[i]);
        la.res = (OhLightDev *)e->light_res.p + i0;
        ohk_light(&la, m, e->stream);
    }));
    OH_TRY(results_fetch(e, &e->light_res, bytes, sg));
    const OhLightDev *r = (const OhLightDev *)sg->p;
    for (int i = 0; i < n; i++) {
        out[i].pixels = (uint64_t)a.W * (uint64_t)a.H;
        out[i].sum = r[i].sum;
        out[i].max = r[i].max; out[i].min = ~r[i].not_min;
        memcpy(out[i].hist, r[i].hist, sizeof(out[i].hist));
    }
    return OH_OK;
}

/* ---------------- comparison of two pictures (compare.hip) ---------------- */
extern "C" int oh_pics_compare(OhEngine *e, const int *a_ids, const int *b_ids, int n, const OhCompareSpec *sp, OhCompare *out)
{
    const char *who = "oh_pics_compare";
    if (!e || n < 0 || !sp || !out || (n && (!a_ids || !b_ids)))
        return OH_E_ARG;
    if (sp->flags & ~OH_CMP_SSIM)
        FAIL(e, OH_E_ARG, "%s: flags %#x: OH_CMP_SSIM is the only one", who, (unsigned)sp->flags);
    if (!n)
        return OH_OK;
    std::vector<int> all(a_ids, a_ids + n);
    all.insert(all.end(), b_ids, b_ids + n);
    const Pic *p0 = alike_pics(e, who, all.data(), 2 * n);
    if (!p0) return OH_E_ARG;
    const OhPicParams &p = p0->p;
    std::string why;
    if (!crop_window_ok(&p, sp->win, true, &why))
        return refuse(e, OH_E_ARG, who, why);
    HIPCHK(e, hipSetDevice(e->device));
    OhCmpArgs a;
    memset(&a, 0, sizeof(a));
    const int np = n_planes(p);
    row_pitches(p0, np, a.pitch);
    for (int c = 0; c < (np > 1 ? 2 : 1); c++) {
        OhCmpClass &k = a.k[c];
        class_window(&p, sp->win, c, &k.x0, &k.y0, &k.w, &k.h);
        k.tx = std::max(1, ((k.w >> 2) + OH_CMP_TW / 4 - 1) / (OH_CMP_TW / 4));
        k.ty = std::max(1, ((k.h >> 2) + OH_CMP_TH / 4 - 1) / (OH_CMP_TH / 4));
    }
    a.np = np; a.bd = p.bit_depth; a.ssim = (sp->flags & OH_CMP_SSIM) != 0;
    const size_t bytes = (size_t)n * 3 * OH_CMP_SLOTS * sizeof(OhCmpDev);
    OhEngine::Stage *sg = nullptr;
    OH_TRY(results_begin(e, who, &e->compare_res, bytes, n, &sg));
    OH_TRY(launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, a_ids[i0 + i]), np, a.a[i]);
            read_planes(get_pic(e, b_ids[i0 + i]), np, a.b[i]);
        }
        a.res = (OhCmpDev *)e->compare_res.p + (size_t)i0 * 3 * OH_CMP_SLOTS;
        ohk_compare(&a, m, e->stream);
    }));
    OH_TRY(results_fetch(e, &e->compare_res, bytes, sg));
    const OhCmpDev *r = (const OhCmpDev *)sg->p;
    for (int i = 0; i < n; i++) {
        memset(&out[i], 0, sizeof(out[i]));
        for (int c = 0; c < 3; c++) {
            OhPlaneDiff &d = out[i].plane[c];
            d.first_x = d.first_y = OH_CMP_NONE;
            if (c >= np)
                continue;
            const OhCmpClass &k = a.k[c != 0];
            uint32_t not_first = 0;
            uint64_t ssim_sum = 0;
            for (int s = 0; s < OH_CMP_SLOTS; s++) {            /* the slots the tiles added into */
                const OhCmpDev &v = r[((size_t)i * 3 + c) * OH_CMP_SLOTS + s];
                d.differing += v.differing; d.sad += v.sad; d.sse += v.sse; ssim_sum += v.ssim_sum;
                d.max_abs = std::max(d.max_abs, v.max_abs); not_first = std::max(not_first, v.not_first);
            }
            d.samples = (uint64_t)k.w * (uint64_t)k.h;
            if (not_first) {
                const uint32_t key = ~not_first;
                d.first_x = key % (uint32_t)k.w; d.first_y = key / (uint32_t)k.w;
            }
            if (a.ssim) {
                d.ssim_windows = (uint64_t)std::max((k.w >> 2) - 1, 0) * (uint64_t)std::max((k.h >> 2) - 1, 0);
                d.ssim_sum = (int64_t)ssim_sum;
            }
        }
    }
    return OH_OK;
}

/* ---------------- resizing into engine pictures (resize.hip) ---------------- */
namespace {
struct ResizeAxis { std::vector<int32_t> first, cnt; std::vector<int16_t> k; int mt = 0; };
/* what a call works out per plane class (0 luma, 1 chroma) beside its OhResizeClass: the taps of both axes, the quads of the horizontal
 * pass, the row groups of the vertical pass, and where each table lies in the blob of `tab` bytes that goes to the device */
struct ResizePlan {
    int ncls = 0;
    ResizeAxis hx[2], vx[2];
    std::vector<int32_t> h_f4[2], h_n4[2], v_lo[2], v_np[2], v_off[2];
    size_t off[2][9] = {}, tab = 0;                             /* h_first, h_cnt, h_k, v_first, v_cnt, v_off, v_k, h_f4, h_n4 */
};
}

static int resize_axis(int S, int T, int filter, int phase, ResizeAxis *ax)
{
    ax->mt = oh_resize_max_taps(S, T, filter);
    if (ax->mt < 1) return OH_E_ARG;
    ax->first.resize((size_t)T); ax->cnt.resize((size_t)T); ax->k.resize((size_t)T * ax->mt);
    return oh_resize_taps(S, T, filter, phase, ax->first.data(), ax->k.data(), ax->mt, ax->cnt.data());
}

/* what oh_pics_resize checks of its arguments (n > 0, the lists present); *s0, *d0: the first source and destination */
static int resize_check(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhResize *rs, const Pic **s0, const Pic **d0)
{
    OH_TRY(srcs_dsts(e, "oh_pics_resize", src_ids, n, dst_ids, n, s0, d0));
    const OhPicParams &sp = (*s0)->p, &dp = (*d0)->p;
    if (rs->filter != OH_RESIZE_BILINEAR && rs->filter != OH_RESIZE_BICUBIC)
        FAIL(e, OH_E_ARG, "oh_pics_resize: filter %d (0 bilinear, 1 bicubic)", rs->filter);
    const int cf = sp.chroma_format_idc, hs = cf == 1 || cf == 2, vs = cf == 1, sw = 1 << hs, sv = 1 << vs;
    std::string why;
    if (!crop_window_ok(&sp, rs->win, true, &why))
        return refuse(e, OH_E_ARG, "oh_pics_resize", why);
    /* the size rules read the SOURCES' chroma format: a destination of another format is refused below */
    if (rs->width < 1 || rs->height < 1 || rs->width > dp.width || rs->height > dp.height || rs->width % sw || rs->height % sv)
        FAIL(e, OH_E_ARG, "oh_pics_resize: image %dx%d: below 1, above the destination's %dx%d, or not multiples of %dx%d", rs->width, rs->height,
             dp.width, dp.height, sw, sv);
    if (dp.bit_depth != sp.bit_depth || dp.chroma_format_idc != cf)
        FAIL(e, OH_E_UNSUPPORTED, "oh_pics_resize: destinations of %d bit, chroma format %d; sources of %d bit, chroma format %d", dp.bit_depth,
             dp.chroma_format_idc, sp.bit_depth, cf);
    int W, H;
    window_size(&sp, rs->win, &W, &H);
    for (int c = 0; c < (cf ? 2 : 1); c++) {
        const int64_t ext[4] = { W >> (c ? hs : 0), rs->width >> (c ? hs : 0), H >> (c ? vs : 0), rs->height >> (c ? vs : 0) };
        for (int a = 0; a < 4; a += 2)
            if (ext[a] > OH_RESIZE_MAX_DOWN * ext[a + 1] || ext[a + 1] > OH_RESIZE_MAX_UP * ext[a])
                FAIL(e, OH_E_UNSUPPORTED, "oh_pics_resize: %d -> %d samples is outside %d:1 .. 1:%d", (int)ext[a], (int)ext[a + 1], OH_RESIZE_MAX_DOWN,
                     OH_RESIZE_MAX_UP);
    }
    return OH_OK;
}

/* the geometry of every plane class from the first source and destination (all pictures of a call are alike): *a but for the device
 * pointers and the pictures, *pl with the contents and the layout of the tables */
static int resize_plan(OhEngine *e, const Pic *s0, const Pic *d0, const OhResize *rs, OhResizeArgs *a, ResizePlan *pl)
{
    const OhPicParams &sp = s0->p;
    const OhWindow &w = rs->win;
    const int bpp = sample_bytes(sp.bit_depth);
    memset(a, 0, sizeof(*a));
    a->np = n_planes(sp); a->bd = sp.bit_depth;
    pl->ncls = a->np > 1 ? 2 : 1;
    uint64_t mid_pic = 0;
    for (int c = 0; c < pl->ncls; c++) {
        OhResizeClass &k = a->k[c];
        const ResizeAxis &hx = pl->hx[c], &vx = pl->vx[c];
        const int hs = oh_hshift(&sp, c), vs = oh_vshift(&sp, c);
        int32_t Sw, Sh;
        class_window(&sp, w, c, &k.x0, &k.y0, &Sw, &Sh);
        k.sh = Sh;
        k.tw = rs->width >> hs; k.th = rs->height >> vs;
        k.cw = d0->w[c]; k.ch = d0->h[c];
        k.src_pitch = s0->stride[c] * bpp; k.dst_pitch = d0->stride[c] * bpp;
        k.mid_stride = (int32_t)align_up((size_t)k.tw + 1, 64);
        int rc = resize_axis(Sw, k.tw, rs->filter, c && hs ? 1 : 2, &pl->hx[c]);
        if (!rc) rc = resize_axis(Sh, k.th, rs->filter, 2, &pl->vx[c]);
        if (rc) FAIL(e, rc, "oh_pics_resize: no taps for %dx%d -> %dx%d", Sw, Sh, k.tw, k.th);
        /* horizontal pass: the widest power-of-two segment whose source columns fit a staged row, then as many rows as fit the LDS */
        int span = 0;
        for (k.segw = 256; ; k.segw >>= 1) {
            span = 0;
            for (int x = 0; x < k.tw; x += k.segw) {
                const int xl = std::min(x + k.segw, k.tw) - 1;
                span = std::max(span, hx.first[xl] + hx.cnt[xl] - hx.first[x]);
            }
            if (span <= OH_RESIZE_SPAN || k.segw == 1) break;
        }
        if (span > OH_RESIZE_SPAN)
            FAIL(e, OH_E_UNSUPPORTED, "oh_pics_resize: one image column reads %d source columns (at most %d)", span, OH_RESIZE_SPAN);
        k.row_bytes = (int32_t)align_up((size_t)span * bpp, 16) + 32;
        k.rpw = std::max(1, std::min({ (int)OH_RESIZE_HROWS, OH_RESIZE_LDS / k.row_bytes, Sh }));
        k.h_stride = (int32_t)align_up((size_t)k.tw, 32);
        /* the taps of a column as QUADS of source columns that start at a multiple of four columns of the plane (an 8- or 4-byte
         * aligned LDS read): zero coefficients in front of the first tap and behind the last */
        int quads = 0;
        for (int x = 0; x < k.tw; x++) {
            const int lead = (k.x0 + hx.first[x]) & 3;
            pl->h_f4[c].push_back(hx.first[x] - lead);
            pl->h_n4[c].push_back((lead + hx.cnt[x] + 3) / 4);
            quads = std::max(quads, pl->h_n4[c].back());
        }
        k.h_groups = (Sh + k.rpw - 1) / k.rpw;
        /* vertical pass: per group of image rows the intermediate rows it reads, in pairs */
        k.v_groups = (k.th + OH_RESIZE_VROWS - 1) / OH_RESIZE_VROWS;
        int32_t pairs = 0;
        for (int g = 0; g < k.v_groups; g++) {
            const int y0 = g * OH_RESIZE_VROWS, y1 = std::min(y0 + OH_RESIZE_VROWS, k.th) - 1;
            const int lo = vx.first[y0], np = (vx.first[y1] + vx.cnt[y1] - lo + 1) / 2;
            pl->v_lo[c].push_back(lo); pl->v_np[c].push_back(np); pl->v_off[c].push_back(pairs);
            pairs += np;
        }
        const size_t sz[9] = { (size_t)k.tw * 4, (size_t)k.tw * 4, (size_t)quads * k.h_stride * 8, (size_t)k.v_groups * 4, (size_t)k.v_groups * 4,
                               (size_t)k.v_groups * 4, (size_t)pairs * OH_RESIZE_VROWS * 4, (size_t)k.tw * 4, (size_t)k.tw * 4 };
        for (int i = 0; i < 9; i++) { pl->off[c][i] = pl->tab; pl->tab += align_up(sz[i], 256); }
        for (int p = c ? 1 : 0; p < (c ? 3 : 1); p++) {
            a->mid_plane[p] = mid_pic;
            mid_pic += align_up((size_t)(Sh + 1) * k.mid_stride, 128);     /* a spare row: the odd half of a group's last pair */
        }
    }
    a->mid_pic = mid_pic;
    return OH_OK;
}

/* the tables of the plan into the host copy h of the blob; *a gets their addresses in the device copy d */
static void resize_fill(const ResizePlan &pl, OhResizeArgs *a, char *h, const char *d)
{
    memset(h, 0, pl.tab);
    for (int c = 0; c < pl.ncls; c++) {
        OhResizeClass &k = a->k[c];
        const ResizeAxis &hx = pl.hx[c], &vx = pl.vx[c];
        const size_t *off = pl.off[c];
        memcpy(h + off[0], hx.first.data(), (size_t)k.tw * 4);
        memcpy(h + off[1], hx.cnt.data(), (size_t)k.tw * 4);
        memcpy(h + off[7], pl.h_f4[c].data(), (size_t)k.tw * 4);
        memcpy(h + off[8], pl.h_n4[c].data(), (size_t)k.tw * 4);
        int16_t *hk = (int16_t *)(h + off[2]);                   /* [quad][column][4] */
        for (int x = 0; x < k.tw; x++) {
            const int lead = hx.first[x] - pl.h_f4[c][x];
            for (int j = 0; j < hx.cnt[x]; j++)
                hk[((size_t)((lead + j) / 4) * k.h_stride + x) * 4 + (lead + j) % 4] = hx.k[(size_t)x * hx.mt + j];
        }
        memcpy(h + off[3], pl.v_lo[c].data(), (size_t)k.v_groups * 4);
        memcpy(h + off[4], pl.v_np[c].data(), (size_t)k.v_groups * 4);
        memcpy(h + off[5], pl.v_off[c].data(), (size_t)k.v_groups * 4);
        int16_t *vk = (int16_t *)(h + off[6]);                   /* [pair][image row of the group][even row, odd row] */
        for (int y = 0; y < k.th; y++) {
            const int g = y / OH_RESIZE_VROWS, i = y % OH_RESIZE_VROWS;
            for (int j = 0; j < vx.cnt[y]; j++) {
                const int r = vx.first[y] + j - pl.v_lo[c][g];
                vk[(((size_t)pl.v_off[c][g] + r / 2) * OH_RESIZE_VROWS + i) * 2 + (r & 1)] = vx.k[(size_t)y * vx.mt + j];
            }
        }
        k.h_first = (const int32_t *)(d + off[0]); k.h_cnt = (const int32_t *)(d + off[1]); k.h_k = (const int16_t *)(d + off[2]);
        k.h_f4 = (const int32_t *)(d + off[7]); k.h_n4 = (const int32_t *)(d + off[8]);
        k.v_first = (const int32_t *)(d + off[3]); k.v_cnt = (const int32_t *)(d + off[4]); k.v_off = (const int32_t *)(d + off[5]);
        k.v_k = (const int32_t *)(d + off[6]);
    }
}

/* the pictures of the call in sets of at most per_set (what the intermediate has room for), one launch set each */
static int resize_launch(OhEngine *e, const int *src_ids, const int *dst_ids, int n, int per_set, int pad, OhResizeArgs *a)
{
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, src_ids[i0 + i]), a->np, a->src[i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), a->np, a->dst[i]);
        }
        ohk_resize(a, m, pad, e->stream);
    }, per_set);
}

extern "C" int oh_pics_resize(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhResize *rs)
{
    if (!e || n < 0 || !rs || (n && (!src_ids || !dst_ids)))
        return OH_E_ARG;
    if (!n)
        return OH_OK;
    const Pic *s0, *d0;
    OH_TRY(resize_check(e, src_ids, dst_ids, n, rs, &s0, &d0));
    OhResizeArgs a;
    ResizePlan pl;
    OH_TRY(resize_plan(e, s0, d0, rs, &a, &pl));
    const size_t mid_bytes = (size_t)a.mid_pic * 2;
    const int per_set = (int)std::max<size_t>(1, std::min<size_t>(OH_RESIZE_MAX_PICS, ((size_t)512 << 20) / mid_bytes));
    const size_t need = pl.tab + (size_t)std::min(n, per_set) * mid_bytes;
    if (need > e->resize_dev.bytes)
        HIPCHK(e, hipStreamSynchronize(e->stream));              /* launches of earlier calls still use the old buffer */
    OH_TRY(scratch_reserve(e, &e->resize_dev, need));            /* the tables, then the intermediate of a launch set */
    char *d = (char *)e->resize_dev.p;
    OH_TRY(upload(e, "oh_pics_resize", "tap tables", &e->resize_dev, pl.tab, [&](void *h) { resize_fill(pl, &a, (char *)h, d); }));
    a.mid = (int16_t *)(d + pl.tab);
    return resize_launch(e, src_ids, dst_ids, n, per_set, rs->width < d0->p.width || rs->height < d0->p.height, &a);
}

/* ---------------- reformatting: bit depth and chroma format (reformat.hip) ---------------- */
extern "C" int oh_pics_reformat(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhReformat *rf)
{
    const char *who = "oh_pics_reformat";
    if (!e || n < 0 || !rf || (n && (!src_ids || !dst_ids)))
        return OH_E_ARG;
    if (rf->depth < OH_RF_ROUND || rf->depth > OH_RF_DITHER)
        FAIL(e, OH_E_ARG, "%s: depth %d (0 round, 1 dither)", who, rf->depth);
    if (rf->chroma_down < OH_RF_POINT || rf->chroma_down > OH_RF_LINEAR || rf->chroma_up < OH_RF_POINT || rf->chroma_up > OH_RF_LINEAR)
        FAIL(e, OH_E_ARG, "%s: chroma_down %d, chroma_up %d (0 point, 1 linear)", who, rf->chroma_down, rf->chroma_up);
    if (!n)
        return OH_OK;
    const Pic *s0, *d0;
    OH_TRY(srcs_dsts(e, who, src_ids, n, dst_ids, n, &s0, &d0));
    const OhPicParams &sp = s0->p, &dp = d0->p;
    if (sp.width != dp.width || sp.height != dp.height)
        FAIL(e, OH_E_ARG, "%s: sources of %dx%d, destinations of %dx%d", who, sp.width, sp.height, dp.width, dp.height);
    OhRfArgs a;
    memset(&a, 0, sizeof(a));
    const int snp = n_planes(sp), dnp = n_planes(dp);            /* sources and destinations: each side its own plane count */
    row_pitches(s0, snp, a.spitch); class_sizes(s0, snp, a.sw, a.sh);
    row_pitches(d0, dnp, a.dpitch); class_sizes(d0, dnp, a.dw, a.dh);
    a.scf = sp.chroma_format_idc; a.dcf = dp.chroma_format_idc;
    a.sbd = sp.bit_depth; a.dbd = dp.bit_depth;
    a.depth = rf->depth; a.down = rf->chroma_down; a.up = rf->chroma_up;
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, src_ids[i0 + i]), snp, a.src[i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), dnp, a.dst[i]);
        }
        ohk_reformat(&a, m, e->stream);
    });
}

/* ---------------- orientation: crop, flip, rotate, transpose (orient.hip) ---------------- */
extern "C" int oh_pics_orient(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhOrient *o)
{
    const char *who = "oh_pics_orient";
    if (!e || n < 0 || !o || (n && (!src_ids || !dst_ids)))
        return OH_E_ARG;
    if (o->orientation < 0 || o->orientation > 7)
        FAIL(e, OH_E_ARG, "%s: orientation %d (0 .. 7: any OR of HFLIP 1, VFLIP 2, TRANSPOSE 4)", who, o->orientation);
    if (!n)
        return OH_OK;
    const Pic *s0, *d0;
    OH_TRY(srcs_dsts(e, who, src_ids, n, dst_ids, n, &s0, &d0));
    const OhPicParams &sp = s0->p, &dp = d0->p;
    const OhWindow &w = o->win;
    std::string why;
    if (!crop_window_ok(&sp, w, true, &why))
        return refuse(e, OH_E_ARG, who, why);
    OH_TRY(same_format(e, who, "destinations", dp, "sources", sp));
    if ((o->orientation & OH_ORIENT_TRANSPOSE) && sp.chroma_format_idc == 2)
        FAIL(e, OH_E_UNSUPPORTED, "%s: orientation %d transposes 4:2:2 pictures into 4:4:0 (reformat to 4:2:0 or 4:4:4 first)", who, o->orientation);
    int W, H, iw = 0, ih = 0;
    window_size(&sp, w, &W, &H);
    (void)oh_orient_size(o->orientation, W, H, &iw, &ih);
    if (iw > dp.width || ih > dp.height)
        FAIL(e, OH_E_ARG, "%s: the image of %dx%d does not fit the destinations' %dx%d", who, iw, ih, dp.width, dp.height);
    OhOrArgs a;
    memset(&a, 0, sizeof(a));
    a.np = n_planes(sp); a.bd = sp.bit_depth; a.orientation = o->orientation;
    row_pitches(s0, a.np, a.spitch);
    row_pitches(d0, a.np, a.dpitch);
    class_sizes(d0, a.np, a.dw, a.dh);
    for (int q = 0; q < (a.np > 1 ? 2 : 1); q++)
        class_window(&sp, w, q, &a.x0[q], &a.y0[q], &a.ws[q], &a.hs[q]);
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, src_ids[i0 + i]), a.np, a.src[i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), a.np, a.dst[i]);
        }
        ohk_orient(&a, m, e->stream);
    });
}

/* ---------------- warping: affine and perspective resampling (warp.hip) ---------------- */
extern "C" int oh_pics_warp(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhWarp *w)
{
    const char *who = "oh_pics_warp";
    if (!e || n < 0 || !w || (n && (!src_ids || !dst_ids)))
        return OH_E_ARG;
    std::string why;
    if (warp_check(w, 16, &why) || warp_image_check(w, &why))           /* the fill against the depth: below, with the pictures */
        return refuse(e, OH_E_ARG, who, why);
    if (!n)
        return OH_OK;
    const Pic *s0, *d0;
    OH_TRY(srcs_dsts(e, who, src_ids, n, dst_ids, n, &s0, &d0));
    const OhPicParams &sp = s0->p, &dp = d0->p;
    if (!crop_window_ok(&sp, w->win, true, &why))
        return refuse(e, OH_E_ARG, who, why);
    const int hs = oh_hshift(&sp, 1), vs = oh_vshift(&sp, 1);
    OH_TRY(same_format(e, who, "destinations", dp, "sources", sp));
    if (w->width > dp.width || w->height > dp.height || w->width % (1 << hs) || w->height % (1 << vs))
        FAIL(e, OH_E_ARG, "%s: image %dx%d: above the destination's %dx%d, or not multiples of %dx%d", who, w->width, w->height, dp.width, dp.height,
             1 << hs, 1 << vs);
    if (warp_check(w, sp.bit_depth, &why))
        return refuse(e, OH_E_ARG, who, why);
    OhWarpArgs a;
    memset(&a, 0, sizeof(a));
    a.np = n_planes(sp); a.bd = sp.bit_depth; a.sx = hs; a.sy = vs;
    a.mode = w->mode; a.filter = w->filter; a.border = w->border;
    for (int c = 0; c < 3; c++) a.fill[c] = w->fill[c];
    for (int k = 0; k < 9; k++) a.m[k] = w->m[k];
    row_pitches(s0, a.np, a.spitch);
    row_pitches(d0, a.np, a.dpitch);
    class_sizes(d0, a.np, a.dw, a.dh);
    for (int q = 0; q < (a.np > 1 ? 2 : 1); q++) {
        class_window(&sp, w->win, q, &a.x0[q], &a.y0[q], &a.ws[q], &a.hs[q]);
        a.iw[q] = w->width >> oh_hshift(&sp, q); a.ih[q] = w->height >> oh_vshift(&sp, q);
    }
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, src_ids[i0 + i]), a.np, a.src[i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), a.np, a.dst[i]);
        }
        ohk_warp(&a, m, e->stream);
    });
}

/* ---------------- fields and deinterlacing (deinterlace.hip) ---------------- */
/* what weave and separate ask of their fields (f0) and frames (F0) */
static int fields_check(OhEngine *e, const char *who, const Pic *f0, const Pic *F0)
{
    const OhPicParams &fp = f0->p, &Fp = F0->p;
    OH_TRY(same_format(e, who, "fields", fp, "frames", Fp));
    if (fp.width != Fp.width || Fp.height != 2 * fp.height)
        FAIL(e, OH_E_ARG, "%s: fields of %dx%d, frames of %dx%d (the same width, twice the height)", who, fp.width, fp.height, Fp.width, Fp.height);
    return OH_OK;
}

/* the launches of weave and separate: role[k] (null: not in this call) holds the ids of a.pic[k]; wr: the roles that are written */
static int fields_launch(OhEngine *e, const Pic *f0, const Pic *F0, const int *const role[4], unsigned wr, int op, int sides, int n)
{
    OhDiArgs a;
    memset(&a, 0, sizeof(a));
    const OhPicParams &Fp = F0->p;
    a.np = n_planes(Fp); a.bd = Fp.bit_depth; a.op = op; a.sides = sides;
    row_pitches(F0, a.np, a.pitch);
    row_pitches(f0, a.np, a.fpitch);
    class_sizes(F0, a.np, a.w, a.h);
    return launch_sets(e, n, [&](int i0, int m) {
        for (int k = 0; k < 4; k++) {
            if (!role[k])
                continue;
            for (int i = 0; i < m; i++) {
                Pic *q = get_pic(e, role[k][i0 + i]);
                if (wr >> k & 1) write_planes(q, a.np, a.pic[k][i]);
                else             read_planes(q, a.np, a.pic[k][i]);
            }
        }
        ohk_fields(&a, m, e->stream);
    });
}

extern "C" int oh_pics_weave(OhEngine *e, const int *top_ids, const int *bottom_ids, const int *dst_ids, int n)
{
    const char *who = "oh_pics_weave";
    if (!e || n < 0 || (n && (!top_ids || !bottom_ids || !dst_ids)))
        return OH_E_ARG;
    if (!n)
        return OH_OK;
    std::vector<int> fields(top_ids, top_ids + n);
    fields.insert(fields.end(), bottom_ids, bottom_ids + n);
    const Pic *f0, *F0;
    OH_TRY(srcs_dsts(e, who, fields.data(), 2 * n, dst_ids, n, &f0, &F0));
    OH_TRY(fields_check(e, who, f0, F0));
    const int *const role[4] = { top_ids, bottom_ids, nullptr, dst_ids };
    return fields_launch(e, f0, F0, role, 1u << 3, OH_DI_WEAVE, 3, n);
}

extern "C" int oh_pics_separate(OhEngine *e, const int *src_ids, const int *top_ids, const int *bottom_ids, int n)
{
    const char *who = "oh_pics_separate";
    if (!e || n < 0 || (n && !src_ids) || (!top_ids && !bottom_ids))
        return OH_E_ARG;
    if (!n)
        return OH_OK;
    std::vector<int> fields;
    if (top_ids) fields.insert(fields.end(), top_ids, top_ids + n);
    if (bottom_ids) fields.insert(fields.end(), bottom_ids, bottom_ids + n);
    const Pic *F0, *f0;
    OH_TRY(srcs_dsts(e, who, src_ids, n, fields.data(), (int)fields.size(), &F0, &f0));
    OH_TRY(fields_check(e, who, f0, F0));
    const int *const role[4] = { src_ids, nullptr, top_ids, bottom_ids };
    return fields_launch(e, f0, F0, role, 3u << 2, OH_DI_SEPARATE, (top_ids ? 1 : 0) | (bottom_ids ? 2 : 0), n);
}

extern "C" int oh_pics_deinterlace(OhEngine *e, const int *prev_ids, const int *cur_ids, const int *next_ids, const int *dst_ids, int n,
                                   const OhDeinterlace *d)
{
    const char *who = "oh_pics_deinterlace";
    if (!e || n < 0 || !d || (n && (!cur_ids || !dst_ids)))
        return OH_E_ARG;
    if (d->mode < OH_DEINT_BOB || d->mode > OH_DEINT_ADAPTIVE)
        FAIL(e, OH_E_ARG, "%s: mode %d (0 bob, 1 blend, 2 lowpass5, 3 adaptive)", who, d->mode);
    if (d->parity < 0 || d->parity > 1 || d->kept_first < 0 || d->kept_first > 1)
        FAIL(e, OH_E_ARG, "%s: parity %d, kept_first %d (0 or 1)", who, d->parity, d->kept_first);
    if (!n)
        return OH_OK;
    Neighbours nb;                                              /* prev and next: read by ADAPTIVE only */
    OH_TRY(neighbours(e, who, "cur", prev_ids, cur_ids, next_ids, n, d->mode == OH_DEINT_ADAPTIVE, &nb));
    const Pic *p0 = alike_apart(e, who, nb.srcs, dst_ids, n);
    if (!p0) return OH_E_ARG;
    const OhPicParams &p = p0->p;
    HIPCHK(e, hipSetDevice(e->device));
    OhDiArgs a;
    memset(&a, 0, sizeof(a));
    a.np = n_planes(p); a.bd = p.bit_depth;
    a.mode = d->mode; a.parity = d->parity; a.kept_first = d->kept_first;
    row_pitches(p0, a.np, a.pitch);
    class_sizes(p0, a.np, a.w, a.h);
    for (int q = 0; q < (a.np > 1 ? 2 : 1); q++)
        if (a.h[q] < 2 || (a.h[q] & 1))
            FAIL(e, OH_E_ARG, "%s: planes of %d rows (an even number, 2 at least)", who, a.h[q]);
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, nb.around[0][i0 + i]), a.np, a.pic[0][i]);
            read_planes(get_pic(e, cur_ids[i0 + i]), a.np, a.pic[1][i]);
            read_planes(get_pic(e, nb.around[1][i0 + i]), a.np, a.pic[2][i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), a.np, a.pic[3][i]);
        }
        ohk_deinterlace(&a, m, e->stream);
    });
}

/* ---------------- filters (filter.hip) ---------------- */
extern "C" int oh_pics_filter(OhEngine *e, const int *prev_ids, const int *src_ids, const int *next_ids, const int *dst_ids, int n,
                              const OhFilter *f)
{
    const char *who = "oh_pics_filter";
    if (!e || n < 0 || !f || (n && (!src_ids || !dst_ids)))
        return OH_E_ARG;
    if (f->mode < OH_FILTER_CONVOLVE || f->mode > OH_FILTER_TEMPORAL)
        FAIL(e, OH_E_ARG, "%s: mode %d (0 convolve, 1 unsharp, 2 median, 3 temporal)", who, f->mode);
    if (!n) {                                                   /* no picture, no bit depth: what does not depend on one */
        std::string why;
        return refuse(e, filter_check(f, 12, &why), who, why);
    }
    Neighbours nb;                                              /* prev and next: read by TEMPORAL only */
    OH_TRY(neighbours(e, who, "src", prev_ids, src_ids, next_ids, n, f->mode == OH_FILTER_TEMPORAL, &nb));
    const Pic *p0 = alike_apart(e, who, nb.srcs, dst_ids, n);
    if (!p0) return OH_E_ARG;
    const OhPicParams &p = p0->p;
    std::string why;
    OH_TRY(refuse(e, filter_check(f, p.bit_depth, &why), who, why));
    HIPCHK(e, hipSetDevice(e->device));
    OhFilterArgs a;
    memset(&a, 0, sizeof(a));
    a.np = n_planes(p); a.bd = p.bit_depth;
    a.mode = f->mode; a.planes = f->planes;
    row_pitches(p0, a.np, a.pitch);
    class_sizes(p0, a.np, a.w, a.h);
    for (int q = 0; q < 2; q++) {
        a.amount[q] = f->amount[q]; a.threshold[q] = f->threshold[q];
        if (f->mode > OH_FILTER_UNSHARP)
            continue;
        const OhFilterTaps &t = f->taps[q];
        for (int k = 0; k < t.nh; k++) a.taps_h[q][OH_FILTER_MAX_TAPS / 2 - t.nh / 2 + k] = t.h[k];
        for (int k = 0; k < t.nv; k++) a.taps_v[q][OH_FILTER_MAX_TAPS / 2 - t.nv / 2 + k] = t.v[k];
        a.radius = std::max(a.radius, std::max(t.nh, t.nv) / 2);
    }
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, nb.around[0][i0 + i]), a.np, a.src[0][i]);
            read_planes(get_pic(e, src_ids[i0 + i]), a.np, a.src[1][i]);
            read_planes(get_pic(e, nb.around[1][i0 + i]), a.np, a.src[2][i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), a.np, a.dst[i]);
        }
        ohk_filter(&a, m, e->stream);
    });
}

/* ---------------- composition (compose.hip) ---------------- */
/* everything oh_pics_compose refuses, before anything is enqueued (dst_ids, cp not null; n > 0) */
static int compose_check(OhEngine *e, const int *dst_ids, int n, const OhCompose *cp)
{
    const char *who = "oh_pics_compose";
    if (cp->flags & ~OH_COMPOSE_FILL)
        FAIL(e, OH_E_ARG, "%s: flags 0x%x (0 or OH_COMPOSE_FILL)", who, (unsigned)cp->flags);
    if (cp->n_layers < 0 || cp->n_layers > OH_COMPOSE_MAX_LAYERS || (cp->n_layers && !cp->layers))
        FAIL(e, OH_E_ARG, "%s: n_layers %d (0 .. %d), or no layers", who, cp->n_layers, OH_COMPOSE_MAX_LAYERS);
    const Pic *d0 = alike_pics(e, who, dst_ids, n);
    if (!d0) return OH_E_ARG;
    std::vector<int> d;
    OH_TRY(distinct_dsts(e, who, dst_ids, n, &d));
    const OhPicParams &dp = d0->p;
    const int cf = dp.chroma_format_idc, sw = 1 << oh_hshift(&dp, 1), sh = 1 << oh_vshift(&dp, 1);
    if (cp->flags & OH_COMPOSE_FILL)
        for (int c = 0; c < (cf ? 3 : 1); c++)
            if (cp->fill[c] < 0 || cp->fill[c] >= 1 << dp.bit_depth)
                FAIL(e, OH_E_ARG, "%s: fill[%d] = %d is not a sample of %d bits", who, c, cp->fill[c], dp.bit_depth);
    for (int k = 0; k < cp->n_layers; k++) {
        const OhLayer &l = cp->layers[k];
        if (!l.src_ids)
            FAIL(e, OH_E_ARG, "%s: layer %d has no src_ids", who, k);
        for (int i = 0; i < n; i++) {
            if (!get_pic(e, l.src_ids[i]))
                FAIL(e, OH_E_ARG, "%s: layer %d: unknown picture %d", who, k, l.src_ids[i]);
            if (std::binary_search(d.begin(), d.end(), l.src_ids[i]))
                FAIL(e, OH_E_ARG, "%s: layer %d: picture %d is both source and destination", who, k, l.src_ids[i]);
        }
        const int so = first_other_params(e, l.src_ids, n);
        if (so < n)
            FAIL(e, OH_E_ARG, "%s: layer %d: picture %d has other params than picture %d", who, k, l.src_ids[so], l.src_ids[0]);
        const OhPicParams &sp = get_pic(e, l.src_ids[0])->p;
        if (l.opacity < 0 || l.opacity > 256)
            FAIL(e, OH_E_ARG, "%s: layer %d: opacity %d (0 .. 256)", who, k, l.opacity);
        if (sp.bit_depth != dp.bit_depth || sp.chroma_format_idc != cf)
            FAIL(e, OH_E_UNSUPPORTED, "%s: layer %d: sources of %d bit, chroma format %d; destinations of %d bit, chroma format %d", who, k,
                 sp.bit_depth, sp.chroma_format_idc, dp.bit_depth, cf);
        if (l.w < 1 || l.h < 1 || l.sx < 0 || l.sy < 0 || l.sx > sp.width - l.w || l.sy > sp.height - l.h)
            FAIL(e, OH_E_ARG, "%s: layer %d: rectangle %dx%d at (%d,%d) is empty or not inside the source's %dx%d", who, k, l.w, l.h, l.sx, l.sy,
                 sp.width, sp.height);
        if (l.sx % sw || l.w % sw || l.dx % sw || l.sy % sh || l.h % sh || l.dy % sh)
            FAIL(e, OH_E_ARG, "%s: layer %d: rectangle %dx%d at (%d,%d) to (%d,%d): not multiples of %dx%d", who, k, l.w, l.h, l.sx, l.sy, l.dx,
                 l.dy, sw, sh);
        if (!l.alpha)
            continue;
        if (l.alpha_pixel_stride < 0 || l.alpha_row_stride < 0 || l.alpha_image_stride < 0)
            FAIL(e, OH_E_ARG, "%s: layer %d: negative alpha strides (%lld, %lld, %lld)", who, k, (long long)l.alpha_pixel_stride,
                 (long long)l.alpha_row_stride, (long long)l.alpha_image_stride);
        /* the last byte the unclipped rectangle of the last image addresses, in 128 bits: the strides are the caller's */
        const unsigned __int128 last = (unsigned __int128)(n - 1) * (uint64_t)l.alpha_image_stride +
                                       (unsigned __int128)(l.h - 1) * (uint64_t)l.alpha_row_stride +
                                       (unsigned __int128)(l.w - 1) * (uint64_t)l.alpha_pixel_stride;
        HIPCHK(e, hipSetDevice(e->device));
        const size_t room = device_room(e, l.alpha);                                       /* bytes from alpha to the allocation's end */
        if (room == ROOM_NONE)
            FAIL(e, OH_E_ARG, "%s: layer %d: alpha is not device memory of device %d", who, k, e->device);
        if (room != ROOM_UNKNOWN && last >= room)
            FAIL(e, OH_E_ARG, "%s: layer %d: the alpha planes of %d rectangles of %dx%d (strides %lld, %lld, %lld) run past the %zu bytes left of "
                 "their allocation", who, k, n, l.w, l.h, (long long)l.alpha_pixel_stride, (long long)l.alpha_row_stride,
                 (long long)l.alpha_image_stride, room);
    }
    return OH_OK;
}

extern "C" int oh_pics_compose(OhEngine *e, const int *dst_ids, int n, const OhCompose *cp)
{
    if (!e || !cp || n < 0 || (n && !dst_ids))
        return OH_E_ARG;
    if (!n)
        return OH_OK;
    OH_TRY(compose_check(e, dst_ids, n, cp));
    const Pic *d0 = get_pic(e, dst_ids[0]);
    const OhPicParams &dp = d0->p;
    const int bpp = sample_bytes(dp.bit_depth), np = n_planes(dp), gs = 16 / bpp;
    const bool fill = (cp->flags & OH_COMPOSE_FILL) != 0;
    OhCpsArgs a;
    memset(&a, 0, sizeof(a));
    row_pitches(d0, np, a.pitch);
    for (int c = 0; c < np; c++) a.fill_v[c] = fill ? cp->fill[c] : 0;
    a.np = np; a.bd = dp.bit_depth; a.cf = dp.chroma_format_idc; a.fill = fill;

    /* the layers that are not wholly outside, with their geometry in both plane classes, and the area they touch */
    std::vector<OhCpsLayer> lay;
    std::vector<int> which;                                      /* their indices in cp->layers */
    int box[2][4] = { { INT32_MAX, INT32_MAX, 0, 0 }, { INT32_MAX, INT32_MAX, 0, 0 } };      /* x0, y0, x1, y1 */
    for (int k = 0; k < cp->n_layers; k++) {
        const OhLayer &l = cp->layers[k];
        const Pic *s0 = get_pic(e, l.src_ids[0]);
        OhCpsLayer L;
        memset(&L, 0, sizeof(L));
        bool empty = false;
        for (int q = 0; q < (np > 1 ? 2 : 1); q++) {
            const int hs = oh_hshift(&dp, q), vs = oh_vshift(&dp, q);
            const int dx = l.dx >> hs, dy = l.dy >> vs;         /* multiples of the sub-sampling: exact, also below zero */
            /* the clip in 64 bits: dx and dy are any int32; a layer that is not wholly outside lies within a picture's extent of zero */
            const int64_t x1 = std::min<int64_t>((int64_t)dx + (l.w >> hs), d0->w[q]), y1 = std::min<int64_t>((int64_t)dy + (l.h >> vs), d0->h[q]);
            if (dx >= x1 || dy >= y1 || x1 <= 0 || y1 <= 0) {
                empty = true;
                break;
            }
            L.x0[q] = std::max(dx, 0); L.x1[q] = (int32_t)x1;
            L.y0[q] = std::max(dy, 0); L.y1[q] = (int32_t)y1;
            L.ox[q] = (l.sx >> hs) - dx; L.oy[q] = (l.sy >> vs) - dy;
            L.dx[q] = dx; L.dy[q] = dy;
            L.spitch[q] = s0->stride[q] * bpp;
        }
        if (empty)
            continue;
        L.opacity = l.opacity; L.has_alpha = l.alpha != nullptr;
        L.a_ps = l.alpha_pixel_stride; L.a_rs = l.alpha_row_stride;
        for (int q = 0; q < (np > 1 ? 2 : 1); q++) {
            box[q][0] = std::min(box[q][0], L.x0[q]); box[q][1] = std::min(box[q][1], L.y0[q]);
            box[q][2] = std::max(box[q][2], L.x1[q]); box[q][3] = std::max(box[q][3], L.y1[q]);
        }
        lay.push_back(L);
        which.push_back(k);
    }
    /* compose writes in place into the finished half, whichever it is, so it does not go through write_planes: final_b stays, and only
     * done_seq is cleared — not written by a reconstruction batch: a download stays behind the engine stream */
    for (int i = 0; i < n; i++)
        get_pic(e, dst_ids[i])->done_seq = 0;
    if (lay.empty() && !fill)
        return OH_OK;                                           /* nothing reaches the destinations */
    for (int q = 0; q < (np > 1 ? 2 : 1); q++) {
        OhCpsClass &kc = a.k[q];
        if (fill) { box[q][0] = box[q][1] = 0; box[q][2] = d0->w[q]; box[q][3] = d0->h[q]; }
        kc.gx0 = box[q][0] / gs; kc.gx1 = (box[q][2] + gs - 1) / gs;     /* whole granules: a row's last one may end in its padding */
        kc.y0 = box[q][1]; kc.y1 = box[q][3];
        kc.tx = (kc.gx1 - kc.gx0 + OH_CPS_TW - 1) / OH_CPS_TW; kc.ty = (kc.y1 - kc.y0 + OH_CPS_TH - 1) / OH_CPS_TH;
    }

    /* the table: the layers, then per launch set [layer][destination of the set]; built in a pinned buffer of the pool and copied on the
     * engine stream — behind the launches of an earlier call that read the device copy, in front of this call's */
    const int nl = (int)lay.size();
    const size_t lay_bytes = align_up((size_t)nl * sizeof(OhCpsLayer), 256);
    const size_t need = lay_bytes + (size_t)nl * (size_t)n * sizeof(OhCpsSrc);
    HIPCHK(e, hipSetDevice(e->device));
    if (nl) {
        if (need > e->compose_dev.bytes)
            HIPCHK(e, hipStreamSynchronize(e->stream));          /* launches of earlier calls still read the old table */
        OH_TRY(upload(e, "oh_pics_compose", "layer table", &e->compose_dev, need, [&](void *h) {
            memset(h, 0, lay_bytes);
            memcpy(h, lay.data(), (size_t)nl * sizeof(OhCpsLayer));
            OhCpsSrc *hs = (OhCpsSrc *)((char *)h + lay_bytes);
            for (int j = 0; j < nl; j++) {
                const OhLayer &l = cp->layers[which[j]];
                for (int i = 0; i < n; i++) {                   /* picture i of the call: number i - i0 of the m in its launch set */
                    const int i0 = i - i % OH_CONV_MAX_PICS, m = std::min(n - i0, (int)OH_CONV_MAX_PICS);
                    OhCpsSrc &t = hs[(size_t)nl * i0 + (size_t)j * m + (i - i0)];
                    read_planes(get_pic(e, l.src_ids[i]), np, t.p);
                    t.alpha = l.alpha ? (const uint8_t *)l.alpha + (size_t)i * (size_t)l.alpha_image_stride : nullptr;
                }
            }
        }));
    }
    a.n_layers = nl;
    a.layers = (const OhCpsLayer *)e->compose_dev.p;
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) read_planes(get_pic(e, dst_ids[i0 + i]), np, a.dst[i]);      /* in place: the finished half */
        a.srcs = nl ? (const OhCpsSrc *)((const char *)e->compose_dev.p + lay_bytes) + (size_t)nl * i0 : nullptr;
        a.n_pics = m;
        ohk_compose(&a, m, e->stream);
    });
}

/* ---------------- histograms of the code values (histogram.hip) ---------------- */
extern "C" int oh_pics_histogram(OhEngine *e, const int *pic_ids, int n, const OhWindow *win, OhHistogram *out)
{
    const char *who = "oh_pics_histogram";
    if (!e || n < 0 || !win || !out || (n && !pic_ids))
        return OH_E_ARG;
    if (!n)
        return OH_OK;
    const Pic *p0 = alike_pics(e, who, pic_ids, n);
    if (!p0) return OH_E_ARG;
    const OhPicParams &p = p0->p;
    std::string why;
    if (!crop_window_ok(&p, *win, true, &why))
        return refuse(e, OH_E_ARG, who, why);
    HIPCHK(e, hipSetDevice(e->device));
    OhHistArgs a;
    memset(&a, 0, sizeof(a));
    const int np = n_planes(p), sb = sample_bytes(p.bit_depth);
    row_pitches(p0, np, a.pitch);
    for (int c = 0; c < (np > 1 ? 2 : 1); c++) {
        OhHistClass &k = a.k[c];
        class_window(&p, *win, c, &k.x0, &k.y0, &k.w, &k.h);
        k.g0 = k.x0 * sb / 16;                                  /* the granules of a row that hold a sample of the window */
        k.ng = ((k.x0 + k.w) * sb + 15) / 16 - k.g0;
        k.tiles = (k.h + OH_HG_ROWS - 1) / OH_HG_ROWS;
    }
    a.np = np; a.bd = p.bit_depth;
    const size_t per_pic = (size_t)3 * OH_HG_BINS, bytes = (size_t)n * per_pic * sizeof(uint32_t);
    OhEngine::Stage *sg = nullptr;
    OH_TRY(results_begin(e, who, &e->hist_res, bytes, n, &sg));
    OH_TRY(launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) read_planes(get_pic(e, pic_ids[i0 + i]), np, a.src[i]);
        a.res = (uint32_t *)e->hist_res.p + (size_t)i0 * per_pic;
        ohk_histogram(&a, m, e->stream);
    }));
    OH_TRY(results_fetch(e, &e->hist_res, bytes, sg));
    const uint32_t *r = (const uint32_t *)sg->p;
    for (int i = 0; i < n; i++) {
        memset(&out[i], 0, sizeof(out[i]));
        for (int c = 0; c < np; c++)
            hist_derive(r + (size_t)i * per_pic + (size_t)c * OH_HG_BINS, &out[i].plane[c]);
    }
    return OH_OK;
}

/* ---------------- look-up tables (lut.hip) ---------------- */
extern "C" int oh_pics_lut(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhLut *lut)
{
    const char *who = "oh_pics_lut";
    if (!e || n < 0 || !lut || (n && (!src_ids || !dst_ids)))
        return OH_E_ARG;
    if (lut->planes < 0 || lut->planes > 7)
        FAIL(e, OH_E_ARG, "%s: planes %d outside 0 .. 7", who, lut->planes);
    if (!n)
        return OH_OK;
    const Pic *s0, *d0;
    OH_TRY(srcs_dsts(e, who, src_ids, n, dst_ids, n, &s0, &d0));
    const OhPicParams &sp = s0->p, &dp = d0->p;
    if (sp.width != dp.width || sp.height != dp.height || sp.chroma_format_idc != dp.chroma_format_idc)
        FAIL(e, OH_E_ARG, "%s: sources of %dx%d, chroma format %d, destinations of %dx%d, chroma format %d", who, sp.width, sp.height,
             sp.chroma_format_idc, dp.width, dp.height, dp.chroma_format_idc);
    std::string why;
    if (lut_check(lut, sp.bit_depth, dp.bit_depth, n_planes(sp), &why))
        return refuse(e, OH_E_ARG, who, why);
    const int np = n_planes(sp);
    /* the tables of the call; the device copy has its full size from the first call on */
    const size_t tab_bytes = (size_t)3 * OH_LUT_MAX * sizeof(uint16_t);
    OH_TRY(upload(e, who, "tables", &e->lut_tabs, tab_bytes, [&](void *h) {
        memset(h, 0, tab_bytes);
        for (int c = 0; c < np; c++)
            if (lut->planes >> c & 1)
                memcpy((uint16_t *)h + (size_t)c * OH_LUT_MAX, lut->table[c], (size_t)lut->n_entries * sizeof(uint16_t));
    }));
    OhLutArgs a;
    memset(&a, 0, sizeof(a));
    row_pitches(s0, np, a.spitch); row_pitches(d0, np, a.dpitch);
    class_sizes(s0, np, a.w, a.h);
    a.np = np; a.sbd = sp.bit_depth; a.dbd = dp.bit_depth;
    a.planes = lut->planes;
    a.tab = (const uint16_t *)e->lut_tabs.p;
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, src_ids[i0 + i]), np, a.src[i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), np, a.dst[i]);
        }
        ohk_lut(&a, m, e->stream);
    });
}

/* ---------------- film grain (grain.hip) ---------------- */
extern "C" int oh_pics_grain(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhGrain *g, const uint32_t *seeds)
{
    const char *who = "oh_pics_grain";
    if (!e || n < 0 || !g || !seeds || (n && (!src_ids || !dst_ids)))
        return OH_E_ARG;
    std::string why;
    if (grain_check(g, 0, &why))                                /* planes, blending, log2_scale: also of a call without pictures */
        return refuse(e, OH_E_ARG, who, why);
    if (!n)
        return OH_OK;
    const Pic *s0, *d0;
    OH_TRY(srcs_dsts(e, who, src_ids, n, dst_ids, n, &s0, &d0));
    if (memcmp(&s0->p, &d0->p, sizeof(OhPicParams)))
        FAIL(e, OH_E_ARG, "%s: destination %d has other params than source %d", who, dst_ids[0], src_ids[0]);
    const OhPicParams &p = s0->p;
    const int np = n_planes(p);
    if (grain_check(g, np, &why))
        return refuse(e, OH_E_ARG, who, why);
    /* the patterns: once per engine */
    if (!e->grain_patterns_ready) {
        OH_TRY(upload(e, who, "patterns", &e->grain_patterns, (size_t)GRAIN_CUTS * GRAIN_CUTS * GRAIN_PAT * GRAIN_PAT, [&](void *h) {
            for (int fh = GRAIN_CUT_MIN; fh <= GRAIN_CUT_MAX; fh++)
                for (int fv = GRAIN_CUT_MIN; fv <= GRAIN_CUT_MAX; fv++)
                    (void)oh_grain_pattern(fh, fv, nullptr, nullptr, (int8_t *)h + (size_t)grain_pattern_index(fh, fv) * GRAIN_PAT * GRAIN_PAT);
        }));
        e->grain_patterns_ready = true;
    }
    /* the tables and the seeds of the call */
    const size_t tab_bytes = (size_t)3 * OH_GRAIN_ENTRIES * sizeof(uint32_t), need = tab_bytes + (size_t)n * sizeof(uint32_t);
    if (need > e->grain_tabs.bytes)
        HIPCHK(e, hipStreamSynchronize(e->stream));              /* launches of earlier calls still read the old block */
    OH_TRY(upload(e, who, "tables and seeds", &e->grain_tabs, need, [&](void *h) {
        memset(h, 0, tab_bytes);
        for (int c = 0; c < np; c++)
            if (g->planes >> c & 1)
                memcpy((uint32_t *)h + (size_t)c * OH_GRAIN_ENTRIES, g->table[c], OH_GRAIN_ENTRIES * sizeof(uint32_t));
        memcpy((char *)h + tab_bytes, seeds, (size_t)n * sizeof(uint32_t));
    }));
    OhGrainArgs a;
    memset(&a, 0, sizeof(a));
    row_pitches(s0, np, a.pitch);
    class_sizes(s0, np, a.w, a.h);
    for (int q = 0; q < (np > 1 ? 2 : 1); q++) {
        a.tx[q] = (a.w[q] + GRAIN_TW * GRAIN_BLOCK - 1) / (GRAIN_TW * GRAIN_BLOCK);
        a.ty[q] = (a.h[q] + GRAIN_BLOCK - 1) / GRAIN_BLOCK;
    }
    a.np = np; a.bd = p.bit_depth;
    a.planes = g->planes; a.blending = g->blending; a.log2_scale = g->log2_scale;
    a.tab = (const uint32_t *)e->grain_tabs.p;
    a.patterns = (const int8_t *)e->grain_patterns.p;
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, src_ids[i0 + i]), np, a.src[i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), np, a.dst[i]);
        }
        a.seeds = (const uint32_t *)((const char *)e->grain_tabs.p + tab_bytes) + i0;
        ohk_grain(&a, m, e->stream);
    });
}

/* ---------------- colour remapping (remap.hip) ---------------- */
extern "C" int oh_pics_colour_remap(OhEngine *e, const int *src_ids, const int *dst_ids, int n, const OhRemap *r)
{
    const char *who = "oh_pics_colour_remap";
    if (!e || n < 0 || !r || (n && (!src_ids || !dst_ids)))
        return OH_E_ARG;
    std::string why;
    if (remap_check(r, &why))                                   /* depths, matrix and tables: also of a call without pictures */
        return refuse(e, OH_E_ARG, who, why);
    if (!n)
        return OH_OK;
    const Pic *s0, *d0;
    OH_TRY(srcs_dsts(e, who, src_ids, n, dst_ids, n, &s0, &d0));
    const OhPicParams &sp = s0->p, &dp = d0->p;
    if (sp.width != dp.width || sp.height != dp.height)
        FAIL(e, OH_E_ARG, "%s: sources of %dx%d, destinations of %dx%d", who, sp.width, sp.height, dp.width, dp.height);
    if (sp.bit_depth != r->in_bit_depth || dp.bit_depth != r->out_bit_depth)
        FAIL(e, OH_E_ARG, "%s: sources of %d bit, destinations of %d bit; the remap is from %d to %d bit", who, sp.bit_depth, dp.bit_depth,
             r->in_bit_depth, r->out_bit_depth);
    if (sp.chroma_format_idc != 3 || dp.chroma_format_idc != 3)
        FAIL(e, OH_E_UNSUPPORTED, "%s: sources of chroma format %d, destinations of chroma format %d; only 4:4:4 "
             "(oh_pics_reformat first, or oh_remap_luts with oh_pics_lut where the matrix is diagonal)", who, sp.chroma_format_idc, dp.chroma_format_idc);
    /* the tables of the call; the device copy has its full size from the first call on */
    const size_t tab_bytes = (size_t)6 * OH_LUT_MAX * sizeof(uint16_t);
    OH_TRY(upload(e, who, "tables", &e->remap_tabs, tab_bytes, [&](void *h) {
        memset(h, 0, tab_bytes);
        for (int c = 0; c < 3; c++) {
            memcpy((uint16_t *)h + (size_t)c * OH_LUT_MAX, r->pre[c], sizeof(uint16_t) << r->in_bit_depth);
            memcpy((uint16_t *)h + (size_t)(3 + c) * OH_LUT_MAX, r->post[c], sizeof(uint16_t) << r->out_bit_depth);
        }
    }));
    OhRemapArgs a;
    memset(&a, 0, sizeof(a));
    row_pitches(s0, 3, a.spitch); row_pitches(d0, 3, a.dpitch);
    a.w = s0->w[0]; a.h = s0->h[0];
    a.sbd = sp.bit_depth; a.dbd = dp.bit_depth;
    memcpy(a.coeff, r->coeff, sizeof(a.coeff));
    a.log2_denom = r->log2_denom;
    a.identity = remap_is_identity(r);
    a.rows = OH_REMAP_ROWS;
    a.tab = (const uint16_t *)e->remap_tabs.p;
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, src_ids[i0 + i]), 3, a.src[i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), 3, a.dst[i]);
        }
        ohk_remap(&a, m, e->stream);
    });
}

/* ---------------- frame packing (packing.hip) ---------------- */
/* what both calls ask of the packed pictures (P0) and the views (v0): one format, and views of the half or the full size.  *full: which;
 * where the two sizes are one, the full size */
static int packing_sizes(OhEngine *e, const char *who, const OhPacking *pk, const Pic *P0, const Pic *v0, int *full)
{
    const OhPicParams &pp = P0->p, &vp = v0->p;
    OH_TRY(same_format(e, who, "views", vp, "packed pictures", pp));
    PkPlane pl[2];
    OhPicParams size[2];
    std::string why;
    for (int f = 0; f < 2; f++)
        if (const int rc = packing_geometry(pk, &pp, f, pl, &size[f], &why))
            return refuse(e, rc, who, why);
    for (int f = 1; f >= 0; f--)
        if (vp.width == size[f].width && vp.height == size[f].height) {
            *full = f;
            return OH_OK;
        }
    FAIL(e, OH_E_ARG, "%s: views of %dx%d, packed pictures of %dx%d (half size %dx%d, full size %dx%d)", who, vp.width, vp.height, pp.width,
         pp.height, size[0].width, size[0].height, size[1].width, size[1].height);
}

static void packing_args(const OhPacking *pk, const Pic *P0, const Pic *v0, int full, OhPkArgs *a)
{
    memset(a, 0, sizeof(*a));
    std::string why;
    (void)packing_geometry(pk, &P0->p, full, a->pl, nullptr, &why);
    a->np = n_planes(P0->p); a->bd = P0->p.bit_depth;
    row_pitches(P0, a->np, a->ppitch);
    row_pitches(v0, a->np, a->vpitch);
    for (int v = 0; v < 2; v++) {
        a->flip[v] = pk->flip[v];
        a->g[v] = pk->arrangement == OH_PACK_SIDE_BY_SIDE ? pk->grid_x[v] : pk->grid_y[v];
    }
}

extern "C" int oh_pics_unpack(OhEngine *e, const int *src_ids, const int *view0_ids, const int *view1_ids, int n, const OhPacking *pk)
{
    const char *who = "oh_pics_unpack";
    if (!e || n < 0 || !pk || (n && !src_ids) || (!view0_ids && !view1_ids))
        return OH_E_ARG;
    std::string why;
    if (packing_check(pk, &why))                                /* also of a call without pictures */
        return refuse(e, OH_E_ARG, who, why);
    if (!n)
        return OH_OK;
    std::vector<int> views;
    if (view0_ids) views.insert(views.end(), view0_ids, view0_ids + n);
    if (view1_ids) views.insert(views.end(), view1_ids, view1_ids + n);
    const Pic *P0, *v0;
    OH_TRY(srcs_dsts(e, who, src_ids, n, views.data(), (int)views.size(), &P0, &v0));
    int full = 0;
    OH_TRY(packing_sizes(e, who, pk, P0, v0, &full));
    OhPkArgs a;
    packing_args(pk, P0, v0, full, &a);
    class_sizes(v0, a.np, a.dw, a.dh);
    a.views = (view0_ids ? 1 : 0) | (view1_ids ? 2 : 0);
    const int *const view_ids[2] = { view0_ids, view1_ids };
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, src_ids[i0 + i]), a.np, a.packed[i]);
            for (int v = 0; v < 2; v++)
                if (view_ids[v])
                    write_planes(get_pic(e, view_ids[v][i0 + i]), a.np, a.view[v][i]);
        }
        ohk_unpack(&a, m, e->stream);
    }, OH_PK_MAX_PICS);
}

extern "C" int oh_pics_pack(OhEngine *e, const int *view0_ids, const int *view1_ids, const int *dst_ids, int n, const OhPacking *pk)
{
    const char *who = "oh_pics_pack";
    if (!e || n < 0 || !pk || (n && (!view0_ids || !view1_ids || !dst_ids)))
        return OH_E_ARG;
    std::string why;
    if (packing_check(pk, &why))
        return refuse(e, OH_E_ARG, who, why);
    if (!n)
        return OH_OK;
    std::vector<int> views(view0_ids, view0_ids + n);
    views.insert(views.end(), view1_ids, view1_ids + n);
    const Pic *v0, *P0;
    OH_TRY(srcs_dsts(e, who, views.data(), 2 * n, dst_ids, n, &v0, &P0));
    int full = 0;
    OH_TRY(packing_sizes(e, who, pk, P0, v0, &full));
    if (!pk->quincunx) {
        /* where the half size rounds up to the full size, the views are taken as halves: there is no other way to pack them */
        PkPlane pl[2];
        OhPicParams half;
        (void)packing_geometry(pk, &P0->p, 0, pl, &half, &why);
        if (v0->p.width == half.width && v0->p.height == half.height)
            full = 0;
        else
            FAIL(e, OH_E_UNSUPPORTED, "%s: full-size views of %dx%d without quincunx sampling: packing them needs the anti-aliased 2 : 1, which is "
                 "oh_pics_resize's; resize, then pack the halves", who, v0->p.width, v0->p.height);
    } else if (!full)
        FAIL(e, OH_E_ARG, "%s: half-size views of %dx%d with quincunx sampling: the lattice is taken from full-size views of %dx%d", who,
             v0->p.width, v0->p.height, P0->p.width, P0->p.height);
    OhPkArgs a;
    packing_args(pk, P0, v0, full, &a);
    class_sizes(P0, a.np, a.dw, a.dh);
    a.views = 3;
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, view0_ids[i0 + i]), a.np, a.view[0][i]);
            read_planes(get_pic(e, view1_ids[i0 + i]), a.np, a.view[1][i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), a.np, a.packed[i]);
        }
        ohk_pack(&a, m, e->stream);
    }, OH_PK_MAX_PICS);
}

/* ---------------- motion search and compensation (motion.hip) ---------------- */
extern "C" int oh_pics_motion(OhEngine *e, const int *cur_ids, const int *ref_ids, int n, const OhMotionSearch *ms, OhMotionVector *out)
{
    const char *who = "oh_pics_motion";
    if (!e || n < 0 || !ms || !out || (n && (!cur_ids || !ref_ids)))
        return OH_E_ARG;
    std::string why;
    if (motion_check(ms, 0, &why))
        return refuse(e, OH_E_ARG, who, why);
    if (!n)
        return OH_OK;
    std::vector<int> all(cur_ids, cur_ids + n);
    all.insert(all.end(), ref_ids, ref_ids + n);
    const Pic *p0 = alike_pics(e, who, all.data(), 2 * n);
    if (!p0) return OH_E_ARG;
    const OhPicParams &p = p0->p;
    OhMoSearchArgs a;
    memset(&a, 0, sizeof(a));
    a.w = p0->w[0]; a.h = p0->h[0]; a.bd = p.bit_depth;
    a.block = ms->block;
    (void)oh_motion_blocks(a.w, a.h, a.block, &a.bw, &a.bh);
    const size_t per_pair = (size_t)a.bw * a.bh;
    if (motion_check(ms, (size_t)n * per_pair, &why))
        return refuse(e, OH_E_ARG, who, why);
    HIPCHK(e, hipSetDevice(e->device));
    int32_t pitch[3];
    row_pitches(p0, 1, pitch);
    a.pitch = pitch[0];
    a.rx = ms->range_x; a.ry = ms->range_y; a.subpel = ms->subpel; a.lambda = ms->lambda;
    if (ms->centres)                                            /* growing the scratch frees the old block, which waits for the device */
        OH_TRY(upload_copy(e, who, "vectors", &e->motion_centres, (size_t)n * per_pair * sizeof(OhMoVec), ms->centres));
    const size_t bytes = (size_t)n * per_pair * sizeof(OhMoDev);
    OhEngine::Stage *sg = nullptr;
    OH_TRY(results_begin(e, who, &e->motion_res, bytes, n, &sg));
    OH_TRY(launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            a.cur[i] = final_planes(get_pic(e, cur_ids[i0 + i]))[0];
            a.ref[i] = final_planes(get_pic(e, ref_ids[i0 + i]))[0];
        }
        a.centres = ms->centres ? (const OhMoVec *)e->motion_centres.p + (size_t)i0 * per_pair : nullptr;
        a.res = (OhMoDev *)e->motion_res.p + (size_t)i0 * per_pair;
        ohk_motion_search(&a, m, e->stream);
    }));
    OH_TRY(results_fetch(e, &e->motion_res, bytes, sg));
    memcpy(out, sg->p, bytes);
    return OH_OK;
}

extern "C" int oh_pics_motion_compensate(OhEngine *e, const int *ref_ids, const int *dst_ids, int n, int block, const OhMotionVector *field)
{
    const char *who = "oh_pics_motion_compensate";
    if (!e || n < 0 || !field || (n && (!ref_ids || !dst_ids)))
        return OH_E_ARG;
    if (block != 8 && block != 16)
        FAIL(e, OH_E_ARG, "%s: block %d (8 or 16)", who, block);
    if (!n)
        return OH_OK;
    const Pic *p0 = alike_apart(e, who, std::vector<int>(ref_ids, ref_ids + n), dst_ids, n);
    if (!p0) return OH_E_ARG;
    const OhPicParams &p = p0->p;
    HIPCHK(e, hipSetDevice(e->device));
    OhMoCompArgs a;
    memset(&a, 0, sizeof(a));
    a.np = n_planes(p); a.bd = p.bit_depth;
    a.hs = oh_hshift(&p, 1); a.vs = oh_vshift(&p, 1);
    row_pitches(p0, a.np, a.pitch);
    class_sizes(p0, a.np, a.w, a.h);
    a.block = block;
    (void)oh_motion_blocks(a.w[0], a.h[0], block, &a.bw, &a.bh);
    const size_t per_pic = (size_t)a.bw * a.bh;
    const size_t n_vec = (size_t)n * per_pic;
    OH_TRY(upload(e, who, "vectors", &e->motion_field, n_vec * sizeof(OhMoVec), [&](void *h) {
        OhMoVec *xy = (OhMoVec *)h;                              /* the x and y of the field: what the kernel reads */
        for (size_t i = 0; i < n_vec; i++) { xy[i].x = field[i].x; xy[i].y = field[i].y; }
    }));
    return launch_sets(e, n, [&](int i0, int m) {
        for (int i = 0; i < m; i++) {
            read_planes(get_pic(e, ref_ids[i0 + i]), a.np, a.ref[i]);
            write_planes(get_pic(e, dst_ids[i0 + i]), a.np, a.dst[i]);
        }
        a.field = (const OhMoVec *)e->motion_field.p + (size_t)i0 * per_pic;
        ohk_motion_compensate(&a, m, e->stream);
    });
}

extern "C" int oh_pic_device_planes(OhEngine *e, int pic_id, void *planes[3], int32_t stride[3], int32_t width[3], int32_t height[3])
{
    if (!e)
        return OH_E_ARG;
    Pic *p = get_pic(e, pic_id);
    if (!p)
        FAIL(e, OH_E_ARG, "unknown picture %d", pic_id);
    for (int c = 0; c < 3; c++) {
        planes[c] = final_planes(p)[c];
        stride[c] = p->stride[c]; width[c] = p->w[c]; height[c] = p->h[c];
    }
    return OH_OK;
}

