/*
 * engine_impl.h — what the engine's translation units share: the engine and picture structures, the error macros and the few
 * helpers more than one of them uses.  engine.hip: engine and picture lifecycle, staging buffers, passes, profiling;
 * engine_handover.hip: work-list hand-over and the arena pool (its host-only parts, which run on several threads, are handover_layout.h
 * and handover_host.h: the layout, the check-and-count of a list and the thread pool, none of which knows the engine; likewise
 * engine_tuning.h, the OHEVC_* switches read once per engine, and intra_plan.h, the forms and the launch plan of the intra pass); engine_pics.hip: plane transfers, hashes, conversion, import, measurement,
 * comparison, resizing, composition, histograms and look-up tables of finished pictures, with the helpers those services share; engine_shvc.hip: SHVC up-sampling.
 * pics_math.hip, the services' host arithmetic, takes no engine and does not include this file (pics_math.h).
 * Internal: the C ABI is include/ohevc_hip.h.
 */
#ifndef OHEVC_ENGINE_IMPL_H
#define OHEVC_ENGINE_IMPL_H

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <string>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/ohevc_hip.h"
#include "handover_layout.h"
#include "handover_host.h"              /* CopyPool, handover_check_chunk: host-only, shared with the CPU checks */
#include "engine_tuning.h"
#include "intra_plan.h"
#include "kernels.h"

#define OH_INTERNAL __attribute__((visibility("hidden")))    /* shared between the engine's files, not part of the library's ABI */

struct Pic {
    bool        used = false;
    OhPicParams p{};
    void       *base = nullptr;          /* one allocation: planes A (recon/deblock) then B (SAO out) */
    bool        owned = true;            /* false: caller-owned memory (oh_pic_wrap)                   */
    void       *a[3] = {}, *b[3] = {};
    int32_t     stride[3] = {}, w[3] = {}, h[3] = {};
    bool        final_b = false;         /* which buffer holds the finished picture */
    uint32_t    gen = 0;                 /* bumped whenever the id is (re)installed: uploaded work lists remember it */
    uint64_t    done_seq = 0;            /* the batch that last reconstructed the picture (OhEngine::batch_ev ring); 0: written by something else, or never */
};

struct EventSet { hipEvent_t ev[OH_N_PASSES + 1]; int n_frames = 1; };

/* What the work lists handed over in one oh_frames_upload call (at most OH_MAX_BATCH of them) share: one device arena
 * (handover_layout.h: handover_chunk_place), one `ready` event and one pinned block for their summaries.  A list uploaded alone is a
 * chunk of one.  The lists are executed, released and freed one by one and in any order; the arena returns to the pool with the last. */
struct OhChunk {
    void      *arena = nullptr;
    size_t     arena_bytes = 0;
    hipEvent_t ready = nullptr;   /* recorded on the copy stream behind the chunk's H2D copies, preparation kernels and summaries */
    bool       waited = false;    /* the engine stream already waits for `ready` */
    void      *sum_host = nullptr;/* pinned: OH_MAX_BATCH DevSummary, one per list */
    int        refs = 0;          /* lists not yet released or freed */
    bool       in_flight = false; /* some list was released while passes that read the arena could still be running */
};

struct OhDevFrame {
    OhChunk   *chunk = nullptr;
    DevFrame  *d = nullptr;       /* the start of the list's copied part in the chunk's arena */
    OhPicParams p{};
    uint32_t   tu_cnt[4] = { 0, 0, 0, 0 };
    uint32_t   n_cross = 0;
    bool       has_sao = false;
    int        cur_pic = -1;      /* engine id of the picture the list reconstructs */
    uint32_t   cur_gen = 0;
    /* reference slots as uploaded: picture id, its generation, and which half DevFrame.refs[] points at — looked up again at
     * every execute (a reference finished or received AFTER the upload moves to its other half: oh_pic_set_final_half, SAO) */
    int        ref_id[OH_MAX_REFS];
    uint32_t   ref_gen[OH_MAX_REFS];
    uint8_t    ref_half[OH_MAX_REFS];
    uint16_t   ref_used = 0;      /* bit i: some PU predicts from slot i */
    void      *sum_host = nullptr;/* pinned, inside chunk->sum_host: the DevSummary the preparation kernels left */
    bool       summary_read = false;
    void      *sum_dev = nullptr; /* the summary in the arena */
    OhPrepCounts cnt{};           /* sizes of the preparation launches */
    uint32_t   prep_err = 0;
    uint32_t   intra_area64 = 0, max_passes = 0;   /* from the summary: samples of the intra blocks / 64; wave passes of the heaviest CTU */
    /* from the summary, over the schedule entries: what lays out the staged intra launch */
    uint32_t   max_items = 0, max_sub = 0, max_res = 0;
    bool       res_scattered = false;             /* some CTU's residual span is not contiguous (not stageable in LDS) */
    uint64_t   sum_items = 0, sum_sub = 0;
    const struct OhEngine *owner = nullptr;   /* picture ids and arenas belong to one engine */
};

struct OhEngine {
    int         device = 0;
    int         n_cu = 256;              /* compute units of the device */
    hipStream_t stream = nullptr;
    bool        own_stream = true;
    std::vector<Pic> pics;
    std::string err;
    int         profile = 0;             /* 0 off, 1 events between passes, 2 also around every batch's intra launches */
    std::vector<EventSet> ev_pool, ev_pending;
    std::vector<hipEvent_t> lev_pool, lev_pending;   /* event pairs around every batch's intra launches (profile mode) */
    double      intra_launch_ms = 0;
    uint64_t    intra_launches = 0;
    double      pass_ms[OH_N_PASSES] = {};
    uint64_t    executes = 0;
    std::vector<OhDevFrame *> deferred;
    uint32_t    pic_gen = 0;
    /* upload path: pinned staging buffers and device arenas are recycled (hipHostMalloc / hipMalloc cost milliseconds);
     * a staging buffer is busy until the H2D copy that reads it has passed `done` */
    struct Stage { void *p; size_t bytes; hipEvent_t done; bool busy; };
    std::vector<Stage> stages;
    /* work lists travel on their own stream so that the copy of picture n+1 overlaps the passes of picture n; the engine stream
     * waits for a list's `ready` event before the first kernel that reads it, and a recycled arena is not overwritten before
     * the engine stream has passed the event recorded when it was released */
    hipStream_t copy_stream = nullptr;
    struct Arena { void *p; size_t bytes; hipEvent_t free_ev; };
    std::vector<Arena> arenas;               /* free device arenas */
    uint64_t    arenas_alive = 0, arena_bytes_alive = 0;      /* device arenas allocated and not freed (pooled or holding a work list): oh_engine_memory */
    std::vector<hipEvent_t> sync_events;     /* pool of timing-disabled events (ready / free_ev) */
    std::vector<void *> sum_pool;            /* pinned blocks of OH_MAX_BATCH * sizeof(DevSummary) bytes: one per chunk */
    double      host_ms[OH_N_HOST_TIMES] = {};   /* where the host time of the hand-over path goes (oh_engine_host_times) */
    uint64_t    host_calls[OH_N_HOST_TIMES] = {};
    uint64_t    up_bytes = 0;                    /* bytes of work lists sent over PCIe since the last reset */
    uint64_t   *dbg = nullptr;           /* diagnostics (OhTuning::stamps + a -DOH_STAMPS build) */
    /* what a kernel can tell the host when it cannot go on (the table slots and the passes have no error channel: hevcdsp.h's slots
     * return void): four words of pinned host memory, [0] OH_KE_* of the first failure, [1] picture id, [2] schedule
     * entry; read by everything that waits for the stream (kernel_error) */
    /* a ring of events, one behind every executed batch: a download of a finished picture waits for ITS batch (on the download
     * stream), not for everything enqueued since — a decoder fetches the picture it outputs while the passes of the pictures it
     * submitted later keep running */
    enum { BATCH_RING = 64 };
    hipEvent_t  batch_ev[BATCH_RING] = {};
    uint64_t    batch_seq = 0;
    hipStream_t dl_stream = nullptr;
    /* ticket counters of the one-launch intra forms: a ring of pairs (direct, staged) in HBM; a batch uses the next pair, cleared on
     * the stream in front of its launches (a pair comes round again 128 batches later: long after its launch has drained) */
    enum { TICKET_RING = 128, TICKET_WORDS = 2 * OH_MAX_BATCH * 32 };      /* per batch: (direct, staged) x pictures, a cache line each (intra.hip: OH_TICKET_STRIDE) */
    uint32_t   *tickets = nullptr;
    uint64_t    ticket_seq = 0;
    /* the hand-over's helper threads (handover_host.h; OhTuning::copy_threads of them, 0: the submitter does everything alone
     * on the same code path): started by the first hand-over BEFORE its check-and-count phase, which they share list by list, as they
     * share the staging copy piece by piece.  They see lists and staging memory, never the engine */
    CopyPool   *copiers = nullptr;
    /* output fetch (oh_pic_download_start / oh_download_finish): its own pinned buffers and copy helpers, usable while another thread
     * drives the engine */
    std::mutex  dl_mu, dl_copy_mu;
    std::vector<Stage *> dl_stages;
    CopyPool   *dl_copiers = nullptr;   /* created with the first fetch (OhTuning::fetch_threads helpers) */
    std::vector<CopyJob> dl_jobs;
    double      dl_wait_ms = 0, dl_copy_ms = 0;     /* OhTuning::fetch_timing: where the time of the fetches went (printed when the engine is destroyed) */
    uint64_t    dl_count = 0;
    std::vector<CopyJob> copy_jobs;
    uint32_t   *kerr = nullptr;
    /* grow-only device scratch (engine_pics.hip: scratch_reserve); reallocated only while the engine stream is idle */
    struct Scratch { void *p = nullptr; size_t bytes = 0; };
    Scratch     hash_dev;                /* oh_pics_hash (CRC / checksum): the job table, its tasks and their values in HBM */
    Scratch     resize_dev;              /* oh_pics_resize: the tap tables of the call, then the int16 intermediate of one launch set */
    /* the tables of the last OhColour a service built (the host's work: a few thousand pow calls), host and device
     * (engine_pics.hip: table_stage); on_dev: the device copy holds them too, so a call with the same OhColour copies nothing */
    struct TableCache {
        OhColour last;
        bool     cached = false, on_dev = false;
        std::vector<int32_t> tab;        /* OH_COLT_N as colour_build lays them out; the entries the service reads go to the device */
        int32_t  misc[OH_COL_NMISC];
        Scratch  dev;
    };
    TableCache  colour_tabs;             /* oh_pics_convert_colour: the three tables of the call (OH_COLT_N int32) */
    TableCache  light_tabs;              /* oh_pics_light_level: table A of its last source curve (OH_COLT_G int32), apart from colour_tabs:
                                          * neither call disturbs the tables the other has cached */
    Scratch     light_res;               /* oh_pics_light_level: the results of the call in HBM */
    Scratch     compare_res;             /* oh_pics_compare: the results of the call in HBM */
    Scratch     hist_res;                /* oh_pics_histogram: the bins of the call in HBM */
    Scratch     lut_tabs;                /* oh_pics_lut: the three tables of the last call (3 x OH_LUT_MAX uint16), rewritten on the stream
                                          * behind the launches that read them */
    Scratch     grain_tabs;              /* oh_pics_grain: the three tables (3 x OH_GRAIN_ENTRIES uint32) and the seeds of the last call, likewise */
    Scratch     grain_patterns;          /* oh_pics_grain: the 169 patterns, built and copied by the engine's first call, then only read */
    bool        grain_patterns_ready = false;
    Scratch     remap_tabs;              /* oh_pics_colour_remap: the six tables of the last call (6 x OH_LUT_MAX uint16), rewritten on the
                                          * stream behind the launches that read them */
    Scratch     motion_res;              /* oh_pics_motion: the vectors of the call in HBM */
    Scratch     motion_centres;          /* oh_pics_motion: the centres of the call, rewritten on the stream behind the launches that read them */
    Scratch     motion_field;            /* oh_pics_motion_compensate: the vectors of the call, likewise */
    Scratch     compose_dev;           /* oh_pics_compose: the layer table of the call (OhCpsLayer, then OhCpsSrc per launch set) */
    OhTuning    tuning;                  /* the OHEVC_* switches as engine_create found them (engine_tuning.h) */
};

#define HIPCHK(e, call)                                                                           \
    do {                                                                                          \
        hipError_t rc_ = (call);                                                                  \
        if (rc_ != hipSuccess) {                                                                  \
            char buf_[512];                                                                       \
            snprintf(buf_, sizeof(buf_), "%s failed: %s (%s:%d)", #call, hipGetErrorString(rc_), __FILE__, __LINE__); \
            (e)->err = buf_;                                                                      \
            return OH_E_HIP;                                                                      \
        }                                                                                         \
    } while (0)

#define FAIL(e, code, ...)                                                                        \
    do {                                                                                          \
        char buf_[512];                                                                           \
        snprintf(buf_, sizeof(buf_), __VA_ARGS__);                                                \
        (e)->err = buf_;                                                                          \
        return (code);                                                                            \
    } while (0)

/* a step that sets the message itself: its code, where it is not OH_OK, is the caller's */
#define OH_TRY(expr)                                                                              \
    do {                                                                                          \
        const int try_rc_ = (expr);                                                               \
        if (try_rc_) return try_rc_;                                                              \
    } while (0)

struct HostTimer {                       /* adds the scope's wall time to one slot of OhEngine::host_ms */
    OhEngine *e; int slot; std::chrono::steady_clock::time_point t0;
    HostTimer(OhEngine *e_, int slot_);
    ~HostTimer();
};
/* pinned staging memory per engine before the host is made to wait (48 buffers of 4 MiB when every list came alone; a group of
 * OH_STAGE_GROUP lists is staged in one buffer: one chunk of 32 4K lists, 132 MB, at a time) */
enum : size_t { OH_STAGE_POOL_BYTES = (size_t)48 * ((size_t)4 << 20) };
/* lists staged into one pinned buffer and sent with ONE copy request: a chunk of OH_MAX_BATCH lists puts OH_MAX_BATCH / OH_STAGE_GROUP
 * copies on the copy stream.  Smaller groups let the DMA start before the host has staged the whole chunk, larger ones put fewer
 * commands on the stream, and that is what counts: 4K Main 10 decode, six runs each beside the parent's 63.5-65.8 Gpixels/s, gave
 * 63.4-70.5 at 8, 65.7-69.0 at 16 and 82.1-87.8 at 32 (profiles/r10_chunk_handover.txt) */
#ifndef OH_STAGE_GROUP
#define OH_STAGE_GROUP 32
#endif

/* the planes of the half that holds the finished picture, and the bytes of one of its samples */
static inline void *const *final_planes(const Pic *p) { return p->final_b ? p->b : p->a; }
static inline int sample_bytes(int bit_depth) { return bit_depth > 8 ? 2 : 1; }
static inline void fill_planes(DevPlanes *dp, const Pic *p, bool use_b)
{
    for (int c = 0; c < 3; c++) {
        dp->p[c] = use_b ? p->b[c] : p->a[c];
        dp->stride[c] = p->stride[c];
        dp->w[c] = p->w[c];
        dp->h[c] = p->h[c];
    }
}

OH_INTERNAL int kernel_error(OhEngine *e);
OH_INTERNAL int check_params(OhEngine *e, const OhPicParams *p);
OH_INTERNAL Pic *get_pic(OhEngine *e, int id);
OH_INTERNAL int check_pics(OhEngine *e, const int *pic_ids, int n, const char *who);
OH_INTERNAL bool stage_create(OhEngine::Stage *c, size_t bytes);
OH_INTERNAL OhEngine::Stage *stage_acquire(OhEngine *e, size_t bytes);
OH_INTERNAL OhEngine::Stage *stage_list(OhEngine *e, const void *list, size_t bytes);
OH_INTERNAL int stage_in_use(OhEngine *e, OhEngine::Stage *sg, hipStream_t st);
OH_INTERNAL hipEvent_t sync_event_get(OhEngine *e);
OH_INTERNAL void sync_event_put(OhEngine *e, hipEvent_t ev);
OH_INTERNAL void free_dev_frame(OhEngine *e, OhDevFrame *df, bool in_flight = false);

#endif
