/*
 * handover_layout.h — the device arena of one work list as a value.  handover_layout() states every segment once (source, bytes,
 * presence, the DevFrame field it backs) and places them; handover_bind() turns the table into the header's pointers for an arena
 * base; handover_copy_jobs() cuts the copied range into the pieces of the staging copy.  Pure host code: no HIP runtime call, no
 * engine — tests/handover_layout_check.cpp and tests/handover_chunk_check.cpp run all of it on the CPU.  handover_chunk_place() puts
 * the lists of one call into one arena, copied parts first.  A list, in this order, every segment 256-byte aligned:
 *   [copied: header, raw lists, side arrays, coefficient pool] [cleared: cursor, summary, ctu_seen, tu_keep]
 *   [device only: prepared lists, scratch] [residual pool] [SAO stale buffer]
 */
#ifndef OHEVC_HANDOVER_LAYOUT_H
#define OHEVC_HANDOVER_LAYOUT_H

#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "dev_frame.h"

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* n boundary strengths (0..2, one per byte: hevc_filter.c's vertical_bs / horizontal_bs) -> (n + 3) / 4 bytes, entry i in bits
 * 2 (i & 3) of byte i >> 2 — the form the deblock pass reads.  32 source bytes per step as eight 32-bit lanes (the compiler's vector
 * extension, lowered to whatever the build's baseline has: shifts, ORs and a narrowing, no lane multiply), each lane folded into its low
 * byte; then four bytes per multiply (the 2-bit fields land in the top byte), then the last one to three entries. */
static inline void pack_bs(uint8_t *dst, const uint8_t *src, size_t n)
{
    typedef uint32_t pb_u32x8 __attribute__((vector_size(32)));
    typedef uint8_t pb_u8x8 __attribute__((vector_size(8)));
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        pb_u32x8 x;
        memcpy(&x, src + i, 32);                               /* any alignment */
        x &= 0x03030303u;
        x |= x >> 6;                                           /* bytes 0 and 2 of a lane: entries 0|1 and 2|3 */
        x = (x | (x >> 12)) & 0xffu;
        const pb_u8x8 y = __builtin_convertvector(x, pb_u8x8);
        memcpy(dst + (i >> 2), &y, 8);
    }
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

/* what the host counts and checks before the hand-over (handover_host.h: handover_check_list) */
struct HostSide {
    OhPrepCounts cnt;
    uint32_t tu_cnt[4], n_cross;      /* transform blocks per size: launch sizes of the residual pass */
    bool     any_dense;               /* some transform block reads the coefficient pool */
    uint16_t ref_used;                /* bit i: some PU predicts from slot i */
    uint32_t ref_ok;                  /* bit i: slot i holds a picture of this geometry */
    const uint32_t *pu_off;           /* [2][n_pu + 1]: where every PU's blocks start in the two MC block lists */
};

/* the header as the host fills it: d is what the kernels see; the four maps of bs_in have no field there (only bs_kernel's launch
 * at the hand-over reads them; null without bs_in) */
struct HandoverHeader { DevFrame d; char *mvf, *cbf_luma, *call_log2, *ctb_flags; };
#define HL_FIELD(m) offsetof(HandoverHeader, m)
enum : size_t { HL_NO_FIELD = ~(size_t)0 };

struct HandoverSeg {
    const void *src;                  /* null: device only */
    size_t bytes, field;              /* field: the HandoverHeader pointer that addresses the segment */
    bool   null_field;                /* the data is absent and the kernels are told so by a null pointer */
    bool   own;                       /* made by the hand-over itself: staged even when the caller's arrays are pulled */
    size_t pack_n;                    /* != 0: src holds pack_n boundary strengths, one per byte */
    size_t off;
};
enum { HL_OPT = 1, HL_OWN = 2 };
/* `bytes` at src when `have`, else an empty segment; HL_OPT: whose pointer is then null */
static inline HandoverSeg hl_in(bool have, const void *src, size_t bytes, size_t field, int how = 0, size_t pack_n = 0)
{
    return HandoverSeg{ have ? src : nullptr, have ? bytes : 0, field, (how & HL_OPT) && !have, (how & HL_OWN) != 0, pack_n, 0 };
}
static inline HandoverSeg hl_dev(size_t bytes, size_t field) { return HandoverSeg{ nullptr, bytes, field, false, false, 0, 0 }; }

enum { HL_N_SEGS = 43 };
struct HandoverLayout {
    HandoverSeg seg[HL_N_SEGS];
    int    ns;
    size_t copy_bytes;                /* what crosses PCIe: [0, copy_bytes) */
    size_t zero_off, zero_bytes;      /* cleared before the preparation kernels run */
    size_t res_off, stale_off, stale_bytes, total;
    size_t own_bytes;                 /* of the `own` segments, each padded to 256: what the pulled form stages */
    bool   packs;                     /* the grids come one strength per byte: packed on the way into the staging buffer */
    bool copied(const HandoverSeg &s) const { return s.bytes && s.src && s.off + s.bytes <= copy_bytes; }
};

template <size_t N> static inline void hl_place(HandoverLayout *L, const HandoverSeg (&segs)[N])
{
    for (const HandoverSeg &s : segs) {
        HandoverSeg &d = L->seg[L->ns++];
        d = s;
        d.off = L->total;
        L->total += align_up(s.bytes ? s.bytes : 1, 256);        /* an empty segment keeps its place */
        if (s.own) L->own_bytes += align_up(s.bytes, 256);
    }
}

/* hdr: where the caller will fill the header (copied from there); h: the counts of this very list */
static inline HandoverLayout handover_layout(const OhFrame *f, const HostSide &h, const DevFrame *hdr)
{
    const OhPicParams &p = f->p;
    const OhPrepCounts &cnt = h.cnt;
    const size_t n_ctb = (size_t)oh_ctb_width(&p) * oh_ctb_height(&p);
    const size_t n_pcm = (size_t)oh_min_pu_width(&p) * oh_min_pu_height(&p);
    const size_t n_mtb = (size_t)(p.width >> p.log2_min_tb_size) * (p.height >> p.log2_min_tb_size);
    const bool has_sao = p.sao_enabled && f->sao;
    const bool has_db = p.deblock_enabled != 0;
    const uint32_t n_levels = f->n_intra ? f->n_levels : 0;
    const bool cip = p.constrained_intra_pred && f->is_intra;
    static const OhBsInputs no_maps{};
    const bool bsi = has_db && f->bs_in;                      /* with bs_in the grids are written by bs_kernel after the copy */
    const OhBsInputs &bm = bsi ? *f->bs_in : no_maps;
    const size_t bs_bytes = bsi ? oh_bs_size(&p) : f->bs_size;
    /* the grids cross PCIe and live in HBM four strengths to the byte (0..2 each: 2 bits) — a megabyte less per 4K picture */
    const size_t bs_packed = (bs_bytes + 3) / 4;
    const bool packs = has_db && !bsi && !(f->flags & OH_FRAME_BS_PACKED);
    /* the PCM / bypass map is read by the deblock and SAO passes only under these two flags (hevc_filter.c:180, 337; deblock.hip, sao.hip):
     * without them its half megabyte per 4K picture stays on the host */
    const bool need_pcm = f->is_pcm && (p.pcm_loop_filter_disable || p.transquant_bypass_enable);
    const bool has_pend = has_sao && f->sao_pending && oh_sao_stale_config(&p);     /* tiled pictures: the driver order as bits per CTB */

    const HandoverSeg copied[] = {
        hl_in(true, hdr, sizeof(DevFrame), HL_NO_FIELD, HL_OWN),
        hl_in(true, f->pu, (size_t)f->n_pu * sizeof(OhPu), HL_FIELD(d.pu)),
        hl_in(true, h.pu_off, 2 * ((size_t)f->n_pu + 1) * sizeof(uint32_t), HL_FIELD(d.pu_off), HL_OWN),
        hl_in(true, f->wp, (size_t)f->n_wp * sizeof(OhWeights), HL_FIELD(d.wp)),
        hl_in(true, f->tu, (size_t)f->n_tu * sizeof(OhTu), HL_FIELD(d.tu_raw)),
        hl_in(f->tu_sparse, f->tu_sparse, (size_t)f->n_tu * sizeof(uint32_t), HL_FIELD(d.tu_sparse), HL_OPT),
        hl_in(f->tu_cross, f->tu_cross, (size_t)f->n_tu * sizeof(uint32_t), HL_FIELD(d.tu_cross), HL_OPT),
        hl_in(f->sparse, f->sparse, (size_t)f->n_sparse * sizeof(uint32_t), HL_FIELD(d.sparse), HL_OPT),
        hl_in(f->scaling, f->scaling, sizeof(OhScalingList), HL_FIELD(d.scaling), HL_OPT),
        hl_in(true, f->intra, (size_t)f->n_intra * sizeof(OhIntra), HL_FIELD(d.intra_raw)),
        hl_in(cnt.n_ictu, f->ictu, (size_t)cnt.n_ictu * sizeof(OhIntraCtu), HL_FIELD(d.ictu_raw)),
        hl_in(n_levels, f->level_start, ((size_t)n_levels + 1) * sizeof(uint32_t), HL_FIELD(d.lvl_start)),
        hl_in(cnt.n_sub, f->sub_start, ((size_t)cnt.n_sub + 1) * sizeof(uint32_t), HL_FIELD(d.sub_start)),
        hl_in(cip, f->is_intra, n_pcm, HL_FIELD(d.is_intra), HL_OPT),
        hl_in(has_db, bsi ? nullptr : f->vertical_bs, bs_packed, HL_FIELD(d.vbs), 0, packs ? bs_bytes : 0),
        hl_in(has_db, bsi ? nullptr : f->horizontal_bs, bs_packed, HL_FIELD(d.hbs), 0, packs ? bs_bytes : 0),
        hl_in(bsi, bm.mvf, n_pcm * sizeof(OhMvField), HL_FIELD(mvf), HL_OPT),
        hl_in(bsi, bm.cbf_luma, n_mtb, HL_FIELD(cbf_luma), HL_OPT),
        hl_in(bsi, bm.call_log2, n_mtb, HL_FIELD(call_log2), HL_OPT),
        hl_in(bsi, bm.ctb_flags, n_ctb, HL_FIELD(ctb_flags), HL_OPT),
        hl_in(has_db, f->qp_y_tab, oh_qp_tab_size(&p), HL_FIELD(d.qp)),
        hl_in(need_pcm, f->is_pcm, n_pcm, HL_FIELD(d.is_pcm), HL_OPT),
        hl_in(has_db, f->deblock, n_ctb * sizeof(OhDeblockCtb), HL_FIELD(d.db)),
        hl_in(has_sao, f->sao, n_ctb * sizeof(OhSaoCtb), HL_FIELD(d.sao), HL_OPT),
        hl_in(has_pend, f->sao_pending, n_ctb, HL_FIELD(d.sao_pending), HL_OPT),
        hl_in(true, f->coeffs, (size_t)f->n_coeff * sizeof(int16_t), HL_FIELD(d.coeffs)),
    };
    const HandoverSeg cleared[] = {
        hl_dev(16 * sizeof(uint32_t), HL_FIELD(d.tu_cursor)),
        hl_dev(sizeof(DevSummary), HL_FIELD(d.summary)),
        hl_dev(cnt.n_intra ? n_ctb * sizeof(uint32_t) : 0, HL_FIELD(d.ctu_seen)),
        hl_dev(f->n_tu, HL_FIELD(d.tu_keep)),
    };
    const HandoverSeg device[] = {
        hl_dev((size_t)cnt.n_mc_luma * sizeof(DevMcJob), HL_FIELD(d.mc_luma)),
        hl_dev((size_t)cnt.n_mc_chroma * sizeof(DevMcJob), HL_FIELD(d.mc_chroma)),
        hl_dev((size_t)cnt.n_ictu * sizeof(uint32_t), HL_FIELD(d.ctu_aux)),
        hl_dev((size_t)f->n_tu * sizeof(DevTu), HL_FIELD(d.tu)),
        hl_dev((size_t)h.n_cross * sizeof(DevCross), HL_FIELD(d.cross)),
        hl_dev((size_t)f->n_intra * sizeof(DevIntra), HL_FIELD(d.intra)),
        hl_dev((size_t)cnt.n_ictu * sizeof(DevIntraCtu), HL_FIELD(d.ictu)),
        hl_dev((size_t)cnt.n_sub * sizeof(uint32_t), HL_FIELD(d.sub_small)),          /* and sub_small_w */
        hl_dev((size_t)f->n_intra * sizeof(uint32_t), HL_FIELD(d.intra_perm)),
        hl_dev((size_t)cnt.n_ictu * 4 * sizeof(uint32_t), HL_FIELD(d.ctu_wait)),
        hl_dev((size_t)cnt.n_ictu * sizeof(uint32_t), HL_FIELD(d.ctu_done)),
        hl_dev((size_t)cnt.n_ictu * sizeof(uint32_t), HL_FIELD(d.ctu_lvl)),
        hl_dev((size_t)cnt.n_ictu * sizeof(uint32_t), HL_FIELD(d.ctu_order)),
    };
    static_assert(sizeof(copied) + sizeof(cleared) + sizeof(device) == HL_N_SEGS * sizeof(HandoverSeg), "HandoverLayout::seg[] holds exactly the segments stated here");

    HandoverLayout L;
    L.ns = 0; L.total = 0; L.own_bytes = 0; L.packs = packs;
    hl_place(&L, copied);
    /* the dense pool is the last copied segment: when every block came as levels nothing of it crosses PCIe */
    L.copy_bytes = h.any_dense || !f->n_tu ? L.total : L.seg[L.ns - 1].off;
    L.zero_off = L.total;
    hl_place(&L, cleared);
    L.zero_bytes = L.total - L.zero_off;
    hl_place(&L, device);
    L.res_off = L.total;
    L.total += align_up((size_t)(f->n_coeff ? f->n_coeff : 1) * sizeof(int16_t), 256);
    L.stale_off = L.total;                                     /* see DevFrame.sao_stale */
    L.stale_bytes = has_db && has_sao && oh_sao_stale_config(&p) ? oh_sao_stale_index(&p, 3, 0, 0) * sizeof(uint16_t) : 0;
    if (L.stale_bytes)
        L.total += align_up(L.stale_bytes, 256);
    return L;
}

/* where offset `off` of a list lies when its copied part [0, copy_bytes) stands at copied_base and the rest at rest_base */
static inline char *hl_at(const HandoverLayout &L, char *copied_base, char *rest_base, size_t off)
{
    return off < L.copy_bytes ? copied_base + off : rest_base + (off - L.copy_bytes);
}

/* the header's pointers for a list in two parts (a chunk's arena: handover_chunk_place); no segment straddles copy_bytes */
static inline void handover_bind_split(const HandoverLayout &L, char *copied_base, char *rest_base, HandoverHeader *H)
{
    for (int i = 0; i < L.ns; i++)
        if (L.seg[i].field != HL_NO_FIELD) {
            char *at = L.seg[i].null_field ? nullptr : hl_at(L, copied_base, rest_base, L.seg[i].off);
            memcpy((char *)H + L.seg[i].field, &at, sizeof(at));
        }
    H->d.sub_small_w = (uint32_t *)H->d.sub_small;
    H->d.res = (int16_t *)hl_at(L, copied_base, rest_base, L.res_off);
    H->d.sao_stale = L.stale_bytes ? (uint16_t *)hl_at(L, copied_base, rest_base, L.stale_off) : nullptr;
    H->d.zero_ptr = (uint32_t *)hl_at(L, copied_base, rest_base, L.zero_off); H->d.zero_words = (uint32_t)(L.zero_bytes / 4);
}

/* the header's pointers for an arena at `base` that holds the list in one piece */
static inline void handover_bind(const HandoverLayout &L, char *base, HandoverHeader *H)
{
    handover_bind_split(L, base, base + L.copy_bytes, H);
}

/* The arena of a chunk: the lists handed over in one call (at most OH_MAX_BATCH) share one arena,
 *   [copied part of list 0 | ... | copied part of list n-1 | rest of list 0 | ... | rest of list n-1]
 * every part 256-byte aligned, so that all the bytes that cross PCIe are one range, [0, copy_bytes), and any run of consecutive
 * lists is copied with one request.  A list's copied part is [0, L.copy_bytes) of its own layout, its rest [L.copy_bytes, L.total). */
struct HandoverChunk {
    int    n;
    size_t copied_off[OH_MAX_BATCH + 1];  /* where list i's copied part starts; [n] = copy_bytes */
    size_t rest_off[OH_MAX_BATCH];        /* where its rest starts */
    size_t copy_bytes, total;
};
static inline HandoverChunk handover_chunk_place(const HandoverLayout *L, int n)
{
    HandoverChunk C;
    memset(&C, 0, sizeof(C));
    C.n = n;
    size_t at = 0;
    for (int i = 0; i < n; i++) { C.copied_off[i] = at; at += align_up(L[i].copy_bytes, 256); }
    C.copied_off[n] = C.copy_bytes = at;
    for (int i = 0; i < n; i++) { C.rest_off[i] = at; at += align_up(L[i].total - L[i].copy_bytes, 256); }
    C.total = at;
    return C;
}

/* the one host copy of the hand-over (the work list into a pinned staging buffer laid out like the arena) as jobs for the copy helpers:
 * pieces of at most 128 KB; a byte grid is packed on the way, four source bytes per byte: pieces of 4 x 128 KB strengths */
struct CopyJob { char *dst; const char *src; size_t n; bool pack; };
/* adds the jobs of one list whose copied part is staged at `stage` (a group of lists is staged by ONE run over the jobs of all of them) */
static inline void handover_copy_jobs_add(const HandoverLayout &L, char *stage, std::vector<CopyJob> &jobs)
{
    const size_t piece = 128 * 1024;
    for (int i = 0; i < L.ns; i++) {
        const HandoverSeg &s = L.seg[i];
        if (!L.copied(s))
            continue;
        const size_t n = s.pack_n ? s.pack_n : s.bytes, step = s.pack_n ? 4 * piece : piece;
        for (size_t o = 0; o < n; o += step)
            jobs.push_back({ stage + s.off + (s.pack_n ? o / 4 : o), (const char *)s.src + o, std::min(step, n - o), s.pack_n != 0 });
    }
}
static inline void handover_copy_jobs(const HandoverLayout &L, char *stage, std::vector<CopyJob> &jobs)
{
    jobs.clear();
    handover_copy_jobs_add(L, stage, jobs);
}

#endif
