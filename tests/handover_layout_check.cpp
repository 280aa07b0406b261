/* handover_layout_check.cpp — the arena layout of a work list, its binding to a header and the staging copy's jobs
 * (openhevc_amd/csrc/handover_layout.h) run on the CPU over small host arrays; built with AddressSanitizer and UBSan by
 * tests/test_handover_layout_host.py.  The staging block has exactly copy_bytes bytes and every source array exactly the bytes the
 * layout may read, so a job one byte out of place is a sanitizer report.  Exit status 0: every check of every list held. */
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../openhevc_amd/csrc/handover_layout.h"

static int failures;
static std::string list_name;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            failures++;                                                                    \
            fprintf(stderr, "%s: %s (line %d): ", list_name.c_str(), #cond, __LINE__);      \
            fprintf(stderr, __VA_ARGS__);                                                  \
            fprintf(stderr, "\n");                                                         \
        }                                                                                  \
    } while (0)

/* a host array of exactly n bytes with a pattern no two neighbours share (the two low bits take every value: packing sees them all) */
static void *bytes(std::vector<std::vector<uint8_t>> &keep, size_t n, unsigned seed)
{
    keep.emplace_back(n);
    for (size_t i = 0; i < n; i++) keep.back()[i] = (uint8_t)((i * 7 + seed * 13 + (i >> 8)) & 0xff);
    return n ? keep.back().data() : nullptr;
}

struct Spec {                       /* what a list carries, stated independently of the layout's own conditions */
    const char *name;
    int w, h, chroma, log2_ctb;
    bool deblock, sao, bs_in, scaling, sparse, cross, cip, pcm, pending, all_sparse, bs_packed_in;
    uint32_t n_pu, n_tu, n_intra, n_coeff;
    long bs_size;                   /* < 0: oh_bs_size() */
};

static void run(const Spec &s)
{
    list_name = s.name;
    std::vector<std::vector<uint8_t>> keep;
    OhFrame f;
    memset(&f, 0, sizeof(f));
    OhPicParams &p = f.p;
    p.width = s.w; p.height = s.h; p.bit_depth = 8; p.chroma_format_idc = s.chroma; p.log2_ctb_size = s.log2_ctb;
    p.log2_min_cb_size = 3; p.log2_min_tb_size = 2; p.log2_min_pu_size = 2;
    p.deblock_enabled = s.deblock; p.sao_enabled = s.sao; p.constrained_intra_pred = s.cip; p.pcm_loop_filter_disable = s.pcm;
    const size_t n_ctb = (size_t)oh_ctb_width(&p) * oh_ctb_height(&p), n_pcm = (size_t)oh_min_pu_width(&p) * oh_min_pu_height(&p);
    const size_t n_mtb = (size_t)(p.width >> 2) * (p.height >> 2);
    unsigned k = 0;
    f.n_pu = s.n_pu; f.pu = (const OhPu *)bytes(keep, s.n_pu * sizeof(OhPu), k++);
    f.n_wp = s.n_pu ? 2 : 0; f.wp = (const OhWeights *)bytes(keep, f.n_wp * sizeof(OhWeights), k++);
    f.n_tu = s.n_tu; f.tu = (const OhTu *)bytes(keep, s.n_tu * sizeof(OhTu), k++);
    f.n_coeff = s.n_coeff; f.coeffs = (const int16_t *)bytes(keep, s.n_coeff * sizeof(int16_t), k++);
    f.n_intra = s.n_intra; f.intra = (const OhIntra *)bytes(keep, s.n_intra * sizeof(OhIntra), k++);
    if (s.n_intra) {
        f.n_ictu = 3; f.ictu = (const OhIntraCtu *)bytes(keep, 3 * sizeof(OhIntraCtu), k++);
        f.n_sub = 5; f.sub_start = (const uint32_t *)bytes(keep, 6 * sizeof(uint32_t), k++);
        f.n_levels = 2; f.level_start = (const uint32_t *)bytes(keep, 3 * sizeof(uint32_t), k++);
    }
    f.bs_size = s.bs_size < 0 ? oh_bs_size(&p) : (uint32_t)s.bs_size;
    OhBsInputs bi;
    memset(&bi, 0, sizeof(bi));
    if (s.deblock) {
        if (s.bs_in) {
            bi.mvf = (const OhMvField *)bytes(keep, n_pcm * sizeof(OhMvField), k++);
            bi.cbf_luma = (const uint8_t *)bytes(keep, n_mtb, k++);
            bi.call_log2 = (const uint8_t *)bytes(keep, n_mtb, k++);
            bi.ctb_flags = (const uint8_t *)bytes(keep, n_ctb, k++);
            f.bs_in = &bi;
        } else {
            const size_t n = s.bs_packed_in ? (f.bs_size + 3) / 4 : f.bs_size;
            f.vertical_bs = (const uint8_t *)bytes(keep, n, k++);
            f.horizontal_bs = (const uint8_t *)bytes(keep, n, k++);
            if (s.bs_packed_in) f.flags |= OH_FRAME_BS_PACKED;
        }
        f.qp_y_tab = (const int8_t *)bytes(keep, oh_qp_tab_size(&p), k++);
        f.deblock = (const OhDeblockCtb *)bytes(keep, n_ctb * sizeof(OhDeblockCtb), k++);
    }
    if (s.pcm) f.is_pcm = (const uint8_t *)bytes(keep, n_pcm, k++);
    if (s.sao) f.sao = (const OhSaoCtb *)bytes(keep, n_ctb * sizeof(OhSaoCtb), k++);
    if (s.cip) f.is_intra = (const uint8_t *)bytes(keep, n_pcm, k++);
    if (s.sparse) {
        f.n_sparse = 37; f.sparse = (const uint32_t *)bytes(keep, 37 * sizeof(uint32_t), k++);
        f.tu_sparse = (const uint32_t *)bytes(keep, s.n_tu * sizeof(uint32_t), k++);
    }
    if (s.scaling) f.scaling = (const OhScalingList *)bytes(keep, sizeof(OhScalingList), k++);
    if (s.cross) f.tu_cross = (const uint32_t *)bytes(keep, s.n_tu * sizeof(uint32_t), k++);
    if (s.pending) f.sao_pending = (const uint8_t *)bytes(keep, n_ctb, k++);

    HostSide h;
    memset(&h, 0, sizeof(h));
    h.cnt.n_pu = s.n_pu; h.cnt.n_mc_luma = 3 * s.n_pu; h.cnt.n_mc_chroma = s.chroma ? 2 * s.n_pu : 0; h.cnt.n_tu = s.n_tu;
    h.cnt.n_intra = s.n_intra; h.cnt.n_sub = f.n_sub; h.cnt.n_ictu = f.n_ictu;
    h.tu_cnt[0] = s.n_tu; h.n_cross = s.cross ? s.n_tu / 2 : 0; h.any_dense = s.n_tu && !s.all_sparse;
    h.pu_off = (const uint32_t *)bytes(keep, 2 * ((size_t)s.n_pu + 1) * sizeof(uint32_t), k++);

    HandoverHeader H;
    memset(&H, 0, sizeof(H));
    const HandoverLayout L = handover_layout(&f, h, &H.d);
    char *arena = (char *)aligned_alloc(256, align_up(L.total, 256));
    handover_bind(L, arena, &H);

    /* offsets: multiples of 256, rising, no two segments overlap, everything inside total */
    CHECK(L.ns == HL_N_SEGS && L.seg[0].off == 0, "%d segments", L.ns);
    for (int i = 0; i < L.ns; i++) {
        const HandoverSeg &g = L.seg[i];
        const size_t next = i + 1 < L.ns ? L.seg[i + 1].off : L.res_off;
        CHECK(g.off % 256 == 0, "segment %d at %zu", i, g.off);
        CHECK(g.off + (g.bytes ? g.bytes : 1) <= next, "segment %d [%zu, +%zu) reaches into the next at %zu", i, g.off, g.bytes, next);
        /* copied segments lie below copy_bytes; only the coefficient pool of a list without dense blocks is left out */
        if (g.src && g.bytes && !L.copied(g))
            CHECK(g.field == HL_FIELD(d.coeffs) && !h.any_dense && L.copy_bytes == g.off, "segment %d is not copied", i);
    }
    CHECK(L.copy_bytes <= L.zero_off, "copied range %zu reaches the cleared one at %zu", L.copy_bytes, L.zero_off);
    if (s.all_sparse && s.n_coeff) CHECK((char *)H.d.coeffs - arena == (long)L.copy_bytes, "the pool of an all-sparse list is copied");
    /* the cleared range: cursor, summary, ctu_seen, tu_keep and nothing else; prep_clear stores 16 bytes at a time */
    const size_t zfields[4] = { HL_FIELD(d.tu_cursor), HL_FIELD(d.summary), HL_FIELD(d.ctu_seen), HL_FIELD(d.tu_keep) };
    int n_in_zero = 0;
    for (int i = 0; i < L.ns; i++) {
        const bool inside = L.seg[i].off >= L.zero_off && L.seg[i].off < L.zero_off + L.zero_bytes;
        if (inside) {
            CHECK(n_in_zero < 4 && L.seg[i].field == zfields[n_in_zero] && !L.seg[i].src, "segment %d lies in the cleared range", i);
            CHECK(L.seg[i].off + L.seg[i].bytes <= L.zero_off + L.zero_bytes, "segment %d leaves the cleared range", i);
            n_in_zero++;
        }
    }
    CHECK(n_in_zero == 4 && L.zero_bytes % 16 == 0, "%d segments in %zu cleared bytes", n_in_zero, L.zero_bytes);
    CHECK((char *)H.d.zero_ptr == arena + L.zero_off && (size_t)H.d.zero_words * 4 == L.zero_bytes && (char *)H.d.tu_cursor == arena + L.zero_off, "zero_ptr");
    /* the tail: residual pool, then the stale buffer under its configuration only */
    const size_t res_bytes = (size_t)(s.n_coeff ? s.n_coeff : 1) * sizeof(int16_t);
    const bool stale = s.deblock && s.sao && s.log2_ctb == 4 && (s.chroma == 1 || s.chroma == 2);
    CHECK((char *)H.d.res == arena + L.res_off && L.res_off % 256 == 0 && L.res_off + res_bytes <= (stale ? L.stale_off : L.total), "residual pool");
    CHECK(stale == (L.stale_bytes != 0) && stale == (H.d.sao_stale != nullptr), "stale buffer: %zu bytes", L.stale_bytes);
    if (stale)
        CHECK((char *)H.d.sao_stale == arena + L.stale_off && L.stale_off % 256 == 0 && L.stale_bytes >= oh_sao_stale_index(&p, 3, 0, 0) * sizeof(uint16_t) &&
              L.stale_off + L.stale_bytes <= L.total, "stale buffer at %zu", L.stale_off);

    /* header pointers: null exactly when the data is absent, for the fields the kernels test; never null otherwise */
    const bool pend = s.sao && s.pending && s.log2_ctb == 4 && (s.chroma == 1 || s.chroma == 2);
    const struct { const char *name; const void *ptr; bool want; } opt[] = {
        { "tu_sparse", H.d.tu_sparse, s.sparse }, { "tu_cross", H.d.tu_cross, s.cross }, { "sparse", H.d.sparse, s.sparse },
        { "scaling", H.d.scaling, s.scaling }, { "is_intra", H.d.is_intra, s.cip }, { "is_pcm", H.d.is_pcm, s.pcm },
        { "sao", H.d.sao, s.sao }, { "sao_pending", H.d.sao_pending, pend }, { "bs_in maps", H.mvf, s.deblock && s.bs_in },
    };
    for (const auto &o : opt) CHECK((o.ptr != nullptr) == o.want, "%s is %s", o.name, o.ptr ? "set" : "null");
    CHECK(!H.mvf == !H.cbf_luma && !H.mvf == !H.call_log2 && !H.mvf == !H.ctb_flags, "bs_in maps");
    const void *const always[] = { H.d.pu, H.d.mc_luma, H.d.mc_chroma, H.d.wp, H.d.tu, H.d.coeffs, H.d.cross, H.d.res, H.d.intra, H.d.ictu, H.d.sub_start,
        H.d.sub_small, H.d.lvl_start, H.d.vbs, H.d.hbs, H.d.qp, H.d.db, H.d.tu_raw, H.d.intra_raw, H.d.ictu_raw, H.d.pu_off, H.d.tu_keep, H.d.tu_cursor,
        H.d.intra_perm, H.d.ctu_seen, H.d.ctu_aux, H.d.ctu_wait, H.d.ctu_done, H.d.ctu_lvl, H.d.ctu_order, H.d.summary };      /* sub_small_w, zero_ptr: aliases, above and below */
    for (size_t i = 0; i < sizeof(always) / sizeof(*always); i++) {
        const char *q = (const char *)always[i];
        CHECK(q && q >= arena && q < arena + L.total && (q - arena) % 256 == 0, "pointer %zu of the header", i);
        for (size_t j = 0; j < i; j++)
            CHECK(always[j] != always[i], "pointers %zu and %zu of the header address the same segment", j, i);
    }
    CHECK((const void *)H.d.sub_small_w == (const void *)H.d.sub_small, "sub_small_w");

    /* the staging copy: every byte of every copied segment written exactly once, nothing else; contents as the source's, packed
     * grids as the per-entry model "entry i in bits 2 (i & 3) of byte i >> 2" */
    char *stage = (char *)malloc(L.copy_bytes);
    std::vector<uint8_t> written(L.copy_bytes, 0), expect(L.copy_bytes, 0);
    std::vector<CopyJob> jobs;
    handover_copy_jobs(L, stage, jobs);
    for (const CopyJob &j : jobs) {
        const size_t out = j.pack ? (j.n + 3) / 4 : j.n;
        CHECK(j.n && j.n <= (j.pack ? 4u : 1u) * 128 * 1024 && j.dst >= stage && j.dst + out <= stage + L.copy_bytes, "job of %zu bytes", j.n);
        if (j.dst < stage || j.dst + out > stage + L.copy_bytes)
            continue;
        for (size_t i = 0; i < out; i++) written[(size_t)(j.dst - stage) + i]++;
        if (j.pack) pack_bs((uint8_t *)j.dst, (const uint8_t *)j.src, j.n);
        else memcpy(j.dst, j.src, j.n);
    }
    int n_packed = 0;
    for (int i = 0; i < L.ns; i++) {
        const HandoverSeg &g = L.seg[i];
        if (!L.copied(g))
            continue;
        for (size_t b = 0; b < g.bytes; b++) expect[g.off + b] = 1;
        if (!g.pack_n) {
            CHECK(memcmp(stage + g.off, g.src, g.bytes) == 0, "segment %d differs from its source", i);
            continue;
        }
        n_packed++;
        CHECK(g.bytes == (g.pack_n + 3) / 4, "segment %d: %zu strengths in %zu bytes", i, g.pack_n, g.bytes);
        std::vector<uint8_t> model(g.bytes, 0);
        for (size_t e = 0; e < g.pack_n; e++) model[e >> 2] |= (uint8_t)((((const uint8_t *)g.src)[e] & 3) << (2 * (e & 3)));
        CHECK(memcmp(stage + g.off, model.data(), g.bytes) == 0, "segment %d: packed grid differs from the per-entry model", i);
    }
    CHECK(n_packed == (s.deblock && !s.bs_in && !s.bs_packed_in ? 2 : 0) && L.packs == (n_packed != 0), "%d packed grids", n_packed);
    CHECK(written == expect, "the jobs do not write every copied byte exactly once");
    free(stage);
    free(arena);
}

int main()
{
    /*                name           w    h  chr ctb  deblk  sao    bs_in  scal   sparse cross  cip    pcm    pend   allsp  packed  pu  tu intra coeff  bs_size */
    const Spec lists[] = {
        { "empty",            64,  64, 1, 6, false, false, false, false, false, false, false, false, false, false, false,  0,  0,  0,    0, 0 },
        { "everything",       72,  40, 2, 4, true,  true,  true,  true,  true,  true,  true,  true,  true,  false, false, 21, 33, 17, 1029, -1 },
        { "everything_grids", 72,  40, 2, 4, true,  true,  false, true,  true,  true,  true,  true,  true,  false, false, 21, 33, 17, 1029, -1 },
        { "mono",            128,  64, 0, 6, true,  true,  false, false, false, false, false, false, false, false, false,  5, 11,  9,  300, -1 },
        { "all_sparse",      136,  88, 1, 5, true,  false, false, true,  true,  false, false, false, false, true,  true,   7, 19,  0,  500, -1 },
        { "grid_1",           64,  64, 1, 6, true,  false, false, false, false, false, false, false, false, false, false,  1,  1,  0,   16, 1 },
        { "grid_2",           64,  64, 1, 6, true,  false, false, false, false, false, false, false, false, false, false,  1,  1,  0,   16, 2 },
        { "grid_3",           64,  64, 1, 6, true,  false, false, false, false, false, false, false, false, false, false,  1,  1,  0,   16, 3 },
        { "grid_4",           64,  64, 1, 6, true,  false, false, false, false, false, false, false, false, false, false,  1,  1,  0,   16, 4 },
        { "grid_5",           64,  64, 1, 6, true,  false, false, false, false, false, false, false, false, false, false,  1,  1,  0,   16, 5 },
        { "grid_4x128k_1",    64,  64, 1, 6, true,  true,  false, false, false, false, false, false, false, false, false,  1,  1,  0,   16, 4 * 128 * 1024 + 1 },
    };
    for (const Spec &s : lists) run(s);
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    else printf("handover layout: %zu lists ok\n", sizeof(lists) / sizeof(*lists));
    return failures ? 1 : 0;
}
