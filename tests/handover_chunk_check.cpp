/* handover_chunk_check.cpp — the arena of a chunk of work lists (openhevc_amd/csrc/handover_layout.h: handover_chunk_place,
 * handover_bind_split, handover_copy_jobs_add) run on the CPU over small host arrays; built with AddressSanitizer and UBSan by
 * tests/test_handover_chunk_host.py.  Chunks of 1, 2, 9 and 32 lists of mixed kinds.  Every staging block has exactly the bytes of
 * its group and every source array exactly the bytes its layout may read, so a job one byte out of place is a sanitizer report.
 * Exit status 0: every check of every chunk held. */
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <string>
#include <vector>

#include "../openhevc_amd/csrc/handover_layout.h"

static int failures;
static std::string chunk_name;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            failures++;                                                                    \
            fprintf(stderr, "%s: %s (line %d): ", chunk_name.c_str(), #cond, __LINE__);     \
            fprintf(stderr, __VA_ARGS__);                                                  \
            fprintf(stderr, "\n");                                                         \
        }                                                                                  \
    } while (0)

enum Kind { EMPTY, ALL_SPARSE, DENSE, BS_IN, BYTE_GRIDS, INTRA_TABLES, DENSE_NO_INTRA, N_KINDS };
static const char *const kind_name[N_KINDS] = { "empty", "all_sparse", "dense", "bs_in", "byte_grids", "intra_tables", "dense_no_intra" };

/* one list with everything its arrays point at; the arrays have exactly the bytes the layout may read */
struct List {
    OhFrame f;
    OhBsInputs bi;
    HostSide h;
    HandoverHeader H;
    HandoverLayout L;
    std::vector<std::vector<uint8_t>> keep;
    void *bytes(size_t n, unsigned seed)
    {
        keep.emplace_back(n);
        for (size_t i = 0; i < n; i++) keep.back()[i] = (uint8_t)((i * 7 + seed * 13 + (i >> 8)) & 0xff);
        return n ? keep.back().data() : nullptr;
    }
    List(Kind kind, unsigned seed)
    {
        memset(&f, 0, sizeof(f)); memset(&bi, 0, sizeof(bi)); memset(&h, 0, sizeof(h)); memset(&H, 0, sizeof(H));
        OhPicParams &p = f.p;
        const bool small = seed & 1;                          /* two geometries in one chunk */
        p.width = small ? 64 : 136; p.height = small ? 64 : 88; p.bit_depth = 8; p.chroma_format_idc = 1; p.log2_ctb_size = small ? 6 : 4;
        p.log2_min_cb_size = 3; p.log2_min_tb_size = 2; p.log2_min_pu_size = 2;
        const bool deblock = kind != EMPTY, sao = kind == DENSE || kind == INTRA_TABLES;
        p.deblock_enabled = deblock; p.sao_enabled = sao;
        const size_t n_ctb = (size_t)oh_ctb_width(&p) * oh_ctb_height(&p), n_pcm = (size_t)oh_min_pu_width(&p) * oh_min_pu_height(&p);
        const size_t n_mtb = (size_t)(p.width >> 2) * (p.height >> 2);
        const uint32_t n_pu = kind == EMPTY ? 0 : 5 + seed % 7, n_tu = kind == EMPTY ? 0 : 11 + seed % 5;
        const uint32_t n_intra = kind == INTRA_TABLES || kind == DENSE ? 9 : 0, n_coeff = kind == EMPTY ? 0 : 300 + 16 * (seed % 9);
        unsigned k = seed * 31;
        f.n_pu = n_pu; f.pu = (const OhPu *)bytes(n_pu * sizeof(OhPu), k++);
        f.n_tu = n_tu; f.tu = (const OhTu *)bytes(n_tu * sizeof(OhTu), k++);
        f.n_coeff = n_coeff; f.coeffs = (const int16_t *)bytes(n_coeff * sizeof(int16_t), k++);
        f.n_intra = n_intra; f.intra = (const OhIntra *)bytes(n_intra * sizeof(OhIntra), k++);
        if (n_intra) {
            f.n_ictu = 3; f.ictu = (const OhIntraCtu *)bytes(3 * sizeof(OhIntraCtu), k++);
            f.n_sub = 5; f.sub_start = (const uint32_t *)bytes(6 * sizeof(uint32_t), k++);
            f.n_levels = 2; f.level_start = (const uint32_t *)bytes(3 * sizeof(uint32_t), k++);
        }
        f.bs_size = oh_bs_size(&p);
        if (deblock) {
            if (kind == BS_IN) {
                bi.mvf = (const OhMvField *)bytes(n_pcm * sizeof(OhMvField), k++);
                bi.cbf_luma = (const uint8_t *)bytes(n_mtb, k++);
                bi.call_log2 = (const uint8_t *)bytes(n_mtb, k++);
                bi.ctb_flags = (const uint8_t *)bytes(n_ctb, k++);
                f.bs_in = &bi;
            } else {
                const bool packed_in = kind != BYTE_GRIDS && kind != DENSE;       /* byte grids are packed on the way */
                const size_t n = packed_in ? (f.bs_size + 3) / 4 : f.bs_size;
                f.vertical_bs = (const uint8_t *)bytes(n, k++);
                f.horizontal_bs = (const uint8_t *)bytes(n, k++);
                if (packed_in) f.flags |= OH_FRAME_BS_PACKED;
            }
            f.qp_y_tab = (const int8_t *)bytes(oh_qp_tab_size(&p), k++);
            f.deblock = (const OhDeblockCtb *)bytes(n_ctb * sizeof(OhDeblockCtb), k++);
        }
        if (sao) f.sao = (const OhSaoCtb *)bytes(n_ctb * sizeof(OhSaoCtb), k++);
        if (kind == ALL_SPARSE || kind == INTRA_TABLES) {
            f.n_sparse = 37; f.sparse = (const uint32_t *)bytes(37 * sizeof(uint32_t), k++);
            f.tu_sparse = (const uint32_t *)bytes(n_tu * sizeof(uint32_t), k++);
        }
        h.cnt.n_pu = n_pu; h.cnt.n_mc_luma = 3 * n_pu; h.cnt.n_mc_chroma = 2 * n_pu; h.cnt.n_tu = n_tu;
        h.cnt.n_intra = n_intra; h.cnt.n_sub = f.n_sub; h.cnt.n_ictu = f.n_ictu;
        h.tu_cnt[0] = n_tu; h.any_dense = n_tu && kind != ALL_SPARSE;
        h.pu_off = (const uint32_t *)bytes(2 * ((size_t)n_pu + 1) * sizeof(uint32_t), k++);
        for (size_t i = 0; i < sizeof(DevFrame); i++) ((uint8_t *)&H.d)[i] = (uint8_t)(i + seed);      /* the header is staged from here */
        L = handover_layout(&f, h, &H.d);
    }
};

struct Range { size_t lo, hi; const char *what; int list; };

static void run(int n, int group)
{
    chunk_name = "chunk of " + std::to_string(n) + ", groups of " + std::to_string(group);
    std::vector<std::unique_ptr<List>> lists;
    std::vector<HandoverLayout> L;
    for (int i = 0; i < n; i++) {
        lists.emplace_back(new List((Kind)((i * 3 + n) % N_KINDS), (unsigned)(i + 1)));
        L.push_back(lists.back()->L);
    }
    const HandoverChunk C = handover_chunk_place(L.data(), n);
    CHECK(C.n == n, "%d lists", C.n);

    /* the copied parts tile [0, copy_bytes) exactly once and in order */
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        CHECK(C.copied_off[i] == at && at % 256 == 0, "copied part of list %d at %zu, expected %zu", i, C.copied_off[i], at);
        CHECK(L[i].copy_bytes % 256 == 0 && L[i].copy_bytes >= sizeof(DevFrame), "list %d copies %zu bytes", i, L[i].copy_bytes);
        at += L[i].copy_bytes;
    }
    CHECK(C.copy_bytes == at && C.copied_off[n] == at, "copied range ends at %zu, expected %zu", C.copy_bytes, at);
    /* no rest part overlaps another part or the copied range; everything inside total */
    std::vector<Range> parts;
    parts.push_back({ 0, C.copy_bytes, "copied range", -1 });
    for (int i = 0; i < n; i++) {
        CHECK(C.rest_off[i] % 256 == 0 && C.rest_off[i] >= C.copy_bytes, "rest of list %d at %zu", i, C.rest_off[i]);
        parts.push_back({ C.rest_off[i], C.rest_off[i] + (L[i].total - L[i].copy_bytes), "rest", i });
    }
    for (size_t a = 0; a < parts.size(); a++) {
        CHECK(parts[a].hi <= C.total, "%s of list %d ends at %zu beyond the arena's %zu", parts[a].what, parts[a].list, parts[a].hi, C.total);
        for (size_t b = 0; b < a; b++)
            CHECK(parts[a].lo >= parts[b].hi || parts[b].lo >= parts[a].hi, "%s of list %d overlaps %s of list %d", parts[a].what, parts[a].list, parts[b].what, parts[b].list);
    }

    /* every bound pointer equals base + expected offset, or is null by the existing rule (handover_bind's: the same null fields) */
    char *arena = (char *)aligned_alloc(256, C.total ? C.total : 256);
    for (int i = 0; i < n; i++) {
        List &ls = *lists[i];
        char *cb = arena + C.copied_off[i], *rb = arena + C.rest_off[i];
        handover_bind_split(L[i], cb, rb, &ls.H);
        HandoverHeader one;                                   /* the same list alone in an arena of its own at address 0x10000 */
        memcpy(&one, &ls.H, sizeof(one));
        char *const fake = (char *)(uintptr_t)0x10000;
        handover_bind(L[i], fake, &one);
        auto expect = [&](size_t off) { return off < L[i].copy_bytes ? cb + off : rb + (off - L[i].copy_bytes); };
        for (int g = 0; g < L[i].ns; g++) {
            const HandoverSeg &sg = L[i].seg[g];
            if (sg.field == HL_NO_FIELD)
                continue;
            char *got, *alone;
            memcpy(&got, (char *)&ls.H + sg.field, sizeof(got));
            memcpy(&alone, (char *)&one + sg.field, sizeof(alone));
            CHECK(!alone == !got && !got == sg.null_field, "list %d segment %d: null in one binding only", i, g);
            if (got) {
                CHECK(got == expect(sg.off) && alone == fake + sg.off, "list %d segment %d bound %zd bytes from the copied part", i, g, (ptrdiff_t)(got - cb));
                CHECK(sg.off + sg.bytes <= L[i].copy_bytes || sg.off >= L[i].copy_bytes, "list %d segment %d straddles the two parts", i, g);
                CHECK(got >= arena && got + sg.bytes <= arena + C.total, "list %d segment %d leaves the arena", i, g);
            }
        }
        CHECK((char *)ls.H.d.res == expect(L[i].res_off) && (char *)ls.H.d.zero_ptr == expect(L[i].zero_off) &&
              (size_t)ls.H.d.zero_words * 4 == L[i].zero_bytes && (const void *)ls.H.d.sub_small_w == (const void *)ls.H.d.sub_small, "list %d: res / zero_ptr / sub_small_w", i);
        CHECK((ls.H.d.sao_stale != nullptr) == (L[i].stale_bytes != 0) && (!L[i].stale_bytes || (char *)ls.H.d.sao_stale == expect(L[i].stale_off)), "list %d: stale buffer", i);
        CHECK(L[i].zero_off >= L[i].copy_bytes && L[i].zero_off + L[i].zero_bytes <= L[i].total, "list %d: the cleared range lies in the rest", i);
    }
    /* n = 1 reproduces handover_bind's header byte for byte */
    if (n == 1) {
        HandoverHeader a, b;
        memcpy(&a, &lists[0]->H, sizeof(a)); memcpy(&b, &lists[0]->H, sizeof(b));
        handover_bind(L[0], arena, &a);
        handover_bind_split(L[0], arena + C.copied_off[0], arena + C.rest_off[0], &b);
        CHECK(memcmp(&a, &b, sizeof(a)) == 0 && C.total == L[0].total && C.rest_off[0] == L[0].copy_bytes, "a chunk of one is not the list's own arena");
    }

    /* the staging jobs of a group write every copied byte of the group once, and the staged bytes are the sources' */
    for (int g0 = 0; g0 < n; g0 += group) {
        const int g1 = std::min(n, g0 + group);
        const size_t bytes = C.copied_off[g1] - C.copied_off[g0];
        char *stage = (char *)malloc(bytes);
        std::vector<uint8_t> written(bytes, 0), expect(bytes, 0);
        std::vector<CopyJob> jobs;
        for (int i = g0; i < g1; i++)
            handover_copy_jobs_add(L[i], stage + (C.copied_off[i] - C.copied_off[g0]), jobs);
        for (const CopyJob &j : jobs) {
            const size_t out = j.pack ? (j.n + 3) / 4 : j.n;
            CHECK(j.n && j.dst >= stage && j.dst + out <= stage + bytes, "job of %zu bytes", j.n);
            if (j.dst < stage || j.dst + out > stage + bytes)
                continue;
            for (size_t b = 0; b < out; b++) written[(size_t)(j.dst - stage) + b]++;
            if (j.pack) pack_bs((uint8_t *)j.dst, (const uint8_t *)j.src, j.n);
            else memcpy(j.dst, j.src, j.n);
        }
        for (int i = g0; i < g1; i++) {
            const size_t base = C.copied_off[i] - C.copied_off[g0];
            std::vector<CopyJob> alone;
            std::vector<char> st1(L[i].copy_bytes);
            handover_copy_jobs(L[i], st1.data(), alone);    /* the list staged alone: the same bytes at the same offsets */
            for (const CopyJob &j : alone) {
                if (j.pack) pack_bs((uint8_t *)j.dst, (const uint8_t *)j.src, j.n);
                else memcpy(j.dst, j.src, j.n);
            }
            for (int g = 0; g < L[i].ns; g++) {
                const HandoverSeg &sg = L[i].seg[g];
                if (!L[i].copied(sg))
                    continue;
                for (size_t b = 0; b < sg.bytes; b++) expect[base + sg.off + b] = 1;
                CHECK(memcmp(stage + base + sg.off, st1.data() + sg.off, sg.bytes) == 0, "list %d segment %d staged in a group differs from staged alone", i, g);
                if (!sg.pack_n)
                    CHECK(memcmp(stage + base + sg.off, sg.src, sg.bytes) == 0, "list %d segment %d differs from its source", i, g);
            }
            CHECK(memcmp(stage + base, &lists[i]->H.d, sizeof(DevFrame)) == 0, "list %d: the header is not at the start of its copied part", i);
        }
        CHECK(written == expect, "group at %d: the jobs do not write every copied byte exactly once", g0);
        free(stage);
    }
    free(arena);
}

int main()
{
    const int sizes[] = { 1, 2, 9, 32 };
    int chunks = 0;
    for (int n : sizes)
        for (int group : { 1, 8, 32 }) { run(n, group); chunks++; }
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    else printf("handover chunks: %d chunks ok\n", chunks);
    return failures ? 1 : 0;
}
