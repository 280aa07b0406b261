/* handover_parallel_check.cpp — the host work of the hand-over that several threads share (openhevc_amd/csrc/handover_host.h:
 * handover_check_list, handover_check_chunk, CopyPool) and the vectorised pack_bs (handover_layout.h), run on the CPU as a stand-alone
 * program; tests/test_handover_parallel_host.py builds it once with AddressSanitizer + UBSan and once with ThreadSanitizer.
 *   1. chunks of 1, 2, 3, 5 and 32 small random lists, checked and counted through a pool of 0, 1, 2 and 5 helpers: every HostSide,
 *      every PU offset array and every error slot equals what a plain loop over the same lists gives;
 *   2. chunks of 32 with bad lists at indices 3 and 17: list 3 is the one reported, 200 times over;
 *   3. the staging copy of a group with its pieces claimed: every job runs once, no two jobs share a byte, every copied byte is
 *      covered, and the staged bytes equal those of the copy dealt by stride;
 *   4. pack_bs against the per-entry model: every length 0..70, lengths around the multiples of 16 and 32, up to 4 x 128 KB + 3, at
 *      all 16 source misalignments; sources and destinations have exactly their bytes, so a step too far is a sanitizer report.
 * Exit status 0: everything held. */
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "../openhevc_amd/csrc/handover_host.h"

static int failures;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            failures++;                                                                    \
            fprintf(stderr, "%s (line %d): ", #cond, __LINE__);                            \
            fprintf(stderr, __VA_ARGS__);                                                  \
            fprintf(stderr, "\n");                                                         \
        }                                                                                  \
    } while (0)

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
    uint32_t below(uint32_t n) { return next() % n; }
};

enum Bad { GOOD, BAD_WEIGHTS, BAD_LEVELS, BAD_NULL };

/* one small list with everything its arrays point at; 64x64 8-bit 4:2:0, byte grids (packed on the way) when it deblocks */
struct List {
    OhFrame f;
    std::vector<OhPu> pu;
    std::vector<OhTu> tu;
    std::vector<OhWeights> wp;
    std::vector<OhIntra> intra;
    std::vector<OhIntraCtu> ictu;
    std::vector<uint32_t> sub_start, level_start, sparse, tu_sparse;
    std::vector<int16_t> coeffs;
    std::vector<uint8_t> vbs, hbs;
    std::vector<int8_t> qp;
    std::vector<OhDeblockCtb> db;
    List(unsigned seed, Bad bad)
    {
        Rng g(seed);
        memset(&f, 0, sizeof(f));
        OhPicParams &p = f.p;
        p.width = 64; p.height = 64; p.bit_depth = 8; p.chroma_format_idc = 1; p.log2_ctb_size = 4;
        p.log2_min_cb_size = 3; p.log2_min_tb_size = 2; p.log2_min_pu_size = 2;
        const unsigned shape = seed % 6;                      /* 0: no PUs, 1: no TUs, 2: all sparse, 3: one dense block, 4 / 5: mixed */
        const uint32_t n_pu = shape == 0 ? 0 : 100 + g.below(300), n_tu = shape == 1 ? 0 : 100 + g.below(300);
        pu.resize(n_pu);
        for (OhPu &u : pu) {
            memset(&u, 0, sizeof(u));
            u.x = (uint16_t)(4 * g.below(16)); u.y = (uint16_t)(4 * g.below(16));
            u.w = (uint8_t)(4 + 4 * g.below(16)); u.h = (uint8_t)(4 + 4 * g.below(16));
            u.ref[0] = g.below(4) ? (uint8_t)g.below(OH_MAX_REFS) : (uint8_t)OH_NO_REF;
            u.ref[1] = g.below(2) ? (uint8_t)g.below(OH_MAX_REFS) : (uint8_t)OH_NO_REF;
            u.wp = OH_NO_WP;
        }
        tu.resize(n_tu);
        const uint32_t dense_at = shape == 3 ? g.below(n_tu ? n_tu : 1) : ~0u;
        uint32_t n_coeff = 0;
        for (uint32_t i = 0; i < n_tu; i++) {
            OhTu &t = tu[i];
            memset(&t, 0, sizeof(t));
            t.log2_size = (uint8_t)(2 + g.below(4));
            t.c_idx = (uint8_t)g.below(3);
            const bool dense = shape == 2 ? false : shape == 3 ? i == dense_at : g.below(3) == 0;
            t.flags = (uint8_t)((dense ? 0 : OH_TUF_SPARSE) | (g.below(2) ? OH_TUF_ADD_NOW : 0));
            t.coeff_off = n_coeff;
            if (dense) n_coeff += 1u << (2 * t.log2_size);
        }
        coeffs.assign(n_coeff, 7);
        sparse.assign(37, 0); tu_sparse.assign(n_tu, 0);
        wp.resize(seed % 3);
        for (OhWeights &w : wp) { memset(&w, 0, sizeof(w)); w.log2_denom[0] = (uint8_t)g.below(8); w.log2_denom[1] = (uint8_t)g.below(8); }
        if (seed % 4 == 1 || bad == BAD_LEVELS) {             /* intra tables: 6 schedule entries in 3 levels */
            intra.resize(9); memset(intra.data(), 0, intra.size() * sizeof(OhIntra));
            ictu.resize(6); memset(ictu.data(), 0, ictu.size() * sizeof(OhIntraCtu));
            sub_start = { 0, 2, 3, 5, 6, 8, 9 };
            level_start = { 0, 1, 3, 6 };
            if (bad == BAD_LEVELS) level_start = { 0, 4, 3, 6 };
        }
        if (bad == BAD_WEIGHTS) {
            wp.resize(3); memset(wp.data(), 0, 3 * sizeof(OhWeights));
            wp[2].log2_denom[1] = 8;
        }
        if (seed % 5 == 2) {                                  /* deblocks: byte grids, four strengths packed into a byte on the way */
            p.deblock_enabled = 1;
            f.bs_size = oh_bs_size(&p);
            vbs.resize(f.bs_size); hbs.resize(f.bs_size);
            for (uint8_t &b : vbs) b = (uint8_t)g.below(3);
            for (uint8_t &b : hbs) b = (uint8_t)g.below(3);
            qp.assign(oh_qp_tab_size(&p), 30);
            db.resize((size_t)oh_ctb_width(&p) * oh_ctb_height(&p)); memset(db.data(), 0, db.size() * sizeof(OhDeblockCtb));
            f.vertical_bs = vbs.data(); f.horizontal_bs = hbs.data(); f.qp_y_tab = qp.data(); f.deblock = db.data();
        }
        auto ptr = [](auto &v) { return v.empty() ? nullptr : v.data(); };
        f.n_pu = n_pu; f.pu = ptr(pu);
        f.n_tu = n_tu; f.tu = ptr(tu);
        f.n_wp = (uint32_t)wp.size(); f.wp = ptr(wp);
        f.n_coeff = n_coeff; f.coeffs = ptr(coeffs);
        f.n_sparse = (uint32_t)sparse.size(); f.sparse = sparse.data(); f.tu_sparse = ptr(tu_sparse);
        f.n_intra = (uint32_t)intra.size(); f.intra = ptr(intra);
        if (!intra.empty()) {
            f.n_ictu = (uint32_t)ictu.size(); f.ictu = ictu.data();
            f.n_sub = (uint32_t)sub_start.size() - 1; f.sub_start = sub_start.data();
            f.n_levels = (uint32_t)level_start.size() - 1; f.level_start = level_start.data();
        }
        if (bad == BAD_NULL) {                                /* a NULL array with a non-zero count */
            if (f.n_pu) f.pu = nullptr;
            else f.tu = nullptr;
        }
    }
};

struct Chunk {
    std::vector<std::unique_ptr<List>> lists;
    std::vector<const OhFrame *> fs;
    std::vector<uint32_t> ref_ok;
    void add(unsigned seed, Bad bad)
    {
        lists.emplace_back(new List(seed, bad));
        fs.push_back(&lists.back()->f);
        ref_ok.push_back(seed * 2654435761u & 0xffffu);
    }
    int n() const { return (int)fs.size(); }
};

/* what the check-and-count phase of a chunk leaves */
struct Result {
    std::vector<HostSide> h;
    std::vector<std::vector<uint32_t>> pu_off;
    std::vector<HandoverCheck> chk;
    int bad;
    explicit Result(int n) : h((size_t)n), pu_off((size_t)n), chk((size_t)n), bad(-1)
    {
        memset(h.data(), 0, h.size() * sizeof(HostSide));
        memset(chk.data(), 0, chk.size() * sizeof(HandoverCheck));
    }
};

static void serial(const Chunk &c, Result *r)
{
    r->bad = -1;
    for (int i = 0; i < c.n(); i++)
        if (handover_check_list(c.fs[i], c.ref_ok[i], &r->h[i], r->pu_off[i], &r->chk[i]) != OH_OK && r->bad < 0)
            r->bad = i;
}

static void same_results(const Chunk &c, const Result &a, const Result &b, const char *tag)
{
    CHECK(a.bad == b.bad, "%s: list %d reported, the loop in order reports %d", tag, b.bad, a.bad);
    for (int i = 0; i < c.n(); i++) {
        const HostSide &x = a.h[i], &y = b.h[i];
        CHECK(a.chk[i].rc == b.chk[i].rc && strcmp(a.chk[i].msg, b.chk[i].msg) == 0, "%s: list %d: error slot (%d, '%s') against (%d, '%s')",
              tag, i, b.chk[i].rc, b.chk[i].msg, a.chk[i].rc, a.chk[i].msg);
        CHECK(memcmp(&x.cnt, &y.cnt, sizeof(x.cnt)) == 0 && memcmp(x.tu_cnt, y.tu_cnt, sizeof(x.tu_cnt)) == 0 && x.n_cross == y.n_cross &&
              x.any_dense == y.any_dense && x.ref_used == y.ref_used && x.ref_ok == y.ref_ok, "%s: list %d: HostSide differs", tag, i);
        if (a.chk[i].rc != OH_OK || b.chk[i].rc != OH_OK)
            continue;
        CHECK(y.pu_off == b.pu_off[i].data() && a.pu_off[i] == b.pu_off[i], "%s: list %d: PU block offsets differ", tag, i);
        CHECK(a.pu_off[i].size() == 2 * ((size_t)c.fs[i]->n_pu + 1), "%s: list %d: %zu offsets", tag, i, a.pu_off[i].size());
    }
}

static const int HELPERS[] = { 0, 1, 2, 5 };

static int check_good_chunks()
{
    int chunks = 0;
    for (int helpers : HELPERS) {
        CopyPool pool;
        pool.start(helpers);
        for (int n : { 1, 2, 3, 5, 32 })
            for (unsigned round = 0; round < 3; round++) {
                Chunk c;
                for (int i = 0; i < n; i++) c.add(1000u * round + 37u * (unsigned)n + (unsigned)i, GOOD);
                Result want(n), got(n);
                serial(c, &want);
                CHECK(want.bad == -1, "a list meant to be well-formed is refused: %s", want.chk[want.bad < 0 ? 0 : want.bad].msg);
                got.bad = handover_check_chunk(&pool, c.fs.data(), c.ref_ok.data(), n, got.h.data(), got.pu_off.data(), got.chk.data());
                const std::string tag = std::to_string(n) + " lists, " + std::to_string(helpers) + " helpers";
                same_results(c, want, got, tag.c_str());
                chunks++;
            }
    }
    return chunks;
}

static void check_bad_chunks()
{
    static const Bad kinds[3] = { BAD_WEIGHTS, BAD_LEVELS, BAD_NULL };
    static const char *const msgs[3] = { "log2 denominator out of range", "intra level table not monotonic", "NULL array" };
    std::unique_ptr<CopyPool> pools[4];
    for (int k = 0; k < 4; k++) { pools[k].reset(new CopyPool()); pools[k]->start(HELPERS[k]); }
    /* the nine pairs of kinds at (3, 17), made once */
    std::vector<std::unique_ptr<Chunk>> chunks;
    std::vector<std::unique_ptr<Result>> wants;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            chunks.emplace_back(new Chunk());
            for (int i = 0; i < 32; i++) chunks.back()->add(5000u + (unsigned)(a * 3 + b) * 64u + (unsigned)i, i == 3 ? kinds[a] : i == 17 ? kinds[b] : GOOD);
            wants.emplace_back(new Result(32));
            serial(*chunks.back(), wants.back().get());
            const Result &w = *wants.back();
            CHECK(w.bad == 3 && w.chk[3].rc == OH_E_ARG && strstr(w.chk[3].msg, msgs[a]), "list 3 of kind %d: (%d, '%s')", a, w.chk[3].rc, w.chk[3].msg);
            CHECK(w.chk[17].rc == OH_E_ARG && strstr(w.chk[17].msg, msgs[b]), "list 17 of kind %d: (%d, '%s')", b, w.chk[17].rc, w.chk[17].msg);
        }
    for (int rep = 0; rep < 200; rep++) {
        const Chunk &c = *chunks[(size_t)rep % chunks.size()];
        Result got(32);
        got.bad = handover_check_chunk(pools[rep % 4].get(), c.fs.data(), c.ref_ok.data(), 32, got.h.data(), got.pu_off.data(), got.chk.data());
        CHECK(got.bad == 3, "repetition %d (%d helpers): list %d reported", rep, HELPERS[rep % 4], got.bad);
        same_results(c, *wants[(size_t)rep % chunks.size()], got, "bad lists at 3 and 17");
    }
}

static void run_jobs_strided(const std::vector<CopyJob> &jobs, int shares)
{
    for (int s = 0; s < shares; s++)
        for (size_t i = (size_t)s; i < jobs.size(); i += (size_t)shares)
            CopyPool::copy_one(jobs[i]);
}

static void check_claimed_copy()
{
    for (int helpers : HELPERS) {
        CopyPool pool;
        pool.start(helpers);
        for (int n : { 1, 5, 32 }) {
            Chunk c;
            for (int i = 0; i < n; i++) c.add(9000u + (unsigned)n * 40u + (unsigned)i, GOOD);
            Result r(n);
            serial(c, &r);
            std::vector<HandoverHeader> H((size_t)n);
            std::vector<HandoverLayout> L;
            for (int i = 0; i < n; i++) {
                memset(&H[i], 0, sizeof(HandoverHeader));
                for (size_t b = 0; b < sizeof(DevFrame); b++) ((uint8_t *)&H[i].d)[b] = (uint8_t)(b + (size_t)i);
                L.push_back(handover_layout(c.fs[i], r.h[i], &H[i].d));
            }
            const HandoverChunk C = handover_chunk_place(L.data(), n);
            std::vector<char> claimed(C.copy_bytes, (char)0xA5), strided(C.copy_bytes, (char)0xA5);
            std::vector<CopyJob> ja, jb;
            for (int i = 0; i < n; i++) {
                handover_copy_jobs_add(L[i], claimed.data() + C.copied_off[i], ja);
                handover_copy_jobs_add(L[i], strided.data() + C.copied_off[i], jb);
            }
            /* no two jobs share a staged byte, and the jobs cover every copied byte */
            std::vector<uint8_t> covered(C.copy_bytes, 0), expect(C.copy_bytes, 0);
            for (const CopyJob &j : ja) {
                const size_t at = (size_t)(j.dst - claimed.data()), out = j.pack ? (j.n + 3) / 4 : j.n;
                CHECK(at + out <= C.copy_bytes && j.n <= (j.pack ? 4u : 1u) * 128 * 1024, "a job of %zu bytes at %zu", j.n, at);
                for (size_t b = 0; b < out && at + b < C.copy_bytes; b++) covered[at + b]++;
            }
            for (int i = 0; i < n; i++)
                for (int s = 0; s < L[i].ns; s++)
                    if (L[i].copied(L[i].seg[s]))
                        for (size_t b = 0; b < L[i].seg[s].bytes; b++) expect[C.copied_off[i] + L[i].seg[s].off + b] = 1;
            CHECK(covered == expect, "%d lists: the jobs do not cover every copied byte exactly once", n);
            /* every job is claimed by exactly one thread */
            std::vector<std::atomic<int>> taken(ja.size());
            for (auto &t : taken) t.store(0);
            const CopyJob *jp = ja.data();
            pool.run(ja.size(), [&taken, jp](size_t i) { taken[i].fetch_add(1); CopyPool::copy_one(jp[i]); });
            for (size_t i = 0; i < ja.size(); i++)
                CHECK(taken[i].load() == 1, "%d lists, %d helpers: job %zu ran %d times", n, helpers, i, taken[i].load());
            run_jobs_strided(jb, 3);
            CHECK(claimed == strided, "%d lists, %d helpers: the claimed copy stages other bytes than the copy dealt by stride", n, helpers);
            /* the entry point the engine uses */
            std::fill(claimed.begin(), claimed.end(), (char)0xA5);
            pool.run(ja);
            CHECK(claimed == strided, "%d lists, %d helpers: CopyPool::run(jobs) stages other bytes", n, helpers);
        }
    }
}

static int check_pack_bs()
{
    std::vector<size_t> lengths;
    for (size_t n = 0; n <= 70; n++) lengths.push_back(n);
    for (size_t m = 80; m <= 1024; m += 16)
        for (size_t n = m - 1; n <= m + 1; n++) lengths.push_back(n);
    for (size_t m = 2048; m <= 4 * 128 * 1024; m *= 2)
        for (size_t n = m - 3; n <= m + 3; n++) lengths.push_back(n);
    int cases = 0;
    Rng g(77);
    for (size_t n : lengths)
        for (size_t mis = 0; mis < 16; mis++) {
            /* 32-byte aligned block, the source `mis` bytes in and ending with the block; the destination has exactly its bytes */
            uint8_t *block = (uint8_t *)aligned_alloc(32, (mis + n + 31) / 32 * 32 + 32);
            uint8_t *src = block + ((mis + n + 31) / 32 * 32 + 32) - n;
            src -= ((uintptr_t)src - mis) & 15;               /* src % 16 == mis */
            uint8_t *buf = (uint8_t *)malloc(n ? n : 1);      /* the copy the packer reads: exactly n bytes, any alignment of its own */
            for (size_t i = 0; i < n; i++) src[i] = (uint8_t)(g.below(3) | (i % 7 == 3 ? 0xfc : 0));     /* model: only the low two bits count */
            memcpy(buf, src, n);
            const size_t out = (n + 3) / 4;
            uint8_t *got = (uint8_t *)malloc(out ? out : 1), *got2 = (uint8_t *)malloc(out ? out : 1);
            std::vector<uint8_t> want(out ? out : 1, 0);
            for (size_t i = 0; i < n; i++) want[i >> 2] |= (uint8_t)((src[i] & 3) << ((i & 3) * 2));
            pack_bs(got, src, n);
            pack_bs(got2, buf, n);
            CHECK(memcmp(got, want.data(), out) == 0 && memcmp(got2, want.data(), out) == 0, "pack_bs of %zu entries at misalignment %zu differs from the per-entry model", n, mis);
            free(got); free(got2); free(buf); free(block);
            cases++;
        }
    return cases;
}

int main()
{
    const int chunks = check_good_chunks();
    check_bad_chunks();
    check_claimed_copy();
    const int packs = check_pack_bs();
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    else printf("handover parallel: %d chunks, 200 refused chunks, claimed copies and %d packings ok\n", chunks, packs);
    return failures ? 1 : 0;
}
