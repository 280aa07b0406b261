/* intra_plan_check.cpp — the engine's switches (openhevc_amd/csrc/engine_tuning.h) and the launch plan of the intra pass
 * (openhevc_amd/csrc/intra_plan.h) run on the CPU; built with AddressSanitizer and UBSan by tests/test_intra_plan_host.py.
 * Every expected value below is written out by hand from the rules the engine had before the two headers existed: none is computed
 * by the code under test.  Exit status 0: every check held. */
#include <stdio.h>
#include <stdlib.h>
#include <string>

#include "../openhevc_amd/csrc/intra_plan.h"

static int failures;
static std::string what;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            failures++;                                                                    \
            fprintf(stderr, "%s: %s (line %d): ", what.c_str(), #cond, __LINE__);           \
            fprintf(stderr, __VA_ARGS__);                                                  \
            fprintf(stderr, "\n");                                                         \
        }                                                                                  \
    } while (0)

/* ---------------- tuning ---------------- */
enum { T_MODE, T_WAVES, T_PHASES, T_RES_LDS, T_SPIN, T_COPY, T_FETCH, T_STAMPS, T_TIMING, T_N };
static const char *const VARS[T_N] = { "OHEVC_INTRA_MODE", "OHEVC_INTRA_WAVES", "OHEVC_INTRA_PHASES", "OHEVC_INTRA_RES_LDS", "OHEVC_SPIN_LIMIT",
                                       "OHEVC_COPY_THREADS", "OHEVC_FETCH_THREADS", "OHEVC_STAMPS", "OHEVC_FETCH_TIMING" };
static const long long DEFAULTS[T_N] = { OH_INTRA_AUTO, 0, 2, -1, 4194304, 2, 3, 0, 0 };

static void flat(const OhTuning &t, long long v[T_N])
{
    v[T_MODE] = t.intra_mode; v[T_WAVES] = t.intra_waves; v[T_PHASES] = t.intra_phases; v[T_RES_LDS] = t.intra_res_lds;
    v[T_SPIN] = t.spin_limit; v[T_COPY] = t.copy_threads; v[T_FETCH] = t.fetch_threads; v[T_STAMPS] = t.stamps; v[T_TIMING] = t.fetch_timing;
}

static void clear_env() { for (const char *n : VARS) unsetenv(n); }

struct TuningRow { int var; const char *value; long long expect; };
/* value -> member, per switch: valid values, then invalid ones.  OHEVC_INTRA_PHASES is kept as given: whether it suits the launch's
 * waves is the plan's business (phases_rows below) */
static const TuningRow TUNING_ROWS[] = {
    { T_MODE, "dag", OH_INTRA_DAG }, { T_MODE, "direct", OH_INTRA_DIRECT }, { T_MODE, "auto", OH_INTRA_AUTO }, { T_MODE, "DAG", OH_INTRA_AUTO },
    { T_MODE, "", OH_INTRA_AUTO }, { T_MODE, "dag ", OH_INTRA_AUTO },
    { T_WAVES, "2", 2 }, { T_WAVES, "4", 4 }, { T_WAVES, "8", 8 }, { T_WAVES, "3", 8 }, { T_WAVES, "0", 8 }, { T_WAVES, "16", 8 },
    { T_WAVES, "-2", 8 }, { T_WAVES, "x", 8 }, { T_WAVES, "", 8 },
    { T_PHASES, "2", 2 }, { T_PHASES, "4", 4 }, { T_PHASES, "8", 8 },
    { T_RES_LDS, "0", 0 }, { T_RES_LDS, "1", 1 }, { T_RES_LDS, "2", 1 }, { T_RES_LDS, "-1", 1 }, { T_RES_LDS, "x", 0 }, { T_RES_LDS, "", 0 },
    { T_SPIN, "1", 1 }, { T_SPIN, "100", 100 }, { T_SPIN, "4194304", 4194304 }, { T_SPIN, "0", 1 }, { T_SPIN, "-5", 1 }, { T_SPIN, "x", 1 },
    { T_COPY, "0", 0 }, { T_COPY, "1", 1 }, { T_COPY, "4", 4 }, { T_COPY, "8", 8 }, { T_COPY, "9", 8 }, { T_COPY, "100", 8 }, { T_COPY, "-1", 0 }, { T_COPY, "x", 0 },
    { T_FETCH, "0", 0 }, { T_FETCH, "1", 1 }, { T_FETCH, "15", 15 }, { T_FETCH, "16", 15 }, { T_FETCH, "-3", 0 }, { T_FETCH, "x", 0 },
    { T_STAMPS, "1", 1 }, { T_STAMPS, "0", 1 }, { T_STAMPS, "", 1 },
    { T_TIMING, "1", 1 }, { T_TIMING, "0", 1 }, { T_TIMING, "", 1 },
};

static void check_tuning()
{
    long long got[T_N];
    what = "tuning, nothing set";
    clear_env();
    flat(tuning_from_env(), got);
    for (int i = 0; i < T_N; i++) CHECK(got[i] == DEFAULTS[i], "%s: %lld, expected %lld", VARS[i], got[i], DEFAULTS[i]);
    flat(OhTuning(), got);                                       /* an engine that read nothing has the same values */
    for (int i = 0; i < T_N; i++) CHECK(got[i] == DEFAULTS[i], "default member %d: %lld, expected %lld", i, got[i], DEFAULTS[i]);
    for (const TuningRow &r : TUNING_ROWS) {
        what = std::string("tuning, ") + VARS[r.var] + "='" + r.value + "'";
        clear_env();
        setenv(VARS[r.var], r.value, 1);
        flat(tuning_from_env(), got);
        for (int i = 0; i < T_N; i++) {                          /* the one member as promised, the others untouched */
            const long long want = i == r.var ? r.expect : DEFAULTS[i];
            CHECK(got[i] == want, "%s: %lld, expected %lld", VARS[i], got[i], want);
        }
    }
    /* all at once; and the environment of the moment counts, not an earlier one */
    what = "tuning, everything set";
    clear_env();
    const char *const all[T_N] = { "direct", "4", "4", "0", "7", "5", "11", "1", "1" };
    const long long all_expect[T_N] = { OH_INTRA_DIRECT, 4, 4, 0, 7, 5, 11, 1, 1 };
    for (int i = 0; i < T_N; i++) setenv(VARS[i], all[i], 1);
    flat(tuning_from_env(), got);
    for (int i = 0; i < T_N; i++) CHECK(got[i] == all_expect[i], "%s: %lld, expected %lld", VARS[i], got[i], all_expect[i]);
    clear_env();
    flat(tuning_from_env(), got);
    for (int i = 0; i < T_N; i++) CHECK(got[i] == DEFAULTS[i], "after unsetting, %s: %lld, expected %lld", VARS[i], got[i], DEFAULTS[i]);
}

/* ---------------- form ---------------- */
static void check_form()
{
    /* 64x64: samples of all planes / 64 per chroma format, and the largest intra_area64 that is still sparse (2 * area < samples/64) */
    static const struct { int chroma; uint32_t samples64, last_sparse; } rows[] = { { 0, 64, 31 }, { 1, 96, 47 }, { 2, 128, 63 }, { 3, 192, 95 } };
    OhTuning automatic, dag, direct;
    dag.intra_mode = OH_INTRA_DAG; direct.intra_mode = OH_INTRA_DIRECT;
    for (const auto &r : rows) {
        what = "form, 64x64 chroma format " + std::to_string(r.chroma);
        OhPicParams p;
        memset(&p, 0, sizeof(p));
        p.width = 64; p.height = 64; p.chroma_format_idc = r.chroma; p.bit_depth = 8; p.log2_ctb_size = 6;
        CHECK(r.last_sparse * 2 + 2 == r.samples64, "the row itself");
        CHECK(intra_plan_direct(&p, 0, automatic), "no intra block at all");
        CHECK(intra_plan_direct(&p, r.last_sparse, automatic), "area %u", r.last_sparse);
        CHECK(!intra_plan_direct(&p, r.last_sparse + 1, automatic), "area %u", r.last_sparse + 1);
        CHECK(!intra_plan_direct(&p, r.samples64, automatic), "all intra");
        CHECK(!intra_plan_direct(&p, 0xffffffffu, automatic), "the largest area a summary can hold");
        for (uint32_t area : { 0u, r.last_sparse, r.last_sparse + 1, r.samples64, 0xffffffffu }) {
            CHECK(!intra_plan_direct(&p, area, dag), "forced dag, area %u", area);
            CHECK(intra_plan_direct(&p, area, direct), "forced direct, area %u", area);
        }
    }
    /* a size whose product needs more than 32 bits before the shift: 65536 x 65536 4:4:4 is 3 * 2^26 units */
    what = "form, 65536x65536 4:4:4";
    OhPicParams p;
    memset(&p, 0, sizeof(p));
    p.width = 65536; p.height = 65536; p.chroma_format_idc = 3;
    CHECK(intra_plan_direct(&p, 100663295u, automatic), "one below half");
    CHECK(!intra_plan_direct(&p, 100663296u, automatic), "half");
}

/* ---------------- layout ---------------- */
static void check_layout_one(int log2_ctb, int chroma, uint32_t waves, bool staged, uint32_t max_items, uint32_t max_sub, uint32_t max_res, const char *name)
{
    what = std::string("layout, ") + name + ", log2_ctb " + std::to_string(log2_ctb) + " chroma " + std::to_string(chroma) + " waves " + std::to_string(waves) +
           (staged ? " staged" : " not staged");
    OhTuning t;
    t.intra_waves = waves; t.intra_res_lds = staged ? 1 : 0;
    OhIntraFigures f;
    f.batch = 1; f.max_items = max_items; f.max_sub = max_sub; f.max_res = max_res;
    f.sum_items = max_items; f.sum_sub = max_sub; f.total_entries = 1;
    const OhIntraLaunch L = intra_plan_launch(log2_ctb, chroma, f, 256, t);
    CHECK(L.waves == waves && L.staged == (staged ? 1u : 0u) && L.phases == 2, "waves %u staged %u phases %u", L.waves, L.staged, L.phases);
    static_assert(sizeof(DevIntra) == 32, "the kernel copies a descriptor as two 16-byte vectors");
    /* the regions in the order intra_ctu_body lays its pointers over them: first byte, bytes, alignment of its accesses */
    const struct { const char *name; uint32_t off; size_t bytes, align; } region[6] = {
        { "samples", 0, (size_t)oh_ctu_areas(log2_ctb, chroma).total * 2, 8 },       /* uint16; rows go as 4-sample vectors */
        { "items", L.off_items, (size_t)max_items * 32, 16 },
        { "sub table", L.off_sub, ((size_t)max_sub + 1) * 4, 4 },
        { "small table", L.off_small, (size_t)max_sub * 4, 4 },
        { "residual", L.off_res, staged ? (size_t)max_res * 2 : 0, 16 },
        { "wave edges", L.off_wave, (size_t)waves * OH_INTRA_WAVE_LDS, 4 },
    };
    for (int i = 0; i < 6; i++) {
        CHECK(region[i].off % region[i].align == 0, "%s at %u", region[i].name, region[i].off);
        if (i + 1 < 6)
            CHECK(region[i].off + region[i].bytes <= region[i + 1].off, "%s [%u, +%zu) runs into %s at %u", region[i].name, region[i].off, region[i].bytes,
                  region[i + 1].name, region[i + 1].off);
    }
    CHECK(L.lds_bytes == L.off_wave + waves * OH_INTRA_WAVE_LDS, "lds_bytes %u, edges end at %u", L.lds_bytes, L.off_wave + waves * OH_INTRA_WAVE_LDS);
    CHECK(L.lds_bytes <= OH_INTRA_MAX_LDS, "lds_bytes %u", L.lds_bytes);
    CHECK(OH_INTRA_WAVE_LDS % 4 == 0, "every wave's edges on a word");
}

static void check_layout()
{
    what = "layout, sample areas";
    CHECK(oh_ctu_areas(4, 0).total == 16 * 20 + 40, "16x16 4:0:0: %u", oh_ctu_areas(4, 0).total);
    CHECK(oh_ctu_areas(6, 3).total == 3 * (64 * 68 + 136), "64x64 4:4:4: %u", oh_ctu_areas(6, 3).total);
    CHECK(oh_ctu_areas(6, 1).total == 64 * 68 + 2 * 32 * 36 + 136 + 2 * 72, "64x64 4:2:0: %u", oh_ctu_areas(6, 1).total);
    CHECK(OH_INTRA_MAX_LDS == 131072, "the grant");
    for (int log2_ctb = 4; log2_ctb <= 6; log2_ctb++)
        for (int chroma = 0; chroma <= 3; chroma++)
            for (uint32_t waves : { 2u, 4u, 8u })
                for (int staged = 0; staged < 2; staged++) {
                    check_layout_one(log2_ctb, chroma, waves, staged != 0, 1, 1, 0, "minimal");
                    /* what prep.hip lets through: OH_MAX_CTU_BLOCKS blocks and sub-levels per schedule entry (prep_intra_ctu fails the list
                     * beyond), and a residual span of at most 3 * 64 * 64 int16 whatever the CTB size and chroma format (a wider one is
                     * not staged: res_cnt = 0) */
                    check_layout_one(log2_ctb, chroma, waves, staged != 0, OH_MAX_CTU_BLOCKS, OH_MAX_CTU_BLOCKS, 3 * 64 * 64, "at the limits");
                    /* odd sizes: the alignments are the plan's, not the inputs' */
                    check_layout_one(log2_ctb, chroma, waves, staged != 0, 7, 3, 4 * 37, "odd");
                }
}

/* ---------------- waves, phases, staging ---------------- */
static void check_waves()
{
    static const struct { int batch; uint64_t sum_items, sum_sub; uint32_t waves; } rows[] = {
        { 1, 0, 0, 2 },                                          /* nothing counted: one block per sub-level */
        { 1, 5, 4, 2 }, { 1, 126, 100, 4 },                      /* 1.25 | 1.26 */
        { 1, 5, 2, 4 }, { 1, 251, 100, 8 },                      /* 2.5 | 2.51 */
        { 7, 5, 2, 4 }, { 7, 251, 100, 8 },
        { 8, 5, 4, 2 }, { 8, 126, 100, 4 },
        { 8, 251, 100, 4 }, { 8, 9, 2, 4 }, { 8, 451, 100, 8 },  /* a batch of 8 or more: 4.5 | 4.51 */
        { 32, 9, 2, 4 }, { 32, 451, 100, 8 },
    };
    for (const auto &r : rows) {
        what = "waves, batch " + std::to_string(r.batch) + " items " + std::to_string(r.sum_items) + " sub-levels " + std::to_string(r.sum_sub);
        OhIntraFigures f;
        f.batch = r.batch; f.sum_items = r.sum_items; f.sum_sub = r.sum_sub;
        const OhIntraLaunch L = intra_plan_launch(6, 1, f, 256, OhTuning());
        CHECK(L.waves == r.waves && L.phases == 2, "waves %u (expected %u), phases %u", L.waves, r.waves, L.phases);
        for (uint32_t forced : { 2u, 4u, 8u }) {
            OhTuning t;
            t.intra_waves = forced;
            CHECK(intra_plan_launch(6, 1, f, 256, t).waves == forced, "forced %u", forced);
        }
    }
    /* OHEVC_INTRA_PHASES against the waves: below 2, above the waves or no divisor of them -> 2 */
    static const struct { const char *waves, *phases; uint32_t expect_waves, expect_phases; } phases_rows[] = {
        { "2", "2", 2, 2 }, { "2", "4", 2, 2 }, { "2", "1", 2, 2 }, { "2", "0", 2, 2 }, { "2", "-1", 2, 2 },
        { "4", "2", 4, 2 }, { "4", "4", 4, 4 }, { "4", "3", 4, 2 }, { "4", "8", 4, 2 },
        { "8", "2", 8, 2 }, { "8", "4", 8, 4 }, { "8", "8", 8, 8 }, { "8", "3", 8, 2 }, { "8", "6", 8, 2 }, { "8", "16", 8, 2 }, { "8", "1", 8, 2 },
        { "8", "x", 8, 2 }, { "8", "-4", 8, 2 }, { "5", "4", 8, 4 }, { "0", "8", 8, 8 },
    };
    for (const auto &r : phases_rows) {
        what = std::string("phases, OHEVC_INTRA_WAVES=") + r.waves + " OHEVC_INTRA_PHASES=" + r.phases;
        clear_env();
        setenv("OHEVC_INTRA_WAVES", r.waves, 1);
        setenv("OHEVC_INTRA_PHASES", r.phases, 1);
        const OhIntraLaunch L = intra_plan_launch(6, 1, OhIntraFigures(), 256, tuning_from_env());
        CHECK(L.waves == r.expect_waves && L.phases == r.expect_phases, "waves %u phases %u", L.waves, L.phases);
    }
    clear_env();
    /* unset, with the waves chosen by content */
    what = "phases, by content";
    for (uint64_t items : { 1u, 2u, 5u }) {
        OhIntraFigures f;
        f.batch = 1; f.sum_items = items; f.sum_sub = 1;
        CHECK(intra_plan_launch(6, 1, f, 256, OhTuning()).phases == 2, "items %llu", (unsigned long long)items);
    }
    /* residual spans in LDS: while the launch has at most a workgroup per CU (schedule entries / 8 <= CUs), unless forced; never when
     * some span is scattered */
    static const struct { int force; bool contiguous; uint64_t entries; int n_cu; uint32_t staged; } staged_rows[] = {
        { -1, true, 0, 256, 1 }, { -1, true, 2055, 256, 1 }, { -1, true, 2056, 256, 0 }, { -1, true, 2048, 256, 1 },
        { -1, true, 839, 104, 1 }, { -1, true, 840, 104, 0 },
        { 1, true, 1000000, 256, 1 }, { 0, true, 1, 256, 0 },
        { -1, false, 1, 256, 0 }, { 1, false, 1, 256, 0 }, { 0, false, 1, 256, 0 },
    };
    for (const auto &r : staged_rows) {
        what = "staging, forced " + std::to_string(r.force) + " contiguous " + std::to_string(r.contiguous) + " entries " + std::to_string(r.entries) +
               " CUs " + std::to_string(r.n_cu);
        OhTuning t;
        t.intra_res_lds = r.force;
        OhIntraFigures f;
        f.batch = 1; f.total_entries = r.entries; f.contiguous = r.contiguous; f.max_res = 64;
        const OhIntraLaunch L = intra_plan_launch(6, 1, f, r.n_cu, t);
        CHECK(L.staged == r.staged, "staged %u", L.staged);
        CHECK(L.off_wave - L.off_res == (r.staged ? 128u : 0u), "residual region of %u bytes", L.off_wave - L.off_res);
    }
}

int main()
{
    check_tuning();
    check_form();
    check_layout();
    check_waves();
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("plan ok\n");
    return 0;
}
