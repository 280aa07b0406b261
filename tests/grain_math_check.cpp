/* grain_math_check.cpp — the host-only functions of the film grain service (openhevc_amd/csrc/pics_math.hip: oh_grain_hash, _gauss,
 * _pattern, _uniform, _from_sei, _block, _mean, _value, _smooth, _blend) run on the CPU as a program of its own; built together with
 * that file, with AddressSanitizer and UBSan, by tests/test_grain_math_host.py.  The arrays they read and write are heap blocks of
 * exactly the sizes they may touch (1024 coefficients, 1024 pattern bytes, 256 entries, 3 x 256 entries, one OhFilmGrainSei), so an
 * access one entry too far is a sanitizer report, and the values are the extremes of their domains, where a signed overflow or a shift
 * of a negative value would be one too.  Exit status 0: every check held. */
#include <stdio.h>
#include <string.h>
#include <memory>

#include "../include/ohevc_annexb.h"
#include "../include/ohevc_hip.h"

static int failures;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            failures++;                                                                    \
            fprintf(stderr, "%s (line %d): ", #cond, __LINE__);                             \
            fprintf(stderr, __VA_ARGS__);                                                  \
            fprintf(stderr, "\n");                                                         \
        }                                                                                  \
    } while (0)

template <typename T> static std::unique_ptr<T[]> heap(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

/* all 169 patterns, each output alone and all together: the coefficients stay in their corner, the pattern in -127 .. 127 with a mean
 * square of 32^2 +- 1/16 */
static long pattern_group(void)
{
    long calls = 0;
    for (int fh = 2; fh <= 14; fh++)
        for (int fv = 2; fv <= 14; fv++) {
            auto c = heap<int16_t>(1024);
            auto r = heap<int16_t>(1024);
            auto p = heap<int8_t>(1024);
            auto p2 = heap<int8_t>(1024);
            CHECK(oh_grain_pattern(fh, fv, c.get(), r.get(), p.get()) == OH_OK, "(%d, %d)", fh, fv);
            CHECK(oh_grain_pattern(fh, fv, nullptr, nullptr, p2.get()) == OH_OK && !memcmp(p.get(), p2.get(), 1024), "(%d, %d) pattern alone", fh, fv);
            CHECK(oh_grain_pattern(fh, fv, c.get(), nullptr, nullptr) == OH_OK && oh_grain_pattern(fh, fv, nullptr, r.get(), nullptr) == OH_OK, "one output");
            calls += 4;
            long long ss = 0;
            int outside = 0, lo = 0;
            for (int v = 0; v < 32; v++)
                for (int u = 0; u < 32; u++) {
                    if ((u >= 2 * fh || v >= 2 * fv || (!u && !v)) && c[v * 32 + u]) outside++;
                    if (c[v * 32 + u] < -4080 || c[v * 32 + u] > 4080) outside++;
                    ss += (long long)p[v * 32 + u] * p[v * 32 + u];
                    if (p[v * 32 + u] < -127) lo++;
                }
            CHECK(!outside && !lo, "(%d, %d): %d coefficients outside, %d samples below -127", fh, fv, outside, lo);
            CHECK(ss >= 961 * 1024 && ss <= 1089 * 1024, "(%d, %d): sum of squares %lld", fh, fv, ss);
        }
    auto p = heap<int8_t>(1024);
    CHECK(oh_grain_pattern(1, 8, nullptr, nullptr, p.get()) == OH_E_ARG && oh_grain_pattern(8, 15, nullptr, nullptr, p.get()) == OH_E_ARG &&
          oh_grain_pattern(-1, -1, nullptr, nullptr, nullptr) == OH_E_ARG && oh_grain_pattern(8, 8, nullptr, nullptr, nullptr) == OH_OK, "pattern refusals");
    return calls + 4;
}

static long hash_group(void)
{
    long calls = 0;
    const uint32_t ends[] = { 0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu };
    int lo = 0, hi = 0;
    for (uint32_t a : ends)
        for (uint32_t b : ends)
            for (uint32_t c : ends)
                for (uint32_t d : ends) {
                    const int32_t g = oh_grain_gauss(oh_grain_hash(a, b, c, d));
                    calls += 2;
                    CHECK(g >= -510 && g <= 510, "gauss %d", g);
                    lo += g < 0; hi += g > 0;
                }
    CHECK(lo > 200 && hi > 200, "gauss is one-sided: %d below, %d above", lo, hi);
    CHECK(oh_grain_gauss(0) == -510 && oh_grain_gauss(0xFFFFFFFFu) == 510, "gauss ends");
    auto ox = heap<int>(1), oy = heap<int>(1), ng = heap<int>(1);
    for (uint32_t seed : ends)
        for (int c = 0; c < 3; c++)
            for (int bx : { 0, 1, 479, 65535 })
                for (int by : { 0, 1, 269, 65535 }) {
                    CHECK(oh_grain_block(seed, c, bx, by, ox.get(), oy.get(), ng.get()) == OH_OK, "block");
                    CHECK(ox[0] >= 0 && ox[0] <= 24 && oy[0] >= 0 && oy[0] <= 24 && (ng[0] == 0 || ng[0] == 1), "block (%d, %d): %d %d %d", bx, by, ox[0], oy[0], ng[0]);
                    calls++;
                }
    CHECK(oh_grain_block(0, 3, 0, 0, ox.get(), oy.get(), ng.get()) == OH_E_ARG && oh_grain_block(0, 0, 65536, 0, ox.get(), oy.get(), ng.get()) == OH_E_ARG &&
          oh_grain_block(0, 0, 0, -1, ox.get(), oy.get(), ng.get()) == OH_E_ARG && oh_grain_block(0, 0, 0, 0, nullptr, oy.get(), ng.get()) == OH_E_ARG &&
          oh_grain_block(0, 0, 0, 0, ox.get(), nullptr, ng.get()) == OH_E_ARG && oh_grain_block(0, 0, 0, 0, ox.get(), oy.get(), nullptr) == OH_E_ARG, "block refusals");
    return calls + 6;
}

/* the sample arithmetic at the ends of every domain */
static long sample_group(void)
{
    long calls = 0;
    for (int bd : { 8, 9, 10, 12 }) {
        const int M = (1 << bd) - 1;
        for (int n : { 64, 32, 16 }) {
            CHECK(oh_grain_mean(0, n, bd) == 0 && oh_grain_mean((uint32_t)(M * n), n, bd) == 255, "mean ends, %d bit, n %d", bd, n);
            CHECK(oh_grain_mean((uint32_t)(M * n - n / 2), n, bd) == 255 && oh_grain_mean((uint32_t)(M * n - n / 2 - 1), n, bd) == 255 - (bd == 8),
                  "mean rounds, %d bit, n %d", bd, n);
            calls += 3;
        }
        CHECK(oh_grain_mean(0, 63, bd) == -1 && oh_grain_mean(0, 0, bd) == -1, "mean refusals");
        int32_t gmin = 0, gmax = 0;
        for (int ls = 0; ls <= 15; ls++)
            for (int sigma : { 0, 1, 255 })
                for (int p : { -127, -1, 0, 1, 127 }) {
                    const int32_t g = oh_grain_value(sigma, p, bd, ls);
                    calls++;
                    CHECK((sigma && p) || g == 0, "value of nothing is %d", g);
                    CHECK(g == -oh_grain_value(sigma, -p, bd, ls) || ((sigma * p * (1 << (bd - 8))) & ((1 << (5 + ls)) - 1)) == (1 << (4 + ls)),
                          "value is not odd in p away from the halves: sigma %d p %d", sigma, p);
                    gmin = g < gmin ? g : gmin; gmax = g > gmax ? g : gmax;
                }
        CHECK(gmax == (255 * 127 * (1 << (bd - 8)) + 16) >> 5 && gmin == (-255 * 127 * (1 << (bd - 8)) + 16) >> 5, "value ends %d %d", gmin, gmax);
        for (int32_t l : { gmin, 0, gmax })
            for (int32_t g : { gmin, 0, gmax })
                for (int32_t r : { gmin, 0, gmax }) {
                    const int32_t s = oh_grain_smooth(l, g, r);
                    calls++;
                    CHECK(s >= gmin && s <= gmax, "smooth leaves the range: %d", s);
                    for (int blending = 0; blending <= 1; blending++)
                        for (int32_t v : { 0, 1, M / 2, M - 1, M }) {
                            const int32_t o = oh_grain_blend(v, s, bd, blending);
                            calls++;
                            CHECK(o >= 0 && o <= M, "blend leaves the range: %d", o);
                            CHECK(s || o == v, "no grain changes the sample");
                        }
                }
    }
    CHECK(oh_grain_mean(0, 64, 11) == -1, "mean at 11 bit");
    /* outside their domains the three answer 0 and shift by nothing */
    CHECK(oh_grain_value(255, 127, 7, 0) == 0 && oh_grain_value(255, 127, 11, 0) == 0 && oh_grain_value(255, 127, INT32_MIN, 0) == 0 &&
          oh_grain_value(255, 127, 8, -1) == 0 && oh_grain_value(255, 127, 8, 16) == 0 && oh_grain_value(255, 127, 8, INT32_MAX) == 0 &&
          oh_grain_value(256, 127, 8, 0) == 0 && oh_grain_value(-1, 127, 8, 0) == 0 && oh_grain_value(255, 128, 8, 0) == 0 &&
          oh_grain_value(INT32_MAX, INT32_MIN, 8, 0) == 0, "value refusals");
    CHECK(oh_grain_smooth(INT32_MAX, INT32_MAX, INT32_MAX) == 0 && oh_grain_smooth(INT32_MIN, 0, 0) == 0 && oh_grain_smooth(0, OH_GRAIN_MAX + 1, 0) == 0 &&
          oh_grain_smooth(OH_GRAIN_MAX, OH_GRAIN_MAX, OH_GRAIN_MAX) == OH_GRAIN_MAX && oh_grain_smooth(-OH_GRAIN_MAX, -OH_GRAIN_MAX, -OH_GRAIN_MAX) == -OH_GRAIN_MAX,
          "smooth refusals and ends");
    CHECK(oh_grain_blend(1, 1, 7, 0) == 0 && oh_grain_blend(1, 1, 64, 0) == 0 && oh_grain_blend(1, 1, 8, 2) == 0 && oh_grain_blend(1, 1, 8, -1) == 0 &&
          oh_grain_blend(-1, 1, 8, 0) == 0 && oh_grain_blend(256, 1, 8, 0) == 0 && oh_grain_blend(4095, INT32_MAX, 12, 1) == 0 &&
          oh_grain_blend(4095, OH_GRAIN_MAX, 12, 1) == 4095 && oh_grain_blend(4095, -OH_GRAIN_MAX, 12, 1) == 0 && oh_grain_blend(4095, -OH_GRAIN_MAX, 12, 0) == 0,
          "blend refusals and ends");
    return calls;
}

/* tables: exactly 256 entries, exactly 3 x 256, one OhFilmGrainSei on the heap with every interval in use */
static long table_group(void)
{
    long calls = 0;
    auto t = heap<uint32_t>(256);
    CHECK(oh_grain_uniform(255, 14, 2, t.get()) == OH_OK && t[0] == (255u | 14u << 8 | 2u << 12) && t[255] == t[0], "uniform");
    CHECK(oh_grain_uniform(256, 8, 8, t.get()) == OH_E_ARG && oh_grain_uniform(-1, 8, 8, t.get()) == OH_E_ARG && oh_grain_uniform(1, 15, 8, t.get()) == OH_E_ARG &&
          oh_grain_uniform(1, 8, 1, t.get()) == OH_E_ARG && oh_grain_uniform(1, 8, 8, nullptr) == OH_E_ARG, "uniform refusals");
    calls += 6;
    std::unique_ptr<OhFilmGrainSei> s(new OhFilmGrainSei);
    auto tabs = heap<uint32_t>(3 * 256);
    std::unique_ptr<OhGrain> g(new OhGrain);
    uint32_t (*tp)[256] = reinterpret_cast<uint32_t (*)[256]>(tabs.get());
    memset(s.get(), 0, sizeof(OhFilmGrainSei));
    s->present = 1;
    s->log2_scale_factor = 15; s->blending_mode_id = 1;
    for (int c = 0; c < 3; c++) {
        s->comp_model_present[c] = 1;
        s->num_intensity_intervals_minus1[c] = 255;
        s->num_model_values_minus1[c] = 2;
        for (int i = 0; i < 256; i++) {
            s->lower[c][i] = s->upper[c][i] = (uint8_t)i;
            s->value[c][i][0] = i; s->value[c][i][1] = 2 + i % 13; s->value[c][i][2] = 14 - i % 13;
        }
    }
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_OK, "256 intervals a component");
    CHECK(g->planes == 7 && g->blending == 1 && g->log2_scale == 15 && g->table[2] == tabs.get() + 512, "fields");
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 256; i++)
            CHECK(tp[c][i] == ((uint32_t)i | (uint32_t)(2 + i % 13) << 8 | (uint32_t)(14 - i % 13) << 12), "entry [%d][%d]", c, i);
    calls++;
    /* the ends of the model values and every refusal */
    s->num_intensity_intervals_minus1[0] = 0;
    s->lower[0][0] = 0; s->upper[0][0] = 255;
    const int32_t bad_sigma[] = { -1, 256, INT32_MAX, INT32_MIN };
    for (int32_t v : bad_sigma) {
        s->value[0][0][0] = v;
        CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_UNSUPPORTED, "sigma %d", v);
        calls++;
    }
    s->value[0][0][0] = 255;
    const int32_t bad_cut[] = { 1, 15, 0, -1, INT32_MAX, INT32_MIN };
    for (int k = 1; k <= 2; k++)
        for (int32_t v : bad_cut) {
            const int32_t keep = s->value[0][0][k];
            s->value[0][0][k] = v;
            CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_UNSUPPORTED, "cut-off %d", v);
            s->value[0][0][k] = keep;
            calls++;
        }
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_OK && tp[0][255] == (255u | 2u << 8 | 14u << 12), "one interval over all");
    s->num_model_values_minus1[1] = 3;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_UNSUPPORTED, "four model values");
    s->num_model_values_minus1[1] = 5;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_UNSUPPORTED, "six model values");
    s->num_model_values_minus1[1] = 0;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_OK && tp[1][7] == (7u | 8u << 8 | 8u << 12), "one model value: the defaults");
    s->upper[2][3] = 4;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_UNSUPPORTED, "overlap");
    s->upper[2][3] = 2;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_UNSUPPORTED, "lower above upper");
    s->upper[2][3] = 3;
    s->model_id = 1;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_UNSUPPORTED, "model 1");
    s->model_id = 0; s->blending_mode_id = 2;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_UNSUPPORTED, "blending 2");
    s->blending_mode_id = 0; s->cancel = 1;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_ARG, "cancelled");
    s->cancel = 0; s->present = 0;
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_E_ARG, "absent");
    s->present = 1;
    CHECK(oh_grain_from_sei(nullptr, tp, g.get()) == OH_E_ARG && oh_grain_from_sei(s.get(), nullptr, g.get()) == OH_E_ARG &&
          oh_grain_from_sei(s.get(), tp, nullptr) == OH_E_ARG, "null pointers");
    CHECK(oh_grain_from_sei(s.get(), tp, g.get()) == OH_OK, "and whole again");
    return calls + 16;
}

int main(void)
{
    printf("patterns: %ld calls\n", pattern_group());
    printf("hash, gauss and blocks: %ld calls\n", hash_group());
    printf("samples: %ld calls\n", sample_group());
    printf("tables: %ld calls\n", table_group());
    if (failures) {
        printf("grain math: %d checks failed\n", failures);
        return 1;
    }
    printf("grain math ok\n");
    return 0;
}
