/* lut_math_check.cpp — the host-only functions of the histograms and look-up tables (openhevc_amd/csrc/pics_math.hip: oh_hist_percentile,
 * oh_hist_distance, oh_lut_identity, oh_lut_range, oh_lut_linear, oh_lut_stretch, oh_lut_equalise, oh_lut_then) run on the CPU as a
 * program of its own; built together with that file, with AddressSanitizer and UBSan, by tests/test_lut_math_host.py.  The tables they
 * write are heap blocks of exactly 2^depth entries and the histograms single heap OhPlaneHist, so an access one entry too far is a
 * sanitizer report, and the values are the extremes of their domains.  Exit status 0: every check held. */
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <memory>

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

static const int DEPTHS[] = { 8, 9, 10, 12 };
static const int32_t I32_MAX = 2147483647, I32_MIN = -2147483647 - 1;

static bool in_range_rising(const uint16_t *t, int n, int top)
{
    for (int v = 0; v < n; v++)
        if (t[v] > top || (v && t[v] < t[v - 1]))
            return false;
    return true;
}

/* identity and the four range tables at every pair of depths, into blocks of exactly 2^bs entries */
static int static_tables_group(void)
{
    int made = 0;
    for (int bs : DEPTHS) for (int bd : DEPTHS) {
        const int n = 1 << bs, Md = (1 << bd) - 1;
        auto t = heap<uint16_t>((size_t)n);
        CHECK(oh_lut_identity(bs, bd, t.get()) == OH_OK && in_range_rising(t.get(), n, Md), "identity %d -> %d", bs, bd);
        CHECK(t[0] == 0 && t[n - 1] == (bd >= bs ? (n - 1) << (bd - bs) : Md), "identity %d -> %d: ends %d, %d", bs, bd, t[0], t[n - 1]);
        made++;
        for (int kind = 0; kind < 4; kind++) {
            CHECK(oh_lut_range(bs, bd, kind & 1, kind >> 1, t.get()) == OH_OK && in_range_rising(t.get(), n, Md), "range %d -> %d, kind %d", bs, bd, kind);
            made++;
        }
    }
    auto one = heap<uint16_t>(1);
    one[0] = 7;
    const int bad[] = { 0, 7, 11, 13, 16, -1, I32_MAX, I32_MIN };
    for (int b : bad) {
        CHECK(oh_lut_identity(b, 8, one.get()) == OH_E_ARG && oh_lut_identity(8, b, one.get()) == OH_E_ARG, "identity, depth %d", b);
        CHECK(oh_lut_range(b, 8, 1, 1, one.get()) == OH_E_ARG && oh_lut_range(8, b, 0, 0, one.get()) == OH_E_ARG, "range, depth %d", b);
        CHECK(oh_lut_linear(b, 8, 65536, 0, 0, one.get()) == OH_E_ARG && oh_lut_linear(8, b, 65536, 0, 0, one.get()) == OH_E_ARG, "linear, depth %d", b);
    }
    CHECK(one[0] == 7, "a refused builder wrote");
    CHECK(oh_lut_identity(8, 8, nullptr) == OH_E_ARG && oh_lut_range(8, 8, 0, 0, nullptr) == OH_E_ARG && oh_lut_linear(8, 8, 0, 0, 0, nullptr) == OH_E_ARG,
          "null tables");
    return made;
}

/* the linear table with gains and pivots at the ends of int32: the products stay inside int64 */
static long linear_group(void)
{
    long made = 0;
    const int32_t ends[] = { I32_MIN, I32_MIN + 1, -65536, -1, 0, 1, 65536, 131072, I32_MAX - 1, I32_MAX };
    for (int bs : DEPTHS) for (int bd : DEPTHS) {
        const int n = 1 << bs, Md = (1 << bd) - 1;
        auto t = heap<uint16_t>((size_t)n);
        for (int32_t g : ends) for (int32_t pi : ends) for (int32_t po : ends) {
            CHECK(oh_lut_linear(bs, bd, g, pi, po, t.get()) == OH_OK, "linear %d -> %d (%d, %d, %d)", bs, bd, g, pi, po);
            bool ok = true;
            for (int v = 0; v < n; v++)
                ok = ok && t[v] <= Md && (!v || (g >= 0 ? t[v] >= t[v - 1] : t[v] <= t[v - 1]));
            CHECK(ok, "linear %d -> %d (%d, %d, %d): outside 0 .. %d or not monotone", bs, bd, g, pi, po, Md);
            made++;
        }
        CHECK(oh_lut_linear(bs, bd, -65536, 0, Md, t.get()) == OH_OK && t[0] == Md && t[std::min(n - 1, Md)] == Md - std::min(n - 1, Md), "inversion %d -> %d", bs, bd);
    }
    return made;
}

/* histograms at their limits: every bin full, one bin, the last bin, none; one heap OhPlaneHist each */
static int histogram_group(void)
{
    int made = 0;
    auto h = heap<OhPlaneHist>(1), g = heap<OhPlaneHist>(1);
    auto fill = [](OhPlaneHist *p, uint32_t every, int only, uint32_t count) {
        memset(p, 0, sizeof(*p));
        for (int v = 0; v < OH_HIST_BINS; v++) p->hist[v] = every;
        if (only >= 0) p->hist[only] = count;
    };
    uint32_t v = 0;
    uint64_t sad = 0;
    for (int bd : DEPTHS) {
        const int n = 1 << bd, M = n - 1;
        auto t = heap<uint16_t>((size_t)n);
        fill(h.get(), 0xFFFFFFFFu, -1, 0);                                  /* 2^44 samples: the products with 10^6 and with M fit 64 bits */
        CHECK(oh_hist_percentile(h.get(), 1, 1000000u, &v) == OH_OK && v == OH_HIST_BINS - 1, "full bins, top: %u", v);
        CHECK(oh_hist_percentile(h.get(), 1, 0, &v) == OH_OK && v == 0, "full bins, bottom: %u", v);
        CHECK(oh_lut_equalise(h.get(), 1, bd, t.get()) == OH_OK && in_range_rising(t.get(), n, M), "equalise of full bins, %d bit", bd);
        CHECK(oh_lut_stretch(h.get(), 1, 0, 0, bd, t.get()) == OH_OK && in_range_rising(t.get(), n, M), "stretch of full bins, %d bit", bd);
        CHECK(oh_lut_stretch(h.get(), 1, 999999u, 0, bd, t.get()) == OH_OK && in_range_rising(t.get(), n, M), "stretch at the top, %d bit", bd);
        fill(g.get(), 0, -1, 0);
        CHECK(oh_hist_distance(h.get(), g.get(), &sad) == OH_OK && sad == (uint64_t)OH_HIST_BINS * 0xFFFFFFFFu, "distance of full and empty");
        CHECK(oh_lut_equalise(g.get(), 1, bd, t.get()) == OH_OK && t[0] == 0 && t[M] == M, "equalise of nothing is the identity");
        CHECK(oh_lut_stretch(g.get(), 1, 0, 0, bd, t.get()) == OH_E_ARG && oh_hist_percentile(g.get(), 1, 0, &v) == OH_E_ARG, "nothing to stretch");
        fill(h.get(), 0, M, 0xFFFFFFFFu);                                   /* everything in the depth's top bin */
        CHECK(oh_hist_percentile(h.get(), 1, 500000u, &v) == OH_OK && v == (uint32_t)M, "top bin: %u", v);
        CHECK(oh_lut_equalise(h.get(), 1, bd, t.get()) == OH_OK && t[M] == M && t[1] == 1, "equalise of one value is the identity");
        CHECK(oh_lut_stretch(h.get(), 1, 0, 0, bd, t.get()) == OH_OK && t[M] == M && t[1] == 1, "stretch of one value is the identity");
        fill(h.get(), 0, OH_HIST_BINS - 1, 1); h[0].hist[0] = 1;            /* the two ends of the bins, whatever the depth */
        CHECK(oh_lut_equalise(h.get(), 1, bd, t.get()) == OH_OK && in_range_rising(t.get(), n, M), "equalise of the two ends, %d bit", bd);
        CHECK(oh_lut_stretch(h.get(), 1, 0, 0, bd, t.get()) == OH_OK && in_range_rising(t.get(), n, M), "stretch of the two ends, %d bit", bd);
        made += 10;
    }
    CHECK(oh_lut_stretch(h.get(), 1, 0xFFFFFFFFu, 0xFFFFFFFFu, 8, nullptr) == OH_E_ARG, "ppm that would wrap");
    CHECK(oh_hist_percentile(h.get(), 1, 1000001u, &v) == OH_E_ARG && oh_hist_percentile(h.get(), 0, 0, &v) == OH_E_ARG, "percentile arguments");
    return made;
}

/* composition: tables of exactly n1 and n2 entries, entries at n2 - 1 and at n2 */
static int then_group(void)
{
    int made = 0;
    for (int bs : DEPTHS) for (int bd : DEPTHS) {
        const int n1 = 1 << bs, n2 = 1 << bd;
        auto first = heap<uint16_t>((size_t)n1), second = heap<uint16_t>((size_t)n2), out = heap<uint16_t>((size_t)n1);
        for (int v = 0; v < n1; v++) { first[v] = (uint16_t)(n2 - 1 - v % n2); out[v] = 0xABCD; }
        for (int v = 0; v < n2; v++) second[v] = (uint16_t)(v ^ 1);
        CHECK(oh_lut_then(first.get(), n1, second.get(), n2, out.get()) == OH_OK, "then %d, %d", n1, n2);
        CHECK(out[0] == ((n2 - 1) ^ 1) && out[n1 - 1] == second[first[n1 - 1]], "then %d, %d: values", n1, n2);
        first[n1 - 1] = (uint16_t)n2; out[0] = 0xABCD;
        CHECK(oh_lut_then(first.get(), n1, second.get(), n2, out.get()) == OH_E_ARG && out[0] == 0xABCD, "an entry at n2 is refused, nothing written");
        first[n1 - 1] = 0xFFFF;
        CHECK(oh_lut_then(first.get(), n1, second.get(), n2, out.get()) == OH_E_ARG, "an entry of 65535");
        made++;
    }
    uint16_t x = 0;
    CHECK(oh_lut_then(&x, 0, &x, 1, &x) == OH_E_ARG && oh_lut_then(&x, 1, &x, 0, &x) == OH_E_ARG && oh_lut_then(&x, -1, &x, 1, &x) == OH_E_ARG, "counts below 1");
    CHECK(oh_lut_then(&x, 1, &x, 1, &x) == OH_OK && x == 0, "in place");
    return made;
}

int main(void)
{
    printf("static tables: %d made\n", static_tables_group());
    printf("linear tables: %ld made\n", linear_group());
    printf("histograms: %d checks\n", histogram_group());
    printf("compositions: %d made\n", then_group());
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("lut math ok\n");
    return 0;
}
