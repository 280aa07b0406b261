/* filter_math_check.cpp — the host-only functions of the filters (openhevc_amd/csrc/pics_math.hip: oh_filter_taps_check,
 * oh_filter_binomial, oh_filter_box, oh_filter_unsharp, oh_filter_median9, oh_filter_temporal) run on the CPU as a program of its own;
 * built together with that file, with AddressSanitizer and UBSan, by tests/test_filter_math_host.py.  The arrays they read and write are
 * heap blocks of exactly nine and fifteen elements, so an access one entry too far is a sanitizer report, and the values are the
 * extremes of their domains.  Exit status 0: every check held. */
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

/* every n: the legal ones fill exactly n entries of a block of n that sum to 256, the others are refused */
static int rows_group(void)
{
    int made = 0;
    for (int n = -1; n <= 17; n++) {
        const bool odd = n >= 1 && n <= OH_FILTER_MAX_TAPS && (n & 1);
        auto row = heap<int16_t>(odd ? (size_t)n : 1);
        row[0] = -7;
        int rc = oh_filter_box(n, row.get());
        CHECK(rc == (odd ? OH_OK : OH_E_ARG), "box %d: %d", n, rc);
        if (odd) {
            int sum = 0;
            for (int i = 0; i < n; i++) { sum += row[i]; CHECK(row[i] == 256 / n + (i == n / 2 ? 256 % n : 0), "box %d, tap %d: %d", n, i, row[i]); }
            CHECK(sum == 256, "box %d sums to %d", n, sum);
            made++;
        } else
            CHECK(row[0] == -7, "box %d wrote", n);
        const bool bin = odd && n <= 9;
        row[0] = -7;
        rc = oh_filter_binomial(n, row.get());
        CHECK(rc == (bin ? OH_OK : OH_E_ARG), "binomial %d: %d", n, rc);
        if (bin) {
            int sum = 0;
            for (int i = 0; i < n; i++) { sum += row[i]; CHECK(row[i] == row[n - 1 - i] && row[i] >= 1, "binomial %d, tap %d: %d", n, i, row[i]); }
            CHECK(sum == 256 && row[n / 2] == std::max<int>(row[0], row[n / 2]), "binomial %d sums to %d", n, sum);
            made++;
        } else
            CHECK(row[0] == -7, "binomial %d wrote", n);
    }
    CHECK(oh_filter_box(3, nullptr) == OH_E_ARG && oh_filter_binomial(3, nullptr) == OH_E_ARG, "null rows");
    return made;
}

/* tap sets at the limits: the largest and the smallest int16 values, fifteen taps on both axes, counts at and past the ends */
static int taps_group(void)
{
    int checked = 0;
    auto t = heap<OhFilterTaps>(1);
    auto set = [&](int nh, int nv, int16_t fill) {
        memset(t.get(), 0, sizeof(OhFilterTaps));
        t[0].nh = nh; t[0].nv = nv;
        for (int i = 0; i < OH_FILTER_MAX_TAPS; i++) t[0].h[i] = t[0].v[i] = fill;
        checked++;
    };
    set(15, 15, 0); t[0].h[0] = 256; t[0].v[14] = 256;
    CHECK(oh_filter_taps_check(t.get()) == OH_OK, "one tap at either end");
    set(15, 15, 0); t[0].h[0] = -128; t[0].h[14] = 384; t[0].v[7] = 256;
    CHECK(oh_filter_taps_check(t.get()) == OH_OK, "magnitudes of exactly 512");
    set(15, 15, 0); t[0].h[0] = -129; t[0].h[14] = 385; t[0].v[7] = 256;
    CHECK(oh_filter_taps_check(t.get()) == OH_E_ARG, "magnitudes of 514");
    set(15, 15, 32767);
    CHECK(oh_filter_taps_check(t.get()) == OH_E_ARG, "fifteen taps of 32767");
    set(15, 15, -32768);
    CHECK(oh_filter_taps_check(t.get()) == OH_E_ARG, "fifteen taps of -32768");
    set(15, 15, 32767); t[0].h[14] = (int16_t)(256 - 14 * 32767 % 65536);      /* a sum that would be 256 in 16-bit arithmetic only */
    CHECK(oh_filter_taps_check(t.get()) == OH_E_ARG, "a sum that wraps");
    set(1, 1, -32768); t[0].h[0] = t[0].v[0] = 256;
    CHECK(oh_filter_taps_check(t.get()) == OH_OK, "the taps behind nh and nv are not read");
    const int bad[] = { 0, 2, 14, 16, 17, -1, -15, 2147483647, -2147483647 - 1 };
    for (int n : bad) {
        set(n, 1, 0); t[0].h[0] = t[0].v[0] = 256;
        CHECK(oh_filter_taps_check(t.get()) == OH_E_ARG, "nh %d", n);
        set(1, n, 0); t[0].h[0] = t[0].v[0] = 256;
        CHECK(oh_filter_taps_check(t.get()) == OH_E_ARG, "nv %d", n);
    }
    CHECK(oh_filter_taps_check(nullptr) == OH_E_ARG, "a null pointer");
    return checked;
}

/* unsharp and temporal at the corners of their domains, the median over every block of nine values 0 / M */
static long samples_group(int bit_depth)
{
    const int32_t M = (1 << bit_depth) - 1;
    long calls = 0;
    const int32_t sv[] = { 0, 1, M - 1, M }, av[] = { -64, -1, 0, 1, 512 }, tv[] = { 0, 1, M - 1, M };
    for (int32_t s : sv) for (int32_t b : sv) for (int32_t a : av) for (int32_t t : tv) {
        const int32_t out = oh_filter_unsharp(s, b, a, t, M);
        calls++;
        CHECK(out >= 0 && out <= M, "unsharp(%d, %d, %d, %d): %d", s, b, a, t, out);
        const int32_t d = s - b;
        if ((d < 0 ? -d : d) <= t || a == 0 || d == 0)
            CHECK(out == s, "unsharp(%d, %d, %d, %d) is no copy: %d", s, b, a, t, out);
        if (a == 64 && (d < 0 ? -d : d) > t)
            CHECK(out == std::min(std::max(s + d, 0), M), "unsharp(%d, %d, 64, %d): %d", s, b, t, out);
    }
    auto v = heap<int32_t>(9);
    for (int k = 0; k < 512; k++) {
        int ones = 0;
        for (int i = 0; i < 9; i++) { v[i] = (k >> i & 1) ? M : 0; ones += k >> i & 1; }
        const int32_t out = oh_filter_median9(v.get());
        calls++;
        CHECK(out == (ones >= 5 ? M : 0), "%d bit, median of pattern %#x: %d", bit_depth, k, out);
    }
    for (int i = 0; i < 9; i++) v[i] = 2147483647 - i;              /* no arithmetic on the values: the largest ints pass */
    CHECK(oh_filter_median9(v.get()) == 2147483647 - 4, "median of the largest ints");
    for (int i = 0; i < 9; i++) v[i] = -2147483647 - 1 + (i * 5) % 9;
    CHECK(oh_filter_median9(v.get()) == -2147483647 - 1 + 4, "median of the smallest ints");
    const int32_t mv[] = { 0, 1, 9 * M - 1, 9 * M };
    for (int32_t c : sv) for (int32_t p : sv) for (int32_t n : sv) for (int32_t mp : mv) for (int32_t mn : mv) for (int32_t t : mv) {
        const int32_t out = oh_filter_temporal(c, p, n, mp, mn, t);
        calls++;
        const int32_t want = ((mp <= t ? p : c) + 2 * c + (mn <= t ? n : c) + 2) >> 2;
        CHECK(out == want && out >= 0 && out <= M, "temporal(%d, %d, %d, %d, %d, %d): %d", c, p, n, mp, mn, t, out);
    }
    return calls;
}

int main(void)
{
    printf("rows: %d made\n", rows_group());
    printf("tap sets: %d\n", taps_group());
    for (int bd : { 8, 9, 10, 12 })
        printf("samples, %d bit: %ld calls\n", bd, samples_group(bd));
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("filter math ok\n");
    return 0;
}
