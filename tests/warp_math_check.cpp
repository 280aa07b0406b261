/* warp_math_check.cpp — the host-only functions of the warp service (openhevc_amd/csrc/pics_math.hip: oh_warp_position, oh_warp_cubic,
 * oh_warp_interp, oh_warp_paths and the map builders) run on the CPU as a program of its own; built together with that file, with
 * AddressSanitizer and UBSan, by tests/test_warp_math_host.py.  The arrays they read and write are heap blocks of exactly the sizes
 * they may touch (16 taps, 4 coefficients, one OhWarp), so an access one entry too far is a sanitizer report, and the values are the
 * extremes of their domains, where a signed overflow or a shift of a negative value would be one too.  Exit status 0: every check held. */
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

static const int64_t B22 = (int64_t)1 << 22, B26 = (int64_t)1 << 26, B36 = (int64_t)1 << 36;

/* every phase: the sum, the mirror, the bound on the magnitudes */
static long cubic_group(void)
{
    long calls = 0;
    auto c = heap<int16_t>(4);
    auto r = heap<int16_t>(4);
    for (int f = 0; f < 64; f++) {
        CHECK(oh_warp_cubic(f, c.get()) == OH_OK, "phase %d", f);
        calls++;
        int sum = 0, mag = 0;
        for (int k = 0; k < 4; k++) { sum += c[k]; mag += c[k] < 0 ? -c[k] : c[k]; }
        CHECK(sum == 1024 && mag <= 1296, "phase %d: sum %d, magnitudes %d", f, sum, mag);
        if (f) {
            CHECK(oh_warp_cubic(64 - f, r.get()) == OH_OK, "phase %d", 64 - f);
            CHECK(c[0] == r[3] && c[1] == r[2] && c[2] == r[1] && c[3] == r[0], "phase %d is not phase %d reversed", f, 64 - f);
        }
    }
    CHECK(oh_warp_cubic(-1, c.get()) == OH_E_ARG && oh_warp_cubic(64, c.get()) == OH_E_ARG && oh_warp_cubic(0, nullptr) == OH_E_ARG, "cubic refusals");
    return calls;
}

/* every fraction of every filter at every depth on neighbourhoods of 0, of M and of the alternating patterns: a constant neighbourhood
 * gives itself, every result lies in 0 .. M, a fraction of zero gives the centre tap */
static long interp_group(int bd)
{
    const int M = (1 << bd) - 1;
    long calls = 0;
    auto t = heap<uint16_t>(16);
    for (int pattern = 0; pattern < 6; pattern++) {
        for (int i = 0; i < 16; i++)
            t[i] = (uint16_t)(pattern == 0 ? 0 : pattern == 1 ? M : pattern < 4 ? ((i + pattern) & 1) * M : ((i + i / 4 + pattern) & 1) * M);
        for (int filter = OH_WARP_NEAREST; filter <= OH_WARP_BICUBIC; filter++)
            for (int fy = 0; fy < 64; fy++)
                for (int fx = 0; fx < 64; fx++) {
                    const int32_t v = oh_warp_interp(t.get(), fx, fy, filter, bd);
                    calls++;
                    CHECK(v >= 0 && v <= M, "%d bit, filter %d, (%d, %d), pattern %d: %d", bd, filter, fx, fy, pattern, v);
                    if (pattern < 2) CHECK(v == t[0], "%d bit, filter %d, (%d, %d) of a constant neighbourhood: %d", bd, filter, fx, fy, v);
                    if ((!fx && !fy) || filter == OH_WARP_NEAREST) CHECK(v == t[5], "%d bit, filter %d without fraction: %d", bd, filter, v);
                }
    }
    CHECK(oh_warp_interp(nullptr, 0, 0, 1, bd) == -1 && oh_warp_interp(t.get(), 64, 0, 1, bd) == -1 && oh_warp_interp(t.get(), 0, -1, 1, bd) == -1 &&
          oh_warp_interp(t.get(), 0, 0, 3, bd) == -1 && oh_warp_interp(t.get(), 0, 0, 1, 11) == -1, "interp refusals");
    return calls;
}

/* positions with every coefficient at either bound, at the corners of the coordinates' domain, in both modes: defined in 64 bits and
 * inside the clamp; then the tile predicate over the same maps */
static long position_group(void)
{
    long calls = 0;
    auto w = heap<OhWarp>(1);
    auto p = heap<int32_t>(2);
    const int xy[] = { 0, 1, 8191, 8192 };
    for (int signs = 0; signs < 256; signs++)
        for (int mode = OH_WARP_AFFINE; mode <= OH_WARP_PERSPECTIVE; mode++) {
            CHECK(oh_warp_identity(w.get()) == OH_OK, "identity");
            w[0].mode = mode;
            const int64_t bound[8] = { B22, B22, B36, B22, B22, B36, B26, B26 };
            for (int k = 0; k < 8; k++) w[0].m[k] = signs >> k & 1 ? -bound[k] : bound[k];
            w[0].m[8] = B36;                                    /* with negative m[6], m[7] the denominator falls below 2^20 far out: refused */
            for (int hs = 0; hs < 2; hs++)
                for (int vs = 0; vs <= hs; vs++)
                    for (int x : xy) for (int y : xy) {
                        const int rc = oh_warp_position(w.get(), hs, vs, x, y, &p[0], &p[1]);
                        calls++;
                        const int64_t D = w[0].m[6] * ((int64_t)x << hs) + w[0].m[7] * ((int64_t)y << vs) + w[0].m[8] + vs * (w[0].m[7] >> 1);
                        const bool low = mode == OH_WARP_PERSPECTIVE && D < (int64_t)1 << 20;
                        CHECK(rc == (low ? OH_E_ARG : OH_OK), "mode %d, signs %d, (%d, %d): %d", mode, signs, x, y, rc);
                        if (!low) CHECK(p[0] >=-(1 << 30) >> hs && p[1] >= (-(1 << 30) - (vs << 15)) >> vs, "below the clamp: %d, %d", p[0], p[1]);
                    }
            w[0].width = 64; w[0].height = 16;
            for (int filter = OH_WARP_NEAREST; filter <= OH_WARP_BICUBIC; filter++) {
                int64_t staged = -1, gathered = -1;
                w[0].filter = filter;
                CHECK(oh_warp_paths(w.get(), 10, 1, 128, 64, &staged, &gathered) == OH_OK && staged + gathered == 8 + 2 * 2, "paths: %lld + %lld",
                      (long long)staged, (long long)gathered);
                calls++;
            }
        }
    CHECK(oh_warp_identity(w.get()) == OH_OK, "identity");
    w[0].mode = OH_WARP_PERSPECTIVE; w[0].m[8] = (int64_t)1 << 20;            /* the smallest denominator */
    w[0].m[2] = B36; w[0].m[5] = -B36;
    CHECK(oh_warp_position(w.get(), 1, 1, 0, 0, &p[0], &p[1]) == OH_OK && p[0] == (int32_t)((((int64_t)1 << 31) - 1) >> 1), "the clamp above: %d", p[0]);
    w[0].m[8]--;
    CHECK(oh_warp_position(w.get(), 0, 0, 0, 0, &p[0], &p[1]) == OH_E_ARG, "a denominator below 2^20");
    CHECK(oh_warp_position(nullptr, 0, 0, 0, 0, &p[0], &p[1]) == OH_E_ARG && oh_warp_position(w.get(), 0, 0, 0, 0, nullptr, &p[1]) == OH_E_ARG, "null pointers");
    return calls;
}

/* the builders at the ends of their arguments: a refusal or a map inside the bounds, never an overflow */
static long builders_group(void)
{
    long calls = 0;
    auto a = heap<OhWarp>(1);
    auto b = heap<OhWarp>(1);
    auto o = heap<OhWarp>(1);
    auto in_bounds = [](const OhWarp &w) {
        auto mag = [](int64_t v) { return v < 0 ? -v : v; };
        return mag(w.m[0]) <= B22 && mag(w.m[1]) <= B22 && mag(w.m[3]) <= B22 && mag(w.m[4]) <= B22 && mag(w.m[2]) <= B36 && mag(w.m[5]) <= B36;
    };
    const int32_t ends[] = { -2147483647 - 1, -1, 0, 1, 2147483647 };
    for (int32_t dx : ends) for (int32_t dy : ends) {
        CHECK(oh_warp_translation(dx, dy, a.get()) == OH_OK && a[0].m[2] == (int64_t)dx * 16384 && a[0].m[5] == (int64_t)dy * 16384, "translation");
        calls++;
    }
    const int64_t lin[] = { -B22, -1, 0, 1, 65536, B22 }, off[] = { -B36, 0, B36 };
    for (int64_t m0 : lin) for (int64_t m1 : lin) for (int64_t m3 : lin) for (int64_t m4 : lin) for (int64_t t : off) {
        (void)oh_warp_identity(a.get());
        a[0].m[0] = m0; a[0].m[1] = m1; a[0].m[2] = t; a[0].m[3] = m3; a[0].m[4] = m4; a[0].m[5] = -t;
        b[0] = a[0];
        b[0].m[2] = -t; b[0].m[0] = m4;
        int rc = oh_warp_then(a.get(), b.get(), o.get());
        CHECK(rc == OH_E_ARG || (rc == OH_OK && in_bounds(o[0])), "then: %d", rc);
        rc = oh_warp_invert(a.get(), o.get());
        CHECK(rc == OH_E_ARG || (rc == OH_OK && in_bounds(o[0])), "invert: %d", rc);
        if (m0 * m4 - m1 * m3 == 0) CHECK(rc == OH_E_ARG, "a singular map was inverted");
        calls += 2;
    }
    const int64_t cs[] = { -B36, 0, B36 };
    for (uint32_t angle : { 0u, 1u, 16383u, 16384u, 32768u, 49152u, 65535u })
        for (int32_t scale : { 1, 65536, 1 << 22 })
            for (int64_t c0 : cs) for (int64_t c1 : cs) {
                const int rc = oh_warp_rotation(angle, c0, c1, c1, c0, scale, o.get());
                CHECK(rc == OH_E_ARG || (rc == OH_OK && in_bounds(o[0]) && o[0].m[0] == o[0].m[4] && o[0].m[1] == -o[0].m[3]), "rotation: %d", rc);
                calls++;
            }
    CHECK(oh_warp_rotation(65536u, 0, 0, 0, 0, 65536, o.get()) == OH_E_ARG && oh_warp_rotation(0, 0, 0, 0, 0, 0, o.get()) == OH_E_ARG &&
          oh_warp_rotation(0, B36 + 1, 0, 0, 0, 65536, o.get()) == OH_E_ARG && oh_warp_rotation(0, 0, 0, 0, 0, 65536, nullptr) == OH_E_ARG, "rotation refusals");
    auto size = heap<int>(2);
    for (uint32_t angle : { 0u, 5461u, 16384u, 40001u, 65535u })
        for (int w : { 1, 2, 1920, 16384 }) for (int h : { 1, 1080, 16384 }) for (int flips = 0; flips < 4; flips++) {
            CHECK(oh_warp_from_sei(flips & 1, flips >> 1, angle, w, h, o.get(), &size[0], &size[1]) == OH_OK && in_bounds(o[0]) && size[0] >= 2 &&
                  size[1] >= 2 && !(size[0] & 1) && !(size[1] & 1) && o[0].width == size[0] && o[0].height == size[1], "from_sei %u %dx%d", angle, w, h);
            calls++;
        }
    CHECK(oh_warp_from_sei(2, 0, 0, 8, 8, o.get(), &size[0], &size[1]) == OH_E_ARG && oh_warp_from_sei(0, 0, 65536u, 8, 8, o.get(), &size[0], &size[1]) == OH_E_ARG &&
          oh_warp_from_sei(0, 0, 0, 0, 8, o.get(), &size[0], &size[1]) == OH_E_ARG && oh_warp_from_sei(0, 0, 0, 8, 8, nullptr, &size[0], &size[1]) == OH_E_ARG &&
          oh_warp_from_sei(0, 0, 0, 8, 8, o.get(), nullptr, &size[1]) == OH_E_ARG, "from_sei refusals");
    return calls;
}

int main(void)
{
    printf("cubic: %ld calls\n", cubic_group());
    for (int bd : { 8, 9, 10, 12 })
        printf("interp, %d bit: %ld calls\n", bd, interp_group(bd));
    printf("positions: %ld calls\n", position_group());
    printf("builders: %ld calls\n", builders_group());
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("warp math ok\n");
    return 0;
}
