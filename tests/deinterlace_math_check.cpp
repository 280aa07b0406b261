/* deinterlace_math_check.cpp — the host-only functions of the fields and deinterlacing services (openhevc_amd/csrc/pics_math.hip:
 * oh_deint_adaptive, oh_field_info) run on the CPU as a program of its own; built together with that file, with AddressSanitizer and
 * UBSan, by tests/test_deinterlace_math_host.py.  The windows are heap blocks of exactly seven elements, so a read one entry too far
 * is a sanitizer report, and the samples are the extremes of every bit depth the engine stores.  Exit status 0: every check held. */
#include <stdio.h>
#include <string.h>
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

/* every window whose fourteen kept samples are 0 or M, with every pattern of 0 and M in the six temporal samples of a few of them */
static long adaptive_group(int bit_depth)
{
    const int32_t M = (1 << bit_depth) - 1;
    auto up = heap<int32_t>(7), dn = heap<int32_t>(7);
    long calls = 0;
    for (int k = 0; k < 1 << 14; k++) {
        for (int i = 0; i < 7; i++) { up[i] = (k >> i & 1) ? M : 0; dn[i] = (k >> (7 + i) & 1) ? M : 0; }
        const int every = k % 257 == 0 ? 1 : 64;                /* all 64 temporal patterns for some windows, one for the others */
        for (int t = every == 1 ? 0 : k & 63; t < 64; t += every) {
            const int32_t v[6] = { (t & 1) ? M : 0, (t & 2) ? M : 0, (t & 4) ? M : 0, (t & 8) ? M : 0, (t & 16) ? M : 0, (t & 32) ? M : 0 };
            const int32_t out = oh_deint_adaptive(up.get(), dn.get(), v[0], v[1], v[2], v[3], v[4], v[5]);
            calls++;
            CHECK(out >= 0 && out <= M, "%d bit, window %#x, temporal %#x: %d", bit_depth, k, t, out);
            if (v[0] == v[1] && v[2] == up[3] && v[4] == up[3] && v[3] == dn[3] && v[5] == dn[3])        /* still: diff is 0, t is a */
                CHECK(out == v[0], "%d bit, window %#x, temporal %#x: still scene gives %d", bit_depth, k, t, out);
        }
    }
    /* a flat window takes the straight direction: the mean of c and e, held within diff of t */
    for (int i = 0; i < 7; i++) { up[i] = M; dn[i] = 0; }
    CHECK(oh_deint_adaptive(up.get(), dn.get(), 0, M, M, 0, M, 0) == M >> 1, "flat window, sp inside");
    CHECK(oh_deint_adaptive(up.get(), dn.get(), M, M, M, 0, M, 0) == M, "flat window, sp below t - diff with diff 0");
    CHECK(oh_deint_adaptive(up.get(), dn.get(), 0, 0, M, 0, M, 0) == 0, "flat window, sp above t + diff with diff 0");
    return calls;
}

static void field_info_group(void)
{
    static const int want[13][5] = { { 0, 0, -1, 0, 1 }, { 1, 0, -1, 0, 1 }, { 2, 0, -1, 0, 1 }, { 0, 0, 1, 0, 1 }, { 0, 0, 0, 0, 1 },
                                     { 0, 0, 1, 1, 1 }, { 0, 0, 0, 1, 1 }, { 0, 0, -1, 0, 2 }, { 0, 0, -1, 0, 3 }, { 1, -1, -1, 0, 1 },
                                     { 2, -1, -1, 0, 1 }, { 1, 1, -1, 0, 1 }, { 2, 1, -1, 0, 1 } };
    auto fi = heap<OhFieldInfo>(1);
    for (int s = 0; s <= 12; s++) {
        memset(fi.get(), 0x5a, sizeof(OhFieldInfo));
        CHECK(oh_field_info(s, fi.get()) == OH_OK, "pic_struct %d", s);
        CHECK(fi[0].kind == want[s][0] && fi[0].pair == want[s][1] && fi[0].top_first == want[s][2] && fi[0].repeat_first == want[s][3] &&
              fi[0].frames == want[s][4], "pic_struct %d: %d %d %d %d %d", s, fi[0].kind, fi[0].pair, fi[0].top_first, fi[0].repeat_first, fi[0].frames);
    }
    const int bad[] = { 13, 14, 15, -1, -2147483647 - 1, 2147483647 };
    for (int s : bad) {
        memset(fi.get(), 0x5a, sizeof(OhFieldInfo));
        CHECK(oh_field_info(s, fi.get()) == OH_E_ARG && fi[0].kind == 0x5a5a5a5a, "pic_struct %d is refused and nothing is written", s);
    }
    CHECK(oh_field_info(3, nullptr) == OH_E_ARG, "a null pointer");
}

int main(void)
{
    for (int bd : { 8, 9, 10, 12, 16 })
        printf("adaptive, %d bit: %ld windows\n", bd, adaptive_group(bd));
    field_info_group();
    printf("field info: 13 values, 6 refused\n");
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("deinterlace math ok\n");
    return 0;
}
