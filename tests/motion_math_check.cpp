/* motion_math_check.cpp — the host-only functions of the motion service (openhevc_amd/csrc/pics_math.hip: oh_motion_qpel,
 * oh_motion_epel, oh_motion_cost, oh_motion_blocks, oh_motion_scale) run on the CPU as a program of its own; built together with that
 * file, with AddressSanitizer and UBSan, by tests/test_motion_math_host.py.  The arrays they read and write are heap blocks of exactly
 * the sizes they may touch (64 and 16 window samples, bwc * bhc vectors, 2 * bw * bh centres), so an access one entry too far is a
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

/* every fraction at every depth on windows of 0, of M, and of both checkerboards: a constant window predicts itself, every result
 * lies in 0 .. M, and a fraction of zero returns the sample at the window's centre */
static long samples_group(int bd)
{
    const int M = (1 << bd) - 1;
    long calls = 0;
    auto q = heap<uint16_t>(64);
    auto c = heap<uint16_t>(16);
    for (int pattern = 0; pattern < 4; pattern++) {
        for (int i = 0; i < 64; i++) q[i] = (uint16_t)(pattern == 0 ? 0 : pattern == 1 ? M : ((i + i / 8 + pattern) & 1) * M);
        for (int i = 0; i < 16; i++) c[i] = (uint16_t)(pattern == 0 ? 0 : pattern == 1 ? M : ((i + i / 4 + pattern) & 1) * M);
        for (int fy = 0; fy < 8; fy++)
            for (int fx = 0; fx < 8; fx++) {
                if (fx < 4 && fy < 4) {
                    const int32_t v = oh_motion_qpel(q.get(), fx, fy, bd);
                    calls++;
                    CHECK(v >= 0 && v <= M, "%d bit, qpel (%d, %d), pattern %d: %d", bd, fx, fy, pattern, v);
                    if (pattern < 2) CHECK(v == q[0], "%d bit, qpel (%d, %d) of a constant window: %d", bd, fx, fy, v);
                    if (!fx && !fy) CHECK(v == q[3 * 8 + 3], "%d bit, qpel without fraction: %d", bd, v);
                }
                const int32_t v = oh_motion_epel(c.get(), fx, fy, bd);
                calls++;
                CHECK(v >= 0 && v <= M, "%d bit, epel (%d, %d), pattern %d: %d", bd, fx, fy, pattern, v);
                if (pattern < 2) CHECK(v == c[0], "%d bit, epel (%d, %d) of a constant window: %d", bd, fx, fy, v);
                if (!fx && !fy) CHECK(v == c[1 * 4 + 1], "%d bit, epel without fraction: %d", bd, v);
            }
    }
    CHECK(oh_motion_qpel(q.get(), 4, 0, bd) == -1 && oh_motion_qpel(q.get(), 0, -1, bd) == -1 && oh_motion_qpel(nullptr, 0, 0, bd) == -1, "qpel refusals");
    CHECK(oh_motion_epel(c.get(), 8, 0, bd) == -1 && oh_motion_epel(c.get(), 0, -1, bd) == -1 && oh_motion_epel(nullptr, 0, 0, bd) == -1, "epel refusals");
    CHECK(oh_motion_qpel(q.get(), 0, 0, 11) == -1 && oh_motion_epel(c.get(), 0, 0, 13) == -1, "another depth");
    return calls;
}

/* the cost at the corners of every argument's domain, and beyond: defined in 64 bits */
static long cost_group(void)
{
    long calls = 0;
    const int big[] = { -2147483647 - 1, -32768, -1, 0, 1, 32767, 2147483647 };
    const uint32_t sads[] = { 0, 1, 256 * 4095, 0xFFFFFFFFu };
    for (uint32_t sad : sads) for (int mvx : big) for (int mvy : big) for (int cx : big) for (int lambda : { 0, 1, 4096 }) {
        const uint64_t v = oh_motion_cost(sad, mvx, mvy, cx, cx / -2, lambda);
        calls++;
        if (!lambda) CHECK(v == sad, "lambda 0: %llu", (unsigned long long)v);
        else CHECK(v >= sad, "cost below the SAD: %llu", (unsigned long long)v);
    }
    CHECK(oh_motion_cost(10, 4 * 5 + 3, 4 * -2 - 2, 5, -2, 7) == 10 + ((7 * 5) >> 2), "a plain case");
    return calls;
}

/* grids of every size around the block sizes, fields of exactly bwc * bhc vectors and centres of exactly 2 * bw * bh values */
static long grids_group(void)
{
    long calls = 0;
    for (int block : { 8, 16 })
        for (int w : { 1, 7, 8, 9, 16, 17, 16384 })
            for (int h : { 1, 8, 15, 16, 2160 }) {
                int bw = -1, bh = -1;
                CHECK(oh_motion_blocks(w, h, block, &bw, &bh) == OH_OK && bw == (w + block - 1) / block && bh == (h + block - 1) / block, "blocks of %dx%d", w, h);
                calls++;
            }
    int bw = -5, bh = -5;
    CHECK(oh_motion_blocks(0, 8, 8, &bw, &bh) == OH_E_ARG && oh_motion_blocks(8, 8, 12, &bw, &bh) == OH_E_ARG && oh_motion_blocks(8, 8, 8, nullptr, &bh) == OH_E_ARG &&
          oh_motion_blocks(8, 8, 8, &bw, nullptr) == OH_E_ARG && bw == -5 && bh == -5, "blocks refusals");
    const int16_t ext[] = { -32768, -16385, -16384, -3, -2, -1, 0, 1, 2, 16383, 16384, 32767 };
    for (int s : { 1, 2, 4, 8 })
        for (int bc : { 8, 16 })
            for (int bf : { 8, 16 })
                for (int bwc : { 1, 3 })
                    for (int bhc : { 1, 2 })
                        for (int gw : { 1, 2, 13 })
                            for (int gh : { 1, 5 }) {
                                auto coarse = heap<OhMotionVector>((size_t)bwc * bhc);
                                auto centres = heap<int16_t>((size_t)2 * gw * gh);
                                for (int i = 0; i < bwc * bhc; i++) {
                                    coarse[i].x = ext[(i + s + gw) % 12]; coarse[i].y = ext[(i * 5 + bc + gh) % 12];
                                    coarse[i].sad = coarse[i].sad_centre = 0xFFFFFFFFu;
                                }
                                CHECK(oh_motion_scale(coarse.get(), bwc, bhc, bc, s, gw, gh, bf, centres.get()) == OH_OK, "scale %d", s);
                                calls++;
                                for (int by = 0; by < gh; by++)
                                    for (int bx = 0; bx < gw; bx++) {
                                        const OhMotionVector &v = coarse[std::min(by * bf / (s * bc), bhc - 1) * bwc + std::min(bx * bf / (s * bc), bwc - 1)];
                                        const int wx = std::min(std::max((s * v.x + 2) >> 2, -(int)OH_MOTION_MAX_CENTRE), (int)OH_MOTION_MAX_CENTRE);
                                        const int wy = std::min(std::max((s * v.y + 2) >> 2, -(int)OH_MOTION_MAX_CENTRE), (int)OH_MOTION_MAX_CENTRE);
                                        CHECK(centres[2 * (by * gw + bx)] == wx && centres[2 * (by * gw + bx) + 1] == wy, "scale %d, block (%d, %d)", s, bx, by);
                                    }
                            }
    auto one = heap<OhMotionVector>(1);
    auto out = heap<int16_t>(2);
    memset(one.get(), 0, sizeof(OhMotionVector));
    out[0] = out[1] = -7;
    for (int s : { 0, 3, 5, 16, -1 })
        CHECK(oh_motion_scale(one.get(), 1, 1, 8, s, 1, 1, 8, out.get()) == OH_E_ARG, "s %d", s);
    CHECK(oh_motion_scale(nullptr, 1, 1, 8, 1, 1, 1, 8, out.get()) == OH_E_ARG && oh_motion_scale(one.get(), 1, 1, 8, 1, 1, 1, 8, nullptr) == OH_E_ARG, "null pointers");
    CHECK(oh_motion_scale(one.get(), 0, 1, 8, 1, 1, 1, 8, out.get()) == OH_E_ARG && oh_motion_scale(one.get(), 1, 1, 8, 1, 1, 0, 8, out.get()) == OH_E_ARG, "sizes below 1");
    CHECK(oh_motion_scale(one.get(), 1, 1, 4, 1, 1, 1, 8, out.get()) == OH_E_ARG && oh_motion_scale(one.get(), 1, 1, 8, 1, 1, 1, 32, out.get()) == OH_E_ARG, "block sizes");
    CHECK(out[0] == -7 && out[1] == -7, "a refused call wrote");
    return calls;
}

int main(void)
{
    for (int bd : { 8, 9, 10, 12 })
        printf("samples, %d bit: %ld calls\n", bd, samples_group(bd));
    printf("costs: %ld calls\n", cost_group());
    printf("grids: %ld calls\n", grids_group());
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("motion math ok\n");
    return 0;
}
