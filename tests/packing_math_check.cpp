/* packing_math_check.cpp — the host-only functions of the frame packing service (openhevc_amd/csrc/pics_math.hip: oh_packing_from_sei,
 * _view_size, _sample, _pack_sample, _views) run on the CPU as a program of its own; built together with that file, with
 * AddressSanitizer and UBSan, by tests/test_packing_math_host.py.  The planes they read are heap blocks of exactly their sizes, so a tap
 * across the edge of the packed plane, or a lattice position one sample too far, is a sanitizer report; the samples are the extremes of
 * their depth, where the sums are largest.  Exit status 0: every check held. */
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

static OhPicParams params(int w, int h, int bd, int cf)
{
    OhPicParams p;
    memset(&p, 0, sizeof(p));
    p.width = w; p.height = h; p.bit_depth = bd; p.chroma_format_idc = cf;
    p.log2_ctb_size = 4; p.log2_min_cb_size = 3; p.log2_min_tb_size = 2; p.log2_min_pu_size = 2;
    return p;
}

static OhPacking packing(int arr, int quincunx, int f0, int f1, int g0, int g1)
{
    OhPacking pk;
    memset(&pk, 0, sizeof(pk));
    pk.arrangement = arr; pk.quincunx = quincunx; pk.flip[0] = f0; pk.flip[1] = f1;
    pk.grid_x[0] = pk.grid_y[0] = g0; pk.grid_x[1] = pk.grid_y[1] = g1;
    return pk;
}

/* every sample of every plane of both views, half and full size, from packed planes in exact heap blocks whose samples alternate
 * between 0 and the maximum, so that a sum of the taps is as large and as small as it gets */
static long sample_group(void)
{
    long calls = 0;
    const int sizes[3][2] = { { 8, 8 }, { 24, 16 }, { 40, 24 } };
    for (const auto &sz : sizes)
        for (int bd : { 8, 12 })
            for (int cf = 0; cf <= 3; cf++)
                for (int arr : { OH_PACK_SIDE_BY_SIDE, OH_PACK_TOP_BOTTOM })
                    for (int mode = 0; mode < 3; mode++)              /* 0 plain, 1 flipped with odd grid positions, 2 quincunx */
                    {
                        const OhPicParams p = params(sz[0], sz[1], bd, cf);
                        const OhPacking pk = packing(arr, mode == 2, mode == 1, mode != 1, mode == 1 ? 15 : 0, mode == 1 ? 7 : 8);
                        const int maxv = (1 << bd) - 1;
                        for (int plane = 0; plane < (cf ? 3 : 1); plane++) {
                            const int hs = plane && (cf == 1 || cf == 2), vs = plane && cf == 1, pw = sz[0] >> hs, ph = sz[1] >> vs;
                            auto s8 = heap<uint8_t>((size_t)pw * ph);
                            auto s16 = heap<uint16_t>((size_t)pw * ph);
                            for (int i = 0; i < pw * ph; i++) {
                                const int v = ((i % pw) + (i / pw) / 2) & 1 ? maxv : (i % 7 == 0 ? 1 : 0);
                                s8[i] = (uint8_t)v; s16[i] = (uint16_t)v;
                            }
                            const void *samples = bd == 8 ? (const void *)s8.get() : (const void *)s16.get();
                            for (int full = 0; full < 2; full++) {
                                OhPicParams vp;
                                CHECK(oh_packing_view_size(&pk, &p, full, &vp) == OH_OK, "view size");
                                const int vw = vp.width >> hs, vh = vp.height >> vs;
                                for (int view = 0; view < 2; view++)
                                    for (int y = 0; y < vh; y++)
                                        for (int x = 0; x < vw; x++, calls++) {
                                            int32_t out = -1;
                                            const int rc = oh_packing_sample(&pk, &p, full, view, plane, x, y, samples, pw, &out);
                                            CHECK(rc == OH_OK && out >= 0 && out <= maxv, "sample %d: %d", rc, out);
                                        }
                                int32_t out = -1;
                                CHECK(oh_packing_sample(&pk, &p, full, 0, plane, vw, 0, samples, pw, &out) == OH_E_ARG && out == -1, "x outside");
                                CHECK(oh_packing_sample(&pk, &p, full, 0, plane, 0, vh, samples, pw, &out) == OH_E_ARG && out == -1, "y outside");
                            }
                        }
                    }
    printf("%ld samples of views\n", calls);
    return calls;
}

/* packing: every sample of the packed planes from views in exact heap blocks, and unpacking it again gives the views back */
static long pack_group(void)
{
    long calls = 0;
    for (int bd : { 8, 10 })
        for (int cf : { 0, 1, 2, 3 })
            for (int arr : { OH_PACK_SIDE_BY_SIDE, OH_PACK_TOP_BOTTOM })
                for (int quincunx = 0; quincunx < 2; quincunx++)
                    for (int flips = 0; flips < 4; flips++) {
                        const OhPicParams p = params(16, 8, bd, cf);
                        const OhPacking pk = packing(arr, quincunx, flips & 1, flips >> 1, 0, 0);
                        for (int plane = 0; plane < (cf ? 3 : 1); plane++) {
                            const int hs = plane && (cf == 1 || cf == 2), vs = plane && cf == 1, pw = 16 >> hs, ph = 8 >> vs;
                            const int sbs = arr == OH_PACK_SIDE_BY_SIDE;
                            const int vw = quincunx ? pw : sbs ? pw / 2 : pw, vh = quincunx ? ph : sbs ? ph : ph / 2;
                            auto v0 = heap<uint16_t>((size_t)vw * vh), v1 = heap<uint16_t>((size_t)vw * vh), pk16 = heap<uint16_t>((size_t)pw * ph);
                            auto b0 = heap<uint8_t>((size_t)vw * vh), b1 = heap<uint8_t>((size_t)vw * vh), pk8 = heap<uint8_t>((size_t)pw * ph);
                            for (int i = 0; i < vw * vh; i++) {
                                v0[i] = (uint16_t)(1 + i); v1[i] = (uint16_t)(129 + i);
                                b0[i] = (uint8_t)v0[i]; b1[i] = (uint8_t)v1[i];
                            }
                            const void *a0 = bd == 8 ? (const void *)b0.get() : (const void *)v0.get();
                            const void *a1 = bd == 8 ? (const void *)b1.get() : (const void *)v1.get();
                            for (int y = 0; y < ph; y++)
                                for (int x = 0; x < pw; x++, calls++) {
                                    int32_t out = -1;
                                    CHECK(oh_packing_pack_sample(&pk, &p, plane, x, y, a0, a1, vw, &out) == OH_OK, "pack sample");
                                    pk16[y * pw + x] = (uint16_t)out; pk8[y * pw + x] = (uint8_t)out;
                                }
                            const void *ps = bd == 8 ? (const void *)pk8.get() : (const void *)pk16.get();
                            int bad = 0;
                            for (int view = 0; view < 2; view++)
                                for (int y = 0; y < vh; y++)
                                    for (int x = 0; x < vw; x++) {
                                        int32_t out = -1;
                                        CHECK(oh_packing_sample(&pk, &p, quincunx, view, plane, x, y, ps, pw, &out) == OH_OK, "sample");
                                        const int on = !quincunx || !((x ^ y ^ view) & 1);
                                        const int want = view ? (bd == 8 ? b1[y * vw + x] : v1[y * vw + x]) : (bd == 8 ? b0[y * vw + x] : v0[y * vw + x]);
                                        bad += on && out != want;
                                    }
                            CHECK(!bad, "arrangement %d quincunx %d flips %d plane %d: %d samples differ", arr, quincunx, flips, plane, bad);
                            int32_t out = -1;
                            CHECK(oh_packing_pack_sample(&pk, &p, plane, pw, 0, a0, a1, vw, &out) == OH_E_ARG, "x outside");
                        }
                    }
    printf("%ld samples of packed pictures, unpacked again\n", calls);
    return calls;
}

static long refusal_group(void)
{
    long calls = 0;
    OhFramePackingSei s;
    OhPacking pk, before;
    memset(&pk, 0x5A, sizeof(pk));
    before = pk;
    for (int type = 0; type < 128; type++)
        for (int fv = 0; fv < 2; fv++, calls++) {
            memset(&s, 0, sizeof(s));
            s.present = 1; s.arrangement_type = type; s.field_views = fv; s.spatial_flipping = 1; s.frame0_flipped = type & 1;
            s.frame1_grid_position_x = 8; s.content_interpretation_type = 2;
            const int ok = (type == 3 || type == 4) && !fv, rc = oh_packing_from_sei(&s, &pk);
            CHECK(rc == (ok ? OH_OK : OH_E_UNSUPPORTED), "type %d field views %d: %d", type, fv, rc);
            CHECK((strlen(oh_packing_unsupported(&s)) == 0) == ok, "type %d: the reason", type);
            if (ok) {
                CHECK(pk.arrangement == type && pk.flip[0] == (type & 1) && pk.flip[1] == !(type & 1) && pk.grid_x[1] == 8 && !pk.quincunx &&
                      pk.content_interpretation == 2, "type %d", type);
                int l = -1, r = -1;
                CHECK(oh_packing_views(&pk, &l, &r) == 1 && l == 1 && r == 0, "views");
                pk = before;
            } else
                CHECK(!memcmp(&pk, &before, sizeof(pk)), "type %d: out was written", type);
        }
    memset(&s, 0, sizeof(s));
    s.present = 1; s.cancel = 1;
    CHECK(oh_packing_from_sei(&s, &pk) == OH_E_ARG && !memcmp(&pk, &before, sizeof(pk)), "cancelled");
    s.present = 0; s.cancel = 0; s.arrangement_type = 3;
    CHECK(oh_packing_from_sei(&s, &pk) == OH_E_ARG, "absent");
    s.present = 1; s.frame0_grid_position_y = 16;
    CHECK(oh_packing_from_sei(&s, &pk) == OH_E_ARG && !memcmp(&pk, &before, sizeof(pk)), "grid position 16");
    CHECK(oh_packing_from_sei(nullptr, &pk) == OH_E_ARG && oh_packing_from_sei(&s, nullptr) == OH_E_ARG, "null");
    /* sizes: each half a whole number of chroma samples */
    OhPicParams vp;
    for (int cf = 0; cf <= 3; cf++) {
        const int hs = cf == 1 || cf == 2, vs = cf == 1;
        for (int w = 8; w <= 32; w += 8, calls++) {
            OhPicParams p = params(w, 8, 8, cf);
            p.width = w - 6;                                   /* the call checks the number alone */
            const OhPacking sbs = packing(OH_PACK_SIDE_BY_SIDE, 0, 0, 0, 0, 0), tb = packing(OH_PACK_TOP_BOTTOM, 0, 0, 0, 0, 0);
            CHECK(oh_packing_view_size(&sbs, &p, 0, &vp) == ((w - 6) % (2 << hs) ? OH_E_ARG : OH_OK), "width %d format %d", w - 6, cf);
            p.width = w; p.height = 6;
            CHECK(oh_packing_view_size(&tb, &p, 0, &vp) == (6 % (2 << vs) ? OH_E_ARG : OH_OK), "height 6 format %d", cf);
        }
    }
    const OhPicParams p = params(80, 24, 10, 1);
    OhPacking bad = packing(5, 0, 0, 0, 0, 0);
    CHECK(oh_packing_view_size(&bad, &p, 0, &vp) == OH_E_ARG, "arrangement 5");
    bad = packing(3, 2, 0, 0, 0, 0);
    CHECK(oh_packing_view_size(&bad, &p, 0, &vp) == OH_E_ARG, "quincunx 2");
    bad = packing(3, 0, 0, -1, 0, 0);
    CHECK(oh_packing_view_size(&bad, &p, 0, &vp) == OH_E_ARG, "flip -1");
    bad = packing(4, 0, 0, 0, 0, 16);
    CHECK(oh_packing_view_size(&bad, &p, 0, &vp) == OH_E_ARG, "grid 16");
    const OhPacking ok = packing(4, 0, 0, 0, 0, 0);
    CHECK(oh_packing_view_size(&ok, &p, 2, &vp) == OH_E_ARG && oh_packing_view_size(&ok, &p, 0, nullptr) == OH_E_ARG, "full 2, null");
    CHECK(oh_packing_view_size(&ok, &p, 0, &vp) == OH_OK && vp.width == 80 && vp.height == 16 && vp.bit_depth == 10, "80x24 top-bottom: 80x12 in 80x16");
    CHECK(oh_packing_view_size(&ok, &p, 1, &vp) == OH_OK && vp.width == 80 && vp.height == 24, "full");
    int l = 5, r = 5;
    CHECK(oh_packing_views(&ok, &l, &r) == 0 && l == 5 && r == 5, "interpretation 0");
    printf("%ld refusals and sizes\n", calls);
    return calls;
}

int main(void)
{
    sample_group();
    pack_group();
    refusal_group();
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("packing math ok\n");
    return 0;
}
