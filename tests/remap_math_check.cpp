/* remap_math_check.cpp — the host-only functions of the colour remapping service (openhevc_amd/csrc/pics_math.hip: oh_remap_curve,
 * _sample, _from_sei, _luts) run on the CPU as a program of its own; built together with that file, with AddressSanitizer and UBSan, by
 * tests/test_remap_math_host.py.  The arrays they read and write are heap blocks of exactly the sizes they may touch (2^bits entries of
 * a table, 33 pivots, 6 x 4096 and 3 x 4096 entries, one OhColourRemapSei), so an access one entry too far is a sanitizer report, and
 * the values are the extremes of their domains, where a signed overflow would be one too.  Exit status 0: every check held. */
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

static const int DEPTHS[4] = { 8, 9, 10, 12 };

/* the definition, point by point, in 64-bit integers */
static int64_t curve_at(int bi, int bo, int n, const uint16_t *x, const uint16_t *y, int v)
{
    int64_t px[35], py[35];
    int np = 0;
    if (!n || x[0] > 0) { px[np] = 0; py[np++] = 0; }
    for (int k = 0; k < n; k++) { px[np] = x[k]; py[np++] = y[k]; }
    if (px[np - 1] < (1 << bi) - 1) { px[np] = (1 << bi) - 1; py[np++] = (1 << bo) - 1; }
    for (int k = 0; k + 1 < np; k++)
        if (v >= px[k] && v <= px[k + 1]) {
            const int64_t dx = px[k + 1] - px[k], t = v - px[k];
            return (py[k] * (dx - t) + py[k + 1] * t + (dx >> 1)) / dx;
        }
    return -1;
}

static long check_curve(int bi, int bo, int n, const uint16_t *x, const uint16_t *y, const char *what)
{
    auto cx = heap<uint16_t>(n ? n : 1), cy = heap<uint16_t>(n ? n : 1);
    if (n) { memcpy(cx.get(), x, n * sizeof(uint16_t)); memcpy(cy.get(), y, n * sizeof(uint16_t)); }
    auto out = heap<uint16_t>((size_t)1 << bi);
    CHECK(oh_remap_curve(bi, bo, n, n ? cx.get() : nullptr, n ? cy.get() : nullptr, out.get()) == OH_OK, "%s at %d -> %d", what, bi, bo);
    int bad = 0;
    for (int v = 0; v < 1 << bi; v++)
        bad += out[v] != curve_at(bi, bo, n, x, y, v);
    CHECK(!bad, "%s at %d -> %d: %d entries differ", what, bi, bo, bad);
    return 1;
}

static long curve_group(void)
{
    long calls = 0;
    for (int bi : DEPTHS)
        for (int bo : DEPTHS) {
            const uint16_t Mi = (uint16_t)((1 << bi) - 1), Mo = (uint16_t)((1 << bo) - 1);
            uint16_t x[33], y[33];
            calls += check_curve(bi, bo, 0, nullptr, nullptr, "no pivots");
            for (int k = 0; k < 33; k++) { x[k] = (uint16_t)((int64_t)Mi * k / 32); y[k] = k & 1 ? Mo : 0; }      /* pivots at 0 and Mi, full swings */
            calls += check_curve(bi, bo, 33, x, y, "33 pivots from 0 to Mi");
            for (int k = 0; k < 33; k++) { x[k] = (uint16_t)(Mi - 32 + k); y[k] = (uint16_t)(Mo - k); }            /* adjacent coded values at the top */
            calls += check_curve(bi, bo, 33, x, y, "33 adjacent pivots");
            for (int k = 0; k < 33; k++) { x[k] = (uint16_t)(1 + k); y[k] = Mo; }
            calls += check_curve(bi, bo, 33, x, y, "33 pivots from 1, (0, 0) and (Mi, Mo) added");
            x[0] = Mi / 2; y[0] = Mo;
            calls += check_curve(bi, bo, 1, x, y, "one pivot in the middle");
            x[0] = 0; y[0] = Mo; x[1] = Mi; y[1] = 0;
            calls += check_curve(bi, bo, 2, x, y, "descending");
            x[0] = 0; y[0] = Mo;
            calls += check_curve(bi, bo, 1, x, y, "one pivot at 0");
            x[0] = Mi; y[0] = 0;
            calls += check_curve(bi, bo, 1, x, y, "one pivot at Mi");
            for (int k = 0; k < 5; k++) { x[k] = (uint16_t)(Mi / 8 * (k + 1)); y[k] = (uint16_t)(Mo / 4 * (4 - k)); }
            calls += check_curve(bi, bo, 5, x, y, "descending targets");
        }
    return calls;
}

static long curve_refusals(void)
{
    long calls = 0;
    auto out = heap<uint16_t>(4096);
    auto x = heap<uint16_t>(34), y = heap<uint16_t>(34);
    for (int k = 0; k < 34; k++) { x[k] = (uint16_t)k; y[k] = (uint16_t)k; }
    memset(out.get(), 0xAB, 4096 * sizeof(uint16_t));
#define REFUSED(call, what)                                                                                   \
    do {                                                                                                      \
        CHECK((call) == OH_E_ARG, what);                                                                      \
        for (int v = 0; v < 4096; v++) if (out[v] != 0xABAB) { CHECK(false, what ": out was written"); break; }  \
        calls++;                                                                                              \
    } while (0)
    REFUSED(oh_remap_curve(8, 8, 2, x.get(), y.get(), nullptr), "null out");
    REFUSED(oh_remap_curve(8, 8, 2, nullptr, y.get(), out.get()), "null coded");
    REFUSED(oh_remap_curve(8, 8, 2, x.get(), nullptr, out.get()), "null target");
    for (int bd : { 0, 7, 11, 13, 16, -8 }) {
        REFUSED(oh_remap_curve(bd, 8, 2, x.get(), y.get(), out.get()), "input depth");
        REFUSED(oh_remap_curve(8, bd, 2, x.get(), y.get(), out.get()), "output depth");
    }
    REFUSED(oh_remap_curve(8, 8, -1, x.get(), y.get(), out.get()), "n -1");
    REFUSED(oh_remap_curve(8, 8, 34, x.get(), y.get(), out.get()), "n 34");
    x[5] = 4;
    REFUSED(oh_remap_curve(8, 8, 33, x.get(), y.get(), out.get()), "coded values that fall");
    x[5] = 6;
    REFUSED(oh_remap_curve(8, 8, 33, x.get(), y.get(), out.get()), "coded values that repeat");
    x[5] = 5; x[32] = 256;
    REFUSED(oh_remap_curve(8, 12, 33, x.get(), y.get(), out.get()), "a coded value above Mi");
    x[32] = 32; y[0] = 256;
    REFUSED(oh_remap_curve(12, 8, 33, x.get(), y.get(), out.get()), "a target above Mo");
    y[0] = 0; y[32] = 4096;
    REFUSED(oh_remap_curve(12, 12, 33, x.get(), y.get(), out.get()), "the last target above Mo");
    y[32] = 4095;
    CHECK(oh_remap_curve(12, 12, 33, x.get(), y.get(), out.get()) == OH_OK && out[32] == 4095 && out[4095] == 4095, "the mended pivots");
    return calls + 1;
}

struct Tables {
    std::unique_ptr<uint16_t[]> t[6];
    OhRemap r;
    Tables(int bi, int bo, uint16_t pre_value, uint16_t post_value)
    {
        memset(&r, 0, sizeof(r));
        r.in_bit_depth = bi; r.out_bit_depth = bo;
        for (int k = 0; k < 6; k++) {
            const size_t n = (size_t)1 << (k < 3 ? bi : bo);
            t[k] = heap<uint16_t>(n);
            for (size_t v = 0; v < n; v++) t[k][v] = k < 3 ? pre_value : post_value;
            (k < 3 ? r.pre[k] : r.post[k - 3]) = t[k].get();
        }
    }
};

/* all-maximal coefficients on all-maximal samples, d = 0 and 15, both signs; 12 -> 8 and 8 -> 12; the refusals */
static long sample_group(void)
{
    long calls = 0;
    for (int bi : DEPTHS)
        for (int bo : DEPTHS) {
            const uint16_t Mi = (uint16_t)((1 << bi) - 1), Mo = (uint16_t)((1 << bo) - 1);
            for (int d : { 0, 1, 15 })
                for (int sign : { 1, -1 }) {
                    Tables tb(bi, bo, Mo, 0);                   /* every pre entry Mo; post: the identity, so that out = m */
                    for (int k = 3; k < 6; k++)
                        for (int v = 0; v <= Mo; v++) tb.t[k][v] = (uint16_t)v;
                    for (int c = 0; c < 3; c++)
                        for (int i = 0; i < 3; i++) tb.r.coeff[c][i] = sign > 0 ? 32767 : -32768;
                    tb.r.log2_denom = d;
                    const uint16_t s[3] = { Mi, Mi, Mi };
                    uint16_t o[3] = { 7, 7, 7 };
                    CHECK(oh_remap_sample(&tb.r, s, o) == 1, "%d -> %d, d %d, sign %d", bi, bo, d, sign);
                    const int64_t sum = 3 * (int64_t)(sign > 0 ? 32767 : -32768) * Mo + (d ? (int64_t)1 << (d - 1) : 0);
                    int64_t m = sum >= 0 ? sum >> d : -((-sum + ((int64_t)1 << d) - 1) >> d);
                    m = m < 0 ? 0 : m > Mo ? Mo : m;
                    CHECK(o[0] == m && o[1] == m && o[2] == m, "%d -> %d, d %d, sign %d: %d, want %lld", bi, bo, d, sign, o[0], (long long)m);
                    /* a sample above Mi is looked up by its low bits: no read leaves the tables of exactly 2^bi entries */
                    const uint16_t above[3] = { 0xFFFF, (uint16_t)(Mi + 1), 0x8000 };
                    CHECK(oh_remap_sample(&tb.r, above, o) == 1 && o[0] == m, "samples above Mi");
                    calls += 2;
                }
        }
    /* the refusals: what oh_pics_colour_remap would refuse */
    Tables ok(10, 8, 255, 255);
    ok.r.coeff[0][0] = ok.r.coeff[1][1] = ok.r.coeff[2][2] = 1;
    const uint16_t s[3] = { 1, 2, 3 };
    uint16_t o[3] = { 9, 9, 9 };
    CHECK(oh_remap_sample(&ok.r, s, o) == 1 && o[0] == 255, "the remap that the refusals start from");
    CHECK(oh_remap_sample(nullptr, s, o) == 0 && oh_remap_sample(&ok.r, nullptr, o) == 0 && oh_remap_sample(&ok.r, s, nullptr) == 0, "null pointers");
    calls += 4;
#define SAMPLE_REFUSED(change, restore, what)                                      \
    do {                                                                           \
        change;                                                                    \
        o[0] = o[1] = o[2] = 9;                                                    \
        CHECK(oh_remap_sample(&ok.r, s, o) == 0 && o[0] == 9 && o[2] == 9, what);   \
        restore;                                                                   \
        calls++;                                                                   \
    } while (0)
    SAMPLE_REFUSED(ok.r.in_bit_depth = 11, ok.r.in_bit_depth = 10, "input depth 11");
    SAMPLE_REFUSED(ok.r.out_bit_depth = 16, ok.r.out_bit_depth = 8, "output depth 16");
    SAMPLE_REFUSED(ok.r.log2_denom = 16, ok.r.log2_denom = 0, "log2_denom 16");
    SAMPLE_REFUSED(ok.r.log2_denom = -1, ok.r.log2_denom = 0, "log2_denom -1");
    SAMPLE_REFUSED(ok.r.coeff[2][1] = 32768, ok.r.coeff[2][1] = 0, "coefficient 32768");
    SAMPLE_REFUSED(ok.r.coeff[0][2] = -32769, ok.r.coeff[0][2] = 0, "coefficient -32769");
    SAMPLE_REFUSED(ok.r.pre[1] = nullptr, ok.r.pre[1] = ok.t[1].get(), "null pre table");
    SAMPLE_REFUSED(ok.r.post[2] = nullptr, ok.r.post[2] = ok.t[5].get(), "null post table");
    SAMPLE_REFUSED(ok.t[2][1023] = 256, ok.t[2][1023] = 255, "pre entry above Mo");
    SAMPLE_REFUSED(ok.t[3][255] = 256, ok.t[3][255] = 255, "post entry above Mo");
    CHECK(oh_remap_sample(&ok.r, s, o) == 1, "restored");
    return calls + 1;
}

static long sei_and_luts_group(void)
{
    long calls = 0;
    auto sei = std::unique_ptr<OhColourRemapSei>(new OhColourRemapSei);
    auto tables = std::unique_ptr<uint16_t[][4096]>(new uint16_t[6][4096]);
    auto lut = std::unique_ptr<uint16_t[][4096]>(new uint16_t[3][4096]);
    OhRemap r;
    for (int bi : DEPTHS)
        for (int bo : DEPTHS) {
            const int Mi = (1 << bi) - 1, Mo = (1 << bo) - 1;
            memset(sei.get(), 0, sizeof(*sei));
            sei->present = 1; sei->input_bit_depth = bi; sei->output_bit_depth = bo;
            for (int c = 0; c < 3; c++) {
                sei->pre_lut_num_val_minus1[c] = c == 1 ? 0 : 32;
                sei->post_lut_num_val_minus1[c] = c == 2 ? 0 : 32;
                for (int k = 0; k < 33; k++) {
                    sei->pre_lut_coded_value[c][k] = (uint16_t)((int64_t)Mi * k / 32); sei->pre_lut_target_value[c][k] = (uint16_t)(k & 1 ? 0 : Mo);
                    sei->post_lut_coded_value[c][k] = (uint16_t)((int64_t)Mo * k / 32); sei->post_lut_target_value[c][k] = (uint16_t)(Mo - Mo * k / 32);
                }
            }
            /* without a matrix: the identity at d = 0 */
            CHECK(oh_remap_from_sei(sei.get(), tables.get(), &r) == OH_OK, "%d -> %d", bi, bo);
            CHECK(r.in_bit_depth == bi && r.out_bit_depth == bo && r.log2_denom == 0 && r.coeff[0][0] == 1 && r.coeff[1][1] == 1 && r.coeff[2][2] == 1 &&
                  !r.coeff[0][1] && !r.coeff[2][0] && r.pre[2] == tables[2] && r.post[0] == tables[3], "what from_sei fills in");
            CHECK(tables[0][0] == Mo && tables[0][Mi] == Mo && tables[1][Mi] == Mo && tables[1][0] == 0 && tables[3][0] == Mo && tables[3][Mo] == 0 &&
                  tables[5][Mo] == Mo, "the ends of the curves");
            CHECK(oh_remap_luts(&r, lut.get()) == OH_OK && lut[1][Mi] == 0 && lut[2][0] == Mo, "luts of the identity");
            /* with the extreme diagonal matrix */
            sei->matrix_present = 1; sei->log2_matrix_denom = 15;
            sei->coeffs[0][0] = 32767; sei->coeffs[1][1] = -32768; sei->coeffs[2][2] = 32767;
            CHECK(oh_remap_from_sei(sei.get(), tables.get(), &r) == OH_OK && r.log2_denom == 15 && r.coeff[1][1] == -32768, "with a matrix");
            CHECK(oh_remap_luts(&r, lut.get()) == OH_OK && lut[1][Mi] == tables[4][0], "luts of a diagonal matrix: a negative product is clipped to 0");
            sei->coeffs[2][0] = 1;
            CHECK(oh_remap_from_sei(sei.get(), tables.get(), &r) == OH_OK, "a full matrix");
            memset(lut.get(), 0xCD, sizeof(uint16_t) * 3 * 4096);
            CHECK(oh_remap_luts(&r, lut.get()) == OH_E_UNSUPPORTED && lut[0][0] == 0xCDCD && lut[2][4095] == 0xCDCD, "luts of a full matrix");
            calls += 7;
        }
    /* the refusals of from_sei leave tables and out untouched */
    memset(tables.get(), 0xEE, sizeof(uint16_t) * 6 * 4096);
    memset(&r, 0x11, sizeof(r));
    OhRemap r0 = r;
#define SEI_REFUSED(change, restore, code, what)                                                                              \
    do {                                                                                                                      \
        change;                                                                                                               \
        CHECK(oh_remap_from_sei(sei.get(), tables.get(), &r) == code && tables[0][0] == 0xEEEE && tables[5][4095] == 0xEEEE && \
              !memcmp(&r, &r0, sizeof(r)), what);                                                                              \
        restore;                                                                                                              \
        calls++;                                                                                                              \
    } while (0)
    SEI_REFUSED(sei->present = 0, sei->present = 1, OH_E_ARG, "absent");
    SEI_REFUSED(sei->cancel = 1, sei->cancel = 0, OH_E_ARG, "cancelled");
    SEI_REFUSED(sei->input_bit_depth = 16, sei->input_bit_depth = 12, OH_E_UNSUPPORTED, "input depth 16");
    SEI_REFUSED(sei->output_bit_depth = 11, sei->output_bit_depth = 12, OH_E_UNSUPPORTED, "output depth 11");
    SEI_REFUSED(sei->pre_lut_coded_value[0][7] = 0, sei->pre_lut_coded_value[0][7] = (uint16_t)(4095 * 7 / 32), OH_E_ARG, "pivots that fall");
    SEI_REFUSED(sei->post_lut_target_value[1][32] = 4096, sei->post_lut_target_value[1][32] = 0, OH_E_ARG, "a target above Mo");
    SEI_REFUSED(sei->pre_lut_num_val_minus1[2] = 33, sei->pre_lut_num_val_minus1[2] = 32, OH_E_ARG, "34 pivots");
    SEI_REFUSED(sei->post_lut_num_val_minus1[0] = -1, sei->post_lut_num_val_minus1[0] = 32, OH_E_ARG, "-1 pivots");
    CHECK(oh_remap_from_sei(nullptr, tables.get(), &r) == OH_E_ARG && oh_remap_from_sei(sei.get(), nullptr, &r) == OH_E_ARG &&
          oh_remap_from_sei(sei.get(), tables.get(), nullptr) == OH_E_ARG && oh_remap_luts(nullptr, lut.get()) == OH_E_ARG, "null pointers");
    CHECK(oh_remap_from_sei(sei.get(), tables.get(), &r) == OH_OK && oh_remap_luts(&r, nullptr) == OH_E_ARG, "restored; null out of luts");
    r.log2_denom = 16;
    CHECK(oh_remap_luts(&r, lut.get()) == OH_E_ARG, "luts of what the service refuses");
    return calls + 3;
}

int main(void)
{
    printf("curves at the 16 depth pairs: %ld calls\n", curve_group());
    printf("curve refusals: %ld calls\n", curve_refusals());
    printf("samples at the extremes and their refusals: %ld calls\n", sample_group());
    printf("from_sei and luts: %ld calls\n", sei_and_luts_group());
    if (failures) {
        printf("remap math: %d checks failed\n", failures);
        return 1;
    }
    printf("remap math ok\n");
    return 0;
}
