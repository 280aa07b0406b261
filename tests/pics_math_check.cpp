/* pics_math_check.cpp — the host arithmetic of the picture services (openhevc_amd/csrc/pics_math.hip) run on the CPU as a program of its
 * own; built together with that file, with AddressSanitizer and UBSan, by tests/test_pics_math_host.py.  Every output array is a heap
 * block of exactly the documented size, so a write one entry too far is a sanitizer report, and the shift, __int128 and llround
 * arithmetic runs at the extremes of its domain.  Exit status 0: every check of every group held. */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../include/ohevc_hip.h"
#include "../openhevc_amd/csrc/pics_math.h"

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

/* one axis with max_taps exactly what oh_resize_max_taps returns: every row sums to 1 << 14 and stays inside the source */
static void resize_axis(int S, int T, int filter, int phase)
{
    const int mt = oh_resize_max_taps(S, T, filter);
    CHECK(mt >= 1 && mt <= S, "%d -> %d filter %d: max_taps %d", S, T, filter, mt);
    if (mt < 1)
        return;
    auto first = heap<int32_t>((size_t)T);
    auto cnt = heap<int>((size_t)T);
    auto k = heap<int16_t>((size_t)T * mt);
    const int rc = oh_resize_taps(S, T, filter, phase, first.get(), k.get(), mt, cnt.get());
    CHECK(rc == OH_OK, "%d -> %d filter %d phase %d: %d", S, T, filter, phase, rc);
    if (rc != OH_OK)
        return;
    CHECK(oh_resize_taps(S, T, filter, phase, first.get(), k.get(), mt - 1, cnt.get()) == OH_E_ARG, "%d -> %d: max_taps - 1 is taken", S, T);
    for (int x = 0; x < T; x++) {
        int sum = 0;
        for (int j = 0; j < mt; j++) sum += k[(size_t)x * mt + j];
        CHECK(sum == 1 << 14, "%d -> %d filter %d phase %d: row %d sums to %d", S, T, filter, phase, x, sum);
        CHECK(first[x] >= 0 && cnt[x] >= 1 && cnt[x] <= mt && first[x] + cnt[x] <= S, "%d -> %d filter %d phase %d: row %d takes %d taps from %d",
              S, T, filter, phase, x, cnt[x], first[x]);
    }
}

static int resize_group(void)
{
    int n = 0;
    const int extreme[4][2] = { { 16384, 1 }, { 1, 16384 }, { 16384, 16383 }, { 4097, 16384 } };
    for (int filter = OH_RESIZE_BILINEAR; filter <= OH_RESIZE_BICUBIC; filter++)
        for (int phase = 1; phase <= 2; phase++) {
            for (int S = 1; S <= 40; S++)
                for (int T = 1; T <= 40; T++, n++) resize_axis(S, T, filter, phase);
            for (const auto &x : extreme) { resize_axis(x[0], x[1], filter, phase); n++; }
        }
    CHECK(oh_resize_max_taps(16385, 1, 0) == OH_E_ARG && oh_resize_max_taps(0, 1, 0) == OH_E_ARG && oh_resize_max_taps(8, 8, 2) == OH_E_ARG, "extents or filter outside the list");
    return n;
}

static int coeffs_group(void)
{
    int n = 0;
    const int depths[4] = { 8, 9, 10, 12 }, matrices[4] = { 1, 5, 6, 9 }, samples[2] = { OH_CONV_U8, OH_CONV_U16 };
    for (int B : depths)
        for (int m : matrices)
            for (int full = 0; full <= 1; full++)
                for (int sample : samples) {
                    OhConvert cv;
                    memset(&cv, 0, sizeof(cv));
                    cv.format = OH_CONV_RGB; cv.sample = sample; cv.matrix = m; cv.full_range = full;
                    const int D = sample == OH_CONV_U8 ? 8 : 16;
                    auto k = heap<int32_t>(OH_CONV_NCOEFFS);
                    CHECK(oh_convert_coeffs(&cv, B, k.get(), OH_CONV_NCOEFFS) == OH_OK, "convert: %d bit, matrix %d, full %d, D %d", B, m, full, D);
                    CHECK(oh_convert_coeffs(&cv, B, k.get(), OH_CONV_NCOEFFS - 1) == OH_E_ARG, "convert: room for one entry less is taken");
                    CHECK(k[0] > 0 && k[1] > 0 && k[2] < 0 && k[3] < 0 && k[4] > 0 && k[5] == (full ? 0 : 16 << (B - 8)) && k[6] == 1 << (B - 1) &&
                          k[7] >= 1 && k[7] <= 30 && k[8] == D, "convert: %d bit, matrix %d, full %d, D %d: shift %d", B, m, full, D, k[7]);
                    auto c = heap<int32_t>(OH_IMPORT_NCOEFFS);
                    CHECK(oh_import_coeffs(&cv, B, c.get(), OH_IMPORT_NCOEFFS) == OH_OK, "import: %d bit, matrix %d, full %d, D %d", B, m, full, D);
                    CHECK(oh_import_coeffs(&cv, B, c.get(), OH_IMPORT_NCOEFFS - 1) == OH_E_ARG, "import: room for one entry less is taken");
                    /* the rows sum to the exact scale: luma to round(2^S ys / (2^D - 1)) (white gives peak luma), chroma to 0 (greys give mid) */
                    const int S = c[11];
                    CHECK(S >= 1 && S <= 30 && c[12] == D && c[9] == (full ? 0 : 16 << (B - 8)) && c[10] == 1 << (B - 1), "import: shift %d, depth %d", S, c[12]);
                    const double ys = full ? (double)((1 << B) - 1) : 219.0 * (1 << (B - 8));
                    CHECK((int64_t)c[0] + c[1] + c[2] == llround(ldexp(ys / (double)((1 << D) - 1), S)), "import: %d bit, matrix %d, full %d, D %d: the luma row sums to %lld",
                          B, m, full, D, (long long)c[0] + c[1] + c[2]);
                    CHECK(c[3] + c[4] + c[5] == 0 && c[6] + c[7] + c[8] == 0, "import: %d bit, matrix %d, full %d, D %d: a chroma row does not sum to 0", B, m, full, D);
                    n++;
                }
    return n;
}

static bool colour_tables_ok(const OhColour &col)
{
    auto A = heap<int32_t>(OH_COL_NA), G = heap<int32_t>(OH_COL_NP), Bt = heap<int32_t>(OH_COL_NP), misc = heap<int32_t>(OH_COL_NMISC);
    const int rc = oh_colour_tables(&col, A.get(), G.get(), Bt.get(), misc.get());
    CHECK(rc == OH_OK, "transfer %d, primaries %d -> %d, out %d, tone %d, norm %d: %d", col.in_transfer, col.in_primaries, col.out_primaries,
          col.out_transfer, col.tone, col.norm, rc);
    if (rc != OH_OK)
        return false;
    for (int r = 0; r < 3; r++)
        CHECK(misc[3 * r] + misc[3 * r + 1] + misc[3 * r + 2] == 1 << 20, "primaries %d -> %d: matrix row %d", col.in_primaries, col.out_primaries, r);
    CHECK(misc[9] + misc[10] + misc[11] == 1 << 14 && A[0] == 0 && A[OH_COL_NA - 1] > 0, "primaries %d: luminance weights, table A", col.in_primaries);
    return true;
}

static int colour_group(void)
{
    int n = 0;
    /* the combinations of tests/test_colour_host.py: BT.2020 -> BT.709, the source peak that test gives each transfer */
    const int transfers[4] = { 16, 18, 13, 1 }, prims[3] = { 1, 9, 12 };
    for (int t : transfers)
        for (int out = OH_COL_LINEAR; out <= OH_COL_GAMMA24; out++)
            for (int tone = OH_TONE_NONE; tone <= OH_TONE_BT2390; tone++)
                for (int norm = OH_NORM_MAXRGB; norm <= OH_NORM_LUMA; norm++) {
                    if (t == 18 && norm == OH_NORM_MAXRGB)
                        continue;
                    const OhColour col = { t, 9, 1, out, tone, norm, t == 16 || t == 18 ? 1000.0f : 203.0f, 100.0f, 203.0f };
                    n += colour_tables_ok(col);
                }
    for (int pi : prims)
        for (int po : prims) {
            const OhColour col = { 16, pi, po, OH_COL_SRGB, OH_TONE_BT2390, OH_NORM_MAXRGB, 1000.0f, 100.0f, 203.0f };
            n += colour_tables_ok(col);
        }
    return n;
}

static int light_group(void)
{
    for (int b = 0; b < OH_LL_NBINS; b++)
        CHECK(oh_light_bin(oh_light_bin_upper(b)) == b, "bin %d: its largest value %u lies in bin %d", b, oh_light_bin_upper(b), oh_light_bin(oh_light_bin_upper(b)));
    CHECK(oh_light_bin_upper(-1) == 0 && oh_light_bin_upper(OH_LL_NBINS) == 1u << 30, "bins outside the histogram");
    int prev = 0;
    for (int e = 0; e <= 31; e++)
        for (int d = -1; d <= 1; d++) {
            const uint32_t v = (1u << e) + (uint32_t)d;
            const int b = oh_light_bin(v);
            CHECK(b >= prev && b < OH_LL_NBINS, "oh_light_bin(%u) = %d after %d", v, b, prev);
            prev = b;
        }
    /* percentiles of 1 and of 3 pictures, and of histograms that hold fewer than `pixels`: the search ends in the last bin */
    int n_cases = 0;
    for (int n = 1; n <= 3; n += 2)
        for (int lacking = 0; lacking <= 1; lacking++, n_cases++) {
            auto ll = heap<OhLightLevel>((size_t)n);
            memset(ll.get(), 0, (size_t)n * sizeof(OhLightLevel));
            for (int i = 0; i < n; i++) {
                ll[i].pixels = 1000; ll[i].max = 1u << 30;
                ll[i].hist[0] = lacking ? 0 : 500; ll[i].hist[100 + i] = lacking ? 10 : 499; ll[i].hist[OH_LL_NBINS - 1] = lacking ? 0 : 1;
            }
            auto v = heap<uint32_t>(1);
            CHECK(oh_light_percentile(ll.get(), n, 500000, v.get()) == OH_OK && v[0] == (lacking ? 1u << 30 : oh_light_bin_upper(0)), "n %d, lacking %d: median %u", n, lacking, v[0]);
            CHECK(oh_light_percentile(ll.get(), n, 999000, v.get()) == OH_OK && v[0] == (lacking ? 1u << 30 : oh_light_bin_upper(100 + n - 1)), "n %d, lacking %d: 99.9 %% at %u",
                  n, lacking, v[0]);
            CHECK(oh_light_percentile(ll.get(), n, 1000000, v.get()) == OH_OK && v[0] == 1u << 30, "n %d, lacking %d: 100 %% at %u", n, lacking, v[0]);
            CHECK(oh_light_percentile(ll.get(), n, 0, v.get()) == OH_OK && v[0] == oh_light_bin_upper(0), "n %d, lacking %d: 0 %% at %u", n, lacking, v[0]);
            CHECK(oh_light_percentile(ll.get(), n, 1000001, v.get()) == OH_E_ARG && oh_light_percentile(ll.get(), 0, 1, v.get()) == OH_E_ARG, "ppm above 10^6, n below 1");
        }
    return OH_LL_NBINS + 96 + n_cases;
}

static int window_and_blend_group(void)
{
    int n = 0;
    /* an 8x8 window of 12-bit samples at its largest sums: both pictures at 4095, and one at 4095 against one at 0 */
    const int depths[4] = { 8, 9, 10, 12 };
    for (int B : depths) {
        const uint64_t M = (1u << B) - 1;
        int64_t c1 = 0, c2 = 0;
        CHECK(oh_compare_ssim_consts(B, &c1, &c2) == OH_OK && c1 > 0 && c2 > c1, "%d bit: c1, c2", B);
        CHECK(oh_compare_ssim_window(B, (uint32_t)(64 * M), (uint32_t)(64 * M), 2 * 64 * M * M, 64 * M * M) == (int64_t)1 << 30, "%d bit: equal windows at the peak", B);
        const int64_t far = oh_compare_ssim_window(B, (uint32_t)(64 * M), 0, 64 * M * M, 0);
        CHECK(far >= 0 && far < 1 << 20, "%d bit: peak against black gives %lld", B, (long long)far);
        CHECK(oh_compare_ssim_window(B, 0, 0, 0, 0) == (int64_t)1 << 30, "%d bit: black against black", B);
        n += 3;
    }
    CHECK(oh_compare_ssim_window(11, 1, 1, 1, 1) == 0 && oh_compare_ssim_consts(11, nullptr, nullptr) == OH_E_ARG, "a bit depth outside the list");
    CHECK(isinf(oh_compare_psnr(0, 64, 12)) && isnan(oh_compare_psnr(1, 0, 12)) && oh_compare_psnr(~(uint64_t)0, ~(uint64_t)0, 12) > 72.0, "PSNR at its corners");
    /* the blend at the corners of its domain: samples 0 and 4095, alpha 0 and 255, opacity 0 and 256 */
    const uint32_t px[2] = { 0, 4095 }, al[2] = { 0, 255 }, op[2] = { 0, 256 };
    for (uint32_t d : px)
        for (uint32_t s : px)
            for (uint32_t a : al)
                for (uint32_t o : op) {
                    CHECK(oh_compose_blend(d, s, a, o) == (a && o ? s : d), "blend(%u, %u, %u, %u) = %u", d, s, a, o, oh_compose_blend(d, s, a, o));
                    n++;
                }
    CHECK(oh_compose_blend(0, 4095, 255, 255) < 4095 && oh_compose_blend(4095, 0, 1, 1) == 4095 && oh_compose_blend(4095, 0, 128, 128) == 3067, "blend between the corners");
    CHECK(oh_compose_chroma_alpha(1, 255, 255, 255, 255) == 255 && oh_compose_chroma_alpha(2, 255, 254, 0, 0) == 255 && oh_compose_chroma_alpha(3, 7, 0, 0, 0) == 7, "chroma alpha");
    return n;
}

/* the ids of a call that writes pictures (ids_apart, neighbours_resolve), every list a heap block of exactly n ints, and the window size */
static int ids_group(void)
{
    int cases = 0;
    const int sizes[2] = { 1, 65 };
    for (int n : sizes) {
        auto dst = heap<int>((size_t)n), src = heap<int>((size_t)n), nbr = heap<int>((size_t)n);
        auto unread = heap<int>(0);                             /* a list that must not be read: any read is a sanitizer report */
        for (int i = 0; i < n; i++) { dst[i] = 1000 - 7 * i; src[i] = 2000 + i; }      /* destinations not in order: 1000 the largest */
        int both = -5;
        CHECK(ids_apart(dst.get(), n, src.get(), n, &both) == 0 && both == -5, "n %d: apart", n);
        CHECK(ids_apart(dst.get(), n, unread.get(), 0, &both) == 0 && ids_apart(dst.get(), n, nullptr, 0, &both) == 0, "n %d: no sources", n);
        for (int at = 0; at < n; at += std::max(n - 1, 1)) {   /* a source equal to the largest (first) and the smallest (last) destination */
            const int keep = src[n - 1 - at];
            src[n - 1 - at] = dst[at];
            CHECK(ids_apart(dst.get(), n, src.get(), n, &both) == 2 && both == dst[at], "n %d: source %d is destination %d: %d", n, n - 1 - at, at, both);
            src[n - 1 - at] = keep;
            cases++;
        }
        if (n > 1) {                                            /* a duplicate of the first and of the last entry */
            for (int at = 0; at < n; at += n - 1) {
                const int other = at ? n / 2 : n - 1, keep = dst[other];
                dst[other] = dst[at];
                src[0] = dst[at];                               /* listed twice comes first, as the services report it */
                CHECK(ids_apart(dst.get(), n, src.get(), n, &both) == 1, "n %d: entry %d again at %d", n, at, other);
                dst[other] = keep; src[0] = 2000;
                cases++;
            }
        }
        const int *const none[2] = { nullptr, nullptr };
        const int *const dead[2] = { unread.get(), unread.get() };
        const int *const given[2] = { nbr.get(), nullptr };
        const int *const later[2] = { nullptr, nbr.get() };
        std::vector<int> around[2], srcs;
        int side = -5;
        CHECK(neighbours_resolve(none, dst.get(), n, true, around, &srcs, &side) == -1 && (int)srcs.size() == n && around[0] == srcs && around[1] == srcs,
              "n %d: null neighbour arrays", n);
        CHECK(neighbours_resolve(dead, dst.get(), n, false, around, &srcs, &side) == -1 && (int)srcs.size() == n && around[0] == srcs && around[1] == srcs,
              "n %d: neighbours that the mode does not use", n);
        for (int i = 0; i < n; i++) nbr[i] = -1;
        CHECK(neighbours_resolve(given, dst.get(), n, true, around, &srcs, &side) == -1 && (int)srcs.size() == 2 * n && around[0] == around[1] &&
              std::equal(around[0].begin(), around[0].end(), dst.get()) && std::equal(around[0].begin(), around[0].end(), srcs.begin() + n), "n %d: all -1", n);
        nbr[n - 1] = 77;
        CHECK(neighbours_resolve(later, dst.get(), n, true, around, &srcs, &side) == -1 && around[1][n - 1] == 77 && srcs.back() == 77 && around[0][n - 1] == dst[n - 1] &&
              around[1][0] == (n > 1 ? dst[0] : 77), "n %d: a next picture in the last slot", n);
        nbr[n - 1] = -2;
        CHECK(neighbours_resolve(later, dst.get(), n, true, around, &srcs, &side) == n - 1 && side == 1, "n %d: -2 in the last slot of next, side %d", n, side);
        CHECK(neighbours_resolve(given, dst.get(), n, true, around, &srcs, &side) == n - 1 && side == 0, "n %d: -2 in the last slot of prev, side %d", n, side);
        CHECK(neighbours_resolve(given, dst.get(), n, false, around, &srcs, &side) == -1 && (int)srcs.size() == n, "n %d: -2 where the mode does not use it", n);
        cases += 7;
    }
    OhPicParams p;
    memset(&p, 0, sizeof(p));
    p.width = 416; p.height = 240; p.chroma_format_idc = 1;
    const OhWindow w = { 200, 215, 100, 139 };
    int W = 0, H = 0;
    window_size(&p, w, &W, &H);
    std::string why;
    CHECK(W == 1 && H == 1 && crop_window_ok(&p, w, false, &why) && !crop_window_ok(&p, w, true, &why), "a window that leaves %d x %d", W, H);
    return cases + 1;
}

/* the window in a plane class (class_window) against plain shifts, every output a heap block of one int32_t */
static int class_window_group(void)
{
    int cases = 0;
    const int sizes[2][2] = { { 16, 8 }, { 24, 16 } }, offs[3] = { 0, 2, 6 };
    for (int cf = 0; cf <= 3; cf++)
        for (const auto &size : sizes)
            for (int l : offs) for (int r : offs) for (int t : offs) for (int b : offs) {
                OhPicParams p;
                memset(&p, 0, sizeof(p));
                p.width = size[0]; p.height = size[1]; p.chroma_format_idc = cf;
                const OhWindow w = { l, r, t, b };
                const int W = p.width - l - r, H = p.height - t - b;
                if (W < 2 || H < 2)
                    continue;
                for (int q = 0; q <= 1; q++, cases++) {
                    const int sx = q && (cf == 1 || cf == 2), sy = q && cf == 1;
                    auto x0 = heap<int32_t>(1), y0 = heap<int32_t>(1), ws = heap<int32_t>(1), hs = heap<int32_t>(1);
                    class_window(&p, w, q, x0.get(), y0.get(), ws.get(), hs.get());
                    CHECK(x0[0] == l >> sx && y0[0] == t >> sy && ws[0] == W >> sx && hs[0] == H >> sy,
                          "chroma format %d, %dx%d, window (%d,%d,%d,%d), class %d: %dx%d at (%d,%d)", cf, p.width, p.height, l, r, t, b, q,
                          ws[0], hs[0], x0[0], y0[0]);
                }
            }
    return cases;
}

int main()
{
    printf("resize taps: %d axes\n", resize_group());
    printf("conversion and import coefficients: %d combinations\n", coeffs_group());
    printf("colour tables: %d OhColour\n", colour_group());
    printf("light bins and percentiles: %d values\n", light_group());
    printf("ssim window and blend: %d points\n", window_and_blend_group());
    printf("ids apart, neighbours and the window size: %d cases\n", ids_group());
    printf("the window in a plane class: %d cases\n", class_window_group());
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    else printf("pics math ok\n");
    return failures ? 1 : 0;
}
