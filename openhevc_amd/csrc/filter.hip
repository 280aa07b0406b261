/*
 * filter.hip — spatial and temporal filters of finished pictures (oh_pics_filter; the exact definitions are in DESIGN.md §3m and
 * tests/filter_model.py; the sample formulas are filter_common.h, shared with the host).
 *
 * A stencil with a halo in both directions.  One workgroup (256 lanes, four wave64) makes a tile of OH_FLT_TW x OH_FLT_TH samples of
 * one plane of one destination; grid (tiles across, tiles down of all planes, pictures of the launch — all of them share one
 * geometry; their plane addresses are in the kernel arguments).  Both global sides move as whole aligned 16-byte granules (plane rows
 * start 256-byte aligned and are padded, so a granule that holds a coded sample lies in its row); the samples behind the coded width
 * in the last granule lie in the row's padding, which nothing reads.
 *
 * Staging: the tile's rows and R rows above and below, its granules and one granule on either side (R <= 7 is less than a granule),
 * go from HBM into LDS one granule per lane and step.  Rows and granules are clamped there, and a granule that holds columns outside
 * the plane gets them replaced by the edge sample, so LDS holds S[r(y)][cx(x)] and the passes below never look at an edge.
 * An item of the passes is one granule of one row: a lane reads the item's granule and its two neighbours (ds_read_b128, consecutive
 * lanes consecutive granules) into a register window of GS + 2 R samples.
 *
 * CONVOLVE / UNSHARP, templated on the radius class R in {1, 2, 4, 7} (the taps of the call, centred in 2 R + 1 with zeros around
 * them, sit in scalar registers): the horizontal pass makes the int32 sums of all TH + 2 R staged rows and leaves them in LDS, four
 * sums per lane and 16-byte word laid out so that consecutive lanes write and read consecutive words; the vertical pass adds 2 R + 1
 * of those rows per item, rounds once, (UNSHARP) takes the source granule from the staged tile, and stores one granule.  The products
 * are 24-bit multiplies (filter_common.h: filter_mul), which legal taps and 12-bit samples never overflow.
 * MEDIAN (R = 1): the three samples of each of the GS + 2 columns of an item are sorted once, an output takes the median of the
 * three columns around it (filter_common.h: filter_median_cols) — min / max / med3 on registers.
 * TEMPORAL (R = 1): the tiles of prev, src and next are staged; the column sums of |P - C| and |N - C| are made once per item and
 * three of them added per output.
 * A plane whose bit is clear in `planes` is copied, granule by granule, by the workgroups of its tiles.
 * Templates on the stored sample type, the mode class and R.
 */
#include <algorithm>
#include "pics_common.h"
#include "filter_common.h"

namespace {

constexpr int TW = OH_FLT_TW, TH = OH_FLT_TH;
enum { K_CONV, K_MEDIAN, K_TEMPORAL };            /* the kernels: CONVOLVE and UNSHARP share one */

typedef int int4v __attribute__((ext_vector_type(4)));

template <typename T>
struct Geo {
    static constexpr int SZ = (int)sizeof(T), GS = 16 / SZ;     /* samples of a granule */
    static constexpr int NG = TW / GS;                          /* granules (items) of a tile row */
    static constexpr int SG = NG + 2;                           /* staged granules of a row: one more on either side */
    static constexpr int PITCH = SG * 16;                       /* bytes of a staged row */
};

template <typename T, int R> constexpr int tile_bytes() { return (TH + 2 * R) * Geo<T>::PITCH; }
template <int R> constexpr int sums_bytes() { return (TH + 2 * R) * TW * 4; }

/* rows Y0 - R .. Y0 + TH + R - 1 (clamped) of the plane at `base`, granules X0 / GS - 1 .. X0 / GS + NG (columns clamped), into `tile` */
template <typename T, int R>
__device__ __forceinline__ void stage_tile(LDS uint8_t *tile, const uint8_t *base, size_t pitch, int W, int H, int X0, int Y0)
{
    typedef Geo<T> Gm;
    constexpr int GS = Gm::GS, N = (TH + 2 * R) * Gm::SG;
    const int G = (W + GS - 1) / GS, last = W - 1 - (G - 1) * GS;      /* granules of a row; where the last coded sample sits in the last one */
    const int gx0 = X0 / GS - 1;
#pragma unroll
    for (int it = 0; it < (N + THREADS - 1) / THREADS; it++) {
        const int i = it * THREADS + (int)threadIdx.x;
        if (i >= N)
            break;
        const int row = i / Gm::SG, j = i - row * Gm::SG;
        const int y = min(max(Y0 - R + row, 0), H - 1);
        const int gx = gx0 + j, gc = min(max(gx, 0), G - 1);
        uint4v v = *(const GLOBAL uint4v *)((uintptr_t)base + (size_t)y * pitch + 16 * (uintptr_t)gc);
        if (gx < 0 || (gx + 1) * GS > W) {                      /* columns outside the plane: the edge sample instead */
            const Samples<T> in(v);
            Samples<T> out;
            T edge = in.s[0];
            if (gx >= 0) {
#pragma unroll
                for (int s = 1; s < GS; s++)
                    edge = s == last ? in.s[s] : edge;
            }
#pragma unroll
            for (int s = 0; s < GS; s++)
                out.s[s] = (gx < 0 || gx > G - 1 || s > last) ? edge : in.s[s];
            v = out.granule();
        }
        *(LDS uint4v *)(tile + row * Gm::PITCH + 16 * j) = v;
    }
}

/* the samples of columns x0 - R .. x0 + GS + R - 1 around item g (columns x0 ..) of a staged row */
template <typename T, int R>
__device__ __forceinline__ void window(const LDS uint8_t *row, int g, int32_t *win)
{
    constexpr int GS = Geo<T>::GS;
    const LDS uint4v *p = (const LDS uint4v *)(row + 16 * g);
    const Samples<T> a(p[0]), b(p[1]), c(p[2]);
#pragma unroll
    for (int t = 0; t < GS + 2 * R; t++) {
        const int idx = GS - R + t;
        win[t] = idx < GS ? a.s[idx] : idx < 2 * GS ? b.s[idx - GS] : c.s[idx - 2 * GS];
    }
}

template <typename T, int KIND, int R>
__global__ __launch_bounds__(THREADS) void filter_kernel(const OhFilterArgs a)
{
    typedef Geo<T> Gm;
    typedef Samples<T> Sm;
    constexpr int GS = Gm::GS, NG = Gm::NG, PITCH = Gm::PITCH, TB = tile_bytes<T, R>();
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_g[];
    LDS uint8_t *lds = (LDS uint8_t *)lds_g;
    const int pic = blockIdx.z;
    const int per[2] = { (a.h[0] + TH - 1) / TH, (a.h[1] + TH - 1) / TH };
    int c, q;
    const int Y0 = grid_row(blockIdx.y, per, c, q) * TH;
    const int W = a.w[q], H = a.h[q], M = (1 << a.bd) - 1;
    const int G = (W + GS - 1) / GS;
    const int X0 = blockIdx.x * TW, G0 = X0 / GS;
    if (G0 >= G)
        return;
    const size_t pitch = (size_t)a.pitch[c];
    const uint8_t *S = (const uint8_t *)a.src[1][pic][c];
    const uintptr_t D = (uintptr_t)a.dst[pic][c];
    auto st = [&](int y, int g, uint4v v) { *(GLOBAL uint4v *)(D + (size_t)y * pitch + 16 * (uintptr_t)g) = v; };

    if (!(a.planes >> c & 1)) {                                 /* not selected: a copy */
        for (int i = threadIdx.x; i < TH * NG; i += THREADS) {
            const int row = i / NG, g = i - row * NG, y = Y0 + row;
            if (y < H && G0 + g < G)
                st(y, G0 + g, *(const GLOBAL uint4v *)((uintptr_t)S + (size_t)y * pitch + 16 * (uintptr_t)(G0 + g)));
        }
        return;
    }

    stage_tile<T, R>(lds, S, pitch, W, H, X0, Y0);
    if constexpr (KIND == K_TEMPORAL) {
        stage_tile<T, R>(lds + TB, (const uint8_t *)a.src[0][pic][c], pitch, W, H, X0, Y0);
        stage_tile<T, R>(lds + 2 * TB, (const uint8_t *)a.src[2][pic][c], pitch, W, H, X0, Y0);
    }
    __syncthreads();

    if constexpr (KIND == K_CONV) {
        LDS int4v *sums = (LDS int4v *)(lds + TB);              /* word ((row * GS / 4 + j) * NG + g): sums 4 j .. 4 j + 3 of item g of a staged row */
        int32_t th[2 * R + 1], tv[2 * R + 1];
#pragma unroll
        for (int k = 0; k < 2 * R + 1; k++) {
            th[k] = a.taps_h[q][OH_FILTER_MAX_TAPS / 2 - R + k];
            tv[k] = a.taps_v[q][OH_FILTER_MAX_TAPS / 2 - R + k];
        }
        for (int i = threadIdx.x; i < (TH + 2 * R) * NG; i += THREADS) {
            const int row = i / NG, g = i - row * NG;
            int32_t win[GS + 2 * R];
            window<T, R>(lds + row * PITCH, g, win);
#pragma unroll
            for (int j = 0; j < GS / 4; j++) {
                int4v acc;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    int32_t v = 0;
#pragma unroll
                    for (int k = 0; k < 2 * R + 1; k++)
                        v += filter_mul(th[k], win[4 * j + e + k]);
                    acc[e] = v;
                }
                sums[(row * (GS / 4) + j) * NG + g] = acc;
            }
        }
        __syncthreads();
        const int unsharp = a.mode == OH_FILTER_UNSHARP, amount = a.amount[q], thr = a.threshold[q];
        for (int i = threadIdx.x; i < TH * NG; i += THREADS) {
            const int row = i / NG, g = i - row * NG, y = Y0 + row;
            if (y >= H || G0 + g >= G)
                continue;
            int32_t acc[GS];
#pragma unroll
            for (int s = 0; s < GS; s++)
                acc[s] = 0;
#pragma unroll
            for (int k = 0; k < 2 * R + 1; k++)
#pragma unroll
                for (int j = 0; j < GS / 4; j++) {
                    const int4v t = sums[((row + k) * (GS / 4) + j) * NG + g];
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        acc[4 * j + e] += filter_mul(tv[k], t[e]);
                }
            const Sm src(*(const LDS uint4v *)(lds + (row + R) * PITCH + 16 * (g + 1)));
            Sm o;
#pragma unroll
            for (int s = 0; s < GS; s++) {
                const int32_t b = filter_round(acc[s], M);
                o.s[s] = (T)(unsharp ? filter_unsharp(src.s[s], b, amount, thr, M) : b);
            }
            st(y, G0 + g, o.granule());
        }
    } else {
        const int thr = a.threshold[q];
        for (int i = threadIdx.x; i < TH * NG; i += THREADS) {
            const int row = i / NG, g = i - row * NG, y = Y0 + row;
            if (y >= H || G0 + g >= G)
                continue;
            int32_t w[3][GS + 2];                               /* w[j][t]: row y - 1 + j, column x0 - 1 + t of src */
#pragma unroll
            for (int j = 0; j < 3; j++)
                window<T, 1>(lds + (row + j) * PITCH, g, w[j]);
            Sm o;
            if constexpr (KIND == K_MEDIAN) {
                int32_t lo[GS + 2], mid[GS + 2], hi[GS + 2];
#pragma unroll
                for (int t = 0; t < GS + 2; t++)
                    filter_sort3(w[0][t], w[1][t], w[2][t], lo[t], mid[t], hi[t]);
#pragma unroll
                for (int s = 0; s < GS; s++)
                    o.s[s] = (T)filter_median_cols(lo + s, mid + s, hi + s);
            } else {
                int32_t cp[GS + 2], cn[GS + 2], pc[GS], nc[GS];  /* column sums of |P - C| and |N - C|; P and N at the outputs' places */
#pragma unroll
                for (int t = 0; t < GS + 2; t++)
                    cp[t] = cn[t] = 0;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    int32_t wp[GS + 2], wn[GS + 2];
                    window<T, 1>(lds + TB + (row + j) * PITCH, g, wp);
                    window<T, 1>(lds + 2 * TB + (row + j) * PITCH, g, wn);
#pragma unroll
                    for (int t = 0; t < GS + 2; t++) {
                        cp[t] += filter_abs(wp[t] - w[j][t]);
                        cn[t] += filter_abs(wn[t] - w[j][t]);
                    }
                    if (j == 1) {
#pragma unroll
                        for (int s = 0; s < GS; s++) { pc[s] = wp[s + 1]; nc[s] = wn[s + 1]; }
                    }
                }
#pragma unroll
                for (int s = 0; s < GS; s++)
                    o.s[s] = (T)filter_temporal(w[1][s + 1], pc[s], nc[s], cp[s] + cp[s + 1] + cp[s + 2], cn[s] + cn[s + 1] + cn[s + 2], thr);
            }
            st(y, G0 + g, o.granule());
        }
    }
}

template <typename T, int KIND, int R>
void launch_as(const OhFilterArgs *a, const dim3 &grid, hipStream_t st)
{
    const size_t lds = KIND == K_CONV ? (size_t)tile_bytes<T, R>() + sums_bytes<R>() : (size_t)(KIND == K_TEMPORAL ? 3 : 1) * tile_bytes<T, R>();
    filter_kernel<T, KIND, R><<<grid, THREADS, lds, st>>>(*a);
}

template <typename T>
void launch(const OhFilterArgs *a, int n, hipStream_t st)
{
    const int cls = a->np > 1 ? 2 : 1;
    int w = 0, rows = 0;
    for (int q = 0; q < cls; q++) {
        w = std::max(w, a->w[q]);
        rows += (q ? 2 : 1) * ((a->h[q] + TH - 1) / TH);
    }
    const dim3 grid((unsigned)((w + TW - 1) / TW), (unsigned)rows, (unsigned)n);
    if (a->mode == OH_FILTER_MEDIAN)        launch_as<T, K_MEDIAN, 1>(a, grid, st);
    else if (a->mode == OH_FILTER_TEMPORAL) launch_as<T, K_TEMPORAL, 1>(a, grid, st);
    else if (a->radius <= 1)                launch_as<T, K_CONV, 1>(a, grid, st);
    else if (a->radius <= 2)                launch_as<T, K_CONV, 2>(a, grid, st);
    else if (a->radius <= 4)                launch_as<T, K_CONV, 4>(a, grid, st);
    else                                    launch_as<T, K_CONV, 7>(a, grid, st);
}

} // namespace

static_assert(sizeof(((OhFilterArgs *)nullptr)->taps_h[0]) / sizeof(int32_t) == OH_FILTER_MAX_TAPS, "the centred taps of one class");
static_assert(OH_FLT_TW % 16 == 0 && OH_FILTER_MAX_TAPS / 2 < 8, "a tile row is whole granules of either sample type; the halo is less than one");
static_assert(tile_bytes<uint16_t, 7>() + sums_bytes<7>() <= 64 << 10 && 3 * tile_bytes<uint16_t, 1>() <= 64 << 10, "LDS of one workgroup");

extern "C" void ohk_filter(const OhFilterArgs *a, int n, hipStream_t st)
{
    if (a->bd == 8) launch<uint8_t>(a, n, st);
    else            launch<uint16_t>(a, n, st);
}
