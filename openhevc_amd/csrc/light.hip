/*
 * light.hip — light-level statistics of finished pictures (oh_pics_light_level; the exact definition is in DESIGN.md §3e and
 * tests/light_model.py): per picture the sum, the maximum, the minimum and a histogram with 16 bins per octave of a norm of the
 * linear-light R, G, B of every pixel of the window — what a tone curve needs to know of a scene, without a host copy of a picture.
 *
 * The shape of colour.hip's kernel — stage the luma and chroma granules of a row segment to LDS, chroma filter, the H.273 matrix to 16
 * bit, the source curve A out of LDS — without the later stages and without an image: what leaves a workgroup is one integer atomic per
 * bin it met plus max / min / 64-bit sum into the picture's zeroed result.  Everything is an integer sum, maximum or count, so the
 * result does not depend on the order in which workgroups arrive.
 *
 * A workgroup loads A (16.4 KB) once and takes OH_LL_ROWS image rows of its segment of OH_LL_CW columns.  Max, min and sum stay in
 * registers per lane until the end.  The histogram lives in LDS, one private copy per wave.  Neighbouring pixels of a natural picture
 * fall into the same bin, and 64 LDS atomics on one address run one after the other: so the lanes of a wave first find the runs of
 * equal bins among them (one ballot) and only the first lane of each run adds, the length of the run.  A flat row costs one atomic per
 * wave, a row of noise 64 to different addresses.
 */
#include "colour_common.h"

namespace {

constexpr int WAVES = THREADS / 64;
constexpr int HS = 264;                                         /* uint32 between the waves' copies of the histogram */

/* bin(v) of DESIGN.md §3e for 0 <= v <= 2^30 */
__device__ __forceinline__ int light_bin(int v)
{
    const int e = 31 - __clz(v | 1);
    return v < (1 << 14) ? 0 : 1 + 16 * (e - 14) + ((v >> (e - 4)) & 15);
}

template <typename TI>
__global__ __launch_bounds__(THREADS) void light_kernel(const OhLightArgs la)
{
    const OhConvArgs &a = la.c;
    constexpr int CW = OH_LL_CW;
    constexpr int RB = ((CW / 2 + 1) * (int)sizeof(TI) + 32 + 15) / 16 * 16;       /* one staged 4:2:x chroma row; 4:4:4 takes two */
    static_assert(CW * (int)sizeof(TI) + 32 <= 2 * RB, "a 4:4:4 chroma row in two staged rows");
    __shared__ __attribute__((aligned(16))) uint8_t lum[CW * sizeof(TI) + 32];
    __shared__ __attribute__((aligned(16))) uint8_t chr[4 * RB];
    __shared__ __attribute__((aligned(16))) int32_t tab[OH_COLT_G];
    __shared__ uint32_t hist[WAVES * HS];
    __shared__ unsigned long long red_sum[WAVES];
    __shared__ uint32_t red_max[WAVES], red_nmin[WAVES];
    const int pic = blockIdx.z, y0 = blockIdx.y * OH_LL_ROWS, x0 = blockIdx.x * CW;
    const int W = a.W, H = a.H;
    if (x0 >= W)
        return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < OH_COLT_G / 4; i += THREADS)            /* visible after the first row's barrier */
        ((uint4v *)tab)[i] = ((const GLOBAL uint4v *)la.tab)[i];
    for (int i = t; i < WAVES * HS; i += THREADS)
        hist[i] = 0;
    const int cnt = min(CW, W - x0), X0 = a.left + x0, y1 = min(y0 + OH_LL_ROWS, H);
    const RgbMatrix mt(a.k);
    const int wr = la.w[0], wg = la.w[1], wb = la.w[2];
    const bool luma = la.luma != 0;
    uint32_t *my_hist = hist + wave * HS;
    unsigned long long sum = 0;
    uint32_t mx = 0, nmn = 0;
    for (int y = y0; y < y1; y++) {
        RgbRows<TI> in;
        in.stage_rows(a, pic, X0, a.top + y, cnt, lum, chr, RB);
        __syncthreads();
        for (int i0 = 0; i0 < cnt; i0 += THREADS) {             /* every lane of a wave takes every turn: the lanes talk to each other */
            const bool on = i0 + t < cnt;
            const int i = on ? i0 + t : cnt - 1;
            int u, v, R, G, B;
            in.chroma(a, X0 + i, i, mt.mid, u, v);
            mt.rgb((int)in.L[i], u, v, R, G, B);
            const int l0 = src_curve(tab, R), l1 = src_curve(tab, G), l2 = src_curve(tab, B);
            const int nrm = luma ? luma_norm_of(wr, wg, wb, l0, l1, l2) : max(l0, max(l1, l2));
            if (on) {
                sum += (uint32_t)nrm;
                mx = max(mx, (uint32_t)nrm);
                nmn = max(nmn, ~(uint32_t)nrm);
            }
            /* runs of equal bins among the lanes: a lane whose lower neighbour has another bin heads a run that ends in front of the
             * next head.  Lanes past the row's end have bin -1 and form the last run, which nobody adds. */
            const int b = on ? light_bin(nrm) : -1;
            const int below = __shfl_up(b, 1);
            const bool head = lane == 0 || below != b;
            const unsigned long long above = (__ballot(head) >> lane) >> 1;
            const int run = above ? __ffsll(above) : 64 - lane;
            if (head && b >= 0)
                atomicAdd(&my_hist[b], (uint32_t)run);
        }
        __syncthreads();                                        /* every lane is done with the staged rows */
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d);
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
        nmn = max(nmn, (uint32_t)__shfl_xor((int)nmn, d));
    }
    if (lane == 0) {
        red_sum[wave] = sum; red_max[wave] = mx; red_nmin[wave] = nmn;
    }
    __syncthreads();                                            /* and the last row's histogram adds are done */
    OhLightDev *res = la.res + pic;
    for (int b = t; b < OH_LL_NBINS; b += THREADS) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++)
            c += hist[w * HS + b];
        if (c)
            atomicAdd(&res->hist[b], c);
    }
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < WAVES; w++) {
            sum += red_sum[w]; mx = max(mx, red_max[w]); nmn = max(nmn, red_nmin[w]);
        }
        atomicAdd(&res->sum, sum);
        atomicMax(&res->max, mx);
        atomicMax(&res->not_min, nmn);
    }
}

} // namespace

static_assert(OH_COLT_G >= OH_COL_NA && OH_COLT_G % 4 == 0, "table A as whole 16-byte granules");
static_assert(OH_LL_NBINS <= HS, "a wave's copy of the histogram");

extern "C" void ohk_light(const OhLightArgs *a, int n, hipStream_t st)
{
    const dim3 grid((unsigned)((a->c.W + OH_LL_CW - 1) / OH_LL_CW), (unsigned)((a->c.H + OH_LL_ROWS - 1) / OH_LL_ROWS), (unsigned)n);
    if (a->c.bd > 8)
        light_kernel<uint16_t><<<grid, THREADS, 0, st>>>(*a);
    else
        light_kernel<uint8_t><<<grid, THREADS, 0, st>>>(*a);
}
