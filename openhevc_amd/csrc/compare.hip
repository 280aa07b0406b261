/*
 * compare.hip — two finished pictures compared plane by plane (oh_pics_compare; the exact definition is in DESIGN.md §3f and
 * tests/compare_model.py): differing samples, sum |a - b|, sum (a - b)^2, max |a - b|, the first differing sample in raster order, and
 * SSIM over 8 x 8 windows at stride 4 as an integer sum of Q30 window values.  A read-only streaming pass over both pictures, no
 * tables, no filtering; everything that leaves a workgroup is an integer sum, maximum or count, so the result does not depend on
 * the order in which workgroups arrive.
 *
 * The plane's window is cut into 4 x 4 blocks anchored at its top-left and into tiles of OH_CMP_TW x OH_CMP_TH samples (64 x 8
 * blocks).  A workgroup takes one tile of one plane of one pair.  A lane loads whole blocks, four samples of a row of each picture per
 * access (the window may start at any sample: the accesses are aligned to samples only), keeps the difference statistics in registers
 * and, with SSIM, writes the block's four sums (sum a, sum b, sum a^2 + b^2, sum ab) to LDS.  The windows whose top-left block lies in
 * the tile are the workgroup's: it also loads one block column to the right and one block row below — recomputed, not exchanged
 * between workgroups — which take no part in its difference statistics.  After a barrier each lane adds 2 x 2 blocks to a window and
 * evaluates compare_ssim_window (compare_common.h, shared with the host).  The columns and rows the blocks leave over (w & 3, h & 3)
 * go through the difference statistics only, sample by sample, in the tiles of the last tile column and row.  Waves reduce with
 * shuffles, the workgroup through LDS, and one lane issues the integer atomics into the pair's zeroed result — into one of OH_CMP_SLOTS
 * partial results per plane, each a 64-byte line of its own, which the host combines: a 4K luma plane has a thousand tiles, and their
 * atomics on one line queue up behind each other.
 */
#include "pics_common.h"
#include "compare_common.h"

namespace {

constexpr int WAVES = THREADS / 64;
constexpr int BX = OH_CMP_TW / 4, BY = OH_CMP_TH / 4;           /* blocks of a tile */
constexpr int LX = BX + 1, LY = BY + 1;                         /* with the column and the row of the neighbours' blocks */

/* what a lane gathers: 32 bits hold its few dozen samples (at 12 bit a squared difference is below 2^24) */
struct Diff {
    uint32_t differing = 0, sad = 0, sse = 0, max_abs = 0, not_first = 0;
    /* samples x of a and y of b whose key is ~nkey */
    __device__ __forceinline__ void add(int x, int y, uint32_t nkey)
    {
        const int d = x - y;
        const uint32_t ad = (uint32_t)abs(d);
        differing += d != 0;
        sad += ad;
        sse += ad * ad;
        max_abs = max(max_abs, ad);
        not_first = max(not_first, d ? nkey : 0u);
    }
};
static_assert(((LX * LY + THREADS - 1) / THREADS * 16 + 8) * 4095ull * 4095ull < (1ull << 32), "a lane's sum of squares in 32 bits");

template <typename T, bool SSIM>
__global__ __launch_bounds__(THREADS) void compare_kernel(const OhCmpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint4v blk[SSIM ? LX * LY : 1];
    __shared__ unsigned long long red_sse[WAVES], red_ssim[WAVES];
    __shared__ uint32_t red_diff[WAVES], red_sad[WAVES], red_max[WAVES], red_nf[WAVES];
    const int pair = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per[2] = { a.k[0].tx * a.k[0].ty, a.k[1].tx * a.k[1].ty };
    int plane, pq;
    const int tile = grid_row(blockIdx.x, per, plane, pq);
    const OhCmpClass &k = a.k[pq];
    const int ty = tile / k.tx, tx = tile - ty * k.tx;
    const int w = k.w, h = k.h, nbx = w >> 2, nby = h >> 2, bx0 = tx * BX, by0 = ty * BY;
    const size_t pitch = (size_t)a.pitch[plane], org = (size_t)k.y0 * pitch + (size_t)k.x0 * sizeof(T);
    const GLOBAL uint8_t *pa = (const GLOBAL uint8_t *)a.a[pair][plane] + org, *pb = (const GLOBAL uint8_t *)a.b[pair][plane] + org;
    Diff df;

    constexpr int lx = SSIM ? LX : BX, ly = SSIM ? LY : BY;
    for (int i = t; i < lx * ly; i += THREADS) {
        const int r = i / lx, c = i - r * lx, bx = bx0 + c, by = by0 + r;
        uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
        if (bx < nbx && by < nby) {
            const bool own = c < BX && r < BY;                  /* not a neighbour's block */
            const size_t o = (size_t)(4 * by) * pitch + (size_t)(4 * bx) * sizeof(T);
            uint2v ra[4], rb[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                ra[j] = load4_pairs((const GLOBAL T *)(pa + o + j * pitch));
                rb[j] = load4_pairs((const GLOBAL T *)(pb + o + j * pitch));
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int x[4] = { (int)(ra[j][0] & 0xffff), (int)(ra[j][0] >> 16), (int)(ra[j][1] & 0xffff), (int)(ra[j][1] >> 16) };
                const int y[4] = { (int)(rb[j][0] & 0xffff), (int)(rb[j][0] >> 16), (int)(rb[j][1] & 0xffff), (int)(rb[j][1] >> 16) };
                const uint32_t nkey = ~((uint32_t)(4 * by + j) * (uint32_t)w + (uint32_t)(4 * bx));
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    if (SSIM) {
                        s1 += x[s]; s2 += y[s];
                        ss += x[s] * x[s] + y[s] * y[s];
                        s12 += x[s] * y[s];
                    }
                    if (own)
                        df.add(x[s], y[s], nkey - s);
                }
            }
        }
        if (SSIM)
            blk[i] = uint4v{ s1, s2, ss, s12 };
    }

    /* the columns right of the last block column and the rows below the last block row */
    const int xe = min(4 * (bx0 + BX), 4 * nbx), ye = min(4 * (by0 + BY), 4 * nby);
    const bool lastx = tx == k.tx - 1, lasty = ty == k.ty - 1;
    auto strip = [&](int xs, int xn, int ys, int yn) {          /* xn x yn samples from (xs, ys) */
        for (int i = t; i < xn * yn; i += THREADS) {
            const int yy = i / xn, y = ys + yy, x = xs + (i - yy * xn);
            const size_t o = (size_t)y * pitch + (size_t)x * sizeof(T);
            df.add((int)*(const GLOBAL T *)(pa + o), (int)*(const GLOBAL T *)(pb + o), ~((uint32_t)y * (uint32_t)w + (uint32_t)x));
        }
    };
    if (lastx && w > 4 * nbx)
        strip(4 * nbx, w - 4 * nbx, 4 * by0, (lasty ? h : ye) - 4 * by0);
    if (lasty && h > 4 * nby && xe > 4 * bx0)
        strip(4 * bx0, xe - 4 * bx0, 4 * nby, h - 4 * nby);

    long long q = 0;
    if (SSIM) {
        __syncthreads();
        int64_t c1, c2;
        compare_ssim_consts(a.bd, &c1, &c2);
        for (int i = t; i < BX * BY; i += THREADS) {
            const int r = i / BX, c = i - r * BX;
            if (bx0 + c < nbx - 1 && by0 + r < nby - 1) {
                const uint4v u = blk[r * LX + c] + blk[r * LX + c + 1] + blk[(r + 1) * LX + c] + blk[(r + 1) * LX + c + 1];
                q += compare_ssim_window(c1, c2, u[0], u[1], u[2], u[3]);
            }
        }
    }

    unsigned long long sse = df.sse, qs = (unsigned long long)q;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sse += __shfl_xor(sse, d);
        qs += __shfl_xor(qs, d);
        df.differing += (uint32_t)__shfl_xor((int)df.differing, d);
        df.sad += (uint32_t)__shfl_xor((int)df.sad, d);
        df.max_abs = max(df.max_abs, (uint32_t)__shfl_xor((int)df.max_abs, d));
        df.not_first = max(df.not_first, (uint32_t)__shfl_xor((int)df.not_first, d));
    }
    if (lane == 0) {
        red_sse[wave] = sse; red_ssim[wave] = qs;
        red_diff[wave] = df.differing; red_sad[wave] = df.sad; red_max[wave] = df.max_abs; red_nf[wave] = df.not_first;
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int v = 1; v < WAVES; v++) {
            sse += red_sse[v]; qs += red_ssim[v];
            df.differing += red_diff[v]; df.sad += red_sad[v];
            df.max_abs = max(df.max_abs, red_max[v]); df.not_first = max(df.not_first, red_nf[v]);
        }
        OhCmpDev *res = a.res + ((size_t)pair * 3 + plane) * OH_CMP_SLOTS + blockIdx.x % OH_CMP_SLOTS;
        if (df.differing) {                                     /* equal tiles add nothing */
            atomicAdd(&res->differing, (unsigned long long)df.differing);
            atomicAdd(&res->sad, (unsigned long long)df.sad);
            atomicAdd(&res->sse, sse);
            atomicMax(&res->max_abs, df.max_abs);
            atomicMax(&res->not_first, df.not_first);
        }
        if (SSIM && qs)
            atomicAdd(&res->ssim_sum, qs);
    }
}

} // namespace

static_assert(OH_CMP_TW % 4 == 0 && OH_CMP_TH % 4 == 0, "tiles of whole blocks");
static_assert(sizeof(OhCmpArgs) <= 4096, "kernel arguments");
static_assert(sizeof(OhCmpDev) == 64, "a slot is a line of its own");

extern "C" void ohk_compare(const OhCmpArgs *a, int n, hipStream_t st)
{
    const dim3 grid((unsigned)(a->k[0].tx * a->k[0].ty + (a->np - 1) * a->k[1].tx * a->k[1].ty), (unsigned)n);
    if (a->bd > 8) {
        if (a->ssim) compare_kernel<uint16_t, true><<<grid, THREADS, 0, st>>>(*a);
        else         compare_kernel<uint16_t, false><<<grid, THREADS, 0, st>>>(*a);
    } else {
        if (a->ssim) compare_kernel<uint8_t, true><<<grid, THREADS, 0, st>>>(*a);
        else         compare_kernel<uint8_t, false><<<grid, THREADS, 0, st>>>(*a);
    }
}
