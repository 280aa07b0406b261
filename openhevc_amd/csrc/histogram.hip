/*
 * histogram.hip — the code values of finished pictures counted plane by plane (oh_pics_histogram; the exact definition is in DESIGN.md
 * §3n and tests/levels_model.py).  A read-only streaming pass over the plane's window; the kernel makes the bins only — samples, sum, sum
 * of squares, minimum and maximum follow from them on the host (engine_pics.hip) — and everything that leaves a workgroup is an integer
 * count, so the result does not depend on the order in which workgroups arrive.
 *
 * The shape of light.hip's histogram without its colour stages.  A workgroup (256 lanes) takes OH_HG_ROWS rows of the window of one
 * plane of one picture; a lane loads one aligned 16-byte granule at a time (plane rows start 256-byte aligned, so every granule that
 * holds a sample of the window lies in its row) and masks the samples left and right of the window.  The histogram lives in LDS, 2^bit
 * depth counters of 32 bits per copy (1 KB at 8 bit, 16 KB at 12), one copy per wave, at 12 bit one for two waves.  Neighbouring samples
 * of a natural picture are often equal, and LDS atomics on one address run one after the other.  So equal values are combined before
 * the atomic, twice:
 *   1. inside the lane's granule: a run of equal samples is one add of its length;
 *   2. across the lanes of the wave: a lane whose whole granule holds one value takes part in light.hip's run search — one ballot
 *      finds the runs of lanes with the same value, and the first lane of a run adds run x samples-per-granule.
 * A flat row costs one atomic per wave and turn, a row of noise one per sample to different addresses.  The counts are 32 bits
 * everywhere: no partial counter is narrower than the result.  At the end the workgroup adds its non-zero bins to the plane's zeroed
 * result with one atomic each.
 */
#include "pics_common.h"

namespace {

constexpr int WAVES = THREADS / 64;

/* the wave's copies of the histogram: as many as keep the LDS of a workgroup at 32 KB */
__host__ __device__ constexpr int copies_of(int bd) { return bd > 10 ? 2 : WAVES; }

template <typename T>
__global__ __launch_bounds__(THREADS) void histogram_kernel(const OhHistArgs a)
{
    constexpr int GS = 16 / (int)sizeof(T), SB = 8 * (int)sizeof(T);
    constexpr uint32_t SM = (1u << SB) - 1, REP = sizeof(T) == 1 ? 0x01010101u : 0x00010001u;
    extern __shared__ uint32_t hist[];                          /* copies_of(bd) << bd */
    const int pic = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per[2] = { a.k[0].tiles, a.k[1].tiles };
    int plane, q;
    const int tile = grid_row(blockIdx.x, per, plane, q);
    const OhHistClass &k = a.k[q];
    const int bins = 1 << a.bd, copies = copies_of(a.bd);
    const uint32_t M = (uint32_t)bins - 1;
    for (int i = t; i < copies * bins; i += THREADS)
        hist[i] = 0;
    __syncthreads();
    uint32_t *my = hist + (wave % copies) * bins;
    const int r0 = tile * OH_HG_ROWS, total = min(OH_HG_ROWS, k.h - r0) * k.ng;
    const size_t pitch = (size_t)a.pitch[plane];
    const GLOBAL uint8_t *base = (const GLOBAL uint8_t *)a.src[pic][plane] + (size_t)(k.y0 + r0) * pitch + (size_t)k.g0 * 16;
    for (int i0 = 0; i0 < total; i0 += THREADS) {               /* every lane of a wave takes every turn: the lanes talk to each other */
        const int i = i0 + t;
        int key = -1;                                           /* the one value of a whole granule inside the window */
        if (i < total) {
            const int r = i / k.ng, g = i - r * k.ng;
            const uint4v v = *(const GLOBAL uint4v *)(base + (size_t)r * pitch + (size_t)g * 16);
            const int xs = (k.g0 + g) * GS;                     /* the plane column of the granule's first sample */
            const int lo = max(k.x0 - xs, 0), hi = min(k.x0 + k.w - xs, GS);
            const uint32_t s0 = v[0] & SM;
            if (lo == 0 && hi == GS && v[0] == s0 * REP && v[1] == v[0] && v[2] == v[0] && v[3] == v[0]) {
                key = (int)min(s0, M);
            } else {                                            /* the runs of equal samples inside the granule */
                uint32_t cur = 0, cnt = 0;
#pragma unroll
                for (int j = 0; j < GS; j++) {
                    const uint32_t s = min(unit_get<T>(&v, j) & SM, M);
                    if (j >= lo && j < hi) {
                        if (cnt && s != cur) {
                            atomicAdd(&my[cur], cnt);
                            cnt = 0;
                        }
                        cur = s; cnt++;
                    }
                }
                if (cnt)
                    atomicAdd(&my[cur], cnt);
            }
        }
        /* runs of equal keys among the lanes: a lane whose lower neighbour has another key heads a run that ends in front of the next
         * head.  Lanes that counted their granule themselves, or have none, have key -1 and form runs that nobody adds. */
        const int below = __shfl_up(key, 1);
        const bool head = lane == 0 || below != key;
        const unsigned long long above = (__ballot(head) >> lane) >> 1;
        const int run = above ? __ffsll(above) : 64 - lane;
        if (head && key >= 0)
            atomicAdd(&my[key], (uint32_t)(run * GS));
    }
    __syncthreads();
    uint32_t *res = a.res + ((size_t)pic * 3 + plane) * OH_HG_BINS;
    for (int b = t; b < bins; b += THREADS) {
        uint32_t c = 0;
        for (int w = 0; w < copies; w++)
            c += hist[w * bins + b];
        if (c)
            atomicAdd(&res[b], c);
    }
}

} // namespace

static_assert(sizeof(OhHistArgs) <= 4096, "kernel arguments");

extern "C" void ohk_histogram(const OhHistArgs *a, int n, hipStream_t st)
{
    const dim3 grid((unsigned)(a->k[0].tiles + (a->np - 1) * a->k[1].tiles), (unsigned)n);
    const size_t lds = (size_t)copies_of(a->bd) * sizeof(uint32_t) << a->bd;
    if (a->bd > 8)
        histogram_kernel<uint16_t><<<grid, THREADS, lds, st>>>(*a);
    else
        histogram_kernel<uint8_t><<<grid, THREADS, lds, st>>>(*a);
}
