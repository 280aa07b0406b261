/*
 * filter_common.h — the sample formulas of DESIGN.md §3m, one function each for the kernel (filter.hip) and for the host's
 * oh_filter_unsharp / oh_filter_median9 / oh_filter_temporal (pics_math.hip), so that the CPU tests pin what the GPU evaluates.
 */
#ifndef OHEVC_FILTER_COMMON_H
#define OHEVC_FILTER_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ inline int32_t filter_abs(int32_t v) { return v < 0 ? -v : v; }
__host__ __device__ inline int32_t filter_min(int32_t a, int32_t b) { return a < b ? a : b; }
__host__ __device__ inline int32_t filter_max(int32_t a, int32_t b) { return a > b ? a : b; }
__host__ __device__ inline int32_t filter_clip(int32_t v, int32_t M) { return filter_min(filter_max(v, 0), M); }

/* a tap times a sample or a horizontal sum: legal taps (the sum of |tap| at most 512) and samples of at most 12 bit keep both factors
 * inside 24 signed bits (|tmp| <= 512 * 4095 < 2^23), which is what the device's multiplier takes at full rate */
__host__ __device__ inline int32_t filter_mul(int32_t tap, int32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(tap, v);
#else
    return tap * v;
#endif
}

/* CONVOLVE: the sum of both passes (taps of sum 256 on either axis) -> the sample; the one rounding */
__host__ __device__ inline int32_t filter_round(int32_t acc, int32_t M) { return filter_clip((acc + 32768) >> 16, M); }

/* UNSHARP: s the source sample, b the CONVOLVE output at its place; amount in 1/64 */
__host__ __device__ inline int32_t filter_unsharp(int32_t s, int32_t b, int32_t amount, int32_t threshold, int32_t M)
{
    const int32_t d = s - b;
    if (filter_abs(d) <= threshold)
        return s;
    return filter_clip(s + ((amount * d + 32) >> 6), M);
}

/* three samples in rising order */
__host__ __device__ inline void filter_sort3(int32_t a, int32_t b, int32_t c, int32_t &lo, int32_t &mid, int32_t &hi)
{
    const int32_t mn = filter_min(a, b), mx = filter_max(a, b);
    lo = filter_min(mn, c);
    hi = filter_max(mx, c);
    mid = filter_max(mn, filter_min(mx, c));
}

__host__ __device__ inline int32_t filter_med3(int32_t a, int32_t b, int32_t c)
{
    return filter_max(filter_min(a, b), filter_min(filter_max(a, b), c));
}

/* MEDIAN: the fifth smallest of nine samples given as three sorted columns (lo[i] <= mid[i] <= hi[i]): the median of the largest of
 * the three smallest, the median of the three middle ones and the smallest of the three largest */
__host__ __device__ inline int32_t filter_median_cols(const int32_t lo[3], const int32_t mid[3], const int32_t hi[3])
{
    return filter_med3(filter_max(filter_max(lo[0], lo[1]), lo[2]), filter_med3(mid[0], mid[1], mid[2]),
                       filter_min(filter_min(hi[0], hi[1]), hi[2]));
}

/* the same of nine samples in any order (v[3 i .. 3 i + 2] is taken as column i) */
__host__ __device__ inline int32_t filter_median9(const int32_t v[9])
{
    int32_t lo[3], mid[3], hi[3];
    for (int i = 0; i < 3; i++)
        filter_sort3(v[3 * i], v[3 * i + 1], v[3 * i + 2], lo[i], mid[i], hi[i]);
    return filter_median_cols(lo, mid, hi);
}

/* TEMPORAL: c / p / n the samples of cur / prev / next at one place, mp / mn the sums of absolute differences of the 3 x 3 windows of
 * prev and of next against cur */
__host__ __device__ inline int32_t filter_temporal(int32_t c, int32_t p, int32_t n, int32_t mp, int32_t mn, int32_t threshold)
{
    const int32_t ps = mp <= threshold ? p : c, ns = mn <= threshold ? n : c;
    return (ps + 2 * c + ns + 2) >> 2;
}

#endif
