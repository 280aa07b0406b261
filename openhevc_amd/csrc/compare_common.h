/*
 * compare_common.h — the SSIM window formula of DESIGN.md §3f, one function for the kernel (compare.hip) and for the host's
 * oh_compare_ssim_window (pics_math.hip), so that the CPU tests pin what the GPU evaluates.
 */
#ifndef OHEVC_COMPARE_COMMON_H
#define OHEVC_COMPARE_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* c1 and c2 of SSIM for 64-sample windows of samples up to M = 2^bit_depth - 1 */
__host__ __device__ inline void compare_ssim_consts(int bit_depth, int64_t *c1, int64_t *c2)
{
    const int64_t M = ((int64_t)1 << bit_depth) - 1;
    *c1 = (64 * M * M + 5000) / 10000;
    *c2 = (9 * 64 * 63 * M * M + 5000) / 10000;
}

/* One 8x8 window from s1 = sum a, s2 = sum b, ss = sum a^2 + sum b^2, s12 = sum ab: rint(n1 n2 / (d1 d2) 2^30).  The integers are exact
 * in 64 bits and, below 2^53, in binary64; what is left is two IEEE multiplications, one IEEE division, an exact scaling and a
 * round-half-to-even — no floating-point addition, so nothing for the compiler to contract into an FMA. */
__host__ __device__ inline int64_t compare_ssim_window(int64_t c1, int64_t c2, uint32_t s1_, uint32_t s2_, uint64_t ss_, uint64_t s12_)
{
    const int64_t s1 = s1_, s2 = s2_, ss = (int64_t)ss_, s12 = (int64_t)s12_;
    const int64_t vars = 64 * ss - s1 * s1 - s2 * s2, covar = 64 * s12 - s1 * s2;
    const int64_t n1 = 2 * s1 * s2 + c1, n2 = 2 * covar + c2, d1 = s1 * s1 + s2 * s2 + c1, d2 = vars + c2;
    const double num = (double)n1 * (double)n2, den = (double)d1 * (double)d2;
    return (int64_t)__builtin_rint(num / den * 1073741824.0);
}

#endif
