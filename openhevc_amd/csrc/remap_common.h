/*
 * remap_common.h — the sample definition of DESIGN.md §3r, one function each for the kernel (remap.hip) and for the host's
 * oh_remap_sample / oh_remap_luts (pics_math.hip), so that the CPU tests pin what the GPU evaluates.  Everything is int32_t, and >> of
 * a negative value is an arithmetic shift (it floors).
 */
#ifndef OHEVC_REMAP_COMMON_H
#define OHEVC_REMAP_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

enum { REMAP_COEFF_MIN = -32768, REMAP_COEFF_MAX = 32767,      /* a coefficient of the matrix */
       REMAP_DENOM_MAX = 15 };                                 /* log2 of its denominator */

/* one row of the matrix on the three pre-table values p (each 0 .. Mo <= 4095), rounded, shifted by d (0 .. REMAP_DENOM_MAX) and
 * clipped to 0 .. Mo.  The sum stays inside int32_t: |k0 p0 + k1 p1 + k2 p2 + r| <= 3 * 32768 * 4095 + 2^14 = 402571264 < 2^31 */
__host__ __device__ inline int32_t remap_row(const int32_t *k, int32_t p0, int32_t p1, int32_t p2, int d, int32_t Mo)
{
    const int32_t r = d ? 1 << (d - 1) : 0;
    const int32_t m = (k[0] * p0 + k[1] * p1 + k[2] * p2 + r) >> d;
    return m < 0 ? 0 : m > Mo ? Mo : m;
}

/* one sample: the three components s through the pre tables (2^bi entries each; a component above Mi is looked up by its low bits, so
 * that no read leaves a table), the matrix k (row-major 3 x 3), the post tables (Mo + 1 entries each).  IDENT: the matrix is the identity
 * (k[c][c] = 2^d, the others 0), which leaves the pre-table values as they are: they lie in 0 .. Mo */
template <bool IDENT, typename T>
__host__ __device__ inline void remap_sample(const T *pre0, const T *pre1, const T *pre2, const T *post0, const T *post1, const T *post2,
                                             const int32_t *k, int d, uint32_t Mi, int32_t Mo, const uint32_t s[3], uint32_t out[3])
{
    const int32_t p0 = pre0[s[0] & Mi], p1 = pre1[s[1] & Mi], p2 = pre2[s[2] & Mi];
    if (IDENT) {
        out[0] = post0[p0]; out[1] = post1[p1]; out[2] = post2[p2];
    } else {
        out[0] = post0[remap_row(k, p0, p1, p2, d, Mo)];
        out[1] = post1[remap_row(k + 3, p0, p1, p2, d, Mo)];
        out[2] = post2[remap_row(k + 6, p0, p1, p2, d, Mo)];
    }
}

#endif
