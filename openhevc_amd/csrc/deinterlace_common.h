/*
 * deinterlace_common.h — the sample formulas of DESIGN.md §3l, one function each for the kernel (deinterlace.hip) and for the host's
 * oh_deint_adaptive (pics_math.hip), so that the CPU tests pin what the GPU evaluates.
 */
#ifndef OHEVC_DEINTERLACE_COMMON_H
#define OHEVC_DEINTERLACE_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ inline int32_t deint_abs(int32_t v) { return v < 0 ? -v : v; }
__host__ __device__ inline int32_t deint_min(int32_t a, int32_t b) { return a < b ? a : b; }
__host__ __device__ inline int32_t deint_max(int32_t a, int32_t b) { return a > b ? a : b; }

/* BOB: a missing sample from the kept samples above and below */
__host__ __device__ inline int32_t deint_bob(int32_t up, int32_t dn) { return (up + dn + 1) >> 1; }

/* BLEND: any sample from the rows above and below (clamped at the plane's edges) */
__host__ __device__ inline int32_t deint_blend(int32_t m1, int32_t c, int32_t p1) { return (m1 + 2 * c + p1 + 2) >> 2; }

/* LOWPASS5: a missing sample from rows y - 2 .. y + 2 (clamped); the shift of the signed sum is arithmetic; M = 2^bit_depth - 1 */
__host__ __device__ inline int32_t deint_lowpass5(int32_t m2, int32_t m1, int32_t c, int32_t p1, int32_t p2, int32_t M)
{
    const int32_t v = (-m2 + 4 * m1 + 2 * c + 4 * p1 - p2 + 4) >> 3;
    return deint_min(deint_max(v, 0), M);
}

/* score(j) of ADAPTIVE on the windows up[i] = C[up][cx(x - 3 + i)], dn[i] = C[dn][cx(x - 3 + i)] */
__host__ __device__ inline int32_t deint_score(const int32_t *up, const int32_t *dn, int j)
{
    return deint_abs(up[2 + j] - dn[2 - j]) + deint_abs(up[3 + j] - dn[3 - j]) + deint_abs(up[4 + j] - dn[4 - j]);
}

/* ADAPTIVE: a missing sample at column x of row y.  up / dn: seven kept samples of cur above and below, columns x - 3 .. x + 3
 * (clamped); a, b: row y of the two pictures that hold the other field before and after the kept one; pu, pd, nu, nd: column x of
 * the rows above and below in prev and next.  The spatial prediction sp is the mean of two samples along the best of five
 * directions (the straight one wins ties; a direction two columns off is tried only when the one next to it won); the temporal
 * one t is the mean of a and b; the result is sp held within diff of t, diff being the largest of three temporal differences.
 * No clip: sp and t are means of two samples, so both lie in [0, M], and clamping sp into [t - diff, t + diff] with diff >= 0
 * yields a value between sp and t. */
__host__ __device__ inline int32_t deint_adaptive(const int32_t *up, const int32_t *dn, int32_t a, int32_t b,
                                                  int32_t pu, int32_t pd, int32_t nu, int32_t nd)
{
    const int32_t c = up[3], e = dn[3];
    const int32_t t = (a + b) >> 1;
    const int32_t d0 = deint_abs(a - b);
    const int32_t d1 = (deint_abs(pu - c) + deint_abs(pd - e)) >> 1;
    const int32_t d2 = (deint_abs(nu - c) + deint_abs(nd - e)) >> 1;
    const int32_t diff = deint_max(deint_max(d0 >> 1, d1), d2);
    int32_t best = deint_score(up, dn, 0) - 1, sp = (c + e) >> 1;
#pragma unroll
    for (int s = -1; s <= 1; s += 2) {
        const int32_t s1 = deint_score(up, dn, s), s2 = deint_score(up, dn, 2 * s);
        if (s1 < best) {
            best = s1; sp = (up[3 + s] + dn[3 - s]) >> 1;
            if (s2 < best) { best = s2; sp = (up[3 + 2 * s] + dn[3 - 2 * s]) >> 1; }
        }
    }
    return deint_min(deint_max(sp, t - diff), t + diff);
}

#endif
