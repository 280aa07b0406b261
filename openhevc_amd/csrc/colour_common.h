/*
 * colour_common.h — what the kernels that go through the source curve share (colour.hip: oh_pics_convert_colour; light.hip:
 * oh_pics_light_level): stage 1 of DESIGN.md §3d and the products of the norm.  Device code only.
 */
#ifndef OHEVC_COLOUR_COMMON_H
#define OHEVC_COLOUR_COMMON_H

#include "convert_common.h"

namespace {

constexpr int FS = 1 << 30;                                    /* full scale of linear light */

/* 32 x 32 -> 64 bit products as one v_mad_i64_i32 / v_mad_u64_u32 each (the u form where both factors are known not negative) */
__device__ __forceinline__ int64_t mul64(int a, int b) { return (int64_t)a * (int64_t)b; }
__device__ __forceinline__ uint64_t mulu64(int a, int b) { return (uint64_t)(uint32_t)a * (uint64_t)(uint32_t)b; }

/* stage 1: a 16-bit code through the source curve.  A does not decrease and steps by less than 2^24 (oh_colour_tables refuses a curve
 * that would not): the product is a full-rate 24-bit multiply. */
__device__ __forceinline__ int src_curve(const int32_t *A, int v)
{
    const int i = v >> 4, f = v & 15, t0 = A[i], t1 = A[i + 1];
    return min(t0 + (int)((__umul24((unsigned)(t1 - t0), (unsigned)f) + 8u) >> 4), FS);
}

/* the luminance of stage 2's norm: Q14 weights that sum to 2^14 */
__device__ __forceinline__ int luma_norm_of(int wr, int wg, int wb, int l0, int l1, int l2)
{
    return (int)((mulu64(wr, l0) + mulu64(wg, l1) + mulu64(wb, l2) + (1u << 13)) >> 14);
}

} // namespace

#endif
