/*
 * compose_common.h — the two integer formulas of DESIGN.md §3h, one definition for the kernel (compose.hip) and for the host's
 * oh_compose_blend / oh_compose_chroma_alpha (pics_math.hip), so that the CPU tests pin what the GPU evaluates.
 */
#ifndef OHEVC_COMPOSE_COMMON_H
#define OHEVC_COMPOSE_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* the weight of a sample is alpha (0 .. 255) times opacity (0 .. 256): 0 .. COMPOSE_ONE */
#define COMPOSE_ONE 65280u
/* 2^47 / 65280 + 1: x * COMPOSE_RCP >> 47 == x / 65280 for every x up to 4095 * 65280 + 32640 < 2^28 (the rounded-up reciprocal adds
 * less than x / 2^47 < 2^-19 to the quotient, below the 1 / 65280 that the fraction of a quotient lacks at least to the next integer);
 * the constant fits 32 bits, so the kernel's division is the high half of one 32 x 32 multiplication and a shift by 15 */
#define COMPOSE_RCP 2155905153ull

/* source over destination in code values: (src w + dst (65280 - w) + 32640) / 65280 with w = alpha opacity.  w = 0 gives dst, w = 65280
 * gives src, anything else a value between the two.  Samples of at most 12 bits: the numerator stays below 2^28. */
__host__ __device__ inline uint32_t compose_blend(uint32_t dst, uint32_t src, uint32_t alpha, uint32_t opacity)
{
    const uint32_t w = alpha * opacity;
    const uint32_t x = src * w + dst * (COMPOSE_ONE - w) + COMPOSE_ONE / 2;
    return (uint32_t)(((uint64_t)x * COMPOSE_RCP) >> 47);
}

/* the alpha of a chroma sample from the luma alphas it covers: a00 a01 on the upper luma row, a10 a11 on the lower one.  4:2:0 the
 * rounded mean of the four, 4:2:2 of the upper two, 4:4:4 (and anything else) a00 */
__host__ __device__ inline uint32_t compose_chroma_alpha(int chroma_format_idc, uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11)
{
    if (chroma_format_idc == 1)
        return (a00 + a01 + a10 + a11 + 2) >> 2;
    if (chroma_format_idc == 2)
        return (a00 + a01 + 1) >> 1;
    return a00;
}

#endif
