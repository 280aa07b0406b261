/*
 * grain_common.h — the sample definition of DESIGN.md §3q, one function each for the kernel (grain.hip) and for the host's
 * oh_grain_hash / oh_grain_block / oh_grain_mean / oh_grain_value / oh_grain_smooth / oh_grain_blend (pics_math.hip), so that the CPU
 * tests pin what the GPU evaluates.  The hash is uint32_t arithmetic (it wraps); everything else is int32_t, and >> of a negative value
 * is an arithmetic shift (it floors).
 */
#ifndef OHEVC_GRAIN_COMMON_H
#define OHEVC_GRAIN_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

enum { GRAIN_CUT_MIN = 2, GRAIN_CUT_MAX = 14,                  /* the cut-offs of a pattern, sixteenths of the band */
       GRAIN_CUTS = GRAIN_CUT_MAX - GRAIN_CUT_MIN + 1,         /* 13 each way: 169 patterns */
       GRAIN_PAT = 32,                                         /* a pattern is GRAIN_PAT x GRAIN_PAT int8 */
       GRAIN_BLOCK = 8,                                        /* a block of a plane: one mean, one offset, one sign */
       GRAIN_OFFSETS = GRAIN_PAT - GRAIN_BLOCK + 1,            /* 25 positions of a block in a pattern each way */
       GRAIN_TW = 32 };                                        /* blocks across the tile of one workgroup (grain.hip) */

__host__ __device__ inline uint32_t grain_fmix(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

__host__ __device__ inline uint32_t grain_hash(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    return grain_fmix(a ^ grain_fmix(b ^ grain_fmix(c ^ grain_fmix(d ^ 0x9e3779b9u))));
}

/* the sum of the four bytes of h, centred: -510 .. 510 */
__host__ __device__ inline int32_t grain_gauss(uint32_t h)
{
    return (int32_t)((h & 255) + (h >> 8 & 255) + (h >> 16 & 255) + (h >> 24)) - 510;
}

/* pattern (fh, fv), both in GRAIN_CUT_MIN .. GRAIN_CUT_MAX, among the 169 */
__host__ __device__ inline int grain_pattern_index(int fh, int fv) { return (fh - GRAIN_CUT_MIN) * GRAIN_CUTS + (fv - GRAIN_CUT_MIN); }

/* the 8-bit mean of a block of n = 64, 32 or 16 samples of bd bits that sum to `sum` */
__host__ __device__ inline int32_t grain_mean(uint32_t sum, int n, int bd) { return (int32_t)((sum + (uint32_t)(n >> 1)) / (uint32_t)n) >> (bd - 8); }

/* block (bx, by) of plane c of a picture with that seed: where it lies in its pattern, and whether the pattern is negated */
__host__ __device__ inline void grain_block(uint32_t seed, int c, int bx, int by, int *ox, int *oy, int *negate)
{
    const uint32_t h = grain_hash(2, seed, (uint32_t)c, (uint32_t)by * 65536u + (uint32_t)bx);
    *ox = (int)(((h & 0xFFFF) * GRAIN_OFFSETS) >> 16);
    *oy = (int)(((h >> 16 & 0x7FFF) * GRAIN_OFFSETS) >> 15);
    *negate = (int)(h >> 31);
}

/* a block as the kernel keeps it: the table entry (16 bits), then ox (5), oy (5), negate (1) */
__host__ __device__ inline uint32_t grain_desc(uint32_t entry, int ox, int oy, int negate)
{
    return (entry & 0xFFFF) | (uint32_t)ox << 16 | (uint32_t)oy << 21 | (uint32_t)negate << 26;
}

/* the grain of one sample before smoothing: p the (signed) pattern value */
__host__ __device__ inline int32_t grain_value(int32_t sigma, int32_t p, int bd, int log2_scale)
{
    return (sigma * p * (1 << (bd - 8)) + (1 << (4 + log2_scale))) >> (5 + log2_scale);
}

/* across a block edge: the sample, its neighbour in its own block and the one in the other block, all unsmoothed */
__host__ __device__ inline int32_t grain_smooth(int32_t left, int32_t g, int32_t right) { return (left + 2 * g + right + 2) >> 2; }

__host__ __device__ inline int32_t grain_blend(int32_t s, int32_t g, int bd, int blending)
{
    const int32_t M = (1 << bd) - 1;
    const int32_t v = blending ? s + ((s * g + (1 << (bd - 1))) >> bd) : s + g;
    return v < 0 ? 0 : v > M ? M : v;
}

#endif
