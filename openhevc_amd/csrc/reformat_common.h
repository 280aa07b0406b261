/*
 * reformat_common.h — the one quantisation of DESIGN.md §3j, one definition for the kernel (reformat.hip) and for the host's
 * oh_reformat_quantise (pics_math.hip), so that the CPU tests pin what the GPU evaluates.
 */
#ifndef OHEVC_REFORMAT_COMMON_H
#define OHEVC_REFORMAT_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* a row of the 4 x 4 ordered-dither matrix B4 as four nibbles: B4[y][x] = (row y >> 4 x) & 15 */
#define REFORMAT_B4_ROW(a, b, c, d) ((uint32_t)(a) | (uint32_t)(b) << 4 | (uint32_t)(c) << 8 | (uint32_t)(d) << 12)

/* a weighted sum of source samples whose weights total 2^f, of a source of Bs bits -> the destination sample of Bd bits, s = f + Bs - Bd:
 * up by -s bits, or down by s bits with one rounding — to nearest (mode 0, OH_RF_ROUND), or with the offset of the sample's place in
 * its 4 x 4 tile (mode 1, OH_RF_DITHER: every offset 0 .. 2^s - 1 equally often for s <= 4) — then the clamp at the top.  sum is at
 * most 8 * 4095 and s at most 7, so every term fits 32 bits. */
__host__ __device__ inline int32_t reformat_quantise(int32_t sum, int s, int mode, int x, int y, int bd)
{
    const int32_t mx = (1 << bd) - 1;
    if (s <= 0) {
        const int32_t v = sum << -s;
        return v < mx ? v : mx;
    }
    int32_t r = 1 << (s - 1);
    if (mode) {
        const uint32_t row = (y & 2) ? ((y & 1) ? REFORMAT_B4_ROW(15, 7, 13, 5) : REFORMAT_B4_ROW(3, 11, 1, 9))
                                     : ((y & 1) ? REFORMAT_B4_ROW(12, 4, 14, 6) : REFORMAT_B4_ROW(0, 8, 2, 10));
        const int32_t t = (int32_t)((row >> (4 * (x & 3))) & 15);
        r = ((2 * t + 1) << s) >> 5;
    }
    const int32_t v = (sum + r) >> s;
    return v < mx ? v : mx;
}

#endif
