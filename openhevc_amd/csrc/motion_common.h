/*
 * motion_common.h — the sample formulas of DESIGN.md §3o, one function each for the kernels (motion.hip) and for the host's
 * oh_motion_qpel / oh_motion_epel / oh_motion_cost (pics_math.hip), so that the CPU tests pin what the GPU evaluates.
 */
#ifndef OHEVC_MOTION_COMMON_H
#define OHEVC_MOTION_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* H.265 table 8-11 (luma, quarter samples) and table 8-12 (chroma, eighth samples); row 0 is the sample itself */
__host__ __device__ inline int32_t motion_tap(int taps, int frac, int k)
{
    constexpr int8_t qpel[4][8] = { { 0, 0, 0, 64, 0, 0, 0, 0 }, { -1, 4, -10, 58, 17, -5, 1, 0 }, { -1, 4, -11, 40, 40, -11, 4, -1 },
                                    { 0, 1, -5, 17, 58, -10, 4, -1 } };
    constexpr int8_t epel[8][4] = { { 0, 64, 0, 0 }, { -2, 58, 10, -2 }, { -4, 54, 16, -2 }, { -6, 46, 28, -4 }, { -4, 36, 36, -4 },
                                    { -4, 28, 46, -6 }, { -2, 16, 54, -4 }, { -2, 10, 58, -2 } };
    return taps == 8 ? qpel[frac][k] : epel[frac][k];
}

/* the 14-bit prediction value -> the sample: the rounding of the uni-predicted case */
__host__ __device__ inline int32_t motion_round(int32_t v, int bd)
{
    const int shift = 14 - bd, M = (1 << bd) - 1;
    v = (v + (1 << (shift - 1))) >> shift;
    return v < 0 ? 0 : v > M ? M : v;
}

/* the predicted sample from a window of TAPS x TAPS reference samples: win[j * pitch + i] is the sample of row yInt - (TAPS / 2 - 1)
 * + j and column xInt - (TAPS / 2 - 1) + i; W: any pointer to samples.  The horizontal stage of the two-stage case is held in 16 bits,
 * as in the reference, which depths up to 12 never overflow (|88 * 4095| >> 4 < 2^15). */
template <int TAPS, typename W>
__host__ __device__ static inline int32_t motion_sample(W win, int pitch, int fx, int fy, int bd)
{
    constexpr int B = TAPS / 2 - 1;
    if (!fx && !fy)
        return motion_round((int32_t)win[B * pitch + B] << (14 - bd), bd);
    if (!fy) {
        int32_t s = 0;
#pragma unroll
        for (int k = 0; k < TAPS; k++)
            s += motion_tap(TAPS, fx, k) * (int32_t)win[B * pitch + k];
        return motion_round(s >> (bd - 8), bd);
    }
    if (!fx) {
        int32_t s = 0;
#pragma unroll
        for (int k = 0; k < TAPS; k++)
            s += motion_tap(TAPS, fy, k) * (int32_t)win[k * pitch + B];
        return motion_round(s >> (bd - 8), bd);
    }
    int32_t s = 0;
#pragma unroll
    for (int j = 0; j < TAPS; j++) {
        int32_t r = 0;
#pragma unroll
        for (int k = 0; k < TAPS; k++)
            r += motion_tap(TAPS, fx, k) * (int32_t)win[j * pitch + k];
        s += motion_tap(TAPS, fy, j) * (int32_t)(int16_t)(r >> (bd - 8));
    }
    return motion_round(s >> 6, bd);
}

__host__ __device__ inline int32_t motion_abs(int32_t v) { return v < 0 ? -v : v; }

/* d(mv) of a vector whose distance from four times the centre is (dx, dy), and the rate term of the cost.  The search keeps |dx|, |dy|
 * at most 4 * OH_MOTION_MAX_RANGE + 3 */
__host__ __device__ inline int32_t motion_dist(int32_t dx, int32_t dy) { return motion_abs(dx) + motion_abs(dy); }
__host__ __device__ inline uint32_t motion_cost(uint32_t sad, int32_t d, int32_t lambda) { return sad + (uint32_t)((lambda * d) >> 2); }

/* the key (cost, d, mvy, mvx) in one word that orders as the tuple does: the components of mv are taken relative to four times the
 * centre, which all candidates of a block share.  cost < 2^28 (a SAD of at most 256 * 4095 and a rate of at most 4096 * 262 / 4),
 * d < 2^9, |dx|, |dy| < 2^8 */
__host__ __device__ inline uint64_t motion_key(uint32_t cost, int32_t dx, int32_t dy)
{
    return (uint64_t)cost << 27 | (uint64_t)motion_dist(dx, dy) << 18 | (uint64_t)(dy + 256) << 9 | (uint64_t)(dx + 256);
}
__host__ __device__ inline int32_t motion_key_dx(uint64_t key) { return (int32_t)(key & 511) - 256; }
__host__ __device__ inline int32_t motion_key_dy(uint64_t key) { return (int32_t)(key >> 9 & 511) - 256; }
__host__ __device__ inline uint32_t motion_key_cost(uint64_t key) { return (uint32_t)(key >> 27); }

#endif
