/*
 * pics_common.h — what the picture-service kernels share (orient, reformat, deinterlace, filter, warp, lut, remap, histogram, grain,
 * compare, compose, motion .hip, and through convert_common.h the kernels that read pictures as images): the workgroup size, the LDS
 * address space, staging of source rows into LDS as 16-byte granules and the aligned store of an LDS image of the destination bytes,
 * the samples of a granule, the map from a grid index to a plane, the units of OH_LUT_UNIT samples and the dispatch on a pair of bit
 * depths.  A new service starts from this header.  Device code only, but for the dispatcher of the launchers.
 */
#ifndef OHEVC_PICS_COMMON_H
#define OHEVC_PICS_COMMON_H

#include "../../include/ohevc_hip.h"
#include "kernels_common.h"

#define LDS __attribute__((address_space(3)))     /* what a kernel staged: say so, or reads through pointers picked at run time turn flat */

namespace {

constexpr int THREADS = 256;

/* n samples of type T at p (a plane row in HBM) -> LDS at lds, as the 16-byte granules that cover them; returns the index (in T) of
 * p[0] in lds.  lds must hold n * sizeof(T) + 30 bytes. */
template <typename T>
__device__ __forceinline__ int stage(uint8_t *lds, const void *p, int n)
{
    const uintptr_t a = (uintptr_t)p, a0 = a & ~(uintptr_t)15, a1 = (a + (uintptr_t)n * sizeof(T) + 15) & ~(uintptr_t)15;
    const int g = (int)((a1 - a0) >> 4);
    for (int i = threadIdx.x; i < g; i += THREADS)
        *(uint4v *)(lds + 16 * i) = *(const GLOBAL uint4v *)(a0 + 16 * (uintptr_t)i);
    return (int)((a - a0) / sizeof(T));
}

/* nbytes bytes to dst from img, the LDS image that holds the byte for dst + i at img[(dst & 15) + i] */
__device__ __forceinline__ void store_out(uint8_t *dst, const uint8_t *img, int nbytes)
{
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)nbytes, a0 = (d0 + 15) & ~(uintptr_t)15, a1 = d1 & ~(uintptr_t)15;
    const int o = (int)(d0 & 15), t = threadIdx.x;
    if (a0 >= a1) {
        for (int i = t; i < nbytes; i += THREADS)
            G_MUT(uint8_t, dst)[i] = img[o + i];
        return;
    }
    const int head = (int)(a0 - d0), tail = (int)(d1 - a1), g = (int)((a1 - a0) >> 4);
    if (t < head)
        G_MUT(uint8_t, dst)[t] = img[o + t];
    else if (t >= 64 && t - 64 < tail)
        G_MUT(uint8_t, a1)[t - 64] = img[o + (int)(a1 - d0) + t - 64];
    for (int i = t; i < g; i += THREADS)                        /* img + o + head is 16-byte aligned: o + head is 0 or 16 */
        *(GLOBAL uint4v *)(a0 + 16 * (uintptr_t)i) = *(const uint4v *)(img + o + head + 16 * i);
}

/* the samples of a 16-byte granule */
template <typename T>
struct Samples {
    static constexpr int GS = 16 / (int)sizeof(T);
    T s[GS];
    __device__ __forceinline__ explicit Samples(uint4v v) { __builtin_memcpy(s, &v, sizeof(v)); }
    __device__ __forceinline__ Samples() {}
    __device__ __forceinline__ uint4v granule() const { uint4v v; __builtin_memcpy(&v, s, sizeof(v)); return v; }
};

/* A grid dimension that runs over the units (rows, row groups, tiles) of all planes of a picture: those of plane 0, then those of
 * planes 1 and 2; per[q]: units per plane of class q (0 luma, 1 chroma).  The plane (c, class q) and the unit of it that index r
 * stands for.  A launch of one plane has no index at or beyond per[0]. */
__device__ __forceinline__ int grid_row(int r, const int per[2], int &c, int &q)
{
    c = 0; q = 0;
    if (r < per[0])
        return r;
    r -= per[0];
    q = 1; c = r < per[1] ? 1 : 2;
    return r - (c - 1) * per[1];
}

/* A unit of OH_LUT_UNIT samples of type T, what a lane of lut.hip and remap.hip takes at a time, as whole granules in registers:
 * N granules, samples of B bits, P of them in a dword */
template <typename T>
struct Unit {
    static constexpr int N = OH_LUT_UNIT * (int)sizeof(T) / 16, B = 8 * (int)sizeof(T), P = 4 / (int)sizeof(T);
};

/* sample j of the granules g, in the low B bits of what is returned: the bits above are the caller's to mask */
template <typename T>
__device__ __forceinline__ uint32_t unit_get(const uint4v *g, int j)
{
    return g[j / Unit<T>::P / 4][j / Unit<T>::P % 4] >> (Unit<T>::B * (j % Unit<T>::P));
}

/* v (of B bits) becomes sample j of the granules g, which started as zeros */
template <typename T>
__device__ __forceinline__ void unit_put(uint4v *g, int j, uint32_t v)
{
    g[j / Unit<T>::P / 4][j / Unit<T>::P % 4] |= v << (Unit<T>::B * (j % Unit<T>::P));
}

/* host: f(TI(), TS()) with the stored sample types of a source of sbd and a destination of dbd bits */
template <typename F>
void with_sample_types(int sbd, int dbd, F f)
{
    if (sbd == 8) {
        if (dbd == 8) f(uint8_t(), uint8_t());
        else          f(uint8_t(), uint16_t());
    } else {
        if (dbd == 8) f(uint16_t(), uint8_t());
        else          f(uint16_t(), uint16_t());
    }
}

} // namespace

#endif
