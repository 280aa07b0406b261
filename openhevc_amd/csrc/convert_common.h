/*
 * convert_common.h — what the kernels that read pictures as images share (convert.hip: oh_pics_convert; colour.hip: oh_pics_convert_colour;
 * light.hip: oh_pics_light_level), on top of pics_common.h: the image layouts and the output sample types, the chroma filter and the
 * integer matrix of DESIGN.md §3b.  Device code only.
 */
#ifndef OHEVC_CONVERT_COMMON_H
#define OHEVC_CONVERT_COMMON_H

#include "pics_common.h"

namespace {

enum { L_PLANAR, L_SEMI, L_RGBP, L_RGBI };          /* YUV planar, YUV semi-planar, RGB planar, RGB / RGBA interleaved */
enum { O_U8, O_U16, O_F16, O_F32 };                 /* output sample type */

template <int O> struct OutT { typedef uint8_t T; };
template <> struct OutT<O_U16> { typedef uint16_t T; };
template <> struct OutT<O_F16> { typedef uint16_t T; };
template <> struct OutT<O_F32> { typedef float T; };

/* the f16 nearest (ties to even) to a non-negative finite f32 below 65520, in integer arithmetic.  A plain conversion of the product
 * below is folded into one v_fma_mixlo_f16, which rounds the exact product to f16 once instead of rounding the f32 product. */
__device__ __forceinline__ uint16_t f16_rne(float f)
{
    const uint32_t x = __float_as_uint(f);
    if (!x)
        return 0;
    const int e = (int)(x >> 23) - 127 + 15;                  /* f16 biased exponent of a normal result */
    const uint32_t m = (x & 0x7FFFFF) | 0x800000;
    const int s = min(13 + max(0, 1 - e), 31);                /* significand bits that go: 13, more for a subnormal result */
    uint32_t q = m >> s;
    const uint32_t r = m & ((1u << s) - 1), half = 1u << (s - 1);
    q += (r > half || (r == half && (q & 1))) ? 1u : 0u;
    return (uint16_t)((e >= 1 ? (uint32_t)(e - 1) << 10 : 0u) + q);   /* a carry out of the significand raises the exponent */
}

/* an integer RGB value of D bits -> the output sample: u8 / u16 as is, F32 = value x (the f32 nearest to 1/65535), F16 = that f32
 * rounded to nearest-even */
template <int O>
__device__ __forceinline__ typename OutT<O>::T out_sample(int v)
{
    constexpr float K = 1.0f / 65535.0f;
    if constexpr (O == O_F32)
        return __fmul_rn((float)v, K);
    else if constexpr (O == O_F16)
        return f16_rne(__fmul_rn((float)v, K));
    else
        return (typename OutT<O>::T)v;
}

/* The source rows of one segment of an RGB image row in LDS: cnt luma samples from plane column X0 of plane row Y, and the chroma
 * rows the filter reads (4:2:0 linear: two).  lum holds CW * sizeof(TI) + 32 bytes; chr four rows of RB bytes (Cb row j0, Cb row j1,
 * Cr row j0, Cr row j1), RB >= (CW / 2 + 1) * sizeof(TI) + 32 and a multiple of 16 — 4:4:4 takes two of them per row. */
template <typename TI>
struct RgbRows {
    const TI *L, *U0, *U1, *V0, *V1;                            /* the staged rows, each at the first sample of the segment */
    int c_lo;                                                   /* the chroma column U0[0] holds */

    __device__ __forceinline__ void stage_rows(const OhConvArgs &a, int pic, int X0, int Y, int cnt, uint8_t *lum, uint8_t *chr, int RB)
    {
        const int hs = a.cf == 1 || a.cf == 2, vs = a.cf == 1;
        const int bl = stage<TI>(lum, (const uint8_t *)a.src[pic][0] + (size_t)Y * a.pitch[0] + (size_t)X0 * sizeof(TI), cnt);
        int bu0 = 0, bu1 = 0, bv0 = 0, bv1 = 0;
        c_lo = 0;
        if (a.cf) {
            c_lo = X0 >> hs;
            const int m = min((X0 + cnt) >> hs, a.cw - 1) - c_lo + 1;                    /* with the right neighbour of the linear filter */
            const int j0 = Y >> vs;
            bu0 = stage<TI>(chr, (const uint8_t *)a.src[pic][1] + (size_t)j0 * a.pitch[1] + (size_t)c_lo * sizeof(TI), m);
            bv0 = stage<TI>(chr + 2 * RB, (const uint8_t *)a.src[pic][2] + (size_t)j0 * a.pitch[2] + (size_t)c_lo * sizeof(TI), m);
            if (a.filter && vs) {                               /* chroma row j sits between luma rows 2j and 2j + 1 */
                const int j1 = min(max(j0 - 1 + 2 * (Y & 1), 0), a.ch - 1);
                bu1 = stage<TI>(chr + RB, (const uint8_t *)a.src[pic][1] + (size_t)j1 * a.pitch[1] + (size_t)c_lo * sizeof(TI), m);
                bv1 = stage<TI>(chr + 3 * RB, (const uint8_t *)a.src[pic][2] + (size_t)j1 * a.pitch[2] + (size_t)c_lo * sizeof(TI), m);
            }
        }
        L = (const TI *)lum + bl;
        U0 = (const TI *)chr + bu0; U1 = (const TI *)(chr + RB) + bu1;
        V0 = (const TI *)(chr + 2 * RB) + bv0; V1 = (const TI *)(chr + 3 * RB) + bv1;
    }

    /* Cb and Cr on the luma grid at sample i of the segment (plane column X): chroma in coded-plane coordinates, clamped at the
     * coded plane's edges; mid where the picture has no chroma */
    __device__ __forceinline__ void chroma(const OhConvArgs &a, int X, int i, int mid, int &u, int &v) const
    {
        u = mid; v = mid;
        if (a.cf == 3) {
            u = U0[i]; v = V0[i];
        } else if (a.cf) {
            const int k = (X >> 1) - c_lo, k2 = (X & 1) ? min((X + 1) >> 1, a.cw - 1) - c_lo : k;
            if (!a.filter) {
                u = U0[k]; v = V0[k];
            } else {
                const int hu = U0[k] + U0[k2], hv = V0[k] + V0[k2];                        /* 2x scale */
                if (a.cf == 1) {
                    u = (3 * hu + U1[k] + U1[k2] + 4) >> 3;
                    v = (3 * hv + V1[k] + V1[k2] + 4) >> 3;
                } else {
                    u = (hu + 1) >> 1;
                    v = (hv + 1) >> 1;
                }
            }
        }
    }
};

/* the integer matrix with the coefficients of oh_convert_coeffs: R, G, B of k[8] bits */
struct RgbMatrix {
    int cy, crv, cgu, cgv, cbu, yoff, mid, S, rnd, mx;
    __device__ __forceinline__ explicit RgbMatrix(const int32_t *k)
        : cy(k[0]), crv(k[1]), cgu(k[2]), cgv(k[3]), cbu(k[4]), yoff(k[5]), mid(k[6]), S(k[7]), rnd(1 << (k[7] - 1)), mx((1 << k[8]) - 1) {}
    __device__ __forceinline__ void rgb(int y, int u, int v, int &R, int &G, int &B) const
    {
        const int dy = cy * (y - yoff) + rnd, du = u - mid, dv = v - mid;
        R = min(max((dy + crv * dv) >> S, 0), mx);
        G = min(max((dy + cgu * du + cgv * dv) >> S, 0), mx);
        B = min(max((dy + cbu * du) >> S, 0), mx);
    }
};

} // namespace

#endif
