/*
 * warp_common.h — the sample definition of DESIGN.md §3p, one function each for the kernel (warp.hip) and for the host's
 * oh_warp_position / oh_warp_cubic / oh_warp_interp / oh_warp_paths (pics_math.hip), so that the CPU tests pin what the GPU evaluates.
 * All position arithmetic is int64_t; >> of a negative value is an arithmetic shift (it floors), products stand where a left shift of
 * a negative value would.
 */
#ifndef OHEVC_WARP_COMMON_H
#define OHEVC_WARP_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

enum { WARP_NEAREST = 0, WARP_BILINEAR, WARP_BICUBIC };         /* OH_WARP_NEAREST .. OH_WARP_BICUBIC */
enum { WARP_TW = 64, WARP_TH = 16,                              /* the destination tile of one workgroup, plane samples */
       WARP_LDS = 16 << 10 };                                   /* bytes of staged source samples per workgroup */

__host__ __device__ inline int64_t warp_floor_div(int64_t a, int64_t b)        /* b > 0 */
{
    const int64_t q = a / b;
    return a % b < 0 ? q - 1 : q;
}

__host__ __device__ inline int64_t warp_clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

/* sample (x, y) of a plane of the image with shifts hs, vs -> its position in the source plane's window, Q16.  The caller has
 * checked the coefficients (and, PERSP, that the denominator is at least 2^20 over the image) */
template <bool PERSP>
__host__ __device__ inline void warp_position(const int64_t *m, int hs, int vs, int x, int y, int32_t *px, int32_t *py)
{
    const int64_t X = (int64_t)x << hs, Y = (int64_t)y << vs, h = vs;
    int64_t Lx = m[0] * X + m[1] * Y + m[2] + h * (m[1] >> 1);
    int64_t Ly = m[3] * X + m[4] * Y + m[5] + h * (m[4] >> 1);
    if (PERSP) {
        const int64_t D = (m[6] * X + m[7] * Y + m[8] + h * (m[7] >> 1)) >> 8;
        Lx = warp_floor_div(Lx * ((int64_t)1 << 22), D);
        Ly = warp_floor_div(Ly * ((int64_t)1 << 22), D);
    }
    const int64_t lo = -((int64_t)1 << 30), hi = ((int64_t)1 << 31) - 1;
    Lx = warp_clamp64(Lx, lo, hi);
    Ly = warp_clamp64(Ly, lo, hi);
    *px = (int32_t)(Lx >> hs);
    *py = (int32_t)((Ly - (int64_t)vs * 32768) >> vs);
}

/* a Q16 plane position -> the integer part and the fraction (1/64) that the filter takes */
__host__ __device__ inline void warp_split(int filter, int32_t p, int *i, int *f)
{
    if (filter == WARP_NEAREST) {
        *i = (int)(((int64_t)p + 32768) >> 16);
        *f = 0;
    } else {
        const int64_t q = ((int64_t)p + 512) >> 10;
        *i = (int)(q >> 6);
        *f = (int)(q & 63);
    }
}

/* Keys' cubic (a = -1/2) at phase f / 64: four taps that sum to 1024 */
__host__ __device__ inline void warp_cubic(int f, int32_t c[4])
{
    const int32_t f2 = f * f, f3 = f2 * f;
    const int32_t n0 = -f3 + 128 * f2 - 4096 * f, n1 = 3 * f3 - 320 * f2 + (1 << 19), n2 = -3 * f3 + 256 * f2 + 4096 * f, n3 = f3 - 64 * f2;
    c[0] = (n0 + 256) >> 9;
    c[3] = (n3 + 256) >> 9;
    if (f <= 32) {
        c[2] = (n2 + 256) >> 9;
        c[1] = 1024 - c[0] - c[2] - c[3];
    } else {
        c[1] = (n1 + 256) >> 9;
        c[2] = 1024 - c[0] - c[1] - c[3];
    }
}

/* the sample at integer part (ix, iy) and fraction (fx, fy): s(i, j) is the tap at plane index (i, j), border rule applied; M the
 * largest code value */
template <typename S>
__host__ __device__ inline int32_t warp_interp(int filter, S s, int ix, int iy, int fx, int fy, int32_t M)
{
    if (filter == WARP_NEAREST)
        return s(ix, iy);
    if (filter == WARP_BILINEAR) {
        const int32_t t0 = (64 - fx) * s(ix, iy) + fx * s(ix + 1, iy);
        const int32_t t1 = (64 - fx) * s(ix, iy + 1) + fx * s(ix + 1, iy + 1);
        return ((64 - fy) * t0 + fy * t1 + (1 << 11)) >> 12;
    }
    int32_t cx[4], cy[4], v = 0;
    warp_cubic(fx, cx);
    warp_cubic(fy, cy);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int32_t t = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            t += cx[k] * s(ix - 1 + k, iy - 1 + j);
        v += cy[j] * ((t + 8) >> 4);
    }
    v = (v + (1 << 15)) >> 16;
    return v < 0 ? 0 : v > M ? M : v;
}

/* The taps that the samples (xa .. xb) x (ya .. yb) of a plane of the image read, as a box of plane indices (unclamped: the border
 * rule comes after), from the positions of the four corners: the map carries the rectangle onto a convex quadrilateral, and the
 * integer part is monotonous in the position.  (The perspective form divides by a rounded denominator, so a sample in between may
 * step over the box by a little: the kernel checks every sample's taps against the box and gathers the strays from global memory.) */
struct WarpBox { int32_t x0, y0, x1, y1; };
template <bool PERSP>
__host__ __device__ inline WarpBox warp_tile_box(const int64_t *m, int hs, int vs, int filter, int xa, int ya, int xb, int yb)
{
    WarpBox b = { INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN };
    for (int k = 0; k < 4; k++) {
        int32_t px, py;
        int ix, iy, f;
        warp_position<PERSP>(m, hs, vs, k & 1 ? xb : xa, k & 2 ? yb : ya, &px, &py);
        warp_split(filter, px, &ix, &f);
        warp_split(filter, py, &iy, &f);
        b.x0 = ix < b.x0 ? ix : b.x0; b.x1 = ix > b.x1 ? ix : b.x1;
        b.y0 = iy < b.y0 ? iy : b.y0; b.y1 = iy > b.y1 ? iy : b.y1;
    }
    const int before = filter == WARP_BICUBIC ? 1 : 0, behind = filter == WARP_BICUBIC ? 2 : filter == WARP_BILINEAR ? 1 : 0;
    b.x0 -= before; b.y0 -= before;
    b.x1 += behind; b.y1 += behind;
    return b;
}

/* whether the workgroup stages the box (samples of sz bytes) in LDS; otherwise its lanes gather from global memory */
__host__ __device__ inline bool warp_box_staged(const WarpBox &b, int sz)
{
    return ((int64_t)b.x1 - b.x0 + 1) * ((int64_t)b.y1 - b.y0 + 1) * sz <= WARP_LDS;
}

/* the tile (tx, ty) of a destination plane of dw x dh samples whose image is iw x ih: the image samples its corners stand for */
__host__ __device__ inline void warp_tile_corners(int tx, int ty, int dw, int dh, int iw, int ih, int *xa, int *ya, int *xb, int *yb)
{
    const int X0 = tx * WARP_TW, Y0 = ty * WARP_TH;
    const int X1 = (X0 + WARP_TW < dw ? X0 + WARP_TW : dw) - 1, Y1 = (Y0 + WARP_TH < dh ? Y0 + WARP_TH : dh) - 1;
    *xa = X0 < iw - 1 ? X0 : iw - 1; *xb = X1 < iw - 1 ? X1 : iw - 1;
    *ya = Y0 < ih - 1 ? Y0 : ih - 1; *yb = Y1 < ih - 1 ? Y1 : ih - 1;
}

#endif
