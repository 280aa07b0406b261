/*
 * packing_common.h — the sample definition of DESIGN.md §3s (frame packing: the two views of a stereo pair in one picture), one
 * function each for the kernels (packing.hip) and for the host's oh_packing_sample / oh_packing_pack_sample (pics_math.hip), so that
 * the CPU tests pin what the GPU evaluates.  Everything is per plane and in the plane's own coordinates; everything is int32_t, and >>
 * of a negative value is an arithmetic shift (it floors).
 *
 * In a plane, view v occupies the rectangle R_v of cw x ch samples: the left (side by side) or top (top-bottom) half for v = 0, the
 * other half for v = 1.  C_v[y][x] is R_v read with the flip undone.  The functions take the samples through an accessor, so that the
 * kernel reads what it staged in LDS and the host reads a plane in memory:
 *   unpack   at(ry, rx)     the stored sample (rx, ry) of R_v, 0 <= rx < cw, 0 <= ry < ch
 *   pack     at(v, sy, sx)  the sample (sx, sy) of view v's plane, inside its window of vw x vh
 * pk_unpack_box / pk_pack_box say which samples the outputs of a run of one row read: what a workgroup stages.
 */
#ifndef OHEVC_PACKING_COMMON_H
#define OHEVC_PACKING_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "up_taps.h"

#define PK_HD __host__ __device__ inline

/* how the position of an output sample on the packed axis follows from its index Z and the grid position g (1/16 of the spacing of
 * the stored samples): the plane is not sub-sampled on that axis, p = 8 Z - g; a sub-sampled horizontal axis, co-sited chroma,
 * p = (16 Z - g + 1) >> 1; a sub-sampled vertical axis, chroma midway between two luma rows (chroma_sample_loc_type 0),
 * p = (16 Z - g - 3) >> 1 */
enum { PK_POS_PLAIN = 0, PK_POS_COSITED, PK_POS_MIDWAY };

/* one plane class (0 luma, 1 chroma) of a call */
struct PkPlane {
    int32_t sbs;                      /* 1 side by side, 0 top-bottom */
    int32_t quincunx;
    int32_t full;                     /* the views are of full size */
    int32_t taps;                     /* 8 luma, 4 chroma */
    int32_t pos;                      /* PK_POS_* */
    int32_t cw, ch;                   /* R_v and C_v: half the packed plane */
    int32_t vw, vh;                   /* the window of a view's plane: cw x ch, or with `full` the packed plane's size */
    int32_t maxv;                     /* 2^bit_depth - 1 */
};

PK_HD int pk_min(int a, int b) { return a < b ? a : b; }
PK_HD int pk_max(int a, int b) { return a > b ? a : b; }
PK_HD int pk_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

PK_HD int pk_pos(int kind, int Z, int g)
{
    return kind == PK_POS_PLAIN ? 8 * Z - g : kind == PK_POS_COSITED ? (16 * Z - g + 1) >> 1 : (16 * Z - g - 3) >> 1;
}

/* tap k of phase ph: the SHVC tables of up_taps.h */
PK_HD int pk_tap(int taps, int ph, int k)
{
    static constexpr int8_t luma[16][8] = { UP_TAPS_LUMA_ROWS };
    static constexpr int8_t chroma[16][4] = { UP_TAPS_CHROMA_ROWS };
    return taps == 8 ? luma[ph][k] : chroma[ph][k];
}

/* C_v[y][x] */
template <typename A>
PK_HD int pk_c(const PkPlane &pl, int flip, A at, int y, int x)
{
    return pl.sbs ? at(y, flip ? pl.cw - 1 - x : x) : at(flip ? pl.ch - 1 - y : y, x);
}

/* the unrounded sum S of the up-sampler at index Z of the packed axis, the other coordinate being o */
template <typename A>
PK_HD int pk_filter_sum(const PkPlane &pl, int flip, int g, int Z, int o, A at)
{
    const int N = pl.sbs ? pl.cw : pl.ch, p = pk_pos(pl.pos, Z, g), i = (p >> 4) - (pl.taps == 8 ? 3 : 1), ph = p & 15;
    int s = 0;
    for (int k = 0; k < pl.taps; k++) {
        const int j = pk_clamp(i + k, 0, N - 1);              /* the view's own samples: never across the seam */
        s += pk_tap(pl.taps, ph, k) * (pl.sbs ? pk_c(pl, flip, at, o, j) : pk_c(pl, flip, at, j, o));
    }
    return s;
}

/* sample (X, Y) of the coded plane of view v, made from the packed plane */
template <typename A>
PK_HD int pk_unpack_sample(const PkPlane &pl, int v, int flip, int g, int X, int Y, A at)
{
    X = pk_min(X, pl.vw - 1); Y = pk_min(Y, pl.vh - 1);         /* behind the window: its last column and row again */
    if (!pl.full)
        return pk_c(pl, flip, at, Y, X);
    if (pl.quincunx) {
        /* side by side: C_v[y][x] is the full-resolution sample (2 x + ((y + v) & 1), y); top-bottom: (x, 2 y + ((x + v) & 1)) */
        if (!((X ^ Y ^ v) & 1))
            return pl.sbs ? pk_c(pl, flip, at, Y, X >> 1) : pk_c(pl, flip, at, Y >> 1, X);
        const int xl = X > 0 ? X - 1 : X + 1, xr = X + 1 < pl.vw ? X + 1 : X - 1;      /* outside the plane: the opposite neighbour */
        const int yu = Y > 0 ? Y - 1 : Y + 1, yd = Y + 1 < pl.vh ? Y + 1 : Y - 1;
        int s;
        if (pl.sbs)
            s = pk_c(pl, flip, at, Y, xl >> 1) + pk_c(pl, flip, at, Y, xr >> 1) + pk_c(pl, flip, at, yu, X >> 1) + pk_c(pl, flip, at, yd, X >> 1);
        else
            s = pk_c(pl, flip, at, Y >> 1, xl) + pk_c(pl, flip, at, Y >> 1, xr) + pk_c(pl, flip, at, yu >> 1, X) + pk_c(pl, flip, at, yd >> 1, X);
        return (s + 2) >> 2;
    }
    const int s = pl.sbs ? pk_filter_sum(pl, flip, g, X, Y, at) : pk_filter_sum(pl, flip, g, Y, X, at);
    return pk_clamp((s + 32) >> 6, 0, pl.maxv);
}

/* the samples of R_v that outputs X0 .. X1 of row Y of view v read: rows ry[0] .. ry[1] (at most 8), columns rx[0] .. rx[1] */
PK_HD void pk_unpack_box(const PkPlane &pl, int flip, int g, int X0, int X1, int Y, int ry[2], int rx[2])
{
    X0 = pk_min(X0, pl.vw - 1); X1 = pk_min(X1, pl.vw - 1); Y = pk_min(Y, pl.vh - 1);
    int x0 = X0, x1 = X1, y0 = Y, y1 = Y;                        /* in C_v */
    if (pl.full && pl.quincunx) {
        x0 = pk_max(X0 - 1, 0); x1 = pk_min(X1 + 1, pl.vw - 1);
        y0 = pk_max(Y - 1, 0); y1 = pk_min(Y + 1, pl.vh - 1);
        if (pl.sbs) { x0 >>= 1; x1 >>= 1; }
        else        { y0 >>= 1; y1 >>= 1; }
    } else if (pl.full) {
        const int off = pl.taps == 8 ? 3 : 1;
        if (pl.sbs) {
            x0 = pk_clamp((pk_pos(pl.pos, X0, g) >> 4) - off, 0, pl.cw - 1);
            x1 = pk_clamp((pk_pos(pl.pos, X1, g) >> 4) - off + pl.taps - 1, 0, pl.cw - 1);
        } else {
            y0 = pk_clamp((pk_pos(pl.pos, Y, g) >> 4) - off, 0, pl.ch - 1);
            y1 = pk_clamp((pk_pos(pl.pos, Y, g) >> 4) - off + pl.taps - 1, 0, pl.ch - 1);
        }
    }
    if (flip && pl.sbs) { const int t = x0; x0 = pl.cw - 1 - x1; x1 = pl.cw - 1 - t; }
    if (flip && !pl.sbs) { const int t = y0; y0 = pl.ch - 1 - y1; y1 = pl.ch - 1 - t; }
    ry[0] = y0; ry[1] = y1; rx[0] = x0; rx[1] = x1;
}

/* where the sample of C_v[cy][cx] lies in the plane of view v as oh_pics_pack takes it: half-size views hold C_v, full-size views of a
 * quincunx arrangement hold the lattice */
PK_HD void pk_view_pos(const PkPlane &pl, int v, int cx, int cy, int *sx, int *sy)
{
    *sx = cx; *sy = cy;
    if (pl.quincunx) {
        if (pl.sbs) *sx = 2 * cx + ((cy + v) & 1);
        else        *sy = 2 * cy + ((cx + v) & 1);
    }
}

/* sample (x, y) of the coded packed plane, made from the planes of the two views */
template <typename A>
PK_HD int pk_pack_sample(const PkPlane &pl, const int32_t flip[2], int x, int y, A at)
{
    x = pk_min(x, (pl.sbs ? 2 : 1) * pl.cw - 1); y = pk_min(y, (pl.sbs ? 1 : 2) * pl.ch - 1);
    const int v = pl.sbs ? x >= pl.cw : y >= pl.ch;
    int cx = x - (pl.sbs ? v * pl.cw : 0), cy = y - (pl.sbs ? 0 : v * pl.ch), sx, sy;
    if (flip[v]) {
        if (pl.sbs) cx = pl.cw - 1 - cx;
        else        cy = pl.ch - 1 - cy;
    }
    pk_view_pos(pl, v, cx, cy, &sx, &sy);
    return at(v, sy, sx);
}

/* the samples of view v's plane that outputs x0 .. x1 of row y of the packed plane read: rows sy[0] .. sy[1] (at most 2), columns
 * sx[0] .. sx[1]; false: none */
PK_HD bool pk_pack_box(const PkPlane &pl, const int32_t flip[2], int v, int x0, int x1, int y, int sy[2], int sx[2])
{
    const int pw = (pl.sbs ? 2 : 1) * pl.cw, ph = (pl.sbs ? 1 : 2) * pl.ch;
    x0 = pk_min(x0, pw - 1); x1 = pk_min(x1, pw - 1); y = pk_min(y, ph - 1);
    int cx0, cx1, cy;
    if (pl.sbs) {
        cx0 = pk_max(x0, v * pl.cw) - v * pl.cw; cx1 = pk_min(x1, (v + 1) * pl.cw - 1) - v * pl.cw; cy = y;
        if (cx0 > cx1)
            return false;
        if (flip[v]) { const int t = cx0; cx0 = pl.cw - 1 - cx1; cx1 = pl.cw - 1 - t; }
    } else {
        if ((y >= pl.ch) != (v != 0))
            return false;
        cx0 = x0; cx1 = x1; cy = y - v * pl.ch;
        if (flip[v]) cy = pl.ch - 1 - cy;
    }
    sx[0] = cx0; sx[1] = cx1; sy[0] = sy[1] = cy;
    if (pl.quincunx) {
        if (pl.sbs) { sx[0] = 2 * cx0; sx[1] = pk_min(2 * cx1 + 1, pl.vw - 1); }
        else        { sy[0] = 2 * cy; sy[1] = pk_min(2 * cy + 1, pl.vh - 1); }
    }
    return true;
}

#endif
