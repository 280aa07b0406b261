/*
 * warp.hip — finished pictures -> finished pictures resampled through an affine or perspective coordinate map (oh_pics_warp; the
 * exact definition is in DESIGN.md §3p, include/ohevc_hip.h and tests/warp_model.py; the formulas are warp_common.h, shared with the
 * host).  A gather: every destination sample reads 1, 4 or 16 source samples around a position that the map gives.
 *
 * One workgroup (256 lanes) per tile of WARP_TW x WARP_TH (64 x 16) destination samples of one plane of one picture; grid (tiles
 * across, tile rows of all planes, pictures).  A lane makes four neighbouring samples of one row and stores them as one dword (u8) or
 * two (u16); a wave writes four whole tile rows.  The destination's coded plane D replicates the image I (Wi x Hi) beyond its last
 * column and row, D[y][x] = I[min(y, Hi - 1)][min(x, Wi - 1)]: the tile that holds such samples computes them at the clamped place.
 *   1. box      the positions of the tile's four corner samples give the box of plane indices that the tile's taps lie in, with the
 *               filter's halo (warp_tile_box: the map carries the tile onto a convex quadrilateral);
 *   2. stage    where the box fits WARP_LDS bytes (warp_box_staged) the workgroup loads it once, row after row with consecutive
 *               lanes on consecutive samples, the border rule applied on the way (indices clamped into the window, or the fill), so
 *               that a tap is one LDS read at (i - x0, j - y0) with no rule left to apply;
 *   3. gather   every sample's position comes from warp_position, its taps from LDS where all of them lie in the staged box, else
 *               (strong minification, large shear: the box does not fit; or a perspective sample that the rounded denominator
 *               carries a little over the corners' box) from global memory through the same border rule.  Both ways run
 *               warp_interp on the same tap values, so they give the same sample.
 * 16 KiB of LDS per workgroup: eight workgroups of four waves fill a CU's 32 wave slots and take 128 of its 160 KiB, so LDS never
 * lowers the occupancy, and a 64 x 16 tile turned by any angle at scale 1 (at most 67 x 67 taps with the cubic halo, 9 KiB of u16) or
 * enlarged fits with room to spare.  The tile is wide so that a wave's stores are whole 64- or 128-byte row pieces.
 * Templates on the stored sample type, the mode (the affine form has no 64-bit division) and the filter.
 */
#include <algorithm>
#include "pics_common.h"
#include "warp_common.h"

namespace {

constexpr int TW = WARP_TW, TH = WARP_TH;

template <typename T, bool PERSP, int FILTER>
__global__ __launch_bounds__(THREADS) void warp_kernel(const OhWarpArgs a)
{
    constexpr int SZ = (int)sizeof(T);
    constexpr int BEFORE = FILTER == WARP_BICUBIC ? 1 : 0, BEHIND = FILTER == WARP_BICUBIC ? 2 : FILTER == WARP_BILINEAR ? 1 : 0;
    __shared__ __attribute__((aligned(16))) T box_s[WARP_LDS / SZ];
    LDS T *box_l = (LDS T *)box_s;
    const int pic = blockIdx.z, tid = threadIdx.x;
    int c, q;
    const int per[2] = { (a.dh[0] + TH - 1) / TH, (a.dh[1] + TH - 1) / TH };
    const int ty = grid_row(blockIdx.y, per, c, q), tx = blockIdx.x;
    const int dw = a.dw[q], dh = a.dh[q];
    if (tx * TW >= dw)
        return;
    const int sx = q ? a.sx : 0, sy = q ? a.sy : 0;
    const int iw = a.iw[q], ih = a.ih[q], Wc = a.ws[q], Hc = a.hs[q];
    int xa, ya, xb, yb;
    warp_tile_corners(tx, ty, dw, dh, iw, ih, &xa, &ya, &xb, &yb);
    const WarpBox b = warp_tile_box<PERSP>(a.m, sx, sy, FILTER, xa, ya, xb, yb);
    const bool staged = warp_box_staged(b, SZ);                 /* the same for the whole workgroup */
    const uintptr_t S = (uintptr_t)a.src[pic][c] + (size_t)a.y0[q] * a.spitch[c] + (size_t)a.x0[q] * SZ;
    const size_t sp = (size_t)a.spitch[c];
    const bool constant = a.border == OH_WARP_CONSTANT;
    const int32_t fill = a.fill[c], M = (1 << a.bd) - 1;
    /* the tap at plane index (i, j) of the window: the border rule, then a sample inside the window */
    auto from_global = [&](int i, int j) -> int32_t {
        const int ic = min(max(i, 0), Wc - 1), jc = min(max(j, 0), Hc - 1);
        const int32_t v = *(const GLOBAL T *)(S + (size_t)jc * sp + (size_t)ic * SZ);
        return constant && (i != ic || j != jc) ? fill : v;
    };
    const int bw = staged ? b.x1 - b.x0 + 1 : 1;
    if (staged) {
        const int cnt = bw * (b.y1 - b.y0 + 1);                 /* at most WARP_LDS / SZ */
        for (int i = tid; i < cnt; i += THREADS) {
            const int r = i / bw, k = i - r * bw;
            box_l[i] = (T)from_global(b.x0 + k, b.y0 + r);
        }
        __syncthreads();
    }
    auto from_lds = [&](int i, int j) -> int32_t { return box_l[(j - b.y0) * bw + (i - b.x0)]; };
    const int y = ty * TH + (tid >> 4), x0 = tx * TW + 4 * (tid & 15);
    if (y >= dh || x0 >= dw)                                    /* dw is a multiple of four */
        return;
    const int yi = min(y, ih - 1);
    T o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int32_t px, py;
        int ix, iy, fx, fy;
        warp_position<PERSP>(a.m, sx, sy, min(x0 + k, iw - 1), yi, &px, &py);
        warp_split(FILTER, px, &ix, &fx);
        warp_split(FILTER, py, &iy, &fy);
        const bool inside = staged && ix - BEFORE >= b.x0 && ix + BEHIND <= b.x1 && iy - BEFORE >= b.y0 && iy + BEHIND <= b.y1;
        o[k] = (T)(inside ? warp_interp(FILTER, from_lds, ix, iy, fx, fy, M) : warp_interp(FILTER, from_global, ix, iy, fx, fy, M));
    }
    const uintptr_t D = (uintptr_t)a.dst[pic][c] + (size_t)y * a.dpitch[c] + (size_t)x0 * SZ;
    if constexpr (SZ == 1) {
        uint32_t v; __builtin_memcpy(&v, o, 4);
        *(GLOBAL uint32_t *)D = v;
    } else {
        uint2v v; __builtin_memcpy(&v, o, 8);
        *(GLOBAL uint2v *)D = v;
    }
}

template <typename T, bool PERSP>
void launch(const OhWarpArgs *a, int n, hipStream_t st)
{
    const int cls = a->np > 1 ? 2 : 1;
    int tiles_x = 0, rows = 0;
    for (int q = 0; q < cls; q++) {
        tiles_x = std::max(tiles_x, (a->dw[q] + TW - 1) / TW);
        rows += (q ? 2 : 1) * ((a->dh[q] + TH - 1) / TH);
    }
    const dim3 grid((unsigned)tiles_x, (unsigned)rows, (unsigned)n);
    switch (a->filter) {
    case WARP_NEAREST:  warp_kernel<T, PERSP, WARP_NEAREST><<<grid, THREADS, 0, st>>>(*a); break;
    case WARP_BILINEAR: warp_kernel<T, PERSP, WARP_BILINEAR><<<grid, THREADS, 0, st>>>(*a); break;
    default:            warp_kernel<T, PERSP, WARP_BICUBIC><<<grid, THREADS, 0, st>>>(*a); break;
    }
}

} // namespace

static_assert(WARP_TW * WARP_TH == 4 * THREADS && WARP_TW == 64, "a lane makes four samples of a row: sixteen lanes a tile row");
static_assert(WARP_NEAREST == OH_WARP_NEAREST && WARP_BILINEAR == OH_WARP_BILINEAR && WARP_BICUBIC == OH_WARP_BICUBIC, "the filters' codes");
static_assert(8 * WARP_LDS <= 160 << 10, "eight workgroups on a CU");

extern "C" void ohk_warp(const OhWarpArgs *a, int n, hipStream_t st)
{
    const bool persp = a->mode == OH_WARP_PERSPECTIVE;
    if (a->bd == 8) { if (persp) launch<uint8_t, true>(a, n, st); else launch<uint8_t, false>(a, n, st); }
    else            { if (persp) launch<uint16_t, true>(a, n, st); else launch<uint16_t, false>(a, n, st); }
}
