/*
 * upsample.hip — SHVC inter-layer up-sampling: the reference's whole-picture slot (upsample_tile_kernel) and its CTB path
 * (upsample_block_kernel) (gfx950; overview of the passes: kernels.hip; bit-exactness: tests/test_gpu_parity.py,
 * tests/test_gpu_shvc_block_path.py)
 */
#include "kernels_common.h"
#include "upblock.h"
#include "up_taps.h"

/* =========================================================================================
 * SHVC inter-layer up-sampling: upsample_base_layer_frame, hevcdsp_template.c:2164-2438 —
 * 16-phase separable resampling of a base-layer plane into the enhancement layer's geometry, 8-tap luma /
 * 4-tap chroma (tables hevcdsp.c:948-986).  One launch per plane, one workgroup per TILE of the enhancement-layer
 * plane (a CTB: 64 x 64 luma, 32 x 32 chroma — the unit the reference's on-demand path up-samples, ff_upsample_block
 * hevc_filter.c:1370-1426 / is_upsampled[]): the base-layer window the tile's taps reach is staged in LDS once
 * (coordinate clamps = the reference's edge buffers), the horizontal pass writes the int16 rows (no rounding, as the
 * reference's short buffer) into LDS, the vertical pass reads them there, rounds (>> 12), clips and stores — the
 * intermediate plane of the reference's two loops never exists in HBM.  Tiles come from a list (the CTBs a picture's
 * inter-layer prediction touches: oh_pic_upsample_ctbs) or are all tiles of the plane (oh_pic_upsample).
 * ======================================================================================= */
__constant__ int8_t c_up_luma[16][8] = { UP_TAPS_LUMA_ROWS };
__constant__ int8_t c_up_chroma[16][4] = { UP_TAPS_CHROMA_ROWS };

#define UP_TILE 64                    /* tile edge (luma CTB); scale <= 1 (EL >= BL): the window is at most UP_TILE + 8 */
#define UP_WIN  (UP_TILE + 8)

template <int TAPS>
__global__ __launch_bounds__(256) void upsample_tile_kernel(const OhUpPlane a, const int tw, const int th, const int tiles_x, const uint32_t *list)
{
    __shared__ uint8_t srcL[UP_WIN][UP_WIN + 8];
    __shared__ int16_t tmpL[UP_WIN][UP_TILE];
    const int tile = list ? (int)list[blockIdx.x] : (int)blockIdx.x;
    const int x0 = (tile % tiles_x) * tw, y0 = (tile / tiles_x) * th;
    if (x0 >= a.w_el || y0 >= a.h_el)
        return;
    const int w = min(tw, a.w_el - x0), h = min(th, a.h_el - y0), tid = threadIdx.x;
    constexpr int B = TAPS / 2 - 1;
    /* the intermediate columns this tile's outputs read: the source column only advances inside the window (:1925) */
    const int c_first = clip3(x0, a.left, a.right_end_v - 1) - a.left, c_last = clip3(x0 + w - 1, a.left, a.right_end_v - 1) - a.left;
    const int nc = c_last - c_first + 1;
    auto xpos = [&](int c) { return ((clip3(c, a.left, a.right_end_h) - a.left) * a.scale_x + a.add_x) >> 12; };     /* 1/16 sample */
    auto ypos = [&](int j) { return (((clip3(j, a.top, a.bottom_end - 1) - a.top) * a.scale_y + a.add_y) >> 12) - a.y_bias; };
    const int p_first = (xpos(c_first) >> 4) - B, p_last = (xpos(c_last) >> 4) - B + TAPS - 1;
    const int r_first = (ypos(y0) >> 4) - B, r_last = (ypos(y0 + h - 1) >> 4) - B + TAPS - 1;
    const int sw = min(p_last - p_first + 1, UP_WIN + 8), sh = min(r_last - r_first + 1, UP_WIN);   /* the host checked scale <= 1 */
    const GLOBAL uint8_t *__restrict__ src = G_CONST(uint8_t, a.src);
    for (int e = tid; e < sw * sh; e += 256) {
        const int r = e / sw, c = e - r * sw;
        srcL[r][c] = src[(size_t)clip3(r_first + r, 0, a.h_bl - 1) * a.sstride + clip3(p_first + c, 0, a.w_bl - 1)];
    }
    __syncthreads();
    for (int e = tid; e < nc * sh; e += 256) {
        const int r = e / nc, c = e - r * nc;
        const int r16 = xpos(c_first + c), phase = r16 & 15, o = (r16 >> 4) - B - p_first;
        int s = 0;
#pragma unroll
        for (int k = 0; k < TAPS; k++)
            s += (TAPS == 8 ? c_up_luma[phase][k] : c_up_chroma[phase][k]) * srcL[r][o + k];
        tmpL[r][c] = (int16_t)s;
    }
    __syncthreads();
    GLOBAL uint8_t *__restrict__ dst = G_MUT(uint8_t, a.dst);
    for (int e = tid; e < w * h; e += 256) {
        const int j = e / w, i = e - j * w;
        const int r16 = ypos(y0 + j), phase = r16 & 15, o = (r16 >> 4) - B - r_first;
        const int col = clip3(x0 + i, a.left, a.right_end_v - 1) - a.left - c_first;
        int s = 0;
#pragma unroll
        for (int k = 0; k < TAPS; k++)
            s += (TAPS == 8 ? c_up_luma[phase][k] : c_up_chroma[phase][k]) * tmpL[o + k][col];
        dst[(size_t)(y0 + j) * a.dstride + x0 + i] = (uint8_t)clip3((s + 2048) >> 12, 0, 255);
    }
}

/* one plane: tiles tw x th, either those of `list` (n_list tile indices, row-major over ceil(w_el / tw) columns; device memory) or all */
extern "C" void ohk_upsample_plane(const OhUpPlane *a, int taps, int tw, int th, const uint32_t *list, int n_list, hipStream_t st)
{
    const int tiles_x = (a->w_el + tw - 1) / tw, tiles_y = (a->h_el + th - 1) / th;
    const int n = list ? n_list : tiles_x * tiles_y;
    if (n <= 0) return;
    if (taps == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(upsample_tile_kernel<8>), dim3(n), dim3(256), 0, st, *a, tw, th, tiles_x, list);
    else           hipLaunchKernelGGL(HIP_KERNEL_NAME(upsample_tile_kernel<4>), dim3(n), dim3(256), 0, st, *a, tw, th, tiles_x, list);
}

/* =========================================================================================
 * The reference's CTB path itself (its default build: ACTIVE_PU_UPSAMPLING hevc.h:117, ff_upsample_block hevc_filter.c:1370-1426):
 * per listed enhancement-layer CTB what upsample_block_luma / upsample_block_mc compute for it (hevc_filter.c:1175-1309) — the
 * driver's base-layer window with its size estimates and margins, the one-edge-per-call emulation (emulated_edge_up_h / _v) and the
 * slot variant UpsamplInf.idx picks (x2 fixed phases, x1.5 exact thirds, the 16.16 generic one, a copy at x1).  The arithmetic is
 * upblock.h's, shared with the host predicate.  One workgroup per CTB and plane (blockIdx.y: Y, Cb, Cr); the base-layer window and
 * the int16 intermediate (with its replicated rows) live in LDS.
 * ======================================================================================= */
__global__ __launch_bounds__(256) void upsample_block_kernel(const OhUpBlkArgs a, const uint32_t *list)
{
    __shared__ uint8_t srcL[UPB_SRC_H][UPB_SRC_W];
    __shared__ int16_t tmpL[UPB_TMP_H][64];
    const int c = blockIdx.y, ctb = list ? (int)list[blockIdx.x] : (int)blockIdx.x;
    const OhUpBlkGeom &g = a.g[c ? 1 : 0];
    const int size = 1 << (g.log2_ctb - g.cr), x0 = (ctb % a.ctbs_x) * size, y0 = (ctb / a.ctbs_x) * size;
    if (x0 >= g.w_el || y0 >= g.h_el)
        return;
    const GLOBAL uint8_t *__restrict__ src = G_CONST(uint8_t, a.src[c]);
    GLOBAL uint8_t *__restrict__ dst = G_MUT(uint8_t, a.dst[c]);
    auto sync = [] { __syncthreads(); };
    if (c == 0) upb_run<8>(g, x0, y0, src, a.sstride[c], dst, a.dstride[c], srcL, tmpL, (int)threadIdx.x, 256, sync);
    else        upb_run<4>(g, x0, y0, src, a.sstride[c], dst, a.dstride[c], srcL, tmpL, (int)threadIdx.x, 256, sync);
}

/* the listed CTBs (raster addresses over ctbs_x columns; device memory) or, list == nullptr, n = every CTB */
extern "C" void ohk_upsample_blocks(const OhUpBlkArgs *a, const uint32_t *list, int n, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(upsample_block_kernel, dim3(n, 3), dim3(256), 0, st, *a, list);
}
