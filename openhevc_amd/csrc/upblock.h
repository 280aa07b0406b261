/*
 * upblock.h — the reference's per-CTB SHVC up-sampling (the block path of its default build, ACTIVE_PU_UPSAMPLING hevc.h:117):
 * the window arithmetic of its block driver (upsample_block_luma / upsample_block_mc, hevc_filter.c:1175-1309), the edge emulation
 * it calls (emulated_edge_up_h / _v, videodsp_template.c:103-160) and the block slots (upsample_filter_block_{luma,cr}_{h,v}_{all,x2,x1_5},
 * hevcdsp_template.c:1834-2162).  Shared by the kernel (upsample.hip: upsample_block_kernel) and the host predicate that says where
 * the reference's output is defined (engine_shvc.hip: oh_upsample_blocks_defined), so both read the same arithmetic.
 */
#ifndef OHEVC_UPBLOCK_H
#define OHEVC_UPBLOCK_H

#include <stdint.h>
#include "up_taps.h"

#if defined(__HIPCC__)
#define UPB_HD  __host__ __device__ inline
#define UPB_DEV __device__ inline
#define UPB_CONST __constant__
#else
#define UPB_HD  static inline
#define UPB_DEV static inline
#define UPB_CONST static const
#endif

/* one plane of an up-sampling call: what the driver and the slots read of HEVCContext / UpsamplInf / the scaled window */
struct OhUpBlkGeom {
    int32_t cr;                       /* 0 luma (8 taps, MAX_EDGE 4), 1 chroma (4 taps, MAX_EDGE_CR 2) */
    int32_t idx;                      /* OH_UP_DEFAULT / X2 / X1_5 / SNR */
    int32_t w_el, h_el;               /* the enhancement-layer plane */
    int32_t bl_w, bl_h;               /* the driver's base-layer plane size (chroma height: hevc_filter.c:1252) */
    int32_t bl_w_act, bl_h_act;       /* the base-layer plane as it is */
    int32_t left, right_end, top, bottom_end;   /* scaled reference layer window in this plane (leftStart, rightEnd, topStart, bottomEnd) */
    int32_t sx, ax, sy, ay;           /* the slots' scale / add of this plane (Lum or Cr) */
    int32_t dsx, dax, dsy, day;       /* the driver's: always the luma ones (hevc_filter.c:1256-1258) */
    int32_t conf_left, conf_top;      /* EL conformance window in this plane's samples (pic_conf_win, hevc_filter.c:1196-1197) */
    int32_t log2_ctb;                 /* the CTB (luma samples) */
};

/* the driver's window for the block at (x0, y0) of a plane (hevc_filter.c:1186-1214, 1249-1268) */
struct OhUpBlk {
    int32_t w, h;                     /* ePbW, ePbH */
    int32_t bl_x, bl_y;               /* first base-layer column / row of the window (y: the chroma one carries the -4) */
    int32_t r0;                       /* base-layer row of intermediate row 0 (bl_y - bl_edge_top) */
    int32_t rows;                     /* intermediate rows the horizontal slot filters: bPbH + bl_edge_top + bl_edge_bottom */
    int32_t h_left, h_right;          /* emulated_edge_up_h replicated the left edge (and returned) / the right edge */
    int32_t v_up;                     /* bl_edge_up handed to emulated_edge_up_v */
    int32_t v_top, v_bot;             /* emulated_edge_up_v replicated the top rows (and returned) / the bottom rows */
    int32_t base;                     /* rows tmp0 advances before the vertical slot: 0 after a top replication, else MAX_EDGE - 1 */
};

UPB_HD int upb_clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

UPB_HD OhUpBlk upb_block(const OhUpBlkGeom &g, int x0, int y0)
{
    const int me = g.cr ? 2 : 4, sh = me - 1, ctb = 1 << (g.log2_ctb - g.cr);
    OhUpBlk b;
    b.w = x0 + ctb > g.w_el ? g.w_el - x0 : ctb;
    b.h = y0 + ctb > g.h_el ? g.h_el - y0 : ctb;
    int bw = (((b.w + 1) * g.dsx + g.dax) >> 12) >> 4;          /* "FIXME: check if this method is correct" */
    int bh = (((b.h + 2) * g.dsy + g.day) >> 12) >> 4;
    b.bl_x = (((x0 - g.conf_left) * g.dsx + g.dax) >> 12) >> 4;
    b.bl_y = ((((y0 - g.conf_top) * g.dsy + g.day) >> 12) - (g.cr ? 4 : 0)) >> 4;
    const int el = (sh - b.bl_x) > 0 ? 0 : sh, et = (sh - b.bl_y) > 0 ? 0 : sh;
    if (b.bl_x + bw > g.bl_w) bw = g.bl_w - b.bl_x;
    if (b.bl_y + bh > g.bl_h) bh = g.bl_h - b.bl_y;
    const int top0 = g.cr && b.bl_y < 0 ? b.bl_y : 0;           /* "the top can go in negative" (chroma only) */
    const int er = me < g.bl_w - b.bl_x - bw ? me : g.bl_w - b.bl_x - bw;
    const int eb = me < g.bl_h - b.bl_y - bh ? me : g.bl_h - b.bl_y - bh;
    b.r0 = b.bl_y - et;
    b.rows = bh + et + eb;
    b.h_left = el < sh;
    b.h_right = !b.h_left && er < sh + 1;
    b.v_up = et + top0;
    b.v_top = b.v_up < sh;
    b.v_bot = !b.v_top && eb < sh + 1;
    b.base = b.v_top ? 0 : sh;
    return b;
}

/* intermediate column the vertical slot reads for output column i: its source pointer advances only inside the window */
UPB_HD int upb_vcol(const OhUpBlkGeom &g, int x0, int i)
{
    const int lo = x0 > g.left ? x0 : g.left, hi = x0 + i - 1 < g.right_end - 2 ? x0 + i - 1 : g.right_end - 2;
    return hi >= lo ? hi - lo + 1 : 0;
}

/* coefficient rows: 0-15 the generic 16-phase table, then the x2 / x1.5 tables of the slot variants (hevcdsp.c:988-1024) */
enum { UPB_L_X2 = 16, UPB_L_X15 = 18, UPB_C_X2H = 16, UPB_C_X2V = 18, UPB_C_X15H = 20, UPB_C_X15V = 23 };

/* horizontal slot: base-layer column of the centre tap (pel[0]) of EL column xe, and its coefficient row */
UPB_HD int upb_hpos(const OhUpBlkGeom &g, int xe, int *row)
{
    const int x = upb_clip(xe, g.left, g.right_end), d = x - g.left;
    if (g.idx == 1) {                                           /* x2: (x - left) >> 1 luma, x >> 1 chroma; phase x & 1 */
        *row = (g.cr ? UPB_C_X2H : UPB_L_X2) + (x & 1);
        return g.cr ? x >> 1 : d >> 1;
    }
    if (g.idx == 2) {                                           /* x1.5: exact thirds */
        *row = (g.cr ? UPB_C_X15H : UPB_L_X15) + d % 3;
        return (d << 1) / 3;
    }
    const int r16 = (d * g.sx + g.ax) >> 12;
    *row = r16 & 15;
    return r16 >> 4;
}

/* vertical slot: the EL row y (already clipped to the window), its base-layer centre row and coefficient row */
UPB_HD int upb_vpos(const OhUpBlkGeom &g, int y, int *row)
{
    const int d = y - g.top;
    if (!g.cr && g.idx == 1) { *row = UPB_L_X2 + (d & 1); return d >> 1; }
    if (!g.cr && g.idx == 2) { *row = UPB_L_X15 + d % 3; return (d << 1) / 3; }
    const int r16 = ((d * g.sy + g.ay) >> 12) - (g.cr ? 4 : 0);
    *row = g.cr && g.idx == 1 ? UPB_C_X2V + (y & 1) : g.cr && g.idx == 2 ? UPB_C_X15V + y % 3 : r16 & 15;
    return r16 >> 4;
}

/* why a block's output is not defined by its own call, or 0 (host predicate; see oh_upsample_blocks_defined) */
enum { UPB_OK = 0, UPB_STALE_ROW, UPB_BL_ROW, UPB_BL_COL, UPB_BL_OVERWRITE, UPB_FOREIGN_ROW };

UPB_HD int upb_check(const OhUpBlkGeom &g, int x0, int y0)
{
    const OhUpBlk b = upb_block(g, x0, y0);
    const int B = g.cr ? 1 : 3, taps = 2 * B + 2;
    if (g.idx == 3)                                             /* SNR: copy_block of the co-located base-layer block */
        return x0 + b.w > g.bl_w_act ? UPB_BL_COL : y0 + b.h > g.bl_h_act ? UPB_BL_ROW : UPB_OK;
    if (b.h_left && b.bl_x > 0)
        return UPB_BL_OVERWRITE;                                /* the left replication would write over base-layer samples */
    /* chroma v slots store at the clipped row: a block whose rows clip into another block's rows writes there */
    if (g.cr && (upb_clip(y0, g.top, g.bottom_end - 1) < y0 || upb_clip(y0 + b.h - 1, g.top, g.bottom_end - 1) > y0 + b.h - 1))
        return UPB_FOREIGN_ROW;
    /* the base-layer columns the consumed intermediate columns read: [0, vcol(w - 1)] (emulated rows copy column vcol(i) too) */
    int rw, c_lo = upb_hpos(g, x0, &rw) - B, c_hi = upb_hpos(g, x0 + upb_vcol(g, x0, b.w - 1), &rw) - B + taps - 1;
    if (c_lo < 0 && !(b.h_left && c_lo >= -B))
        return UPB_BL_COL;
    if (c_hi >= g.bl_w_act && !(b.h_right && g.bl_w == g.bl_w_act && c_hi <= g.bl_w_act + B))
        return UPB_BL_COL;
    /* the intermediate rows the vertical slot reads (tmp0 rows): positions are monotonic in y */
    const int p_lo = upb_vpos(g, upb_clip(y0, g.top, g.bottom_end - 1), &rw), p_hi = upb_vpos(g, upb_clip(y0 + b.h - 1, g.top, g.bottom_end - 1), &rw);
    for (int t = p_lo - b.bl_y - B + b.base; t <= p_hi - b.bl_y - B + taps - 1 + b.base; t++) {
        int s = t;
        if (b.v_top && t >= -B && t <= -b.v_up - 1) s = -b.v_up;
        else if (b.v_bot && t >= b.rows && t <= b.rows + B) s = b.rows - 1;
        if (s < 0 || s >= b.rows)
            return UPB_STALE_ROW;                               /* neither filtered nor replicated by this call: scratch of an earlier one */
        if (b.r0 + s < 0 || b.r0 + s >= g.bl_h_act)
            return UPB_BL_ROW;
    }
    return UPB_OK;
}

/* ---- the per-block computation (device; one workgroup per block) ---- */
#define UPB_SRC_H 80                  /* h-filtered rows: bPbH + 7 <= 75 for scale <= 1 */
#define UPB_SRC_W 80                  /* base-layer columns: <= 64 + 8 */
#define UPB_TMP_H 96                  /* intermediate rows incl. the replicated ones, offset UPB_TMP_OFF */
#define UPB_TMP_OFF 8

UPB_CONST int8_t upb_luma[21][8] = {
    UP_TAPS_LUMA_ROWS,
    { 0, 0, 0, 64, 0, 0, 0, 0 }, { -1, 4, -11, 40, 40, -11, 4, -1 },                                            /* x2 */
    { 0, 0, 0, 64, 0, 0, 0, 0 }, { -1, 3, -8, 26, 52, -11, 4, -1 }, { -1, 4, -11, 52, 26, -8, 3, -1 } };       /* x1.5 */
UPB_CONST int8_t upb_chroma[26][4] = {
    UP_TAPS_CHROMA_ROWS,
    { 0, 64, 0, 0 }, { -4, 36, 36, -4 },                                   /* x2, horizontal */
    { -2, 10, 58, -2 }, { -6, 46, 28, -4 },                                /* x2, vertical */
    { 0, 64, 0, 0 }, { -2, 20, 52, -6 }, { -6, 52, 20, -2 },               /* x1.5, horizontal */
    { 0, 4, 62, -2 }, { -4, 30, 42, -4 }, { -4, 54, 16, -2 } };            /* x1.5, vertical */

template <int TAPS>
UPB_DEV int upb_coef(int row, int k) { return TAPS == 8 ? upb_luma[row][k] : upb_chroma[row][k]; }

/* the block at (x0, y0) of one plane: stage the base-layer window, horizontal slot into the int16 intermediate (no rounding), the
 * vertical edge emulation, vertical slot (round, clip, store).  tid / nt: this thread among nt; sync(): a barrier of the nt.
 * Samples beyond the base-layer plane are clamped: where the predicate holds, those are exactly the replicated edges. */
template <int TAPS, typename SRC, typename DST, typename SYNC>
UPB_DEV void upb_run(const OhUpBlkGeom &g, int x0, int y0, SRC src, int sstride, DST dst, int dstride,
                     uint8_t (*srcL)[UPB_SRC_W], int16_t (*tmpL)[64], int tid, int nt, SYNC sync)
{
    constexpr int B = TAPS / 2 - 1;
    const OhUpBlk b = upb_block(g, x0, y0);
    if (g.idx == 3) {                                           /* SNR (x1): copy_block */
        for (int e = tid; e < b.w * b.h; e += nt) {
            const int j = e / b.w, i = e - j * b.w;
            dst[(size_t)(y0 + j) * dstride + x0 + i] = src[(size_t)upb_clip(y0 + j, 0, g.bl_h_act - 1) * sstride + upb_clip(x0 + i, 0, g.bl_w_act - 1)];
        }
        return;
    }
    int rw;
    const int c_lo = upb_hpos(g, x0, &rw) - B;
    const int sw = upb_clip(upb_hpos(g, x0 + b.w - 1, &rw) - B + TAPS - c_lo, 1, UPB_SRC_W), sh = upb_clip(b.rows, 0, UPB_SRC_H);
    for (int e = tid; e < sw * sh; e += nt) {
        const int r = e / sw, c = e - r * sw;
        srcL[r][c] = src[(size_t)upb_clip(b.r0 + r, 0, g.bl_h_act - 1) * sstride + upb_clip(c_lo + c, 0, g.bl_w_act - 1)];
    }
    sync();
    for (int e = tid; e < sh * b.w; e += nt) {                   /* horizontal slot: intermediate row t, column i */
        const int t = e / b.w, i = e - t * b.w;
        const int o = upb_hpos(g, x0 + i, &rw) - B - c_lo;
        int s = 0;
#pragma unroll
        for (int k = 0; k < TAPS; k++)
            s += upb_coef<TAPS>(rw, k) * srcL[t][upb_clip(o + k, 0, UPB_SRC_W - 1)];
        tmpL[t + UPB_TMP_OFF][i] = (int16_t)s;
    }
    sync();
    if (b.v_top) {                                              /* rows -(v_up + 1) .. -B := row -v_up, column vcol(i) */
        const int n = B - b.v_up;
        for (int e = tid; e < n * b.w; e += nt) {
            const int j = e / b.w, i = e - j * b.w;
            tmpL[upb_clip(-(b.v_up + j) - 1 + UPB_TMP_OFF, 0, UPB_TMP_H - 1)][i] = tmpL[upb_clip(-b.v_up + UPB_TMP_OFF, 0, UPB_TMP_H - 1)][upb_vcol(g, x0, i)];
        }
    } else if (b.v_bot) {                                       /* rows rows .. rows + B := row rows - 1, column vcol(i) */
        for (int e = tid; e < (B + 1) * b.w; e += nt) {
            const int j = e / b.w, i = e - j * b.w;
            tmpL[upb_clip(b.rows + j + UPB_TMP_OFF, 0, UPB_TMP_H - 1)][i] = tmpL[upb_clip(b.rows - 1 + UPB_TMP_OFF, 0, UPB_TMP_H - 1)][upb_vcol(g, x0, i)];
        }
    }
    sync();
    for (int e = tid; e < b.h * b.w; e += nt) {                  /* vertical slot */
        const int j = e / b.w, i = e - j * b.w;
        const int y = upb_clip(y0 + j, g.top, g.bottom_end - 1);
        const int t = upb_vpos(g, y, &rw) - b.bl_y - B + b.base + UPB_TMP_OFF, col = upb_vcol(g, x0, i);
        int s = 0;
#pragma unroll
        for (int k = 0; k < TAPS; k++)
            s += upb_coef<TAPS>(rw, k) * tmpL[upb_clip(t + k, 0, UPB_TMP_H - 1)][col];
        const int v = (s + 2048) >> 12;
        dst[(size_t)(g.cr ? y : y0 + j) * dstride + x0 + i] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
}

#endif
