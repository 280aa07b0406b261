/*
 * oracle_px.inc — pixel-typed part of the oracle, included twice by oracle.c with
 *   PX = uint8_t,  FN(x) = x##_8     (bit depth 8)
 *   PX = uint16_t, FN(x) = x##_16    (bit depth 9..14)
 * TEST INFRASTRUCTURE ONLY (see oracle.h).  Strides in this file are in PIXELS.
 */

static inline int FN(clip_px)(int v, int bd)
{
    int mx = (1 << bd) - 1;
    return v < 0 ? 0 : (v > mx ? mx : v);
}

/* ---- residual add: hevcdsp_template.c:45-111 ---- */
static void FN(transform_add)(int bd, PX *dst, const int16_t *res, ptrdiff_t stride, int n)
{
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++)
            dst[y * stride + x] = (PX)FN(clip_px)(dst[y * stride + x] + res[y * n + x], bd);
}

/* ---- interpolation core: hevcdsp_template.c:610-1609 ----
 * Produces the 14-bit intermediate prediction sample of every position as int32 into
 * out[h][w] (row stride w).  The reference keeps the horizontal pass of the hv case in an
 * int16 array (tmp_array, :776) — that truncation is reproduced. */
static void FN(mc_intermediate)(int bd, int taps, int32_t *out, const PX *src, ptrdiff_t sstride,
                                int w, int h, int fx, int fy)
{
    const int before = taps / 2 - 1;
    const int8_t *cx = taps == 8 ? oh_qpel_taps[fx] : oh_epel_taps[fx];
    const int8_t *cy = taps == 8 ? oh_qpel_taps[fy] : oh_epel_taps[fy];

    if (!fx && !fy) {                                   /* pel_pixels :610-624 */
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++)
                out[y * w + x] = src[y * sstride + x] << (14 - bd);
    } else if (fx && !fy) {                             /* _h :731-745 */
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int s = 0;
                for (int k = 0; k < taps; k++)
                    s += cx[k] * src[y * sstride + x + k - before];
                out[y * w + x] = s >> (bd - 8);
            }
    } else if (!fx && fy) {                             /* _v :747-761 */
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int s = 0;
                for (int k = 0; k < taps; k++)
                    s += cy[k] * src[(y + k - before) * sstride + x];
                out[y * w + x] = s >> (bd - 8);
            }
    } else {                                            /* _hv :763-794 */
        int16_t rowbuf[(64 + 7) * 64];
        for (int y = 0; y < h + taps - 1; y++)
            for (int x = 0; x < w; x++) {
                int s = 0;
                for (int k = 0; k < taps; k++)
                    s += cx[k] * src[(y - before) * sstride + x + k - before];
                rowbuf[y * 64 + x] = (int16_t)(s >> (bd - 8));
            }
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int s = 0;
                for (int k = 0; k < taps; k++)
                    s += cy[k] * rowbuf[(y + k) * 64 + x];
                out[y * w + x] = s >> 6;
            }
    }
}

/* uni-directional epilogue (:626-640 copy, :796-943) */
static void FN(mc_store_uni)(int bd, PX *dst, ptrdiff_t dstride, const int32_t *v, int w, int h)
{
    int shift = 14 - bd, off = 1 << (shift - 1);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            dst[y * dstride + x] = (PX)FN(clip_px)((v[y * w + x] + off) >> shift, bd);
}
/* bi-directional epilogue (:642-666, :822-983): src2 is list 0's int16 intermediate */
static void FN(mc_store_bi)(int bd, PX *dst, ptrdiff_t dstride, const int32_t *v,
                            const int16_t *src2, ptrdiff_t s2stride, int w, int h)
{
    int shift = 15 - bd, off = 1 << (shift - 1);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            dst[y * dstride + x] = (PX)FN(clip_px)((v[y * w + x] + src2[y * s2stride + x] + off) >> shift, bd);
}
/* explicit weighting, one list (:668-690, :985-1134) */
static void FN(mc_store_uni_w)(int bd, PX *dst, ptrdiff_t dstride, const int32_t *v, int w, int h,
                               int denom, int wx, int ox)
{
    int shift = denom + 14 - bd, off = 1 << (shift - 1);
    ox = ox * (1 << (bd - 8));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            dst[y * dstride + x] = (PX)FN(clip_px)(((v[y * w + x] * wx + off) >> shift) + ox, bd);
}
/* explicit weighting, two lists (:692-716, :1012-1174): v is list 1, src2 is list 0 */
static void FN(mc_store_bi_w)(int bd, PX *dst, ptrdiff_t dstride, const int32_t *v,
                              const int16_t *src2, ptrdiff_t s2stride, int w, int h,
                              int denom, int wx0, int wx1, int ox0, int ox1)
{
    int log2wd = denom + 14 - bd;
    ox0 = ox0 * (1 << (bd - 8));
    ox1 = ox1 * (1 << (bd - 8));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            dst[y * dstride + x] = (PX)FN(clip_px)((v[y * w + x] * wx1 + src2[y * s2stride + x] * wx0 +
                                                    ((ox0 + ox1 + 1) << log2wd)) >> (log2wd + 1), bd);
}

/* ---- intra prediction from prepared edges: hevcpred_template.c:359-538 ---- */
static void FN(pred_planar)(PX *dst, const PX *top, const PX *left, ptrdiff_t stride, int log2)
{
    int n = 1 << log2;
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++)
            dst[y * stride + x] = (PX)(((n - 1 - x) * left[y] + (x + 1) * top[n] +
                                        (n - 1 - y) * top[x] + (y + 1) * left[n] + n) >> (log2 + 1));
}

static void FN(pred_dc)(PX *dst, const PX *top, const PX *left, ptrdiff_t stride, int log2, int c_idx)
{
    int n = 1 << log2, dc = n;
    for (int i = 0; i < n; i++)
        dc += left[i] + top[i];
    dc >>= log2 + 1;
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++)
            dst[y * stride + x] = (PX)dc;
    g_cnt[c_idx == 0 && n < 32 ? OH_CNT_I_DC_EDGE : OH_CNT_I_DC_PLAIN]++;
    if (c_idx == 0 && n < 32) {                          /* :410-416 */
        dst[0] = (PX)((left[0] + 2 * dc + top[0] + 2) >> 2);
        for (int x = 1; x < n; x++)
            dst[x] = (PX)((top[x] + 3 * dc + 2) >> 2);
        for (int y = 1; y < n; y++)
            dst[y * stride] = (PX)((left[y] + 3 * dc + 2) >> 2);
    }
}

static void FN(pred_angular)(int bd, PX *dst, const PX *top, const PX *left, ptrdiff_t stride,
                             int log2, int c_idx, int mode)
{
    int n = 1 << log2;
    int angle = oh_intra_angle[mode - 2];
    int vertical = mode >= 18;
    const PX *main_ = vertical ? top : left;             /* reference array along the iteration axis */
    const PX *side  = vertical ? left : top;
    PX refbuf[3 * 32 + 4];
    PX *ref = refbuf + 32;                               /* ref[i] == main_[i-1] for i >= 0 */
    int last = (n * angle) >> 5;

    for (int i = 0; i <= 2 * n; i++)
        ref[i] = main_[i - 1];
    if (angle < 0 && last < -1) {                        /* projected side samples :447-453, :480-486 */
        g_cnt[OH_CNT_I_PROJECTED]++;
        int inv = oh_inv_angle[mode - 11];
        for (int i = last; i <= -1; i++)
            ref[i] = side[-1 + ((i * inv + 128) >> 8)];
    }
    for (int a = 0; a < n; a++) {                        /* a: row (vertical modes) or column */
        int idx  = ((a + 1) * angle) >> 5;
        int fact = ((a + 1) * angle) & 31;
        for (int b = 0; b < n; b++) {
            int v = fact ? ((32 - fact) * ref[b + idx + 1] + fact * ref[b + idx + 2] + 16) >> 5
                         : ref[b + idx + 1];
            if (vertical) dst[a * stride + b] = (PX)v;
            else          dst[b * stride + a] = (PX)v;
        }
    }
    if (c_idx == 0 && n < 32) {                          /* boundary smoothing :474-477, :501-508 */
        if (mode == 26)
            for (int y = 0; y < n; y++) {
                const int v = top[0] + ((left[y] - left[-1]) >> 1);
                g_cnt[v < 0 ? OH_CNT_I_CLIP26_LOW : v >= (1 << bd) ? OH_CNT_I_CLIP26_HIGH : OH_CNT_I_CLIP26_NONE]++;
                dst[y * stride] = (PX)FN(clip_px)(v, bd);
            }
        if (mode == 10)
            for (int x = 0; x < n; x++) {
                const int v = left[0] + ((top[x] - top[-1]) >> 1);
                g_cnt[v < 0 ? OH_CNT_I_CLIP10_LOW : v >= (1 << bd) ? OH_CNT_I_CLIP10_HIGH : OH_CNT_I_CLIP10_NONE]++;
                dst[x] = (PX)FN(clip_px)(v, bd);
            }
    }
}

static int FN(isi)(const uint8_t *map, int mpw, int mph, int lpu, int lx, int ly)
{
    int px = lx >> lpu, py = ly >> lpu;                 /* arithmetic shifts: -1 and -2 both land in cell -1 */
    return px >= 0 && py >= 0 && px < mpw && py < mph && map[px + py * mpw];
}

/* ---- neighbour gathering + smoothing: hevcpred_template.c:30-344 ----
 * Constrained intra prediction (:116-163, :185-249): neighbours that belong to inter CUs count as missing;
 * the candidate flags are re-derived from the min-PU intra map and the gathered edges are patched in
 * groups of four samples from the nearest intra sample, in the reference's order of sweeps (left column
 * downwards, then upwards from its end, then the top row rightwards).  The sweeps are stated per sample
 * here; `isi(dx, dy)` is the reference's IS_INTRA(x, y) for a sample offset relative to the block. */
static void FN(intra_pred)(const OhPicParams *p, PX *plane, ptrdiff_t stride, int pw, int ph,
                           int x0, int y0, int c_idx, int log2, int mode, int avail, const uint8_t *is_intra)
{
    int bd = p->bit_depth;
    int n = 1 << log2;
    PX lbuf[2 * 32 + 1], tbuf[2 * 32 + 1], flbuf[2 * 32 + 1], ftbuf[2 * 32 + 1];
    PX *left = lbuf + 1, *top = tbuf + 1, *fleft = flbuf + 1, *ftop = ftbuf + 1;
    PX *src = plane + y0 * stride + x0;
    int a_bl = !!(avail & OH_AV_BOTTOM_LEFT), a_l = !!(avail & OH_AV_LEFT), a_ul = !!(avail & OH_AV_UP_LEFT);
    int a_u = !!(avail & OH_AV_UP), a_ur = !!(avail & OH_AV_UP_RIGHT);
    /* samples that exist inside the picture below-left / above-right (:111-114) */
    int bl_size = (y0 + 2 * n < ph ? y0 + 2 * n : ph) - (y0 + n);
    int tr_size = (x0 + 2 * n < pw ? x0 + 2 * n : pw) - (x0 + n);
    if (bl_size < 0) bl_size = 0;
    if (tr_size < 0) tr_size = 0;

    for (int i = 0; i < 2 * 32 + 1; i++) lbuf[i] = tbuf[i] = 0;

    const int cip = p->constrained_intra_pred && is_intra;
    const int hs = oh_hshift(p, c_idx), vs = oh_vshift(p, c_idx), lpu = p->log2_min_pu_size;
    const int mpw = p->width >> lpu, mph = p->height >> lpu, X0 = x0 << hs, Y0 = y0 << vs;
    /* IS_INTRA(dx, dy): the map cell of the luma position of sample (dx, dy); positions outside the map read 0
     * (the reference would read outside tab_mvf there) */
#define ISI(dx, dy) FN(isi)(is_intra, mpw, mph, lpu, X0 + (dx) * (1 << hs), Y0 + (dy) * (1 << vs))
    if (cip) {
        const int sl_h = n << hs, sl_v = n << vs;
        int pu_v = sl_v >> lpu, pu_h = sl_h >> lpu;
        const int on_x = !(X0 & ((1 << lpu) - 1)), on_y = !(Y0 & ((1 << lpu) - 1));
        if (!pu_h) pu_h++;                                                 /* :124-125 (only the horizontal count) */
#define CELL(px, py) ((px) >= 0 && (py) >= 0 && (px) < mpw && (py) < mph && is_intra[(px) + (py) * mpw])
        if (a_bl && on_x) {                                                /* every other min PU, :126-133 */
            int xl = (X0 - 1) >> lpu, yb = (Y0 + sl_v) >> lpu, mx = pu_v < mph - yb ? pu_v : mph - yb;
            a_bl = 0;
            for (int i = 0; i < mx; i += 2) a_bl |= CELL(xl, yb + i);
            if (!a_bl) g_cnt[OH_CNT_I_CIP_FLAG_CLEARED]++;
        }
        if (a_l && on_x) {
            int xl = (X0 - 1) >> lpu, yl = Y0 >> lpu, mx = pu_v < mph - yl ? pu_v : mph - yl;
            a_l = 0;
            for (int i = 0; i < mx; i += 2) a_l |= CELL(xl, yl + i);
            if (!a_l) g_cnt[OH_CNT_I_CIP_FLAG_CLEARED]++;
        }
        if (a_ul) {
            a_ul = CELL((X0 - 1) >> lpu, (Y0 - 1) >> lpu);
            if (!a_ul) g_cnt[OH_CNT_I_CIP_FLAG_CLEARED]++;
        }
        if (a_u && on_y) {
            int xt = X0 >> lpu, yt = (Y0 - 1) >> lpu, mx = pu_h < mpw - xt ? pu_h : mpw - xt;
            a_u = 0;
            for (int i = 0; i < mx; i += 2) a_u |= CELL(xt + i, yt);
            if (!a_u) g_cnt[OH_CNT_I_CIP_FLAG_CLEARED]++;
        }
        if (a_ur && on_y) {
            int yt = (Y0 - 1) >> lpu, xr = (X0 + sl_h) >> lpu, mx = pu_h < mpw - xr ? pu_h : mpw - xr;
            a_ur = 0;
            for (int i = 0; i < mx; i += 2) a_ur |= CELL(xr + i, yt);
            if (!a_ur) g_cnt[OH_CNT_I_CIP_FLAG_CLEARED]++;
        }
#undef CELL
        /* memset(left / top, 128, 64 * sizeof(pixel)): BYTES of 128, i.e. 0x8080 for 16-bit samples (:158-160) */
        for (int i = 0; i < 64; i++) left[i] = top[i] = (PX)(sizeof(PX) == 1 ? 128 : 0x8080);
        top[-1] = 128;
    }

    if (a_ul) left[-1] = top[-1] = src[-stride - 1];
    if (a_u)  for (int i = 0; i < n; i++) top[i] = src[-stride + i];
    if (a_ur) {
        if (tr_size > 0 && tr_size < n) g_cnt[OH_CNT_I_TR_PARTIAL]++;
        for (int i = 0; i < tr_size; i++) top[n + i] = src[-stride + n + i];
        for (int i = tr_size; i < n; i++) top[n + i] = src[-stride + n + tr_size - 1];
    }
    if (a_l)  for (int i = 0; i < n; i++) left[i] = src[i * stride - 1];
    if (a_bl) {
        if (bl_size > 0 && bl_size < n) g_cnt[OH_CNT_I_BL_PARTIAL]++;
        for (int i = 0; i < bl_size; i++) left[n + i] = src[(n + i) * stride - 1];
        for (int i = bl_size; i < n; i++) left[n + i] = src[(n + bl_size - 1) * stride - 1];
    }

    if (cip && (a_bl || a_l || a_ul || a_u || a_ur)) {                    /* :185-249 */
        int size_max_x = x0 + 2 * n < pw ? 2 * n : pw - x0, size_max_y = y0 + 2 * n < ph ? 2 * n : ph - y0;
        int j = n + (a_bl ? bl_size : 0) - 1;
        if (!a_ur) size_max_x = x0 + n < pw ? n : pw - x0;
        if (!a_bl) size_max_y = y0 + n < ph ? n : ph - y0;
        if (a_bl || a_l || a_ul) {
            while (j > -1 && !ISI(-1, j)) j--;
            if (!ISI(-1, j)) {                                             /* nothing intra on the left side: take it from the top row */
                g_cnt[OH_CNT_I_CIP_TOP_START]++;
                j = 0;
                while (j < size_max_x && !ISI(j, -1)) j++;
                for (int i = j; i > -1; i--)
                    if (!ISI(i - 1, -1)) top[i - 1] = top[i];
                left[-1] = top[-1];
            }
        } else {
            g_cnt[OH_CNT_I_CIP_NO_LEFT]++;
            j = 0;
            while (j < size_max_x && !ISI(j, -1)) j++;
            if (j > 0) {
                if (x0 > 0) {
                    for (int i = j; i > -1; i--)
                        if (!ISI(i - 1, -1)) top[i - 1] = top[i];
                } else {
                    for (int i = j; i > 0; i--)
                        if (!ISI(i - 1, -1)) top[i - 1] = top[i];
                    top[-1] = top[0];
                }
            }
            left[-1] = top[-1];
        }
        left[-1] = top[-1];
        if (a_bl || a_l) {                                                 /* downwards: non-intra groups take the last intra sample above */
            PX a = left[-1];
            for (int i = 0; i < size_max_y; i += 4) {
                if (!ISI(-1, i)) { left[i] = left[i + 1] = left[i + 2] = left[i + 3] = a; }
                else a = left[i + 3];
            }
        }
        if (!a_l)  for (int i = 0; i < n; i++) left[i] = left[-1];
        if (!a_bl) for (int i = 0; i < n; i++) left[n + i] = left[n - 1];
        if (x0 != 0 && y0 != 0) {                                          /* upwards from the end of the column */
            PX a = left[size_max_y - 1];
            g_cnt[OH_CNT_I_CIP_UP_SWEEP]++;
            for (int i = size_max_y - 1; i > -1; i -= 4) {
                if (!ISI(-1, i - 3)) { left[i - 3] = left[i - 2] = left[i - 1] = left[i] = a; }
                else a = left[i - 3];
            }
            if (!ISI(-1, -1)) { left[-1] = left[0]; g_cnt[OH_CNT_I_CIP_CORNER]++; }
        } else if (x0 == 0) {
            g_cnt[OH_CNT_I_CIP_X0_ZERO]++;
            for (int i = 0; i < size_max_y; i++) left[i] = 0;             /* EXTEND(left, 0, size_max_y), :236 */
        } else {
            PX a = left[size_max_y - 1];
            g_cnt[OH_CNT_I_CIP_UP_SWEEP]++;
            for (int i = size_max_y - 1; i > -1; i -= 4) {
                if (!ISI(-1, i - 3)) { left[i - 3] = left[i - 2] = left[i - 1] = left[i] = a; }
                else a = left[i - 3];
            }
        }
        top[-1] = left[-1];
        if (y0 != 0) {                                                     /* the top row rightwards */
            PX a = left[-1];
            for (int i = 0; i < size_max_x; i += 4) {
                if (!ISI(i, -1)) { top[i] = top[i + 1] = top[i + 2] = top[i + 3] = a; }
                else a = top[i + 3];
            }
        }
    }
#undef ISI

    /* substitution of unavailable samples (:251-286) */
    if (!a_bl) {
        g_cnt[a_l ? OH_CNT_I_SUB_L : a_ul ? OH_CNT_I_SUB_UL : a_u ? OH_CNT_I_SUB_U : a_ur ? OH_CNT_I_SUB_UR : OH_CNT_I_SUB_NONE]++;
        if (a_l) {
            for (int i = 0; i < n; i++) left[n + i] = left[n - 1];
        } else if (a_ul) {
            for (int i = 0; i < 2 * n; i++) left[i] = left[-1];
            a_l = 1;
        } else if (a_u) {
            left[-1] = top[0];
            for (int i = 0; i < 2 * n; i++) left[i] = left[-1];
            a_ul = a_l = 1;
        } else if (a_ur) {
            for (int i = 0; i < n; i++) top[i] = top[n];
            left[-1] = top[n];
            for (int i = 0; i < 2 * n; i++) left[i] = left[-1];
            a_u = a_ul = a_l = 1;
        } else {
            left[-1] = (PX)(1 << (bd - 1));
            for (int i = 0; i < 2 * n; i++) top[i] = left[i] = left[-1];
        }
    }
    if (!a_l)  g_cnt[OH_CNT_I_FILL_L]++;
    if (!a_ul) g_cnt[OH_CNT_I_FILL_UL]++;
    if (!a_u)  g_cnt[OH_CNT_I_FILL_U]++;
    if (!a_ur) g_cnt[OH_CNT_I_FILL_UR]++;
    if (!a_l)  for (int i = 0; i < n; i++) left[i] = left[n];
    if (!a_ul) left[-1] = left[0];
    if (!a_u)  for (int i = 0; i < n; i++) top[i] = left[-1];
    if (!a_ur) for (int i = 0; i < n; i++) top[n + i] = top[n - 1];
    top[-1] = left[-1];

    /* smoothing (:288-326) */
    int filtered = 0;
    if (!p->intra_smoothing_disabled && (c_idx == 0 || p->chroma_format_idc == 3) &&
        mode != 1 && n != 4) {
        static const int thresh[3] = { 7, 1, 0 };
        int d26 = mode > 26 ? mode - 26 : 26 - mode;
        int d10 = mode > 10 ? mode - 10 : 10 - mode;
        int dist = d26 < d10 ? d26 : d10;
        if (dist > thresh[log2 - 3]) {
            int lim = 1 << (bd - 5);
            int t = lim, l = lim;
            if (log2 == 5) {
                t = abs(top[-1]  + top[63]  - 2 * top[31]);
                l = abs(left[-1] + left[63] - 2 * left[31]);
                if (c_idx == 0)
                    g_cnt[t < lim ? (l < lim ? OH_CNT_I_TL_PP : OH_CNT_I_TL_PF) : (l < lim ? OH_CNT_I_TL_FP : OH_CNT_I_TL_FF)]++;
            }
            if (p->strong_intra_smoothing && c_idx == 0 && log2 == 5 && t < lim && l < lim) {
                g_cnt[OH_CNT_INTRA_STRONG_32]++;
                filtered = 2;
                ftop[-1] = top[-1];  ftop[63] = top[63];
                fleft[-1] = left[-1]; fleft[63] = left[63];
                for (int i = 0; i < 63; i++) {
                    ftop[i]  = (PX)(((63 - i) * top[-1]  + (i + 1) * top[63]  + 32) >> 6);
                    fleft[i] = (PX)(((63 - i) * left[-1] + (i + 1) * left[63] + 32) >> 6);
                }
            } else {
                filtered = 1;
                fleft[2 * n - 1] = left[2 * n - 1];
                ftop[2 * n - 1]  = top[2 * n - 1];
                for (int i = 2 * n - 2; i >= 0; i--) {
                    fleft[i] = (PX)((left[i + 1] + 2 * left[i] + left[i - 1] + 2) >> 2);
                    ftop[i]  = (PX)((top[i + 1]  + 2 * top[i]  + top[i - 1]  + 2) >> 2);
                }
                ftop[-1] = fleft[-1] = (PX)((left[0] + 2 * left[-1] + top[0] + 2) >> 2);
            }
            left = fleft;
            top = ftop;
        }
    }

    g_cnt[filtered == 2 ? OH_CNT_I_FILT_STRONG : filtered ? OH_CNT_I_FILT_3TAP : OH_CNT_I_FILT_NONE]++;
    if (mode == 0)      FN(pred_planar)(src, top, left, stride, log2);
    else if (mode == 1) FN(pred_dc)(src, top, left, stride, log2, c_idx);
    else                FN(pred_angular)(bd, src, top, left, stride, log2, c_idx, mode);
}

/* ---- deblocking of one 8-sample edge: hevcdsp_template.c:1629-1757 ----
 * The CNT() lines count which decisions the content reached (oh_or_counters, oracle.h); they change no sample. */
static void FN(loop_filter_luma)(int bd, PX *pix, ptrdiff_t xs, ptrdiff_t ys, int beta,
                                 const int *tc_, const uint8_t *no_p_, const uint8_t *no_q_)
{
    beta <<= bd - 8;
    for (int seg = 0; seg < 2; seg++, pix += 4 * ys) {
        PX *l0 = pix, *l3 = pix + 3 * ys;
        int tc = tc_[seg] << (bd - 8);
        int no_p = no_p_[seg], no_q = no_q_[seg];
        const int cnt = g_cnt_ctx.dir >= 0 && g_cnt_ctx.bs[seg] > 0;      /* a luma segment with bs > 0 inside oh_or_pass_deblock */
#define CNT(k) do { if (cnt) g_cnt[g_cnt_ctx.dir * OH_CNT_PER_DIR + (k)]++; } while (0)
        CNT(OH_CNT_SEGMENTS);
        int dp0 = abs(l0[-3 * xs] - 2 * l0[-2 * xs] + l0[-xs]);
        int dq0 = abs(l0[2 * xs] - 2 * l0[xs] + l0[0]);
        int dp3 = abs(l3[-3 * xs] - 2 * l3[-2 * xs] + l3[-xs]);
        int dq3 = abs(l3[2 * xs] - 2 * l3[xs] + l3[0]);
        int d0 = dp0 + dq0, d3 = dp3 + dq3;
        if (d0 + d3 >= beta)
            continue;
        CNT(OH_CNT_FILTER_ON);
        if (no_p || no_q) CNT(OH_CNT_FILTER_ON_PCM);
        int beta3 = beta >> 3, beta2 = beta >> 2, tc25 = (tc * 5 + 1) >> 1;
        int strong =
            abs(l0[-4 * xs] - l0[-xs]) + abs(l0[3 * xs] - l0[0]) < beta3 && abs(l0[-xs] - l0[0]) < tc25 &&
            abs(l3[-4 * xs] - l3[-xs]) + abs(l3[3 * xs] - l3[0]) < beta3 && abs(l3[-xs] - l3[0]) < tc25 &&
            (d0 << 1) < beta2 && (d3 << 1) < beta2;
        if (strong) {
            int tc2 = tc << 1;
            CNT(OH_CNT_STRONG);
            if (no_p || no_q) CNT(OH_CNT_STRONG_PCM);
#define CLIP_TC2(v) oh_clip3_cnt(v, -tc2, tc2, cnt ? &g_cnt[g_cnt_ctx.dir * OH_CNT_PER_DIR + OH_CNT_STRONG_TC2_HITS] : NULL)
            for (int d = 0; d < 4; d++) {
                PX *q = pix + d * ys;
                int p3 = q[-4 * xs], p2 = q[-3 * xs], p1 = q[-2 * xs], p0 = q[-xs];
                int q0 = q[0], q1 = q[xs], q2 = q[2 * xs], q3 = q[3 * xs];
                if (!no_p) {
                    q[-xs]     = (PX)(p0 + CLIP_TC2(((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3) - p0));
                    q[-2 * xs] = (PX)(p1 + CLIP_TC2(((p2 + p1 + p0 + q0 + 2) >> 2) - p1));
                    q[-3 * xs] = (PX)(p2 + CLIP_TC2(((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3) - p2));
                }
                if (!no_q) {
                    q[0]      = (PX)(q0 + CLIP_TC2(((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3) - q0));
                    q[xs]     = (PX)(q1 + CLIP_TC2(((p0 + q0 + q1 + q2 + 2) >> 2) - q1));
                    q[2 * xs] = (PX)(q2 + CLIP_TC2(((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3) - q2));
                }
            }
#undef CLIP_TC2
        } else {
            int side = (beta + (beta >> 1)) >> 3, tc_2 = tc >> 1;
            int nd_p = dp0 + dp3 < side, nd_q = dq0 + dq3 < side;
            CNT(OH_CNT_NORMAL);
            if (no_p || no_q) CNT(OH_CNT_NORMAL_PCM);
            if (!no_p && nd_p) CNT(OH_CNT_ND_P);
            if (!no_q && nd_q) CNT(OH_CNT_ND_Q);
            for (int d = 0; d < 4; d++) {
                PX *q = pix + d * ys;
                int p2 = q[-3 * xs], p1 = q[-2 * xs], p0 = q[-xs];
                int q0 = q[0], q1 = q[xs], q2 = q[2 * xs];
                int delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4;
                if (abs(delta) >= 10 * tc) {
                    CNT(OH_CNT_LINES_SKIPPED);
                    continue;
                }
                delta = oh_clip3(delta, -tc, tc);
                if ((!no_p && FN(clip_px)(p0 + delta, bd) != p0 + delta) || (!no_q && FN(clip_px)(q0 - delta, bd) != q0 - delta))
                    CNT(OH_CNT_LINES_PX_CLIPPED);
                if (!no_p) q[-xs] = (PX)FN(clip_px)(p0 + delta, bd);
                if (!no_q) q[0]   = (PX)FN(clip_px)(q0 - delta, bd);
                if (!no_p && nd_p)
                    q[-2 * xs] = (PX)FN(clip_px)(p1 + oh_clip3((((p2 + p0 + 1) >> 1) - p1 + delta) >> 1, -tc_2, tc_2), bd);
                if (!no_q && nd_q)
                    q[xs]      = (PX)FN(clip_px)(q1 + oh_clip3((((q2 + q0 + 1) >> 1) - q1 - delta) >> 1, -tc_2, tc_2), bd);
            }
        }
#undef CNT
    }
}

static void FN(loop_filter_chroma)(int bd, PX *pix, ptrdiff_t xs, ptrdiff_t ys,
                                   const int *tc_, const uint8_t *no_p_, const uint8_t *no_q_)
{
    for (int seg = 0; seg < 2; seg++, pix += 4 * ys) {
        int tc = tc_[seg] << (bd - 8);
        if (tc <= 0)
            continue;
        for (int d = 0; d < 4; d++) {
            PX *q = pix + d * ys;
            int p1 = q[-2 * xs], p0 = q[-xs], q0 = q[0], q1 = q[xs];
            int delta = oh_clip3((((q0 - p0) * 4) + p1 - q1 + 4) >> 3, -tc, tc);
            if (!no_p_[seg]) q[-xs] = (PX)FN(clip_px)(p0 + delta, bd);
            if (!no_q_[seg]) q[0]   = (PX)FN(clip_px)(q0 - delta, bd);
        }
    }
}

/* ---- SAO: hevcdsp_template.c:340-365 (band), :372-567 (edge) ---- */
static void FN(sao_band)(int bd, PX *dst, const PX *src, ptrdiff_t ds, ptrdiff_t ss,
                         const int16_t *offset_val, int band_position, int w, int h)
{
    int table[32] = { 0 };
    int shift = bd - 5;
    for (int k = 0; k < 4; k++)
        table[(k + band_position) & 31] = offset_val[k + 1];
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            dst[y * ds + x] = (PX)FN(clip_px)(src[y * ss + x] + table[src[y * ss + x] >> shift], bd);
}

/* Per-sample statement of sao_edge_filter_{0,1} (:414-567), valid because SaoOffsetVal[0] == 0
 * (hevc.c:1112-1181 never sets it): the reference filters every sample and then overwrites
 * (a) samples whose comparison neighbour would lie outside the picture (borders[], :433-471)
 * with src + offset_val[0] and, in variant 1, (b) samples whose neighbour lies in a CTB across a
 * non-filterable slice/tile edge with src (:533-566).  Both are "keep the deblocked sample". */
static void FN(sao_edge)(int bd, PX *dst, const PX *src, ptrdiff_t ds, ptrdiff_t ss,
                         const int16_t *offset_val, int eo, const int *borders, int w, int h,
                         int restore, const uint8_t *vert_edge, const uint8_t *horiz_edge,
                         const uint8_t *diag_edge)
{
    static const int8_t nb[4][2][2] = {          /* [class][a|b][dx,dy] */
        { { -1, 0 }, { 1, 0 } }, { { 0, -1 }, { 0, 1 } }, { { -1, -1 }, { 1, 1 } }, { { 1, -1 }, { -1, 1 } },
    };
    static const uint8_t category[5] = { 1, 2, 0, 3, 4 };

    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int c = src[y * ss + x];
            int keep = 0;
            for (int k = 0; k < 2 && !keep; k++) {
                int nx = x + nb[eo][k][0], ny = y + nb[eo][k][1];
                int rx = nx < 0 ? -1 : (nx >= w ? 1 : 0);       /* which neighbouring CTB */
                int ry = ny < 0 ? -1 : (ny >= h ? 1 : 0);
                if ((rx < 0 && borders[0]) || (rx > 0 && borders[2]) ||
                    (ry < 0 && borders[1]) || (ry > 0 && borders[3]))
                    keep = 1;                                    /* outside the picture */
                else if (restore && (rx || ry)) {
                    if (rx && ry) keep = diag_edge[ry < 0 ? (rx < 0 ? 0 : 1) : (rx > 0 ? 2 : 3)];
                    else if (rx)  keep = vert_edge[rx > 0];
                    else          keep = horiz_edge[ry > 0];
                }
            }
            if (keep) {
                dst[y * ds + x] = (PX)FN(clip_px)(c + offset_val[0], bd);
            } else {
                int a = src[(y + nb[eo][0][1]) * ss + x + nb[eo][0][0]];
                int b = src[(y + nb[eo][1][1]) * ss + x + nb[eo][1][0]];
                int idx = category[2 + (c > a) - (c < a) + (c > b) - (c < b)];
                dst[y * ds + x] = (PX)FN(clip_px)(c + offset_val[idx], bd);
            }
        }
}
