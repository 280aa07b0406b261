/*
 * sao.hip — pass 5: sample adaptive offset (band / edge), cur -> out
 * (gfx950; overview of the passes: kernels.hip; bit-exactness: tests/test_gpu_parity.py, tests/test_gpu_sao_forms.py)
 */
#include "kernels_common.h"

/* =========================================================================================
 * pass 5: SAO — hevcdsp_template.c:340-567 driven per CTB by sao_filter_CTB (hevc_filter.c:197-322),
 * here one whole-picture pass from the deblocked planes (cur) into the output planes (out).
 * One lane owns 8 consecutive samples of a row (8- or 16-byte accesses); a group never straddles a
 * CTB (CTB widths are multiples of 8 samples in every plane).  Rows are 256-byte aligned and padded,
 * so whole-vector accesses past the picture width stay inside the row.
 * ======================================================================================= */
template <typename PX> struct Vec8;
template <> struct Vec8<uint8_t>  { typedef unsigned int  T __attribute__((ext_vector_type(2))); enum { N = 2 }; };
template <> struct Vec8<uint16_t> { typedef unsigned int  T __attribute__((ext_vector_type(4))); enum { N = 4 }; };

template <typename PX>
static __device__ __forceinline__ typename Vec8<PX>::T load8(const GLOBAL PX *p) { return *(const GLOBAL typename Vec8<PX>::T *)p; }
template <typename PX>
static __device__ __forceinline__ void unpack8(const typename Vec8<PX>::T r, int v[8])
{
    if (sizeof(PX) == 1) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = (r[j >> 2] >> (8 * (j & 3))) & 0xff;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = (r[j >> 1] >> (16 * (j & 1))) & 0xffff;
    }
}
template <typename PX>
static __device__ __forceinline__ typename Vec8<PX>::T pack8(const int v[8])
{
    typename Vec8<PX>::T r;
    if (sizeof(PX) == 1) {
        r[0] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        r[1] = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) r[j] = v[2 * j] | (v[2 * j + 1] << 16);
    }
    return r;
}

/* the value of the previous / next lane of the same row of 16 lanes (DPP row_shr:1 / row_shl:1; 0 at the row's ends).  The 1, 2, 4
 * or 8 lanes that share a picture row are consecutive and aligned, so a row of 16 lanes holds whole groups of them. */
static __device__ __forceinline__ unsigned lane_prev(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true); }
static __device__ __forceinline__ unsigned lane_next(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true); }

/* -1, 0, 1: the sign of d as one instruction (written as min(max(d, -1), 1) the compiler makes two compares and two selects of it) */
static __device__ __forceinline__ int sign3(int d)
{
    int r;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(r) : "v"(d));
    return r;
}

/* what the edge classes need besides the lane's own samples.
 * x, y: the lane's first sample (of lanes outside the picture: the clamped position their loads use); gl / gmax: the lane's place in
 * the group of lanes that share its row / the last such place; t9: the border table (sao_border_table); m: samples from x to the CTB's
 * right edge, 0..9; ly, h: row inside the CTB and the CTB's height in the picture; tbl / off4: the offsets by sign sum (see sao_edge8) */
struct SaoEdgeCtx {
    int x, y, pw, ph, sstride, gl, gmax, t9, m, ly, h, bd, cx, cy, ctbw, ctbh, vs;
    uint64_t tbl; int off4;
    const GLOBAL uint16_t *stale; const GLOBAL uint8_t *pending;
};

/* 16x16 CTBs with subsampled chroma (DevFrame.sao_stale): sample (x0 + 8, yr) — first column of the right neighbour — as
 * sao_filter_CTB of this CTB saw it: rows touched by a horizontal chroma edge of a pending CTB row (stale_r bit 0: row cy, bit 1: row cy + 1) were not filtered yet */
static __device__ __forceinline__ int sao_stale_or(const SaoEdgeCtx &e, const int stale_r, const OhPicParams &pp, int c, int yr, int v)
{
    const int p0 = (yr & 7) == 7, ye = p0 ? yr + 1 : yr;
    if ((ye & 7) == 0 && ye > 0 && ye < e.ph && ((stale_r >> ((((ye << e.vs) >> 4) > e.cy) ? 1 : 0)) & 1))
        return e.stale[oh_sao_stale_index(&pp, c, ye >> 3, e.cx + 1) + (p0 ? 0 : 1)];
    return v;
}

/* The samples of the 3x3 regions around a CTB that SAO may not read, as 9 bits indexed by 3 * (ry + 1) + (rx + 1) (rx, ry = -1, 0, 1:
 * left / inside / right, above / inside / below): the picture's borders, and the slice / tile edges of OhSaoCtb.edge_flags (bit 0 left,
 * 1 right, 2 up, 3 bottom, 4 up-left, 5 up-right, 6 bottom-right, 7 bottom-left).  A sample with such a neighbour keeps its value
 * (hevcdsp_template.c:386-430 restores those columns, rows and corners).  The same for every sample of a CTB. */
static __device__ __forceinline__ int sao_border_table(int cx, int cy, int ctbw, int ctbh, int flags)
{
    const int f = flags;
    int t = ((f >> 4) & 1) | ((f >> 2) & 1) << 1 | ((f >> 5) & 1) << 2 | (f & 1) << 3 | ((f >> 1) & 1) << 5 | ((f >> 7) & 1) << 6 | ((f >> 3) & 1) << 7 | ((f >> 6) & 1) << 8;
    if (cx == 0)        t |= 0111;          /* octal: one digit per row of regions */
    if (cx == ctbw - 1) t |= 0444;
    if (cy == 0)        t |= 0007;
    if (cy == ctbh - 1) t |= 0700;
    return t;
}

/* sample x - 1 of the row whose samples x .. x + 7 this lane holds in `row`: from the previous lane, from memory at a CTB's first column */
template <typename PX>
static __device__ __forceinline__ int sao_left_of(const GLOBAL PX *__restrict__ src, const SaoEdgeCtx &e, const typename Vec8<PX>::T row, const int yr)
{
    int n = lane_prev(row[Vec8<PX>::N - 1]) >> (32 - 8 * sizeof(PX));
    if (e.gl == 0) {
        n = 0;
        if (e.x > 0) n = src[(size_t)yr * e.sstride + e.x - 1];
    }
    return n;
}
/* sample x + 8 of that row: from the next lane, from memory (as the reference's driver saw it) at a CTB's last column */
template <typename PX>
static __device__ __forceinline__ int sao_right_of(const GLOBAL PX *__restrict__ src, const SaoEdgeCtx &e, const typename Vec8<PX>::T row, const int yr,
                                                   const OhPicParams &pp, const int c)
{
    int n = lane_next(row[0]) & ((1 << (8 * sizeof(PX))) - 1);
    if (e.gl == e.gmax) {
        n = 0;
        if (e.x + 8 < e.pw) {
            n = src[(size_t)yr * e.sstride + e.x + 8];
            /* the chroma CTB is one 8-sample group wide in that configuration: x + 8 is the neighbour's first column */
            if (e.stale && e.cx + 2 < e.ctbw) {
                /* rows pending when the reference's driver ran this CTB's SAO: from min(cy + 1, ctbh - 2) on — from min(cy + 1, ctbh - 1) on when
                 * the CTB after the neighbour is the last of its row (its deblocking call comes a CTB earlier, hevc_filter.c:1058-1059) */
                const int r_lag = e.cx + 2 == e.ctbw - 1 ? e.ctbh - 1 : (e.ctbh >= 2 ? e.ctbh - 2 : 0), r_pending = min(e.cy + 1, r_lag);
                /* as bits: 0 = the edges of CTB row cy pending, 1 = those of row cy + 1; handed over per CTB when the picture was not decoded
                 * in raster order (tiles: DevFrame.sao_pending, OhFrame.sao_pending) */
                const int pend = e.pending ? e.pending[e.cy * e.ctbw + e.cx] : (e.cy >= r_pending ? 1 : 0) | (e.cy + 1 >= r_pending ? 2 : 0);
                n = sao_stale_or(e, pend, pp, c, yr, n);
            }
        }
    }
    return n;
}

/* first neighbour a = (x+DX, y+DY), second b = (x-DX, y-DY) (pos[][] of hevcdsp_template.c:379-384).
 *
 * Which samples keep their value is decided per lane, as 8 bits: the vertical region of a neighbour row is the same for the lane's
 * eight samples, and its horizontal region differs from "inside" only for sample 0 of a CTB's first group (neighbour x - 1) and from
 * the last sample at or before the CTB's right edge on (neighbour x + 1; e.m counts the samples up to that edge).
 *
 * Neighbour columns x - 1 and x + 8 come from the adjacent lanes' registers.  Every lane of the wave takes part (no lane has left),
 * also the lanes whose samples lie outside the picture; those loaded a clamped position, so what they hold is not the neighbour.  It
 * never reaches a result: a lane at x >= pw is only ever the right neighbour of the picture's last group in a row, that group lies in
 * the last CTB column, and there the right-hand regions are in the table (cx == ctbw - 1), so the one sample that looks at x + 8 is
 * kept.  Lanes of rows y >= ph share their row only with lanes that store nothing either. */
template <typename PX, int DX, int DY>
static __device__ __forceinline__ void sao_edge8(const GLOBAL PX *__restrict__ src, const SaoEdgeCtx &e, const typename Vec8<PX>::T raw, const int v[8], int r[8],
                                                 const OhPicParams &pp, const int c)
{
    typedef typename Vec8<PX>::T V;
    int a[10], b[10];                                       /* samples x-1..x+8 of rows y+DY and y-DY */
    a[0] = b[0] = a[9] = b[9] = 0;
    int ta, tb;                                             /* the table's row of regions for each neighbour row: bit 0 left, 1 inside, 2 right */
    if (DY == 0) {                                          /* both neighbours lie in the lane's own row */
#pragma unroll
        for (int j = 0; j < 8; j++) a[1 + j] = b[1 + j] = v[j];
        a[0] = sao_left_of<PX>(src, e, raw, e.y);
        b[9] = sao_right_of<PX>(src, e, raw, e.y, pp, c);
        ta = tb = (e.t9 >> 3) & 7;
    } else {
        const int ya = max(e.y - 1, 0), yb = min(e.y + 1, e.ph - 1);
        const V ra = load8<PX>(src + (size_t)ya * e.sstride + e.x), rb = load8<PX>(src + (size_t)yb * e.sstride + e.x);
        unpack8<PX>(ra, a + 1);
        unpack8<PX>(rb, b + 1);
        if (DX < 0) { a[0] = sao_left_of<PX>(src, e, ra, ya); b[9] = sao_right_of<PX>(src, e, rb, yb, pp, c); }
        if (DX > 0) { a[9] = sao_right_of<PX>(src, e, ra, ya, pp, c); b[0] = sao_left_of<PX>(src, e, rb, yb); }
        ta = (e.ly == 0 ? e.t9 : e.t9 >> 3) & 7;
        tb = (e.ly + 1 >= e.h ? e.t9 >> 6 : e.t9 >> 3) & 7;
    }
    const int ge = ((0x1ff << e.m) >> 1) & 0xff;            /* samples whose neighbour x + 1 lies right of the CTB */
    int keep = (0xff << e.m) & 0xff;                        /* samples right of the picture */
    if (DX == 0) {
        if ((ta | tb) & 2) keep = 0xff;
    } else {
        const int tl = DX < 0 ? ta : tb, tr = DX < 0 ? tb : ta;     /* the rows of the neighbours at x - 1 and at x + 1 */
        keep |= (tl & 2 ? 0xfe : 0) | ((e.gl == 0 ? tl : tl >> 1) & 1);
        keep |= (tr & 2 ? ge ^ 0xff : 0) | (tr & 4 ? ge : 0);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int na = a[1 + j + DX], nb = b[1 + j - DX];
        /* sign sum + 2: 0, 1, 2, 3, 4 take offsets 1, 2, 0, 3, 4 (edge_idx[] of :372); e.tbl holds the first four as 16-bit fields */
        const int idx = 2 + sign3(v[j] - na) + sign3(v[j] - nb);
        const int o = idx == 4 ? e.off4 : (int16_t)(e.tbl >> (16 * (idx & 3)));
        r[j] = (keep >> j) & 1 ? v[j] : clip_px(v[j] + o, e.bd);
    }
}

/* Lane -> sample mapping: a wave covers ONE CTB-wide strip (wc samples x 512/wc rows); a workgroup of 4 waves covers 4 such strips
 * stacked vertically.  grid = (CTB columns, strips of rows of every plane, pictures).
 * ONE_CTB: in every plane a wave's strip is no taller than a CTB (the launcher knows), so the CTB's parameters, the SAO type and class
 * and the border table are the same for the wave: they live in scalar registers and the type dispatch is not divergent.  Otherwise
 * (16x16 CTBs, 32x32 with vertically subsampled chroma) a strip spans several CTBs of one column and they are per lane. */
template <typename PX, bool ONE_CTB>
__global__ __launch_bounds__(256) void sao_kernel(const OhBatch B, const int strips_luma, const int strips_chroma)
{
    typedef typename Vec8<PX>::T V;
    const DevFrame *__restrict__ f = B.f[blockIdx.z];
    const OhPicParams &pp = f->pp;
    /* grid.y: the luma strips, then the strips of Cb, then those of Cr (a chroma plane of 4:2:0 needs a quarter of the
     * luma plane's workgroups: no workgroup is launched just to exit) */
    int strip = blockIdx.y, c = 0;
    if (strip >= strips_luma) {
        strip -= strips_luma;
        c = strip >= strips_chroma ? 2 : 1;
        strip -= (c - 1) * strips_chroma;
    }
    const int pw = f->cur.w[c], ph = f->cur.h[c];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hs = hsh(pp, c), vs = vsh(pp, c), lc = pp.log2_ctb_size;
    const int log2_gx = lc - hs - 3;                                  /* 8-sample groups per CTB row: 1 << log2_gx */
    const int rows_per_wave = 64 >> log2_gx;
    const int gmax = (1 << log2_gx) - 1, gl = lane & gmax;
    const int xs = (blockIdx.x << (log2_gx + 3)) + (gl << 3);
    const int ys = (strip * 4 + wave) * rows_per_wave + (lane >> log2_gx);
    if (__builtin_amdgcn_readfirstlane(ys) >= ph)                     /* lane 0 has the wave's first row: the whole wave lies below the picture */
        return;
    /* No single lane leaves before the store: its neighbours read its registers (sao_edge8).  A lane outside the picture works on the
     * picture's last group / last row instead, so that all its addresses are good, and stores nothing. */
    const bool inside = xs < pw && ys < ph;
    const int x = min(xs, (pw - 1) & ~7), y = min(ys, ph - 1);
    const int bd = pp.bit_depth;
    const int ctbw = (pp.width + (1 << lc) - 1) >> lc, ctbh = (pp.height + (1 << lc) - 1) >> lc;
    const int sstride = f->cur.stride[c];
    const GLOBAL PX *__restrict__ src = G_CONST(PX, f->cur.p[c]);
    GLOBAL PX *__restrict__ dst = G_MUT(PX, f->out.p[c]) + (size_t)ys * f->out.stride[c] + xs;
    const int cx = blockIdx.x;
    int cy = (y << vs) >> lc;
    if (ONE_CTB) cy = __builtin_amdgcn_readfirstlane(cy);
    /* the CTB's parameters as dwords (the array is 256-byte aligned in the work-list arena, an entry is 40 bytes):
     * [7] ..., band_position[0], [1]; [8] band_position[2], eo_class[0..2]; [9] type_idx[0..2], edge_flags */
    const GLOBAL uint32_t *s = G_CONST(uint32_t, f->sao) + (size_t)(cy * ctbw + cx) * (sizeof(OhSaoCtb) / 4);
    const uint32_t s9 = s[9];
    const int type = (s9 >> (8 * c)) & 0xff;
    const V raw = load8<PX>(src + (size_t)y * sstride + x);
    V res = raw;
    if (type != 0) {                                        /* off: the samples as they were loaded; the PCM restore changes nothing there */
        /* offset_val[c][0..4]: 10 bytes from byte 10 * c on, brought to dword alignment */
        const GLOBAL uint32_t *so = s + ((10 * c) >> 2);
        const int sh = c == 1 ? 16 : 0;
        const uint32_t o0 = so[0], o1 = so[1], o2 = so[2];
        const uint32_t q0 = (uint32_t)((((uint64_t)o1 << 32) | o0) >> sh), q1 = (uint32_t)((((uint64_t)o2 << 32) | o1) >> sh), q2 = o2 >> sh;
        int v[8], r[8];
        unpack8<PX>(raw, v);
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = v[j];
        if (type == 1) {                                    /* band, :340-365: bands bp .. bp + 3 (mod 32) take offsets 1..4 */
            const uint32_t s8 = s[8];
            const int bp = c == 2 ? s8 & 0xff : (s[7] >> (16 + 8 * c)) & 0xff;
            const uint64_t tbl = (uint64_t)(q0 >> 16) | ((uint64_t)q1 << 16) | ((uint64_t)(q2 & 0xffff) << 48);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int k = ((v[j] >> (bd - 5)) - bp) & 31;
                const int o = (int16_t)(tbl >> (16 * (k & 3)));
                r[j] = k < 4 ? clip_px(v[j] + o, bd) : v[j];
            }
        } else if (type == 2) {                             /* edge, :372-567 (per-sample form) */
            const int eo = (s[8] >> (8 + 8 * c)) & 0xff;
            const int x0 = (cx << lc) >> hs, y0 = (cy << lc) >> vs;
            const int w = min((1 << lc) >> hs, pw - x0), h = min((1 << lc) >> vs, ph - y0);
            SaoEdgeCtx ec;
            ec.x = x; ec.y = y; ec.pw = pw; ec.ph = ph; ec.sstride = sstride; ec.gl = gl; ec.gmax = gmax;
            ec.t9 = sao_border_table(cx, cy, ctbw, ctbh, s9 >> 24);
            ec.m = min(max(w - (gl << 3), 0), 9);
            ec.ly = y - y0; ec.h = h; ec.bd = bd; ec.cx = cx; ec.cy = cy; ec.ctbw = ctbw; ec.ctbh = ctbh; ec.vs = vs;
            ec.tbl = (uint64_t)(q0 >> 16) | ((uint64_t)(q1 & 0xffff) << 16) | ((uint64_t)(q0 & 0xffff) << 32) | ((uint64_t)(q1 >> 16) << 48);
            ec.off4 = (int16_t)q2;
            ec.stale = c && pp.deblock_enabled ? G_CONST(uint16_t, f->sao_stale) : nullptr;
            ec.pending = G_CONST(uint8_t, f->sao_pending);
            switch (eo) {                                   /* compile-time neighbour offsets: no indexed registers */
            case 0:  sao_edge8<PX, -1, 0>(src, ec, raw, v, r, pp, c); break;
            case 1:  sao_edge8<PX, 0, -1>(src, ec, raw, v, r, pp, c); break;
            case 2:  sao_edge8<PX, -1, -1>(src, ec, raw, v, r, pp, c); break;
            default: sao_edge8<PX, 1, -1>(src, ec, raw, v, r, pp, c); break;
            }
        }
        if (f->is_pcm && (pp.transquant_bypass_enable || pp.pcm_loop_filter_disable)) {
            /* restore_tqb_pixels (hevc_filter.c:163-193) with its geometry quirks: the min-PU range is
             * derived from the CTB's LUMA origin plus the COMPONENT's size, and the row copy length
             * is (min_pu >> hshift) BYTES whatever the sample size. */
            const int l = pp.log2_min_pu_size, mpw = pp.width >> l;
            const int X0 = cx << lc, Y0 = cy << lc;
            const int wc = min((1 << lc) >> hs, pw - (X0 >> hs)), hc = min((1 << lc) >> vs, ph - (Y0 >> vs));
            const int py = (y << vs) >> l;
            const GLOBAL uint8_t *pcm = G_CONST(uint8_t, f->is_pcm);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int px = ((x + j) << hs) >> l;
                if (px >= (X0 >> l) && px < ((X0 + wc) >> l) && py >= (Y0 >> l) && py < ((Y0 + hc) >> l) && pcm[py * mpw + px]) {
                    int sx = (px << l) >> hs;
                    int len_samples = ((1 << l) >> hs) / (int)sizeof(PX);
                    if (x + j - sx < len_samples)
                        r[j] = v[j];
                }
            }
        }
        res = pack8<PX>(r);
    }
    if (inside)
        __builtin_nontemporal_store(res, (GLOBAL V *)dst);  /* the output is next read by another picture's MC: stream it past the L2 */
}

/* =========================================================================================
 * launcher
 * ======================================================================================= */
template <typename PX>
static void sao_launch(const bool one_ctb, const dim3 grid, hipStream_t st, const OhBatch *B, const int sl, const int sc)
{
    if (one_ctb) hipLaunchKernelGGL(HIP_KERNEL_NAME(sao_kernel<PX, true>), grid, dim3(256), 0, st, *B, sl, sc);
    else         hipLaunchKernelGGL(HIP_KERNEL_NAME(sao_kernel<PX, false>), grid, dim3(256), 0, st, *B, sl, sc);
}

extern "C" void ohk_sao(const OhBatch *B, int n, const OhPicParams *p, hipStream_t st)
{
    const int lc = p->log2_ctb_size, ctbw = (p->width + (1 << lc) - 1) >> lc;
    const int hs = p->chroma_format_idc == 1 || p->chroma_format_idc == 2, vs = p->chroma_format_idc == 1;
    const int rows_luma = 4 * (64 >> (lc - 3)), rows_chroma = 4 * (64 >> (lc - hs - 3));     /* rows per workgroup: 4 waves x (512 / CTB width) */
    const int sl = (p->height + rows_luma - 1) / rows_luma;
    const int sc = p->chroma_format_idc ? ((p->height >> vs) + rows_chroma - 1) / rows_chroma : 0;
    /* a wave's rows (a power of two, as a CTB's) lie in one CTB when they are no more than the CTB has in that plane */
    const bool one_ctb = rows_luma / 4 <= (1 << lc) && (!p->chroma_format_idc || rows_chroma / 4 <= (1 << lc) >> vs);
    dim3 grid(ctbw, sl + 2 * sc, n);
    if (p->bit_depth == 8) sao_launch<uint8_t>(one_ctb, grid, st, B, sl, sc);
    else                   sao_launch<uint16_t>(one_ctb, grid, st, B, sl, sc);
}
