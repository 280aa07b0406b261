/*
 * convert.hip — finished pictures -> standard images in caller-owned device memory (oh_pics_convert; the exact definitions are in
 * DESIGN.md §3b and tests/convert_model.py).
 *
 * Memory-bound streaming: every source sample the window covers is read once from HBM, every image byte written once.  One workgroup
 * (256 lanes) per segment of up to CW output samples (YUV) or pixels (RGB) of one image row; grid (segments, image rows, pictures of
 * the launch — all of them share one geometry; their plane addresses are in the kernel arguments).  Three phases, two barriers:
 *   1. stage   the source row(s) of the segment go to LDS as whole 16-byte granules (global_load_dwordx4).  A plane's rows are padded
 *              to 256 bytes, so the granules around an unaligned window edge stay inside the row.  The second chroma row of the
 *              linear 4:2:0 filter is a row the segments of the neighbouring image rows read too: it comes from L2.
 *   2. compute each lane converts samples out of LDS and writes the output samples into an LDS image of the destination bytes, placed
 *              at the destination's address modulo 16;
 *   3. store   the 16-byte-aligned middle of the destination with global_store_dwordx4, the at most 15 + 15 bytes of head and tail
 *              byte by byte (odd widths and unaligned image strides, e.g. a torch N x H x W x 3 u8 tensor).
 * Templates on what changes the inner loop (input sample type, output sample type, layout); the chroma format, filter, range and
 * channel count are uniform branches.
 */
#include "convert_common.h"

namespace {

/* YUV formats: image row r is a row of the Y plane, of Cb or Cr (planar) or of the interleaved CbCr plane (semi-planar).
 * TI -> O: u8 -> u8 (copy), u16 -> u16 (copy, shifted to the MSB in the semi-planar form), u16 -> u8 (rounded, saturated). */
template <typename TI, int O, int LAY>
__global__ __launch_bounds__(THREADS) void convert_yuv_kernel(const OhConvArgs a)
{
    typedef typename OutT<O>::T TO;
    constexpr int CW = 4096, HALF = CW / 2 * (int)sizeof(TI) + 32;
    __shared__ __attribute__((aligned(16))) uint8_t in_l[2 * HALF];
    __shared__ __attribute__((aligned(16))) uint8_t out_l[CW * sizeof(TO) + 16];
    const int pic = blockIdx.z, r = blockIdx.y, x0 = blockIdx.x * CW;
    const int W = a.W, H = a.H, hs = a.cf == 1 || a.cf == 2, vs = a.cf == 1, Wc = W >> hs, Hc = H >> vs;
    int c, y, n;
    size_t off;                                                 /* samples from the image start to the row */
    if (r < H) {
        c = 0; y = r; n = W; off = (size_t)r * W;
    } else if (LAY == L_PLANAR) {
        const int rr = r - H;
        c = rr < Hc ? 1 : 2; y = rr - (c - 1) * Hc; n = Wc; off = (size_t)W * H + (size_t)(c - 1) * Wc * Hc + (size_t)y * Wc;
    } else {
        c = 1; y = r - H; n = 2 * Wc; off = (size_t)W * H + (size_t)y * 2 * Wc;
    }
    if (x0 >= n)
        return;
    const int cnt = min(CW, n - x0);
    uint8_t *dst = (uint8_t *)a.dst + pic * a.image_stride + (off + x0) * sizeof(TO);
    const int cs = c ? hs : 0, row = (a.top >> (c ? vs : 0)) + y;
    const bool inter = LAY == L_SEMI && c;                      /* CbCr: x0 and cnt are even */
    int b0, b1 = 0;
    if (!inter) {
        b0 = stage<TI>(in_l, (const uint8_t *)a.src[pic][c] + (size_t)row * a.pitch[c] + (size_t)((a.left >> cs) + x0) * sizeof(TI), cnt);
    } else {
        const size_t o = (size_t)row * a.pitch[1] + (size_t)((a.left >> hs) + (x0 >> 1)) * sizeof(TI);
        b0 = stage<TI>(in_l, (const uint8_t *)a.src[pic][1] + o, cnt >> 1);
        b1 = stage<TI>(in_l + HALF, (const uint8_t *)a.src[pic][2] + o, cnt >> 1);
    }
    __syncthreads();
    const TI *s0 = (const TI *)in_l, *s1 = (const TI *)(in_l + HALF);
    TO *o = (TO *)(out_l + ((uintptr_t)dst & 15));
    const int bd = a.bd, sh = LAY == L_SEMI ? 16 - bd : 0;
    for (int i = threadIdx.x; i < cnt; i += THREADS) {
        const int v = inter ? ((i & 1) ? s1[b1 + (i >> 1)] : s0[b0 + (i >> 1)]) : s0[b0 + i];
        if constexpr (sizeof(TI) == 1)
            o[i] = (TO)v;
        else if constexpr (O == O_U8)
            o[i] = (TO)min((v + (1 << (bd - 9))) >> (bd - 8), 255);
        else
            o[i] = (TO)(v << sh);
    }
    __syncthreads();
    store_out(dst, out_l, cnt * (int)sizeof(TO));
}

/* RGB formats: image row y, chroma onto the luma grid in coded-plane coordinates (clamped at the coded plane's edges), the matrix in
 * int32 with the coefficients of oh_convert_coeffs, then the output sample type */
template <typename TI, int O, int LAY>
__global__ __launch_bounds__(THREADS) void convert_rgb_kernel(const OhConvArgs a)
{
    typedef typename OutT<O>::T TO;
    constexpr int CW = 2048 / (int)sizeof(TO);
    constexpr int RB = ((CW / 2 + 1) * (int)sizeof(TI) + 32 + 15) / 16 * 16;       /* one staged 4:2:x chroma row; 4:4:4 takes two */
    constexpr int OUTB = (LAY == L_RGBP ? 1 : 4) * CW * (int)sizeof(TO) + 16;
    __shared__ __attribute__((aligned(16))) uint8_t lum[CW * sizeof(TI) + 32];
    __shared__ __attribute__((aligned(16))) uint8_t chr[4 * RB];                   /* Cb row j0, Cb row j1, Cr row j0, Cr row j1 */
    __shared__ __attribute__((aligned(16))) uint8_t out_l[LAY == L_RGBP ? 3 : 1][OUTB];
    const int pic = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * CW;
    const int W = a.W, H = a.H;
    if (x0 >= W)
        return;
    const int cnt = min(CW, W - x0), X0 = a.left + x0, Y = a.top + y;
    RgbRows<TI> in;
    in.stage_rows(a, pic, X0, Y, cnt, lum, chr, RB);
    __syncthreads();
    const RgbMatrix mt(a.k);
    const int nc = a.nc;
    const size_t plane = (size_t)W * H;
    uint8_t *dst = (uint8_t *)a.dst + pic * a.image_stride + ((size_t)y * W + x0) * (LAY == L_RGBP ? 1 : nc) * sizeof(TO);
    TO *o0 = (TO *)(out_l[0] + ((uintptr_t)dst & 15));
    TO *o1 = o0, *o2 = o0;
    if constexpr (LAY == L_RGBP) {
        o1 = (TO *)(out_l[LAY == L_RGBP ? 1 : 0] + ((uintptr_t)(dst + plane * sizeof(TO)) & 15));
        o2 = (TO *)(out_l[LAY == L_RGBP ? 2 : 0] + ((uintptr_t)(dst + 2 * plane * sizeof(TO)) & 15));
    }
    for (int i = threadIdx.x; i < cnt; i += THREADS) {
        int u, v, R, G, B;
        in.chroma(a, X0 + i, i, mt.mid, u, v);
        mt.rgb((int)in.L[i], u, v, R, G, B);
        if constexpr (LAY == L_RGBP) {
            o0[i] = out_sample<O>(R); o1[i] = out_sample<O>(G); o2[i] = out_sample<O>(B);
        } else {
            TO *q = o0 + i * nc;
            q[0] = out_sample<O>(R); q[1] = out_sample<O>(G); q[2] = out_sample<O>(B);
            if (nc == 4) q[3] = out_sample<O>(mt.mx);
        }
    }
    __syncthreads();
    if constexpr (LAY == L_RGBP) {
        for (int c = 0; c < 3; c++)
            store_out(dst + c * plane * sizeof(TO), out_l[c], cnt * (int)sizeof(TO));
    } else {
        store_out(dst, out_l[0], cnt * nc * (int)sizeof(TO));
    }
}

template <typename TI, int O, int LAY>
void launch(const OhConvArgs *a, int n, hipStream_t st)
{
    const bool yuv = LAY == L_PLANAR || LAY == L_SEMI;
    const int cw = yuv ? 4096 : 2048 / (int)sizeof(typename OutT<O>::T);
    const int hs = a->cf == 1 || a->cf == 2, vs = a->cf == 1, Hc = a->H >> vs;
    const int rows = LAY == L_PLANAR ? a->H + (a->cf ? 2 * Hc : 0) : LAY == L_SEMI ? a->H + Hc : a->H;
    /* the longest image row: an interleaved CbCr row holds 2 * (W >> hs) samples, twice the luma row's in 4:4:4 (NV24 / P410) */
    const int longest = LAY == L_SEMI ? max(a->W, 2 * (a->W >> hs)) : a->W;
    const dim3 grid((unsigned)((longest + cw - 1) / cw), (unsigned)rows, (unsigned)n);
    if constexpr (LAY == L_PLANAR || LAY == L_SEMI)
        convert_yuv_kernel<TI, O, LAY><<<grid, THREADS, 0, st>>>(*a);
    else
        convert_rgb_kernel<TI, O, LAY><<<grid, THREADS, 0, st>>>(*a);
}

template <int LAY>
void launch_rgb(const OhConvArgs *a, int sample, int n, hipStream_t st)
{
    const bool wide = a->bd > 8;
    switch (sample) {
    case OH_CONV_U8:  wide ? launch<uint16_t, O_U8, LAY>(a, n, st)  : launch<uint8_t, O_U8, LAY>(a, n, st);  break;
    case OH_CONV_U16: wide ? launch<uint16_t, O_U16, LAY>(a, n, st) : launch<uint8_t, O_U16, LAY>(a, n, st); break;
    case OH_CONV_F16: wide ? launch<uint16_t, O_F16, LAY>(a, n, st) : launch<uint8_t, O_F16, LAY>(a, n, st); break;
    default:          wide ? launch<uint16_t, O_F32, LAY>(a, n, st) : launch<uint8_t, O_F32, LAY>(a, n, st); break;
    }
}

template <int LAY>
void launch_yuv(const OhConvArgs *a, int sample, int n, hipStream_t st)
{
    if (a->bd == 8)
        launch<uint8_t, O_U8, LAY>(a, n, st);
    else if (sample == OH_CONV_U8)
        launch<uint16_t, O_U8, LAY>(a, n, st);
    else
        launch<uint16_t, O_U16, LAY>(a, n, st);
}

} // namespace


extern "C" void ohk_convert(const OhConvArgs *a, int format, int sample, int n, hipStream_t st)
{
    switch (format) {
    case OH_CONV_PLANAR:     launch_yuv<L_PLANAR>(a, sample, n, st); break;
    case OH_CONV_SEMIPLANAR: launch_yuv<L_SEMI>(a, sample, n, st); break;
    case OH_CONV_RGB_PLANAR: launch_rgb<L_RGBP>(a, sample, n, st); break;
    default:                 launch_rgb<L_RGBI>(a, sample, n, st); break;
    }
}
