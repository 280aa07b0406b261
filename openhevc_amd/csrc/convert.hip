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
#include "../../include/ohevc_hip.h"
#include "kernels_common.h"

namespace {

constexpr int THREADS = 256;
enum { L_PLANAR, L_SEMI, L_RGBP, L_RGBI };          /* YUV planar, YUV semi-planar, RGB planar, RGB / RGBA interleaved */
enum { O_U8, O_U16, O_F16, O_F32 };                 /* output sample type */

template <int O> struct OutT { typedef uint8_t T; };
template <> struct OutT<O_U16> { typedef uint16_t T; };
template <> struct OutT<O_F16> { typedef uint16_t T; };
template <> struct OutT<O_F32> { typedef float T; };

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
    const int hs = a.cf == 1 || a.cf == 2, vs = a.cf == 1, lin = a.filter;
    const int bl = stage<TI>(lum, (const uint8_t *)a.src[pic][0] + (size_t)Y * a.pitch[0] + (size_t)X0 * sizeof(TI), cnt);
    int c_lo = 0, bu0 = 0, bu1 = 0, bv0 = 0, bv1 = 0;
    if (a.cf) {
        c_lo = X0 >> hs;
        const int m = min((X0 + cnt) >> hs, a.cw - 1) - c_lo + 1;                    /* with the right neighbour of the linear filter */
        const int j0 = Y >> vs;
        bu0 = stage<TI>(chr, (const uint8_t *)a.src[pic][1] + (size_t)j0 * a.pitch[1] + (size_t)c_lo * sizeof(TI), m);
        bv0 = stage<TI>(chr + 2 * RB, (const uint8_t *)a.src[pic][2] + (size_t)j0 * a.pitch[2] + (size_t)c_lo * sizeof(TI), m);
        if (lin && vs) {                                        /* chroma row j sits between luma rows 2j and 2j + 1 */
            const int j1 = min(max(j0 - 1 + 2 * (Y & 1), 0), a.ch - 1);
            bu1 = stage<TI>(chr + RB, (const uint8_t *)a.src[pic][1] + (size_t)j1 * a.pitch[1] + (size_t)c_lo * sizeof(TI), m);
            bv1 = stage<TI>(chr + 3 * RB, (const uint8_t *)a.src[pic][2] + (size_t)j1 * a.pitch[2] + (size_t)c_lo * sizeof(TI), m);
        }
    }
    __syncthreads();
    const TI *L = (const TI *)lum, *U0 = (const TI *)chr, *U1 = (const TI *)(chr + RB), *V0 = (const TI *)(chr + 2 * RB),
             *V1 = (const TI *)(chr + 3 * RB);
    const int cy = a.k[0], crv = a.k[1], cgu = a.k[2], cgv = a.k[3], cbu = a.k[4], yoff = a.k[5], mid = a.k[6], S = a.k[7];
    const int rnd = 1 << (S - 1), mx = (1 << a.k[8]) - 1, nc = a.nc, cwm = a.cw - 1;
    const size_t plane = (size_t)W * H;
    uint8_t *dst = (uint8_t *)a.dst + pic * a.image_stride + ((size_t)y * W + x0) * (LAY == L_RGBP ? 1 : nc) * sizeof(TO);
    TO *o0 = (TO *)(out_l[0] + ((uintptr_t)dst & 15));
    TO *o1 = o0, *o2 = o0;
    if constexpr (LAY == L_RGBP) {
        o1 = (TO *)(out_l[LAY == L_RGBP ? 1 : 0] + ((uintptr_t)(dst + plane * sizeof(TO)) & 15));
        o2 = (TO *)(out_l[LAY == L_RGBP ? 2 : 0] + ((uintptr_t)(dst + 2 * plane * sizeof(TO)) & 15));
    }
    for (int i = threadIdx.x; i < cnt; i += THREADS) {
        const int X = X0 + i;
        int u = mid, v = mid;
        if (a.cf == 3) {
            u = U0[bu0 + i]; v = V0[bv0 + i];
        } else if (a.cf) {
            const int k = (X >> 1) - c_lo, k2 = (X & 1) ? min((X + 1) >> 1, cwm) - c_lo : k;
            if (!lin) {
                u = U0[bu0 + k]; v = V0[bv0 + k];
            } else {
                const int hu = U0[bu0 + k] + U0[bu0 + k2], hv = V0[bv0 + k] + V0[bv0 + k2];   /* 2x scale */
                if (vs) {
                    u = (3 * hu + U1[bu1 + k] + U1[bu1 + k2] + 4) >> 3;
                    v = (3 * hv + V1[bv1 + k] + V1[bv1 + k2] + 4) >> 3;
                } else {
                    u = (hu + 1) >> 1;
                    v = (hv + 1) >> 1;
                }
            }
        }
        const int dy = cy * ((int)L[bl + i] - yoff) + rnd, du = u - mid, dv = v - mid;
        const int R = min(max((dy + crv * dv) >> S, 0), mx);
        const int G = min(max((dy + cgu * du + cgv * dv) >> S, 0), mx);
        const int B = min(max((dy + cbu * du) >> S, 0), mx);
        if constexpr (LAY == L_RGBP) {
            o0[i] = out_sample<O>(R); o1[i] = out_sample<O>(G); o2[i] = out_sample<O>(B);
        } else {
            TO *q = o0 + i * nc;
            q[0] = out_sample<O>(R); q[1] = out_sample<O>(G); q[2] = out_sample<O>(B);
            if (nc == 4) q[3] = out_sample<O>(mx);
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

static_assert(sizeof(((OhConvArgs *)nullptr)->src) / sizeof(((OhConvArgs *)nullptr)->src[0]) == OH_CONV_MAX_PICS, "one launch's pictures");

extern "C" void ohk_convert(const OhConvArgs *a, int format, int sample, int n, hipStream_t st)
{
    switch (format) {
    case OH_CONV_PLANAR:     launch_yuv<L_PLANAR>(a, sample, n, st); break;
    case OH_CONV_SEMIPLANAR: launch_yuv<L_SEMI>(a, sample, n, st); break;
    case OH_CONV_RGB_PLANAR: launch_rgb<L_RGBP>(a, sample, n, st); break;
    default:                 launch_rgb<L_RGBI>(a, sample, n, st); break;
    }
}
