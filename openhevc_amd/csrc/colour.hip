/*
 * colour.hip — finished pictures -> RGB images in another transfer function and other primaries (oh_pics_convert_colour; the exact
 * definition is in DESIGN.md §3d and tests/colour_model.py): HDR (PQ / HLG, BT.2020) to SDR or to linear light.
 *
 * The shape of convert.hip's RGB kernel — stage the luma and chroma granules of a row segment to LDS, compute into an LDS image of the
 * destination bytes, store 16-byte aligned with a byte head and tail — with four integer stages between the H.273 matrix (here always
 * to 16 bit) and the output sample:
 *   1. source curve   A, 4096 linear segments over the 16-bit code -> linear light, 2^30 = full scale
 *   2. gain           one Q20 factor looked up in G at a norm of the three channels (the HLG OOTF, the BT.2390 tone curve)
 *   3. primaries      3 x 3 in Q20 with 64-bit sums, clipped to [0, 2^30]
 *   4. output         LINEAR: one int-to-float conversion and one f32 multiply; SRGB / GAMMA24: the code looked up in B
 * G and B are piecewise-logarithmic (64 segments per octave above 128, every integer below).  No floating-point library function and
 * no float expression the compiler could contract: the tables are built on the host (pics_math.hip: oh_colour_tables).
 *
 * The three tables (29 KB) live in LDS beside the staging arrays.  A workgroup loads them once and converts OH_COL_ROWS image rows of
 * its segment, so the table loads (out of L2) stay a fraction of the pixel traffic.  Stages 2 and 3 are skipped (uniform branches)
 * where they are the identity: no tone curve and no HLG; equal primaries.
 */
#include "colour_common.h"

namespace {

/* P(T, l) of DESIGN.md §3d for 0 <= l <= 2^30, without a branch: below 128 s is 0, so k = l, the fraction is 0 and the second read
 * (T[l + 1], which exists) does not count.  x is l with its bit s + 6 moved to bit 30: the six bits below it are l >> s, the twelve
 * below those the fraction — shifted-in zeros for s <= 12, the truncation of fr >> (s - 12) above. */
__device__ __forceinline__ int lut(const int32_t *T, int l)
{
    const int s = max(25 - __clz(l), 0);                       /* floor(log2 l) - 6 */
    const unsigned x = (unsigned)l << (24 - s);
    const int k = (s << 6) + (int)(x >> 24), f12 = (int)((x >> 12) & 4095u);
    const int t0 = T[k], t1 = T[k + 1];
    return t0 + ((__mul24(t1 - t0, f12) + 2048) >> 12);            /* |t1 - t0| < 2^19 from entry 128 on, f12 < 2^12 */
}

template <int O>
__device__ __forceinline__ typename OutT<O>::T linear_sample(int m, float K)
{
    const float f = __fmul_rn((float)m, K);
    if constexpr (O == O_F32)
        return f;
    else
        return f >= 65520.0f ? (uint16_t)0x7BFF : f16_rne(f);  /* saturates at the largest finite f16 */
}

/* a 16-bit output code as the output sample */
template <int O>
__device__ __forceinline__ typename OutT<O>::T code_sample(int c)
{
    if constexpr (O == O_U8)
        return (uint8_t)((unsigned)(c + 128) / 257u);
    else
        return out_sample<O>(c);
}

template <typename TI, int O, int LAY>
__global__ __launch_bounds__(THREADS) void colour_rgb_kernel(const OhColArgs ca)
{
    typedef typename OutT<O>::T TO;
    const OhConvArgs &a = ca.c;
    constexpr int CW = 2048 / (int)sizeof(TO);
    constexpr int RB = ((CW / 2 + 1) * (int)sizeof(TI) + 32 + 15) / 16 * 16;       /* one staged 4:2:x chroma row; 4:4:4 takes two */
    constexpr int OUTB = (LAY == L_RGBP ? 1 : 4) * CW * (int)sizeof(TO) + 16;
    __shared__ __attribute__((aligned(16))) uint8_t lum[CW * sizeof(TI) + 32];
    __shared__ __attribute__((aligned(16))) uint8_t chr[4 * RB];
    __shared__ __attribute__((aligned(16))) uint8_t out_l[LAY == L_RGBP ? 3 : 1][OUTB];
    __shared__ __attribute__((aligned(16))) int32_t tab[OH_COLT_N];
    static_assert(sizeof(lum) + sizeof(chr) + sizeof(out_l) + sizeof(tab) <= 64 * 1024, "static LDS of one workgroup");
    const int pic = blockIdx.z, y0 = blockIdx.y * OH_COL_ROWS, x0 = blockIdx.x * CW;
    const int W = a.W, H = a.H;
    if (x0 >= W)
        return;
    for (int i = threadIdx.x; i < OH_COLT_N / 4; i += THREADS)  /* visible after the first row's barrier */
        ((uint4v *)tab)[i] = ((const GLOBAL uint4v *)ca.tab)[i];
    const int32_t *A = tab, *Gt = tab + OH_COLT_G, *Bt = tab + OH_COLT_B;
    const int cnt = min(CW, W - x0), X0 = a.left + x0, y1 = min(y0 + OH_COL_ROWS, H);
    const RgbMatrix mt(a.k);
    const int32_t *mc = ca.misc;
    const bool luma_norm = mc[12] == OH_NORM_LUMA, by_table = mc[13] != 0, gain_on = mc[15] != 0, mat_on = mc[16] != 0;
    const float K = __int_as_float(mc[14]);
    const int nc = a.nc;
    const size_t plane = (size_t)W * H;
    for (int y = y0; y < y1; y++) {
        RgbRows<TI> in;
        in.stage_rows(a, pic, X0, a.top + y, cnt, lum, chr, RB);
        __syncthreads();                                        /* also: every lane is done with the previous row's out_l */
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
            int l0 = src_curve(A, R), l1 = src_curve(A, G), l2 = src_curve(A, B);
            if (gain_on) {
                const int nrm = luma_norm ? luma_norm_of(mc[9], mc[10], mc[11], l0, l1, l2) : max(l0, max(l1, l2));
                const int g = lut(Gt, nrm);
                l0 = (int)((mulu64(l0, g) + (1u << 19)) >> 20);
                l1 = (int)((mulu64(l1, g) + (1u << 19)) >> 20);
                l2 = (int)((mulu64(l2, g) + (1u << 19)) >> 20);
            }
            if (mat_on) {
                const int a0 = l0, a1 = l1, a2 = l2;
                const int64_t lo = 0, hi = FS;
                l0 = (int)min(max((mul64(mc[0], a0) + mul64(mc[1], a1) + mul64(mc[2], a2) + (1 << 19)) >> 20, lo), hi);
                l1 = (int)min(max((mul64(mc[3], a0) + mul64(mc[4], a1) + mul64(mc[5], a2) + (1 << 19)) >> 20, lo), hi);
                l2 = (int)min(max((mul64(mc[6], a0) + mul64(mc[7], a1) + mul64(mc[8], a2) + (1 << 19)) >> 20, lo), hi);
            }
            TO s0, s1, s2, sa;
            if constexpr (O == O_U8 || O == O_U16) {            /* LINEAR has no integer form */
                s0 = code_sample<O>(min(max(lut(Bt, l0), 0), 65535));
                s1 = code_sample<O>(min(max(lut(Bt, l1), 0), 65535));
                s2 = code_sample<O>(min(max(lut(Bt, l2), 0), 65535));
                sa = code_sample<O>(65535);
            } else if (by_table) {
                s0 = code_sample<O>(min(max(lut(Bt, l0), 0), 65535));
                s1 = code_sample<O>(min(max(lut(Bt, l1), 0), 65535));
                s2 = code_sample<O>(min(max(lut(Bt, l2), 0), 65535));
                sa = code_sample<O>(65535);
            } else {
                s0 = linear_sample<O>(l0, K); s1 = linear_sample<O>(l1, K); s2 = linear_sample<O>(l2, K);
                if constexpr (O == O_F32) sa = 1.0f; else sa = (TO)0x3C00;
            }
            if constexpr (LAY == L_RGBP) {
                o0[i] = s0; o1[i] = s1; o2[i] = s2;
            } else {
                TO *q = o0 + i * nc;
                q[0] = s0; q[1] = s1; q[2] = s2;
                if (nc == 4) q[3] = sa;
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
}

template <typename TI, int O, int LAY>
void launch(const OhColArgs *a, int n, hipStream_t st)
{
    const int cw = 2048 / (int)sizeof(typename OutT<O>::T);
    const dim3 grid((unsigned)((a->c.W + cw - 1) / cw), (unsigned)((a->c.H + OH_COL_ROWS - 1) / OH_COL_ROWS), (unsigned)n);
    colour_rgb_kernel<TI, O, LAY><<<grid, THREADS, 0, st>>>(*a);
}

template <int LAY>
void launch_rgb(const OhColArgs *a, int sample, int n, hipStream_t st)
{
    const bool wide = a->c.bd > 8;
    switch (sample) {
    case OH_CONV_U8:  wide ? launch<uint16_t, O_U8, LAY>(a, n, st)  : launch<uint8_t, O_U8, LAY>(a, n, st);  break;
    case OH_CONV_U16: wide ? launch<uint16_t, O_U16, LAY>(a, n, st) : launch<uint8_t, O_U16, LAY>(a, n, st); break;
    case OH_CONV_F16: wide ? launch<uint16_t, O_F16, LAY>(a, n, st) : launch<uint8_t, O_F16, LAY>(a, n, st); break;
    default:          wide ? launch<uint16_t, O_F32, LAY>(a, n, st) : launch<uint8_t, O_F32, LAY>(a, n, st); break;
    }
}

} // namespace

static_assert(OH_COLT_G >= OH_COL_NA && OH_COLT_B - OH_COLT_G >= OH_COL_NP && OH_COLT_N - OH_COLT_B >= OH_COL_NP && OH_COLT_N % 4 == 0,
              "the tables as whole 16-byte granules");

extern "C" void ohk_colour(const OhColArgs *a, int format, int sample, int n, hipStream_t st)
{
    if (format == OH_CONV_RGB_PLANAR)
        launch_rgb<L_RGBP>(a, sample, n, st);
    else
        launch_rgb<L_RGBI>(a, sample, n, st);
}
