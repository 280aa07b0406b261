/*
 * import.hip — standard images in caller-owned device memory -> finished pictures (oh_pics_import, the inverse of convert.hip; the
 * exact definitions are in DESIGN.md §3g and tests/import_model.py).
 *
 * Memory-bound streaming over CODED plane coordinates: a plane sample at (X, Y) is the window sample at the clamped position, so the
 * replicated margins around the window are written by the same pass, and every plane byte is written once.  Every image byte is read
 * once from HBM, apart from the filter's one-column halo at segment boundaries and the edge rows and columns the margins repeat.  One
 * workgroup (256 lanes) per segment of up to CW plane columns of one unit of rows; grid (segments, units, pictures of the launch — all
 * of them share one geometry; their plane addresses are in the kernel arguments).  Three phases, two barriers:
 *   1. stage   the image row(s) of the segment go to LDS as whole 16-byte granules (global_load_dwordx4).  Packed images start at any
 *              byte; an aligned granule that holds one byte of the image lies in the image's page, so the up to 15 bytes in front of
 *              and behind a row are read and never used.
 *   2. compute each lane converts samples out of LDS and writes the stored samples into an LDS image of the plane rows;
 *   3. store   plane rows are padded to 256 bytes and start 256-byte aligned, so a row is stored as whole 16-byte granules
 *              (global_store_dwordx4) up to the granule that holds its last sample; the samples behind the coded width in that granule
 *              lie in the row's padding, which nothing reads.
 * A unit of rows is one plane row, or for RGB into 4:2:0 the pair of image rows that gives two luma rows and one chroma row from one
 * reading of the pixels.  Templates on what changes the inner loop (input sample type, layout, stored sample type); the chroma format,
 * filter and channel count are uniform branches.
 */
#include <algorithm>
#include "convert_common.h"

namespace {

/* whole 16-byte granules from an LDS image to a 16-byte aligned plane address */
__device__ __forceinline__ void store_granules(void *dst, const uint8_t *img, int nbytes)
{
    for (int i = threadIdx.x; i < (nbytes >> 4); i += THREADS)
        *(GLOBAL uint4v *)((uintptr_t)dst + 16 * (uintptr_t)i) = *(const uint4v *)(img + 16 * i);
}

/* YUV images.  Unit r: a coded row of the Y plane, then of Cb and Cr (planar), or of Cb and Cr together from one interleaved CbCr row
 * (semi-planar).  TI -> TS: u8 -> u8 (copy), u16 -> u16 (planar: clamped to the bit depth, semi-planar: shifted down from the MSB),
 * u8 -> u16 (shifted up). */
template <typename TI, typename TS, int LAY>
__global__ __launch_bounds__(THREADS) void import_yuv_kernel(const OhImpArgs a)
{
    constexpr int CW = 4096, GS = 16 / (int)sizeof(TS);         /* image samples per segment: an interleaved CbCr segment gives CW / 2 of each */
    __shared__ __attribute__((aligned(16))) uint8_t in_l[CW * sizeof(TI) + 32];
    __shared__ __attribute__((aligned(16))) uint8_t out_l[CW * sizeof(TS)];
    const int pic = blockIdx.z, r = blockIdx.y;
    const int W = a.W, H = a.H, hs = a.cf == 1 || a.cf == 2, vs = a.cf == 1, Wc = W >> hs, Hc = H >> vs;
    int c, Y;
    if (r < a.ph[0]) {
        c = 0; Y = r;
    } else if (LAY == L_PLANAR) {
        const int rr = r - a.ph[0];
        c = rr < a.ph[1] ? 1 : 2; Y = rr - (c - 1) * a.ph[1];
    } else {
        c = 1; Y = r - a.ph[0];
    }
    const bool inter = LAY == L_SEMI && c;
    const int seg = inter ? CW / 2 : CW, X0 = blockIdx.x * seg;
    const int pw = (a.pw[c ? 1 : 0] + GS - 1) & ~(GS - 1);       /* with the rest of the last granule */
    if (X0 >= pw)
        return;
    const int cnt = min(seg, pw - X0);
    const int x0 = c ? a.left >> hs : a.left, y0 = c ? a.top >> vs : a.top, w = c ? Wc : W, h = c ? Hc : H;
    const int wy = min(max(Y - y0, 0), h - 1), lo = min(max(X0 - x0, 0), w - 1), hi = min(max(X0 + cnt - 1 - x0, 0), w - 1);
    size_t off;                                                 /* samples from the image start to the first one staged */
    if (!c)
        off = (size_t)wy * W + lo;
    else if (LAY == L_PLANAR)
        off = (size_t)W * H + (size_t)(c - 1) * Wc * Hc + (size_t)wy * Wc + lo;
    else
        off = (size_t)W * H + ((size_t)wy * Wc + lo) * 2;
    const uint8_t *img = (const uint8_t *)a.src + pic * a.image_stride;
    const int b0 = stage<TI>(in_l, img + off * sizeof(TI), (hi - lo + 1) << (inter ? 1 : 0));
    __syncthreads();
    const TI *s = (const TI *)in_l + b0;
    TS *o0 = (TS *)out_l, *o1 = o0 + CW / 2;
    const int bd = a.bd, mx = (1 << bd) - 1;
    auto cvt = [&](int v) -> TS {
        if constexpr (sizeof(TI) == sizeof(TS))
            return (TS)(sizeof(TS) == 1 ? v : LAY == L_SEMI ? v >> (16 - bd) : min(v, mx));
        else
            return (TS)(v << (bd - 8));
    };
    for (int i = threadIdx.x; i < cnt; i += THREADS) {
        const int k = min(max(X0 + i - x0, 0), w - 1) - lo;
        if (inter) {
            o0[i] = cvt(s[2 * k]); o1[i] = cvt(s[2 * k + 1]);
        } else {
            o0[i] = cvt(s[k]);
        }
    }
    __syncthreads();
    const size_t to = (size_t)Y * a.pitch[c] + (size_t)X0 * sizeof(TS);
    store_granules((uint8_t *)a.dst[pic][c] + to, out_l, cnt * (int)sizeof(TS));
    if (inter)
        store_granules((uint8_t *)a.dst[pic][2] + to, out_l + CW / 2 * sizeof(TS), cnt * (int)sizeof(TS));
}

/* an RGB sample -> its integer of D bits: u8 and u16 as they are; f32 one multiplication rounded to nearest even, then
 * the clamp (NaN gives 0) and rint; f16 through its exact f32 */
template <int I>
__device__ __forceinline__ int in_sample(typename OutT<I>::T v)
{
    if constexpr (I == O_F32 || I == O_F16) {
        float f;
        if constexpr (I == O_F16)
            f = (float)__builtin_bit_cast(_Float16, v);
        else
            f = v;
        return (int)rintf(fminf(fmaxf(__fmul_rn(f, 65535.0f), 0.0f), 65535.0f));
    } else {
        return (int)v;
    }
}

/* one staged image row of a segment: channel c of pixel x (counted from the first staged column) is c[x * nc] */
template <int I>
struct RgbRow {
    typedef typename OutT<I>::T TI;
    const TI *r, *g, *b;
    __device__ __forceinline__ void load(int x, int &R, int &G, int &B) const
    {
        R = in_sample<I>(r[x]); G = in_sample<I>(g[x]); B = in_sample<I>(b[x]);
    }
};

/* the forward matrix with the coefficients of oh_import_coeffs */
struct YuvMatrix {
    int ry, gy, by, ru, gu, bu, rv, gv, bv, yo, co, S, mx;
    __device__ __forceinline__ YuvMatrix(const int32_t *k, int bd)
        : ry(k[0]), gy(k[1]), by(k[2]), ru(k[3]), gu(k[4]), bu(k[5]), rv(k[6]), gv(k[7]), bv(k[8]),
          yo((k[9] << k[11]) + (1 << (k[11] - 1))), co((k[10] << k[11]) + (1 << (k[11] - 1))), S(k[11]), mx((1 << bd) - 1) {}
    __device__ __forceinline__ int luma(int R, int G, int B) const { return min(max((ry * R + gy * G + by * B + yo) >> S, 0), mx); }
    __device__ __forceinline__ int cb(int R, int G, int B) const { return min(max((ru * R + gu * G + bu * B + co) >> S, 0), mx); }
    __device__ __forceinline__ int cr(int R, int G, int B) const { return min(max((rv * R + gv * G + bv * B + co) >> S, 0), mx); }
};

/* RGB images.  Unit j: coded chroma row j with the luma rows it covers (4:2:0: two, from the pair of image rows the chroma row
 * filters), or coded luma row j where chroma is not sub-sampled vertically.  I: input sample type, TS: stored sample type. */
template <int I, typename TS, int LAY>
__global__ __launch_bounds__(THREADS) void import_rgb_kernel(const OhImpArgs a)
{
    typedef typename OutT<I>::T TI;
    constexpr int CW = 2048 / (int)sizeof(TI), GS = 16 / (int)sizeof(TS);
    constexpr int NR = LAY == L_RGBP ? 3 : 1;                                       /* staged spans per image row */
    constexpr int RB = ((CW + 4) * (LAY == L_RGBP ? 1 : 4) * (int)sizeof(TI) + 32 + 15) / 16 * 16;
    __shared__ __attribute__((aligned(16))) uint8_t in_l[2][NR][RB];
    __shared__ __attribute__((aligned(16))) uint8_t out_y[2][CW * sizeof(TS)];
    __shared__ __attribute__((aligned(16))) uint8_t out_c[2][CW * sizeof(TS)];
    const int pic = blockIdx.z, j = blockIdx.y, X0 = blockIdx.x * CW;
    const int W = a.W, H = a.H, cf = a.cf, hs = cf == 1 || cf == 2, vs = cf == 1, Wc = W >> hs, Hc = H >> vs;
    const int pw = ((a.pw[hs] + GS - 1) & ~(GS - 1)) << hs;      /* luma columns, with the rest of the last (chroma) granule */
    if (X0 >= pw)
        return;
    const int cnt = min(CW, pw - X0), nrows = 1 + vs;
    /* the image rows of the unit, and which of them each luma row of the unit takes */
    const int jw = j - (a.top >> vs), yc = min(max(jw, 0), Hc - 1), r0 = yc << vs;
    const int k0 = vs && jw > Hc - 1 ? 1 : 0, k1 = vs && jw >= 0 ? 1 : 0;
    /* the image columns: those of the luma samples and, sub-sampled, the three the filter reads around each chroma sample */
    const int left = a.left;
    int lo = min(max(X0 - left, 0), W - 1), hi = min(max(X0 + cnt - 1 - left, 0), W - 1);
    if (hs) {
        const int c_lo = min(max((X0 - left) >> 1, 0), Wc - 1), c_hi = min(max((X0 + cnt - 1 - left) >> 1, 0), Wc - 1);
        lo = min(lo, max(2 * c_lo - 1, 0)); hi = max(hi, min(2 * c_hi + 1, W - 1));
    }
    const int nc = LAY == L_RGBP ? 1 : a.nc, m = hi - lo + 1;
    const uint8_t *img = (const uint8_t *)a.src + pic * a.image_stride;
    RgbRow<I> row[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (k && !vs) {
            row[1] = row[0];
            break;
        }
        const size_t at = (size_t)(r0 + k) * W + lo;
        if constexpr (LAY == L_RGBP) {
            row[k].r = (const TI *)in_l[k][0] + stage<TI>(in_l[k][0], img + at * sizeof(TI), m);
            row[k].g = (const TI *)in_l[k][1] + stage<TI>(in_l[k][1], img + ((size_t)W * H + at) * sizeof(TI), m);
            row[k].b = (const TI *)in_l[k][2] + stage<TI>(in_l[k][2], img + (2 * (size_t)W * H + at) * sizeof(TI), m);
        } else {
            row[k].r = (const TI *)in_l[k][0] + stage<TI>(in_l[k][0], img + at * nc * sizeof(TI), m * nc);
            row[k].g = row[k].r + 1; row[k].b = row[k].r + 2;
        }
    }
    const RgbRow<I> ca = row[0], cb = row[1];                    /* the rows the chroma filter adds */
    const RgbRow<I> la = k0 ? cb : ca, lb = k1 ? cb : ca;        /* the rows of the unit's luma rows */
    __syncthreads();
    const YuvMatrix mt(a.k, a.bd);
    TS *y0 = (TS *)out_y[0], *y1 = (TS *)out_y[1], *ub = (TS *)out_c[0], *vb = (TS *)out_c[1];
    const int units = cnt >> hs, filter = a.filter;
    for (int i = threadIdx.x; i < units; i += THREADS) {
        const int X = X0 + (i << hs);
        int R, G, B;
        for (int dx = 0; dx <= hs; dx++) {
            const int x = min(max(X + dx - left, 0), W - 1) - lo;
            la.load(x * nc, R, G, B);
            y0[(i << hs) + dx] = (TS)mt.luma(R, G, B);
            if (vs) {
                lb.load(x * nc, R, G, B);
                y1[(i << hs) + dx] = (TS)mt.luma(R, G, B);
            }
        }
        if (!cf)
            continue;
        if (hs) {                                               /* cf == 3: the pixel itself, still in R, G, B */
            const int xc = min(max((X - left) >> 1, 0), Wc - 1), xm = (2 * xc - lo) * nc;
            if (!filter) {
                ca.load(xm, R, G, B);
            } else {
                const int xl = (max(2 * xc - 1, 0) - lo) * nc, xr = (min(2 * xc + 1, W - 1) - lo) * nc;
                int r1, g1, b1, r2, g2, b2;
                ca.load(xl, r1, g1, b1); ca.load(xm, R, G, B); ca.load(xr, r2, g2, b2);
                R = 2 * R + r1 + r2; G = 2 * G + g1 + g2; B = 2 * B + b1 + b2;
                if (vs) {
                    int r3, g3, b3;
                    cb.load(xl, r1, g1, b1); cb.load(xm, r3, g3, b3); cb.load(xr, r2, g2, b2);
                    R = (R + 2 * r3 + r1 + r2 + 4) >> 3; G = (G + 2 * g3 + g1 + g2 + 4) >> 3; B = (B + 2 * b3 + b1 + b2 + 4) >> 3;
                } else {
                    R = (R + 2) >> 2; G = (G + 2) >> 2; B = (B + 2) >> 2;
                }
            }
        }
        ub[i] = (TS)mt.cb(R, G, B); vb[i] = (TS)mt.cr(R, G, B);
    }
    __syncthreads();
    for (int k = 0; k < nrows; k++)
        store_granules((uint8_t *)a.dst[pic][0] + (size_t)((j << vs) + k) * a.pitch[0] + (size_t)X0 * sizeof(TS), out_y[k], cnt * (int)sizeof(TS));
    if (cf)
        for (int c = 1; c < 3; c++)
            store_granules((uint8_t *)a.dst[pic][c] + (size_t)j * a.pitch[c] + (size_t)(X0 >> hs) * sizeof(TS), out_c[c - 1],
                           units * (int)sizeof(TS));
}

template <typename TI, typename TS, int LAY>
void launch_yuv(const OhImpArgs *a, int n, hipStream_t st)
{
    const int rows = a->ph[0] + (a->cf ? (LAY == L_PLANAR ? 2 : 1) * a->ph[1] : 0);
    /* the longest row in image samples: an interleaved CbCr row holds 2 * pw[1], twice the luma row's in 4:4:4 (NV24 / P410) */
    const int longest = std::max(a->pw[0], (LAY == L_SEMI ? 2 : 1) * a->pw[1]);
    const dim3 grid((unsigned)((longest + 4095) / 4096), (unsigned)rows, (unsigned)n);
    import_yuv_kernel<TI, TS, LAY><<<grid, THREADS, 0, st>>>(*a);
}

template <int LAY>
void launch_yuv(const OhImpArgs *a, int sample, int n, hipStream_t st)
{
    if (a->bd == 8)
        launch_yuv<uint8_t, uint8_t, LAY>(a, n, st);
    else if (sample == OH_CONV_U8)
        launch_yuv<uint8_t, uint16_t, LAY>(a, n, st);
    else
        launch_yuv<uint16_t, uint16_t, LAY>(a, n, st);
}

template <int I, int LAY>
void launch_rgb(const OhImpArgs *a, int n, hipStream_t st)
{
    const int vs = a->cf == 1, cw = 2048 / (int)sizeof(typename OutT<I>::T);
    const dim3 grid((unsigned)((a->pw[0] + cw - 1) / cw), (unsigned)(a->ph[0] >> vs), (unsigned)n);
    if (a->bd == 8)
        import_rgb_kernel<I, uint8_t, LAY><<<grid, THREADS, 0, st>>>(*a);
    else
        import_rgb_kernel<I, uint16_t, LAY><<<grid, THREADS, 0, st>>>(*a);
}

template <int LAY>
void launch_rgb(const OhImpArgs *a, int sample, int n, hipStream_t st)
{
    switch (sample) {
    case OH_CONV_U8:  launch_rgb<O_U8, LAY>(a, n, st);  break;
    case OH_CONV_U16: launch_rgb<O_U16, LAY>(a, n, st); break;
    case OH_CONV_F16: launch_rgb<O_F16, LAY>(a, n, st); break;
    default:          launch_rgb<O_F32, LAY>(a, n, st); break;
    }
}

} // namespace


extern "C" void ohk_import(const OhImpArgs *a, int format, int sample, int n, hipStream_t st)
{
    switch (format) {
    case OH_CONV_PLANAR:     launch_yuv<L_PLANAR>(a, sample, n, st); break;
    case OH_CONV_SEMIPLANAR: launch_yuv<L_SEMI>(a, sample, n, st); break;
    case OH_CONV_RGB_PLANAR: launch_rgb<L_RGBP>(a, sample, n, st); break;
    default:                 launch_rgb<L_RGBI>(a, sample, n, st); break;
    }
}
