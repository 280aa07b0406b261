/*
 * reformat.hip — finished pictures -> finished pictures of another bit depth and / or chroma format (oh_pics_reformat; the exact
 * definitions are in DESIGN.md §3j and tests/reformat_model.py).
 *
 * Memory-bound streaming over the CODED planes of the destinations, in the shape of import.hip's YUV kernel: one workgroup (256 lanes)
 * per segment of one unit of rows of one plane; grid (segments, units, pictures of the launch — all of them share one geometry; their
 * plane addresses are in the kernel arguments).  A unit is one destination row, or where chroma is up-sampled vertically the PAIR of
 * destination rows 2j, 2j + 1 that share source row j (the linear filter reads rows j - 1, j, j + 1 once for both).  A chroma row that
 * is sub-sampled vertically reads its two source rows.  Two phases, one barrier:
 *   1. stage   the one to three source rows of the segment, with the filter's one-sample halo left and right, go to LDS as whole
 *              16-byte granules (plane rows start 256-byte aligned and are padded, so a granule that holds a coded sample lies in its row);
 *   2. convert each lane takes one 16-byte granule of a destination row at a time: it adds the weighted source samples of each of its 8
 *              or 16 samples out of LDS, quantises every sum once (reformat_common.h) and stores the granule (global_store_dwordx4), up
 *              to the one that holds the last coded sample; the samples behind the coded width in that granule lie in the row's
 *              padding, which nothing reads.  Chroma that changes its width goes in runs of 8 samples, so that 8-bit rows (half a
 *              granule, global_store_dwordx2) keep every lane busy.  Where a sample takes the source sample of its own column (luma,
 *              chroma of an unchanged width), and in the 1-2-1 filter, the lane reads its source samples as whole granules of LDS
 *              (ds_read_b128); the other forms read sample by sample.  No LDS image of the destination, no second barrier.
 * The LDS of a launch is what its format pair stages (one row of a segment for a plain depth change, three half rows for 4:2:0 ->
 * 4:4:4), so that a CU holds as many workgroups — bytes in flight — as its waves allow.  Templates on the stored sample types of source
 * and destination; depth mode, filters and the format pair are uniform branches, the horizontal form one switch outside the loop.
 */
#include <algorithm>
#include "pics_common.h"
#include "reformat_common.h"

namespace {

enum { H_COPY, H_DOWN_POINT, H_DOWN_LIN, H_UP_NEAR, H_UP_LIN };     /* what a destination sample takes of one staged source row */

/* how the chroma planes of a format pair are made (both sides have chroma): the horizontal form, the staged source rows and destination
 * rows of a unit, the weights of the two source rows of a destination row (wb = 0: one row) and f, the log2 of the weights' total */
struct ChromaPlan { int hm, nin, nout, wa, wb, f; };
__host__ __device__ inline ChromaPlan chroma_plan(int scf, int dcf, int down, int up)
{
    const int shs = scf == 1 || scf == 2, svs = scf == 1, dhs = dcf == 1 || dcf == 2, dvs = dcf == 1;
    ChromaPlan p = { H_COPY, 1, 1, 1, 0, 0 };
    if (dhs > shs) { p.hm = down ? H_DOWN_LIN : H_DOWN_POINT; p.f = down ? 2 : 0; }
    else if (dhs < shs) { p.hm = up ? H_UP_LIN : H_UP_NEAR; p.f = up ? 1 : 0; }
    if (dvs > svs) {
        if (down) { p.nin = 2; p.wb = 1; p.f += 1; }
    } else if (dvs < svs) {
        p.nout = 2;
        if (up) { p.nin = 3; p.wa = 3; p.wb = 1; p.f += 2; }
    }
    return p;
}

/* bytes of one staged row in LDS: a segment of source samples and the halo, or half of it where chroma is up-sampled horizontally */
template <typename TI>
__host__ __device__ constexpr int slot_bytes(int hm)
{
    return (((hm == H_UP_NEAR || hm == H_UP_LIN ? OH_RF_SEG / 2 : OH_RF_SEG) + 2) * (int)sizeof(TI) + 32 + 15) / 16 * 16;
}

/* the horizontal sum at destination column X of a staged row whose sample 0 is source column lo; sw: the source plane's coded width */
template <int HM, typename TI>
__device__ __forceinline__ int hsum(const LDS TI *row, int X, int lo, int sw)
{
    if constexpr (HM == H_COPY) {
        return row[X - lo];
    } else if constexpr (HM == H_DOWN_POINT) {
        return row[2 * X - lo];
    } else if constexpr (HM == H_DOWN_LIN) {
        return row[max(2 * X - 1, 0) - lo] + 2 * row[2 * X - lo] + row[min(2 * X + 1, sw - 1) - lo];
    } else {
        const int k = X >> 1;
        if constexpr (HM == H_UP_NEAR)
            return row[k - lo];
        const int k2 = (X & 1) ? min(k + 1, sw - 1) : k;
        return row[k - lo] + row[k2 - lo];
    }
}

/* what a unit's rows share */
struct RowJob {
    int X0, cnt, dw, lo, sw;         /* destination columns [X0, X0 + cnt) of a plane dw wide; the staged source columns start at lo */
    int wa, wb;                      /* weights of the two source rows; wb = 0: one row */
    int s, mode, bd;                 /* the quantisation */
};

/* destination row Y of the unit, from the staged rows A and B, to dst, the address of its column X0 */
template <int HM, typename TI, typename TS>
__device__ __forceinline__ void convert_row(void *dst, const LDS TI *A, const LDS TI *B, const RowJob &j, int Y)
{
    /* what a lane takes at a time: a granule of 16 bytes, or where 8-bit samples are filtered across half of one, so that a segment
     * has work for every lane; IB: bytes of as many source samples */
    constexpr int GS = HM == H_COPY ? 16 / (int)sizeof(TS) : 8, IB = GS * (int)sizeof(TI);
    typedef uint32_t StoreT __attribute__((ext_vector_type(GS * (int)sizeof(TS) / 4)));
    for (int g = threadIdx.x; g < j.cnt / GS; g += THREADS) {
        const int Xg = j.X0 + g * GS;
        TS o[GS];
        if constexpr (HM == H_DOWN_LIN) {
            /* source columns 2 Xg .. 2 Xg + 15 of each row are whole granules (the staged rows keep the plane's alignment); the left
             * neighbour of the first is clamped at the plane's edge, and 2 x + 1 never reaches the right edge */
            typedef TI Cols __attribute__((ext_vector_type(16)));
            typedef Cols ColsA __attribute__((aligned(16)));
            const int at = 2 * Xg - j.lo, lf = max(2 * Xg - 1, 0) - j.lo;
            const Cols va = *(const LDS ColsA *)(A + at), vb = j.wb ? *(const LDS ColsA *)(B + at) : va;
            int la = A[lf], lb = j.wb ? B[lf] : 0;
#pragma unroll
            for (int k = 0; k < GS; k++) {
                int sum = j.wa * (la + 2 * va[2 * k] + va[2 * k + 1]);
                if (j.wb)
                    sum += j.wb * (lb + 2 * vb[2 * k] + vb[2 * k + 1]);
                la = va[2 * k + 1]; lb = vb[2 * k + 1];
                o[k] = (TS)reformat_quantise(sum, j.s, j.mode, Xg + k, Y, j.bd);
            }
        } else if constexpr (HM == H_COPY) {                    /* lo = X0: the lane's source samples are whole, aligned granules */
            TI a[GS], b[GS];
            typedef TI Granule __attribute__((ext_vector_type(GS)));            /* the staged rows start 16-byte aligned */
            typedef Granule GranuleA __attribute__((aligned(IB < 16 ? IB : 16)));
            const Granule va = *(const LDS GranuleA *)(A + g * GS), vb = j.wb ? *(const LDS GranuleA *)(B + g * GS) : va;
#pragma unroll
            for (int k = 0; k < GS; k++) { a[k] = va[k]; b[k] = vb[k]; }
#pragma unroll
            for (int k = 0; k < GS; k++) {
                int sum = j.wa * a[k];
                if (j.wb)
                    sum += j.wb * b[k];
                o[k] = (TS)reformat_quantise(sum, j.s, j.mode, Xg + k, Y, j.bd);
            }
        } else {
#pragma unroll
            for (int k = 0; k < GS; k++) {
                const int X = min(Xg + k, j.dw - 1);            /* behind the coded width: the rest of the last granule */
                int sum = j.wa * hsum<HM>(A, X, j.lo, j.sw);
                if (j.wb)
                    sum += j.wb * hsum<HM>(B, X, j.lo, j.sw);
                o[k] = (TS)reformat_quantise(sum, j.s, j.mode, X, Y, j.bd);
            }
        }
        StoreT v;
        __builtin_memcpy(&v, o, sizeof(v));
        *(GLOBAL StoreT *)((uintptr_t)dst + sizeof(v) * (uintptr_t)g) = v;
    }
}

template <typename TI, typename TS>
__global__ __launch_bounds__(THREADS) void reformat_kernel(const OhRfArgs a)
{
    constexpr int SEG = OH_RF_SEG, GS = 16 / (int)sizeof(TS);
    extern __shared__ __attribute__((aligned(16))) uint8_t in_l[];            /* the staged rows, slot_bytes each */
    const int pic = blockIdx.z, r = blockIdx.y;
    /* the unit: plane c (class q), destination rows Y .. Y + nout - 1, source rows rows[0 .. nin) */
    int c = 0, q = 0, Y = r;
    int rows[3] = { r, 0, 0 };
    bool mid = false;                                           /* chroma from a 4:0:0 source */
    ChromaPlan p = { H_COPY, 1, 1, 1, 0, 0 };
    if (r >= a.dh[0]) {
        q = 1;
        if (a.scf) {
            p = chroma_plan(a.scf, a.dcf, a.down, a.up);
        } else {
            mid = true; p.nin = 0;
        }
        const int units = a.dh[1] >> (p.nout - 1), rr = r - a.dh[0];
        c = rr < units ? 1 : 2;
        const int u = rr - (c - 1) * units;
        Y = u; rows[0] = u;
        if (p.nout == 2) {                                      /* up: destination rows 2u, 2u + 1 from source row u and its neighbours */
            Y = 2 * u;
            rows[1] = max(u - 1, 0); rows[2] = min(u + 1, a.sh[1] - 1);
        } else if (a.scf && a.dh[1] < a.sh[1]) {                /* down: destination row u from source rows 2u, 2u + 1 */
            rows[0] = 2 * u; rows[1] = 2 * u + 1;
        }
    }
    const int hm = p.hm;
    const int dseg = hm == H_DOWN_POINT || hm == H_DOWN_LIN ? SEG / 2 : SEG;
    RowJob j;
    j.wa = p.wa; j.wb = p.wb;
    j.dw = a.dw[q]; j.sw = a.sw[q];
    j.X0 = blockIdx.x * dseg;
    const int pw = (j.dw + GS - 1) & ~(GS - 1);                 /* with the rest of the last granule */
    if (j.X0 >= pw)
        return;
    j.cnt = min(dseg, pw - j.X0);
    const int Xl = min(j.X0 + j.cnt - 1, j.dw - 1);
    int hi;
    switch (hm) {
    case H_COPY:       j.lo = j.X0; hi = j.X0 + j.cnt - 1; break;                 /* whole granules: the last may end in the source row's padding */
    case H_DOWN_POINT: j.lo = 2 * j.X0; hi = 2 * Xl; break;
    case H_DOWN_LIN:   j.lo = max(2 * j.X0 - 1, 0); hi = 2 * (j.X0 + j.cnt) - 1; break;          /* whole granules, as for H_COPY */
    default:           j.lo = j.X0 >> 1; hi = min((Xl + 1) >> 1, j.sw - 1); break;
    }
    const int slot = slot_bytes<TI>(hm);
    int at[3] = { 0, 0, 0 };                                    /* where each staged row starts in in_l, bytes */
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (k < p.nin)
            at[k] = k * slot + (int)sizeof(TI) *
                    stage<TI>(in_l + k * slot, (const uint8_t *)a.src[pic][c] + (size_t)rows[k] * a.spitch[c] + (size_t)j.lo * sizeof(TI), hi - j.lo + 1);
    __syncthreads();
    j.s = p.f + a.sbd - a.dbd; j.mode = a.depth; j.bd = a.dbd;
#pragma unroll
    for (int o = 0; o < 2; o++) {
        if (o >= p.nout)
            break;
        void *dst = (uint8_t *)a.dst[pic][c] + (size_t)(Y + o) * a.dpitch[c] + (size_t)j.X0 * sizeof(TS);
        const LDS TI *A = (const LDS TI *)((const LDS uint8_t *)in_l + at[0]), *B = (const LDS TI *)((const LDS uint8_t *)in_l + at[1 + o]);
        if (mid) {
            uint4v v;
            for (int k = 0; k < 4; k++)
                v[k] = (uint32_t)(1 << (a.dbd - 1)) * (sizeof(TS) == 1 ? 0x01010101u : 0x00010001u);
            for (int g = threadIdx.x; g < j.cnt / GS; g += THREADS)
                *(GLOBAL uint4v *)((uintptr_t)dst + 16 * (uintptr_t)g) = v;
            continue;
        }
        switch (hm) {
        case H_COPY:       convert_row<H_COPY, TI, TS>(dst, A, B, j, Y + o); break;
        case H_DOWN_POINT: convert_row<H_DOWN_POINT, TI, TS>(dst, A, B, j, Y + o); break;
        case H_DOWN_LIN:   convert_row<H_DOWN_LIN, TI, TS>(dst, A, B, j, Y + o); break;
        case H_UP_NEAR:    convert_row<H_UP_NEAR, TI, TS>(dst, A, B, j, Y + o); break;
        default:           convert_row<H_UP_LIN, TI, TS>(dst, A, B, j, Y + o); break;
        }
    }
}

template <typename TI, typename TS>
void launch(const OhRfArgs *a, int n, hipStream_t st)
{
    ChromaPlan p = { H_COPY, 0, 1, 1, 0, 0 };                   /* no chroma staged: a 4:0:0 side */
    if (a->scf && a->dcf)
        p = chroma_plan(a->scf, a->dcf, a->down, a->up);
    const int cseg = p.hm == H_DOWN_POINT || p.hm == H_DOWN_LIN ? OH_RF_SEG / 2 : OH_RF_SEG;
    const int segs = std::max((a->dw[0] + OH_RF_SEG - 1) / OH_RF_SEG, a->dcf ? (a->dw[1] + cseg - 1) / cseg : 0);
    const int units = a->dh[0] + (a->dcf ? 2 * (a->dh[1] >> (p.nout - 1)) : 0);
    const int lds = std::max(slot_bytes<TI>(H_COPY), p.nin * slot_bytes<TI>(p.hm));      /* the luma row, or the chroma rows */
    const dim3 grid((unsigned)segs, (unsigned)units, (unsigned)n);
    reformat_kernel<TI, TS><<<grid, THREADS, (size_t)lds, st>>>(*a);
}

} // namespace

static_assert(OH_RF_SEG % 32 == 0, "half a segment is whole 16-byte granules of either sample type");

extern "C" void ohk_reformat(const OhRfArgs *a, int n, hipStream_t st)
{
    with_sample_types(a->sbd, a->dbd, [&](auto ti, auto ts) { launch<decltype(ti), decltype(ts)>(a, n, st); });
}
