/*
 * packing.hip — frame-packed stereo pictures -> the two views, and back (oh_pics_unpack, oh_pics_pack; the exact definition is in
 * DESIGN.md §3s and tests/packing_model.py, the sample formulas in packing_common.h, shared with the host).  Memory-bound passes in
 * the shape of orient.hip's row kernel: one workgroup (256 lanes) per segment of OH_PK_SEG_BYTES of one destination row, both global
 * sides as whole aligned 16-byte granules (plane rows start 256-byte aligned and are padded, so a granule that holds a coded sample
 * lies in its row).
 *   1. stage    the source samples that the segment reads go to LDS as the aligned granules that cover them (pics_common.h: stage),
 *               one LDS row per source row: one row for a copy and for the side-by-side up-sampler (half a segment plus the halo of
 *               the taps), three or two for the quincunx interpolation; packing stages the row (two under top-bottom quincunx) of
 *               each view that the segment reads.  The seam between the halves falls anywhere in a granule: the staged granules
 *               start wherever the half starts, and the lanes index LDS by sample.
 *   2. assemble each lane makes one aligned destination granule from LDS.  The copies, the quincunx forms and packing go sample by
 *               sample through packing_common.h — flips, the replicated last column and row and the lattice are index arithmetic
 *               there.  The side-by-side up-sampler (upsample_across) gathers the GS / 2 + TAPS samples of C_v that the granule reads
 *               once, clamped to the view's own samples, and applies the two phases of the granule's even and odd outputs, whose taps
 *               are the workgroup's.
 * The top-bottom up-sampler (upsample_down) stages nothing: phase and taps are those of the row, a lane reads its granule from each of
 * the eight (chroma: four) source rows with plain aligned loads, which neighbouring rows share through the caches, and sums them.
 * Both views of a packed picture are made in the same launch: grid (segments, rows of all planes, pictures x views).
 */
#include <algorithm>
#include "pics_common.h"
#include "packing_common.h"

namespace {

constexpr int PK_ROW = OH_PK_SEG_BYTES + 64;                    /* bytes of an LDS row of the unpacking kernel: a segment, the halo, the granule rests */
constexpr int PK_ROWS = 3;                                      /* its most rows: the quincunx interpolation side by side */
constexpr int PKP_ROW = 2 * OH_PK_SEG_BYTES + 64;               /* of the packing kernel: the lattice of a quincunx view is twice as wide */

/* The up-sampler down the picture (top-bottom, full size, no quincunx): position and phase are those of the row, so the taps are the
 * workgroup's; a lane reads its granule from each of the TAPS source rows with plain aligned loads (R_v starts at column 0) and sums
 * them.  A granule that reaches behind the coded width reads and writes row padding. */
template <typename T, int TAPS>
__device__ __forceinline__ void upsample_down(const PkPlane &pl, int flip, int g, int Y, uintptr_t rv, int pitch, uintptr_t dst, int cnt)
{
    constexpr int GS = 16 / (int)sizeof(T);
    const int p = pk_pos(pl.pos, Y, g), i = (p >> 4) - (TAPS == 8 ? 3 : 1), ph = p & 15;
    int coef[TAPS];
    uintptr_t row[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; t++) {
        const int j = pk_clamp(i + t, 0, pl.ch - 1);            /* the view's own rows */
        coef[t] = pk_tap(TAPS, ph, t);
        row[t] = rv + (size_t)(flip ? pl.ch - 1 - j : j) * pitch;
    }
    for (int gi = threadIdx.x; gi < cnt / GS; gi += THREADS) {
        int acc[GS];
#pragma unroll
        for (int k = 0; k < GS; k++)
            acc[k] = 32;
#pragma unroll
        for (int t = 0; t < TAPS; t++) {
            const Samples<T> s(*(const GLOBAL uint4v *)(row[t] + 16 * (uintptr_t)gi));
#pragma unroll
            for (int k = 0; k < GS; k++)
                acc[k] += coef[t] * (int)s.s[k];
        }
        Samples<T> o;
#pragma unroll
        for (int k = 0; k < GS; k++)
            o.s[k] = (T)pk_clamp(acc[k] >> 6, 0, pl.maxv);
        *(GLOBAL uint4v *)(dst + 16 * (uintptr_t)gi) = o.granule();
    }
}

/* The up-sampler across the picture (side by side, full size, no quincunx), from the staged row `in_s`, whose element at0 + rx is the
 * stored sample rx of R_v.  The position of output X is p = 8 X + c0 with c0 = pk_pos(kind, 0, g) for both kinds of horizontal
 * position, and a granule starts at a multiple of 8, so its even outputs share the phase c0 & 15 and its odd ones that plus 8, and
 * output k reads from C_v index i0 + (k >> 1) (+ 1 for an odd k where the phase wrapped) on: a lane gathers the samples of C_v that the even
 * and the odd outputs of its granule read, GS / 2 + TAPS - 1 each, clamped to [lo, hi], the part of 0 .. cw - 1 that the segment reads. */
template <typename T, int TAPS>
__device__ __forceinline__ void upsample_across(const PkPlane &pl, int flip, int g, const T *in_s, int at0, int lo, int hi, int X0, uintptr_t dst, int cnt)
{
    constexpr int GS = 16 / (int)sizeof(T), NW = GS / 2 + TAPS;
    const int c0 = pk_pos(pl.pos, 0, g), r = c0 & 15, wrapped = r >> 3;
    int ce[TAPS], co[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; t++) {
        ce[t] = pk_tap(TAPS, r, t);
        co[t] = pk_tap(TAPS, (r + 8) & 15, t);
    }
    for (int gi = threadIdx.x; gi < cnt / GS; gi += THREADS) {
        const int i0 = ((8 * (X0 + gi * GS) + c0) >> 4) - (TAPS == 8 ? 3 : 1);
        int w[NW], wo[NW - 1];
#pragma unroll
        for (int m = 0; m < NW; m++) {
            const int j = pk_clamp(i0 + m, lo, hi);
            w[m] = in_s[at0 + (flip ? pl.cw - 1 - j : j)];
        }
#pragma unroll
        for (int m = 0; m < NW - 1; m++) {                      /* gathered again: a select between w[m] and w[m + 1] becomes an array in scratch */
            const int j = pk_clamp(i0 + wrapped + m, lo, hi);
            wo[m] = in_s[at0 + (flip ? pl.cw - 1 - j : j)];
        }
        Samples<T> o;
#pragma unroll
        for (int k = 0; k < GS; k++) {
            int s = 32;
#pragma unroll
            for (int t = 0; t < TAPS; t++)
                s += (k & 1) ? co[t] * wo[(k >> 1) + t] : ce[t] * w[(k >> 1) + t];
            o.s[k] = (T)pk_clamp(s >> 6, 0, pl.maxv);
        }
        *(GLOBAL uint4v *)(dst + 16 * (uintptr_t)gi) = o.granule();
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void unpack_kernel(const OhPkArgs a)
{
    constexpr int SZ = (int)sizeof(T), GS = 16 / SZ, SEG = OH_PK_SEG_BYTES / SZ;
    extern __shared__ __attribute__((aligned(16))) uint8_t in_l[];
    const int pic = a.views == 3 ? blockIdx.z >> 1 : blockIdx.z, v = a.views == 3 ? blockIdx.z & 1 : a.views >> 1;
    int c, q;
    const int Y = grid_row(blockIdx.y, a.dh, c, q);
    const PkPlane &pl = a.pl[q];
    const int pw = (a.dw[q] + GS - 1) & ~(GS - 1);              /* with the rest of the last granule */
    const int X0 = blockIdx.x * SEG;
    if (X0 >= pw)
        return;
    const int cnt = min(SEG, pw - X0), flip = a.flip[v], g = a.g[v];
    const int ox = pl.sbs ? v * pl.cw : 0, oy = pl.sbs ? 0 : v * pl.ch;        /* R_v in the packed plane */
    const uintptr_t dst = (uintptr_t)a.view[v][pic][c] + (size_t)Y * a.vpitch[c] + (size_t)X0 * SZ;
    const bool filtered = pl.full && !pl.quincunx;
    if (filtered && !pl.sbs) {                                  /* plain loads, nothing staged */
        const uintptr_t rv = (uintptr_t)a.packed[pic][c] + (size_t)oy * a.ppitch[c] + (size_t)X0 * SZ;
        if (pl.taps == 8) upsample_down<T, 8>(pl, flip, g, Y, rv, a.ppitch[c], dst, cnt);
        else              upsample_down<T, 4>(pl, flip, g, Y, rv, a.ppitch[c], dst, cnt);
        return;
    }
    int ry[2], rx[2];
    pk_unpack_box(pl, flip, g, X0, X0 + cnt - 1, Y, ry, rx);
    int base = 0;
    for (int r = ry[0]; r <= ry[1]; r++)
        base = stage<T>(in_l + (r - ry[0]) * PK_ROW, (const uint8_t *)a.packed[pic][c] + (size_t)(oy + r) * a.ppitch[c] + (size_t)(ox + rx[0]) * SZ,
                        rx[1] - rx[0] + 1);
    __syncthreads();
    const T *in_s = (const T *)in_l;
    const int at0 = base - rx[0] - ry[0] * (PK_ROW / SZ);
    if (filtered) {                                             /* one staged row: ry[0] = ry[1] = Y */
        const int lo = flip ? pl.cw - 1 - rx[1] : rx[0], hi = flip ? pl.cw - 1 - rx[0] : rx[1];       /* the box in C_v */
        if (pl.taps == 8) upsample_across<T, 8>(pl, flip, g, in_s, at0 + Y * (PK_ROW / SZ), lo, hi, X0, dst, cnt);
        else              upsample_across<T, 4>(pl, flip, g, in_s, at0 + Y * (PK_ROW / SZ), lo, hi, X0, dst, cnt);
        return;
    }
    auto at = [&](int y, int x) -> int { return in_s[at0 + y * (PK_ROW / SZ) + x]; };
    for (int gi = threadIdx.x; gi < cnt / GS; gi += THREADS) {
        Samples<T> o;
#pragma unroll
        for (int k = 0; k < GS; k++)
            o.s[k] = (T)pk_unpack_sample(pl, v, flip, g, X0 + gi * GS + k, Y, at);
        *(GLOBAL uint4v *)(dst + 16 * (uintptr_t)gi) = o.granule();
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void pack_kernel(const OhPkArgs a)
{
    constexpr int SZ = (int)sizeof(T), GS = 16 / SZ, SEG = OH_PK_SEG_BYTES / SZ;
    extern __shared__ __attribute__((aligned(16))) uint8_t in_l[];             /* [view][row 0 .. 1] of PKP_ROW bytes */
    const int pic = blockIdx.z;
    int c, q;
    const int Y = grid_row(blockIdx.y, a.dh, c, q);
    const PkPlane &pl = a.pl[q];
    const int pw = (a.dw[q] + GS - 1) & ~(GS - 1);
    const int X0 = blockIdx.x * SEG;
    if (X0 >= pw)
        return;
    const int cnt = min(SEG, pw - X0);
    int at0[2] = { 0, 0 };
#pragma unroll
    for (int v = 0; v < 2; v++) {
        int sy[2], sx[2];
        if (!pk_pack_box(pl, a.flip, v, X0, X0 + cnt - 1, Y, sy, sx))
            continue;
        int base = 0;
        for (int r = sy[0]; r <= sy[1]; r++)
            base = stage<T>(in_l + (2 * v + r - sy[0]) * PKP_ROW, (const uint8_t *)a.view[v][pic][c] + (size_t)r * a.vpitch[c] + (size_t)sx[0] * SZ,
                            sx[1] - sx[0] + 1);
        at0[v] = base - sx[0] + (2 * v - sy[0]) * (PKP_ROW / SZ);
    }
    __syncthreads();
    const T *in_s = (const T *)in_l;
    auto at = [&](int v, int y, int x) -> int { return in_s[at0[v] + y * (PKP_ROW / SZ) + x]; };
    const uintptr_t dst = (uintptr_t)a.packed[pic][c] + (size_t)Y * a.ppitch[c] + (size_t)X0 * SZ;
    for (int gi = threadIdx.x; gi < cnt / GS; gi += THREADS) {
        Samples<T> o;
#pragma unroll
        for (int k = 0; k < GS; k++)
            o.s[k] = (T)pk_pack_sample(pl, a.flip, X0 + gi * GS + k, Y, at);
        *(GLOBAL uint4v *)(dst + 16 * (uintptr_t)gi) = o.granule();
    }
}

template <typename T>
dim3 grid_of(const OhPkArgs *a, int n)
{
    const int G = 16 / (int)sizeof(T), SEG = OH_PK_SEG_BYTES / (int)sizeof(T), cls = a->np > 1 ? 2 : 1;
    int pw = 0;
    for (int q = 0; q < cls; q++)
        pw = std::max(pw, (a->dw[q] + G - 1) / G * G);
    return dim3((unsigned)((pw + SEG - 1) / SEG), (unsigned)(a->dh[0] + (cls > 1 ? 2 * a->dh[1] : 0)), (unsigned)n);
}

/* the LDS rows that a row of the unpacked view reads */
int unpack_rows(const OhPkArgs *a)
{
    const PkPlane &pl = a->pl[0];
    return !pl.full ? 1 : pl.quincunx ? (pl.sbs ? PK_ROWS : 2) : pl.sbs ? 1 : 0;   /* upsample_down stages nothing */
}

} // namespace

static_assert(sizeof(OhPkArgs) <= 4096, "kernel arguments");
static_assert(OH_PK_SEG_BYTES == 16 * THREADS, "a granule per lane");
static_assert(PK_ROWS * PK_ROW <= 64 * 1024 && 4 * PKP_ROW <= 64 * 1024, "the staged rows fit the LDS of a workgroup");

extern "C" void ohk_unpack(const OhPkArgs *a, int n, hipStream_t st)
{
    const int nv = a->views == 3 ? 2 : 1;
    const size_t lds = (size_t)unpack_rows(a) * PK_ROW;
    if (a->bd == 8) unpack_kernel<uint8_t><<<grid_of<uint8_t>(a, n * nv), THREADS, lds, st>>>(*a);
    else            unpack_kernel<uint16_t><<<grid_of<uint16_t>(a, n * nv), THREADS, lds, st>>>(*a);
}

extern "C" void ohk_pack(const OhPkArgs *a, int n, hipStream_t st)
{
    const size_t lds = (size_t)4 * PKP_ROW;
    if (a->bd == 8) pack_kernel<uint8_t><<<grid_of<uint8_t>(a, n), THREADS, lds, st>>>(*a);
    else            pack_kernel<uint16_t><<<grid_of<uint16_t>(a, n), THREADS, lds, st>>>(*a);
}
