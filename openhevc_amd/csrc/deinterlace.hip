/*
 * deinterlace.hip — fields to frames, frames to fields and deinterlacing of finished pictures (oh_pics_weave, oh_pics_separate,
 * oh_pics_deinterlace; the exact definitions are in DESIGN.md §3l and tests/deinterlace_model.py; the sample formulas are
 * deinterlace_common.h, shared with the host).
 *
 * Memory-bound streaming over the CODED planes of the destinations, in the shape of reformat.hip: one workgroup (256 lanes) per
 * segment of OH_DI_SEG samples of one unit of rows of one plane; grid (segments, units of all planes, pictures of the launch — all of
 * them share one geometry; their plane addresses are in the kernel arguments).  Both global sides move as whole aligned 16-byte
 * granules (plane rows start 256-byte aligned and are padded, so a granule that holds a coded sample lies in its row); the samples
 * behind the coded width in the last granule lie in the row's padding, which nothing reads.
 *
 * fields_kernel (weave, separate): a unit is one row of one field; the row map is frame row 2 y + side <-> row y of the field of that
 * side.  A lane copies a granule at a time: global_load_dwordx4, global_store_dwordx4, nothing in between.
 *
 * deint_kernel: the rows go in PAIRS 2 u, 2 u + 1 of one plane, one of them kept (y % 2 == parity), one missing, so that every row a
 * lane loads serves both.  The vertical filters read only column x of their rows: a lane loads the granule of its columns from each of
 * the two (BOB), four (BLEND) or five (LOWPASS5) rows of a pair into registers, filters its 8 or 16 samples and stores two granules.
 * Their unit is four pairs, one after the other: the row window of a pair is that of the pair above it moved down by two rows, so the
 * rows they share stay in registers and a pair behind the first loads one (BOB) or two rows — 5, 10 and 11 loads for eight rows, not
 * 8, 16 and 20 that the caches had to absorb (at 10 bit BLEND went from 1.15 to 1.08 of a copy's time and LOWPASS5 from 1.33 to 1.08:
 * DESIGN.md §3l).
 * ADAPTIVE, whose unit is one pair, compares seven columns of the two kept rows up / dn of cur around x: those two rows of the segment, with one granule of halo
 * on either side, are staged in LDS (pics_common.h: stage; one barrier), and a lane reads the granule of its columns and the two
 * next to it (ds_read_b128: consecutive lanes read consecutive granules, no conflicts) into a window of GS + 6 samples in registers;
 * the granule at either edge of the plane takes its samples one by one, columns clamped.  Of prev, next and row y of cur it needs
 * column x only: six register granules straight from HBM.  The kept row is copied out of the staged one.
 * Templates on the stored sample type and on ADAPTIVE (LDS, more registers); the other modes are a uniform branch.
 */
#include <algorithm>
#include "pics_common.h"
#include "deinterlace_common.h"

namespace {

constexpr int SEG = OH_DI_SEG;

/* pairs of rows in a unit of deint_kernel: the vertical filters take four, which share the rows between them */
__host__ __device__ constexpr int unit_pairs(bool adaptive) { return adaptive ? 1 : 4; }

/* bytes of one staged row of ADAPTIVE: a segment and a granule of halo on either side */
template <typename T>
constexpr int slot_bytes() { return (SEG * (int)sizeof(T) + 2 * 16 + 32 + 15) / 16 * 16; }

template <typename T>
__global__ __launch_bounds__(THREADS) void fields_kernel(const OhDiArgs a)
{
    constexpr int SZ = (int)sizeof(T), GS = 16 / SZ;
    const int pic = blockIdx.z;
    const int per[2] = { a.h[0] >> 1, a.h[1] >> 1 };            /* rows of a field's planes */
    const int units = per[0] + (a.np > 1 ? 2 * per[1] : 0);
    const int si = blockIdx.y / units;
    const int side = a.sides == 3 ? si : a.sides >> 1;          /* 0 top, 1 bottom */
    int c, q;
    const int y = grid_row(blockIdx.y - si * units, per, c, q);
    const int pw = (a.w[q] + GS - 1) & ~(GS - 1);               /* with the rest of the last granule */
    const int X0 = blockIdx.x * SEG;
    if (X0 >= pw)
        return;
    const int cnt = min(SEG, pw - X0);
    const size_t in_frame = (size_t)(2 * y + side) * a.pitch[c] + (size_t)X0 * SZ, in_field = (size_t)y * a.fpitch[c] + (size_t)X0 * SZ;
    uintptr_t src, dst;
    if (a.op == OH_DI_WEAVE) {
        src = (uintptr_t)a.pic[side][pic][c] + in_field;
        dst = (uintptr_t)a.pic[3][pic][c] + in_frame;
    } else {
        src = (uintptr_t)a.pic[0][pic][c] + in_frame;
        dst = (uintptr_t)a.pic[2 + side][pic][c] + in_field;
    }
    for (int g = threadIdx.x; g < cnt / GS; g += THREADS)
        *(GLOBAL uint4v *)(dst + 16 * (uintptr_t)g) = *(const GLOBAL uint4v *)(src + 16 * (uintptr_t)g);
}

template <typename T, bool ADAPT>
__global__ __launch_bounds__(THREADS) void deint_kernel(const OhDiArgs a)
{
    constexpr int SZ = (int)sizeof(T), GS = 16 / SZ;
    typedef Samples<T> Sm;
    extern __shared__ __attribute__((aligned(16))) uint8_t rows_l[];           /* ADAPTIVE: rows up and dn of cur, slot_bytes each */
    constexpr int PAIRS = unit_pairs(ADAPT);
    const int pic = blockIdx.z;
    const int per[2] = { ((a.h[0] >> 1) + PAIRS - 1) / PAIRS, ((a.h[1] >> 1) + PAIRS - 1) / PAIRS };
    int c, q;
    const int u = grid_row(blockIdx.y, per, c, q) * PAIRS;      /* the unit's first pair */
    const int W = a.w[q], H = a.h[q], M = (1 << a.bd) - 1;
    const int pw = (W + GS - 1) & ~(GS - 1);                    /* with the rest of the last granule */
    const int X0 = blockIdx.x * SEG;
    if (X0 >= pw)
        return;
    const int cnt = min(SEG, pw - X0);
    const int k = 2 * u + a.parity, y = 2 * u + 1 - a.parity;  /* the kept row and the missing one */
    const int up = y - 1 >= 0 ? y - 1 : y + 1, dn = y + 1 <= H - 1 ? y + 1 : y - 1;      /* mirrored: kept rows; one of them is k */
    const size_t pitch = (size_t)a.pitch[c], at = (size_t)X0 * SZ;
    const uintptr_t C = (uintptr_t)a.pic[1][pic][c] + at, D = (uintptr_t)a.pic[3][pic][c] + at;
    auto ld = [&](uintptr_t plane, int row, int g) { return *(const GLOBAL uint4v *)(plane + (size_t)row * pitch + 16 * (uintptr_t)g); };
    auto st = [&](int row, int g, uint4v v) { *(GLOBAL uint4v *)(D + (size_t)row * pitch + 16 * (uintptr_t)g) = v; };
    auto r = [&](int row) { return min(max(row, 0), H - 1); }; /* clamped */

    if constexpr (!ADAPT) {
        /* the unit's pairs one after the other, the rows they share kept in registers: the row window of a pair is that of the pair
         * above it moved down by two rows (clamping and mirroring included), so a pair behind the first loads one (BOB) or two rows */
        const int n_pairs = min(PAIRS, (H >> 1) - u);
        for (int g = threadIdx.x; g < cnt / GS; g += THREADS) {
            Sm o;
            if (a.mode == OH_DEINT_BOB) {
                uint4v vu = ld(C, up, g);                       /* the row above the first missing one; below it: the next pair's above */
                for (int i = 0; i < n_pairs; i++) {
                    const int yi = y + 2 * i;
                    const uint4v vd = ld(C, yi + 1 <= H - 1 ? yi + 1 : yi - 1, g);
                    const Sm su(vu), sd(vd);
#pragma unroll
                    for (int s = 0; s < GS; s++)
                        o.s[s] = (T)deint_bob(su.s[s], sd.s[s]);
                    st(k + 2 * i, g, a.parity ? vd : vu);
                    st(yi, g, o.granule());
                    vu = vd;
                }
            } else if (a.mode == OH_DEINT_BLEND) {
                uint4v w0 = ld(C, r(2 * u - 1), g), w1 = ld(C, 2 * u, g);
                for (int i = 0; i < n_pairs; i++) {
                    const int y0 = 2 * (u + i);
                    const uint4v w2 = ld(C, y0 + 1, g), w3 = ld(C, r(y0 + 2), g);
                    const Sm r0(w0), r1(w1), r2(w2), r3(w3);
#pragma unroll
                    for (int s = 0; s < GS; s++)
                        o.s[s] = (T)deint_blend(r0.s[s], r1.s[s], r2.s[s]);
                    st(y0, g, o.granule());
#pragma unroll
                    for (int s = 0; s < GS; s++)
                        o.s[s] = (T)deint_blend(r1.s[s], r2.s[s], r3.s[s]);
                    st(y0 + 1, g, o.granule());
                    w0 = w2; w1 = w3;
                }
            } else {                                            /* OH_DEINT_LOWPASS5: the kept row is y - 1 or y + 1, never clamped */
                uint4v w0 = ld(C, r(y - 2), g), w1 = ld(C, r(y - 1), g), w2 = ld(C, y, g);
                for (int i = 0; i < n_pairs; i++) {
                    const int yi = y + 2 * i;
                    const uint4v w3 = ld(C, r(yi + 1), g), w4 = ld(C, r(yi + 2), g);
                    const Sm m2(w0), m1(w1), c0(w2), p1(w3), p2(w4);
#pragma unroll
                    for (int s = 0; s < GS; s++)
                        o.s[s] = (T)deint_lowpass5(m2.s[s], m1.s[s], c0.s[s], p1.s[s], p2.s[s], M);
                    st(k + 2 * i, g, a.parity ? w3 : w1);
                    st(yi, g, o.granule());
                    w0 = w2; w1 = w3; w2 = w4;
                }
            }
        }
    } else {
        constexpr int SLOT = slot_bytes<T>();
        /* the staged columns [lo, hi] of rows up and dn: the segment and a granule on either side, inside the row's granules */
        const int lo = max(X0 - GS, 0), hi = min(X0 + cnt + GS, pw) - 1;
        const int bu = stage<T>(rows_l, (const uint8_t *)a.pic[1][pic][c] + (size_t)up * pitch + (size_t)lo * SZ, hi - lo + 1);
        const int bd = stage<T>(rows_l + SLOT, (const uint8_t *)a.pic[1][pic][c] + (size_t)dn * pitch + (size_t)lo * SZ, hi - lo + 1);
        __syncthreads();
        const LDS T *U = (const LDS T *)((const LDS uint8_t *)rows_l) + bu - lo;           /* U[x]: column x of row up */
        const LDS T *E = (const LDS T *)((const LDS uint8_t *)rows_l + SLOT) + bd - lo;
        const uintptr_t P = (uintptr_t)a.pic[0][pic][c] + at, N = (uintptr_t)a.pic[2][pic][c] + at;
        const uintptr_t O = a.kept_first ? P : N;               /* the other picture that holds the missing field next to the kept one */
        for (int g = threadIdx.x; g < cnt / GS; g += THREADS) {
            const int Xg = X0 + g * GS;
            const Sm cy(ld(C, y, g)), oy(ld(O, y, g)), pu(ld(P, up, g)), pd(ld(P, dn, g)), nu(ld(N, up, g)), nd(ld(N, dn, g));
            int32_t wu[GS + 6], wd[GS + 6];                     /* wu[j]: column cx(Xg - 3 + j) of row up */
            if (Xg >= GS && Xg + GS + 2 <= W - 1) {             /* the granules on either side are staged and nothing is clamped */
                typedef T Granule __attribute__((ext_vector_type(GS)));
                typedef Granule GranuleA __attribute__((aligned(16)));      /* plane rows are 16-byte aligned, and so are lo and Xg */
#pragma unroll
                for (int t = 0; t < 3; t++) {
                    const Granule gu = *(const LDS GranuleA *)(U + Xg + (t - 1) * GS), gd = *(const LDS GranuleA *)(E + Xg + (t - 1) * GS);
#pragma unroll
                    for (int i = 0; i < GS; i++) {
                        const int j = (t - 1) * GS + i + 3;
                        if (j >= 0 && j < GS + 6) { wu[j] = gu[i]; wd[j] = gd[i]; }
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < GS + 6; j++) {
                    const int x = min(max(Xg - 3 + j, 0), W - 1);
                    wu[j] = U[x]; wd[j] = E[x];
                }
            }
            Sm o, kept;
#pragma unroll
            for (int i = 0; i < GS; i++) {
                o.s[i] = (T)deint_adaptive(wu + i, wd + i, oy.s[i], cy.s[i], pu.s[i], pd.s[i], nu.s[i], nd.s[i]);
                kept.s[i] = (T)(a.parity ? wd[3 + i] : wu[3 + i]);
            }
            st(k, g, kept.granule());
            st(y, g, o.granule());
        }
    }
}

template <typename T>
void launch_fields(const OhDiArgs *a, int n, hipStream_t st)
{
    const int G = 16 / (int)sizeof(T), cls = a->np > 1 ? 2 : 1;
    int pw = 0;
    for (int q = 0; q < cls; q++)
        pw = std::max(pw, (a->w[q] + G - 1) / G * G);
    const int units = (a->h[0] >> 1) + (cls > 1 ? 2 * (a->h[1] >> 1) : 0);
    const dim3 grid((unsigned)((pw + SEG - 1) / SEG), (unsigned)(units * (a->sides == 3 ? 2 : 1)), (unsigned)n);
    fields_kernel<T><<<grid, THREADS, 0, st>>>(*a);
}

template <typename T>
void launch_deint(const OhDiArgs *a, int n, hipStream_t st)
{
    const int G = 16 / (int)sizeof(T), cls = a->np > 1 ? 2 : 1;
    int pw = 0;
    for (int q = 0; q < cls; q++)
        pw = std::max(pw, (a->w[q] + G - 1) / G * G);
    const int pairs = unit_pairs(a->mode == OH_DEINT_ADAPTIVE);
    const int units = ((a->h[0] >> 1) + pairs - 1) / pairs + (cls > 1 ? 2 * (((a->h[1] >> 1) + pairs - 1) / pairs) : 0);
    const dim3 grid((unsigned)((pw + SEG - 1) / SEG), (unsigned)units, (unsigned)n);
    if (a->mode == OH_DEINT_ADAPTIVE)
        deint_kernel<T, true><<<grid, THREADS, (size_t)2 * slot_bytes<T>(), st>>>(*a);
    else
        deint_kernel<T, false><<<grid, THREADS, 0, st>>>(*a);
}

} // namespace

static_assert(OH_DI_SEG % 16 == 0, "a segment is whole 16-byte granules of either sample type");

extern "C" void ohk_deinterlace(const OhDiArgs *a, int n, hipStream_t st)
{
    if (a->bd == 8) launch_deint<uint8_t>(a, n, st);
    else            launch_deint<uint16_t>(a, n, st);
}

extern "C" void ohk_fields(const OhDiArgs *a, int n, hipStream_t st)
{
    if (a->bd == 8) launch_fields<uint8_t>(a, n, st);
    else            launch_fields<uint16_t>(a, n, st);
}
