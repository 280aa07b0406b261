/*
 * remap.hip — finished 4:4:4 pictures -> finished 4:4:4 pictures whose samples are a function of all three components of the source
 * sample (oh_pics_colour_remap; the exact definition is in DESIGN.md §3r and tests/remap_model.py): a table per component, a 3 x 3
 * matrix, a second table per component, at any pair of bit depths.  It is lut.hip with three planes at a time.
 *
 * A workgroup (256 lanes) takes a band of a.rows rows of one picture and first copies the six tables into LDS as packed uint16 entries:
 * (3 * 2^bi + 3 * 2^bo) * 2 bytes, 3 KB at 8 -> 8, 12 KB at 10 -> 10, 48 KB at 12 -> 12, which leaves three workgroups a CU of the
 * 160 KiB — once for the band, not once per row.  A lane then takes units of OH_LUT_UNIT = 16 samples: one or two aligned 16-byte
 * granules from the same place of each of the three source planes, 48 pre gathers, 16 samples through the matrix of remap_common.h,
 * 48 post gathers, and whole granules stored to the three destination planes, whatever the pair of sample types.  Plane rows start
 * 256-byte aligned and are padded to 256 bytes, so the unit that holds the last coded sample lies in its row on both sides; the samples
 * behind the coded width in it come from the source rows' padding and go to the destination rows', which nothing reads.  A source
 * sample above 2^bi - 1 is looked up by its low bits, a matrix result is clipped to 0 .. 2^bo - 1, and the host has seen to it that no
 * pre-table entry lies above 2^bo - 1: no read leaves a table.
 */
#include "pics_common.h"
#include "remap_common.h"

namespace {

template <typename TI, typename TS, bool IDENT>
__global__ __launch_bounds__(THREADS) void remap_kernel(const OhRemapArgs a)
{
    constexpr int U = OH_LUT_UNIT, NI = Unit<TI>::N, NO = Unit<TS>::N;         /* granules of a unit, in and out */
    extern __shared__ __attribute__((aligned(16))) uint16_t tab[];               /* 3 << sbd pre entries, then 3 << dbd post entries */
    const int pic = blockIdx.y, t = threadIdx.x;
    const int ni = 1 << a.sbd, no = 1 << a.dbd;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const GLOBAL uint4v *src_tab = (const GLOBAL uint4v *)(a.tab + k * OH_LUT_MAX);
        uint4v *lds = (uint4v *)(tab + (k < 3 ? k * ni : 3 * ni + (k - 3) * no));
        for (int i = t; i < (k < 3 ? ni : no) / 8; i += THREADS)
            lds[i] = src_tab[i];
    }
    __syncthreads();
    const uint16_t *pre0 = tab, *pre1 = tab + ni, *pre2 = tab + 2 * ni, *post0 = tab + 3 * ni, *post1 = post0 + no, *post2 = post1 + no;
    const uint32_t Mi = (uint32_t)ni - 1;
    const int32_t Mo = no - 1;
    const int units = (a.w + U - 1) / U, r0 = blockIdx.x * a.rows, total = min(a.rows, a.h - r0) * units;
    for (int i = t; i < total; i += THREADS) {
        const int r = i / units, u = i - r * units;
        uint4v in[3][NI];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const GLOBAL uint4v *s = (const GLOBAL uint4v *)((const GLOBAL uint8_t *)a.src[pic][c] + (size_t)(r0 + r) * (size_t)a.spitch[c] +
                                                             (size_t)u * (U * sizeof(TI)));
#pragma unroll
            for (int g = 0; g < NI; g++)
                in[c][g] = s[g];
        }
        uint4v out[3][NO];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int g = 0; g < NO; g++)
                out[c][g] = uint4v{ 0, 0, 0, 0 };
#pragma unroll
        for (int j = 0; j < U; j++) {
            uint32_t s[3], o[3];
#pragma unroll
            for (int c = 0; c < 3; c++)
                s[c] = unit_get<TI>(in[c], j);                  /* remap_sample keeps the low bits */
            remap_sample<IDENT>(pre0, pre1, pre2, post0, post1, post2, a.coeff, a.log2_denom, Mi, Mo, s, o);
#pragma unroll
            for (int c = 0; c < 3; c++)
                unit_put<TS>(out[c], j, o[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            GLOBAL uint4v *d = (GLOBAL uint4v *)((GLOBAL uint8_t *)a.dst[pic][c] + (size_t)(r0 + r) * (size_t)a.dpitch[c] + (size_t)u * (U * sizeof(TS)));
#pragma unroll
            for (int g = 0; g < NO; g++)
                d[g] = out[c][g];
        }
    }
}

template <typename TI, typename TS>
void launch(const OhRemapArgs *a, int n, hipStream_t st)
{
    const dim3 grid((unsigned)((a->h + a->rows - 1) / a->rows), (unsigned)n);
    const size_t lds = (((size_t)3 << a->sbd) + ((size_t)3 << a->dbd)) * sizeof(uint16_t);
    if (a->identity) remap_kernel<TI, TS, true><<<grid, THREADS, lds, st>>>(*a);
    else             remap_kernel<TI, TS, false><<<grid, THREADS, lds, st>>>(*a);
}

} // namespace

static_assert(sizeof(OhRemapArgs) <= 4096, "kernel arguments");
static_assert(OH_LUT_UNIT == 16, "a unit is whole granules of 8-bit and of 16-bit samples, and a 256-byte row holds whole units of both");
static_assert(6 * OH_LUT_MAX * sizeof(uint16_t) <= 64 * 1024, "the six tables at 12 -> 12 bit fit the LDS of a workgroup");

extern "C" void ohk_remap(const OhRemapArgs *a, int n, hipStream_t st)
{
    with_sample_types(a->sbd, a->dbd, [&](auto ti, auto ts) { launch<decltype(ti), decltype(ts)>(a, n, st); });
}
