/*
 * lut.hip — finished pictures -> finished pictures whose samples are a function of the source sample alone (oh_pics_lut; the exact
 * definition is in DESIGN.md §3n and tests/levels_model.py): dst = table[plane][src] over the whole coded planes, at any pair of bit
 * depths; a plane that is not selected is copied.
 *
 * Memory-bound streaming like reformat.hip's copy form, without its staging: a sample needs no neighbour, so a lane goes from HBM to
 * HBM through registers.  A workgroup (256 lanes) takes OH_LUT_ROWS rows of one plane of one picture and first copies the plane's table
 * into LDS as uint16 entries (512 bytes at 8 bit, 8 KB at 12) — once for 16 rows, not once per row.  A lane then takes units of
 * OH_LUT_UNIT = 16 samples: one or two aligned 16-byte granules of the source row (global_load_dwordx4), sixteen ds_read_u16 gathers,
 * one or two whole granules stored (global_store_dwordx4), whatever the pair of sample types.  Plane rows start 256-byte aligned and are
 * padded to 256 bytes, so the unit that holds the last coded sample lies in its row on both sides; the samples behind the coded width in
 * it come from the source row's padding and go to the destination row's, which nothing reads.
 *
 * The gather and the LDS banks: entries are packed two to a bank word.  Beside one entry per word this halves the LDS of a workgroup
 * and the words a wave's 64 lookups can fall into; two lanes that read the two halves of one word are served together, as are lanes
 * that read the same entry — which is the common case in a natural picture.  Lookups that fall into different words of one bank are
 * served one after the other: that is inherent in a gather of random values, and copies of the table would only help if lanes were
 * bound to copies, which costs the LDS that lets more workgroups share a CU.  A source sample above 2^bit depth - 1, which no decoder
 * and no service writes, is looked up by its low bits: no read leaves the table.
 */
#include "pics_common.h"

namespace {

template <typename TI, typename TS>
__global__ __launch_bounds__(THREADS) void lut_kernel(const OhLutArgs a)
{
    constexpr int U = OH_LUT_UNIT, NI = Unit<TI>::N, NO = Unit<TS>::N;         /* granules of a unit, in and out */
    extern __shared__ __attribute__((aligned(16))) uint16_t tab[];               /* 1 << sbd entries */
    const int pic = blockIdx.y, t = threadIdx.x;
    const int per[2] = { (a.h[0] + OH_LUT_ROWS - 1) / OH_LUT_ROWS, (a.h[1] + OH_LUT_ROWS - 1) / OH_LUT_ROWS };
    int plane, q;
    const int tile = grid_row(blockIdx.x, per, plane, q);
    const bool sel = (a.planes >> plane) & 1;                   /* the same for the whole workgroup */
    const uint32_t mask = (1u << a.sbd) - 1;
    if (sel) {
        const GLOBAL uint4v *src_tab = (const GLOBAL uint4v *)(a.tab + plane * OH_LUT_MAX);
        for (int i = t; i < (2 << a.sbd) / 16; i += THREADS)
            ((uint4v *)tab)[i] = src_tab[i];
        __syncthreads();
    }
    const int units = (a.w[q] + U - 1) / U, r0 = tile * OH_LUT_ROWS, total = min(OH_LUT_ROWS, a.h[q] - r0) * units;
    const size_t sp = (size_t)a.spitch[plane], dp = (size_t)a.dpitch[plane];
    const GLOBAL uint8_t *sb = (const GLOBAL uint8_t *)a.src[pic][plane] + (size_t)r0 * sp;
    GLOBAL uint8_t *db = (GLOBAL uint8_t *)a.dst[pic][plane] + (size_t)r0 * dp;
    for (int i = t; i < total; i += THREADS) {
        const int r = i / units, u = i - r * units;
        const GLOBAL uint4v *s = (const GLOBAL uint4v *)(sb + (size_t)r * sp + (size_t)u * (U * sizeof(TI)));
        GLOBAL uint4v *d = (GLOBAL uint4v *)(db + (size_t)r * dp + (size_t)u * (U * sizeof(TS)));
        uint4v in[NI];
#pragma unroll
        for (int g = 0; g < NI; g++)
            in[g] = s[g];
        if (!sel) {                                             /* the copy: the host has seen to equal depths */
            if constexpr (NI == NO) {
#pragma unroll
                for (int g = 0; g < NO; g++)
                    d[g] = in[g];
            }
            continue;
        }
        uint4v out[NO];
#pragma unroll
        for (int g = 0; g < NO; g++)
            out[g] = uint4v{ 0, 0, 0, 0 };
#pragma unroll
        for (int j = 0; j < U; j++) {
            unit_put<TS>(out, j, tab[unit_get<TI>(in, j) & mask]);
        }
#pragma unroll
        for (int g = 0; g < NO; g++)
            d[g] = out[g];
    }
}

template <typename TI, typename TS>
void launch(const OhLutArgs *a, int n, hipStream_t st)
{
    const int tiles = (a->h[0] + OH_LUT_ROWS - 1) / OH_LUT_ROWS + (a->np - 1) * ((a->h[1] + OH_LUT_ROWS - 1) / OH_LUT_ROWS);
    const dim3 grid((unsigned)tiles, (unsigned)n);
    lut_kernel<TI, TS><<<grid, THREADS, (size_t)2 << a->sbd, st>>>(*a);
}

} // namespace

static_assert(sizeof(OhLutArgs) <= 4096, "kernel arguments");
static_assert(OH_LUT_UNIT == 16, "a unit is whole granules of 8-bit and of 16-bit samples, and a 256-byte row holds whole units of both");

extern "C" void ohk_lut(const OhLutArgs *a, int n, hipStream_t st)
{
    with_sample_types(a->sbd, a->dbd, [&](auto ti, auto ts) { launch<decltype(ti), decltype(ts)>(a, n, st); });
}
