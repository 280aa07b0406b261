/*
 * compose.hip — finished pictures composed in place (oh_pics_compose; the exact definition is in DESIGN.md §3h and
 * tests/compose_model.py): an optional fill, then up to OH_COMPOSE_MAX_LAYERS rectangles of other finished pictures, each with an
 * opacity and an optional 8-bit alpha plane, source over destination in code values.
 *
 * One memory-bound pass, no intermediate picture.  A lane owns one 16-byte granule of one destination row — 16 samples at 8 bit, 8
 * above — and a workgroup a tile of OH_CPS_TW granules x OH_CPS_TH rows of one plane of one destination, one wave per row, so a wave
 * reads and writes 1 KiB of consecutive addresses.  The grid covers the area the call touches and nothing else: the bounding box of
 * the clipped layers, widened to whole granules, or the whole coded planes with a fill.  The lane walks the layers in list order with
 * the granule in registers: the destination is loaded at most once — not at all with a fill, and not before a layer needs it: an
 * opaque layer without alpha over the whole granule replaces it unread — and stored once, as one aligned 16-byte store (plane rows
 * start 256-byte aligned and are padded to 256 bytes); a granule no layer reaches is neither loaded nor stored.  Samples of a granule
 * that lie outside a layer get the weight 0, which the blend returns unchanged.
 *
 * The layer table is the same for every lane of a wave (the row is the wave's, the layer index the loop's): it is read through the
 * constant address space, into SGPRs.  Source rows and alpha planes lie anywhere relative to the destination's granules: a granule
 * whose 16 source bytes lie inside the source row (with its padding) takes them in one access aligned to the sample only, and a
 * granule that lies wholly inside a layer with unit alpha pixel stride takes its 8 to 64 alpha bytes in 8- and 16-byte accesses aligned
 * to nothing; the granules at a source row's ends, at a layer's left and right edge and alpha planes with another pixel stride (the
 * alpha channel of an RGBA image) go sample by sample and read nothing outside the layer.
 */
#include "pics_common.h"
#include "compose_common.h"

namespace {

#define CONSTANT __attribute__((address_space(4)))

typedef uint4v uint4v_a1 __attribute__((aligned(1)));
typedef uint4v uint4v_a2 __attribute__((aligned(2)));
typedef uint2v uint2v_a1 __attribute__((aligned(1)));

/* sample j of a granule */
template <typename T>
__device__ __forceinline__ uint32_t get(const uint4v &g, int j)
{
    if (sizeof(T) == 1)
        return (g[j >> 2] >> (8 * (j & 3))) & 0xff;
    return (g[j >> 1] >> (16 * (j & 1))) & 0xffff;
}
template <typename T>
__device__ __forceinline__ void put(uint4v &g, int j, uint32_t v)           /* into a zero */
{
    if (sizeof(T) == 1)
        g[j >> 2] |= v << (8 * (j & 3));
    else
        g[j >> 1] |= v << (16 * (j & 1));
}
__device__ __forceinline__ uint32_t byte_of(const uint32_t *w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xff; }

/* NB consecutive bytes from any address */
template <int NB>
__device__ __forceinline__ void load_bytes(uintptr_t p, uint32_t *w)
{
    static_assert(NB == 8 || NB == 16 || NB == 32, "8, 16 or 32 bytes");
    if (NB == 8) {
        const uint2v t = *(const GLOBAL uint2v_a1 *)p;
        w[0] = t[0]; w[1] = t[1];
    } else {
#pragma unroll
        for (int i = 0; i < NB / 16; i++) {
            const uint4v t = *(const GLOBAL uint4v_a1 *)(p + 16 * i);
            w[4 * i] = t[0]; w[4 * i + 1] = t[1]; w[4 * i + 2] = t[2]; w[4 * i + 3] = t[3];
        }
    }
}

template <typename T, bool FILL>
__global__ __launch_bounds__(THREADS) void compose_kernel(const OhCpsArgs a)
{
    constexpr int N = 16 / (int)sizeof(T);                      /* samples of a granule */
    const int pic = blockIdx.y, lane = threadIdx.x & 63, wrow = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per[2] = { a.k[0].tx * a.k[0].ty, a.k[1].tx * a.k[1].ty };
    int plane, q;
    const int tile = grid_row(blockIdx.x, per, plane, q);
    const OhCpsClass kc = a.k[q];                               /* a copy: the whole block in one load, under way during the division below */
    const int ty = tile / kc.tx, tx = tile - ty * kc.tx;
    const int Y = kc.y0 + ty * OH_CPS_TH + wrow, g = kc.gx0 + tx * OH_CPS_TW + lane;
    if (Y >= kc.y1 || g >= kc.gx1)
        return;
    const int X0 = g * N;                                       /* the granule's first sample in the plane */
    GLOBAL uint4v *dp = (GLOBAL uint4v *)((uintptr_t)a.dst[pic][plane] + (size_t)Y * (size_t)a.pitch[plane] + (size_t)g * 16);
    const int hs = q && (a.cf == 1 || a.cf == 2), vs = q && a.cf == 1;      /* luma alphas per sample of this plane: 1 << hs across, 1 << vs down */
    uint4v v = { 0, 0, 0, 0 };
    bool have = FILL;                                           /* v holds the granule */
    if (FILL) {
        const uint32_t f = (uint32_t)a.fill_v[plane] * (sizeof(T) == 1 ? 0x01010101u : 0x00010001u);
        v = uint4v{ f, f, f, f };
    }
    const CONSTANT OhCpsLayer *layers = (const CONSTANT OhCpsLayer *)a.layers;
    const CONSTANT OhCpsSrc *srcs = (const CONSTANT OhCpsSrc *)a.srcs;
    for (int k = 0; k < a.n_layers; k++) {
        const CONSTANT OhCpsLayer *L = layers + k;
        const int x0 = L->x0[q], x1 = L->x1[q];
        if (Y < L->y0[q] || Y >= L->y1[q])                      /* the wave's row: a uniform branch */
            continue;
        if (X0 + N <= x0 || X0 >= x1)
            continue;
        const bool whole = X0 >= x0 && X0 + N <= x1;            /* every sample of the granule is inside the layer */
        const CONSTANT OhCpsSrc *S = srcs + (size_t)k * (size_t)a.n_pics + (size_t)pic;
        const int opacity = L->opacity, has_alpha = L->has_alpha;

        /* the source samples under the granule */
        const int sp = L->spitch[q];
        const int sb = (X0 + L->ox[q]) * (int)sizeof(T);        /* byte of the source row under sample 0: may lie outside the row */
        const uintptr_t srow = (uintptr_t)S->p[plane] + (size_t)(Y + L->oy[q]) * (size_t)sp;
        uint4v s = { 0, 0, 0, 0 };
        if (sb >= 0 && sb + 16 <= sp) {
            if (sizeof(T) == 1)
                s = *(const GLOBAL uint4v_a1 *)(srow + sb);
            else
                s = *(const GLOBAL uint4v_a2 *)(srow + sb);
        } else {
#pragma unroll
            for (int j = 0; j < N; j++)
                if (X0 + j >= x0 && X0 + j < x1)
                    put<T>(s, j, *(const GLOBAL T *)(srow + (intptr_t)sb + j * (int)sizeof(T)));
        }
        if (whole && opacity == 256 && !has_alpha) {            /* the source as it is: the destination is not needed */
            v = s;
            have = true;
            continue;
        }

        /* the alpha of every sample: 0 outside the layer */
        uint32_t al[N];
        if (!has_alpha) {
#pragma unroll
            for (int j = 0; j < N; j++)
                al[j] = X0 + j >= x0 && X0 + j < x1 ? 255u : 0u;
        } else {
            const int64_t ps = L->a_ps, rs = L->a_rs;
            const uintptr_t arow = (uintptr_t)S->alpha + (uintptr_t)((int64_t)((Y - L->dy[q]) << vs) * rs);
            const int xa = (X0 - L->dx[q]) << hs;               /* the luma alpha column of sample 0: negative left of the layer */
            if (whole && ps == 1) {
                const uintptr_t p0 = arow + (uintptr_t)(int64_t)xa;
                if (!hs) {
                    uint32_t w[N / 4];
                    load_bytes<N>(p0, w);
#pragma unroll
                    for (int j = 0; j < N; j++)
                        al[j] = byte_of(w, j);
                } else {
                    uint32_t w0[N / 2], w1[N / 2];
                    load_bytes<2 * N>(p0, w0);
                    if (vs) {
                        load_bytes<2 * N>(p0 + (uintptr_t)rs, w1);
#pragma unroll
                        for (int j = 0; j < N; j++)
                            al[j] = compose_chroma_alpha(1, byte_of(w0, 2 * j), byte_of(w0, 2 * j + 1), byte_of(w1, 2 * j), byte_of(w1, 2 * j + 1));
                    } else {
#pragma unroll
                        for (int j = 0; j < N; j++)
                            al[j] = compose_chroma_alpha(2, byte_of(w0, 2 * j), byte_of(w0, 2 * j + 1), 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < N; j++) {
                    al[j] = 0;
                    if (X0 + j >= x0 && X0 + j < x1) {
                        const GLOBAL uint8_t *pa = (const GLOBAL uint8_t *)(arow + (uintptr_t)((int64_t)(xa + (j << hs)) * ps));
                        const uint32_t a00 = pa[0], a01 = hs ? pa[ps] : 0u;
                        const uint32_t a10 = vs ? pa[rs] : 0u, a11 = vs ? pa[rs + ps] : 0u;
                        al[j] = compose_chroma_alpha(vs ? 1 : hs ? 2 : 3, a00, a01, a10, a11);
                    }
                }
            }
        }

        if (!have) {
            v = *dp;
            have = true;
        }
        uint4v r = { 0, 0, 0, 0 };
#pragma unroll
        for (int j = 0; j < N; j++)
            put<T>(r, j, compose_blend(get<T>(v, j), get<T>(s, j), al[j], (uint32_t)opacity));
        v = r;
    }
    if (have)
        *dp = v;
}

} // namespace

static_assert(OH_CPS_TW * OH_CPS_TH == THREADS && OH_CPS_TW == 64, "a wave per tile row");
static_assert(sizeof(OhCpsArgs) <= 4096, "kernel arguments");
static_assert(sizeof(OhCpsLayer) % 8 == 0 && sizeof(OhCpsSrc) == 32, "the table's layout");

extern "C" void ohk_compose(const OhCpsArgs *a, int n, hipStream_t st)
{
    const dim3 grid((unsigned)(a->k[0].tx * a->k[0].ty + (a->np - 1) * a->k[1].tx * a->k[1].ty), (unsigned)n);
    if (a->bd > 8) {
        if (a->fill) compose_kernel<uint16_t, true><<<grid, THREADS, 0, st>>>(*a);
        else         compose_kernel<uint16_t, false><<<grid, THREADS, 0, st>>>(*a);
    } else {
        if (a->fill) compose_kernel<uint8_t, true><<<grid, THREADS, 0, st>>>(*a);
        else         compose_kernel<uint8_t, false><<<grid, THREADS, 0, st>>>(*a);
    }
}
