/*
 * grain.hip — finished pictures -> finished pictures with synthesised film grain added (oh_pics_grain; the exact definition is in
 * include/ohevc_hip.h, DESIGN.md §3q and tests/grain_model.py; the arithmetic of a sample is grain_common.h, which the host shares).
 *
 * One kernel, one pass over the picture.  A workgroup (256 lanes) takes one row of 8 x 8 blocks, GRAIN_TW = 32 blocks (256 samples)
 * across, of one plane of one picture: lane (r, b) holds the 8 samples of row r of block b in registers from its one load (8 or 16
 * bytes, a whole row of 256 samples per 32 lanes) to its one store.
 *   1. every lane sums its 8 samples into LDS (sums[r][b]); the first 16 lanes also sum the rows of the block on either side of the
 *      tile, whose grain the smoothing of the tile's outer columns reads;
 *   2. 34 lanes add the 8 row sums of a block — no atomics — and make its descriptor: the table entry of its mean, and from the hash of
 *      (seed, plane, block) where it lies in its pattern and whether the pattern is negated (desc[], 4 bytes a block);
 *   3. every lane reads its own and the two neighbouring descriptors, gathers its 8 pattern bytes as two dwords at any byte address and
 *      one byte of each neighbour's pattern, smooths its two outer samples, blends and stores.
 * The patterns (169 KB) stay in HBM behind the caches: a call uses the few that its tables name, 1 KB each.  A plane that is not selected
 * is copied by the same lanes.  Plane rows start 256-byte aligned and are padded to 256 bytes, and plane widths are multiples of 4: a
 * block cut by the right edge is loaded and stored whole, its last 4 samples in the padding of the rows, which nothing reads; they
 * stay out of the sums.  A source sample above 2^bit depth - 1, which no decoder and no service writes, cannot take a mean past
 * the table: the mean is clamped to 255.
 */
#include "pics_common.h"
#include "grain_common.h"

namespace {

template <typename T> struct Row;                               /* the 8 samples of a lane */
template <> struct Row<uint8_t>  { typedef uint2v V; };
template <> struct Row<uint16_t> { typedef uint4v V; };

template <typename T> __device__ __forceinline__ int sample_of(const typename Row<T>::V &v, int i)
{
    constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    return (int)(v[i / PER] >> (BITS * (i % PER))) & ((1 << BITS) - 1);
}

/* the sum of the first `valid` (8 or 4) samples */
template <typename T> __device__ __forceinline__ uint32_t row_sum(const typename Row<T>::V &v, int valid)
{
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < GRAIN_BLOCK; i++)
        s += i < valid ? (uint32_t)sample_of<T>(v, i) : 0u;
    return s;
}

/* the unsmoothed grain of the sample at column i (0 .. 7) of row r of a block with descriptor d */
__device__ __forceinline__ int32_t edge_grain(const GLOBAL int8_t *patterns, uint32_t d, int r, int i, int bd, int log2_scale)
{
    const int sigma = (int)(d & 255);
    if (!sigma)
        return 0;
    const int fh = (int)(d >> 8 & 15), fv = (int)(d >> 12 & 15), ox = (int)(d >> 16 & 31), oy = (int)(d >> 21 & 31);
    const int p = patterns[grain_pattern_index(fh, fv) * (GRAIN_PAT * GRAIN_PAT) + (oy + r) * GRAIN_PAT + ox + i];
    return grain_value(sigma, (d >> 26 & 1) ? -p : p, bd, log2_scale);
}

template <typename T>
__global__ __launch_bounds__(THREADS) void grain_kernel(const OhGrainArgs a)
{
    typedef typename Row<T>::V V;
    __shared__ uint32_t sums[GRAIN_BLOCK][GRAIN_TW + 2];        /* [row][block]: 0 and GRAIN_TW + 1 the blocks beside the tile */
    __shared__ uint32_t desc[GRAIN_TW + 2];
    const int pic = blockIdx.y, t = threadIdx.x;
    const int per[2] = { a.tx[0] * a.ty[0], a.tx[1] * a.ty[1] };
    int plane, q;
    const int tile = grid_row(blockIdx.x, per, plane, q);
    const int W = a.w[q], H = a.h[q];
    const int by = tile / a.tx[q], bx0 = (tile - by * a.tx[q]) * GRAIN_TW;      /* the tile's block row and its first block */
    const int r = t / GRAIN_TW, b = t % GRAIN_TW;
    const int bx = bx0 + b, x0 = bx * GRAIN_BLOCK, y = by * GRAIN_BLOCK + r;
    const bool in = x0 < W && y < H;
    const bool sel = (a.planes >> plane) & 1;                   /* the same for the whole workgroup */
    const size_t pitch = (size_t)a.pitch[plane];
    const GLOBAL uint8_t *sp = (const GLOBAL uint8_t *)a.src[pic][plane];
    V v = {};
    if (in)
        v = *(const GLOBAL V *)(sp + (size_t)y * pitch + (size_t)x0 * sizeof(T));
    if (!sel) {                                                 /* the copy */
        if (in)
            *(GLOBAL V *)((GLOBAL uint8_t *)a.dst[pic][plane] + (size_t)y * pitch + (size_t)x0 * sizeof(T)) = v;
        return;
    }
    sums[r][b + 1] = in ? row_sum<T>(v, min(GRAIN_BLOCK, W - x0)) : 0u;
    if (t < 2 * GRAIN_BLOCK) {                                  /* row t & 7 of the block in front of the tile (side 0) or behind it */
        const int side = t / GRAIN_BLOCK, hr = t % GRAIN_BLOCK;
        const int hx = (side ? bx0 + GRAIN_TW : bx0 - 1) * GRAIN_BLOCK, hy = by * GRAIN_BLOCK + hr;
        uint32_t s = 0;
        if (hx >= 0 && hx < W && hy < H) {
            const V hv = *(const GLOBAL V *)(sp + (size_t)hy * pitch + (size_t)hx * sizeof(T));
            s = row_sum<T>(hv, min(GRAIN_BLOCK, W - hx));
        }
        sums[hr][side ? GRAIN_TW + 1 : 0] = s;
    }
    __syncthreads();
    if (t < GRAIN_TW + 2) {
        const int dbx = bx0 - 1 + t, dx0 = dbx * GRAIN_BLOCK;
        uint32_t d = 0;
        if (dbx >= 0 && dx0 < W) {
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < GRAIN_BLOCK; i++)
                s += sums[i][t];
            const int n = min(GRAIN_BLOCK, W - dx0) * min(GRAIN_BLOCK, H - by * GRAIN_BLOCK);
            const int a8 = min(grain_mean(s, n, a.bd), OH_GRAIN_ENTRIES - 1);
            const uint32_t entry = ((const GLOBAL uint32_t *)a.tab)[plane * OH_GRAIN_ENTRIES + a8];
            int ox, oy, negate;
            grain_block(((const GLOBAL uint32_t *)a.seeds)[pic], plane, dbx, by, &ox, &oy, &negate);
            d = grain_desc(entry, ox, oy, negate);
        }
        desc[t] = d;
    }
    __syncthreads();
    if (!in)
        return;
    const GLOBAL int8_t *patterns = (const GLOBAL int8_t *)a.patterns;
    const uint32_t d = desc[b + 1];
    const int sigma = (int)(d & 255);
    V out = v;
    if (sigma || (desc[b] & 255) || (desc[b + 2] & 255)) {      /* else neither the block nor a neighbour has grain */
        int32_t g[GRAIN_BLOCK] = {};
        if (sigma) {
            const int fh = (int)(d >> 8 & 15), fv = (int)(d >> 12 & 15), ox = (int)(d >> 16 & 31), oy = (int)(d >> 21 & 31);
            const bool negate = d >> 26 & 1;
            const GLOBAL int8_t *p = patterns + grain_pattern_index(fh, fv) * (GRAIN_PAT * GRAIN_PAT) + (oy + r) * GRAIN_PAT + ox;
            const uint32_t lo = *(const GLOBAL unsigned_a1 *)p, hi = *(const GLOBAL unsigned_a1 *)(p + 4);
#pragma unroll
            for (int i = 0; i < GRAIN_BLOCK; i++) {
                const int pv = (int)(int8_t)((i < 4 ? lo : hi) >> (8 * (i & 3)));
                g[i] = grain_value(sigma, negate ? -pv : pv, a.bd, a.log2_scale);
            }
        }
        const int32_t g0 = bx > 0 ? grain_smooth(edge_grain(patterns, desc[b], r, GRAIN_BLOCK - 1, a.bd, a.log2_scale), g[0], g[1]) : g[0];
        const int32_t g7 = x0 + GRAIN_BLOCK < W ? grain_smooth(g[6], g[7], edge_grain(patterns, desc[b + 2], r, 0, a.bd, a.log2_scale)) : g[7];
        g[0] = g0; g[7] = g7;
        constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
        out = V{};
#pragma unroll
        for (int i = 0; i < GRAIN_BLOCK; i++)
            out[i / PER] |= (uint32_t)grain_blend(sample_of<T>(v, i), g[i], a.bd, a.blending) << (BITS * (i % PER));
    }
    *(GLOBAL V *)((GLOBAL uint8_t *)a.dst[pic][plane] + (size_t)y * pitch + (size_t)x0 * sizeof(T)) = out;
}

} // namespace

static_assert(sizeof(OhGrainArgs) <= 4096, "kernel arguments");
static_assert(GRAIN_TW * GRAIN_BLOCK == THREADS, "a lane per row of a block of the tile");
static_assert(GRAIN_TW + 2 <= THREADS && 2 * GRAIN_BLOCK <= THREADS, "lanes for the descriptors and for the blocks beside the tile");

extern "C" void ohk_grain(const OhGrainArgs *a, int n, hipStream_t st)
{
    const dim3 grid((unsigned)(a->tx[0] * a->ty[0] + (a->np - 1) * a->tx[1] * a->ty[1]), (unsigned)n);
    if (a->bd == 8) grain_kernel<uint8_t><<<grid, THREADS, 0, st>>>(*a);
    else            grain_kernel<uint16_t><<<grid, THREADS, 0, st>>>(*a);
}
