/*
 * orient.hip — finished pictures -> finished pictures, cropped, mirrored, turned by quarter turns or transposed (oh_pics_orient; the
 * exact definition is in DESIGN.md §3k and tests/orient_model.py).  A permutation of stored samples: memory-bound, every byte moves
 * once in each direction, both global sides as whole aligned 16-byte granules (plane rows start 256-byte aligned and are padded, so a
 * granule that holds a coded sample lies in its row).  Per plane S is the source window (Ws x Hs); the image I is Wi x Hi; the
 * destination's coded plane D replicates I's last column and row: D[y][x] = I[min(y, Hi - 1)][min(x, Wi - 1)].
 *
 * Orientations 0 .. 3 (I[y][x] = S[VFLIP ? Hs - 1 - y : y][HFLIP ? Ws - 1 - x : x]): orient_rows_kernel, in the shape of reformat.hip.
 * One workgroup (256 lanes) per segment of OH_OR_SEG samples of one destination row; grid (segments, rows of all planes, pictures).
 *   1. stage    the source samples of the segment go to LDS as the aligned granules that cover them (pics_common.h: stage);
 *   2. assemble each lane makes one aligned destination granule at a time: the 16 source bytes behind it lie anywhere in LDS, so it
 *               reads the five dwords that cover them and funnel-shifts them into four (v_alignbit_b32; the shift is the same for the
 *               whole workgroup); under HFLIP the four come out in reverse order with their samples reversed (v_perm_b32 / a rotate).
 *               VFLIP is the row index.  A granule that reaches behind the image's last column takes its samples one by one out of
 *               LDS, clamped; a row below the image reads the image's last row again.
 *
 * Orientations 4 .. 7 (I[y][x] = S[HFLIP ? Hs - 1 - x : x][VFLIP ? Ws - 1 - y : y], Wi = Hs, Hi = Ws): orient_tile_kernel.  One
 * workgroup of ONE wave per run of OR_RUN_X x OR_RUN_Y square tiles of OH_OR_TILE x OH_OR_TILE destination samples, one tile after the
 * other; grid (runs across, runs down of all planes, pictures).  Per tile:
 *   1. stage    LDS row j holds the source row that destination column X0 + j reads (so HFLIP and the replicated columns are the
 *               choice of that row), as the aligned granules that cover the source columns of the tile's destination rows, with a
 *               pitch of the tile row, one granule and ONE DWORD of padding: 21 dwords for u8, 37 for u16, odd, so that the
 *               column-wise dword reads of a half wave (ds_read_b32: 32 banks, 32 lanes at a time) fall on 32 different banks —
 *               at row i of its blocks a half wave reads dword (G bx + i) pitch + by for BXH columns bx of blocks and 32 / BXH
 *               consecutive by: u8 two bx (16 * 21 = 16 mod 32) by sixteen, u16 four bx (8 * 37 = 8 mod 32) by eight;
 *   2. turn     each lane takes a block of one destination granule (16 / 8 LDS rows) by one source dword (4 / 2 destination rows):
 *               per LDS row the two dwords that cover its source columns, funnel-shifted into one (the shift is the same for the
 *               whole tile), then 4 x 4 bytes (u8) or 2 x 2 halves (u16) transposed in registers with v_perm_b32, and one
 *               16-byte store per destination row — a store instruction of the wave writes whole tile rows, 64 or 128 bytes;
 *               VFLIP picks the transposed dwords in reverse order.  A block that reaches below the image's last row takes its
 *               samples one by one out of LDS, clamped.
 * The granules of the run's next tile are loaded into registers before the current one is turned, so that the wave has loads in
 * flight while it works in LDS; the run is 2 x 2 so that one workgroup reads both halves of the source's 128-byte lines and writes
 * both halves of the destination's where a tile row of u8 samples is 64 bytes.
 * No second pass, no LDS image of the destination.  Templates on the stored sample type; the orientation is a uniform branch.
 */
#include <algorithm>
#include "pics_common.h"

namespace {

constexpr int TILE = OH_OR_TILE, SEG = OH_OR_SEG, TILE_THREADS = 64;
constexpr int OR_RUN_X = 2, OR_RUN_Y = 2;                       /* tiles across and down that one workgroup of the transposing kernel makes, one after the other */

/* the low dword of hi:lo shifted down by sh bits (0, 8, 16 or 24) */
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int sh)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

/* the samples of a dword in reverse order */
template <typename T>
__device__ __forceinline__ uint32_t reversed(uint32_t v)
{
    if constexpr (sizeof(T) == 1)
        return __builtin_amdgcn_perm(0, v, 0x00010203);
    else
        return __builtin_amdgcn_perm(0, v, 0x01000302);
}

template <typename T>
__global__ __launch_bounds__(THREADS) void orient_rows_kernel(const OhOrArgs a)
{
    constexpr int SZ = (int)sizeof(T), GS = 16 / SZ;
    extern __shared__ __attribute__((aligned(16))) uint8_t in_l[];             /* the staged samples: SEG * SZ + 64 bytes */
    const int pic = blockIdx.z;
    int c, q;
    const int Y = grid_row(blockIdx.y, a.dh, c, q);
    const bool hf = a.orientation & OH_ORIENT_HFLIP, vf = a.orientation & OH_ORIENT_VFLIP;
    const int Wi = a.ws[q], Hi = a.hs[q];
    const int pw = (a.dw[q] + GS - 1) & ~(GS - 1);                              /* with the rest of the last granule */
    const int X0 = blockIdx.x * SEG;
    if (X0 >= pw)
        return;
    const int cnt = min(SEG, pw - X0);
    const int yi = min(Y, Hi - 1), ys = vf ? Hi - 1 - yi : yi;
    const int xa = min(X0, Wi - 1), xb = min(X0 + cnt - 1, Wi - 1);             /* the image columns of the segment */
    const int lo = hf ? Wi - 1 - xb : xa, hi = hf ? Wi - 1 - xa : xb;           /* the window columns they read */
    const int base = stage<T>(in_l, (const uint8_t *)a.src[pic][c] + (size_t)(a.y0[q] + ys) * a.spitch[c] + (size_t)(a.x0[q] + lo) * SZ, hi - lo + 1);
    __syncthreads();
    const uintptr_t dst = (uintptr_t)a.dst[pic][c] + (size_t)Y * a.dpitch[c] + (size_t)X0 * SZ;
    const uint32_t *in_w = (const uint32_t *)in_l;
    const T *in_s = (const T *)in_l;
    for (int g = threadIdx.x; g < cnt / GS; g += THREADS) {
        const int X = X0 + g * GS;
        uint4v v;
        if (X + GS <= Wi) {                                     /* 16 source bytes in a row: window columns cf .. cf + GS - 1 */
            const int cf = hf ? Wi - GS - X : X;
            const int b = (base + cf - lo) * SZ, d = b >> 2, sh = (b & 3) * 8;
            uint32_t w[5];
#pragma unroll
            for (int k = 0; k < 5; k++)
                w[k] = in_w[d + k];
#pragma unroll
            for (int k = 0; k < 4; k++)
                v[k] = funnel(w[k], w[k + 1], sh);
            if (hf)
                v = uint4v{ reversed<T>(v[3]), reversed<T>(v[2]), reversed<T>(v[1]), reversed<T>(v[0]) };
        } else {                                                /* behind the image's last column */
            Samples<T> o;
#pragma unroll
            for (int k = 0; k < GS; k++) {
                const int xi = min(X + k, Wi - 1);
                o.s[k] = in_s[base + (hf ? Wi - 1 - xi : xi) - lo];
            }
            v = o.granule();
        }
        *(GLOBAL uint4v *)(dst + 16 * (uintptr_t)g) = v;
    }
}

/* one tile of destination samples and the granules of source rows it stages: LDS row j holds the window row that destination column
 * X0 + j reads, as the ng aligned granules from row0 on that cover window columns cmin and up (cmin lies base bytes into the first) */
template <typename T, int NG>
struct Tile {
    uintptr_t row0;                                             /* the first granule of window row 0 */
    int X0, Y0, nj;                                             /* nj destination columns: whole granules */
    int cmin, base, ng;

    __device__ __forceinline__ Tile(const OhOrArgs &a, int pic, int c, int q, int X0_, int Y0_) : X0(X0_), Y0(Y0_)
    {
        constexpr int SZ = (int)sizeof(T), G = 16 / SZ;
        const bool vf = a.orientation & OH_ORIENT_VFLIP;
        const int Ws = a.ws[q], Hi = Ws;
        nj = min(TILE, ((a.dw[q] + G - 1) & ~(G - 1)) - X0);
        /* the window columns that the tile's destination rows read */
        const int yia = min(Y0, Hi - 1), yib = min(min(Y0 + TILE, a.dh[q]) - 1, Hi - 1);
        cmin = vf ? Ws - 1 - yib : yia;
        const int cmax = vf ? Ws - 1 - yia : yib;
        const uintptr_t plane = (uintptr_t)a.src[pic][c] + (size_t)a.y0[q] * a.spitch[c];
        const uintptr_t bs = plane + (size_t)(a.x0[q] + cmin) * SZ, be = plane + (size_t)(a.x0[q] + cmax + 1) * SZ;
        base = (int)(bs & 15);
        row0 = bs & ~(uintptr_t)15;
        ng = (int)((((be + 15) & ~(uintptr_t)15) - row0) >> 4);
    }

    /* the granules this lane stages: granule g = idx % NG of LDS row j = idx / NG, idx = lane + 64 it */
    __device__ __forceinline__ void load(uint4v (&t)[NG], int pitch, int Wi, bool hf) const
    {
#pragma unroll
        for (int it = 0; it < NG; it++) {
            const int idx = (int)threadIdx.x + TILE_THREADS * it, j = idx / NG, g = idx % NG;
            if (j < nj && g < ng) {
                const int xi = min(X0 + j, Wi - 1), r = hf ? Wi - 1 - xi : xi;
                t[it] = *(const GLOBAL uint4v *)(row0 + (size_t)r * pitch + 16 * (uintptr_t)g);
            }
        }
    }
};

template <typename T>
__global__ __launch_bounds__(TILE_THREADS, sizeof(T) == 1 ? 6 : 4) void orient_tile_kernel(const OhOrArgs a)
{
    constexpr int SZ = (int)sizeof(T);
    constexpr int G = 16 / SZ, R = 4 / SZ;                      /* a block: G LDS rows (one destination granule) by R source columns (one dword) */
    constexpr int NBX = TILE / G, NBY = TILE / R;
    constexpr int BXH = NBX / 2, BYL = 32 / BXH;                /* a half wave's blocks: BXH across, BYL down */
    constexpr int NG = TILE * SZ / 16 + 1;                      /* most granules of a staged row */
    constexpr int PD = (TILE * SZ + 16 + 4) / 4;                /* dwords between LDS rows: odd */
    static_assert(PD % 2 == 1 && TILE % G == 0 && TILE * NG % TILE_THREADS == 0 && NBY % BYL == 0, "the banking and the loops count on it");
    static_assert((G * PD * BXH) % 32 == 0 && (G * PD) % BYL == 0 && (G * PD / BYL) % 2 == 1, "a half wave's column reads fall on 32 different banks");
    __shared__ __attribute__((aligned(16))) uint32_t tile_l[TILE * PD + 4];
    const int pic = blockIdx.z, l = threadIdx.x;
    int c, q;
    const int per[2] = { (a.dh[0] + TILE * OR_RUN_Y - 1) / (TILE * OR_RUN_Y), (a.dh[1] + TILE * OR_RUN_Y - 1) / (TILE * OR_RUN_Y) };
    const int ty0 = grid_row(blockIdx.y, per, c, q) * OR_RUN_Y, tx0 = blockIdx.x * OR_RUN_X;
    const bool hf = a.orientation & OH_ORIENT_HFLIP, vf = a.orientation & OH_ORIENT_VFLIP;
    const int Ws = a.ws[q], Hs = a.hs[q], Wi = Hs, Hi = Ws, dh = a.dh[q];
    const int pw = (a.dw[q] + G - 1) & ~(G - 1);
    if (tx0 * TILE >= pw)
        return;
    /* the run: vx tiles across by vy down, row by row */
    const int vx = min(OR_RUN_X, (pw + TILE - 1) / TILE - tx0), n_tiles = vx * min(OR_RUN_Y, (dh + TILE - 1) / TILE - ty0);
    /* this lane's blocks: column bx of the tile's granules, rows by = byl, byl + BYL, ... of its dword rows */
    const int bx = (l >> 5) * BXH + (l & 31) / BYL, byl = l % BYL;
    uint4v t[NG];
    Tile<T, NG> nx(a, pic, c, q, tx0 * TILE, ty0 * TILE);
    nx.load(t, a.spitch[c], Wi, hf);
    for (int k = 0; k < n_tiles; k++) {
        const Tile<T, NG> tl = nx;
        const int X0 = tl.X0, Y0 = tl.Y0, nj = tl.nj, cmin = tl.cmin, base = tl.base;
#pragma unroll
        for (int it = 0; it < NG; it++) {
            const int idx = l + TILE_THREADS * it, j = idx / NG, g = idx % NG;
            if (j < nj && g < tl.ng) {
#pragma unroll
                for (int w = 0; w < 4; w++)
                    tile_l[j * PD + 4 * g + w] = t[it][w];
            }
        }
        __syncthreads();
        if (k + 1 < n_tiles) {                                  /* the next tile's granules are on their way while this one is turned */
            nx = Tile<T, NG>(a, pic, c, q, (tx0 + (k + 1) % vx) * TILE, (ty0 + (k + 1) / vx) * TILE);
            nx.load(t, a.spitch[c], Wi, hf);
        }
        const uint32_t *rows = tile_l + G * bx * PD;
        for (int by = byl; by < NBY; by += BYL) {
            const int yb = Y0 + R * by;
            if (G * bx >= nj || yb >= dh)
                break;
            const uintptr_t dst = (uintptr_t)a.dst[pic][c] + (size_t)yb * a.dpitch[c] + (size_t)(X0 + G * bx) * SZ;
            if (yb + R <= Hi) {                                 /* R destination rows inside the image: R source columns in a row */
                const int c0 = vf ? Ws - R - yb : yb;
                const int off = base + (c0 - cmin) * SZ, d = off >> 2, sh = (off & 3) * 8;
                uint32_t r[G];
#pragma unroll
                for (int i = 0; i < G; i++)
                    r[i] = funnel(rows[i * PD + d], rows[i * PD + d + 1], sh);
                uint4v o[R];                                    /* o[k]: source column c0 + k of the G LDS rows */
                if constexpr (SZ == 1) {
#pragma unroll
                    for (int k4 = 0; k4 < 4; k4++) {
                        const uint32_t p = __builtin_amdgcn_perm(r[4 * k4 + 1], r[4 * k4], 0x06020400), s = __builtin_amdgcn_perm(r[4 * k4 + 1], r[4 * k4], 0x07030501);
                        const uint32_t u = __builtin_amdgcn_perm(r[4 * k4 + 3], r[4 * k4 + 2], 0x06020400), w = __builtin_amdgcn_perm(r[4 * k4 + 3], r[4 * k4 + 2], 0x07030501);
                        o[0][k4] = __builtin_amdgcn_perm(u, p, 0x05040100);
                        o[1][k4] = __builtin_amdgcn_perm(w, s, 0x05040100);
                        o[2][k4] = __builtin_amdgcn_perm(u, p, 0x07060302);
                        o[3][k4] = __builtin_amdgcn_perm(w, s, 0x07060302);
                    }
                } else {
#pragma unroll
                    for (int k4 = 0; k4 < 4; k4++) {
                        o[0][k4] = __builtin_amdgcn_perm(r[2 * k4 + 1], r[2 * k4], 0x05040100);
                        o[1][k4] = __builtin_amdgcn_perm(r[2 * k4 + 1], r[2 * k4], 0x07060302);
                    }
                }
#pragma unroll
                for (int m = 0; m < R; m++)
                    *(GLOBAL uint4v *)(dst + (size_t)m * a.dpitch[c]) = vf ? o[R - 1 - m] : o[m];
            } else {                                            /* below the image's last row */
                const T *rows_s = (const T *)rows;
                for (int m = 0; m < R && yb + m < dh; m++) {
                    const int yi = min(yb + m, Hi - 1), at = (base >> (SZ - 1)) + (vf ? Ws - 1 - yi : yi) - cmin;
                    Samples<T> o;
#pragma unroll
                    for (int i = 0; i < G; i++)
                        o.s[i] = rows_s[i * (PD * 4 / SZ) + at];
                    *(GLOBAL uint4v *)(dst + (size_t)m * a.dpitch[c]) = o.granule();
                }
            }
        }
        __syncthreads();                                        /* the next tile overwrites the staged rows */
    }
}

template <typename T>
void launch(const OhOrArgs *a, int n, hipStream_t st)
{
    const int G = 16 / (int)sizeof(T), cls = a->np > 1 ? 2 : 1;
    int pw = 0;
    for (int q = 0; q < cls; q++)
        pw = std::max(pw, (a->dw[q] + G - 1) / G * G);
    if (a->orientation & OH_ORIENT_TRANSPOSE) {
        int rows = 0;
        for (int q = 0; q < cls; q++)
            rows += (q ? 2 : 1) * ((a->dh[q] + TILE * OR_RUN_Y - 1) / (TILE * OR_RUN_Y));
        const dim3 grid((unsigned)((pw + TILE * OR_RUN_X - 1) / (TILE * OR_RUN_X)), (unsigned)rows, (unsigned)n);
        orient_tile_kernel<T><<<grid, TILE_THREADS, 0, st>>>(*a);
    } else {
        const dim3 grid((unsigned)((pw + SEG - 1) / SEG), (unsigned)(a->dh[0] + (cls > 1 ? 2 * a->dh[1] : 0)), (unsigned)n);
        orient_rows_kernel<T><<<grid, THREADS, (size_t)SEG * sizeof(T) + 64, st>>>(*a);
    }
}

} // namespace

static_assert(OH_OR_TILE == 64, "one wave per tile: a tile row of LDS per lane of the staging loop");
static_assert(OH_OR_SEG % 16 == 0, "a segment is whole 16-byte granules of either sample type");

extern "C" void ohk_orient(const OhOrArgs *a, int n, hipStream_t st)
{
    if (a->bd == 8) launch<uint8_t>(a, n, st);
    else            launch<uint16_t>(a, n, st);
}
