/*
 * resize.hip — finished pictures -> resized engine pictures (oh_pics_resize; the exact definition is in DESIGN.md §3c and
 * tests/resize_model.py).
 *
 * Two kernels over an int16 intermediate of (window rows) x (image columns) in engine-owned HBM, then the replicated padding:
 *   1. resize_h   a workgroup (256 lanes) takes `segw` image columns x `rpw` source rows of one plane: the source columns those image
 *                 columns read go to LDS as whole 16-byte granules (as in convert.hip: plane rows are padded to 256 bytes), a lane owns
 *                 one image column and walks its taps as QUADS of source columns aligned to four plane columns: one 8-byte coefficient
 *                 read (the table is [quad][column]: neighbouring lanes read neighbouring entries) serves four rows, each with one
 *                 aligned LDS read and two v_dot2_i32_i16.  The host picks segw and rpw so that the rows fit OH_RESIZE_LDS whatever
 *                 the ratio; narrow segments put several row groups side by side so that all 256 lanes work.
 *   2. resize_v   a workgroup (128 lanes) takes 256 image columns x OH_RESIZE_VROWS image rows: a lane owns two neighbouring columns
 *                 (one dword of the intermediate per row) and walks the intermediate rows the group reads in PAIRS, one v_dot2_i32_i16
 *                 per image row and column; the group's coefficients are a dense [pair][image row] table, zero where an image row has no
 *                 tap on a row, addressed by the workgroup only (scalar loads).
 *   3. resize_pad the coded planes outside the image replicate its last column and last row.
 * Every source sample of the window is read once from HBM; the intermediate is written once and read once per row group that needs
 * the row.  Grids are (segments, workgroup rows of all planes, pictures of the launch set): the launches do not grow with the pictures.
 */
#include "../../include/ohevc_hip.h"
#include "kernels_common.h"

namespace {

constexpr int H_THREADS = 256, V_THREADS = 128, V_COLS = 2 * V_THREADS, VR = OH_RESIZE_VROWS, RPT = 4;

typedef short short2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int dot2(unsigned a, unsigned b, int c)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), c, false);
}

/* four consecutive samples in LDS as one aligned read -> two dwords of 16-bit pairs */
template <typename TI> struct Quad { typedef uint32_t T; };
template <> struct Quad<uint16_t> { typedef uint2v T; };
__device__ __forceinline__ uint2v pairs(uint32_t w) { return uint2v{ __builtin_amdgcn_perm(0, w, 0x0c010c00), __builtin_amdgcn_perm(0, w, 0x0c030c02) }; }
__device__ __forceinline__ uint2v pairs(uint2v w) { return w; }

/* blockIdx.y -> plane c and the workgroup row g inside it, for `per[class]` workgroup rows per plane; false: past the last plane */
__device__ __forceinline__ bool plane_of(int y, int np, int g0, int g1, int *c, int *g)
{
    if (y < g0) { *c = 0; *g = y; return true; }
    y -= g0;
    if (np == 1 || y >= 2 * g1) return false;
    *c = 1 + (y >= g1); *g = y - (*c - 1) * g1;
    return true;
}

template <typename TI>
__global__ __launch_bounds__(H_THREADS) void resize_h_kernel(const OhResizeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];      /* rpw x row_bytes of the larger class, at most OH_RESIZE_LDS */
    int c, g;
    if (!plane_of(blockIdx.y, a.np, a.k[0].h_groups, a.k[1].h_groups, &c, &g))
        return;
    const OhResizeClass &k = a.k[c != 0];
    const int x_seg = blockIdx.x * k.segw;
    if (x_seg >= k.tw)
        return;
    const int pic = blockIdx.z, t = threadIdx.x;
    const int x_last = min(x_seg + k.segw, k.tw) - 1;
    const int s0 = G_CONST(int32_t, k.h_first)[x_seg];
    const int span = G_CONST(int32_t, k.h_first)[x_last] + G_CONST(int32_t, k.h_cnt)[x_last] - s0;
    const int r0 = g * k.rpw, rows = min(k.rpw, k.sh - r0);
    const uint8_t *src = (const uint8_t *)a.src[pic][c] + (size_t)(k.y0 + r0) * k.src_pitch + (size_t)(k.x0 + s0) * sizeof(TI);
    /* the granules of one row after the other; every row starts at the same address modulo 16 (the pitch is a multiple of 256) */
    const uintptr_t sa = (uintptr_t)src, ga = sa & ~(uintptr_t)15;
    const int b = (int)((sa - ga) / sizeof(TI)), gr = (int)(((sa + (uintptr_t)span * sizeof(TI) + 15) & ~(uintptr_t)15) - ga) >> 4;
    /* this lane's image column: its taps are asked for before the rows, so that the two waits overlap.  The quads start at a multiple
     * of four plane columns and the staged granules at a multiple of eight or sixteen: every quad is one aligned LDS read */
    const int nrg = H_THREADS / k.segw, xl = t % k.segw, rg = t / k.segw, x = min(x_seg + xl, x_last);    /* segw divides 256 */
    const int f = G_CONST(int32_t, k.h_f4)[x] - s0 + b, n = G_CONST(int32_t, k.h_n4)[x];
    for (int i = t; i < rows * gr; i += H_THREADS) {
        const int r = i / gr, q = i - r * gr;
        *(uint4v *)(lds + r * k.row_bytes + 16 * q) = *(const GLOBAL uint4v *)(ga + (size_t)r * k.src_pitch + 16 * (uintptr_t)q);
    }
    __syncthreads();
    if (x_seg + xl > x_last)
        return;
    const GLOBAL uint2v *kp = (const GLOBAL uint2v *)k.h_k + x;
    const int bd = a.bd, rnd = 1 << (bd - 1);
    int16_t *mid = a.mid + pic * a.mid_pic + a.mid_plane[c] + (size_t)r0 * k.mid_stride + x;
    typedef typename Quad<TI>::T QT;
    for (int rq = rg; rq < rows; rq += RPT * nrg) {            /* rows rq, rq + nrg, ...: each coefficient quad is read once for RPT rows */
        const QT *row[RPT];
        int acc[RPT];
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            row[q] = (const QT *)(lds + min(rq + q * nrg, rows - 1) * k.row_bytes + f * (int)sizeof(TI));   /* a row past the last repeats it, not stored */
            acc[q] = 0;
        }
        for (int j = 0; j < n; j++) {
            const uint2v kj = kp[(size_t)j * k.h_stride];
#pragma unroll
            for (int q = 0; q < RPT; q++) {
                const uint2v s = pairs(row[q][j]);
                acc[q] = dot2(s[1], kj[1], dot2(s[0], kj[0], acc[q]));
            }
        }
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            const int r = rq + q * nrg;
            if (r < rows)
                G_MUT(int16_t, mid)[(size_t)r * k.mid_stride] = (int16_t)((acc[q] + rnd) >> bd);
        }
    }
}

template <typename TO>
__global__ __launch_bounds__(V_THREADS) void resize_v_kernel(const OhResizeArgs a)
{
    int c, g;
    if (!plane_of(blockIdx.y, a.np, a.k[0].v_groups, a.k[1].v_groups, &c, &g))
        return;
    const OhResizeClass &k = a.k[c != 0];
    const int x = blockIdx.x * V_COLS + 2 * threadIdx.x;
    if (x >= k.tw)
        return;
    const int pic = blockIdx.z;
    const int lo = G_CONST(int32_t, k.v_first)[g], np = G_CONST(int32_t, k.v_cnt)[g];
    const GLOBAL uint4v *kk = (const GLOBAL uint4v *)(G_CONST(int32_t, k.v_k) + (size_t)G_CONST(int32_t, k.v_off)[g] * VR);
    /* mid_stride is even and x is even: one dword holds this lane's two columns of a row */
    const GLOBAL uint32_t *m = (const GLOBAL uint32_t *)(a.mid + pic * a.mid_pic + a.mid_plane[c] + (size_t)lo * k.mid_stride + x);
    const size_t ms = (size_t)k.mid_stride / 2;
    int acc0[VR], acc1[VR];
#pragma unroll
    for (int i = 0; i < VR; i++) acc0[i] = acc1[i] = 0;
    for (int p = 0; p < np; p++) {
        const uint32_t e = m[0], o = m[ms];                    /* rows lo + 2p and lo + 2p + 1 (the plane has a spare row past its last) */
        m += 2 * ms;
        const uint32_t p0 = (e & 0xffffu) | (o << 16), p1 = (e >> 16) | (o & 0xffff0000u);
        const uint4v ka = kk[2 * p], kb = kk[2 * p + 1];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            acc0[i] = dot2(p0, ka[i], acc0[i]);         acc1[i] = dot2(p1, ka[i], acc1[i]);
            acc0[4 + i] = dot2(p0, kb[i], acc0[4 + i]); acc1[4 + i] = dot2(p1, kb[i], acc1[4 + i]);
        }
    }
    const int bd = a.bd, sh = 28 - bd, rnd = 1 << (sh - 1), mx = (1 << bd) - 1;
    const bool two = x + 1 < k.tw;
    uint8_t *dst = (uint8_t *)a.dst[pic][c] + (size_t)(g * VR) * k.dst_pitch + (size_t)x * sizeof(TO);
#pragma unroll
    for (int i = 0; i < VR; i++) {
        if (g * VR + i >= k.th)
            break;
        const int v0 = min(max((acc0[i] + rnd) >> sh, 0), mx), v1 = min(max((acc1[i] + rnd) >> sh, 0), mx);
        GLOBAL TO *q = G_MUT(TO, dst + (size_t)i * k.dst_pitch);
        if (!two)
            q[0] = (TO)v0;
        else if constexpr (sizeof(TO) == 1)
            *(GLOBAL uint16_t *)q = (uint16_t)(v0 | (v1 << 8));
        else
            *(GLOBAL uint32_t *)q = (uint32_t)v0 | ((uint32_t)v1 << 16);
    }
}

/* coded samples outside the image: the image's sample of the same row in its last column / of its last row */
template <typename TO>
__global__ __launch_bounds__(256) void resize_pad_kernel(const OhResizeArgs a)
{
    const int h0 = a.k[0].ch, h1 = a.k[1].ch;
    int c, y;
    if (!plane_of(blockIdx.y, a.np, h0, h1, &c, &y))
        return;
    const OhResizeClass &k = a.k[c != 0];
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= k.cw || (x < k.tw && y < k.th))
        return;
    uint8_t *pl = (uint8_t *)a.dst[blockIdx.z][c];
    G_MUT(TO, pl + (size_t)y * k.dst_pitch)[x] = G_CONST(TO, pl + (size_t)min(y, k.th - 1) * k.dst_pitch)[min(x, k.tw - 1)];
}

template <typename T>
void launch(const OhResizeArgs *a, int n, int pad, hipStream_t st)
{
    const int nc = a->np == 3 ? 2 : 0;
    const OhResizeClass &l = a->k[0], &c = a->k[1];
    const int hx = max((l.tw + l.segw - 1) / l.segw, nc ? (c.tw + c.segw - 1) / c.segw : 0);
    const int vx = (max(l.tw, nc ? c.tw : 0) + V_COLS - 1) / V_COLS;
    const size_t lds = (size_t)max(l.rpw * l.row_bytes, nc ? c.rpw * c.row_bytes : 0);
    resize_h_kernel<T><<<dim3((unsigned)hx, (unsigned)(l.h_groups + nc * c.h_groups), (unsigned)n), H_THREADS, lds, st>>>(*a);
    resize_v_kernel<T><<<dim3((unsigned)vx, (unsigned)(l.v_groups + nc * c.v_groups), (unsigned)n), V_THREADS, 0, st>>>(*a);
    if (pad)
        resize_pad_kernel<T><<<dim3((unsigned)((l.cw + 255) / 256), (unsigned)(l.ch + nc * c.ch), (unsigned)n), 256, 0, st>>>(*a);
}

} // namespace

static_assert(sizeof(OhResizeArgs) <= 4096, "kernel arguments");

extern "C" void ohk_resize(const OhResizeArgs *a, int n, int pad, hipStream_t st)
{
    if (a->bd > 8)
        launch<uint16_t>(a, n, pad, st);
    else
        launch<uint8_t>(a, n, pad, st);
}
