/*
 * motion.hip — block-matching motion search between finished pictures and the motion-compensated prediction of a field
 * (oh_pics_motion, oh_pics_motion_compensate; the exact definitions are in DESIGN.md §3o and tests/motion_model.py; the sample formulas,
 * the cost and the key are motion_common.h, shared with the host).
 *
 * Both kernels give one wave64 (a workgroup of 64 lanes) to one block of one picture; grid (blocks across, blocks down, pictures of the
 * launch — all of them share one geometry; their plane addresses are in the kernel arguments).  Centres differ per block, so the
 * reference window is per block and not per tile.
 *
 * Search.  The block's current samples (rows of 16) and its reference window go into LDS: the columns x0 + cx - rx - 4 .. x0 + cx + w - 1
 * + rx + 4 and the rows likewise, where 4 = OH_MO_REACH is what the last sub-sample stage can reach beyond the integer range (three
 * quarters further, so one whole sample before with the filter's three in front of it, and the filter's four behind).  Rows and columns
 * are clamped while staging, sample by sample (a centre may point wholly outside the plane), so LDS holds HEVC's padded reference and
 * the stages below never look at an edge.
 * A stage is a list of candidates.  An item is one candidate's rows part * rows .. (part + 1) * rows - 1, with P parts per candidate, a
 * power of two chosen so that few candidates still fill the wave (range 0: one candidate, sixteen lanes, a row each); the items are
 * dealt to the lanes in order, 64 at a time, the P partial SADs of a candidate, which sit in neighbouring lanes, are added with
 * xor-shuffles, and every lane keeps the smallest key it has seen.  An integer candidate takes its SAD four bytes at a time with the
 * ISA's packed absolute-difference-and-accumulate (v_sad_u8 at 8 bit, v_sad_u16 above); consecutive lanes hold consecutive
 * displacements, so their window reads are consecutive LDS addresses, and the current samples are one address for all of them, a
 * broadcast.  A fractional candidate evaluates motion_sample per sample from the same window.  The wave's smallest key is a
 * butterfly of shuffles; the key orders totally (motion_common.h: motion_key), so neither the dealing nor the butterfly's order can
 * change the winner.  Stage 1 and 2 run from the winner so far, which every lane holds after the butterfly.
 *
 * Compensation.  Per plane the block's window of (w + taps - 1) x (h + taps - 1) reference samples is staged, clamped, and an item is a
 * run of eight samples of a row (four where a chroma block is four wide), stored as one aligned access of 4, 8 or 16 bytes.
 * Templates on the stored sample type.
 */
#include <algorithm>
#include "pics_common.h"
#include "motion_common.h"

namespace {

constexpr int MT = 64;                            /* lanes of a workgroup: one wave */
constexpr int REACH = OH_MO_REACH;
constexpr int CUR_PITCH = 16;                     /* samples between the rows of the staged current block */
constexpr int CMP_PITCH = 24;                     /* samples between the rows of a compensation window: 16 + 7, rounded up */

/* samples between the rows of a search window: what it holds, in whole dwords */
__host__ __device__ constexpr int win_pitch(int block, int rx) { return (block + 2 * rx + 2 * REACH + 3) & ~3; }
template <typename T> constexpr size_t search_lds(int block, int rx, int ry)
{
    return sizeof(T) * (size_t)(16 * CUR_PITCH + win_pitch(block, rx) * (block + 2 * ry + 2 * REACH));
}

__device__ __forceinline__ uint32_t lds_dword(const LDS void *p)
{
    uint32_t v;
    __builtin_memcpy(&v, (const LDS uint8_t *)p, 4);            /* any sample address */
    return v;
}

/* the SAD of `rows` rows of w samples (a multiple of 8): c the current ones (dword aligned), r the reference ones */
template <typename T>
__device__ __forceinline__ uint32_t sad_rows(const LDS T *c, const LDS T *r, int rpitch, int w, int rows)
{
    constexpr int PER = 4 / (int)sizeof(T);                     /* samples of a dword */
    uint32_t sad = 0;
    for (int y = 0; y < rows; y++) {
        for (int x = 0; x < w; x += PER) {
            const uint32_t cv = *(const LDS uint32_t *)(c + y * CUR_PITCH + x), rv = lds_dword(r + y * rpitch + x);
            sad = sizeof(T) == 1 ? __builtin_amdgcn_sad_u8(cv, rv, sad) : __builtin_amdgcn_sad_u16(cv, rv, sad);
        }
    }
    return sad;
}

/* the same against the prediction with the fractions (fx, fy), not both zero: r the reference sample at (xInt, yInt) of the first row */
template <typename T>
__device__ __forceinline__ uint32_t sad_rows_frac(const LDS T *c, const LDS T *r, int rpitch, int w, int rows, int fx, int fy, int bd)
{
    uint32_t sad = 0;
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < w; x++)
            sad += (uint32_t)motion_abs((int32_t)c[y * CUR_PITCH + x] - motion_sample<8>(r + (y - 3) * rpitch + x - 3, rpitch, fx, fy, bd));
    return sad;
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v)
{
#pragma unroll
    for (int s = 1; s < MT; s <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, s), hi = __shfl_xor((uint32_t)(v >> 32), s);
        const uint64_t o = (uint64_t)hi << 32 | lo;
        v = o < v ? o : v;
    }
    return v;
}

struct Block {                                    /* what the stages share */
    int w, h, bd, lambda;
    int ox, oy;                                   /* where the sample of the block's first one, displaced by the centre, sits in the window */
    int wp;                                       /* samples between the window's rows */
};

/* one stage: ncand candidates, candidate k at the distance at(k, dx, dy) (quarter samples) from four times the centre.  Returns the
 * smallest key, in every lane; centre_sad: the SAD of the candidate at distance zero, if the stage has one, else 0 */
template <typename T, typename F>
__device__ __forceinline__ uint64_t run_stage(const Block &b, const LDS T *cur, const LDS T *win, int ncand, F at, uint32_t *centre_sad)
{
    const int lane = threadIdx.x;
    int P = 1;
    while (P < b.h && ncand * P < MT)
        P <<= 1;
    const int rows = b.h / P, items = ncand * P;
    uint64_t best = ~(uint64_t)0;
    uint32_t csad = 0;
    for (int i0 = 0; i0 < items; i0 += MT) {                    /* the same trips for every lane: the shuffles below need them all */
        const int i = i0 + lane;
        const bool on = i < items;
        const int k = on ? i / P : 0, part = i & (P - 1);
        int dx, dy;
        at(k, dx, dy);
        uint32_t sad = 0;
        if (on) {
            const LDS T *c = cur + part * rows * CUR_PITCH;
            const LDS T *r = win + (b.oy + (dy >> 2) + part * rows) * b.wp + b.ox + (dx >> 2);
            sad = (dx & 3) | (dy & 3) ? sad_rows_frac<T>(c, r, b.wp, b.w, rows, dx & 3, dy & 3, b.bd) : sad_rows<T>(c, r, b.wp, b.w, rows);
        }
        for (int s = 1; s < P; s <<= 1)                         /* the parts of a candidate: P neighbouring lanes, all on or all off */
            sad += __shfl_xor(sad, s);
        if (on) {
            const uint64_t key = motion_key(motion_cost(sad, motion_dist(dx, dy), b.lambda), dx, dy);
            best = key < best ? key : best;
            if (!(dx | dy))
                csad = sad;
        }
    }
    if (centre_sad) {
#pragma unroll
        for (int s = 1; s < MT; s <<= 1)
            csad = max(csad, (uint32_t)__shfl_xor(csad, s));
        *centre_sad = csad;
    }
    return wave_min(best);
}

template <typename T>
__global__ __launch_bounds__(MT) void motion_search_kernel(const OhMoSearchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_g[];
    LDS T *cur = (LDS T *)lds_g, *win = cur + 16 * CUR_PITCH;
    const int lane = threadIdx.x, pair = blockIdx.z;
    const int B = a.block, x0 = blockIdx.x * B, y0 = blockIdx.y * B;
    const size_t at_blk = ((size_t)pair * a.bh + blockIdx.y) * a.bw + blockIdx.x;
    int cx = 0, cy = 0;
    if (a.centres) {
        const uint32_t c = *(const GLOBAL uint32_t *)(a.centres + at_blk);
        cx = (int16_t)(c & 0xffff); cy = (int16_t)(c >> 16);
    }
    Block b;
    b.w = min(B, a.w - x0); b.h = min(B, a.h - y0); b.bd = a.bd; b.lambda = a.lambda;
    b.wp = win_pitch(B, a.rx);
    b.ox = a.rx + REACH; b.oy = a.ry + REACH;
    const size_t pitch = (size_t)a.pitch;
    const uintptr_t C = (uintptr_t)a.cur[pair], R = (uintptr_t)a.ref[pair];
    for (int i = lane; i < b.w * b.h; i += MT) {
        const int r = i / b.w, c = i - r * b.w;
        cur[r * CUR_PITCH + c] = *(const GLOBAL T *)(C + (size_t)(y0 + r) * pitch + sizeof(T) * (size_t)(x0 + c));
    }
    const int wc = b.w + 2 * b.ox, wr = b.h + 2 * b.oy;        /* staged columns and rows: wc <= wp */
    const int wx0 = x0 + cx - b.ox, wy0 = y0 + cy - b.oy;
    for (int i = lane; i < wc * wr; i += MT) {
        const int r = i / wc, c = i - r * wc;
        const int y = min(max(wy0 + r, 0), a.h - 1), x = min(max(wx0 + c, 0), a.w - 1);
        win[r * b.wp + c] = *(const GLOBAL T *)(R + (size_t)y * pitch + sizeof(T) * (size_t)x);
    }
    __syncthreads();

    const int nx = 2 * a.rx + 1, ny = 2 * a.ry + 1, rx = a.rx, ry = a.ry;
    uint32_t sad_centre;
    uint64_t best = run_stage<T>(b, cur, win, nx * ny, [=](int k, int &dx, int &dy) {
        const int j = k / nx;
        dx = 4 * (k - j * nx - rx); dy = 4 * (j - ry);
    }, &sad_centre);
    for (int s = 1; s <= a.subpel; s++) {
        const int step = 3 - s, bx = motion_key_dx(best), by = motion_key_dy(best);
        best = run_stage<T>(b, cur, win, 9, [=](int k, int &dx, int &dy) {
            const int j = k / 3;
            dx = bx + step * (k - 3 * j - 1); dy = by + step * (j - 1);
        }, nullptr);
    }
    if (lane == 0) {
        const int dx = motion_key_dx(best), dy = motion_key_dy(best);
        const uint32_t sad = motion_key_cost(best) - motion_cost(0, motion_dist(dx, dy), a.lambda);
        GLOBAL uint32_t *o = (GLOBAL uint32_t *)(a.res + at_blk);
        o[0] = (uint32_t)(uint16_t)(4 * cx + dx) | (uint32_t)(uint16_t)(4 * cy + dy) << 16;
        o[1] = sad;
        o[2] = sad_centre;
    }
}

/* one plane of the block: TAPS 8 luma, 4 chroma; (px, py) and pw x ph its rectangle in the plane of W x H samples, (xi, yi) the
 * reference sample of its first one, (fx, fy) the fractions */
template <typename T, int TAPS>
__device__ __forceinline__ void compensate_plane(LDS T *win, const void *ref, void *dst, size_t pitch, int W, int H, int px, int py, int pw,
                                                 int ph, int xi, int yi, int fx, int fy, int bd)
{
    constexpr int BEFORE = TAPS / 2 - 1;
    const int lane = threadIdx.x;
    const int wc = pw + TAPS - 1, wr = ph + TAPS - 1;
    const uintptr_t R = (uintptr_t)ref, D = (uintptr_t)dst;
    for (int i = lane; i < wc * wr; i += MT) {
        const int r = i / wc, c = i - r * wc;
        const int y = min(max(yi - BEFORE + r, 0), H - 1), x = min(max(xi - BEFORE + c, 0), W - 1);
        win[r * CMP_PITCH + c] = *(const GLOBAL T *)(R + (size_t)y * pitch + sizeof(T) * (size_t)x);
    }
    __syncthreads();
    const int run = min(8, pw), per_row = pw / run;             /* pw: 4, 8 or 16 */
    for (int i = lane; i < per_row * ph; i += MT) {
        const int r = i / per_row, c = (i - r * per_row) * run;
        T s[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            s[k] = k < run ? (T)motion_sample<TAPS>(win + r * CMP_PITCH + c + k, CMP_PITCH, fx, fy, bd) : (T)0;
        const uintptr_t o = D + (size_t)(py + r) * pitch + sizeof(T) * (size_t)(px + c);
        const int bytes = run * (int)sizeof(T);
        if (bytes == 16) {
            uint4v v; __builtin_memcpy(&v, s, 16);
            *(GLOBAL uint4v *)o = v;
        } else if (bytes == 8) {
            uint2v v; __builtin_memcpy(&v, s, 8);
            *(GLOBAL uint2v *)o = v;
        } else {
            uint32_t v; __builtin_memcpy(&v, s, 4);
            *(GLOBAL uint32_t *)o = v;
        }
    }
    __syncthreads();                                            /* the next plane stages into the same window */
}

template <typename T>
__global__ __launch_bounds__(MT) void motion_compensate_kernel(const OhMoCompArgs a)
{
    __shared__ __attribute__((aligned(16))) T win_s[CMP_PITCH * (16 + 7)];
    LDS T *win = (LDS T *)win_s;
    const int pic = blockIdx.z;
    const int B = a.block, x0 = blockIdx.x * B, y0 = blockIdx.y * B;
    const int w = min(B, a.w[0] - x0), h = min(B, a.h[0] - y0);
    const uint32_t v = *(const GLOBAL uint32_t *)(a.field + ((size_t)pic * a.bh + blockIdx.y) * a.bw + blockIdx.x);
    const int mvx = (int16_t)(v & 0xffff), mvy = (int16_t)(v >> 16);
    compensate_plane<T, 8>(win, a.ref[pic][0], a.dst[pic][0], (size_t)a.pitch[0], a.w[0], a.h[0], x0, y0, w, h, x0 + (mvx >> 2), y0 + (mvy >> 2),
                           mvx & 3, mvy & 3, a.bd);
    const int hs = a.hs, vs = a.vs;
    for (int c = 1; c < a.np; c++)
        compensate_plane<T, 4>(win, a.ref[pic][c], a.dst[pic][c], (size_t)a.pitch[c], a.w[1], a.h[1], x0 >> hs, y0 >> vs, w >> hs, h >> vs,
                               (x0 >> hs) + (mvx >> (2 + hs)), (y0 >> vs) + (mvy >> (2 + vs)), (mvx & ((4 << hs) - 1)) << (1 - hs),
                               (mvy & ((4 << vs) - 1)) << (1 - vs), a.bd);
}

} // namespace

static_assert(sizeof(OhMoDev) == sizeof(OhMotionVector) && sizeof(OhMoDev) == 12 && sizeof(OhMoVec) == 4, "the vectors as the kernels store and load them");
static_assert(search_lds<uint16_t>(16, OH_MOTION_MAX_RANGE, OH_MOTION_MAX_RANGE) <= 64 << 10, "LDS of one workgroup");
static_assert(4 * OH_MOTION_MAX_RANGE + 3 < 256 && 4 * OH_MOTION_MAX_CENTRE + 4 * OH_MOTION_MAX_RANGE + 3 < 32768, "the key's fields; a vector is int16");

extern "C" void ohk_motion_search(const OhMoSearchArgs *a, int n, hipStream_t st)
{
    const dim3 grid((unsigned)a->bw, (unsigned)a->bh, (unsigned)n);
    if (a->bd == 8) motion_search_kernel<uint8_t><<<grid, MT, search_lds<uint8_t>(a->block, a->rx, a->ry), st>>>(*a);
    else            motion_search_kernel<uint16_t><<<grid, MT, search_lds<uint16_t>(a->block, a->rx, a->ry), st>>>(*a);
}

extern "C" void ohk_motion_compensate(const OhMoCompArgs *a, int n, hipStream_t st)
{
    const dim3 grid((unsigned)a->bw, (unsigned)a->bh, (unsigned)n);
    if (a->bd == 8) motion_compensate_kernel<uint8_t><<<grid, MT, 0, st>>>(*a);
    else            motion_compensate_kernel<uint16_t><<<grid, MT, 0, st>>>(*a);
}
