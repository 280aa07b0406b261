/*
 * hash.hip — the two parallel forms of the decoded-picture-hash SEI (H.265 Annex D, hash_type 1 CRC and 2 checksum) of whole coded
 * planes: the plane's rows packed, one byte per sample at 8 bit, two (low byte first) above.  md5.hip has the serial form (type 0).
 *
 * A plane's packed bytes are cut into tasks of OH_HASH_TASK bytes, one workgroup (256 lanes) each, all tasks of all planes of the
 * call in ONE launch; a second, small launch combines a plane's task results and writes its value.
 *
 * Checksum: sum over bytes of (byte ^ mask(x, y)) mod 2^32 with mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8), x the sample's
 * column.  Lane sums (v_sad_u8 over masked dwords), a workgroup sum per task, the task sums added up per plane.
 *
 * CRC: the Annex D register (0xFFFF, message bits, 16 zero bits) is the direct CRC with polynomial P = x^16 + x^12 + x^5 + 1 and
 * initial value 0x1D0F: with CRC0 the direct CRC of zero initial value, CRC0(A || B) = CRC0(A) * x^(8|B|) ^ CRC0(B) (mod P), and the
 * value of an N-byte plane is 0x1D0F * x^(8N) ^ CRC0(plane).  x has order 32767 modulo P, so every power is taken with its exponent
 * reduced mod 32767 — a negative exponent is a division by x, which is how bytes beyond the end of a plane (read as zeros, CRC0 of
 * trailing zeros multiplies by x^8 each) are taken out again.
 *   - lane t of a workgroup takes the 16 bytes at 16 t of every 4096-byte block of its task: CRC0 of them is the XOR of 16 lookups
 *     in byte tables (slicing: table k holds CRC0 of a byte followed by k zero bytes) held in LDS;
 *   - the lane's blocks lie 4096 bytes apart: x^(8 * 4096) = x^32768 = x, so one shift-and-reduce per block chains them (Horner);
 *   - then x^(128 (255 - t)) moves the lane's value to the end of the task, the workgroup XORs its lanes: CRC0 of the task;
 *   - the combine launch moves each task's value to the end of the plane (powers x^(2^i)), XORs them and adds the 0x1D0F term.
 */
#include "kernels_common.h"

namespace {

constexpr int THREADS = 256, CHUNK = 16, BLOCK = THREADS * CHUNK, TASK_BLOCKS = OH_HASH_TASK / BLOCK, GROUP = 8;
static_assert(OH_HASH_TASK % (BLOCK * GROUP) == 0, "a task is whole groups of whole blocks");
constexpr uint32_t ORD = 32767;                               /* order of x modulo P */

constexpr uint32_t mulx(uint32_t a) { a <<= 1; return a & 0x10000 ? a ^ 0x11021 : a; }
constexpr uint32_t mulmod_c(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = mulx(r);
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}

struct Tables {
    uint16_t slice[16][256];                                  /* slice[k][b] = CRC0(b, then k zero bytes) = b x^(8k + 16) mod P */
    uint16_t lane[THREADS];                                   /* x^(128 (255 - t)): lane t's last chunk -> the end of its task */
    uint16_t pw[15];                                          /* x^(2^i) */
};

constexpr Tables make_tables()
{
    Tables t{};
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t c = b << 8;
        for (int i = 0; i < 8; i++) c = c & 0x8000 ? ((c << 1) ^ 0x1021) & 0xFFFF : (c << 1) & 0xFFFF;
        t.slice[0][b] = (uint16_t)c;
    }
    for (int k = 1; k < 16; k++)
        for (int b = 0; b < 256; b++) {
            const uint32_t c = t.slice[k - 1][b];
            t.slice[k][b] = (uint16_t)(((c << 8) & 0xFFFF) ^ t.slice[0][c >> 8]);
        }
    uint32_t m = 1;
    for (int l = THREADS - 1; l >= 0; l--) {
        t.lane[l] = (uint16_t)m;
        for (int i = 0; i < CHUNK; i++) m = ((m << 8) & 0xFFFF) ^ t.slice[0][m >> 8];
    }
    t.pw[0] = 2;
    for (int i = 1; i < 15; i++) t.pw[i] = (uint16_t)mulmod_c(t.pw[i - 1], t.pw[i - 1]);
    return t;
}

__device__ const Tables kTab = make_tables();

__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 15; i >= 0; i--)
        r = mulx(r) ^ (((b >> i) & 1) ? a : 0u);
    return r;
}

/* a * x^e mod P, 0 <= e < ORD */
__device__ __forceinline__ uint32_t mul_xpow(uint32_t a, uint32_t e)
{
    for (int i = 0; i < 15; i++)
        if ((e >> i) & 1) a = mulmod(a, kTab.pw[i]);
    return a;
}

/* 8 * v mod ORD for a signed byte distance v */
__device__ __forceinline__ uint32_t bits_mod(int64_t v)
{
    const int64_t r = (8 * v) % (int64_t)ORD;
    return (uint32_t)(r < 0 ? r + ORD : r);
}

/* CRC0 of the 16 bytes of w (byte 0 = low byte of w[0] first) */
__device__ __forceinline__ uint32_t chunk_crc0(const uint4v w, const uint16_t (*tab)[256])
{
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < CHUNK; i++)
        c ^= tab[CHUNK - 1 - i][(w[i >> 2] >> (8 * (i & 3))) & 0xFF];
    return c;
}

/* checksum of 16 packed bytes that start at byte column col (a multiple of 16) of row y */
__device__ __forceinline__ uint32_t chunk_checksum(const uint4v w, uint32_t col, uint32_t y, uint32_t bps, uint32_t sum)
{
    const uint32_t x0 = bps == 2 ? col >> 1 : col;            /* a multiple of 8: the 8 or 16 samples share x >> 8 */
    const uint32_t m = ((x0 & 0xFF) ^ (x0 >> 8) ^ (y & 0xFF) ^ (y >> 8)) * 0x01010101u;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        /* x & 0xFF of the dword's bytes: x0's plus 4d .. 4d + 3 (one byte per sample) or 2d, 2d, 2d + 1, 2d + 1 (two) */
        const uint32_t lo = bps == 2 ? 0x01010000u + 0x02020202u * d : 0x03020100u + 0x04040404u * d;
        sum = __builtin_amdgcn_sad_u8(w[d] ^ m ^ lo, 0, sum);
    }
    return sum;
}

template <int KIND>
__device__ __forceinline__ void hash_task(const OhMd5Job *jobs, const uint2v *task_map, uint32_t *partials, const uint16_t (*tab)[256],
                                          uint32_t *red)
{
    const int t = threadIdx.x;
    const uint2v tm = gload(task_map + blockIdx.x);          /* (job, task of the job) */
    const OhMd5Job j = gload(jobs + tm[0]);
    const uint32_t rb = j.row_bytes, bps = j.bps;
    const uint64_t o0 = (uint64_t)tm[1] * OH_HASH_TASK + (uint64_t)t * CHUNK;
    uint32_t row = (uint32_t)(o0 / rb), col = (uint32_t)(o0 - (uint64_t)row * rb);
    const uint32_t step_rows = BLOCK / rb, step_col = BLOCK % rb;
    const GLOBAL uint8_t *base = (const GLOBAL uint8_t *)j.base;
    const bool fast = ((rb | j.pitch | (uint32_t)(uintptr_t)j.base) & (CHUNK - 1)) == 0;   /* chunks are whole, aligned and inside a row */
    uint32_t acc = 0;
    for (int g = 0; g < TASK_BLOCKS; g += GROUP) {
        uint4v w[GROUP];
        uint32_t rows_[GROUP], cols_[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; k++) {                     /* the group's loads first: GROUP x 16 bytes in flight per lane */
            rows_[k] = row; cols_[k] = col;
            w[k] = uint4v{ 0, 0, 0, 0 };
            if (fast) {
                if (row < j.rows)
                    w[k] = *(const GLOBAL uint4v *)(base + (size_t)row * j.pitch + col);
            } else {
                uint32_t v[4] = { 0, 0, 0, 0 };
                for (int i = 0; i < CHUNK; i++) {             /* byte by byte: rows that are not whole chunks (or unaligned planes) */
                    uint32_t r = row, c = col + i;
                    while (c >= rb) { c -= rb; r++; }
                    if (r < j.rows) {
                        const uint32_t b = base[(size_t)r * j.pitch + c];
                        v[i >> 2] |= b << (8 * (i & 3));
                        if (KIND == 2) {
                            const uint32_t x = bps == 2 ? c >> 1 : c;
                            acc += b ^ ((x & 0xFF) ^ (r & 0xFF) ^ (x >> 8) ^ (r >> 8));
                        }
                    }
                }
                w[k] = uint4v{ v[0], v[1], v[2], v[3] };
            }
            col += step_col; row += step_rows;
            if (col >= rb) { col -= rb; row++; }
        }
#pragma unroll
        for (int k = 0; k < GROUP; k++) {
            if (KIND == 1)
                acc = mulx(acc) ^ chunk_crc0(w[k], tab);      /* x^(8 * BLOCK) = x */
            else if (fast && rows_[k] < j.rows)
                acc = chunk_checksum(w[k], cols_[k], rows_[k], bps, acc);
        }
    }
    if (KIND == 1)
        acc = mulmod(acc, kTab.lane[t]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o = __shfl_xor(acc, s, 64);
        acc = KIND == 1 ? acc ^ o : acc + o;
    }
    if ((t & 63) == 0)
        red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        uint32_t v = red[0];
        for (int i = 1; i < THREADS / 64; i++) v = KIND == 1 ? v ^ red[i] : v + red[i];
        partials[blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(THREADS) void crc_kernel(const OhMd5Job *jobs, const uint2v *task_map, uint32_t *partials)
{
    __shared__ uint16_t tab[16][256];
    __shared__ uint32_t red[THREADS / 64];
    const GLOBAL uint4v *src = (const GLOBAL uint4v *)&kTab.slice[0][0];
    uint4v *dst = (uint4v *)&tab[0][0];
    for (int i = threadIdx.x; i < (int)(sizeof(tab) / 16); i += THREADS)
        dst[i] = src[i];
    __syncthreads();
    hash_task<1>(jobs, task_map, partials, tab, red);
}

__global__ __launch_bounds__(THREADS) void checksum_kernel(const OhMd5Job *jobs, const uint2v *task_map, uint32_t *partials)
{
    __shared__ uint32_t red[THREADS / 64];
    hash_task<2>(jobs, task_map, partials, nullptr, red);
}

/* one workgroup per plane: its tasks' values -> the plane's CRC / checksum, written to out[job] (pinned host memory) */
__global__ __launch_bounds__(THREADS) void hash_combine_kernel(const OhMd5Job *jobs, const uint32_t *first, const uint32_t *partials, int kind,
                                                               uint32_t *out)
{
    __shared__ uint32_t red[THREADS / 64];
    const int t = threadIdx.x, job = blockIdx.x;
    const OhMd5Job j = gload(jobs + job);
    const int64_t n = (int64_t)j.row_bytes * j.rows;
    const uint32_t f0 = first[job], f1 = first[job + 1];
    uint32_t acc = 0;
    for (uint32_t k = t; k < f1 - f0; k += THREADS) {
        const uint32_t p = partials[f0 + k];
        if (kind == 1)
            acc ^= mul_xpow(p, bits_mod(n - (int64_t)(k + 1) * OH_HASH_TASK));
        else
            acc += p;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o = __shfl_xor(acc, s, 64);
        acc = kind == 1 ? acc ^ o : acc + o;
    }
    if ((t & 63) == 0)
        red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        uint32_t v = red[0];
        for (int i = 1; i < THREADS / 64; i++) v = kind == 1 ? v ^ red[i] : v + red[i];
        if (kind == 1)
            v ^= mul_xpow(0x1D0F, bits_mod(n));
        ((GLOBAL uint32_t *)out)[job] = v;
    }
}

} // namespace

/* kind 1 CRC, 2 checksum.  jobs / first / task_map / partials: device memory (first: n_jobs + 1 task offsets, task_map: (job, task of
 * the job) per task, partials: n_tasks words); out: n_jobs words, pinned host memory */
extern "C" void ohk_hash(int kind, const OhMd5Job *jobs, const uint32_t *first, const uint32_t *task_map, int n_jobs, int n_tasks, uint32_t *partials,
                         uint32_t *out, hipStream_t st)
{
    if (n_jobs <= 0 || n_tasks <= 0)
        return;
    const uint2v *tm = (const uint2v *)task_map;
    if (kind == 1)
        hipLaunchKernelGGL(crc_kernel, dim3(n_tasks), dim3(THREADS), 0, st, jobs, tm, partials);
    else
        hipLaunchKernelGGL(checksum_kernel, dim3(n_tasks), dim3(THREADS), 0, st, jobs, tm, partials);
    hipLaunchKernelGGL(hash_combine_kernel, dim3(n_jobs), dim3(THREADS), 0, st, jobs, first, partials, kind, out);
}
