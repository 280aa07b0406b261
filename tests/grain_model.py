"""numpy model of the film grain service (oh_pics_grain), written from the definition in the text, not from
csrc/grain_common.h: the hash, the 169 patterns (HEVC's 32 x 32 inverse transform of band-limited noise), the intensity tables, the
block descriptors and the samples.  The tests compare the C helpers and every plane the GPU writes with it bit for bit.  Python
integers and int64 arrays throughout: >> of a negative value floors, as the arithmetic shift of the definition does."""
import functools

import numpy as np

CUTS = range(2, 15)
M32 = 0xFFFFFFFF


def fmix(h):
    """h: a Python int or an int64 / uint64 array holding uint32 values"""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def H(a, b, c, d):
    """works on Python ints and on uint64 arrays (every product stays below 2^64)"""
    return fmix(a ^ fmix(b ^ fmix(c ^ fmix(d ^ 0x9E3779B9))))


def gauss(h):
    return (h & 255) + (h >> 8 & 255) + (h >> 16 & 255) + (h >> 24 & 255) - 510


@functools.lru_cache(maxsize=None)
def _basis():
    """M[k][n]: HEVC's 32-point transform matrix (H.265 8.6.4.2), from its first column's 31 distinct magnitudes"""
    c = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4]
    m = np.zeros((32, 32), dtype=np.int64)
    for k in range(32):
        for n in range(32):
            a = (k * (2 * n + 1)) % 128                        # the angle in units of pi / 64
            if a > 64:
                a = 128 - a
            m[k, n] = 64 if k == 0 else 0 if a == 32 else c[a] if a < 32 else -c[64 - a]
    return m


def inverse32(C):
    """HEVC's inverse 32 x 32 transform at bit depth 8: columns with shift 7, a 16-bit clip, rows with shift 12, a 16-bit clip"""
    m = _basis()
    e = np.clip((m.T @ np.asarray(C, dtype=np.int64) + 64) >> 7, -32768, 32767)
    return np.clip((e @ m + 2048) >> 12, -32768, 32767)


def isqrt(v):
    r = int(np.sqrt(float(v)))
    while r * r > v:
        r -= 1
    while (r + 1) * (r + 1) <= v:
        r += 1
    return r


@functools.lru_cache(maxsize=None)
def pattern_parts(fh, fv):
    """(coefficients, raw, pattern, r) of pattern (fh, fv), int64 arrays of 32 x 32"""
    v, u = np.meshgrid(np.arange(32, dtype=np.uint64), np.arange(32, dtype=np.uint64), indexing="ij")
    g = gauss(H(np.uint64(1), np.uint64(fh * 16 + fv), u, v).astype(np.int64))
    C = np.where((u < 2 * fh) & (v < 2 * fv) & ((u != 0) | (v != 0)), 8 * g, 0)
    raw = inverse32(C)
    r = isqrt(int((raw * raw).sum()) // 1024)
    P = np.clip((64 * raw + r) // (2 * r), -127, 127)           # // floors
    return C, raw, P, r


def pattern(fh, fv):
    return pattern_parts(fh, fv)[2]


def entry(sigma, fh, fv):
    return sigma | fh << 8 | fv << 12


def uniform(sigma, fh=8, fv=None):
    return np.full(256, entry(sigma, fh, fh if fv is None else fv), dtype=np.uint32)


def from_sei(d):
    """the film grain dict of annexb.film_grain -> ("ok", tables [3][256], planes, blending, log2_scale), or ("arg",) for a cancelled
    message, or ("unsupported",)"""
    if d is None or d.get("cancel"):
        return ("arg",)
    if d["model_id"] != 0 or d["blending_mode_id"] > 1:
        return ("unsupported",)
    tables = np.zeros((3, 256), dtype=np.uint32)
    planes = 0
    for c, comp in enumerate(d["components"]):
        if comp is None:
            continue
        planes |= 1 << c
        taken = np.zeros(256, dtype=bool)
        for lo, hi, vals in comp:
            if len(vals) > 3:
                return ("unsupported",)
            sigma = vals[0]
            fh = vals[1] if len(vals) > 1 else 8
            fv = vals[2] if len(vals) > 2 else fh
            if not 0 <= sigma <= 255 or fh not in CUTS or fv not in CUTS or lo > hi or taken[lo:hi + 1].any():
                return ("unsupported",)
            taken[lo:hi + 1] = True
            tables[c, lo:hi + 1] = entry(sigma, fh, fv)
    return ("ok", tables, planes, d["blending_mode_id"], d["log2_scale_factor"])


def block(seed, c, bx, by):
    """(ox, oy, negate) of block (bx, by) of plane c"""
    h = H(2, seed & M32, c, (by * 65536 + bx) & M32)
    return ((h & 0xFFFF) * 25) >> 16, ((h >> 16 & 0x7FFF) * 25) >> 15, h >> 31


def mean8(samples, bd):
    n = samples.size
    return ((int(samples.astype(np.int64).sum()) + n // 2) // n) >> (bd - 8)


def value(sigma, p, bd, log2_scale):
    return (sigma * p * (1 << (bd - 8)) + (1 << (4 + log2_scale))) >> (5 + log2_scale)


def unsmoothed(plane, c, bd, table, seed, log2_scale):
    """g of every sample of plane c, int64"""
    Hh, W = plane.shape
    g = np.zeros((Hh, W), dtype=np.int64)
    for by in range((Hh + 7) // 8):
        for bx in range((W + 7) // 8):
            blk = plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
            e = int(table[mean8(blk, bd)])
            sigma, fh, fv = e & 255, e >> 8 & 15, e >> 12 & 15
            if not sigma:
                continue
            ox, oy, neg = block(seed, c, bx, by)
            p = pattern(fh, fv)[oy:oy + blk.shape[0], ox:ox + blk.shape[1]]
            g[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = value(sigma, -p if neg else p, bd, log2_scale)
    return g


def smoothed(g):
    W = g.shape[1]
    out = g.copy()
    for x in range(W):
        if (x % 8 == 7 and x + 1 < W) or (x % 8 == 0 and x > 0):
            out[:, x] = (g[:, x - 1] + 2 * g[:, x] + g[:, x + 1] + 2) >> 2
    return out


def blend(s, g, bd, blending):
    s = s.astype(np.int64)
    v = s + ((s * g + (1 << (bd - 1))) >> bd) if blending else s + g
    return np.clip(v, 0, (1 << bd) - 1)


def apply(planes, bd, tables, seed, mask=7, blending=0, log2_scale=0, smooth=True):
    """the coded planes of the destination of one picture: grain on plane c where bit c of mask is set, else a copy"""
    out = []
    for c, pl in enumerate(planes):
        if not mask >> c & 1:
            out.append(pl.copy())
            continue
        g = unsmoothed(pl, c, bd, tables[c], seed, log2_scale)
        out.append(blend(pl, smoothed(g) if smooth else g, bd, blending).astype(pl.dtype))
    return out
