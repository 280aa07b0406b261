"""A model of oh_pics_warp in Python integers and numpy int64, written from the definition's text and not from the C
code: the position of a sample, the integer part and fraction each filter takes, the border rule, the three filters, and the layout of
the destination.  Every function takes Python ints or int64 arrays alike (>> of a negative value floors in both, // floors)."""
import numpy as np

AFFINE, PERSPECTIVE = 0, 1
NEAREST, BILINEAR, BICUBIC = 0, 1, 2
REPLICATE, CONSTANT = 0, 1
ONE, ONE30 = 1 << 16, 1 << 30
IDENTITY = (ONE, 0, 0, 0, ONE, 0, 0, 0, ONE30)


def shifts(cf, c):
    """(hs, vs) of plane c at chroma format cf"""
    return (int(c > 0 and cf in (1, 2)), int(c > 0 and cf == 1))


def _clamp(v, lo, hi):
    return np.clip(v, lo, hi) if isinstance(v, np.ndarray) else min(max(v, lo), hi)


def position(m, mode, hs, vs, x, y):
    """sample (x, y) of a plane with shifts (hs, vs) of the image -> (Px, Py), Q16, in the plane's window"""
    X, Y, h = x << hs, y << vs, vs
    nx = m[0] * X + m[1] * Y + m[2] + h * (m[1] >> 1)
    ny = m[3] * X + m[4] * Y + m[5] + h * (m[4] >> 1)
    if mode == PERSPECTIVE:
        d = (m[6] * X + m[7] * Y + m[8] + h * (m[7] >> 1)) >> 8
        nx, ny = (nx << 22) // d, (ny << 22) // d
    lx, ly = _clamp(nx, -(1 << 30), (1 << 31) - 1), _clamp(ny, -(1 << 30), (1 << 31) - 1)
    return lx >> hs, (ly - vs * (1 << 15)) >> vs


def split(filt, p):
    """a Q16 position -> (integer part, fraction in 1/64)"""
    if filt == NEAREST:
        return (p + (1 << 15)) >> 16, p * 0
    q = (p + 512) >> 10
    return q >> 6, q & 63


def cubic(f):
    """the four taps of phase f: Keys, a = -1/2, as exact integers that sum to 1024"""
    n = [-f ** 3 + 128 * f ** 2 - 4096 * f, 3 * f ** 3 - 320 * f ** 2 + (1 << 19), -3 * f ** 3 + 256 * f ** 2 + 4096 * f, f ** 3 - 64 * f ** 2]
    assert sum(n) == 1 << 19
    c = [(v + 256) >> 9 for v in n]
    big = 1 if f <= 32 else 2
    c[big] = 1024 - sum(c[k] for k in range(4) if k != big)
    return c


CUBIC_LIST = [cubic(f) for f in range(64)]
CUBIC = np.array(CUBIC_LIST, dtype=np.int64)


def cubic_of(f):
    """the four taps at phase f: four ints, or four arrays where f is one"""
    return [CUBIC[f, k] for k in range(4)] if isinstance(f, np.ndarray) else CUBIC_LIST[f]


def interp(s, filt, ix, iy, fx, fy, top):
    """the sample: s(i, j) gives the tap at plane index (i, j), the border rule applied; ints or int64 arrays"""
    if filt == NEAREST:
        return s(ix, iy)
    if filt == BILINEAR:
        t = [(64 - fx) * s(ix, iy + j) + fx * s(ix + 1, iy + j) for j in (0, 1)]
        return ((64 - fy) * t[0] + fy * t[1] + (1 << 11)) >> 12
    cx, cy = cubic_of(fx), cubic_of(fy)
    v = 0
    for j in range(4):
        t = sum(cx[k] * s(ix - 1 + k, iy - 1 + j) for k in range(4))
        v = v + cy[j] * ((t + 8) >> 4)
    return _clamp((v + (1 << 15)) >> 16, 0, top)


def interp_taps(taps, fx, fy, filt, bit_depth):
    """one sample from its 4 x 4 neighbourhood, taps[4 j + i] = s(ix - 1 + i, iy - 1 + j), in Python integers"""
    return int(interp(lambda i, j: int(taps[4 * j + i]), filt, 1, 1, fx, fy, (1 << bit_depth) - 1))


def warp_plane(S, m, mode, filt, border, fill, hs, vs, iw, ih, dw, dh, bit_depth):
    """the coded destination plane (dh x dw) from the plane's window S: the image iw x ih, then its last column and row replicated"""
    Hc, Wc = S.shape
    S64 = S.astype(np.int64)
    y, x = np.meshgrid(np.arange(ih, dtype=np.int64), np.arange(iw, dtype=np.int64), indexing="ij")
    px, py = position([int(v) for v in m], mode, hs, vs, x, y)
    ix, fx = split(filt, px)
    iy, fy = split(filt, py)

    def s(i, j):
        ic, jc = np.clip(i, 0, Wc - 1), np.clip(j, 0, Hc - 1)
        v = S64[jc, ic]
        return np.where((ic != i) | (jc != j), np.int64(fill), v) if border == CONSTANT else v

    img = interp(s, filt, ix, iy, fx, fy, (1 << bit_depth) - 1)
    assert img.min() >= 0 and img.max() < 1 << bit_depth
    return img[np.ix_(np.minimum(np.arange(dh), ih - 1), np.minimum(np.arange(dw), iw - 1))].astype(S.dtype)


def warp(planes, sp, window, m, size, dp, mode=AFFINE, filt=BILINEAR, border=REPLICATE, fill=(0, 0, 0)):
    """the coded planes of a destination of params dp: planes are the source's coded planes (params sp), window = (left, right, top,
    bottom) in luma samples, size = (width, height) of the image in luma samples"""
    left, right, top, bottom = window
    out = []
    for c, P in enumerate(planes):
        hs, vs = shifts(sp.chroma_format_idc, c)
        S = P[top >> vs:(sp.height - bottom) >> vs, left >> hs:(sp.width - right) >> hs]
        out.append(warp_plane(S, m, mode, filt, border, fill[c], hs, vs, size[0] >> hs, size[1] >> vs, dp.width >> hs, dp.height >> vs, sp.bit_depth))
    return out


# ---- the map builders, in Python integers ----
def translation(dx_q2, dy_q2):
    return [ONE, 0, dx_q2 * 16384, 0, ONE, dy_q2 * 16384, 0, 0, ONE30]


def then(a, b):
    """warping by a, then warping its image by b: A_a A_b, every product (p q + 2^15) >> 16"""
    def p(u, v):
        return (u * v + (1 << 15)) >> 16
    return [p(a[0], b[0]) + p(a[1], b[3]), p(a[0], b[1]) + p(a[1], b[4]), p(a[0], b[2]) + p(a[1], b[5]) + a[2],
            p(a[3], b[0]) + p(a[4], b[3]), p(a[3], b[1]) + p(a[4], b[4]), p(a[3], b[2]) + p(a[4], b[5]) + a[5], 0, 0, ONE30]


def rdiv(n, d):
    """n / d to the nearest integer, halves up"""
    if d < 0:
        n, d = -n, -d
    return (2 * n + d) // (2 * d)


def invert(f):
    a, b, tx, c, d, ty = f[:6]
    det = a * d - b * c
    if det == 0:
        return None
    return [rdiv(d << 32, det), rdiv(-b << 32, det), rdiv((b * ty - d * tx) << 16, det),
            rdiv(-c << 32, det), rdiv(a << 32, det), rdiv((c * tx - a * ty) << 16, det), 0, 0, ONE30]


def rotation_offsets(m, cs, cd):
    """m[2], m[5] of a rotation with the terms m[0], m[1], m[3], m[4] about the centres cs (source) and cd (destination), Q16"""
    return (cs[0] - ((m[0] * cd[0] + m[1] * cd[1] + (1 << 15)) >> 16), cs[1] - ((m[3] * cd[0] + m[4] * cd[1] + (1 << 15)) >> 16))


def in_bounds(m):
    return all(abs(m[k]) <= 1 << 22 for k in (0, 1, 3, 4)) and all(abs(m[k]) <= 1 << 36 for k in (2, 5))


def orient_map(o, w, h):
    """orientation o (0 .. 7 of oh_pics_orient: TRANSPOSE 4 first, then HFLIP 1, then VFLIP 2) of a w x h window as an exact integer
    inverse map, and the image's size"""
    iw, ih = (h, w) if o & 4 else (w, h)
    # image (x, y) -> after undoing VFLIP and HFLIP -> (u, v) of T; T[v][u] = S[u][v] under TRANSPOSE
    ux, u0 = (-1, iw - 1) if o & 1 else (1, 0)
    vy, v0 = (-1, ih - 1) if o & 2 else (1, 0)
    if o & 4:                                                   # source column = v, source row = u
        m = [0, vy * ONE, v0 * ONE, ux * ONE, 0, u0 * ONE]
    else:
        m = [ux * ONE, 0, u0 * ONE, 0, vy * ONE, v0 * ONE]
    return m + [0, 0, ONE30], (iw, ih)
