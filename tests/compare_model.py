"""numpy model of oh_pics_compare (include/ohevc_hip.h), bit for bit, written from the definition only.

Per plane of a pair over the plane's window: samples, differing, sad, sse, max_abs and the first differing sample in raster order —
plain integer sums, counts and extrema — and SSIM in the common 8x8-window, stride-4 form: the window is tiled into 4x4 blocks
anchored at its top-left (leftover columns and rows take no part), a window is the sum of 2x2 neighbouring blocks, its value is
rint(n1 n2 / (d1 d2) 2^30) with the four integers exact in int64 and the quotient in float64 (two multiplications, one division,
an exact scaling), and ssim_sum is the integer sum of the window values."""
import numpy as np

Q = 1 << 30
NONE = 0xFFFFFFFF                                                           # OH_CMP_NONE
FIELDS = ("samples", "differing", "sad", "sse", "max_abs", "first", "ssim_windows", "ssim_sum")


def ssim_consts(bit_depth):
    M = (1 << bit_depth) - 1
    return (64 * M * M + 5000) // 10000, (9 * 64 * 63 * M * M + 5000) // 10000


def ssim_window(bit_depth, s1, s2, ss, s12):
    """the Q30 values of windows with the sums s1 = sum a, s2 = sum b, ss = sum a^2 + sum b^2, s12 = sum ab (int64 arrays or scalars)"""
    c1, c2 = ssim_consts(bit_depth)
    s1, s2, ss, s12 = (np.asarray(v, dtype=np.int64) for v in (s1, s2, ss, s12))
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    n1, n2 = 2 * s1 * s2 + c1, 2 * covar + c2
    d1, d2 = s1 * s1 + s2 * s2 + c1, vars_ + c2
    num = n1.astype(np.float64) * n2.astype(np.float64)
    den = d1.astype(np.float64) * d2.astype(np.float64)
    return np.rint(num / den * np.float64(Q)).astype(np.int64)


def window_values(a, b, bit_depth):
    """the Q30 value of every 8x8 window of two planes, an int64 array of (max(nby - 1, 0), max(nbx - 1, 0))"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    h, w = a.shape
    nbx, nby = w >> 2, h >> 2
    if nbx < 2 or nby < 2:
        return np.zeros((max(nby - 1, 0), max(nbx - 1, 0)), np.int64)

    def blocks(v):
        return v[:4 * nby, :4 * nbx].reshape(nby, 4, nbx, 4).sum(axis=(1, 3))

    def windows(v):
        return v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:]

    s1, s2, ss, s12 = (windows(blocks(v)) for v in (a, b, a * a + b * b, a * b))
    return ssim_window(bit_depth, s1, s2, ss, s12)


def plane_diff(a, b, bit_depth, ssim=True):
    """one plane's window of both pictures (equal shapes) -> a dict of FIELDS; first: None or (x, y)"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    assert a.shape == b.shape and a.ndim == 2
    h, w = a.shape
    d = a - b
    nz = np.flatnonzero(d)
    out = dict(samples=w * h, differing=int(nz.size), sad=int(np.abs(d).sum()), sse=int((d * d).sum()),
               max_abs=int(np.abs(d).max()) if d.size else 0, first=(int(nz[0] % w), int(nz[0] // w)) if nz.size else None,
               ssim_windows=0, ssim_sum=0)
    if ssim:
        q = window_values(a, b, bit_depth)
        out["ssim_windows"] = max((w >> 2) - 1, 0) * max((h >> 2) - 1, 0)
        assert q.size == out["ssim_windows"]
        out["ssim_sum"] = int(q.sum())
    return out


ABSENT = dict(samples=0, differing=0, sad=0, sse=0, max_abs=0, first=None, ssim_windows=0, ssim_sum=0)


def compare(planes_a, planes_b, p, window=(0, 0, 0, 0), ssim=True):
    """the coded planes of two pictures with params p -> three dicts of FIELDS (planes a 4:0:0 picture lacks: ABSENT)"""
    left, right, top, bottom = window
    cf = p.chroma_format_idc
    out = []
    for c in range(3):
        if c and not cf:
            out.append(dict(ABSENT))
            continue
        hs = 1 if c and cf in (1, 2) else 0
        vs = 1 if c and cf == 1 else 0
        x0, y0 = left >> hs, top >> vs
        w, h = (p.width - left - right) >> hs, (p.height - top - bottom) >> vs
        out.append(plane_diff(planes_a[c][y0:y0 + h, x0:x0 + w], planes_b[c][y0:y0 + h, x0:x0 + w], p.bit_depth, ssim))
    return out
