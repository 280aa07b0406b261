"""numpy statement of the picture resizing of DESIGN.md §3c (oh_pics_resize): what the kernels must produce bit for bit.

Each plane is resampled on its own, separably, horizontal pass first.  Along one axis, S = extent of the source window in the plane,
T = extent of the image in the plane, p = phase (2: sample centred in its cell; 1: the co-sited chroma columns of 4:2:0 / 4:2:2).
All positions are integers in units of 1/(4T) source samples: source sample i sits at (4i + p) T, image sample x at (4x + p) S.
"""
import numpy as np

PREC = 14
BILINEAR, BICUBIC = 0, 1                                       # OH_RESIZE_BILINEAR, OH_RESIZE_BICUBIC
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC}


def filter_id(filt):
    return FILTERS[filt] if isinstance(filt, str) else int(filt)


def weights(S, T, filt, p, x):
    """(first source index, exact integer weights) of image sample x: the samples 0 <= i < S with n = |(4i + p) T - (4x + p) S| < R D"""
    D = 4 * max(S, T)                                          # one filter unit: the filter stretches by max(1, S / T)
    R = 1 if filter_id(filt) == BILINEAR else 2
    c = (4 * x + p) * S
    lo = -(-(c - R * D - p * T + 1) // (4 * T))
    hi = (c + R * D - p * T - 1) // (4 * T)
    lo, hi = max(lo, 0), min(hi, S - 1)
    w = []
    for i in range(lo, hi + 1):
        n = abs((4 * i + p) * T - c)
        if R == 1:
            w.append(D - n)
        elif n <= D:
            w.append(3 * n ** 3 - 5 * n * n * D + 2 * D ** 3)   # Keys cubic, a = -1/2, scaled by 2 D^3
        else:
            w.append(-(n ** 3 - 5 * n * n * D + 8 * n * D * D - 4 * D ** 3))
    return lo, w


def taps(S, T, filt, p=2):
    """per image sample: (first source index, integer coefficients summing to 1 << PREC, the exact weights w_i / sum(w))"""
    out = []
    for x in range(T):
        lo, w = weights(S, T, filt, p, x)
        s = sum(w)
        assert s > 0
        k = [(2 * wi * (1 << PREC) + s) // (2 * s) for wi in w]    # round half up (floor division, also for negative weights)
        k[k.index(max(k))] += (1 << PREC) - sum(k)               # the first largest takes the remainder
        out.append((lo, k, [wi / s for wi in w]))
    return out


def max_taps(S, T, filt):
    R = 1 if filter_id(filt) == BILINEAR else 2
    return min(S, (2 * R * 4 * max(S, T) - 2) // (4 * T) + 1)


def resize_plane(src, tw, th, bd, filt, ph=2, pv=2, check=True):
    """one plane (2-D integer array) -> th x tw, int64"""
    sh, sw = src.shape
    tx, ty = taps(sw, tw, filt, ph), taps(sh, th, filt, pv)
    s = src.astype(np.int64)
    mid = np.zeros((sh, tw), np.int64)
    for x, (lo, k, _) in enumerate(tx):
        mid[:, x] = (s[:, lo:lo + len(k)] @ np.array(k, np.int64) + (1 << (bd - 1))) >> bd
    if check:
        assert np.abs(mid).max() < 32768
    out = np.zeros((th, tw), np.int64)
    sft = 2 * PREC - bd
    for y, (lo, k, _) in enumerate(ty):
        acc = np.array(k, np.int64) @ mid[lo:lo + len(k), :]
        if check:
            assert np.abs(acc).max() + (1 << (sft - 1)) < 2 ** 31
        out[y] = np.clip((acc + (1 << (sft - 1))) >> sft, 0, (1 << bd) - 1)
    return out


def resize_plane_exact(src, tw, th, filt, ph=2, pv=2):
    """the same taps with their exact weights in float64, no rounding, no clamp"""
    sh, sw = src.shape
    tx, ty = taps(sw, tw, filt, ph), taps(sh, th, filt, pv)
    s = src.astype(np.float64)
    mid = np.zeros((sh, tw))
    for x, (lo, _, w) in enumerate(tx):
        mid[:, x] = s[:, lo:lo + len(w)] @ np.array(w)
    out = np.zeros((th, tw))
    for y, (lo, _, w) in enumerate(ty):
        out[y] = np.array(w) @ mid[lo:lo + len(w)]
    return out


def shifts(cf, c):
    return (1 if c and cf in (1, 2) else 0), (1 if c and cf == 1 else 0)


def resize(planes, cf, bd, size, filt, window=(0, 0, 0, 0)):
    """the coded planes of a picture (chroma format cf, bit depth bd) -> the image planes of size = (width, height) luma samples,
    from the window (left, right, top, bottom) in luma samples"""
    l, r, t, b = window
    H, W = planes[0].shape
    W, H = W - l - r, H - t - b
    out = []
    for c, pl in enumerate(planes):
        hs, vs = shifts(cf, c)
        src = pl[t >> vs:(t >> vs) + (H >> vs), l >> hs:(l >> hs) + (W >> hs)]
        out.append(resize_plane(src, size[0] >> hs, size[1] >> vs, bd, filt, 1 if c and hs else 2, 2).astype(pl.dtype))
    return out


def pad_to(planes, cf, coded):
    """image planes -> the coded planes of a destination of coded = (width, height): the last column and row replicated"""
    out = []
    for c, pl in enumerate(planes):
        hs, vs = shifts(cf, c)
        out.append(np.pad(pl, ((0, (coded[1] >> vs) - pl.shape[0]), (0, (coded[0] >> hs) - pl.shape[1])), mode="edge"))
    return out
