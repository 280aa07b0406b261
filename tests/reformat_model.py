"""numpy model of oh_pics_reformat, int64 throughout and literal: coded planes in, coded planes out.  Every destination
sample is a weighted sum of source samples of its plane whose weights total 2^f, then ONE quantisation by s = f + Bs - Bd bits."""
import numpy as np

ROUND, DITHER = 0, 1                                                        # OH_RF_ROUND, OH_RF_DITHER
POINT, LINEAR = 0, 1                                                        # OH_RF_POINT, OH_RF_LINEAR
B4 = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64)


def shifts(cf):
    """(hshift, vshift) of the chroma planes"""
    return (1 if cf in (1, 2) else 0, 1 if cf == 1 else 0)


def offsets(s, mode, shape):
    """the rounding offset r of every sample of a plane of that shape, s > 0"""
    if mode == ROUND:
        return np.full(shape, 1 << (s - 1), np.int64)
    y, x = np.indices(shape)
    return ((2 * B4[y & 3, x & 3] + 1) << s) >> 5


def quantise(sums, s, mode, bd, x=None, y=None):
    """a plane of sums -> samples of bd bits; (x, y) default to the plane's own coordinates, else scalars or arrays of its shape"""
    sums = np.asarray(sums, np.int64)
    mx = (1 << bd) - 1
    if s <= 0:
        return np.minimum(sums << -s, mx)
    if x is None:
        r = offsets(s, mode, sums.shape)
    elif mode == ROUND:
        r = 1 << (s - 1)
    else:
        r = ((2 * B4[np.asarray(y) & 3, np.asarray(x) & 3] + 1) << s) >> 5
    return np.minimum((sums + r) >> s, mx)


def down_h(C, filt):
    """half the columns: (sums, f)"""
    if filt == POINT:
        return C[:, 0::2], 0
    w = C.shape[1]
    x2 = 2 * np.arange(w // 2)
    return C[:, np.maximum(x2 - 1, 0)] + 2 * C[:, x2] + C[:, np.minimum(x2 + 1, w - 1)], 2


def down_v(C, filt):
    if filt == POINT:
        return C[0::2], 0
    return C[0::2] + C[1::2], 1


def up_h(C, filt):
    """twice the columns: (sums, f)"""
    cw = C.shape[1]
    X = np.arange(2 * cw)
    k = X >> 1
    if filt == POINT:
        return C[:, k], 0
    k2 = np.where(X & 1, np.minimum(k + 1, cw - 1), k)
    return C[:, k] + C[:, k2], 1


def up_v(C, filt):
    ch = C.shape[0]
    Y = np.arange(2 * ch)
    j0 = Y >> 1
    if filt == POINT:
        return C[j0], 0
    j1 = np.clip(j0 - 1 + 2 * (Y & 1), 0, ch - 1)
    return 3 * C[j0] + C[j1], 2


def chroma_sums(C, scf, dcf, down, up):
    """(sums on the destination's chroma grid, f) of one source chroma plane; scf, dcf in 1 .. 3.  Both steps are linear and of one
    direction, so their order does not matter: the vertical one first."""
    (shs, svs), (dhs, dvs) = shifts(scf), shifts(dcf)
    S, f = np.asarray(C, np.int64), 0
    if dvs > svs:
        S, g = down_v(S, down)
        f += g
    elif dvs < svs:
        S, g = up_v(S, up)
        f += g
    if dhs > shs:
        S, g = down_h(S, down)
        f += g
    elif dhs < shs:
        S, g = up_h(S, up)
        f += g
    return S, f


def reformat(src_planes, sbd, scf, dbd, dcf, depth=ROUND, down=LINEAR, up=LINEAR):
    """the coded planes of one destination: src_planes = [Y] or [Y, Cb, Cr] of a picture of sbd bits and chroma format scf"""
    k = sbd - dbd
    Y = np.asarray(src_planes[0], np.int64)
    out = [quantise(Y, k, depth, dbd)]
    if dcf == 0:
        return out
    H, W = Y.shape
    dhs, dvs = shifts(dcf)
    for c in (1, 2):
        if scf == 0:
            out.append(np.full((H >> dvs, W >> dhs), 1 << (dbd - 1), np.int64))
            continue
        S, f = chroma_sums(src_planes[c], scf, dcf, down, up)
        assert S.shape == (H >> dvs, W >> dhs)
        out.append(quantise(S, f + k, depth, dbd))
    return out
