"""The numpy model of oh_pics_orient, written from its three index formulas — not from np.rot90, which the tests
hold against it.  Per plane c, S is the plane's window, Ws x Hs:
    1. TRANSPOSE first:  T[y][x] = S[x][y]            (without it T = S)
    2. HFLIP next:       U[y][x] = T[y][Wt - 1 - x]
    3. VFLIP last:       I[y][x] = U[Ht - 1 - y][x]
and the destination's coded plane replicates I's last column and row: D[y][x] = I[min(y, Hi - 1)][min(x, Wi - 1)]."""
import numpy as np

HFLIP, VFLIP, TRANSPOSE = 1, 2, 4


def hshift(cf, c):
    return int(bool(c) and cf in (1, 2))


def vshift(cf, c):
    return int(bool(c) and cf == 1)


def orient_plane(S, orientation):
    """the image I of one plane's window S"""
    S = np.asarray(S)
    Hs, Ws = S.shape
    if orientation & TRANSPOSE:
        T = np.empty((Ws, Hs), S.dtype)
        for y in range(Ws):
            for x in range(Hs):
                T[y, x] = S[x, y]
    else:
        T = S.copy()
    Ht, Wt = T.shape
    U = T.copy()
    if orientation & HFLIP:
        for x in range(Wt):
            U[:, x] = T[:, Wt - 1 - x]
    out = U.copy()
    if orientation & VFLIP:
        for y in range(Ht):
            out[y, :] = U[Ht - 1 - y, :]
    return out


def orient(planes, params, window, orientation, dst_params):
    """planes: the coded planes of a source with OhPicParams params; window = (left, right, top, bottom), luma samples -> the coded
    planes of a destination with dst_params (the sources' bit depth and chroma format), edge replication included"""
    cf = params.chroma_format_idc
    left, right, top, bottom = window
    W, H = params.width - left - right, params.height - top - bottom
    assert W > 0 and H > 0 and 0 <= orientation <= 7 and dst_params.chroma_format_idc == cf
    out = []
    for c, pl in enumerate(planes):
        hs, vs = hshift(cf, c), vshift(cf, c)
        S = np.asarray(pl)[top >> vs:(top >> vs) + (H >> vs), left >> hs:(left >> hs) + (W >> hs)]
        img = orient_plane(S, orientation)
        Hi, Wi = img.shape
        dw, dh = dst_params.width >> hs, dst_params.height >> vs
        assert Wi <= dw and Hi <= dh
        ys, xs = np.minimum(np.arange(dh), Hi - 1), np.minimum(np.arange(dw), Wi - 1)
        out.append(img[np.ix_(ys, xs)])
    return out
