"""The numpy model of the frame packing service (include/ohevc_hip.h: oh_pics_unpack, oh_pics_pack), written from the
definition and not from the kernels.  Everything is per plane: a packed plane is a 2-D integer array, a view's plane the window of that
view; coded() replicates the last column and row over the rest of a coded plane."""
import numpy as np

SBS, TB = 3, 4

LUMA = np.array([
    [0, 0, 0, 64, 0, 0, 0, 0], [0, 1, -3, 63, 4, -2, 1, 0], [-1, 2, -5, 62, 8, -3, 1, 0], [-1, 3, -8, 60, 13, -4, 1, 0],
    [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 52, 26, -8, 3, -1], [-1, 3, -9, 47, 31, -10, 4, -1], [-1, 4, -11, 45, 34, -10, 4, -1],
    [-1, 4, -11, 40, 40, -11, 4, -1], [-1, 4, -10, 34, 45, -11, 4, -1], [-1, 4, -10, 31, 47, -9, 3, -1], [-1, 3, -8, 26, 52, -11, 4, -1],
    [0, 1, -5, 17, 58, -10, 4, -1], [0, 1, -4, 13, 60, -8, 3, -1], [0, 1, -3, 8, 62, -5, 2, -1], [0, 1, -2, 4, 63, -3, 1, 0]], dtype=np.int64)
CHROMA = np.array([
    [0, 64, 0, 0], [-2, 62, 4, 0], [-2, 58, 10, -2], [-4, 56, 14, -2], [-4, 54, 16, -2], [-6, 52, 20, -2], [-6, 46, 28, -4], [-4, 42, 30, -4],
    [-4, 36, 36, -4], [-4, 30, 42, -4], [-4, 28, 46, -6], [-2, 20, 52, -6], [-2, 16, 54, -4], [-2, 14, 56, -4], [-2, 10, 58, -2], [0, 4, 62, -2]],
    dtype=np.int64)


def shifts(chroma_format_idc, plane):
    """(hs, vs) of a plane"""
    if plane == 0:
        return 0, 0
    return {1: (1, 1), 2: (1, 0), 3: (0, 0)}[chroma_format_idc]


def constituent(packed, arrangement, v, flip):
    """C_v of a packed plane: the rectangle R_v with the flip undone"""
    H, W = packed.shape
    if arrangement == SBS:
        r = packed[:, v * (W // 2):(v + 1) * (W // 2)]
        return r[:, ::-1] if flip else r
    r = packed[v * (H // 2):(v + 1) * (H // 2), :]
    return r[::-1, :] if flip else r


def positions(n_out, g, kind):
    """p of output indices 0 .. n_out - 1: kind 0 a plane that is not sub-sampled on the packed axis, 1 a sub-sampled horizontal axis
    (co-sited), 2 a sub-sampled vertical axis (midway)"""
    Z = np.arange(n_out, dtype=np.int64)
    if kind == 0:
        return 8 * Z - g
    return (16 * Z - g + 1) >> 1 if kind == 1 else (16 * Z - g - 3) >> 1


def filter_sums(c, g, kind, chroma):
    """the unrounded sums S of the up-sampler along the last axis of c (N stored samples -> 2 N)"""
    N = c.shape[-1]
    p = positions(2 * N, g, kind)
    i, ph = p >> 4, p & 15
    taps, off = (CHROMA, 1) if chroma else (LUMA, 3)
    s = np.zeros(c.shape[:-1] + (2 * N,), dtype=np.int64)
    for k in range(taps.shape[1]):
        s += taps[ph, k] * c[..., np.clip(i + k - off, 0, N - 1)].astype(np.int64)
    return s


def quincunx_full(c, arrangement, v):
    """the full-resolution plane from the lattice samples of C_v: the project's own reading of the lattice"""
    h, w = c.shape
    H, W = (h, 2 * w) if arrangement == SBS else (2 * h, w)
    Y, X = np.mgrid[0:H, 0:W]

    def lattice(y, x):                                        # the lattice sample at full-resolution (x, y), which lies on the lattice
        return c[y, x >> 1] if arrangement == SBS else c[y >> 1, x]

    on = ((X ^ Y ^ v) & 1) == 0
    xl, xr = np.where(X > 0, X - 1, X + 1), np.where(X + 1 < W, X + 1, X - 1)
    yu, yd = np.where(Y > 0, Y - 1, Y + 1), np.where(Y + 1 < H, Y + 1, Y - 1)
    avg = (lattice(Y, xl).astype(np.int64) + lattice(Y, xr) + lattice(yu, X) + lattice(yd, X) + 2) >> 2
    return np.where(on, lattice(Y, X), avg)                     # lattice(Y, X) of an off-lattice place is some stored sample: not taken


def unpack_plane(packed, arrangement, v, *, flip=False, g=0, quincunx=False, full=True, plane=0, chroma_format_idc=1, bit_depth=8):
    """the window of view v's plane.  g: the grid position on the packed axis"""
    c = constituent(np.asarray(packed).astype(np.int64), arrangement, v, flip)
    if not full:
        return c
    if quincunx:
        return quincunx_full(c, arrangement, v)
    hs, vs = shifts(chroma_format_idc, plane)
    if arrangement == SBS:
        s = filter_sums(c, g, 1 if hs else 0, plane > 0)
    else:
        s = filter_sums(c.T, g, 2 if vs else 0, plane > 0).T
    return np.clip((s + 32) >> 6, 0, (1 << bit_depth) - 1)


def coded(window, coded_h, coded_w):
    """a coded plane whose top left is `window` and whose rest replicates the window's last column and row"""
    h, w = window.shape
    return window[np.minimum(np.arange(coded_h), h - 1)[:, None], np.minimum(np.arange(coded_w), w - 1)[None, :]]


def pack_plane(view0, view1, arrangement, *, flip=(False, False), quincunx=False):
    """the packed plane of two views' windows: half-size views are placed with the flips applied; with quincunx full-size views are
    point-sampled on the lattice"""
    halves = []
    for v, a in enumerate((np.asarray(view0), np.asarray(view1))):
        if quincunx:
            H, W = a.shape
            if arrangement == SBS:
                y, x = np.mgrid[0:H, 0:W // 2]
                a = a[y, 2 * x + ((y + v) & 1)]
            else:
                y, x = np.mgrid[0:H // 2, 0:W]
                a = a[2 * y + ((x + v) & 1), x]
        if flip[v]:
            a = a[:, ::-1] if arrangement == SBS else a[::-1, :]
        halves.append(a)
    return np.concatenate(halves, axis=1 if arrangement == SBS else 0)


def view_size(W, H, arrangement, full, min_cb=8):
    """(window width, window height, coded width, coded height) of a view of packed pictures of W x H luma samples"""
    w, h = (W, H) if full else (W // 2, H) if arrangement == SBS else (W, H // 2)
    return w, h, -(-w // min_cb) * min_cb, -(-h // min_cb) * min_cb
