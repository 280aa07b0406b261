"""The numpy model of oh_pics_weave, oh_pics_separate and oh_pics_deinterlace (include/ohevc_hip.h), written from the
text of their definitions, sample by sample where the definition is sample by sample — not from the kernel.

Per plane (H x W coded samples, H even), M = 2^bit_depth - 1.  Rows with y % 2 == parity are kept, the others are missing.
    clamped rows   r(k) = min(max(k, 0), H - 1)
    mirrored rows  up = y - 1 if y - 1 >= 0 else y + 1;  dn = y + 1 if y + 1 <= H - 1 else y - 1      (always kept rows)
    columns        cx(k) = min(max(k, 0), W - 1)
"""
import numpy as np

BOB, BLEND, LOWPASS5, ADAPTIVE = 0, 1, 2, 3


def weave_plane(T, B):
    """D[2y][x] = T[y][x], D[2y + 1][x] = B[y][x]"""
    T, B = np.asarray(T), np.asarray(B)
    assert T.shape == B.shape and T.dtype == B.dtype
    D = np.empty((2 * T.shape[0], T.shape[1]), T.dtype)
    for y in range(T.shape[0]):
        D[2 * y] = T[y]
        D[2 * y + 1] = B[y]
    return D


def separate_plane(D):
    """the exact inverse: (T, B)"""
    D = np.asarray(D)
    assert D.shape[0] % 2 == 0
    T = np.empty((D.shape[0] // 2, D.shape[1]), D.dtype)
    B = np.empty_like(T)
    for y in range(T.shape[0]):
        T[y] = D[2 * y]
        B[y] = D[2 * y + 1]
    return T, B


def weave(top_planes, bottom_planes):
    return [weave_plane(t, b) for t, b in zip(top_planes, bottom_planes)]


def separate(planes):
    both = [separate_plane(p) for p in planes]
    return [t for t, _ in both], [b for _, b in both]


def _mirrored(y, H):
    return (y - 1 if y - 1 >= 0 else y + 1), (y + 1 if y + 1 <= H - 1 else y - 1)


def bob_plane(C, parity):
    C = np.asarray(C).astype(np.int64)
    H = C.shape[0]
    out = C.copy()
    for y in range(H):
        if y % 2 != parity:
            up, dn = _mirrored(y, H)
            out[y] = (C[up] + C[dn] + 1) >> 1
    return out


def blend_plane(C):
    C = np.asarray(C).astype(np.int64)
    H = C.shape[0]
    out = np.empty_like(C)
    for y in range(H):
        out[y] = (C[max(y - 1, 0)] + 2 * C[y] + C[min(y + 1, H - 1)] + 2) >> 2
    return out


def lowpass5_plane(C, parity, bit_depth):
    C = np.asarray(C).astype(np.int64)
    H = C.shape[0]
    M = (1 << bit_depth) - 1
    out = C.copy()

    def r(k):
        return min(max(k, 0), H - 1)
    for y in range(H):
        if y % 2 != parity:
            v = (-C[r(y - 2)] + 4 * C[r(y - 1)] + 2 * C[y] + 4 * C[r(y + 1)] - C[r(y + 2)] + 4) >> 3      # numpy's >> of a signed array is arithmetic
            out[y] = np.clip(v, 0, M)
    return out


def adaptive_sample(up, dn, a, b, pu, pd, nu, nd):
    """one missing sample from its window (the arguments of oh_deint_adaptive): (out, j*, clamp outcome -1 below / 0 inside / +1 above,
    (d0 >> 1, d1, d2))"""
    up, dn = [int(v) for v in up], [int(v) for v in dn]
    a, b, pu, pd, nu, nd = int(a), int(b), int(pu), int(pd), int(nu), int(nd)
    c, e = up[3], dn[3]
    t = (a + b) >> 1
    d0 = abs(a - b)
    d1 = (abs(pu - c) + abs(pd - e)) >> 1
    d2 = (abs(nu - c) + abs(nd - e)) >> 1
    diff = max(d0 >> 1, d1, d2)

    def score(j):
        return sum(abs(up[3 + k + j] - dn[3 + k - j]) for k in (-1, 0, 1))
    best, js = score(0) - 1, 0
    for s in (-1, 1):
        if score(s) < best:
            best, js = score(s), s
            if score(2 * s) < best:
                best, js = score(2 * s), 2 * s
    sp = (up[3 + js] + dn[3 - js]) >> 1
    out = min(max(sp, t - diff), t + diff)
    outcome = -1 if sp < t - diff else 1 if sp > t + diff else 0
    return out, js, outcome, (d0 >> 1, d1, d2)


def adaptive_plane(P, C, N, parity, kept_first, detail=False):
    """the plane of the destination; with detail also three int arrays over the plane (meaningful in missing rows): j*, the clamp outcome
    (-1 / 0 / +1) and which of d0 >> 1, d1, d2 was the strict maximum (0 / 1 / 2, -1 where none was)"""
    P, C, N = (np.asarray(v).astype(np.int64) for v in (P, C, N))
    H, W = C.shape
    A, B = (P, C) if kept_first else (C, N)
    out = C.copy()
    jst, outcome, which = np.zeros((H, W), int), np.zeros((H, W), int), np.full((H, W), -1)
    for y in range(H):
        if y % 2 == parity:
            continue
        up, dn = _mirrored(y, H)
        for x in range(W):
            cols = [min(max(x - 3 + i, 0), W - 1) for i in range(7)]
            v, js, oc, ds = adaptive_sample(C[up, cols], C[dn, cols], A[y, x], B[y, x], P[up, x], P[dn, x], N[up, x], N[dn, x])
            out[y, x] = v
            jst[y, x], outcome[y, x] = js, oc
            top = max(ds)
            if ds.count(top) == 1:
                which[y, x] = ds.index(top)
    return (out, jst, outcome, which) if detail else out


def plane_shapes(w, h, cf):
    """(rows, columns) of the coded planes of a w x h picture of chroma format cf"""
    if cf == 0:
        return [(h, w)]
    cw, ch = (w // 2 if cf in (1, 2) else w), (h // 2 if cf == 1 else h)
    return [(h, w), (ch, cw), (ch, cw)]


def random_triplet(bit_depth, w, h, cf):
    """independent uniform random prev, cur, next of the GPU tests, each a list of coded planes: numpy.random.default_rng(bit_depth),
    the three luma planes first (so they do not depend on cf: the host tests assert what they make the model do), then the chroma"""
    rng = np.random.default_rng(bit_depth)
    dt = np.uint8 if bit_depth == 8 else np.uint16
    shapes = plane_shapes(w, h, cf)
    pics = [[rng.integers(0, 1 << bit_depth, shapes[0], dtype=dt)] for _ in range(3)]
    for pic in pics:
        for s in shapes[1:]:
            pic.append(rng.integers(0, 1 << bit_depth, s, dtype=dt))
    return pics


def deinterlace(cur, mode, parity, bit_depth, kept_first=1, prev=None, nxt=None):
    """cur / prev / nxt: the coded planes of the pictures (prev, nxt None: cur) -> the coded planes of the destination, in cur's dtype"""
    assert mode in (BOB, BLEND, LOWPASS5, ADAPTIVE) and parity in (0, 1) and kept_first in (0, 1)
    prev = cur if prev is None else prev
    nxt = cur if nxt is None else nxt
    out = []
    for c, pl in enumerate(cur):
        pl = np.asarray(pl)
        assert pl.shape[0] % 2 == 0 and pl.shape[0] >= 2
        if mode == BOB:
            v = bob_plane(pl, parity)
        elif mode == BLEND:
            v = blend_plane(pl)
        elif mode == LOWPASS5:
            v = lowpass5_plane(pl, parity, bit_depth)
        else:
            v = adaptive_plane(prev[c], pl, nxt[c], parity, kept_first)
        assert v.min() >= 0 and v.max() <= (1 << bit_depth) - 1
        out.append(v.astype(pl.dtype))
    return out
