"""The numpy model of oh_pics_filter and its host helpers (include/ohevc_hip.h), written from the text of the
definitions, vectorised over a plane — not from the kernel.  tests/test_filter_host.py holds it against a per-sample restatement.

Per plane (H x W coded samples), M = 2^bit_depth - 1.
    rows     r(k)  = min(max(k, 0), H - 1)
    columns  cx(k) = min(max(k, 0), W - 1)
Clamping an index is padding the array with its edge samples, which is what the functions below do.

Also the planes and parameters of the GPU tests (tests/test_gpu_filter.py), so that the host tests can assert which branches they reach.
"""
import numpy as np

CONVOLVE, UNSHARP, MEDIAN, TEMPORAL = 0, 1, 2, 3
MAX_TAPS = 15


# ---------------------------------------------------------------- helpers
def binomial(n):
    """row n - 1 of Pascal's triangle scaled to sum 256, n in {1, 3, 5, 7, 9}"""
    if n not in (1, 3, 5, 7, 9):
        raise ValueError(n)
    row = np.array([1], dtype=np.int64)
    for _ in range(n - 1):
        row = np.convolve(row, [1, 1])
    return [int(v) * (256 // (1 << (n - 1))) for v in row]


def box(n):
    """n equal taps, n odd in 1 .. 15: 256 // n each, the middle one the remainder more"""
    if n < 1 or n > MAX_TAPS or n % 2 == 0:
        raise ValueError(n)
    t = [256 // n] * n
    t[n // 2] += 256 % n
    return t


def taps_legal(h, v):
    return all(1 <= len(t) <= MAX_TAPS and len(t) % 2 == 1 and sum(t) == 256 and sum(abs(k) for k in t) <= 512 for t in (h, v))


def unsharp_sample(s, b, amount, threshold, M):
    d = s - b
    if abs(d) <= threshold:
        return s
    return min(max(s + ((amount * d + 32) >> 6), 0), M)


def median9(v):
    assert len(v) == 9
    return sorted(int(k) for k in v)[4]


def temporal_sample(c, p, n, mp, mn, threshold):
    ps = p if mp <= threshold else c
    ns = n if mn <= threshold else c
    return (ps + 2 * c + ns + 2) >> 2


# ---------------------------------------------------------------- the modes, a plane at a time
def _shifted(A, ry, rx):
    """the (2 ry + 1) (2 rx + 1) arrays A[r(y + j)][cx(x + i)], j = -ry .. ry outermost, i = -rx .. rx"""
    H, W = A.shape
    P = np.pad(A, ((ry, ry), (rx, rx)), mode="edge")
    return [P[j:j + H, i:i + W] for j in range(2 * ry + 1) for i in range(2 * rx + 1)]


def convolve_acc(S, h, v):
    """acc of CONVOLVE in int64 (the caller may look at its range)"""
    S = np.asarray(S).astype(np.int64)
    assert taps_legal(h, v)
    tmp = sum(int(k) * a for k, a in zip(h, _shifted(S, 0, len(h) // 2)))
    return sum(int(k) * a for k, a in zip(v, _shifted(tmp, len(v) // 2, 0)))


def convolve_plane(S, h, v, bit_depth):
    M = (1 << bit_depth) - 1
    acc = convolve_acc(S, h, v)
    assert np.abs(acc).max() < (1 << 31) - (1 << 15)
    return np.clip((acc + 32768) >> 16, 0, M)                   # numpy's >> of a signed array is arithmetic


def unsharp_plane(S, h, v, amount, threshold, bit_depth, detail=False):
    """with detail also (|d| <= threshold, the value before the clip)"""
    M = (1 << bit_depth) - 1
    S = np.asarray(S).astype(np.int64)
    d = S - convolve_plane(S, h, v, bit_depth)
    keep = np.abs(d) <= threshold
    raw = S + ((amount * d + 32) >> 6)
    out = np.where(keep, S, np.clip(raw, 0, M))
    return (out, keep, raw) if detail else out


def median_plane(S):
    S = np.asarray(S).astype(np.int64)
    return np.sort(np.stack(_shifted(S, 1, 1)), axis=0)[4]


def temporal_sums(P, C, N):
    """mp, mn"""
    P, C, N = (np.asarray(v).astype(np.int64) for v in (P, C, N))
    return sum(_shifted(np.abs(P - C), 1, 1)), sum(_shifted(np.abs(N - C), 1, 1))


def temporal_plane(P, C, N, threshold):
    P, C, N = (np.asarray(v).astype(np.int64) for v in (P, C, N))
    mp, mn = temporal_sums(P, C, N)
    ps = np.where(mp <= threshold, P, C)
    ns = np.where(mn <= threshold, N, C)
    return (ps + 2 * C + ns + 2) >> 2


def _pair(v):
    return tuple(v) if hasattr(v, "__len__") else (v, v)


def filter_pic(src, mode, bit_depth, *, luma=None, chroma=None, amount=64, threshold=0, planes=7, prev=None, nxt=None):
    """src / prev / nxt: the coded planes of the pictures (prev, nxt None: src) -> the coded planes of the destination, in src's dtype.
    The arguments are those of Engine.pics_filter."""
    assert mode in (CONVOLVE, UNSHARP, MEDIAN, TEMPORAL)
    prev = src if prev is None else prev
    nxt = src if nxt is None else nxt
    taps = [(binomial(3), binomial(3)) if t is None else t for t in (luma, chroma)]
    amount, threshold = _pair(amount), _pair(threshold)
    M = (1 << bit_depth) - 1
    out = []
    for c, pl in enumerate(src):
        pl = np.asarray(pl)
        q = int(c > 0)
        if not planes >> c & 1:
            v = pl.astype(np.int64)
        elif mode == CONVOLVE:
            v = convolve_plane(pl, taps[q][0], taps[q][1], bit_depth)
        elif mode == UNSHARP:
            v = unsharp_plane(pl, taps[q][0], taps[q][1], amount[q], threshold[q], bit_depth)
        elif mode == MEDIAN:
            v = median_plane(pl)
        else:
            v = temporal_plane(prev[c], pl, nxt[c], threshold[q])
        assert v.min() >= 0 and v.max() <= M
        out.append(v.astype(pl.dtype))
    return out


# ---------------------------------------------------------------- planes
def plane_shapes(w, h, cf):
    """(rows, columns) of the coded planes of a w x h picture of chroma format cf"""
    if cf == 0:
        return [(h, w)]
    cw, ch = (w // 2 if cf in (1, 2) else w), (h // 2 if cf == 1 else h)
    return [(h, w), (ch, cw), (ch, cw)]


def sample_dtype(bit_depth):
    return np.uint8 if bit_depth == 8 else np.uint16


def random_planes(bit_depth, w, h, cf, seed):
    """independent uniform random coded planes"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bit_depth, s, dtype=sample_dtype(bit_depth)) for s in plane_shapes(w, h, cf)]


def related_triplet(bit_depth, w, h, cf, seed=None):
    """prev, cur, next for TEMPORAL, each a list of coded planes.  cur is uniform random.  Per plane, prev equals cur in the left third
    of the columns, is cur plus noise of -2 .. 2 (clipped) in the middle third and independent of cur in the right third; next is made
    the same way by thirds of the ROWS, so that all nine combinations of the two meet somewhere."""
    rng = np.random.default_rng(bit_depth * 7 + 1 if seed is None else seed)
    M = (1 << bit_depth) - 1
    dt = sample_dtype(bit_depth)
    prev, cur, nxt = [], [], []
    for H, W in plane_shapes(w, h, cf):
        C = rng.integers(0, M + 1, (H, W)).astype(np.int64)
        others = []
        for axis, extent in ((1, W), (0, H)):
            noisy = np.clip(C + rng.integers(-2, 3, (H, W)), 0, M)
            indep = rng.integers(0, M + 1, (H, W))
            pos = np.arange(extent).reshape((1, W) if axis == 1 else (H, 1))
            a, b = extent // 3, extent - extent // 3
            others.append(np.where(pos < a, C, np.where(pos < b, noisy, indep)))
        prev.append(others[0].astype(dt))
        cur.append(C.astype(dt))
        nxt.append(others[1].astype(dt))
    return prev, cur, nxt


def extreme_planes(bit_depth, w, h, cf):
    """(name, coded planes): all 0, all M, checkerboards of 0 / M in both phases"""
    M = (1 << bit_depth) - 1
    dt = sample_dtype(bit_depth)
    shapes = plane_shapes(w, h, cf)
    yx = [np.add.outer(np.arange(H), np.arange(W)) for H, W in shapes]
    return [("zeros", [np.zeros(s, dt) for s in shapes]), ("full", [np.full(s, M, dt) for s in shapes]),
            ("checker", [((g & 1) * M).astype(dt) for g in yx]), ("checker'", [(((g + 1) & 1) * M).astype(dt) for g in yx])]


# ---------------------------------------------------------------- what the GPU tests run (tests/test_gpu_filter.py)
SIZES = [(16, 8), (24, 16)]
DEPTHS = (8, 10)
# 15 taps with negative lobes, not symmetric (a filter applied backwards shows), the magnitudes sum to exactly 512
LOBES15 = [-8, -16, -24, -16, 0, 48, 80, 128, 80, 48, 0, -16, -24, -8, -16]
SKEW15 = [-128, 0, 0, 0, 0, 0, 0, 256, 0, 0, 0, 0, 0, 0, 128]
SKEW3 = [32, 128, 96]
assert taps_legal(LOBES15, SKEW15) and taps_legal(SKEW3, SKEW3)
assert sum(abs(k) for k in LOBES15) == 512 and sum(abs(k) for k in SKEW15) == 512
# (name, luma (h, v), chroma (h, v)) of the CONVOLVE cases
CONVOLVE_SETS = [
    ("binomial 3", (binomial(3), binomial(3)), (binomial(3), binomial(3))),
    ("binomial 5", (binomial(5), binomial(5)), (binomial(5), binomial(3))),
    ("binomial 9", (binomial(9), binomial(9)), (binomial(9), binomial(9))),
    ("box 7 x 3", (box(7), box(3)), (box(7), box(3))),
    ("skew 3 x 1", (SKEW3, [256]), ([256], SKEW3)),
    ("lobes 15 x 15", (LOBES15, SKEW15), (SKEW15, LOBES15)),
]


def unsharp_cases(bit_depth):
    """(name, keyword arguments of pics_filter / filter_pic) of the UNSHARP cases"""
    M = (1 << bit_depth) - 1
    b3, b5 = (binomial(3), binomial(3)), (binomial(5), binomial(5))
    return [("plus", dict(luma=b3, chroma=b3, amount=64, threshold=0)),
            ("plus, threshold", dict(luma=b5, chroma=b3, amount=(96, 64), threshold=(M // 8, M // 6))),
            ("minus", dict(luma=b3, chroma=b5, amount=-64, threshold=0)),
            ("minus, threshold", dict(luma=b3, chroma=b3, amount=(-32, -64), threshold=M // 8)),
            ("most", dict(luma=(LOBES15, SKEW15), chroma=(SKEW15, LOBES15), amount=512, threshold=(1, 0)))]


def temporal_thresholds(bit_depth):
    """(luma, chroma) threshold pairs of the TEMPORAL cases: above the noise of related_triplet (9 x 2), far below independent planes"""
    M = (1 << bit_depth) - 1
    return [(18, 24), (0, 9 * M), (M, 40)]


def source_seed(bit_depth, w, h, cf):
    """the seed of random_planes for the sources of the per-mode GPU tests"""
    return bit_depth * 10000 + w * 100 + h * 4 + cf
