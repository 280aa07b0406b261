"""A numpy model of the colour remapping of DESIGN.md §3r (oh_pics_colour_remap and its host helpers), written from the definition and
not from the library's code: the piecewise-linear curve through pivots, the sample (pre tables, matrix, post tables), whole pictures,
and the per-plane tables of a diagonal matrix.  Everything is in Python ints or int64, so nothing wraps; the *_ints forms are plain
loops over Python ints that tests/test_remap_host.py holds the numpy forms to."""
import numpy as np

DEPTHS = (8, 9, 10, 12)


def points(bi, bo, pivots):
    """the points of a curve: the pivots, (0, 0) in front where the first coded value is above 0, (Mi, Mo) behind where the last is
    below Mi"""
    Mi, Mo = (1 << bi) - 1, (1 << bo) - 1
    pts = [(int(x), int(y)) for x, y in pivots]
    if not pts or pts[0][0] > 0:
        pts.insert(0, (0, 0))
    if pts[-1][0] < Mi:
        pts.append((Mi, Mo))
    return pts


def curve_ints(bi, bo, pivots):
    pts = points(bi, bo, pivots)
    out = [None] * (1 << bi)
    out[pts[0][0]] = pts[0][1]
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        dx = x1 - x0
        for v in range(x0, x1 + 1):
            t = v - x0
            out[v] = (y0 * (dx - t) + y1 * t + (dx >> 1)) // dx
    return out


def curve(bi, bo, pivots=()):
    """the table of 2^bi entries (uint16)"""
    pts = points(bi, bo, pivots)
    out = np.zeros(1 << bi, dtype=np.int64)
    out[pts[0][0]] = pts[0][1]
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        dx = x1 - x0
        t = np.arange(0, dx + 1, dtype=np.int64)
        out[x0:x1 + 1] = (y0 * (dx - t) + y1 * t + (dx >> 1)) // dx
    return out.astype(np.uint16)


def matrix(p, coeff, d, bo):
    """p: three int64 arrays of pre-table values -> the three clipped matrix results; also how many were clipped below and above"""
    Mo = (1 << bo) - 1
    r = 1 << (d - 1) if d else 0
    m, low, high = [], 0, 0
    for c in range(3):
        v = (int(coeff[c][0]) * p[0] + int(coeff[c][1]) * p[1] + int(coeff[c][2]) * p[2] + r) >> d          # floors: numpy's >> on int64
        low += int((v < 0).sum())
        high += int((v > Mo).sum())
        m.append(np.clip(v, 0, Mo))
    return m, low, high


def apply(planes, pre, coeff, d, post, bi, bo, counts=None):
    """three planes (or three arrays of any one shape) of bi bits -> three of bo bits.  pre (3, 2^bi), post (3, 2^bo).  A sample above
    Mi is looked up by its low bits.  counts: a list that gets (clipped below, clipped above)"""
    Mi = (1 << bi) - 1
    p = [np.asarray(pre[c], dtype=np.int64)[np.asarray(planes[c], dtype=np.int64) & Mi] for c in range(3)]
    m, low, high = matrix(p, coeff, d, bo)
    if counts is not None:
        counts.append((low, high))
    dt = np.uint16 if bo > 8 else np.uint8
    return [np.asarray(post[c], dtype=np.int64)[m[c]].astype(dt) for c in range(3)]


def sample_ints(s, pre, coeff, d, post, bi, bo):
    """one sample in Python ints"""
    Mi, Mo = (1 << bi) - 1, (1 << bo) - 1
    p = [int(pre[i][int(s[i]) & Mi]) for i in range(3)]
    r = 1 << (d - 1) if d else 0
    out = []
    for c in range(3):
        v = (sum(int(coeff[c][i]) * p[i] for i in range(3)) + r) >> d                                       # Python's >> floors
        out.append(int(post[c][min(max(v, 0), Mo)]))
    return tuple(out)


def luts(pre, coeff, d, post, bi, bo):
    """the per-plane tables (3, 2^bi) of a diagonal matrix; None for any other"""
    if any(coeff[c][i] for c in range(3) for i in range(3) if c != i):
        return None
    Mo = (1 << bo) - 1
    r = 1 << (d - 1) if d else 0
    out = np.zeros((3, 1 << bi), dtype=np.uint16)
    for c in range(3):
        v = (int(coeff[c][c]) * np.asarray(pre[c], dtype=np.int64) + r) >> d
        out[c] = np.asarray(post[c], dtype=np.int64)[np.clip(v, 0, Mo)]
    return out


def luts_ints(pre, coeff, d, post, bi, bo):
    Mo = (1 << bo) - 1
    r = 1 << (d - 1) if d else 0
    return [[int(post[c][min(max((int(coeff[c][c]) * int(pre[c][v]) + r) >> d, 0), Mo)]) for v in range(1 << bi)] for c in range(3)]


def random_pivots(rng, bi, bo, n):
    """n pivots with strictly increasing coded values over 0 .. Mi and any targets over 0 .. Mo"""
    Mi, Mo = (1 << bi) - 1, (1 << bo) - 1
    xs = np.sort(rng.choice(np.arange(Mi + 1), n, replace=False))
    return [(int(x), int(y)) for x, y in zip(xs, rng.integers(0, Mo + 1, n))]


def random_tables(rng, bi, bo):
    """pre (3, 2^bi) and post (3, 2^bo), random over the full output range"""
    return (rng.integers(0, 1 << bo, (3, 1 << bi)).astype(np.uint16), rng.integers(0, 1 << bo, (3, 1 << bo)).astype(np.uint16))


def random_matrix(rng, d):
    """a matrix of denominator 2^d with negative entries: a diagonal of about one, row 0 takes a whole component away and row 1 adds
    one, so that results fall below 0 and above Mo"""
    one = 1 << d
    k = rng.integers(-one, one + 1, (3, 3))
    k[np.arange(3), np.arange(3)] = one + rng.integers(-(one >> 1), (one >> 1) + 1, 3)
    k[0, 1], k[1, 2] = -one, one
    return np.clip(k, -32768, 32767).astype(np.int32)
