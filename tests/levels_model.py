"""numpy model of oh_pics_histogram, oh_pics_lut and their host-only helpers (include/ohevc_hip.h): the histogram of a
plane's window with the fields derived from it, percentile and distance, every table builder in Python integers, and the application
of a table.  The GPU tests compare with it bit for bit; tests/test_levels_host.py checks it against a per-sample restatement and the C
helpers against it."""
import numpy as np

BINS = 4096
DEPTHS = (8, 9, 10, 12)


def shifts(cf, c):
    """(hshift, vshift) of plane c at chroma format cf"""
    return (1 if c and cf in (1, 2) else 0, 1 if c and cf == 1 else 0)


def plane_window(plane, cf, c, window):
    """plane c's part of the luma window (left, right, top, bottom)"""
    hs, vs = shifts(cf, c)
    left, right, top, bottom = window
    h, w = plane.shape
    return plane[top >> vs:h - (bottom >> vs), left >> hs:w - (right >> hs)]


class PlaneHist:
    def __init__(self, hist):
        """from the BINS counts: everything else follows, in Python integers"""
        self.hist = np.asarray(hist, dtype=np.uint32)
        assert self.hist.shape == (BINS,)
        c = [int(v) for v in self.hist]
        present = [v for v in range(BINS) if c[v]]
        self.samples = sum(c)
        self.sum = sum(v * c[v] for v in present)
        self.sum_sq = sum(v * v * c[v] for v in present)
        self.min = present[0] if present else 0
        self.max = present[-1] if present else 0

    def fields(self):
        return (self.samples, self.sum, self.sum_sq, self.min, self.max)


def plane_hist(samples):
    """the PlaneHist of an array of samples; None: a plane the picture lacks"""
    if samples is None:
        return PlaneHist(np.zeros(BINS, dtype=np.uint32))
    return PlaneHist(np.bincount(np.asarray(samples, dtype=np.int64).reshape(-1), minlength=BINS))


def histogram(planes, cf, window=(0, 0, 0, 0)):
    """[PlaneHist] * 3 of a picture's coded planes (one or three) over the luma window"""
    return [plane_hist(plane_window(planes[c], cf, c, window) if c < len(planes) else None) for c in range(3)]


def pooled(hists):
    c = [0] * BINS
    for h in hists:
        for v in np.nonzero(h.hist)[0]:
            c[int(v)] += int(h.hist[v])
    return c


def percentile(hists, ppm):
    """the smallest v with cum(v) > 0 and cum(v) 10^6 >= ppm N; None: no samples"""
    c = pooled(hists)
    N = sum(c)
    if not N or not 0 <= ppm <= 10 ** 6 or not hists:
        return None
    cum = 0
    for v in range(BINS):
        cum += c[v]
        if cum and cum * 10 ** 6 >= ppm * N:
            return v


def distance(a, b):
    return int(np.abs(a.hist.astype(np.int64) - b.hist.astype(np.int64)).sum())


def _table(values):
    return np.array(values, dtype=np.uint16)


def lut_identity(bs, bd):
    s, Md = bs - bd, (1 << bd) - 1
    return _table([v << -s if s <= 0 else min((v + (1 << (s - 1))) >> s, Md) for v in range(1 << bs)])


def lut_range(bs, bd, to_full, chroma):
    Ms, Md, ks, kd = (1 << bs) - 1, (1 << bd) - 1, 1 << (bs - 8), 1 << (bd - 8)
    out = []
    for v in range(Ms + 1):
        if to_full and not chroma:
            c = min(max(v, 16 * ks), 235 * ks) - 16 * ks
            o = (c * Md + (219 * ks >> 1)) // (219 * ks)
        elif to_full:
            d = min(max(v, 16 * ks), 240 * ks) - 128 * ks
            m = (abs(d) * Md + 112 * ks) // (224 * ks)
            o = min(max((1 << (bd - 1)) + (-m if d < 0 else m), 0), Md)
        elif not chroma:
            o = 16 * kd + (v * 219 * kd + (Ms >> 1)) // Ms
        else:
            d = v - (1 << (bs - 1))
            m = (abs(d) * 224 * kd + (Ms >> 1)) // Ms
            o = min(max(128 * kd + (-m if d < 0 else m), 16 * kd), 240 * kd)
        out.append(o)
    return _table(out)


def lut_linear(bs, bd, gain_q16, pivot_in, pivot_out):
    Md = (1 << bd) - 1
    return _table([min(max(((v - pivot_in) * gain_q16 + pivot_out * 65536 + 32768) >> 16, 0), Md) for v in range(1 << bs)])


def lut_stretch(hists, lo_ppm, hi_ppm, bd):
    """None: refused"""
    if lo_ppm + hi_ppm >= 10 ** 6:
        return None
    lo, hi = percentile(hists, lo_ppm), percentile(hists, 10 ** 6 - hi_ppm)
    if lo is None:
        return None
    M = (1 << bd) - 1
    if hi <= lo:
        return _table(range(M + 1))
    return _table([((min(max(v, lo), hi) - lo) * M + ((hi - lo) >> 1)) // (hi - lo) for v in range(M + 1)])


def lut_equalise(hists, bd):
    c = pooled(hists)
    N, M = sum(c), (1 << bd) - 1
    cmin = next((n for n in c if n), 0)
    if N == cmin:
        return _table(range(M + 1))
    out, cum = [], 0
    for v in range(M + 1):
        cum += c[v]
        out.append(0 if cum < cmin else ((cum - cmin) * M + ((N - cmin) >> 1)) // (N - cmin))
    return _table(out)


def lut_then(first, second):
    """None: an entry of first is outside second"""
    first, second = np.asarray(first), np.asarray(second)
    if not first.size or not second.size or int(first.max()) >= second.size:
        return None
    return second[first].astype(np.uint16)


def apply(planes, tables, mask, dbd):
    """the coded planes of the destination: plane c through tables[c] where bit c of mask is set, else a copy"""
    dt = np.uint16 if dbd > 8 else np.uint8
    return [np.asarray(tables[c])[pl.astype(np.int64)].astype(dt) if mask >> c & 1 else pl.astype(dt) for c, pl in enumerate(planes)]


# ---- the planes the GPU tests count and map: named so that the host suite can check what they reach ----
def content(kind, shape, bd, rng, start=0):
    """a plane of `kind`: "random" (with 0 and M present), "zero", "top" (all M), "ramp" (every value in turn from `start`, as far as
    the plane reaches), "flat" (one value in the middle of the range), "sparse" (random multiples of 3: two of every three bins stay
    empty)"""
    M = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    n = shape[0] * shape[1]
    if kind == "random":
        v = rng.integers(0, M + 1, n)
        v[rng.permutation(n)[:2]] = (0, M)
    elif kind == "zero":
        v = np.zeros(n, dtype=np.int64)
    elif kind == "top":
        v = np.full(n, M)
    elif kind == "ramp":
        v = (np.arange(n) + start) % (M + 1)
    elif kind == "flat":
        v = np.full(n, M // 2 + 1)
    elif kind == "sparse":
        v = rng.integers(0, M // 3 + 1, n) * 3
    else:
        raise ValueError(kind)
    return v.astype(dt).reshape(shape)
