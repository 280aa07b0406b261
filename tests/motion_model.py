"""The numpy model of the motion service (include/ohevc_hip.h): P(mv) for luma and chroma as H.265 8.5.3.3.3 defines the
uni-predicted samples, the three-stage block search with the key order (cost, d, mvy, mvx), the compensation of a whole picture,
motion_scale, the content generators and the cases that the GPU tests run (tests/test_motion_host.py asserts on the CPU what they
reach).  Everything is integer arithmetic in int64; tests/test_motion_host.py holds predict() against the oracle's oh_or_mc_uni."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from filter_model import plane_shapes, random_planes, sample_dtype                    # noqa: F401  (re-exported to the tests)

MAX_RANGE, MAX_CENTRE, MAX_LAMBDA = 32, 4096, 4096
QPEL = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]], dtype=np.int64)
EPEL = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4],
                 [-2, 10, 58, -2]], dtype=np.int64)
VECTOR = np.dtype([("x", np.int16), ("y", np.int16), ("sad", np.uint32), ("sad_centre", np.uint32)])


# ---------------------------------------------------------------- prediction
def sample_from_window(win, fx, fy, bd):
    """one predicted sample from its taps x taps window (taps = 8: luma, fractions in quarters; 4: chroma, in eighths), the scalar
    restatement that oh_motion_qpel / oh_motion_epel are held against"""
    win = np.asarray(win, dtype=np.int64)
    taps = win.shape[0]
    T, b = (QPEL if taps == 8 else EPEL), taps // 2 - 1
    if not fx and not fy:
        v = int(win[b, b]) << (14 - bd)
    elif not fy:
        v = int((T[fx] * win[b]).sum()) >> (bd - 8)
    elif not fx:
        v = int((T[fy] * win[:, b]).sum()) >> (bd - 8)
    else:
        rows = [int((T[fx] * win[j]).sum()) >> (bd - 8) for j in range(taps)]
        assert all(-32768 <= r <= 32767 for r in rows)
        v = sum(int(T[fy][j]) * rows[j] for j in range(taps)) >> 6
    shift = 14 - bd
    return min(max((v + (1 << (shift - 1))) >> shift, 0), (1 << bd) - 1)


def window(ref, xi, yi, w, h, taps):
    """the (h + taps - 1) x (w + taps - 1) reference samples around the rectangle whose first sample refers to (xi, yi), clamped to the
    plane, and how many of them lay outside it"""
    H, W = ref.shape
    b = taps // 2 - 1
    ys, xs = np.arange(yi - b, yi - b + h + taps - 1), np.arange(xi - b, xi - b + w + taps - 1)
    outside = (h + taps - 1) * (w + taps - 1) - int(((ys >= 0) & (ys < H)).sum()) * int(((xs >= 0) & (xs < W)).sum())
    return np.asarray(ref)[np.ix_(np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1))].astype(np.int64), outside


def predict(ref, xi, yi, w, h, fx, fy, bd, taps=8):
    """P: the w x h predicted samples of the rectangle whose first sample refers to (xi, yi) of the plane ref, with fractions (fx, fy)"""
    win, _ = window(ref, xi, yi, w, h, taps)
    T, b = (QPEL if taps == 8 else EPEL), taps // 2 - 1
    if not fx and not fy:
        v = win[b:b + h, b:b + w] << (14 - bd)
    elif not fy:
        v = sum(T[fx][k] * win[b:b + h, k:k + w] for k in range(taps)) >> (bd - 8)
    elif not fx:
        v = sum(T[fy][k] * win[k:k + h, b:b + w] for k in range(taps)) >> (bd - 8)
    else:
        rows = sum(T[fx][k] * win[:, k:k + w] for k in range(taps)) >> (bd - 8)
        assert rows.min() >= -32768 and rows.max() <= 32767             # the reference keeps them in int16
        v = sum(T[fy][k] * rows[k:k + h] for k in range(taps)) >> 6
    shift = 14 - bd
    return np.clip((v + (1 << (shift - 1))) >> shift, 0, (1 << bd) - 1)


def predict_luma(ref, x0, y0, w, h, mvx, mvy, bd):
    return predict(ref, x0 + (mvx >> 2), y0 + (mvy >> 2), w, h, mvx & 3, mvy & 3, bd, 8)


def predict_chroma(ref, xc, yc, wc, hc, mvx, mvy, hs, vs, bd):
    return predict(ref, xc + (mvx >> (2 + hs)), yc + (mvy >> (2 + vs)), wc, hc, (mvx & ((4 << hs) - 1)) << (1 - hs),
                   (mvy & ((4 << vs) - 1)) << (1 - vs), bd, 4)


# ---------------------------------------------------------------- blocks, cost, key
def blocks(width, height, block):
    return -(-width // block), -(-height // block)


def rect(W, H, block, bx, by):
    x0, y0 = bx * block, by * block
    return x0, y0, min(block, W - x0), min(block, H - y0)


def cost(sad, mvx, mvy, cx, cy, lam):
    d = abs(mvx - 4 * cx) + abs(mvy - 4 * cy)
    return sad + ((lam * d) >> 2)


def key(sad, mvx, mvy, cx, cy, lam):
    return (cost(sad, mvx, mvy, cx, cy, lam), abs(mvx - 4 * cx) + abs(mvy - 4 * cy), mvy, mvx)


def _decided_by(keys):
    """which component of the key separates the smallest of the keys from the runner-up (0 cost .. 3 mvx; one candidate: 0)"""
    if len(keys) < 2:
        return 0
    a, b = sorted(keys)[:2]
    return next(i for i in range(4) if a[i] != b[i])


def search_block(cur, ref, x0, y0, w, h, centre, rng_xy, subpel, lam, bd, stats=None):
    """(mvx, mvy, sad, sad_centre) of one block.  stats, a dict of counters, learns which stage's candidate won (the fraction class of
    the winner), which component of the key decided stage 0, and how many stage-0 candidates read beyond the plane"""
    H, W = ref.shape
    cx, cy = int(centre[0]), int(centre[1])
    rx, ry = rng_xy
    cb = np.asarray(cur)[y0:y0 + h, x0:x0 + w].astype(np.int64)
    ys = np.clip(np.arange(y0 + cy - ry, y0 + cy + ry + h), 0, H - 1)
    xs = np.clip(np.arange(x0 + cx - rx, x0 + cx + rx + w), 0, W - 1)
    views = sliding_window_view(np.asarray(ref)[np.ix_(ys, xs)].astype(np.int64), (h, w))          # [j][i]: displacement (i - rx, j - ry)
    sads = np.abs(views - cb).sum(axis=(2, 3))
    keys = [key(int(sads[j, i]), 4 * (cx + i - rx), 4 * (cy + j - ry), cx, cy, lam) for j in range(2 * ry + 1) for i in range(2 * rx + 1)]
    best = min(keys)
    sad_centre = int(sads[ry, rx])
    if stats is not None:
        stats["decided", _decided_by(keys)] = stats.get(("decided", _decided_by(keys)), 0) + 1
        ax, ay = x0 + cx - rx, y0 + cy - ry                                   # the first sample the stage reads; the last is w + 2 rx - 1 further
        inside_x = sum(1 for i in range(2 * rx + 1) if ax + i >= 0 and ax + i + w <= W)
        inside_y = sum(1 for j in range(2 * ry + 1) if ay + j >= 0 and ay + j + h <= H)
        stats["clamped"] = stats.get("clamped", 0) + len(keys) - inside_x * inside_y
        stats["candidates"] = stats.get("candidates", 0) + len(keys)
    for s in range(1, subpel + 1):
        step, bx, by = 3 - s, best[3], best[2]
        cands = []
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                mvx, mvy = bx + step * i, by + step * j
                sad = int(np.abs(cb - predict_luma(ref, x0, y0, w, h, mvx, mvy, bd)).sum())
                cands.append(key(sad, mvx, mvy, cx, cy, lam))
        best = min(cands)
    mvx, mvy = best[3], best[2]
    if stats is not None:
        stage = 2 if (mvx | mvy) & 1 else 1 if (mvx | mvy) & 2 else 0
        stats["stage", stage] = stats.get(("stage", stage), 0) + 1
    return mvx, mvy, best[0] - ((lam * best[1]) >> 2), sad_centre


def search(cur, ref, bd, block=16, rng_xy=(8, 8), subpel=2, lam=0, centres=None, stats=None):
    """the field of one pair of luma planes: a structured array (bh, bw) of VECTOR; centres: None or (bh, bw, 2)"""
    H, W = ref.shape
    bw, bh = blocks(W, H, block)
    out = np.zeros((bh, bw), dtype=VECTOR)
    for by in range(bh):
        for bx in range(bw):
            x0, y0, w, h = rect(W, H, block, bx, by)
            c = (0, 0) if centres is None else centres[by, bx]
            out[by, bx] = search_block(cur, ref, x0, y0, w, h, c, rng_xy, subpel, lam, bd, stats)
    return out


# ---------------------------------------------------------------- compensation
def field_xy(field):
    """(bh, bw, 2) int64 of a field given as VECTOR or as (x, y) pairs"""
    f = np.asarray(field)
    if f.dtype.names:
        return np.stack([f["x"], f["y"]], axis=-1).astype(np.int64)
    return f.astype(np.int64)


def compensate(planes, cf, bd, field, block=16):
    """the coded planes of the prediction of one picture (its coded planes) by a field (bh, bw) / (bh, bw, 2)"""
    xy = field_xy(field)
    H, W = planes[0].shape
    bw, bh = blocks(W, H, block)
    assert xy.shape == (bh, bw, 2)
    hs, vs = int(cf in (1, 2)), int(cf == 1)
    out = [np.zeros_like(p) for p in planes]
    for by in range(bh):
        for bx in range(bw):
            x0, y0, w, h = rect(W, H, block, bx, by)
            mvx, mvy = int(xy[by, bx, 0]), int(xy[by, bx, 1])
            out[0][y0:y0 + h, x0:x0 + w] = predict_luma(planes[0], x0, y0, w, h, mvx, mvy, bd)
            for c in range(1, len(planes)):
                xc, yc, wc, hc = x0 >> hs, y0 >> vs, w >> hs, h >> vs
                out[c][yc:yc + hc, xc:xc + wc] = predict_chroma(planes[c], xc, yc, wc, hc, mvx, mvy, hs, vs, bd)
    return out


# ---------------------------------------------------------------- coarse to fine
def motion_scale(coarse, block_c, s, grid, block_f):
    """the centres (bh, bw, 2) int16 of the grid = (bw, bh) of blocks of block_f from the field coarse (bhc, bwc) of blocks of block_c on
    pictures reduced by s"""
    xy = field_xy(coarse)
    bhc, bwc = xy.shape[:2]
    bw, bh = grid
    out = np.zeros((bh, bw, 2), dtype=np.int16)
    for by in range(bh):
        for bx in range(bw):
            v = xy[min(by * block_f // (s * block_c), bhc - 1), min(bx * block_f // (s * block_c), bwc - 1)]
            out[by, bx] = [min(max((s * int(k) + 2) >> 2, -MAX_CENTRE), MAX_CENTRE) for k in v]
    return out


# ---------------------------------------------------------------- content
def noise(bd, w, h, seed):
    return np.random.default_rng(seed).integers(0, 1 << bd, (h, w), dtype=sample_dtype(bd))


def smooth(bd, w, h, seed):
    """a plane without fine detail whose every block has structure: a sum of a few waves of random phase over a ramp"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = np.zeros((h, w))
    for _ in range(6):
        fx, fy, ph = rng.uniform(0.1, 0.45) * rng.choice([-1, 1]), rng.uniform(0.1, 0.45), rng.uniform(0, 6.28)
        v += np.sin(fx * x + fy * y + ph) * rng.uniform(0.5, 1.0)
    v = (v - v.min()) / (v.max() - v.min())
    return np.round(v * ((1 << bd) - 1)).astype(sample_dtype(bd))


def constant(bd, w, h, value):
    return np.full((h, w), value, dtype=sample_dtype(bd))


def random_field(w, h, block, lo, hi, seed):
    """a field (bh, bw, 2) of quarter-sample vectors with components in lo .. hi"""
    bw, bh = blocks(w, h, block)
    return np.random.default_rng(seed).integers(lo, hi + 1, (bh, bw, 2)).astype(np.int64)


def planted(bd, w, h, block, seed, reach=(2, 1)):
    """(cur, ref, field): ref smooth, cur the model's compensation of ref by a random quarter-sample field within reach = (x, y) whole
    samples and three quarters, so every block of cur is predicted without error by its vector of the field"""
    ref = smooth(bd, w, h, seed)
    bw, bh = blocks(w, h, block)
    rng = np.random.default_rng(seed + 1)
    field = np.stack([rng.integers(-(4 * reach[0] + 3), 4 * reach[0] + 4, (bh, bw)), rng.integers(-(4 * reach[1] + 3), 4 * reach[1] + 4, (bh, bw))],
                     axis=-1).astype(np.int64)
    return compensate([ref], 0, bd, field, block)[0], ref, field


def interior(w, h, block, rng_xy):
    """(bh, bw) bool: the blocks none of whose candidates, whatever the stage, reads beyond the plane (centres zero)"""
    bw, bh = blocks(w, h, block)
    m = np.zeros((bh, bw), dtype=bool)
    for by in range(bh):
        for bx in range(bw):
            x0, y0, bw_, bh_ = rect(w, h, block, bx, by)
            m[by, bx] = (x0 - rng_xy[0] - 4 >= 0 and y0 - rng_xy[1] - 4 >= 0 and x0 + bw_ + rng_xy[0] + 4 <= w and y0 + bh_ + rng_xy[1] + 4 <= h)
    return m


def random_centres(w, h, block, reach, seed):
    bw, bh = blocks(w, h, block)
    return np.random.default_rng(seed).integers(-reach, reach + 1, (bh, bw, 2)).astype(np.int16)


def outside_centres(w, h, block, seed):
    """every centre at +-MAX_CENTRE in both components: wholly outside the picture, so every read clamps"""
    bw, bh = blocks(w, h, block)
    return (np.random.default_rng(seed).integers(0, 2, (bh, bw, 2)) * 2 - 1).astype(np.int16) * MAX_CENTRE


# ---------------------------------------------------------------- the cases of the GPU tests
SIZES = [(16, 8), (24, 16), (40, 24), (72, 40)]
DEPTHS = (8, 10, 12)
RANGES = [(0, 0), (1, 0), (3, 2), (8, 8), (32, 32)]
LAMBDAS = (0, 7, 4096)


def _case(name, w, h, bd, block, rng_xy, subpel, lam, centres, content):
    return dict(name=name, w=w, h=h, bd=bd, block=block, range=rng_xy, subpel=subpel, lam=lam, centres=centres, content=content)


def search_cases():
    """the cases of tests/test_gpu_motion.py, dictionaries of: name, w, h, bd, block, range, subpel, lam, centres (None, "random",
    "outside"), content ("noise", "planted", "flat", "opposed", "same")"""
    cases = []
    k = 0
    for w, h in SIZES:                                            # every size, depth and block size: noise, centres within +-6
        for bd in DEPTHS:
            for block in (8, 16):
                cases.append(_case("sizes", w, h, bd, block, (3, 2), k % 3, LAMBDAS[k % 3], "random" if k % 2 else None, "noise"))
                k += 1
    for rng_xy in RANGES[:4]:                                     # every range but the largest with every subpel, on blocks cut at both edges
        for subpel in (0, 1, 2):
            cases.append(_case("ranges", 24, 16, DEPTHS[k % 3], (8, 16)[k % 2], rng_xy, subpel, LAMBDAS[(k // 2) % 3], "random", "noise"))
            k += 1
    for bd, block, lam in ((8, 8, 0), (10, 16, 7), (12, 8, 4096)):    # the largest range, far beyond the picture: almost every read clamps
        cases.append(_case("beyond", 16, 8, bd, block, (32, 32), 2, lam, None, "noise"))
    for (w, h), bd, block in (((16, 8), 8, 16), ((40, 24), 10, 8), ((24, 16), 12, 16)):      # centres wholly outside
        cases.append(_case("outside", w, h, bd, block, (3, 2), 2, 7, "outside", "noise"))
    for (w, h), bd, block in (((72, 40), 8, 16), ((72, 40), 10, 8), ((40, 24), 12, 8)):       # a planted displacement
        cases.append(_case("planted", w, h, bd, block, (3, 2), 2, 0, None, "planted"))
    for bd, block in ((8, 8), (10, 8)):                             # candidates that tie in cost and in d: mvy, then mvx decides
        cases.append(_case("diagonal", 40, 24, bd, block, (3, 2), 2, 0, None, "diagonal"))
        cases.append(_case("stripes", 40, 24, bd, block, (3, 2), 2, 0, None, "stripes"))
    for bd, block, lam, rng_xy in ((8, 16, 0, (3, 2)), (10, 8, 7, (8, 8)), (12, 16, 4096, (1, 0))):
        cases.append(_case("flat", 24, 16, bd, block, rng_xy, 2, lam, "random", "flat"))      # every candidate ties in SAD
        cases.append(_case("opposed", 24, 16, bd, block, rng_xy, 2, lam, "random", "opposed"))
    for bd, block in ((8, 8), (10, 16)):
        cases.append(_case("same", 40, 24, bd, block, (3, 2), 2, 0, None, "same"))             # cur is ref
        cases.append(_case("same", 40, 24, bd, block, (3, 2), 2, 7, "random", "same"))
    return cases


# the smooth content of this seed is one on which the three greedy stages recover the planted vector of every interior block at every
# depth and block size of the planted cases, which tests/test_motion_host.py asserts on the model; not every seed gives that
PLANTED_SEED = 9700


def case_seed(i):
    return 9000 + 17 * i


def case_inputs(i, case):
    """(cur, ref, centres or None, planted field or None) of case i of search_cases()"""
    w, h, bd, block, seed = case["w"], case["h"], case["bd"], case["block"], case_seed(i)
    M = (1 << bd) - 1
    field = None
    if case["content"] == "noise":
        cur, ref = noise(bd, w, h, seed), noise(bd, w, h, seed + 1)
    elif case["content"] == "planted":
        cur, ref, field = planted(bd, w, h, block, PLANTED_SEED)
    elif case["content"] == "diagonal":                           # a sample depends on x + y alone: one to the right is one down
        v = np.random.default_rng(seed).integers(0, 1 << bd, w + h + 1, dtype=sample_dtype(bd))
        y, x = np.mgrid[0:h, 0:w]
        cur, ref = v[x + y + 1], v[x + y]
    elif case["content"] == "stripes":                            # columns of period two: one to the right is one to the left
        v = np.random.default_rng(seed).integers(0, 1 << bd, (h, 2), dtype=sample_dtype(bd))
        x = np.arange(w)
        cur, ref = v[:, (x + 1) % 2], v[:, x % 2]
    elif case["content"] == "flat":
        cur, ref = constant(bd, w, h, M // 3), constant(bd, w, h, M // 3 + 5)
    elif case["content"] == "opposed":
        cur, ref = constant(bd, w, h, M), constant(bd, w, h, 0)
    else:
        cur = ref = noise(bd, w, h, seed)
    centres = {None: None, "random": random_centres(w, h, block, 6, seed + 2), "outside": outside_centres(w, h, block, seed + 3)}[case["centres"]]
    return cur, ref, centres, field


def case_id(case):
    return "{name}-{w}x{h}-{bd}bit-B{block}-r{range[0]}x{range[1]}-s{subpel}-l{lam}-{centres}".format(**case)


_cache = {}


def case_result(i, case):
    """inputs and the model's field of case i, computed once and shared (the arrays are read-only)"""
    if i not in _cache:
        cur, ref, centres, field = case_inputs(i, case)
        stats = {}
        want = search(cur, ref, case["bd"], case["block"], case["range"], case["subpel"], case["lam"], centres, stats)
        for a in (cur, ref, want) + ((centres,) if centres is not None else ()):
            a.setflags(write=False)
        _cache[i] = (cur, ref, centres, field, want, stats)
    return _cache[i]


# fraction classes of compensation: one vector per pair of eighth-sample chroma fractions at 4:2:0 (which covers the 16 luma classes),
# each with a whole part of its own sign
def class_vectors():
    return [((fx if (fx + fy) % 2 else fx - 8 * (1 + fy % 3)), (fy if fx % 3 else fy + 8 * (fx % 5) - 16)) for fy in range(8) for fx in range(8)]
