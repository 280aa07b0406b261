"""Host tests of the filters (oh_pics_filter), no GPU: the numpy model of tests/filter_model.py against a per-sample
restatement of the definitions in include/ohevc_hip.h, properties of the model, the host-only helpers of the library
(openhevc_amd/csrc/pics_math.hip, which evaluate csrc/filter_common.h like the kernel) against the model, the int32 bound of legal
taps, and which branches the planes of tests/test_gpu_filter.py make the model take."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import filter_model as FM                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

MODES = (FM.CONVOLVE, FM.UNSHARP, FM.MEDIAN, FM.TEMPORAL)


# ---------------------------------------------------------------- 1. the definitions, sample by sample
def restated(mode, S, bit_depth, h=None, v=None, amount=0, threshold=0, P=None, N=None):
    """one plane by the text of include/ohevc_hip.h: lists of Python ints, nested loops, explicit clamps"""
    H, W = len(S), len(S[0])
    M = 2 ** bit_depth - 1

    def r(k):
        return min(max(k, 0), H - 1)

    def cx(k):
        return min(max(k, 0), W - 1)
    out = [[None] * W for _ in range(H)]
    if mode in (FM.CONVOLVE, FM.UNSHARP):
        nh, nv = len(h), len(v)
        tmp = [[0] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                for k in range(nh):
                    tmp[y][x] += h[k] * S[y][cx(x + k - nh // 2)]
        for y in range(H):
            for x in range(W):
                acc = 0
                for k in range(nv):
                    acc += v[k] * tmp[r(y + k - nv // 2)][x]
                b = min(max((acc + 32768) >> 16, 0), M)
                if mode == FM.CONVOLVE:
                    out[y][x] = b
                    continue
                d = S[y][x] - b
                if abs(d) <= threshold:
                    out[y][x] = S[y][x]
                else:
                    out[y][x] = min(max(S[y][x] + ((amount * d + 32) >> 6), 0), M)
    elif mode == FM.MEDIAN:
        for y in range(H):
            for x in range(W):
                nine = []
                for j in (-1, 0, 1):
                    for i in (-1, 0, 1):
                        nine.append(S[r(y + j)][cx(x + i)])
                nine.sort()
                out[y][x] = nine[4]
    else:
        for y in range(H):
            for x in range(W):
                mp = mn = 0
                for j in (-1, 0, 1):
                    for i in (-1, 0, 1):
                        mp += abs(P[r(y + j)][cx(x + i)] - S[r(y + j)][cx(x + i)])
                        mn += abs(N[r(y + j)][cx(x + i)] - S[r(y + j)][cx(x + i)])
                ps = P[y][x] if mp <= threshold else S[y][x]
                ns = N[y][x] if mn <= threshold else S[y][x]
                out[y][x] = (ps + 2 * S[y][x] + ns + 2) >> 2
    return out


@pytest.mark.parametrize("bd", (8, 10))
@pytest.mark.parametrize("shape", ((5, 7), (1, 9), (6, 1), (9, 12)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_against_the_restated_definitions(bd, shape):
    """every mode on small planes, narrower and lower than the longest taps among them"""
    rng = np.random.default_rng(bd * 31 + shape[0])
    M = (1 << bd) - 1
    S, P, N = (rng.integers(0, M + 1, shape) for _ in range(3))
    P[:, : shape[1] // 2] = S[:, : shape[1] // 2]                            # so that the temporal sums fall on both sides
    N[: shape[0] // 2] = np.clip(S[: shape[0] // 2] + rng.integers(-1, 2, (shape[0] // 2, shape[1])), 0, M)
    Sl, Pl, Nl = (a.tolist() for a in (S, P, N))
    for name, (h, v), _ in FM.CONVOLVE_SETS:
        assert FM.convolve_plane(S, h, v, bd).tolist() == restated(FM.CONVOLVE, Sl, bd, h, v), name
    for (h, v), amount, thr in (((FM.binomial(3), FM.binomial(5)), 64, 0), ((FM.SKEW3, FM.box(5)), -64, 3), ((FM.LOBES15, FM.SKEW15), 512, 1),
                                ((FM.binomial(9), FM.SKEW3), 37, M // 10)):
        assert FM.unsharp_plane(S, h, v, amount, thr, bd).tolist() == restated(FM.UNSHARP, Sl, bd, h, v, amount, thr), (amount, thr)
    assert FM.median_plane(S).tolist() == restated(FM.MEDIAN, Sl, bd)
    for thr in (0, 9, M, 9 * M):
        assert FM.temporal_plane(P, S, N, thr).tolist() == restated(FM.TEMPORAL, Sl, bd, threshold=thr, P=Pl, N=Nl), thr


def test_filter_pic_takes_the_class_of_each_plane():
    """luma with taps[0], amount[0], threshold[0]; both chroma planes with index 1; planes not selected are the source"""
    bd = 10
    src = FM.random_planes(bd, 12, 6, 2, 5)
    kw = dict(luma=(FM.SKEW3, FM.binomial(5)), chroma=(FM.box(5), FM.SKEW3), amount=(80, -20), threshold=(4, 9))
    got = FM.filter_pic(src, FM.UNSHARP, bd, planes=5, **kw)
    assert got[0].tolist() == restated(FM.UNSHARP, src[0].tolist(), bd, FM.SKEW3, FM.binomial(5), 80, 4)
    assert np.array_equal(got[1], src[1]) and got[1].dtype == src[1].dtype
    assert got[2].tolist() == restated(FM.UNSHARP, src[2].tolist(), bd, FM.box(5), FM.SKEW3, -20, 9)


# ---------------------------------------------------------------- 2. properties
@pytest.mark.parametrize("bd", (8, 10, 12))
def test_copies_and_fixed_points(bd):
    M = (1 << bd) - 1
    src = FM.random_planes(bd, 14, 10, 1, bd)
    P, _, N = FM.related_triplet(bd, 14, 10, 1)
    one = ([256], [256])

    def same(got):
        return all(np.array_equal(a, b) for a, b in zip(got, src))
    assert same(FM.filter_pic(src, FM.CONVOLVE, bd, luma=one, chroma=one))
    assert same(FM.filter_pic(src, FM.UNSHARP, bd, amount=0))
    assert same(FM.filter_pic(src, FM.UNSHARP, bd, luma=one, chroma=one, amount=512))
    for mode in MODES:
        assert same(FM.filter_pic(src, mode, bd, planes=0, threshold=M, prev=P, nxt=N)), mode
    assert same(FM.filter_pic(src, FM.TEMPORAL, bd, threshold=9 * M))                       # P = C = N
    assert same(FM.filter_pic(src, FM.TEMPORAL, bd, threshold=0, prev=src, nxt=src))
    for value in (0, 1, M // 2, M):
        flat = [np.full(s, value, FM.sample_dtype(bd)) for s in FM.plane_shapes(14, 10, 1)]
        for mode in MODES:
            for kw in (dict(), dict(luma=(FM.LOBES15, FM.SKEW15), chroma=(FM.box(15), FM.box(7)), amount=512)):
                got = FM.filter_pic(flat, mode, bd, **kw)
                assert all(np.array_equal(a, b) for a, b in zip(got, flat)), (value, mode)


def test_one_vertical_tap_is_the_horizontal_filter():
    bd = 10
    S = FM.random_planes(bd, 20, 6, 0, 3)[0].astype(np.int64)
    for h in (FM.binomial(5), FM.SKEW3, FM.LOBES15):
        want = np.empty_like(S)
        r = len(h) // 2
        for x in range(S.shape[1]):
            acc = sum(h[k] * S[:, min(max(x + k - r, 0), S.shape[1] - 1)] for k in range(len(h)))
            want[:, x] = np.clip((acc * 256 + 32768) >> 16, 0, 1023)
        assert np.array_equal(FM.convolve_plane(S, h, [256], bd), want)
        assert np.array_equal(FM.convolve_plane(S.T, [256], h, bd), want.T)


def test_median_removes_an_impulse():
    for bd, where in itertools.product((8, 10), ((0, 0), (3, 4), (5, 8), (0, 5))):
        M = (1 << bd) - 1
        S = np.full((6, 9), M // 3, FM.sample_dtype(bd))
        S[where] = M
        assert (FM.median_plane(S) == M // 3).all()
        S[where] = 0
        assert (FM.median_plane(S) == M // 3).all()


def test_temporal_at_the_largest_threshold_is_the_plain_average():
    for bd in (8, 10, 12):
        M = (1 << bd) - 1
        P, Cu, N = (FM.random_planes(bd, 10, 8, 0, s)[0].astype(np.int64) for s in (1, 2, 3))
        assert np.array_equal(FM.temporal_plane(P, Cu, N, 9 * M), (P + 2 * Cu + N + 2) >> 2)
        assert np.array_equal(FM.temporal_plane(Cu, Cu, Cu, 0), Cu)


# ---------------------------------------------------------------- 3. the library's host helpers
def test_tap_helpers():
    L = E.lib()
    want = {1: [256], 3: [64, 128, 64], 5: [16, 64, 96, 64, 16], 7: [4, 24, 60, 80, 60, 24, 4], 9: [1, 8, 28, 56, 70, 56, 28, 8, 1]}
    buf = (C.c_int16 * 16)()
    for n in range(-2, 18):
        buf[:] = [-7] * 16
        rc = L.oh_filter_binomial(n, buf)
        if n in want:
            assert rc == 0 and list(buf[:n]) == want[n] == FM.binomial(n) == E.filter_binomial(n) and buf[n] == -7
        else:
            assert rc == E.OH_E_ARG and list(buf) == [-7] * 16
            with pytest.raises(E.EngineError):
                E.filter_binomial(n)
        buf[:] = [-7] * 16
        rc = L.oh_filter_box(n, buf)
        if 1 <= n <= 15 and n % 2:
            assert rc == 0 and list(buf[:n]) == FM.box(n) == E.filter_box(n) and buf[n] == -7 and sum(buf[:n]) == 256
        else:
            assert rc == E.OH_E_ARG and list(buf) == [-7] * 16
    assert L.oh_filter_binomial(3, None) == E.OH_E_ARG and L.oh_filter_box(3, None) == E.OH_E_ARG


def raw_taps(nh, nv, h, v):
    t = E.OhFilterTaps(nh, nv)
    t.h[:len(h)] = h
    t.v[:len(v)] = v
    return t


def test_taps_check():
    L = E.lib()
    ok = [([256], [256]), (FM.binomial(9), FM.box(15)), (FM.LOBES15, FM.SKEW15), ([-128, 384, 0], [0, 0, 256]), ([128, 256, -128], [256])]
    for h, v in ok:
        assert FM.taps_legal(h, v) and L.oh_filter_taps_check(C.byref(raw_taps(len(h), len(v), h, v))) == 0, (h, v)
        assert list(E.filter_taps(h, v).h[:len(h)]) == h
    bad = [(2, 1, [128, 128], [256]),                                                   # an even count
           (1, 4, [256], [64, 64, 64, 64]),
           (0, 1, [], [256]), (1, 0, [256], []), (-1, 1, [256], [256]),                  # no taps
           (17, 1, [256], [256]), (1, 16, [256], [256]),                                # too many
           (3, 1, [64, 128, 63], [256]), (1, 3, [256], [64, 128, 65]),                   # the sum is not 256
           (3, 1, [0, 0, 0], [256]),
           (3, 1, [-129, 514, -129], [256]), (1, 3, [256], [-200, 456, 0]),              # the magnitudes pass 512
           (3, 3, [-128, 512, -128], [-129, 513, -128])]
    for nh, nv, h, v in bad:
        assert L.oh_filter_taps_check(C.byref(raw_taps(nh, nv, h, v))) == E.OH_E_ARG, (nh, nv, h, v)
        if 1 <= nh == len(h) and 1 <= nv == len(v):
            assert not FM.taps_legal(h, v)
            with pytest.raises(E.EngineError):
                E.filter_taps(h, v)
    assert L.oh_filter_taps_check(None) == E.OH_E_ARG
    # taps behind nh / nv are not read
    t = raw_taps(3, 1, [64, 128, 64] + [999] * 12, [256] + [-999] * 14)
    assert L.oh_filter_taps_check(C.byref(t)) == 0


def test_sample_helpers():
    L = E.lib()
    rng = np.random.default_rng(9)
    for bd in (8, 9, 10, 12):
        M = (1 << bd) - 1
        edge = [0, 1, M // 2, M - 1, M]
        # unsharp: the extremes of every argument, then random ones
        for s, b, amount, thr in itertools.product(edge, edge, (-64, -1, 0, 1, 64, 512), (0, 1, M // 2, M)):
            assert L.oh_filter_unsharp(s, b, amount, thr, M) == FM.unsharp_sample(s, b, amount, thr, M), (s, b, amount, thr)
        for _ in range(400):
            s, b, thr = (int(v) for v in rng.integers(0, M + 1, 3))
            amount = int(rng.integers(-64, 513))
            assert L.oh_filter_unsharp(s, b, amount, thr, M) == FM.unsharp_sample(s, b, amount, thr, M)
        # median: every pattern of 0 / M, then random values with many ties, then without
        for k in range(512):
            v = [M if k >> i & 1 else 0 for i in range(9)]
            assert L.oh_filter_median9((C.c_int32 * 9)(*v)) == FM.median9(v), v
        for hi in (3, M + 1):
            for _ in range(400):
                v = [int(x) for x in rng.integers(0, hi, 9)]
                assert L.oh_filter_median9((C.c_int32 * 9)(*v)) == FM.median9(v), v
        for v in itertools.islice(itertools.permutations(range(9)), 0, 362880, 997):
            assert L.oh_filter_median9((C.c_int32 * 9)(*v)) == 4
        # temporal
        for c, p, n, mp, mn, thr in itertools.product((0, M), (0, M), (0, M), (0, 9 * M), (0, 1, 9 * M), (0, 9 * M)):
            assert L.oh_filter_temporal(c, p, n, mp, mn, thr) == FM.temporal_sample(c, p, n, mp, mn, thr)
        for _ in range(400):
            c, p, n = (int(v) for v in rng.integers(0, M + 1, 3))
            mp, mn, thr = (int(v) for v in rng.integers(0, 9 * M + 1, 3))
            assert L.oh_filter_temporal(c, p, n, mp, mn, thr) == FM.temporal_sample(c, p, n, mp, mn, thr)
            assert L.oh_filter_temporal(c, p, n, thr, thr + 1, thr) == (p + 3 * c + 2) >> 2


def test_mode_names():
    assert [E.filter_mode(k) for k in ("convolve", "unsharp", "median", "temporal")] == [0, 1, 2, 3] == [E.filter_mode(i) for i in range(4)]
    assert (E.FILTER_CONVOLVE, E.FILTER_UNSHARP, E.FILTER_MEDIAN, E.FILTER_TEMPORAL) == MODES
    for bad in ("blur", 4, -1):
        with pytest.raises(ValueError):
            E.filter_mode(bad)
    assert C.sizeof(E.OhFilterTaps) == 68 and C.sizeof(E.OhFilter) == 8 + 2 * 68 + 16


# ---------------------------------------------------------------- 4. the int32 bound
def test_worst_case_taps_stay_inside_int32():
    """legal taps whose magnitudes sum to 512 on both axes over 12-bit planes built to push one sample as far as it goes either way"""
    M = 4095
    limit = (1 << 31) - (1 << 15)
    assert 512 * 512 * M < limit
    worst = 0
    for h, v in ((FM.SKEW15, FM.SKEW15), (FM.LOBES15, FM.SKEW15), (FM.LOBES15, FM.LOBES15), ([-128, 384, 0], [0, 384, -128])):
        assert sum(abs(k) for k in h) == 512 == sum(abs(k) for k in v)
        sign = np.sign(np.outer(v, h))
        for s in (1, -1):
            S = np.where(s * sign > 0, M, 0)                                # a window of the taps' size: its middle sample sees all of it
            acc = FM.convolve_acc(S, h, v)
            tmp = sum(int(k) * a for k, a in zip(h, FM._shifted(S.astype(np.int64), 0, len(h) // 2)))
            assert np.abs(tmp).max() <= 512 * M < 1 << 23                    # what the 24-bit multiplier takes
            mid = acc[len(v) // 2, len(h) // 2]
            assert mid == s * M * (512 * 512 + s * 256 * 256) // 2
            assert np.abs(acc).max() <= 512 * 512 * M
            worst = max(worst, int(np.abs(acc).max()))
            got = FM.convolve_plane(S, h, v, 12)
            assert got[len(v) // 2, len(h) // 2] == (M if s > 0 else 0)
    assert M * (512 * 512 + 256 * 256) // 2 <= worst < limit


# ---------------------------------------------------------------- 5. the branches the GPU tests' planes reach
@pytest.mark.parametrize("w,h", FM.SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("bd", FM.DEPTHS)
def test_gpu_planes_reach_every_branch(bd, w, h):
    M = (1 << bd) - 1
    for cf in range(4):
        src = FM.random_planes(bd, w, h, cf, FM.source_seed(bd, w, h, cf))
        # CONVOLVE with negative lobes clips at both ends (before the clip the value lies outside [0, M])
        name, luma, chroma = FM.CONVOLVE_SETS[-1]
        lo = hi = False
        for c, pl in enumerate(src):
            hh, vv = chroma if c else luma
            val = (FM.convolve_acc(pl, hh, vv) + 32768) >> 16
            lo, hi = lo or (val < 0).any(), hi or (val > M).any()
        assert lo and hi, (cf, "convolve", lo, hi)
        # UNSHARP: both sides of the threshold in every plane of the cases with one, the clip at both ends in the strongest case
        for name, kw in FM.unsharp_cases(bd):
            amount, thr = FM._pair(kw["amount"]), FM._pair(kw["threshold"])
            lo = hi = False
            for c, pl in enumerate(src):
                q = int(c > 0)
                taps = kw["chroma"] if c else kw["luma"]
                _, keep, raw = FM.unsharp_plane(pl, taps[0], taps[1], amount[q], thr[q], bd, detail=True)
                if "threshold" in name:
                    assert keep.any() and not keep.all(), (cf, name, c)
                lo, hi = lo or (~keep & (raw < 0)).any(), hi or (~keep & (raw > M)).any()
            if name == "most":
                assert lo and hi, (cf, name, lo, hi)
        # TEMPORAL: mp <= thr and mn <= thr true and false in every plane, with the first pair of thresholds
        P, Cu, N = FM.related_triplet(bd, w, h, cf)
        thr = FM.temporal_thresholds(bd)[0]
        for c in range(len(Cu)):
            mp, mn = FM.temporal_sums(P[c], Cu[c], N[c])
            t = thr[int(c > 0)]
            for m in (mp, mn):
                assert (m <= t).any() and (m > t).any(), (cf, c)
            # and where the choice matters: the sample taken differs from cur's on either side
            assert ((mp <= t) & (P[c] != Cu[c])).any() and ((mp > t) & (P[c] != Cu[c])).any(), (cf, c)
            assert ((mn <= t) & (N[c] != Cu[c])).any() and ((mn > t) & (N[c] != Cu[c])).any(), (cf, c)
