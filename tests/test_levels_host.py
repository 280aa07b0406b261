"""No GPU: the numpy model of tests/levels_model.py against a per-sample restatement in plain Python, the host-only helpers of
include/ohevc_hip.h (oh_hist_percentile, oh_hist_distance, the oh_lut_* builders) against the model over every pair of bit depths,
their argument rules, and what the planes of the GPU tests reach."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import levels_model as LM                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

DEPTHS = LM.DEPTHS
PAIRS = list(itertools.product(DEPTHS, DEPTHS))
ARG = E.OH_E_ARG


def to_e(mh, bd=12):
    """the model's PlaneHist as the binding's"""
    return E.PlaneHist(mh.samples, mh.sum, mh.sum_sq, mh.min, mh.max, mh.hist[:1 << bd])


def refused(fn, *args, **kw):
    with pytest.raises(E.EngineError) as ei:
        fn(*args, **kw)
    return ei.value.code == ARG


# ---- the model against a per-sample restatement ----
@pytest.mark.parametrize("cf", (0, 1, 2, 3))
def test_model_histogram_per_sample(cf):
    rng = np.random.default_rng(cf)
    W, H, bd = 12, 8, 10
    sw, sh = (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)
    planes = [rng.integers(0, 1 << bd, (H, W)).astype(np.uint16)]
    if cf:
        planes += [rng.integers(0, 1 << bd, (H // sh, W // sw)).astype(np.uint16) for _ in range(2)]
    for window in ((0, 0, 0, 0), (2, 4, 2, 0), (4, 0, 0, 6), (10, 0, 6, 0)):
        left, right, top, bottom = window
        got = LM.histogram(planes, cf, window)
        for c in range(3):
            count = [0] * LM.BINS
            if c < len(planes):
                dx, dy = (sw, sh) if c else (1, 1)
                for y in range(top // dy, (H - bottom) // dy):
                    for x in range(left // dx, (W - right) // dx):
                        count[int(planes[c][y][x])] += 1
            assert [int(v) for v in got[c].hist] == count, (window, c)
            vals = [v for v in range(LM.BINS) for _ in range(count[v])]
            want = (len(vals), sum(vals), sum(v * v for v in vals), min(vals, default=0), max(vals, default=0))
            assert got[c].fields() == want, (window, c)
        assert got[0].samples == (W - left - right) * (H - top - bottom)


def test_model_percentile_distance_apply_per_sample():
    rng = np.random.default_rng(5)
    vals = sorted(int(v) for v in rng.integers(3, 200, 37))
    h = LM.plane_hist(np.array(vals))
    for ppm in (0, 1, 250000, 500000, 999999, 10 ** 6):
        # the smallest value such that at least ppm millionths of the samples are at or below it (and at least one)
        need = max(1, -(-ppm * len(vals) // 10 ** 6))
        assert LM.percentile([h], ppm) == vals[need - 1], ppm
    assert LM.percentile([h], 0) == vals[0] and LM.percentile([h], 10 ** 6) == vals[-1]
    assert LM.percentile([h, h], 500000) == LM.percentile([h], 500000)
    assert LM.percentile([LM.plane_hist(None)], 0) is None
    other = LM.plane_hist(np.array(vals[:20] + [4000] * 17))
    assert LM.distance(h, other) == sum(abs(vals.count(v) - (vals[:20] + [4000] * 17).count(v)) for v in range(LM.BINS))
    assert LM.distance(h, h) == 0
    planes = [rng.integers(0, 256, (4, 6)).astype(np.uint8) for _ in range(3)]
    tabs = [rng.integers(0, 1024, 256).astype(np.uint16) for _ in range(3)]
    out = LM.apply(planes, tabs, 5, 10)
    for c in range(3):
        assert out[c].dtype == np.uint16
        for y, x in itertools.product(range(4), range(6)):
            assert out[c][y][x] == (tabs[c][planes[c][y][x]] if c != 1 else planes[c][y][x])


# ---- the C builders against the model, every pair of depths ----
@pytest.mark.parametrize("bs,bd", PAIRS, ids=[f"{a}to{b}" for a, b in PAIRS])
def test_builders_against_model(bs, bd):
    Ms, Md, ks, kd = (1 << bs) - 1, (1 << bd) - 1, 1 << (bs - 8), 1 << (bd - 8)
    ident = E.lut_identity(bs, bd)
    assert ident.dtype == np.uint16 and ident.shape == (Ms + 1,)
    assert np.array_equal(ident, LM.lut_identity(bs, bd))
    for v in (0, 1, Ms // 2, Ms - 1, Ms):                                   # the whole table: test_identity_is_reformat_quantise
        assert ident[v] == E.reformat_quantise(v, bs - bd, "round", 0, 0, bd)
    for to_full, chroma in itertools.product((False, True), (False, True)):
        t = E.lut_range(bs, bd, to_full, chroma)
        assert np.array_equal(t, LM.lut_range(bs, bd, to_full, chroma)), (to_full, chroma)
        assert int(t.max()) <= Md and np.all(np.diff(t.astype(np.int64)) >= 0)
    # end points map to end points.  Full-range chroma is not symmetric about its middle (Ms - 2^(bs-1) is half a step short of
    # 2^(bs-1)), so its top arrives up to ceil(112 kd / Ms) below 240 kd; the bottom is held by the clamp
    full_y, full_c = E.lut_range(bs, bd, True, False), E.lut_range(bs, bd, True, True)
    lim_y, lim_c = E.lut_range(bs, bd, False, False), E.lut_range(bs, bd, False, True)
    assert (full_y[16 * ks], full_y[235 * ks], full_y[0], full_y[Ms]) == (0, Md, 0, Md)
    assert (full_c[16 * ks], full_c[128 * ks], full_c[240 * ks], full_c[0], full_c[Ms]) == (0, 1 << (bd - 1), Md, 0, Md)
    assert (lim_y[0], lim_y[Ms]) == (16 * kd, 235 * kd)
    assert (lim_c[0], lim_c[1 << (bs - 1)]) == (16 * kd, 128 * kd)
    assert 240 * kd - -(-112 * kd // Ms) <= lim_c[Ms] <= 240 * kd
    cases = [(65536, 0, 0), (-65536, 0, Md), (-65536, Ms, 0), (131072, Ms // 2, Md // 2), (1, 0, 0), (-1, 5, 7), (2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1),
             (-2 ** 31, 2 ** 31 - 1, -2 ** 31), (2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31), (-2 ** 31, -2 ** 31, 2 ** 31 - 1), (0, 3, Md), (40000, 17, -3)]
    for gain, pi, po in cases:
        assert np.array_equal(E.lut_linear(bs, bd, gain, pi, po), LM.lut_linear(bs, bd, gain, pi, po)), (gain, pi, po)
    if bs == bd:
        inv = E.lut_linear(bs, bd, -65536, 0, Md)
        assert np.array_equal(inv, Md - np.arange(Ms + 1)) and np.array_equal(E.lut_then(inv, inv), np.arange(Ms + 1))
        assert np.array_equal(E.lut_linear(bs, bd, 65536), ident)
        # The round trips at equal depth.  Limited range has 219 ks + 1 luma codes (224 ks + 1 chroma codes) for the 2^bs of full range,
        # so full -> limited -> full cannot be the identity for any table (two full-range values must share a limited code); what the
        # formulas give is the identity the other way round, on the legal codes, and a full -> limited -> full that moves a value by at
        # most one code: the limited code is at most half a limited step (255/219 or 255/224 of a full one: below 0.59) from v, and the
        # way back rounds by at most half a code more — below 1.09, so at most 1 in integers.
        v = np.arange(Ms + 1)
        legal_y, legal_c = v[16 * ks:235 * ks + 1], v[16 * ks:240 * ks + 1]
        assert np.array_equal(E.lut_then(full_y, lim_y)[legal_y], legal_y)
        assert np.array_equal(E.lut_then(full_c, lim_c)[legal_c], legal_c)
        for back in (E.lut_then(lim_y, full_y), E.lut_then(lim_c, full_c)):
            d = np.abs(back.astype(np.int64) - v)
            print(f"{bs} bit: full -> limited -> full moves {np.count_nonzero(d)} of {Ms + 1} values, by at most {d.max()}")
            assert d.max() == 1 and back[0] == 0 and back[Ms] == Ms


@pytest.mark.parametrize("bs,bd", PAIRS, ids=[f"{a}to{b}" for a, b in PAIRS])
def test_identity_is_reformat_quantise(bs, bd):
    ident = E.lut_identity(bs, bd)
    L = E.lib()
    assert [int(v) for v in ident] == [L.oh_reformat_quantise(v, bs - bd, 0, 0, 0, bd) for v in range(1 << bs)]


def shapes(bd):
    """histograms with empty bins, of a single value, and of a full ramp, as model PlaneHist"""
    M = (1 << bd) - 1
    rng = np.random.default_rng(bd)
    return {"empty bins": LM.plane_hist(LM.content("sparse", (16, 32), bd, rng)), "single": LM.plane_hist(np.full(100, M // 3)),
            "ramp": LM.plane_hist(np.arange(M + 1)), "two ends": LM.plane_hist(np.array([0] * 7 + [M])),
            "skewed": LM.plane_hist(np.minimum(rng.geometric(0.05, 5000) + 3, M))}


@pytest.mark.parametrize("bd", DEPTHS)
def test_equalise_and_stretch(bd):
    M = (1 << bd) - 1
    ident = np.arange(M + 1)
    for name, mh in shapes(bd).items():
        eh = to_e(mh, bd)
        eq = E.lut_equalise([eh], bd)
        assert np.array_equal(eq, LM.lut_equalise([mh], bd)), name
        assert np.all(np.diff(eq.astype(np.int64)) >= 0), name
        if name == "single":
            assert np.array_equal(eq, ident)
        else:
            assert eq[mh.max] == M and eq[mh.min] == 0, name
        for lo_ppm, hi_ppm in ((0, 0), (10000, 10000), (0, 999999), (999999, 0), (500000, 499999)):
            st = E.lut_stretch([eh], bd, lo_ppm, hi_ppm)
            assert np.array_equal(st, LM.lut_stretch([mh], lo_ppm, hi_ppm, bd)), (name, lo_ppm, hi_ppm)
            assert np.all(np.diff(st.astype(np.int64)) >= 0)
        st = E.lut_stretch([eh], bd)
        if name == "single":
            assert np.array_equal(st, ident)
        else:
            assert st[mh.max] == M and st[mh.min] == 0, name
        if name == "ramp":
            assert np.array_equal(eq, ident) and np.array_equal(st, ident)
    # pooled: two histograms count as their sum
    a, b = shapes(bd)["empty bins"], shapes(bd)["skewed"]
    both = LM.PlaneHist(a.hist + b.hist)
    assert np.array_equal(E.lut_equalise([to_e(a, bd), to_e(b, bd)], bd), LM.lut_equalise([both], bd))
    assert np.array_equal(E.lut_stretch([to_e(a, bd), to_e(b, bd)], bd, 5000, 5000), LM.lut_stretch([both], 5000, 5000, bd))
    # no samples at all: N == cmin == 0, the identity
    assert np.array_equal(E.lut_equalise([to_e(LM.plane_hist(None), bd)], bd), ident)


@pytest.mark.parametrize("bd", DEPTHS)
def test_percentile_and_distance(bd):
    sh = shapes(bd)
    for name, mh in sh.items():
        eh = to_e(mh, bd)
        for ppm in (0, 1, 1000, 499999, 500000, 500001, 999999, 10 ** 6):
            assert E.hist_percentile([eh], ppm) == LM.percentile([mh], ppm), (name, ppm)
        assert E.hist_percentile(eh, 0) == mh.min and E.hist_percentile([eh], 10 ** 6) == mh.max
    for a, b in itertools.combinations(sh, 2):
        assert E.hist_distance(to_e(sh[a], bd), to_e(sh[b], bd)) == LM.distance(sh[a], sh[b])
    a, b = sh["empty bins"], sh["skewed"]
    assert E.hist_percentile([to_e(a, bd), to_e(b, bd)], 700000) == LM.percentile([a, b], 700000)
    assert E.hist_distance(to_e(a, bd), to_e(a, bd)) == 0
    big = LM.PlaneHist(np.where(np.arange(LM.BINS) < 2, 2 ** 32 - 1, 0))     # counts near 2^32: the sums need 64 bits
    assert E.hist_distance(to_e(big), to_e(LM.plane_hist(None))) == 2 * (2 ** 32 - 1)
    assert E.hist_percentile([to_e(big)] * 3, 500001) == 1


def test_then():
    rng = np.random.default_rng(1)
    first, second = rng.integers(0, 1024, 256), rng.integers(0, 4096, 1024)
    assert np.array_equal(E.lut_then(first, second), LM.lut_then(first, second))
    first[17] = 1023
    assert np.array_equal(E.lut_then(first, second), second[first])
    first[17] = 1024
    assert LM.lut_then(first, second) is None and refused(E.lut_then, first, second)
    assert refused(E.lut_then, [], second) and refused(E.lut_then, first[:3], [])


def test_argument_rules():
    import ctypes as C
    L = E.lib()
    out = (C.c_uint16 * 4096)()
    h = to_e(LM.plane_hist(np.arange(100))).as_struct()
    empty = to_e(LM.plane_hist(None)).as_struct()
    v, s = C.c_uint32(77), C.c_uint64(77)
    for bad in (7, 11, 13, 16, 0, -8):
        assert L.oh_lut_identity(bad, 8, out) == ARG and L.oh_lut_identity(8, bad, out) == ARG
        assert L.oh_lut_range(bad, 8, 1, 0, out) == ARG and L.oh_lut_range(8, bad, 0, 1, out) == ARG
        assert L.oh_lut_linear(bad, 8, 65536, 0, 0, out) == ARG and L.oh_lut_linear(8, bad, 65536, 0, 0, out) == ARG
        assert L.oh_lut_stretch(C.byref(h), 1, 0, 0, bad, out) == ARG and L.oh_lut_equalise(C.byref(h), 1, bad, out) == ARG
    assert L.oh_lut_identity(8, 8, None) == ARG and L.oh_lut_range(8, 8, 1, 1, None) == ARG and L.oh_lut_linear(8, 8, 1, 0, 0, None) == ARG
    assert L.oh_lut_stretch(None, 1, 0, 0, 8, out) == ARG and L.oh_lut_stretch(C.byref(h), 1, 0, 0, 8, None) == ARG
    assert L.oh_lut_stretch(C.byref(h), 0, 0, 0, 8, out) == ARG and L.oh_lut_stretch(C.byref(h), -1, 0, 0, 8, out) == ARG
    assert L.oh_lut_stretch(C.byref(h), 1, 500000, 500000, 8, out) == ARG and L.oh_lut_stretch(C.byref(h), 1, 10 ** 6, 0, 8, out) == ARG
    assert L.oh_lut_stretch(C.byref(h), 1, 0xFFFFFFFF, 0xFFFFFFFF, 8, out) == ARG             # the sum does not wrap
    assert L.oh_lut_stretch(C.byref(h), 1, 500000, 499999, 8, out) == 0
    assert L.oh_lut_stretch(C.byref(empty), 1, 0, 0, 8, out) == ARG                           # no samples
    assert L.oh_lut_equalise(None, 1, 8, out) == ARG and L.oh_lut_equalise(C.byref(h), 1, 8, None) == ARG
    assert L.oh_lut_equalise(C.byref(h), 0, 8, out) == ARG
    assert L.oh_lut_then(None, 4, out, 4, out) == ARG and L.oh_lut_then(out, 4, None, 4, out) == ARG and L.oh_lut_then(out, 4, out, 4, None) == ARG
    assert L.oh_lut_then(out, 0, out, 4, out) == ARG and L.oh_lut_then(out, 4, out, 0, out) == ARG
    assert L.oh_hist_percentile(None, 1, 0, C.byref(v)) == ARG and L.oh_hist_percentile(C.byref(h), 1, 0, None) == ARG
    assert L.oh_hist_percentile(C.byref(h), 0, 0, C.byref(v)) == ARG and L.oh_hist_percentile(C.byref(h), 1, 10 ** 6 + 1, C.byref(v)) == ARG
    assert L.oh_hist_percentile(C.byref(empty), 1, 0, C.byref(v)) == ARG and v.value == 77
    assert L.oh_hist_percentile(C.byref(h), 1, 10 ** 6, C.byref(v)) == 0 and v.value == 99
    assert L.oh_hist_distance(None, C.byref(h), C.byref(s)) == ARG and L.oh_hist_distance(C.byref(h), None, C.byref(s)) == ARG
    assert L.oh_hist_distance(C.byref(h), C.byref(h), None) == ARG and s.value == 77
    # a refused builder leaves out as it was
    mark = (C.c_uint16 * 256)(*([0xABCD] * 256))
    first = (C.c_uint16 * 256)(*([300] * 256))
    assert L.oh_lut_then(first, 256, first, 256, mark) == ARG and L.oh_lut_identity(8, 7, mark) == ARG
    assert L.oh_lut_stretch(C.byref(empty), 1, 0, 0, 8, mark) == ARG
    assert all(x == 0xABCD for x in mark)
    # the binding: structures of the header's sizes
    assert C.sizeof(E.OhPlaneHist) == 32 + 4 * 4096 and C.sizeof(E.OhHistogram) == 3 * C.sizeof(E.OhPlaneHist)
    assert C.sizeof(E.OhLut) == 8 + 3 * C.sizeof(C.c_void_p)
    for fn, args in ((E.lut_identity, (8, 11)), (E.lut_range, (7, 8, True)), (E.lut_linear, (8, 13, 65536)), (E.lut_equalise, ([], 8)),
                     (E.lut_stretch, ([to_e(LM.plane_hist(None))], 8)), (E.hist_percentile, ([], 0))):
        assert refused(fn, *args), fn.__name__


def test_plane_hist_object():
    mh = LM.plane_hist(np.array([2, 2, 5, 9]))
    eh = to_e(mh, 8)
    assert eh.hist.shape == (256,) and eh.mean == 4.5 and eh.variance == (4 * (4 + 4 + 25 + 81) - 18 * 18) / 16
    none = to_e(LM.plane_hist(None), 8)
    assert none.mean is None and none.variance is None and none.samples == 0


def test_what_the_gpu_planes_reach():
    """the contents the GPU tests count and map reach bin 0, bin M, an empty bin and a bin that every sample hits"""
    for bd in DEPTHS:
        M = (1 << bd) - 1
        rng = np.random.default_rng(bd)
        rnd = LM.plane_hist(LM.content("random", (40, 96), bd, rng))
        assert rnd.hist[0] and rnd.hist[M] and rnd.min == 0 and rnd.max == M
        sparse = LM.plane_hist(LM.content("sparse", (40, 96), bd, rng))
        assert sparse.hist[1] == 0 and sparse.hist[2] == 0 and sparse.hist[0]
        for kind, v in (("zero", 0), ("top", M), ("flat", M // 2 + 1)):
            h = LM.plane_hist(LM.content(kind, (40, 96), bd, rng))
            assert h.hist[v] == 40 * 96 == h.samples and h.min == h.max == v
        n = 96 * 40
        covered = np.zeros(M + 1, dtype=bool)
        for c in range(3):                                                  # the ramps of the three planes start a third of the range apart
            r = LM.plane_hist(LM.content("ramp", (40, 96), bd, rng, start=c * ((M + 1) // 3)))
            covered |= r.hist[:M + 1] > 0
            assert r.samples == n and int(r.hist.max()) == -(-n // (M + 1))
        assert covered.all()
