"""The host-only helpers of the light-level pass (include/ohevc_hip.h: oh_light_bin, oh_light_bin_upper, oh_light_percentile) and the
Python helpers on top of them (light_nits, source_peak) — no GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import light_model as LM                                                    # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

FS = 1 << 30


def edges():
    """the smallest v of every bin above 0"""
    return [(16 + j) << (e - 4) for e in range(14, 30) for j in range(16)] + [FS]


def test_bin_equals_the_model():
    vals = [0, (1 << 14) - 1, 1 << 14] + [1 << k for k in range(31)]
    for x in edges():
        vals += [x - 1, x, x + 1]
    vals += [int(x) for x in np.random.default_rng(258).integers(0, FS + 1, 100000)]
    vals = [min(v, FS) for v in vals]
    want = LM.bin_of(np.array(vals, np.int64))
    got = np.array([E.light_bin(v) for v in vals])
    assert np.array_equal(got, want)
    assert E.light_bin(FS) == 257 and E.light_bin(FS - 1) == 256 and E.light_bin(0xFFFFFFFF) == 257   # clamped to 2^30
    assert [E.light_bin(x) for x in edges()] == list(range(1, 258))


def test_bin_upper_is_the_largest_value_of_the_bin():
    assert E.LL_NBINS == LM.NBINS == 258
    for b in range(258):
        up = E.light_bin_upper(b)
        assert up == LM.bin_upper(b), b
        assert E.light_bin(up) == b, b
        assert up == FS or E.light_bin(up + 1) == b + 1, b
    assert E.light_bin_upper(0) == (1 << 14) - 1 and E.light_bin_upper(257) == FS and E.light_bin_upper(256) == FS - 1


def ll(counts, mx, mn=0, pixels=None):
    h = np.zeros(258, np.uint32)
    for b, c in counts.items():
        h[b] = c
    n = int(h.sum()) if pixels is None else pixels
    return E.LightLevel(n, 0, mx, mn, h)


def as_model(x):
    return dict(pixels=x.pixels, max=x.max, hist=x.hist)


def test_percentile_on_hand_made_histograms():
    up = E.light_bin_upper
    one = ll({40: 1000}, FS)
    for ppm in (0, 1, 500000, 999900, 1000000):
        want = up(0) if ppm == 0 else up(40)              # nothing needs to be reached at ppm 0: the first bin
        assert E.light_percentile([one], ppm) == want, ppm
    # two pictures pooled: 1500 pixels in bin 10, 400 in bin 100, 100 in bin 200
    a, b = ll({10: 1000, 100: 400}, FS), ll({10: 500, 200: 100}, FS)
    assert E.light_percentile([a, b], 750000) == up(10)                     # an exact tie: 1500 * 10^6 == 750000 * 2000
    assert E.light_percentile([a, b], 750001) == up(100)
    assert E.light_percentile([a, b], 950000) == up(100)                    # again a tie, at 1900
    assert E.light_percentile([a, b], 950001) == up(200)
    assert E.light_percentile([a, b], 1000000) == up(200)
    assert E.light_percentile([a], 750000) == up(100) and E.light_percentile([b], 750000) == up(10)
    # the largest max of the pictures clips the bin's upper edge
    lo = up(200) - 5
    assert E.light_percentile([ll({10: 500, 200: 100}, lo), ll({10: 1000}, 3)], 1000000) == lo
    assert E.light_percentile([ll({200: 7}, lo)], 0) == up(0)
    for lls, ppm in (([a, b], 0), ([a, b], 123456), ([a, b], 999900), ([one], 1000000)):
        assert E.light_percentile(lls, ppm) == LM.percentile([as_model(x) for x in lls], ppm)
    rng = np.random.default_rng(5)
    for _ in range(20):
        lls = []
        for _ in range(3):
            h = rng.integers(0, 50, 258).astype(np.uint32) * (rng.random(258) < 0.2)
            h[3] += 1
            lls.append(E.LightLevel(int(h.sum()), 0, int(rng.integers(1, FS + 1)), 0, h))
        ppm = int(rng.integers(0, 1000001))
        assert E.light_percentile(lls, ppm) == LM.percentile([as_model(x) for x in lls], ppm)


def test_percentile_argument_rules():
    L = E.lib()
    one = ll({40: 10}, FS).as_struct()
    v = C.c_uint32(77)
    arg = E.OH_E_ARG
    assert L.oh_light_percentile(C.byref(one), 0, 5, C.byref(v)) == arg
    assert L.oh_light_percentile(C.byref(one), -1, 5, C.byref(v)) == arg
    assert L.oh_light_percentile(C.byref(one), 1, 1000001, C.byref(v)) == arg
    assert L.oh_light_percentile(None, 1, 5, C.byref(v)) == arg
    assert L.oh_light_percentile(C.byref(one), 1, 5, None) == arg
    empty = ll({}, 0).as_struct()
    assert L.oh_light_percentile(C.byref(empty), 1, 5, C.byref(v)) == arg   # no pixels
    assert v.value == 77
    assert L.oh_light_percentile(C.byref(one), 1, 1000000, C.byref(v)) == 0 and v.value == E.light_bin_upper(40)
    with pytest.raises(E.EngineError) as ei:
        E.light_percentile([])
    assert ei.value.code == arg


def test_light_nits():
    assert E.light_nits(FS, 16, 400.0) == 10000.0                           # PQ: src_peak is not read
    assert E.light_nits(FS >> 1, 16, 1.0) == 5000.0
    assert E.light_nits(FS, 18, 1000.0) == 1000.0
    assert E.light_nits(FS >> 2, 1, 100.0) == 25.0
    assert E.light_nits(0, 13, 80.0) == 0.0


def test_source_peak_prefers_measurement_then_maxcll_then_mastering_then_default():
    measured = [E.LightLevel(100, 0, FS >> 3, 0, ll({230: 100}, FS >> 3).hist, 10000.0)]
    sei_all = dict(max_cll=1200, max_fall=300, max_lum=40000000, min_lum=50)
    want = E.light_nits(E.light_percentile(measured), 16, 0)
    assert want == 1250.0                                                   # clipped by max = 2^27
    assert E.source_peak(16, measured, sei_all) == want
    assert E.source_peak(16, None, sei_all) == 1200.0
    assert E.source_peak(16, [], sei_all) == 1200.0
    assert E.source_peak(16, None, dict(sei_all, max_cll=0)) == 4000.0      # MaxCLL 0 means unknown
    assert E.source_peak(16, None, dict(max_cll=0, max_fall=0)) == 1000.0
    assert E.source_peak(16, None, dict(max_lum=0, min_lum=0), default=600.0) == 600.0
    assert E.source_peak(16, None, dict(preferred_transfer=18)) == 1000.0
    assert E.source_peak(16) == 1000.0 and E.source_peak(16, default=2000) == 2000.0
    # another ppm moves the measurement; other transfers scale by the full scale the levels were measured with
    two = [E.LightLevel(100, 0, FS, 0, ll({100: 90, 257: 10}, FS).hist, 250.0)]
    assert E.source_peak(1, two, ppm=900000) == E.light_nits(E.light_bin_upper(100), 1, 250.0)
    assert E.source_peak(1, two, ppm=900001) == 250.0
    assert "tone=\"none\"" in E.source_peak.__doc__ and "dst_peak" in E.source_peak.__doc__
