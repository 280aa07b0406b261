"""The motion service on the CPU (include/ohevc_hip.h): the numpy model of tests/motion_model.py against the oracle's
uni-prediction at every fraction (the anchor to the reference: 16 quarter-sample luma and 64 eighth-sample chroma classes, three bit
depths, random and extreme content, blocks of 8 x 8 and 16 x 16), the host-only helpers of the library against the model, and what the
cases of tests/test_gpu_motion.py reach: which stage wins, which component of the key decides, how many reads clamp.  No GPU."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import motion_model as MM                                                   # noqa: E402
from oracle_lib import off_u8p, oracle, u8p                                  # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

DEPTHS = (8, 10, 12)
ARG = E.OH_E_ARG


def contents(bd, n, seed):
    """(name, plane of n x n): random, and the extremes 0 / M as constants and as checkerboards of both phases"""
    M = (1 << bd) - 1
    dt = MM.sample_dtype(bd)
    y, x = np.mgrid[0:n, 0:n]
    return [("random", np.random.default_rng(seed).integers(0, M + 1, (n, n), dtype=dt)), ("zero", np.zeros((n, n), dt)),
            ("M", np.full((n, n), M, dt)), ("checker", (((x + y) & 1) * M).astype(dt)), ("checker'", (((x + y + 1) & 1) * M).astype(dt)),
            ("columns", ((x & 1) * M + 0 * y).astype(dt)), ("rows", ((y & 1) * M + 0 * x).astype(dt))]


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("taps", (8, 4))
def test_model_equals_the_oracle_at_every_fraction(bd, taps):
    """predict() is oh_or_mc_uni: every fraction pair, blocks of 8 x 8 and 16 x 16 in the middle of a plane (the oracle does not clamp)"""
    o = oracle()
    n, bpp = 40, 1 if bd == 8 else 2
    for name, plane in contents(bd, n, 100 * bd + taps):
        plane = np.ascontiguousarray(plane)
        for size in (8, 16):
            x0, y0 = 9, 11
            for fy in range(32 // taps):                          # 4 quarter-sample, 8 eighth-sample fractions
                for fx in range(32 // taps):
                    dst = np.zeros((size, size), plane.dtype)
                    o.oh_or_mc_uni(bd, taps, u8p(dst), dst.strides[0], off_u8p(plane, y0 * plane.strides[0] + x0 * bpp), plane.strides[0], size,
                                   fx, fy, size)
                    got = MM.predict(plane, x0, y0, size, size, fx, fy, bd, taps)
                    assert np.array_equal(got, dst), (name, size, fx, fy)


@pytest.mark.parametrize("bd", DEPTHS)
def test_model_clamps_like_a_padded_plane(bd):
    """rows and columns clamp to the plane: predicting across an edge equals the oracle on a copy of the plane padded by its edge samples;
    and the luma / chroma vector arithmetic (whole part, fraction) is that of the definition for vectors of either sign"""
    o = oracle()
    bpp = 1 if bd == 8 else 2
    plane = MM.noise(bd, 24, 16, 7 + bd)
    pad = 40
    big = np.ascontiguousarray(np.pad(plane, pad, mode="edge"))
    for mvx, mvy in [(-37, 5), (95, -66), (-4, -4), (3, 0), (0, -1), (127, 127), (-128, -128), (2, 2)]:
        for x0, y0, w, h in ((0, 0, 16, 16), (16, 0, 8, 16), (16, 8, 8, 8)):
            dst = np.zeros((h, w), plane.dtype)
            xi, yi = x0 + (mvx >> 2) + pad, y0 + (mvy >> 2) + pad
            o.oh_or_mc_uni(bd, 8, u8p(dst), dst.strides[0], off_u8p(big, yi * big.strides[0] + xi * bpp), big.strides[0], h, mvx & 3, mvy & 3, w)
            assert np.array_equal(MM.predict_luma(plane, x0, y0, w, h, mvx, mvy, bd), dst), (mvx, mvy, x0, y0)
            for hs, vs in ((1, 1), (1, 0), (0, 0)):
                cp = MM.noise(bd, 24 >> hs, 16 >> vs, 70 + bd + hs + vs)
                cbig = np.ascontiguousarray(np.pad(cp, pad, mode="edge"))
                xc, yc, wc, hc = x0 >> hs, y0 >> vs, w >> hs, h >> vs
                fx, fy = (mvx & ((4 << hs) - 1)) << (1 - hs), (mvy & ((4 << vs) - 1)) << (1 - vs)
                assert 0 <= fx < 8 and 0 <= fy < 8
                dst = np.zeros((hc, wc), cp.dtype)
                xi, yi = xc + (mvx >> (2 + hs)) + pad, yc + (mvy >> (2 + vs)) + pad
                o.oh_or_mc_uni(bd, 4, u8p(dst), dst.strides[0], off_u8p(cbig, yi * cbig.strides[0] + xi * bpp), cbig.strides[0], hc, fx, fy, wc)
                assert np.array_equal(MM.predict_chroma(cp, xc, yc, wc, hc, mvx, mvy, hs, vs, bd), dst), (mvx, mvy, hs, vs)


def test_a_zero_field_copies_and_the_scalar_form_agrees():
    for bd in DEPTHS:
        for cf in range(4):
            planes = MM.random_planes(bd, 24, 16, cf, 5 + cf)
            bw, bh = MM.blocks(24, 16, 16)
            for a, b in zip(MM.compensate(planes, cf, bd, np.zeros((bh, bw, 2), np.int64), 16), planes):
                assert np.array_equal(a, b)
        for taps, nf in ((8, 4), (4, 8)):
            plane = MM.noise(bd, 16, 16, 50 + bd)
            for fx, fy in itertools.product(range(nf), repeat=2):
                got = MM.predict(plane, 5, 6, 4, 4, fx, fy, bd, taps)
                b = taps // 2 - 1
                for y, x in ((0, 0), (3, 2)):
                    win = plane[6 + y - b:6 + y - b + taps, 5 + x - b:5 + x - b + taps]
                    assert MM.sample_from_window(win, fx, fy, bd) == got[y, x]


# ---------------------------------------------------------------- the library's host-only helpers
def test_sample_helpers_equal_the_model():
    L = E.lib()
    for bd in (8, 9, 10, 12):
        M = (1 << bd) - 1
        rng = np.random.default_rng(900 + bd)
        wins = [rng.integers(0, M + 1, 64, dtype=np.uint16) for _ in range(6)] + [np.zeros(64, np.uint16), np.full(64, M, np.uint16),
                                                                                   ((np.arange(64) + np.arange(64) // 8) % 2 * M).astype(np.uint16)]
        for win in wins:
            p = win.ctypes.data_as(C.POINTER(C.c_uint16))
            for fx, fy in itertools.product(range(4), repeat=2):
                assert L.oh_motion_qpel(p, fx, fy, bd) == MM.sample_from_window(win.reshape(8, 8), fx, fy, bd), (bd, fx, fy)
            w4 = np.ascontiguousarray(win[:16])
            p4 = w4.ctypes.data_as(C.POINTER(C.c_uint16))
            for fx, fy in itertools.product(range(8), repeat=2):
                assert L.oh_motion_epel(p4, fx, fy, bd) == MM.sample_from_window(w4.reshape(4, 4), fx, fy, bd), (bd, fx, fy)
    win = np.zeros(64, np.uint16)
    p = win.ctypes.data_as(C.POINTER(C.c_uint16))
    for bad in ((-1, 0, 8), (4, 0, 8), (0, 4, 8), (0, -1, 8), (0, 0, 7), (0, 0, 11), (0, 0, 16)):
        assert L.oh_motion_qpel(p, *bad) == -1, bad
    for bad in ((-1, 0, 8), (8, 0, 8), (0, 8, 8), (0, 0, 14)):
        assert L.oh_motion_epel(p, *bad) == -1, bad
    assert L.oh_motion_qpel(None, 0, 0, 8) == -1 and L.oh_motion_epel(None, 0, 0, 8) == -1


def test_cost_equals_the_model():
    L = E.lib()
    rng = np.random.default_rng(31)
    for _ in range(300):
        sad = int(rng.integers(0, 256 * 4095 + 1))
        cx, cy = (int(v) for v in rng.integers(-4096, 4097, 2))
        mvx, mvy = 4 * cx + int(rng.integers(-131, 132)), 4 * cy + int(rng.integers(-131, 132))
        lam = int(rng.choice([0, 1, 3, 7, 4095, 4096]))
        assert L.oh_motion_cost(sad, mvx, mvy, cx, cy, lam) == MM.cost(sad, mvx, mvy, cx, cy, lam)
    assert L.oh_motion_cost(0xFFFFFFFF, 32767, -32768, -4096, 4096, 4096) == MM.cost(0xFFFFFFFF, 32767, -32768, -4096, 4096, 4096)
    assert L.oh_motion_cost(5, 1, 0, 0, 0, 3) == 5 and L.oh_motion_cost(5, 1, 1, 0, 0, 3) == 6      # the rate term is floored


def test_blocks():
    for w, h, b in itertools.product((8, 16, 24, 72, 3840, 16384), (8, 40, 2160), (8, 16)):
        assert E.motion_blocks(w, h, b) == MM.blocks(w, h, b)
    bw, bh = C.c_int(-7), C.c_int(-7)
    L = E.lib()
    for bad in ((0, 8, 8), (8, 0, 8), (-8, 8, 16), (8, 8, 4), (8, 8, 0), (8, 8, 32), (8, 8, 12)):
        assert L.oh_motion_blocks(*bad, C.byref(bw), C.byref(bh)) == ARG and (bw.value, bh.value) == (-7, -7), bad
    assert L.oh_motion_blocks(8, 8, 8, None, C.byref(bh)) == ARG and L.oh_motion_blocks(8, 8, 8, C.byref(bw), None) == ARG
    with pytest.raises(E.EngineError):
        E.motion_blocks(16, 16, 4)


def test_scale_equals_the_model():
    rng = np.random.default_rng(77)
    for s, bc, bf, (bwc, bhc), grid in [(2, 8, 16, (5, 3), (5, 3)), (2, 16, 8, (3, 2), (9, 5)), (4, 8, 8, (2, 2), (9, 5)), (1, 16, 8, (3, 2), (5, 3)),
                                        (8, 8, 16, (1, 1), (5, 3)), (2, 8, 8, (2, 1), (9, 5))]:
        coarse = np.zeros((bhc, bwc), dtype=MM.VECTOR)
        coarse["x"], coarse["y"] = rng.integers(-32768, 32768, (bhc, bwc)), rng.integers(-600, 600, (bhc, bwc))
        coarse["sad"] = 12345
        got = E.motion_scale(coarse, bc, s, grid, bf)
        want = MM.motion_scale(coarse, bc, s, grid, bf)
        assert got.dtype == np.int16 and got.shape == (grid[1], grid[0], 2) and np.array_equal(got, want), (s, bc, bf)
        assert np.abs(got).max() <= MM.MAX_CENTRE
    # the rounding and the clamp: (s mv + 2) >> 2 with an arithmetic shift
    one = np.zeros((1, 1), dtype=MM.VECTOR)
    for mv, s, want in ((-1, 1, 0), (-2, 1, 0), (-3, 1, -1), (2, 1, 1), (1, 1, 0), (-5, 2, -2), (32767, 8, 4096), (-32768, 8, -4096), (8191, 2, 4096)):
        one["x"], one["y"] = mv, -mv - 1 if mv > -32768 else 0
        got = E.motion_scale(one, 8, s, (1, 1), 8)
        assert got[0, 0, 0] == want == MM.motion_scale(one, 8, s, (1, 1), 8)[0, 0, 0], (mv, s)
    # (x, y) pairs in place of a structured field
    assert np.array_equal(E.motion_scale(np.array([[[8, -8]]]), 8, 2, (2, 2), 8), np.array([[[4, -4]] * 2] * 2))
    L = E.lib()
    vec = (E.OhMotionVector * 4)()
    out = (C.c_int16 * 8)(*([99] * 8))
    ok = dict(bwc=2, bhc=2, block_c=8, s=2, bw=2, bh=2, block_f=8)

    def call(coarse=vec, centres=out, **kw):
        a = dict(ok, **kw)
        return L.oh_motion_scale(coarse, a["bwc"], a["bhc"], a["block_c"], a["s"], a["bw"], a["bh"], a["block_f"], centres)
    for bad in (dict(coarse=None), dict(centres=None), dict(bwc=0), dict(bhc=-1), dict(bw=0), dict(bh=0), dict(s=0), dict(s=3), dict(s=16), dict(s=-2),
                dict(block_c=4), dict(block_c=32), dict(block_f=0), dict(block_f=12)):
        assert call(**bad) == ARG and list(out) == [99] * 8, bad
    assert call() == 0 and list(out) == [0] * 8


def test_field_conversion_of_the_wrapper():
    f = E.motion_field(np.array([[[1, -2], [32767, -32768]]]))
    assert f.dtype == E.MOTION_DTYPE and f.shape == (1, 2) and list(f["x"][0]) == [1, 32767] and list(f["y"][0]) == [-2, -32768]
    assert E.MOTION_DTYPE.itemsize == C.sizeof(E.OhMotionVector) == 12 and E.MOTION_DTYPE == MM.VECTOR
    g = np.zeros((2, 2), dtype=E.MOTION_DTYPE)
    assert E.motion_field(g).shape == (2, 2)
    for bad in (np.zeros((2, 3)), np.zeros((2, 3), int), np.array([[40000, 0]]), 5):
        with pytest.raises(ValueError):
            E.motion_field(bad)


# ---------------------------------------------------------------- what the GPU cases reach
CASES = MM.search_cases()


def test_the_gpu_cases_cover_the_parameters():
    seen = {k: {c[k] if k != "range" else tuple(c[k]) for c in CASES} for k in ("bd", "block", "range", "subpel", "lam", "centres", "content")}
    assert seen["bd"] == {8, 10, 12} and seen["block"] == {8, 16} and seen["range"] == set(MM.RANGES)
    assert seen["subpel"] == {0, 1, 2} and seen["lam"] == set(MM.LAMBDAS) and seen["centres"] == {None, "random", "outside"}
    assert seen["content"] == {"noise", "planted", "diagonal", "stripes", "flat", "opposed", "same"}
    assert {(c["w"], c["h"]) for c in CASES} == set(MM.SIZES)
    assert len({MM.case_id(c) + c["content"] for c in CASES}) == len(CASES)


def test_what_the_gpu_cases_reach():
    """per case and in all: blocks won at every stage, every component of the key deciding somewhere, and reads that clamp"""
    total = {}
    for i, c in enumerate(CASES):
        cur, ref, centres, field, want, stats = MM.case_result(i, c)
        n_blocks = want.size
        assert sum(stats.get(("stage", s), 0) for s in range(3)) == n_blocks == sum(stats.get(("decided", k), 0) for k in range(4))
        for s in range(c["subpel"] + 1, 3):
            assert ("stage", s) not in stats, (MM.case_id(c), "a finer vector than the call asked for")
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
        M = (1 << c["bd"]) - 1
        xy = MM.field_xy(want)
        if c["name"] == "beyond":                                  # far beyond the 16 x 8 picture: almost every candidate reads outside
            assert stats["clamped"] * 100 >= stats["candidates"] * 99
        if c["centres"] == "outside":
            assert stats["clamped"] == stats["candidates"]
            assert (np.abs(xy) >= 4 * MM.MAX_CENTRE - 4 * 3 - 3).all()
        if c["content"] in ("flat", "opposed"):                    # every candidate ties in SAD: the key's order alone makes the centre win
            samples = np.array([[MM.rect(c["w"], c["h"], c["block"], bx, by)[2] * MM.rect(c["w"], c["h"], c["block"], bx, by)[3]
                                 for bx in range(want.shape[1])] for by in range(want.shape[0])])
            diff = M if c["content"] == "opposed" else 5
            assert np.array_equal(xy, 4 * centres.astype(np.int64)) and np.array_equal(want["sad"], diff * samples)
            assert np.array_equal(want["sad_centre"], want["sad"])
            assert stats.get(("decided", 1 if c["lam"] < 4 else 0), 0) == n_blocks
        if c["content"] == "same" and c["centres"] is None:
            assert not xy.any() and not want["sad"].any() and not want["sad_centre"].any()
        if c["content"] == "planted":                              # the planted field comes back: without error in the interior at least
            inner = MM.interior(c["w"], c["h"], c["block"], c["range"])
            assert inner.sum() >= 3 and not want["sad"][inner].any() and np.array_equal(xy[inner], field[inner])
            assert stats.get(("stage", 2), 0) >= 3 and (want["sad_centre"][inner] > 0).all()
        if c["content"] == "diagonal":
            assert stats.get(("decided", 2), 0) >= 3
        if c["content"] == "stripes":
            assert stats.get(("decided", 3), 0) >= 3
        if c["name"] in ("sizes", "ranges"):                       # noise read mostly inside the plane: unique minima, the cost decides
            assert stats.get(("decided", 0), 0) == n_blocks
    for s in range(3):
        assert total["stage", s] >= 50, s
    for k in range(4):
        assert total["decided", k] >= 10, k
    assert total["clamped"] > total["candidates"] // 2 and total["candidates"] - total["clamped"] > 5000
