"""oh_reformat_quantise and the integer definition of oh_pics_reformat on the host, no GPU: the function the kernel
evaluates (csrc/reformat_common.h) against the numpy model of tests/reformat_model.py, the identities the definition promises — asserted
on the library function —, and the model against itself."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reformat_model as RM                                                 # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

DEPTHS = (8, 9, 10, 12)
MODES = (RM.ROUND, RM.DITHER)
TOP = 8 * 4095                                                              # the largest sum of all: f = 3 on 12-bit samples


def lib_q(sums, s, mode, x, y, bd):
    """oh_reformat_quantise over an array of sums at one place"""
    f = E.lib().oh_reformat_quantise
    return np.fromiter((f(int(v), s, mode, x, y, bd) for v in np.asarray(sums).ravel()), np.int64).reshape(np.shape(sums))


def lib_tile(v, s, mode, bd):
    """the 4 x 4 tile of outputs of one sum"""
    f = E.lib().oh_reformat_quantise
    return np.array([[f(int(v), s, mode, x, y, bd) for x in range(4)] for y in range(4)], np.int64)


def largest_sum(s, bd):
    """the largest sum a call can produce with this s into this depth: 2^f (2^Bs - 1) over f = 0 .. 3 and the source depths Bs with
    f + Bs - bd == s; where no call has this pair, the largest sum of all"""
    legal = [(1 << f) * ((1 << bs) - 1) for f in range(4) for bs in DEPTHS if f + bs - bd == s]
    return max(legal) if legal else TOP


def sums_of(s, bd):
    """0, 1, every sum around the last rounding steps below and the first ones above the clamp, a stride through the range, the largest"""
    top, mx = largest_sum(s, bd), (1 << bd) - 1
    if s > 0:
        near = np.arange((mx - 2) << s, ((mx + 2) << s) + 1)                # both sides of the steps to mx - 1, mx and beyond, for every r
    else:
        near = np.arange((mx >> -s) - 2, (mx >> -s) + 3)
    v = np.concatenate([[0, 1, top - 1, top], near, np.arange(0, top + 1, 97)])
    return np.unique(v[(v >= 0) & (v <= top)])


@pytest.mark.parametrize("bd", DEPTHS)
def test_quantise_equals_the_model(bd):
    for s, mode in itertools.product(range(-4, 8), MODES):
        v = sums_of(s, bd)
        assert v[-1] == largest_sum(s, bd) and v[0] == 0
        for y, x in itertools.product(range(4), range(4)):
            want = RM.quantise(v, s, mode, bd, x=x, y=y)
            assert np.array_equal(lib_q(v, s, mode, x, y, bd), want), (s, mode, x, y)
    # the place counts modulo 4 only
    f = E.lib().oh_reformat_quantise
    for x, y in ((5, 2), (4094, 7), (8191, 16383)):
        assert f(1000, 3, RM.DITHER, x, y, bd) == f(1000, 3, RM.DITHER, x & 3, y & 3, bd)


def test_dither_offsets_are_uniform():
    """s = 1 .. 4: r takes every value 0 .. 2^s - 1 equally often over a 4 x 4 tile — in the model and, read back as
    quantise(0 .. 2^s - 1 - r ...), in the library: a sum v gives 1 exactly where v + r >= 2^s"""
    for s in range(1, 5):
        r = RM.offsets(s, RM.DITHER, (4, 4))
        assert np.array_equal(np.bincount(r.ravel(), minlength=1 << s), np.full(1 << s, 16 >> s)), s
        for v in range(1 << s):
            assert np.array_equal(lib_tile(v, s, RM.DITHER, 8), (v + r) >> s), (s, v)
    for s in range(5, 8):                                                   # beyond: sixteen different offsets, 2^(s - 5) (2 t + 1)
        r = RM.offsets(s, RM.DITHER, (4, 4))
        assert len(set(r.ravel())) == 16 and r.min() == 1 << (s - 5) and r.max() == 31 << (s - 5)


@pytest.mark.parametrize("bd", DEPTHS)
def test_dithered_tile_sum_is_exact(bd):
    """over an aligned 4 x 4 tile of a constant v (away from the clamp) the sixteen dithered outputs sum to exactly 16 v / 2^s"""
    mx = (1 << bd) - 1
    rng = np.random.default_rng(bd)
    for s in range(1, 5):
        hi = min((mx << s) - (1 << s), TOP)                                 # (hi + r) >> s < mx for every r
        for v in [0, 1, (1 << s) - 1, 1 << s, hi] + [int(t) for t in rng.integers(0, hi + 1, 200)]:
            assert int(lib_tile(v, s, RM.DITHER, bd).sum()) * (1 << s) == 16 * v, (s, v)


def test_up_then_down_is_the_identity():
    """k bits up and k bits down again, every sample value, both modes, every place of the tile"""
    f = E.lib().oh_reformat_quantise
    for lo, hi in ((8, 9), (8, 10), (8, 12), (9, 10), (9, 12), (10, 12)):
        k = hi - lo
        for mode, (y, x) in itertools.product(MODES, itertools.product(range(4), range(4))):
            for v in range(1 << lo):
                u = f(v, -k, mode, x, y, hi)
                assert u == v << k and f(u, k, mode, x, y, lo) == v, (lo, hi, mode, x, y, v)


def const_planes(w, h, cf, vals):
    hs, vs = RM.shifts(cf)
    return [np.full((h, w), vals[0])] + ([np.full((h >> vs, w >> hs), v) for v in vals[1:]] if cf else [])


@pytest.mark.parametrize("sbd,dbd", [(8, 8), (8, 10), (10, 8), (12, 8), (10, 12), (9, 10), (12, 9)])
def test_constants_stay_constant(sbd, dbd):
    """a constant plane c gives quantise(c, k) through every filter and every format pair, by the library function at every place"""
    k, smx = sbd - dbd, (1 << sbd) - 1
    for vals in ((0, smx, smx // 3), (smx, 0, smx - 1), (smx // 2, 1, smx)):
        for scf, dcf, depth, down, up in itertools.product(range(4), range(4), MODES, (RM.POINT, RM.LINEAR), (RM.POINT, RM.LINEAR)):
            got = RM.reformat(const_planes(16, 8, scf, vals), sbd, scf, dbd, dcf, depth, down, up)
            assert len(got) == (3 if dcf else 1)
            for c, g in enumerate(got):
                if c and not scf:
                    assert (g == 1 << (dbd - 1)).all()
                    continue
                tile = lib_tile(vals[c], k, depth, dbd)
                assert np.array_equal(g, np.tile(tile, (g.shape[0] // 4, g.shape[1] // 4))), (vals, scf, dcf, depth, down, up, c)


def random_planes(w, h, bd, cf, rng):
    hs, vs = RM.shifts(cf)
    shapes = [(h, w)] + ([(h >> vs, w >> hs)] * 2 if cf else [])
    out = [rng.integers(0, 1 << bd, s) for s in shapes]
    for p in out:
        p[0, 0], p[-1, -1] = 0, (1 << bd) - 1
    return out


def test_the_model_against_itself():
    rng = np.random.default_rng(7)
    for bd, cf in itertools.product(DEPTHS, range(4)):
        src = random_planes(24, 16, bd, cf, rng)
        for depth, down, up in itertools.product(MODES, (RM.POINT, RM.LINEAR), (RM.POINT, RM.LINEAR)):
            got = RM.reformat(src, bd, cf, bd, cf, depth, down, up)         # same format and depth: a copy
            assert len(got) == len(src) and all(np.array_equal(g, s) for g, s in zip(got, src))
    for bd in DEPTHS:                                                       # 4:2:0 -> 4:4:4 nearest -> 4:2:0 point: the identity
        src = random_planes(24, 16, bd, 1, rng)
        for mid_cf in (3, 2):
            wide = RM.reformat(src, bd, 1, bd, mid_cf, up=RM.POINT)
            back = RM.reformat(wide, bd, mid_cf, bd, 1, down=RM.POINT)
            assert all(np.array_equal(b, s) for b, s in zip(back, src))
    # the sums of the linear filters by hand at the clamps: 16 x 8 luma, 4:2:0 chroma 8 x 4
    C = rng.integers(0, 1024, (4, 8))
    S, f = RM.chroma_sums(C, 1, 3, RM.LINEAR, RM.LINEAR)
    assert f == 3 and S.shape == (8, 16)
    assert S[0, 0] == 8 * C[0, 0] and S[0, 1] == 4 * (C[0, 0] + C[0, 1])    # row 0: j1 clamps to 0; column 0: k2 = k
    assert S[7, 15] == 8 * C[3, 7] and S[3, 15] == 6 * C[1, 7] + 2 * C[2, 7]
    assert S[2, 3] == 3 * (C[1, 1] + C[1, 2]) + C[0, 1] + C[0, 2]
    C = rng.integers(0, 1024, (8, 16))
    S, f = RM.chroma_sums(C, 3, 1, RM.LINEAR, RM.LINEAR)
    assert f == 3 and S.shape == (4, 8)
    assert S[0, 0] == 3 * (C[0, 0] + C[1, 0]) + C[0, 1] + C[1, 1]           # column -1 clamps to 0
    assert S[3, 7] == C[6, 13] + C[7, 13] + 2 * (C[6, 14] + C[7, 14]) + C[6, 15] + C[7, 15]
    assert RM.chroma_sums(C, 3, 2, RM.LINEAR, RM.LINEAR)[1] == 2 and RM.chroma_sums(C, 2, 1, RM.LINEAR, RM.LINEAR)[1] == 1
    assert RM.chroma_sums(C, 2, 3, RM.LINEAR, RM.LINEAR)[1] == 1 and RM.chroma_sums(C, 1, 2, RM.LINEAR, RM.LINEAR)[1] == 2
