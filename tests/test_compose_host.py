"""oh_compose_blend, oh_compose_chroma_alpha and the integer definition of oh_pics_compose on the host, no GPU: the two
functions the kernel evaluates (csrc/compose_common.h) against the numpy model of tests/compose_model.py — whose division is a plain
integer division, the library's a multiplication and a shift —, the identities at the ends of the weight's range, the bounds and the
monotony of the blend, and the model against itself."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compose_model as PM                                                  # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

ALPHAS, OPACITIES = (0, 1, 127, 128, 254, 255), (0, 1, 128, 255, 256)


def lib_blend(dst, src, alpha, opacity):
    """oh_compose_blend over arrays"""
    f = E.lib().oh_compose_blend
    d, s, a, o = np.broadcast_arrays(dst, src, alpha, opacity)
    return np.array([f(int(w), int(x), int(y), int(z)) for w, x, y, z in zip(d.ravel(), s.ravel(), a.ravel(), o.ravel())],
                    np.int64).reshape(d.shape)


def test_the_reciprocal_divides_exactly():
    """x * (2^47 // 65280 + 1) >> 47 == x // 65280: a quotient changes at the multiples of 65280 only, so the numerators on both sides
    of every multiple up to the 12-bit maximum decide it; then every numerator at stride 7"""
    M, top = (1 << 47) // PM.ONE + 1, 4095 * PM.ONE + PM.ONE // 2
    assert M == 2155905153 and M < 1 << 32 and top == 267354240 < 1 << 31
    m = np.arange(0, top // PM.ONE + 2, dtype=np.uint64) * np.uint64(PM.ONE)
    for x in (m, m + np.uint64(1), m[1:] - np.uint64(1), np.arange(0, top + 1, 7, dtype=np.uint64), np.array([top], np.uint64)):
        x = x[x <= top]
        assert np.array_equal((x * np.uint64(M)) >> np.uint64(47), x // np.uint64(PM.ONE))


def test_blend_equals_the_model_on_all_8_bit_pairs():
    d, s = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    f = E.lib().oh_compose_blend
    for a, o in itertools.product(ALPHAS, OPACITIES):
        want = PM.blend(d, s, a, o)
        got = np.fromiter((f(int(x), int(y), a, o) for x, y in zip(d.ravel(), s.ravel())), np.int64, d.size).reshape(d.shape)
        assert np.array_equal(got, want), (a, o)


@pytest.mark.parametrize("bd", (10, 12))
def test_blend_equals_the_model_above_8_bit(bd):
    top = (1 << bd) - 1
    ext = np.array(list(itertools.product((0, 1, top - 1, top), (0, 1, top - 1, top), (0, 1, 254, 255), (0, 1, 255, 256))), np.int64)
    assert np.array_equal(lib_blend(ext[:, 0], ext[:, 1], ext[:, 2], ext[:, 3]), PM.blend(ext[:, 0], ext[:, 1], ext[:, 2], ext[:, 3]))
    rng = np.random.default_rng(bd)
    n = 100000
    d, s = rng.integers(0, top + 1, n), rng.integers(0, top + 1, n)
    a, o = rng.integers(0, 256, n), rng.integers(0, 257, n)
    assert np.array_equal(lib_blend(d, s, a, o), PM.blend(d, s, a, o))


def test_identities_bounds_and_monotony():
    for bd in (8, 10, 12):
        top = (1 << bd) - 1
        rng = np.random.default_rng(100 + bd)
        d = np.concatenate([[0, top, 0, top], rng.integers(0, top + 1, 400)])
        s = np.concatenate([[0, top, top, 0], rng.integers(0, top + 1, 400)])
        for a, o in ((0, 256), (255, 0), (0, 0), (17, 0), (0, 99)):         # w = 0: dst exactly
            assert np.array_equal(lib_blend(d, s, a, o), d)
        assert np.array_equal(lib_blend(d, s, 255, 256), s)                 # w = 65280: src exactly
        lo, hi = np.minimum(d, s), np.maximum(d, s)
        prev = None
        ws = sorted({a * o for a in range(256) for o in (0, 1, 2, 64, 128, 200, 255, 256)})
        by_w = {}
        for a in range(256):
            for o in (0, 1, 2, 64, 128, 200, 255, 256):
                by_w.setdefault(a * o, (a, o))
        for w in ws[::7] + [ws[-1]]:
            a, o = by_w[w]
            r = lib_blend(d[:64], s[:64], a, o)
            assert np.all((lo[:64] <= r) & (r <= hi[:64])), (bd, a, o)       # between dst and src
            if prev is not None:                                            # monotone in w: towards src
                assert np.all(np.where(s[:64] >= d[:64], r >= prev, r <= prev)), (bd, a, o)
            prev = r


def test_chroma_alpha_equals_the_model():
    f = E.lib().oh_compose_chroma_alpha
    rng = np.random.default_rng(3)
    quads = np.concatenate([[[0, 0, 0, 0], [255, 255, 255, 255], [255, 0, 0, 0], [0, 255, 0, 0], [0, 0, 255, 0], [0, 0, 0, 255],
                             [255, 255, 255, 254], [1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 0, 0]], rng.integers(0, 256, (2000, 4))])
    for cf in (0, 1, 2, 3):
        got = np.array([f(cf, *(int(v) for v in q)) for q in quads], np.int64)
        assert np.array_equal(got, PM.chroma_alpha(cf, quads[:, 0], quads[:, 1], quads[:, 2], quads[:, 3])), cf
    assert f(1, 255, 255, 255, 255) == f(2, 255, 255, 7, 9) == f(3, 255, 1, 2, 3) == 255
    assert f(1, 0, 0, 0, 0) == f(2, 0, 0, 200, 200) == f(3, 0, 9, 9, 9) == 0
    assert f(1, 1, 0, 0, 1) == 1 and f(1, 1, 0, 0, 0) == 0 and f(2, 1, 0, 0, 0) == 1      # halves round up


def planes(p, rng):
    return [rng.integers(0, 1 << p.bit_depth, (F.plane_dims(p, c)[1], F.plane_dims(p, c)[0])) for c in range(F.n_planes(p))]


@pytest.mark.parametrize("bd,cf", [(8, 1), (10, 2), (12, 3), (8, 0)])
def test_the_model_against_itself(bd, cf):
    p = F.pic_params(48, 24, bit_depth=bd, chroma_format_idc=cf)
    rng = np.random.default_rng(bd + cf)
    dst, a, b = planes(p, rng), planes(p, rng), planes(p, rng)
    keep = [d.copy() for d in dst]
    # an opaque whole-picture layer is a copy
    got = PM.compose(dst, p, [{"src": a}])
    assert all(np.array_equal(g, s) for g, s in zip(got, a))
    assert all(np.array_equal(d, k) for d, k in zip(dst, keep))             # the model leaves its input alone
    # two half-transparent layers in swapped order differ where they overlap, and only there
    la = {"src": a, "rect": (0, 0, 32, 16), "at": (4, 2), "opacity": 128}
    lb = {"src": b, "rect": (8, 4, 32, 16), "at": (16, 6), "opacity": 200}
    ab, ba = PM.compose(dst, p, [la, lb]), PM.compose(dst, p, [lb, la])
    for c in range(len(dst)):
        hs, vs = PM.shifts(cf, c)
        diff = ab[c] != ba[c]
        assert diff.any()
        over = np.zeros_like(diff)
        over[6 >> vs:18 >> vs, 16 >> hs:36 >> hs] = True
        assert not (diff & ~over).any()
    # a layer wholly outside is a no-op, on every side
    for at in ((48, 0), (0, 24), (-32, 0), (0, -16), (1000, 1000)):
        got = PM.compose(dst, p, [{"src": a, "rect": (0, 0, 32, 16), "at": at}])
        assert all(np.array_equal(g, d) for g, d in zip(got, dst)), at
    # fill then nothing gives constant planes
    fill = (5, 1 << (bd - 1), (1 << bd) - 1)
    got = PM.compose(dst, p, [], fill)
    assert all((g == fill[c]).all() and g.shape == dst[c].shape for c, g in enumerate(got))
    # an alpha of 255 everywhere is no alpha; an alpha of 0 everywhere no layer
    full, none = np.full((16, 32), 255), np.zeros((16, 32), np.int64)
    assert all(np.array_equal(x, y) for x, y in zip(PM.compose(dst, p, [dict(la, alpha=full)]), PM.compose(dst, p, [la])))
    assert all(np.array_equal(x, y) for x, y in zip(PM.compose(dst, p, [dict(la, alpha=none)]), dst))
