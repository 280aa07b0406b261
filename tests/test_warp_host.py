"""The host-only functions of the warp service (openhevc_amd/csrc/pics_math.hip over csrc/warp_common.h, the code the kernel runs)
against the model of tests/warp_model.py and against Python integers: the cubic taps, one sample from its neighbourhood, the position
of a sample, the map builders, and their argument rules.  No GPU."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import warp_model as WM                                                     # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

ARG = E.OH_E_ARG


def L():
    return E.lib()


def as_warp(m, mode=0):
    w = E.warp_identity()
    w.mode = mode
    for k, v in enumerate(m):
        w.m[k] = v
    return w


def c_position(m, mode, hs, vs, x, y):
    px, py = C.c_int32(), C.c_int32()
    rc = L().oh_warp_position(C.byref(as_warp(m, mode)), hs, vs, x, y, C.byref(px), C.byref(py))
    return rc, px.value, py.value


def c_cubic(f):
    c = (C.c_int16 * 4)()
    assert L().oh_warp_cubic(f, c) == 0
    return list(c)


def test_cubic_taps():
    """all 64 phases: the model's taps, the sums, the mirror symmetry, the bound that keeps 12 bit in int32, the two phases named"""
    for f in range(64):
        c = c_cubic(f)
        assert c == WM.cubic(f), f
        assert sum(c) == 1024 and sum(abs(v) for v in c) <= 1296, (f, c)
        if f:
            assert c == c_cubic(64 - f)[::-1], f
    assert c_cubic(0) == [0, 1024, 0, 0] and c_cubic(32) == [-64, 576, 576, -64]
    c = (C.c_int16 * 4)()
    assert L().oh_warp_cubic(64, c) == ARG and L().oh_warp_cubic(-1, c) == ARG and L().oh_warp_cubic(3, None) == ARG


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_interp_against_the_model(bd):
    """every (fx, fy) of both filters, and nearest: random neighbourhoods and the extremes — all 0, all max, and the alternating 0 / max
    patterns, the largest cubic overshoot on both sides of the clip"""
    top = (1 << bd) - 1
    rng = np.random.default_rng(bd)
    hoods = [np.zeros(16, np.uint16), np.full(16, top, np.uint16)]
    for phase in (0, 1):
        hoods.append(np.array([((i + phase) & 1) * top for i in range(16)], np.uint16))                 # columns alternate
        hoods.append(np.array([((i // 4 + phase) & 1) * top for i in range(16)], np.uint16))            # rows alternate
        hoods.append(np.array([((i + i // 4 + phase) & 1) * top for i in range(16)], np.uint16))        # checkerboard
        hoods.append(np.array([top * (phase ^ (i % 4 in (1, 2) and i // 4 in (1, 2))) for i in range(16)], np.uint16))  # centre against ring
    hoods += [rng.integers(0, top + 1, 16).astype(np.uint16) for _ in range(4)]
    clipped = set()
    for taps in hoods:
        ptr = taps.ctypes.data_as(C.POINTER(C.c_uint16))
        for filt in (WM.NEAREST, WM.BILINEAR, WM.BICUBIC):
            for fx, fy in itertools.product(range(64), range(64)):
                got = L().oh_warp_interp(ptr, fx, fy, filt, bd)
                want = WM.interp_taps(taps, fx, fy, filt, bd)
                assert got == want and 0 <= got <= top, (filt, fx, fy, taps.tolist(), got, want)
                if filt == WM.BICUBIC and 0 < fx and 0 < fy and len(set(taps.tolist())) > 1:
                    clipped.add(got)
    assert 0 in clipped and top in clipped                      # the clip was reached on both sides
    ptr = hoods[-1].ctypes.data_as(C.POINTER(C.c_uint16))
    assert L().oh_warp_interp(ptr, 0, 0, WM.BICUBIC, bd) == hoods[-1][5] and L().oh_warp_interp(ptr, 0, 0, WM.BILINEAR, bd) == hoods[-1][5]
    for bad in ((None, 0, 0, 1, bd), (ptr, 64, 0, 1, bd), (ptr, 0, -1, 1, bd), (ptr, 0, 0, 3, bd), (ptr, 0, 0, -1, bd), (ptr, 0, 0, 1, 11)):
        assert L().oh_warp_interp(*bad) == -1, bad


B22, B36, B26 = 1 << 22, 1 << 36, 1 << 26


def test_position_against_python_integers():
    """every chroma format's shifts, coefficients at +- their bounds, the largest coordinates, a denominator at its lower bound"""
    maps = [list(WM.IDENTITY), [B22, B22, B36, B22, B22, B36, 0, 0, WM.ONE30], [-B22, -B22, -B36, -B22, -B22, -B36, 0, 0, WM.ONE30],
            [B22, -B22, -B36, -B22, B22, B36, 0, 0, WM.ONE30], [65537, -12345, 7 << 13, 4321, 65001, -(9 << 12), 0, 0, WM.ONE30],
            [3, -1, -1, -3, 1, 1, 0, 0, WM.ONE30]]
    pts = [(0, 0), (1, 0), (0, 1), (7, 5), (1001, 777), (8191, 8191), (8192, 8192)]
    for m, (hs, vs), (x, y) in itertools.product(maps, ((0, 0), (1, 0), (1, 1)), pts):
        rc, px, py = c_position(m, 0, hs, vs, x, y)
        assert rc == 0 and (px, py) == WM.position(m, 0, hs, vs, x, y), (m, hs, vs, x, y)
    assert c_position(maps[1], 0, 0, 0, 16384, 16384)[0] == 0
    rc, px, py = c_position(maps[1], 0, 0, 0, 16384, 16384)
    assert (px, py) == ((1 << 31) - 1, (1 << 31) - 1)                         # the clamp
    rc, px, py = c_position(maps[2], 0, 0, 0, 16384, 16384)
    assert (px, py) == (-(1 << 30), -(1 << 30))
    # perspective: the denominator exactly 2^20 at (x, y), then every bound at once
    for (hs, vs), (x, y) in itertools.product(((0, 0), (1, 0), (1, 1)), pts[:5]):
        X, Y = x << hs, y << vs
        for m67 in ((0, 0), (B26, -B26), (-B26, -B26), (-12345, 54321)):
            for lin in maps:
                m8 = (1 << 20) - m67[0] * X - m67[1] * Y - vs * (m67[1] >> 1)
                if not 0 < m8 <= B36:
                    continue
                m = lin[:6] + [m67[0], m67[1], m8]
                rc, px, py = c_position(m, 1, hs, vs, x, y)
                assert rc == 0 and (px, py) == WM.position(m, 1, hs, vs, x, y), (m, hs, vs, x, y)
                m[8] -= 1                                                   # one below the bound
                if m[8] > 0:
                    assert c_position(m, 1, hs, vs, x, y)[0] == ARG
    m = [B22, B22, B36, -B22, -B22, -B36, B26, B26, B36]
    for x, y in pts:
        rc, px, py = c_position(m, 1, 1, 1, x, y)
        assert rc == 0 and (px, py) == WM.position(m, 1, 1, 1, x, y)
    # the rules
    ident = list(WM.IDENTITY)
    px = C.c_int32()
    assert L().oh_warp_position(None, 0, 0, 0, 0, C.byref(px), C.byref(px)) == ARG
    assert L().oh_warp_position(C.byref(as_warp(ident)), 0, 0, 0, 0, None, C.byref(px)) == ARG
    for hs, vs, x, y in ((2, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, 16385), (1, 0, 8193, 0), (1, 1, 0, 8193)):
        assert c_position(ident, 0, hs, vs, x, y)[0] == ARG, (hs, vs, x, y)
    for k, over in ((0, B22 + 1), (1, -B22 - 1), (3, B22 + 1), (4, -B22 - 1), (2, B36 + 1), (5, -B36 - 1)):
        m = list(ident)
        m[k] = over
        assert c_position(m, 0, 0, 0, 0, 0)[0] == ARG and c_position(m, 1, 0, 0, 0, 0)[0] == ARG, k
    for k, over in ((6, B26 + 1), (7, -B26 - 1), (8, 0), (8, -1), (8, B36 + 1)):
        m = list(ident)
        m[k] = over
        assert c_position(m, 1, 0, 0, 0, 0)[0] == ARG, k
        assert c_position(m, 0, 0, 0, 0, 0)[0] == 0, k                      # the affine mode does not read them
    assert c_position(ident, 2, 0, 0, 0, 0)[0] == ARG and c_position(ident, -1, 0, 0, 0, 0)[0] == ARG


def test_builders_against_python_integers():
    ident = E.warp_identity()
    assert list(ident.m) == list(WM.IDENTITY) and (ident.mode, ident.filter, ident.border, ident.width, ident.height) == (0, 1, 0, 0, 0)
    assert list(ident.fill) == [0, 0, 0] and (ident.win.left, ident.win.right, ident.win.top, ident.win.bottom) == (0, 0, 0, 0)
    for dx, dy in ((0, 0), (1, -1), (-7, 13), (2 ** 31 - 1, -2 ** 31), (4 << 20, 0)):
        assert list(E.warp_translation(dx, dy).m) == WM.translation(dx, dy)
    with pytest.raises(E.EngineError):
        E.warp_then(E.warp_translation(2 ** 31 - 1, 0), E.warp_translation(2 ** 31 - 1, 0))   # 2^46: beyond m[2]'s bound
    rng = np.random.default_rng(5)
    some = [list(WM.IDENTITY), WM.translation(5, -9), [0, -WM.ONE, 23 << 16, WM.ONE, 0, 0, 0, 0, WM.ONE30], [B22, -B22, B36, B22, B22, -B36, 0, 0, WM.ONE30]]
    for _ in range(40):
        some.append([int(v) for v in rng.integers(-(1 << 18), 1 << 18, 2)] + [int(rng.integers(-(1 << 30), 1 << 30))] +
                    [int(v) for v in rng.integers(-(1 << 18), 1 << 18, 2)] + [int(rng.integers(-(1 << 30), 1 << 30)), 0, 0, WM.ONE30])
    for a, b in itertools.product(some[:12], some[:12]):
        want = WM.then(a, b)
        wa, wb = as_warp(a), as_warp(b)
        wa.filter, wa.border, wb.width, wb.height = 2, 1, 40, 24
        if WM.in_bounds(want):
            got = E.warp_then(wa, wb)
            assert list(got.m) == want and (got.filter, got.border, got.width, got.height) == (2, 1, 40, 24), (a, b)
        else:
            with pytest.raises(E.EngineError):
                E.warp_then(wa, wb)
    for a in some:
        want = WM.invert(a)
        if want is None or not WM.in_bounds(want):
            with pytest.raises(E.EngineError):
                E.warp_invert(as_warp(a))
        else:
            assert list(E.warp_invert(as_warp(a)).m) == want, a
    assert list(E.warp_invert(as_warp(some[2])).m)[:6] == [0, WM.ONE, 0, -WM.ONE, 0, 23 << 16]       # a quarter turn back
    for sing in ([0, 0, 0, 0, 0, 0], [2, 4, 0, 1, 2, 0], [WM.ONE, WM.ONE, 5, WM.ONE, WM.ONE, 9]):
        with pytest.raises(E.EngineError) as err:
            E.warp_invert(as_warp(sing + [0, 0, WM.ONE30]))
        assert err.value.code == ARG
    persp = as_warp(WM.IDENTITY, 1)
    for call in (lambda: E.warp_then(persp, ident), lambda: E.warp_then(ident, persp), lambda: E.warp_invert(persp)):
        with pytest.raises(E.EngineError):
            call()                                                          # affine maps only
    assert L().oh_warp_identity(None) == ARG and L().oh_warp_translation(0, 0, None) == ARG
    assert L().oh_warp_then(None, C.byref(ident), C.byref(ident)) == ARG and L().oh_warp_then(C.byref(ident), C.byref(ident), None) == ARG
    assert L().oh_warp_invert(C.byref(ident), None) == ARG and L().oh_warp_invert(None, C.byref(ident)) == ARG


def test_rotation():
    """the four terms within one unit of numpy's (libm and numpy may differ in the last bit before the rounding, which moves a Q16
    result by one unit at most: the whole allowance), the offsets exactly the integer formula of the returned terms, quarter turns
    exact"""
    cs, cd = (23 << 15, 15 << 15), (-(5 << 16) + 7, 1 << 28)
    for scale in (65536, 49152, 98304, 1, 1 << 22):
        for code in list(range(0, 65536, 1 << 13)) + [1, 5461, 5462, 21845, 65535, 12345, 40001]:
            m = list(E.warp_rotation(code, cs, cd, scale).m)
            t = code * (2 * np.pi / 65536)
            want = [round(float(scale * np.cos(t))), -round(float(scale * np.sin(t))), round(float(scale * np.sin(t))), round(float(scale * np.cos(t)))]
            assert all(abs(g - v) <= 1 for g, v in zip((m[0], m[1], m[3], m[4]), want)), (scale, code, m, want)
            assert m[0] == m[4] and m[1] == -m[3] and m[6:] == [0, 0, WM.ONE30]
            assert (m[2], m[5]) == WM.rotation_offsets(m, cs, cd), (scale, code)
            if code % (1 << 14) == 0:
                k = code >> 14
                assert (m[0], m[3]) == ((scale, 0), (0, scale), (-scale, 0), (0, -scale))[k], (scale, code)
    for bad in (lambda: E.warp_rotation(65536, cs, cd), lambda: E.warp_rotation(0, cs, cd, 0), lambda: E.warp_rotation(0, cs, cd, (1 << 22) + 1),
                lambda: E.warp_rotation(0, ((1 << 36) + 1, 0), cd), lambda: E.warp_rotation(0, cs, (0, -(1 << 36) - 1)),
                lambda: E.warp_rotation(0, (1 << 36, 0), (-(1 << 36), 0))):      # the offset leaves its bound
        with pytest.raises(E.EngineError) as err:
            bad()
        assert err.value.code == ARG
    assert L().oh_warp_rotation(0, 0, 0, 0, 0, 65536, None) == ARG


def test_from_sei():
    """exactly the integer formulas over the rotation's terms; at quarter turns the map of the orientation that oh_orient_from_sei gives"""
    for (w, h), hf, vf, code in itertools.product(((24, 16), (17, 9), (1, 1), (16384, 16384)), (0, 1), (0, 1), (0, 1 << 14, 2 << 14, 3 << 14, 5461, 30000, 65535)):
        r = list(E.warp_rotation(code, (0, 0), (0, 0)).m)
        ow = ((abs(r[0]) * w + abs(r[1]) * h + 65535) >> 16) + 1 & ~1
        oh = ((abs(r[3]) * w + abs(r[4]) * h + 65535) >> 16) + 1 & ~1
        cs, cd = ((w - 1) << 15, (h - 1) << 15), ((ow - 1) << 15, (oh - 1) << 15)
        m = r[:]
        m[2], m[5] = WM.rotation_offsets(r, cs, cd)
        if hf:
            m[0], m[1], m[2] = -m[0], -m[1], ((w - 1) << 16) - m[2]
        if vf:
            m[3], m[4], m[5] = -m[3], -m[4], ((h - 1) << 16) - m[5]
        got, size = E.warp_from_sei(hf, vf, code, w, h)
        assert list(got.m) == m and size == (ow, oh) and (got.width, got.height) == (ow, oh), (w, h, hf, vf, code)
        assert (got.mode, got.filter, got.border) == (0, 1, 0)
        if code % (1 << 14) == 0 and w % 2 == 0 and h % 2 == 0:
            o = E.orientation_from_sei(hf, vf, code)
            assert (list(got.m), size) == WM.orient_map(o, w, h), (hf, vf, code)
    w, ow, oh = E.OhWarp(), C.c_int(), C.c_int()
    for bad in ((2, 0, 0, 8, 8), (0, -1, 0, 8, 8), (0, 0, 65536, 8, 8), (0, 0, 0, 0, 8), (0, 0, 0, 8, 16385)):
        assert L().oh_warp_from_sei(*bad, C.byref(w), C.byref(ow), C.byref(oh)) == ARG, bad
    assert L().oh_warp_from_sei(0, 0, 0, 8, 8, None, C.byref(ow), C.byref(oh)) == ARG
    assert L().oh_warp_from_sei(0, 0, 0, 8, 8, C.byref(w), None, C.byref(oh)) == ARG


def test_identity_reproduces_the_input():
    """the model under the identity map at every filter and chroma format: the source's planes"""
    rng = np.random.default_rng(9)
    for cf, bd, filt in itertools.product(range(4), (8, 10), (WM.NEAREST, WM.BILINEAR, WM.BICUBIC)):
        p = F.pic_params(24, 16, bit_depth=bd, chroma_format_idc=cf)
        planes = [rng.integers(0, 1 << bd, (16 >> WM.shifts(cf, c)[1], 24 >> WM.shifts(cf, c)[0])).astype(np.uint16 if bd > 8 else np.uint8)
                  for c in range(3 if cf else 1)]
        out = WM.warp(planes, p, (0, 0, 0, 0), WM.IDENTITY, (24, 16), p, filt=filt)
        assert all(np.array_equal(a, b) for a, b in zip(out, planes)), (cf, bd, filt)


def test_paths_predicate():
    """oh_warp_paths counts every tile once, and the identity stages all of them"""
    w = E.warp_identity()
    w.width, w.height = 72, 40
    assert E.warp_paths(w, 10, 1, 72, 40) == (2 * 3 + 2 * (1 * 2), 0)         # luma 2 x 3 tiles of 64 x 16, chroma 1 x 2 each
    w.m[0] = w.m[4] = 8 << 16                                               # 8 : 1: a tile reads 512 x 128 samples
    w.width, w.height = 64, 16
    assert E.warp_paths(w, 10, 0, 64, 16) == (0, 1)
    for bad in (lambda: E.warp_paths(w, 11, 0, 64, 16), lambda: E.warp_paths(w, 10, 4, 64, 16), lambda: E.warp_paths(w, 10, 0, 32, 16)):
        with pytest.raises(E.EngineError):
            bad()
