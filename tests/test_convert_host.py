"""CPU checks of the picture conversion (oh_pics_convert): the integers oh_convert_coeffs hands the kernel against the
H.273 matrices, the numpy model (tests/convert_model.py) against a float64 evaluation and published anchors, the chroma up-sampling,
oh_convert_image_bytes and the argument rules that need no device."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import convert_model as M
from openhevc_amd import engine as E
from openhevc_amd import frame as F

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openhevc_amd", "libohevc_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libohevc_hip.so not built (run __graft_entry__.build())")

MATRICES = (1, 5, 6, 9)
DEPTHS = (8, 9, 10, 12)
SAMPLES_D = ((E.CONV_U8, 8), (E.CONV_U16, 16), (E.CONV_F16, 16), (E.CONV_F32, 16))


def rounded(x):
    """round half away from zero"""
    return int(np.sign(x) * np.floor(abs(x) + 0.5))


def real_coeffs(matrix, full_range, bd, D):
    kr, kb = M.KR_KB[matrix]
    kg = 1 - kr - kb
    u = 1 << (bd - 8)
    ys, cs = ((1 << bd) - 1.0, (1 << bd) - 1.0) if full_range else (219.0 * u, 224.0 * u)
    mx = (1 << D) - 1
    return [mx / ys, mx * 2 * (1 - kr) / cs, -mx * 2 * kb * (1 - kb) / (kg * cs), -mx * 2 * kr * (1 - kr) / (kg * cs), mx * 2 * (1 - kb) / cs]


def worst(c, yoff, mid, bd, S):
    dy, dc = max(yoff, (1 << bd) - 1 - yoff), mid
    ty, r = abs(c[0]) * dy, 1 << (S - 1)
    return max(ty + abs(c[1]) * dc + r, ty + (abs(c[2]) + abs(c[3])) * dc + r, ty + abs(c[4]) * dc + r)


@pytest.mark.parametrize("matrix,full_range,bd,sd", list(itertools.product(MATRICES, (0, 1), DEPTHS, SAMPLES_D)))
def test_coefficients_are_the_rounded_matrix_and_cannot_overflow(matrix, full_range, bd, sd):
    sample, D = sd
    cv = E.make_convert("rgb", sample, matrix=matrix, full_range=full_range)
    cy, crv, cgu, cgv, cbu, yoff, mid, S, D2 = E.convert_coeffs(cv, bd)
    assert D2 == D
    assert mid == 1 << (bd - 1)
    assert yoff == (0 if full_range else 16 << (bd - 8))
    real = real_coeffs(matrix, full_range, bd, D)
    got = [cy, crv, cgu, cgv, cbu]
    assert got == [rounded(r * 2.0 ** S) for r in real]
    assert worst(got, yoff, mid, bd, S) <= 2 ** 31 - 1                     # every term and sum stays in int32
    nxt = [rounded(r * 2.0 ** (S + 1)) for r in real]
    assert S == 30 or worst(nxt, yoff, mid, bd, S + 1) > 2 ** 31 - 1      # and S is the largest such shift
    # the extremes of the sums, evaluated in int64, stay inside int32 too
    ys = np.array([0, (1 << bd) - 1], np.int64) - yoff
    cs = np.array([0, (1 << bd) - 1], np.int64) - mid
    for a, b in itertools.product(cs, cs):
        for t in (cy * ys + crv * b, cy * ys + cgu * a + cgv * b, cy * ys + cbu * a):
            assert np.all(np.abs(t + (1 << (S - 1))) < 2 ** 31)


@pytest.mark.parametrize("matrix,full_range,bd,sd", list(itertools.product(MATRICES, (0, 1), DEPTHS, SAMPLES_D[:2])))
def test_model_agrees_with_float64_within_one_lsb(matrix, full_range, bd, sd):
    sample, D = sd
    rng = np.random.default_rng(matrix * 100 + bd * 3 + full_range)
    Y = rng.integers(0, 1 << bd, (32, 48))
    U = rng.integers(0, 1 << bd, (32, 48))
    V = rng.integers(0, 1 << bd, (32, 48))
    rgb, D2 = M.rgb_int([Y, U, V], bd, 3, sample, matrix=matrix, full_range=bool(full_range))
    assert D2 == D
    want = M.float_rgb(Y, U, V, bd, matrix, full_range, D)
    for c in range(3):
        assert np.max(np.abs(rgb[..., c] - want[c])) <= 1.0, c


def one_pixel(y, u, v, bd, sample, matrix=1, full_range=False):
    rgb, _ = M.rgb_int([np.array([[y]]), np.array([[u]]), np.array([[v]])], bd, 3, sample, matrix=matrix, full_range=full_range)
    return [int(x) for x in rgb[0, 0]]


@pytest.mark.parametrize("bd,sd,matrix", list(itertools.product(DEPTHS, SAMPLES_D[:2], MATRICES)))
def test_anchors(bd, sd, matrix):
    sample, D = sd
    mx, u = (1 << D) - 1, 1 << (bd - 8)
    assert one_pixel(16 * u, 128 * u, 128 * u, bd, sample, matrix) == [0, 0, 0]                 # limited black
    assert one_pixel(235 * u, 128 * u, 128 * u, bd, sample, matrix) == [mx, mx, mx]            # limited white
    grey = one_pixel(16 * u + 219 * u // 2, 128 * u, 128 * u, bd, sample, matrix)              # grey: R = G = B = its level
    assert all(abs(g - mx * (219 * u // 2) / (219 * u)) <= 1 for g in grey) and grey[0] == grey[1] == grey[2]
    assert abs(grey[0] - mx / 2) <= (mx / 219 if bd == 8 else 1)                               # mid (8 bit: 109.5 is not a code)
    top = (1 << bd) - 1
    assert one_pixel(0, 1 << (bd - 1), 1 << (bd - 1), bd, sample, matrix, True) == [0, 0, 0]    # full-range extremes
    assert one_pixel(top, 1 << (bd - 1), 1 << (bd - 1), bd, sample, matrix, True) == [mx, mx, mx]
    assert one_pixel(235 * u, 128 * u, 240 * u, bd, sample, matrix)[0] == mx                     # out of gamut: R clamps at the top
    assert one_pixel(16 * u, 16 * u, 128 * u, bd, sample, matrix)[2] == 0                        # ... and B at zero


# BT.709 75 % colour bars: (Y, Cb, Cr) -> (R, G, B), 8-bit limited range, as published (ITU-R BT.2111 / SMPTE RP 219 75 % bars)
BARS_709 = [((180, 128, 128), (191, 191, 191)), ((168, 44, 136), (191, 191, 0)), ((145, 147, 44), (0, 191, 191)),
            ((133, 63, 52), (0, 191, 0)), ((63, 193, 204), (191, 0, 191)), ((51, 109, 212), (191, 0, 0)),
            ((28, 212, 120), (0, 0, 191)), ((16, 128, 128), (0, 0, 0))]


@pytest.mark.parametrize("bd", DEPTHS)
def test_bt709_colour_bars(bd):
    u = 1 << (bd - 8)
    for (y, cb, cr), want in BARS_709:
        got = one_pixel(y * u, cb * u, cr * u, bd, E.CONV_U8, 1)
        assert all(abs(g - w) <= 1 for g, w in zip(got, want)), ((y, cb, cr), got, want)


@pytest.mark.parametrize("cf", (1, 2))
def test_linear_chroma_reproduces_a_ramp_and_clamps_at_the_edges(cf):
    hs, vs = M.shifts(cf)
    W, H = 64, 32
    wc, hc = W >> hs, H >> vs
    j, i = np.mgrid[0:hc, 0:wc]
    C = 16 * i + 32 * j + 100                                 # linear in x and y, even steps: the filter's positions are exact
    up = M.upsample(C, cf, True, W, H, 10)
    y, x = np.mgrid[0:H, 0:W]
    cx = x / 2.0                                              # type 0 siting: co-sited with the even luma columns
    cy = (y - 0.5) / 2.0 if vs else y.astype(np.float64)      # 4:2:0: chroma row j between luma rows 2j and 2j + 1
    want = 16 * cx + 32 * cy + 100
    inner = (x < W - 1) & ((y > 0) & (y < H - 1) if vs else True)
    assert np.all(np.abs(up[inner] - want[inner]) <= 0.5)
    # the edges clamp to the coded plane: the last (odd) column takes the last chroma column twice, i.e. the value of the column before
    assert np.array_equal(up[:, W - 1], up[:, W - 2])
    if vs:                                                    # the first and last luma rows take their own chroma row twice
        h_first = M._hfilter(C, np.zeros(1, int), np.arange(W))[0]
        h_last = M._hfilter(C, np.full(1, hc - 1), np.arange(W))[0]
        assert np.array_equal(up[0], (h_first + 1) >> 1) and np.array_equal(up[H - 1], (h_last + 1) >> 1)
    nearest = M.upsample(C, cf, False, W, H, 10)
    assert np.array_equal(nearest, C[(np.arange(H) >> vs)[:, None], (np.arange(W) >> hs)[None, :]])


def test_planar_and_semiplanar_models():
    rng = np.random.default_rng(5)
    p = F.pic_params(16, 8, bit_depth=10, chroma_format_idc=1)
    planes = [rng.integers(0, 1024, (8, 16)), rng.integers(0, 1024, (4, 8)), rng.integers(0, 1024, (4, 8))]
    win = (2, 4, 2, 0)
    ys, cb, cr = planes[0][2:, 2:12], planes[1][1:, 1:6], planes[2][1:, 1:6]
    planar = M.convert(planes, p, "planar", E.CONV_NATIVE, win)
    assert planar.dtype == np.uint16 and planar.shape == ((6 * 10 + 2 * 3 * 5) // 10, 10)
    assert np.array_equal(planar.ravel(), np.concatenate([ys.ravel(), cb.ravel(), cr.ravel()]))
    semi = M.convert(planes, p, "semiplanar", E.CONV_NATIVE, win).ravel()
    assert np.array_equal(semi[:60], ys.ravel() << 6)
    assert np.array_equal(semi[60::2], cb.ravel() << 6) and np.array_equal(semi[61::2], cr.ravel() << 6)
    u8 = M.convert(planes, p, "planar", E.CONV_U8, win).ravel()
    assert u8.dtype == np.uint8 and np.array_equal(u8[:60], np.minimum((ys.ravel() + 2) >> 2, 255))
    assert M.convert([planes[0][:, :] & 255], F.pic_params(16, 8, chroma_format_idc=0), "planar", E.CONV_U8).shape == (8, 16)


def bytes_of(w, h, bd, cf, fmt, sample, win=(0, 0, 0, 0), matrix=1):
    return E.convert_image_bytes(F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf), E.make_convert(fmt, sample, win, matrix))


def test_image_bytes():
    assert bytes_of(1920, 1088, 8, 1, "planar", E.CONV_NATIVE, (0, 0, 0, 8)) == 1920 * 1080 * 3 // 2
    assert bytes_of(1920, 1088, 10, 1, "semiplanar", E.CONV_NATIVE, (0, 0, 0, 8)) == 1920 * 1080 * 3
    assert bytes_of(1920, 1088, 10, 1, "planar", E.CONV_U8, (0, 0, 0, 8)) == 1920 * 1080 * 3 // 2
    assert bytes_of(64, 64, 12, 2, "planar", E.CONV_NATIVE) == 64 * 64 * 2 * 2
    assert bytes_of(64, 64, 12, 3, "semiplanar", E.CONV_U8) == 64 * 64 * 3
    assert bytes_of(64, 64, 8, 0, "planar", E.CONV_NATIVE) == 64 * 64
    assert bytes_of(40, 24, 10, 3, "rgb_planar", E.CONV_F32, (1, 2, 0, 3)) == 37 * 21 * 3 * 4
    assert bytes_of(40, 24, 10, 1, "rgb", E.CONV_U8) == 40 * 24 * 3
    assert bytes_of(40, 24, 10, 1, "rgba", E.CONV_F16) == 40 * 24 * 4 * 2
    assert bytes_of(40, 24, 8, 0, "rgba", E.CONV_U16) == 40 * 24 * 4 * 2


@pytest.mark.parametrize("case", [
    (64, 64, 8, 1, "planar", E.CONV_NATIVE, (1, 0, 0, 0), 1),        # window offset not a multiple of SubWidthC
    (64, 64, 8, 1, "planar", E.CONV_NATIVE, (0, 0, 0, 1), 1),        # ... of SubHeightC
    (64, 64, 8, 2, "rgb", E.CONV_U8, (0, 3, 0, 0), 1),
    (64, 64, 8, 1, "rgb", E.CONV_U8, (32, 32, 0, 0), 1),             # empty
    (64, 64, 8, 1, "rgb", E.CONV_U8, (0, 0, 40, 40), 1),
    (64, 64, 8, 1, "rgb", E.CONV_U8, (-2, 0, 0, 0), 1),
    (64, 64, 8, 0, "semiplanar", E.CONV_NATIVE, (0, 0, 0, 0), 1),    # 4:0:0 has no semi-planar form
    (64, 64, 10, 1, "planar", E.CONV_F32, (0, 0, 0, 0), 1),          # YUV takes NATIVE or U8
    (64, 64, 10, 1, "planar", E.CONV_U16, (0, 0, 0, 0), 1),
    (64, 64, 10, 1, "rgb", E.CONV_NATIVE, (0, 0, 0, 0), 1),          # RGB has no native sample
    (64, 64, 10, 1, "rgb", E.CONV_U8, (0, 0, 0, 0), 4),              # matrix outside {1, 5, 6, 9}
    (64, 64, 10, 1, "rgba", E.CONV_U8, (0, 0, 0, 0), 2),
    (64, 64, 10, 1, 7, E.CONV_U8, (0, 0, 0, 0), 1),                  # unknown format
])
def test_invalid_combinations_have_no_image_size(case):
    w, h, bd, cf, fmt, sample, win, matrix = case
    assert bytes_of(w, h, bd, cf, fmt, sample, win, matrix) == 0


def test_odd_windows_in_444_and_monochrome_are_valid():
    assert bytes_of(64, 64, 8, 3, "rgb", E.CONV_U8, (1, 2, 3, 0)) == 61 * 61 * 3
    assert bytes_of(64, 64, 8, 0, "planar", E.CONV_NATIVE, (3, 0, 1, 0)) == 61 * 63
    assert bytes_of(64, 64, 8, 2, "planar", E.CONV_NATIVE, (2, 0, 1, 0)) == 62 * 63 * 2


def test_coefficients_arguments():
    L = E.lib()
    out = (C.c_int32 * E.CONV_NCOEFFS)()
    cv = E.make_convert("rgb", E.CONV_U8)
    assert L.oh_convert_coeffs(C.byref(cv), 10, out, E.CONV_NCOEFFS) == 0
    assert L.oh_convert_coeffs(C.byref(cv), 10, out, E.CONV_NCOEFFS - 1) == E.OH_E_ARG
    assert L.oh_convert_coeffs(C.byref(cv), 11, out, E.CONV_NCOEFFS) == E.OH_E_ARG
    assert L.oh_convert_coeffs(C.byref(E.make_convert("rgb", E.CONV_U8, matrix=4)), 10, out, E.CONV_NCOEFFS) == E.OH_E_UNSUPPORTED
    assert L.oh_convert_coeffs(C.byref(E.make_convert("planar", E.CONV_U8)), 10, out, E.CONV_NCOEFFS) == E.OH_E_UNSUPPORTED
    assert E.convert_coeffs(E.make_convert("rgb", E.CONV_U8, matrix=5), 8) == E.convert_coeffs(E.make_convert("rgb", E.CONV_U8, matrix=6), 8)


def test_convert_without_an_engine_is_an_argument_error():
    """no engine, no OhConvert: OH_E_ARG before anything touches a device"""
    L = E.lib()
    ids = (C.c_int * 1)(0)
    cv = E.make_convert("rgb", E.CONV_U8)
    assert L.oh_pics_convert(None, ids, 1, C.byref(cv), None, 0, 0) == E.OH_E_ARG
