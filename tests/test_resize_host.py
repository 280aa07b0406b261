"""CPU checks of the picture resizing (oh_pics_resize): the integers oh_resize_taps hands the kernels against the numpy
model (tests/resize_model.py), the model against torch's float64 anti-aliased interpolate within a bound computed from the tables,
identities and overflow margins, the chroma siting, the padding rule and the argument rules that need no device."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import resize_model as M
from openhevc_amd import engine as E

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openhevc_amd", "libohevc_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libohevc_hip.so not built (run __graft_entry__.build())")

FILTERS = ("bilinear", "bicubic")
ONE = 1 << M.PREC

# (source extent, image extent): 1, 2, odd, equal, the largest extent, 34:1, enlarging, the worst known sum of |k| (14 -> 13)
EXTENTS = [(1, 1), (1, 2), (2, 1), (1, 8), (2, 2), (2, 3), (3, 2), (5, 17), (17, 5), (7, 7), (14, 13), (13, 14), (37, 11), (53, 9), (64, 32),
           (100, 100), (200, 299), (299, 200), (208, 112), (416, 3328), (640, 1280), (1080, 224), (1920, 224), (2160, 1080), (3840, 1920),
           (3840, 224), (7680, 224), (4320, 224), (16384, 8), (16384, 16384 // 64), (2048, 16384)]


@pytest.mark.parametrize("filt,phase", list(itertools.product(FILTERS, (1, 2))))
def test_taps_equal_the_model(filt, phase):
    for S, T in EXTENTS:
        got, want = E.resize_taps(S, T, filt, phase), M.taps(S, T, filt, phase)
        assert len(got) == len(want) == T
        mt = E.lib().oh_resize_max_taps(S, T, E.resize_filter(filt))
        assert mt == M.max_taps(S, T, filt)
        for x, ((gf, gk), (wf, wk, _)) in enumerate(zip(got, want)):
            assert gf == wf and gk == wk, (S, T, x)
            assert 1 <= len(gk) <= mt and 0 <= gf and gf + len(gk) <= S, (S, T, x)
            assert sum(gk) == ONE, (S, T, x)
            assert sum(abs(k) for k in gk) < 1 << 15, (S, T, x)
            if filt == "bilinear" and S <= 64 * T:          # beyond, the remainder can outweigh the largest of thousands of tiny taps
                assert min(gk) >= 0, (S, T, x)


def test_worst_known_coefficients():
    """14 -> 13 bicubic: the largest sum of |k| found over 10 348 geometries"""
    assert E.resize_taps(14, 13, "bicubic", 2)[6] == (5, [-1101, 9293, 9293, -1101])


# ---- the model against torch (float64, antialias=True) ----
GEOMS = [(64, 48, 32, 24), (416, 240, 224, 224), (200, 120, 299, 171), (1920, 1080, 224, 224), (3840, 2160, 224, 224), (3840, 2160, 1920, 1080),
         (640, 360, 1280, 720), (100, 100, 100, 100), (37, 53, 11, 9)]


def gain_and_quantisation(S, T, filt):
    """g = max_x sum |k| / 2^14, q = max_x sum_i |k_i / 2^14 - w_i / sum w|"""
    g = q = 0.0
    for _, k, w in M.taps(S, T, filt, 2):
        g = max(g, sum(abs(v) for v in k) / ONE)
        q = max(q, sum(abs(a / ONE - b) for a, b in zip(k, w)))
    return g, q


def images(ws, hs, bd, rng):
    mx = (1 << bd) - 1
    yy, xx = np.mgrid[0:hs, 0:ws]
    return {"noise": rng.integers(0, 1 << bd, (hs, ws)), "two_level": mx * rng.integers(0, 2, (hs, ws)),
            "smooth": np.clip(mx * (0.5 + 0.5 * np.sin(xx / 37.0) * np.cos(yy / 23.0)), 0, mx).astype(np.int64)}


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("geom", GEOMS, ids=["%dx%d_%dx%d" % g for g in GEOMS])
def test_model_against_torch_float64(geom, filt):
    """|model - clamp(torch)| <= 1/2 (final rounding) + 2^(B-15) g_v (the intermediate's rounding through the vertical gain)
    + (2^B - 1)(q_h g_v + q_v g_h) (coefficient quantisation of each pass through the other's gain)"""
    import torch
    import torch.nn.functional as TF
    ws, hs, wd, hd = geom
    (g_h, q_h), (g_v, q_v) = gain_and_quantisation(ws, wd, filt), gain_and_quantisation(hs, hd, filt)
    rng = np.random.default_rng(ws + hd)
    for bd in (8, 10, 12):
        mx = (1 << bd) - 1
        bound = 0.5 + 2.0 ** (bd - 15) * g_v + mx * (q_h * g_v + q_v * g_h)
        for name, src in images(ws, hs, bd, rng).items():
            got = M.resize_plane(src, wd, hd, bd, filt)
            t = torch.from_numpy(src.astype(np.float64))[None, None]
            ref = TF.interpolate(t, size=(hd, wd), mode=filt, antialias=True, align_corners=False)[0, 0].numpy()
            diff = float(np.abs(got - np.clip(ref, 0, mx)).max())
            print(f"{filt} {bd} bit {ws}x{hs} -> {wd}x{hd} {name}: |model - torch| {diff:.3f}, bound {bound:.3f}")
            assert diff <= bound, (bd, name, diff, bound)
            exact = M.resize_plane_exact(src, wd, hd, filt)
            assert np.abs(exact - ref).max() < 1e-9 * mx, (bd, name)   # the definition with float64 weights is torch's


# ---- identities and overflow margins ----
@pytest.mark.parametrize("filt", FILTERS)
def test_equal_sizes_return_the_source(filt):
    rng = np.random.default_rng(3)
    for bd, (w, h), (ph, pv) in itertools.product((8, 9, 10, 12), ((1, 1), (7, 5), (64, 33)), ((2, 2), (1, 2))):
        src = rng.integers(0, 1 << bd, (h, w))
        assert np.array_equal(M.resize_plane(src, w, h, bd, filt, ph, pv), src), (bd, w, h, ph)


@pytest.mark.parametrize("filt", FILTERS)
def test_constant_planes_stay_constant(filt):
    for bd, (ws, hs, wd, hd) in itertools.product((8, 9, 10, 12), ((64, 48, 5, 7), (5, 7, 40, 41), (130, 9, 2, 72), (37, 53, 11, 9), (14, 14, 13, 13))):
        for v in (0, 1 << (bd - 1), (1 << bd) - 1):
            for ph in (1, 2):
                assert np.all(M.resize_plane(np.full((hs, ws), v), wd, hd, bd, filt, ph, 2) == v), (bd, ws, hs, wd, hd, v, ph)


def test_extreme_two_level_images_stay_inside_int16_and_int32():
    """the image that drives an output hardest takes 2^B - 1 where its coefficient is positive and 0 elsewhere (or the reverse):
    the intermediate stays inside int16 and every vertical sum, rounding included, inside int32 (evaluated in Python integers)"""
    pairs = [(S, T) for S in range(1, 40) for T in range(1, 40)] + [(14, 13), (3840, 224), (224, 1792), (1920, 30), (53, 9)]
    for S, T in pairs:
        if S > 64 * T or T > 8 * S:
            continue
        for ph in (1, 2):
            pos = max(sum(v for v in k if v > 0) for _, k, _ in M.taps(S, T, "bicubic", ph))
            neg = min(sum(v for v in k if v < 0) for _, k, _ in M.taps(S, T, "bicubic", ph))
            for bd in (8, 9, 10, 12):
                mx = (1 << bd) - 1
                m_hi, m_lo = (pos * mx + (1 << (bd - 1))) >> bd, (neg * mx + (1 << (bd - 1))) >> bd
                assert -32768 <= m_lo <= 0 <= m_hi <= 32767, (S, T, bd)
                # any vertical filter of the grid over such intermediates
                hi = pos * m_hi + neg * m_lo + (1 << (27 - bd))
                lo = pos * m_lo + neg * m_hi + (1 << (27 - bd))
                assert -2 ** 31 <= lo and hi < 2 ** 31, (S, T, bd)
    # and on an actual image: 14 -> 13, the worst known taps on both axes
    for bd in (8, 12):
        mx = (1 << bd) - 1
        kx = np.zeros(14, np.int64)
        lo, k, _ = M.taps(14, 13, "bicubic", 2)[6]
        kx[lo:lo + len(k)] = k
        src = np.where(np.outer(kx, kx) > 0, mx, 0)
        out = M.resize_plane(src, 13, 13, bd, "bicubic")          # check=True asserts both ranges
        assert out[6, 6] == mx and out.min() >= 0


# ---- chroma siting ----
def lib_line(S, T, filt, phase, line):
    """one axis of a ramp through the LIBRARY's integers, in float (no rounding)"""
    return np.array([sum(k * line[f + j] for j, k in enumerate(ks)) / ONE for f, ks in E.resize_taps(S, T, filt, phase)])


def exact_line(S, T, filt, phase, line):
    return np.array([sum(w * line[f + j] for j, w in enumerate(ws)) for f, _, ws in M.taps(S, T, filt, phase)])


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("S,T", [(208, 112), (104, 208), (120, 299), (540, 112)])
def test_chroma_ramp_lands_on_the_cosited_line(S, T, filt):
    """a ramp of step 4 per source sample: horizontally through phase 1 it comes out on (x + 1/4) S / T - 1/4, through phase 2 (and
    vertically) on (x + 1/2) S / T - 1/2.  Enlarging, both filters reproduce a line: within 1 LSB (the two roundings of the model).
    Shrinking, within 1 LSB of the float64 evaluation of the same taps, which stays within a quarter of the step of the line."""
    bd, step, base = 12, 4, 100
    R = 1 if filt == "bilinear" else 2
    edge = int(np.ceil(R * max(1.0, S / T)))                  # image samples whose taps the window's edge may have cut
    wide = int(np.ceil(R * max(T / S, S / T))) + 1            # ... or re-normalised by any amount (the float checks below)
    ramp = base + step * np.arange(S)
    xs, xw = np.arange(T)[edge:T - edge], np.arange(T)[wide:T - wide]
    rows = 16
    qb = {}
    for phase, u in ((1, (np.arange(T) + 0.25) * S / T - 0.25), (2, (np.arange(T) + 0.5) * S / T - 0.5)):
        line = base + step * u
        exact = exact_line(S, T, filt, phase, ramp)
        got = [M.resize_plane(np.tile(ramp, (rows, 1)), T, rows, bd, filt, phase, 2)[rows // 2]]
        if phase == 2:                                        # the vertical axis of every plane is centred
            got.append(M.resize_plane(np.tile(ramp[:, None], (1, rows)), rows, T, bd, filt, 1, 2)[:, rows // 2])
        for g in got:
            if T >= S:
                assert np.abs(g[xs] - line[xs]).max() <= 1.0, (phase,)
            else:
                assert np.abs(g[xs] - exact[xs]).max() <= 1.0, (phase,)
        if T < S:
            dev = np.abs(exact[xs] - line[xs]).max()
            print(f"{filt} {S} -> {T} phase {phase}: float64 taps within {dev / step:.3f} of a step of the line")
            assert dev <= step / 4, (phase, dev)
        else:
            assert np.abs(exact[xw] - line[xw]).max() <= 1e-9 * ramp.max(), (phase,)
        # the library's integers: off the float64 weights by at most their quantisation times the largest sample
        qb[phase] = max(sum(abs(k / ONE - w) for k, w in zip(ks, ws)) for _, ks, ws in M.taps(S, T, filt, phase)) * ramp.max()
        assert np.abs(lib_line(S, T, filt, phase, ramp) - exact).max() <= qb[phase] + 1e-9
    # ignoring the phase displaces the result by (S / T - 1) / 4 chroma samples: each result lies on its own line, exactly (to the
    # quantisation) when enlarging, within a quarter of a step when shrinking
    want = step * (S / T - 1) / 4
    slack = qb[1] + qb[2] + (0 if T >= S else step / 2)
    d = lib_line(S, T, filt, 2, ramp)[xw] - lib_line(S, T, filt, 1, ramp)[xw]
    assert np.abs(d - want).max() <= slack
    if abs(want) > slack:                                     # every sample moves, and the right way
        assert np.all(np.sign(d) == np.sign(want))


def test_chroma_planes_of_a_picture_use_the_cosited_columns():
    rng = np.random.default_rng(8)
    for cf, (w, h), size in ((1, (64, 48), (40, 30)), (2, (64, 48), (100, 31)), (3, (63, 47), (41, 29)), (0, (63, 47), (41, 29))):
        planes = [rng.integers(0, 1024, (h >> (M.shifts(cf, c)[1]), w >> (M.shifts(cf, c)[0]))) for c in range(3 if cf else 1)]
        out = M.resize(planes, cf, 10, size, "bicubic")
        for c, pl in enumerate(planes):
            hs, vs = M.shifts(cf, c)
            assert np.array_equal(out[c], M.resize_plane(pl, size[0] >> hs, size[1] >> vs, 10, "bicubic", 1 if c and hs else 2, 2)), (cf, c)
    # a window is cut out of the planes before anything is filtered: samples outside it never take part
    planes = [rng.integers(0, 256, (48, 64)), rng.integers(0, 256, (24, 32)), rng.integers(0, 256, (24, 32))]
    out = M.resize(planes, 1, 8, (20, 10), "bilinear", (4, 8, 2, 6))
    cut = [planes[0][2:42, 4:56], planes[1][1:21, 2:28], planes[2][1:21, 2:28]]
    assert all(np.array_equal(a, b) for a, b in zip(out, M.resize(cut, 1, 8, (20, 10), "bilinear")))


# ---- padding and the argument rules that need no device ----
def test_padding_replicates_the_last_column_and_row():
    img = [np.arange(6).reshape(2, 3), np.array([[7]]), np.array([[9]])]
    y, cb, cr = M.pad_to(img, 1, (8, 8))
    assert y.shape == (8, 8) and cb.shape == (4, 4) and cr.shape == (4, 4)
    assert np.array_equal(y[:2, :3], img[0]) and np.all(y[0, 3:] == 2) and np.all(y[1:, 3:] == 5) and np.array_equal(y[5, :3], [3, 4, 5])
    assert np.all(cb == 7) and np.all(cr == 9)
    same = M.pad_to(img, 1, (3, 2))
    assert all(np.array_equal(a, b) for a, b in zip(same, img))


def test_argument_rules_without_a_device():
    L = E.lib()
    rs = E.OhResize(0, E.OhWindow(0, 0, 0, 0), 16, 16)
    ids = (C.c_int * 1)(0)
    assert L.oh_pics_resize(None, ids, ids, 1, C.byref(rs)) == E.OH_E_ARG
    assert L.oh_pics_resize(None, ids, ids, 0, C.byref(rs)) == E.OH_E_ARG

    def taps(S, T, filt, phase, room):
        first, cnt, k = (C.c_int32 * max(T, 1))(), (C.c_int * max(T, 1))(), (C.c_int16 * (max(T, 1) * max(room, 1)))()
        return L.oh_resize_taps(S, T, filt, phase, first, k, room, cnt)

    assert L.oh_resize_max_taps(3840, 224, 0) == 35 and L.oh_resize_max_taps(3840, 224, 1) == 69
    assert L.oh_resize_max_taps(224, 3840, 0) == 2 and L.oh_resize_max_taps(224, 3840, 1) == 4 and L.oh_resize_max_taps(1, 5, 1) == 1
    assert taps(3840, 224, 1, 2, 69) == 0
    assert taps(3840, 224, 1, 2, 68) == E.OH_E_ARG                          # too little room
    assert taps(3840, 224, 0, 2, 0) == E.OH_E_ARG
    for S, T in ((0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385)):
        assert taps(S, T, 0, 2, 64) == E.OH_E_ARG, (S, T)
        assert L.oh_resize_max_taps(S, T, 0) == E.OH_E_ARG, (S, T)
    assert taps(64, 32, 2, 2, 16) == E.OH_E_ARG and taps(64, 32, -1, 2, 16) == E.OH_E_ARG      # unknown filter
    assert L.oh_resize_max_taps(64, 32, 2) == E.OH_E_ARG
    assert taps(64, 32, 0, 0, 16) == E.OH_E_ARG and taps(64, 32, 0, 3, 16) == E.OH_E_ARG       # unknown phase
    first, cnt = (C.c_int32 * 32)(), (C.c_int * 32)()
    assert L.oh_resize_taps(64, 32, 0, 2, first, None, 16, cnt) == E.OH_E_ARG
    with pytest.raises(E.EngineError):
        E.resize_taps(0, 8)
    with pytest.raises(ValueError):
        E.resize_taps(8, 8, "lanczos")
