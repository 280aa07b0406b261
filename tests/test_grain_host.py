"""The host arithmetic of the film grain service (openhevc_amd/csrc/pics_math.hip: oh_grain_*) — no GPU.  The pattern
builder is held against the CPU oracle's inverse transform (oh_or_idct) and against the numpy model of tests/grain_model.py, every other
helper against the model; then statistical properties that do not depend on the model: the patterns' RMS, the share of their energy
outside the band, and the standard deviation of the grain on a flat plane composed from the library's own helpers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grain_model as GM                                                    # noqa: E402
from oracle_lib import i16p, oracle                                         # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

CUT_PAIRS = [(fh, fv) for fh in GM.CUTS for fv in GM.CUTS]


@pytest.fixture(scope="module")
def patterns():
    """{(fh, fv): (coeffs, raw, pattern)} of the library, built once"""
    return {k: E.grain_pattern(*k, parts=True) for k in CUT_PAIRS}


def test_hash_and_gauss_against_the_model():
    L = E.lib()
    rng = np.random.default_rng(19)
    cases = [(0, 0, 0, 0), (0xFFFFFFFF,) * 4, (1, 2 * 16 + 2, 0, 1), (2, 0x80000000, 2, 65535 * 65536 + 65535)]
    cases += [tuple(int(v) for v in rng.integers(0, 1 << 32, 4)) for _ in range(200)]
    for a, b, c, d in cases:
        h = GM.H(a, b, c, d)
        assert E.grain_hash(a, b, c, d) == h and L.oh_grain_gauss(h) == GM.gauss(h), (a, b, c, d)
    assert GM.fmix(0) == 0 and GM.fmix(1) == 0x514E28B7                     # MurmurHash3's finaliser
    assert L.oh_grain_gauss(0) == -510 and L.oh_grain_gauss(0xFFFFFFFF) == 510 and L.oh_grain_gauss(0x80007F01) == 128 + 127 + 1 - 510


def test_raw_is_the_oracles_inverse_transform(patterns):
    o = oracle()
    for (fh, fv), (c, raw, _) in patterns.items():
        assert c.dtype == np.int16 and (c[2 * fv:, :] == 0).all() and (c[:, 2 * fh:] == 0).all() and c[0, 0] == 0
        assert np.count_nonzero(c) >= (4 * fh * fv - 1) * 0.9 and np.abs(c).max() <= 8 * 510 and not (c % 8).any()   # gauss is seldom 0
        t = c.copy()
        o.oh_or_idct(8, i16p(t), 5)
        assert np.array_equal(t, raw), (fh, fv)


def test_patterns_against_the_model(patterns):
    for (fh, fv), (c, raw, p) in patterns.items():
        mc, mraw, mp, _ = GM.pattern_parts(fh, fv)
        assert np.array_equal(c, mc) and np.array_equal(raw, mraw) and np.array_equal(p, mp), (fh, fv)
    assert len({p.tobytes() for _, _, p in patterns.values()}) == 169
    # any of the three outputs may be null; cut-offs outside 2 .. 14 are refused
    p = np.zeros((32, 32), np.int8)
    assert E.lib().oh_grain_pattern(8, 8, None, None, p.ctypes.data_as(C.POINTER(C.c_int8))) == 0 and np.array_equal(p, patterns[8, 8][2])
    assert E.lib().oh_grain_pattern(8, 8, None, None, None) == 0
    for fh, fv in ((1, 8), (8, 1), (15, 8), (8, 15), (0, 0), (-2, 8)):
        with pytest.raises(E.EngineError) as ei:
            E.grain_pattern(fh, fv)
        assert ei.value.code == E.OH_E_ARG


def test_pattern_rms_is_32(patterns):
    """every pattern has an RMS of 32 +- 1 (sigma is in units of 1/32 of a pattern's RMS).  127 is four times the RMS: at most 16 of
    the 1024 samples may be clipped, 1.6 %, so that the clip cannot move the RMS out of its bound"""
    rms = {k: float(np.sqrt((p.astype(np.float64) ** 2).mean())) for k, (_, _, p) in patterns.items()}
    r = {k: GM.isqrt(int((raw.astype(np.int64) ** 2).sum()) // 1024) for k, (_, raw, _) in patterns.items()}
    clipped = {k: int((np.abs((64 * raw.astype(np.int64) + r[k]) // (2 * r[k])) > 127).sum()) for k, (_, raw, _) in patterns.items()}
    print(f"pattern RMS {min(rms.values()):.2f} .. {max(rms.values()):.2f}, r {min(r.values())} .. {max(r.values())}, "
          f"at most {max(clipped.values())} clipped samples")
    for k in CUT_PAIRS:
        assert 31.0 <= rms[k] <= 33.0, (k, rms[k])
        assert patterns[k][2].min() >= -127 and clipped[k] <= 16, (k, clipped[k])


def test_pattern_energy_stays_in_its_band(patterns):
    """the share of a pattern's energy outside its 2 fv x 2 fh corner, measured with a float orthonormal DCT, is below 1 %: what the
    integer transform, the normalisation and the clip add"""
    k, n = np.arange(32)[:, None], np.arange(32)[None, :]
    D = np.sqrt(2.0 / 32) * np.cos((2 * n + 1) * k * np.pi / 64)
    D[0] /= np.sqrt(2.0)
    assert np.allclose(D @ D.T, np.eye(32))
    worst = 0.0
    for (fh, fv), (_, _, p) in patterns.items():
        e = (D @ p.astype(np.float64) @ D.T) ** 2
        out = 1.0 - e[:2 * fv, :2 * fh].sum() / e.sum()
        worst = max(worst, out)
        assert out < 0.01, (fh, fv, out)
    print(f"energy outside the band: at most {100 * worst:.2f} %")


def library_flat_plane(w, h, s, fh, fv, sigma, seed, log2_scale, smooth):
    """a flat plane 0 of value s at 8 bit with uniform grain, composed from the library's own helpers and nothing of the model:
    oh_grain_block, oh_grain_pattern, oh_grain_value, oh_grain_smooth, oh_grain_blend"""
    L = E.lib()
    pat = E.grain_pattern(fh, fv).astype(np.int64)
    value = np.array([L.oh_grain_value(sigma, p, 8, log2_scale) for p in range(-127, 128)], dtype=np.int64)     # by p + 127
    g = np.zeros((h, w), dtype=np.int64)
    for by in range(h // 8):
        for bx in range(w // 8):
            ox, oy, neg = E.grain_block(seed, 0, bx, by)
            p = pat[oy:oy + 8, ox:ox + 8]
            g[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = value[(-p if neg else p) + 127]
    out = g.copy()
    if smooth:
        for x in range(w):
            if (x % 8 == 7 and x + 1 < w) or (x % 8 == 0 and x > 0):
                out[:, x] = [L.oh_grain_smooth(int(g[y, x - 1]), int(g[y, x]), int(g[y, x + 1])) for y in range(h)]
    blend = {int(v): L.oh_grain_blend(s, int(v), 8, 0) for v in np.unique(out)}
    return np.vectorize(blend.get)(out).astype(np.uint8)


@pytest.mark.parametrize("fh,fv", [(2, 2), (8, 8), (14, 14), (2, 14), (14, 2)])
def test_grain_on_a_flat_plane_has_the_standard_deviation_of_sigma(fh, fv):
    """a flat 136 x 72 plane, composed from the library's helpers: the standard deviation of out - src over sigma / 2^log2_scale
    lies in 0.75 .. 1.10; the model makes the same plane"""
    src = np.full((72, 136), 128, dtype=np.uint8)
    for sigma, ls in ((16, 2), (255, 6), (8, 0)):
        tab = [GM.uniform(sigma, fh, fv)]
        for smooth in (True, False):
            got = library_flat_plane(136, 72, 128, fh, fv, sigma, 22, ls, smooth)
            assert np.array_equal(got, GM.apply([src], 8, tab, 22, log2_scale=ls, smooth=smooth)[0]), (sigma, ls, smooth)
            d = got.astype(np.int64) - 128
            ratio = float(d.std()) / (sigma / 2.0 ** ls)
            print(f"({fh}, {fv}) sigma {sigma} log2_scale {ls} {'smoothed' if smooth else 'unsmoothed'}: {ratio:.3f}")
            assert 0.75 <= ratio <= 1.10, (sigma, ls, smooth, ratio)
            assert abs(float(d.mean())) < 0.25 * sigma / 2.0 ** ls


def test_block_mean_value_smooth_blend_against_the_model():
    L = E.lib()
    rng = np.random.default_rng(5)
    seen = set()
    for seed in (0, 1, 0xFFFFFFFF, 12345):
        for c in range(3):
            for bx, by in [(0, 0), (65535, 65535), (1, 0), (0, 1)] + [tuple(int(v) for v in rng.integers(0, 65536, 2)) for _ in range(60)]:
                got = E.grain_block(seed, c, bx, by)
                assert got == GM.block(seed, c, bx, by) and 0 <= got[0] <= 24 and 0 <= got[1] <= 24 and got[2] in (0, 1)
                seen.add(got)
    assert {g[0] for g in seen} == set(range(25)) and {g[1] for g in seen} == set(range(25)) and {g[2] for g in seen} == {0, 1}
    for bad in ((0, 3, 0, 0), (0, -1, 0, 0), (0, 0, 65536, 0), (0, 0, 0, -1)):
        with pytest.raises(E.EngineError):
            E.grain_block(*bad)
    for bd in (8, 9, 10, 12):
        M = (1 << bd) - 1
        for n in (64, 32, 16):
            for blk in [np.zeros(n, int), np.full(n, M), np.array([M] * (n // 2) + [M - 1] * (n // 2))] + [rng.integers(0, M + 1, n) for _ in range(20)]:
                a8 = L.oh_grain_mean(int(blk.sum()), n, bd)
                assert a8 == GM.mean8(blk, bd) and 0 <= a8 <= 255
        assert L.oh_grain_mean(100, 48, bd) == -1 and L.oh_grain_mean(100, 64, 11) == -1
        for ls in (0, 2, 6, 15):
            for sigma in (0, 1, 16, 255):
                for p in (-127, -1, 0, 1, 37, 127):
                    assert L.oh_grain_value(sigma, p, bd, ls) == GM.value(sigma, p, bd, ls), (sigma, p, bd, ls)
        for blending in (0, 1):
            for s in (0, 1, M // 2, M - 1, M):
                for g in (-16192 * 16, -300, -1, 0, 1, 300, 16192 * 16):
                    want = int(GM.blend(np.array([s]), np.array([g]), bd, blending)[0])
                    assert L.oh_grain_blend(s, g, bd, blending) == want, (s, g, bd, blending)
    for left, g, right in ((0, 0, 0), (-1, -1, -1), (-3, 0, 0), (5, -7, 100), (-16192, -16192, -16192), (16192, 0, -16191)):
        assert L.oh_grain_smooth(left, g, right) == (left + 2 * g + right + 2) >> 2


def test_uniform_and_make_grain():
    t = np.zeros(256, np.uint32)
    assert E.lib().oh_grain_uniform(40, 6, 10, t.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert np.array_equal(t, GM.uniform(40, 6, 10)) and t[0] == 40 | 6 << 8 | 10 << 12
    g = E.make_grain(25)
    assert np.array_equal(g.tables, np.stack([GM.uniform(25, 8, 8)] * 3)) and (g.planes, g.blending, g.log2_scale) == (7, 0, 0)
    g = E.make_grain(0, 2, 14, log2_scale=15, blending="multiplicative", planes=5)
    assert g.tables[2][255] == 2 << 8 | 14 << 12 and (g.planes, g.blending, g.log2_scale) == (5, 1, 15)
    for bad in ((-1, 8, 8), (256, 8, 8), (1, 1, 8), (1, 8, 15)):
        with pytest.raises(E.EngineError) as ei:
            E.make_grain(*bad)
        assert ei.value.code == E.OH_E_ARG
    assert E.lib().oh_grain_uniform(1, 8, 8, None) == E.OH_E_ARG


def sei(components, **kw):
    d = dict(cancel=False, model_id=0, colour=None, blending_mode_id=0, log2_scale_factor=0, components=components, persistence=False)
    d.update(kw)
    return d


def test_from_sei_defaults_gaps_and_fields():
    d = sei([[(16, 63, [40, 6, 10]), (100, 127, [30, 3, 3]), (128, 128, [12, 14, 2])], None, [(0, 255, [20, 5, 5])]],
            blending_mode_id=1, log2_scale_factor=5)
    g = E.grain_from_sei(d)
    ok, tabs, planes, blending, ls = GM.from_sei(d)
    assert ok == "ok" and np.array_equal(g.tables, tabs) and (g.planes, g.blending, g.log2_scale) == (planes, blending, ls) == (5, 1, 5)
    t = g.tables
    assert not t[0][:16].any() and not t[0][64:100].any() and not t[0][129:].any() and not t[1].any()      # gaps, and no model
    assert t[0][16] == t[0][63] == 40 | 6 << 8 | 10 << 12 and t[0][128] == 12 | 14 << 8 | 2 << 12 and (t[2] == 20 | 5 << 8 | 5 << 12).all()
    # missing values: fh = 8, fv = fh
    one, two = E.grain_from_sei(sei([[(0, 9, [7])], None, None])), E.grain_from_sei(sei([None, [(0, 9, [7, 3])], None]))
    assert one.tables[0][9] == 7 | 8 << 8 | 8 << 12 and one.planes == 1 and two.tables[1][0] == 7 | 3 << 8 | 3 << 12 and two.planes == 2
    # the separate colour description changes nothing
    colour = dict(bit_depth_luma=10, bit_depth_chroma=10, full_range=True, colour_primaries=9, transfer_characteristics=16, matrix_coeffs=9)
    assert np.array_equal(E.grain_from_sei(dict(d, colour=colour)).tables, t)
    # a struct read from bytes is taken as it is
    s = A.film_grain_to_struct(d)
    assert np.array_equal(E.grain_from_sei(s).tables, t)
    # sigma 0 with cut-offs is an entry without grain; 256 touching intervals
    many = sei([[(i, i, [i, 2 + i % 13, 14 - i % 13]) for i in range(256)], None, None])
    assert np.array_equal(E.grain_from_sei(many).tables, GM.from_sei(many)[1])


def test_from_sei_refusals():
    base = [(16, 63, [40, 6, 10])]
    unsupported = [sei([base, None, None], model_id=1), sei([base, None, None], blending_mode_id=2),
                   sei([[(0, 9, [1, 8, 8, 0])], None, None]), sei([[(0, 9, [1, 8, 8, 0, 0, 0])], None, None]),     # more than 3 model values
                   sei([[(0, 9, [256])], None, None]), sei([[(0, 9, [-1])], None, None]),                         # sigma
                   sei([[(0, 9, [1, 1])], None, None]), sei([[(0, 9, [1, 15])], None, None]),                     # cut-offs
                   sei([[(0, 9, [1, 8, 1])], None, None]), sei([[(0, 9, [1, 8, 15])], None, None]), sei([[(0, 9, [0, 0, 0])], None, None]),
                   sei([[(10, 9, [1])], None, None]),                                                             # lower above upper
                   sei([[(0, 9, [1]), (9, 20, [2])], None, None]), sei([None, None, [(0, 255, [1]), (7, 7, [2])]]),      # overlap
                   sei([base, [(5, 5, [1]), (0, 9, [2])], None])]
    for d in unsupported:
        assert GM.from_sei(d) == ("unsupported",), d
        with pytest.raises(E.EngineError) as ei:
            E.grain_from_sei(d)
        assert ei.value.code == E.OH_E_UNSUPPORTED, d
    assert GM.from_sei(dict(cancel=True)) == ("arg",)
    with pytest.raises(E.EngineError) as ei:
        E.grain_from_sei(dict(cancel=True))
    assert ei.value.code == E.OH_E_ARG
    with pytest.raises(E.EngineError) as ei:                                # an absent message: a struct with present 0
        E.grain_from_sei(A.OhFilmGrainSei())
    assert ei.value.code == E.OH_E_ARG
    with pytest.raises(ValueError):
        E.grain_from_sei(None)
    # a refusal leaves tables and out untouched
    L = E.lib()
    t = np.full((3, 256), 0xABCD, np.uint32)
    g = E.OhGrain(9, 9, 9)
    s = A.film_grain_to_struct(unsupported[-1])
    assert L.oh_grain_from_sei(C.byref(s), t.ctypes.data_as(C.c_void_p), C.byref(g)) == E.OH_E_UNSUPPORTED
    assert (t == 0xABCD).all() and (g.planes, g.blending, g.log2_scale) == (9, 9, 9)
    assert L.oh_grain_from_sei(None, t.ctypes.data_as(C.c_void_p), C.byref(g)) == E.OH_E_ARG
    assert L.oh_grain_from_sei(C.byref(s), None, C.byref(g)) == E.OH_E_ARG and L.oh_grain_from_sei(C.byref(s), t.ctypes.data_as(C.c_void_p), None) == E.OH_E_ARG
