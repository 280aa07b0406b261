"""CPU: the integers of oh_colour_tables against the curves in numpy float64, the integer model of tests/colour_model.py (which uses
those tables) against the same stages in float64, and the refusal rules.  No device."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import colour_model as M                                                    # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

SRC_PEAK = {16: 1000.0, 18: 1000.0, 13: 203.0, 1: 203.0}
COMBOS = [(t, o, tone, norm) for t, o, tone, norm in itertools.product((16, 18, 13, 1), ("linear", "srgb", "gamma24"), ("none", "bt2390"),
                                                                       ("maxrgb", "luma")) if not (t == 18 and norm == "maxrgb")]


def colour(t, out, tone, norm, in_prim=9, out_prim=1, **kw):
    kw.setdefault("src_peak", SRC_PEAK[t])
    return E.make_colour(t, in_prim, out=out, out_primaries=out_prim, tone=tone, norm=norm, **kw)


def fixed(row, q=14):
    """a row of fractions summing to 1 with q fraction bits, corrected on its largest entry"""
    k = [int(np.floor(v * (1 << q) + 0.5)) for v in row]
    k[int(np.argmax(k))] += (1 << q) - sum(k)
    return k


@pytest.mark.parametrize("t,out,tone,norm", COMBOS, ids=["-".join(map(str, c)) for c in COMBOS])
def test_tables_equal_the_curves_in_float64(t, out, tone, norm):
    col = colour(t, out, tone, norm)
    A, G, B, misc = [x.astype(np.int64) for x in E.colour_tables(col)]
    Lfs = M.full_scale(col)
    wantA = np.rint(2.0**30 * M.source_curve(t, 16 * np.arange(E.COL_NA) / 65535))
    assert np.abs(A - wantA).max() <= 1
    assert A[0] == 0 and np.all(np.diff(A) >= 0)
    x = M.nodes() / 2.0**30
    wantG = np.rint(2.0**20 * M.gain(col, x))
    assert np.abs(G - wantG).max() <= 1
    assert G.max() <= 1 << 20
    if tone == "none" and t != 18:
        assert np.all(G == 1 << 20) and misc[15] == 0
    else:
        assert misc[15] == 1
    if out == "linear":
        assert misc[13] == 0 and np.all(B == 0)
        K = np.array([misc[14]], np.int32).view(np.float32)[0]
        assert K == np.float32(Lfs / (203.0 * 2.0**30))
    else:
        wantB = np.rint(65535 * M.output_curve(col, x * Lfs / 100.0))
        assert np.abs(B - wantB).max() <= 1
        assert np.all(np.diff(B) >= 0) and misc[13] == 1
        assert np.abs(np.diff(B[128:])).max() < 1 << 19
    assert np.abs(np.diff(G[128:])).max() < 1 << 19 and np.abs(np.diff(A)).max() < 1 << 24
    assert misc[12] == E.COL_NORM[norm]
    assert [int(sum(misc[3 * r:3 * r + 3])) for r in range(3)] == [1 << 20] * 3 and int(sum(misc[9:12])) == 16384 and misc[16] == 1


def test_matrices_from_the_chromaticities():
    """BT.2020 -> BT.709 and the luminance weights, derived here from the chromaticities and the D65 white"""
    def to_xyz(prim, white=(0.3127, 0.3290)):
        P = np.array([[x / y, 1.0, (1 - x - y) / y] for x, y in prim]).T
        S = np.linalg.inv(P) @ np.array([white[0] / white[1], 1.0, (1 - white[0] - white[1]) / white[1]])
        return P @ np.diag(S)

    p709 = ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060))
    p2020 = ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))
    p3 = ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))
    for (ci, pi), (co, po) in itertools.product(((1, p709), (9, p2020), (12, p3)), repeat=2):
        misc = E.colour_tables(E.make_colour(16, ci, out="srgb", out_primaries=co))[3].astype(np.int64)
        Mq = misc[:9].reshape(3, 3)
        assert list(Mq.sum(axis=1)) == [1 << 20] * 3 and int(misc[9:12].sum()) == 16384
        assert np.abs(misc[9:12] - np.array(fixed(to_xyz(pi)[1]))).max() <= 1
        if ci == co:
            assert np.array_equal(Mq, (1 << 20) * np.eye(3, dtype=np.int64)) and misc[16] == 0
        else:
            want = np.array([fixed(r, 20) for r in np.linalg.inv(to_xyz(po)) @ to_xyz(pi)])
            assert np.abs(Mq - want).max() <= 1, (ci, co)
    # the BT.2087 figures of the 2020 -> 709 matrix, to the table's precision
    m = E.colour_tables(E.make_colour(16, 9, out="srgb", out_primaries=1))[3][:9].reshape(3, 3) / 2.0**20
    assert np.abs(m - np.array([[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]])).max() < 2e-4


def triples(n=400_000, seed=2084):
    """random R'G'B' over the full 16-bit range; one twentieth greys, one twentieth near black (every channel below 4096)"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 65536, (n, 3), dtype=np.int64)
    g = n // 20
    v[:g] = v[:g, :1]
    v[g:2 * g] = rng.integers(0, 4096, (g, 3), dtype=np.int64)
    return v


PIPELINES = {
    "pq2020_srgb709": dict(t=16, out="srgb", tone="bt2390", norm="maxrgb", src_peak=1000.0, dst_peak=100.0),
    "hlg2020_gamma24_709": dict(t=18, out="gamma24", tone="bt2390", norm="luma", src_peak=1000.0, dst_peak=100.0),
    "srgb709_linear": dict(t=13, out="linear", tone="none", norm="maxrgb", in_prim=1, src_peak=100.0),
}


def pipeline(name):
    return colour(**PIPELINES[name])


@pytest.mark.parametrize("name", ["pq2020_srgb709", "hlg2020_gamma24_709"])
def test_integer_model_against_float64_codes(name):
    """U8: at most 1 code apart, on at most 0.5 % of the samples.  U16: at most 8 apart — with GAMMA24 where the float64 result of every
    channel is at least 4096 (the pure power law has unbounded slope at 0).  Measured: PQ -> sRGB: U16 maximum 3.04,
    mean 0.13, U8 differing by 1 on 0.037 %; HLG -> GAMMA24: U16 maximum 2.73 at or above 4096 and 45 below it, U8 differing by 1 on
    0.055 %.  With the primaries' matrix in Q14 the U16 maxima were 26 and 110: an entry's rounding of 3e-5 times a bright channel lands
    on a dark one; hence Q20."""
    col = pipeline(name)
    v = triples()
    by_table, got = M.stages(v, col)
    _, want = M.float_pipeline(v, col)
    assert by_table
    d16 = np.abs(got - want)
    sel = np.ones(len(v), bool) if col.out_transfer == E.COL_OUT["srgb"] else (want >= 4096).all(axis=-1)
    got8 = M.out_samples(True, got, E.CONV_U8, None).astype(np.int64)
    want8 = np.floor(want / 257 + 0.5).astype(np.int64)
    d8 = np.abs(got8 - want8)
    print(f"{name}: u16 max {d16[sel].max():.2f} mean {d16[sel].mean():.3f} (of {sel.sum()} triples; elsewhere max "
          f"{d16[~sel].max() if (~sel).any() else 0:.1f}); u8 max {d8.max()} differing {100 * (d8 > 0).mean():.4f} %")
    assert d8.max() <= 1
    assert (d8 > 0).mean() <= 0.005
    assert d16[sel].max() <= 8


def test_integer_model_against_float64_linear():
    """sRGB -> LINEAR f32.  The bound is 2^-22 of the full scale: the chord of a 16-code segment of the sRGB curve lies within
    h^2 / 8 * max E'' = (16 / 65535)^2 / 8 * 3.02 = 2.3e-8 of it, within slope step * h / 4 = 8.5e-8 in the one segment that holds
    the curve's join at 0.04045, the Q30 table and interpolation roundings add 2e-9 and the f32 result 2^-24 = 6e-8 of its value:
    1.7e-7 in all, below 2^-22 = 2.4e-7.  Measured: 9.0e-8."""
    col = pipeline("srgb709_linear")
    v = triples()
    tables = E.colour_tables(col)
    by_table, m = M.stages(v, col, tables)
    assert not by_table and m.max() <= 1 << 30
    got = M.out_samples(False, m, E.CONV_F32, M.k_linear(col, tables)).astype(np.float64)
    _, want = M.float_pipeline(v, col)
    scale = 100.0 / 203.0                                                   # full scale over white
    d = np.abs(got - want * scale) / scale
    print(f"srgb709_linear: f32 max error {d.max():.3e} of the full scale")
    assert d.max() <= 2.0**-22
    h = M.out_samples(False, m, E.CONV_F16, M.k_linear(col, tables))
    assert np.array_equal(h, got.astype(np.float32).astype(np.float16))


def test_saturated_and_black_inputs_reach_the_ends():
    """the tables hold the smooth curves and the clips are the kernel's: a saturated PQ input comes out at 65535, black at 0"""
    for name in ("pq2020_srgb709", "hlg2020_gamma24_709"):
        _, c = M.stages(np.array([[65535, 65535, 65535], [0, 0, 0]], np.int64), pipeline(name))
        assert c[0].tolist() == [65535] * 3 and c[1].tolist() == [0] * 3, name
    col = colour(16, "linear", "none", "maxrgb", white=10000.0)
    _, m = M.stages(np.array([[65535, 65535, 65535]], np.int64), col)
    assert m[0].tolist() == [1 << 30] * 3
    f = M.out_samples(False, np.array([1 << 30]), E.CONV_F16, np.float32(2.0**-10))   # 2^20: past the f16 range
    assert f.view(np.uint16)[0] == 0x7BFF


def test_refusals():
    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    L = E.lib()
    P = C.POINTER(C.c_int32)
    bufs = [np.full(n, 77, np.int32) for n in (E.COL_NA, E.COL_NP, E.COL_NP, E.COL_NMISC)]

    def rc(col):
        return L.oh_colour_tables(C.byref(col) if col is not None else None, *[b.ctypes.data_as(P) for b in bufs])

    ok = E.make_colour(16, 9)
    assert rc(None) == arg
    for field, bad in (("out_transfer", 3), ("out_transfer", -1), ("tone", 2), ("tone", -1), ("norm", 2), ("norm", -1)):
        col = E.make_colour(16, 9)
        setattr(col, field, bad)
        assert rc(col) == arg, (field, bad)
    for field, bad in itertools.product(("src_peak", "dst_peak", "white"), (0.0, -1.0, float("inf"), float("nan"))):
        col = E.make_colour(16, 9)
        setattr(col, field, bad)
        assert rc(col) == arg, (field, bad)
    for t in (0, 2, 4, 8, 17, 19):
        assert rc(E.make_colour(t, 9)) == uns, t
    for prim in (0, 2, 5, 10, 11, 22):
        assert rc(E.make_colour(16, prim)) == uns and rc(E.make_colour(16, 9, out_primaries=prim)) == uns, prim
    assert rc(E.make_colour(18, 9, norm="maxrgb")) == uns
    for pk in (399.0, 10001.0):
        assert rc(E.make_colour(18, 9, norm="luma", src_peak=pk, tone="none")) == uns, pk
    assert rc(E.make_colour(18, 9, norm="luma", src_peak=400.0)) == 0 and rc(E.make_colour(18, 9, norm="luma", src_peak=10000.0)) == 0
    assert rc(E.make_colour(16, 9, src_peak=100.0, dst_peak=100.0)) == uns
    assert rc(E.make_colour(16, 9, src_peak=100.0, dst_peak=400.0)) == uns
    assert rc(E.make_colour(16, 9, src_peak=100.0, dst_peak=400.0, tone="none")) == 0
    assert rc(E.make_colour(16, 9, src_peak=10000.0, dst_peak=10.0)) == uns             # the knee of the tone curve below black
    assert rc(E.make_colour(16, 9, dst_peak=1e-30, tone="none")) == uns                 # an output table beyond int32
    for b in bufs:
        b[...] = 77
    assert rc(E.make_colour(16, 7)) == uns and all(np.all(b == 77) for b in bufs), "a refused call wrote its tables"
    assert rc(ok) == 0
    with pytest.raises(ValueError):
        E.make_colour(16, 9, out="rec709")
    with pytest.raises(E.EngineError) as ei:
        E.colour_tables(E.make_colour(18, 9))
    assert ei.value.code == uns
