"""oh_import_coeffs and the integer definition of oh_pics_import on the host, no GPU: the coefficients against an
independent float64 computation and the int32 rule that fixes their shift, the integer model of tests/import_model.py against the
float64 H.273 equations within a bound derived per case, the exact round trip of in-gamut samples through convert_model, the float
sample types, and the chroma siting."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import convert_model as CM                                                  # noqa: E402
import import_model as IM                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

DEPTHS = (8, 9, 10, 12)
SAMPLE_OF_D = {8: E.CONV_U8, 16: E.CONV_U16}


def coeffs(bd, D, matrix, fr):
    return E.import_coeffs(E.make_convert("rgb", SAMPLE_OF_D[D], (0, 0, 0, 0), matrix, fr), bd)


CASES = list(itertools.product(DEPTHS, (8, 16), (1, 5, 6, 9), (False, True)))


@pytest.mark.parametrize("bd,D,matrix,fr", CASES)
def test_coefficients(bd, D, matrix, fr):
    k = coeffs(bd, D, matrix, fr)
    ry, gy, by, ru, gu, bu, rv, gv, bv, yoff, mid, S, Dk = k
    y0, ys, cs, m0 = IM.scales(bd, fr)
    assert (yoff, mid, Dk) == (y0, m0, D)
    # independent float64: every directly rounded coefficient within 1/2, the derived ones within the roundings they absorb
    ex = [c * 2.0 ** S for c in IM.float_coeffs(bd, D, matrix, fr)]
    tol = [0.5, 1.5, 0.5, 0.5, 1.0, 0.5, 0.5, 1.0, 0.5]
    for i in range(9):
        assert abs(k[i] - ex[i]) <= tol[i] + 1e-6, (i, k[i], ex[i])
    assert k == IM.coeffs_at(bd, D, matrix, fr, S)
    # the sum identities: greys give exactly mid, white exactly peak luma, black the luma offset
    assert gu == -ru - bu and gv == -rv - bv and bu == rv
    M = (1 << D) - 1
    assert ((ry + gy + by) * M + (yoff << S) + (1 << (S - 1))) >> S == yoff + ys
    assert ((yoff << S) + (1 << (S - 1))) >> S == yoff
    for g in (0, 1, M // 2, M):
        assert ((ru + gu + bu) * g + (mid << S) + (1 << (S - 1))) >> S == mid
        assert ((rv + gv + bv) * g + (mid << S) + (1 << (S - 1))) >> S == mid
    # S: the largest shift the int32 rule allows
    assert IM.shift_bound_ok(k, D)
    assert not IM.shift_bound_ok(IM.coeffs_at(bd, D, matrix, fr, S + 1), D)
    if D == 16 and bd in (10, 12):
        assert S == (20 if bd == 10 else 18)


def test_coefficient_argument_rules():
    out_of = lambda **kw: E.make_convert(kw.get("fmt", "rgb"), kw.get("sample", E.CONV_U8), (0, 0, 0, 0), kw.get("matrix", 1))  # noqa: E731
    for cv, bd, code in ((out_of(matrix=4), 10, E.OH_E_UNSUPPORTED), (out_of(fmt="planar"), 10, E.OH_E_UNSUPPORTED),
                         (out_of(sample=E.CONV_NATIVE), 10, E.OH_E_UNSUPPORTED), (out_of(), 11, E.OH_E_ARG)):
        with pytest.raises(E.EngineError) as ei:
            E.import_coeffs(cv, bd)
        assert ei.value.code == code


def quantisation(k, bd, D, matrix, fr):
    """per row: sum |c_i - exact_i| M / 2^S, the most the rounded coefficients move a result"""
    S, M = k[11], (1 << D) - 1
    ex = [c * 2.0 ** S for c in IM.float_coeffs(bd, D, matrix, fr)]
    return [sum(abs(k[3 * r + i] - ex[3 * r + i]) for i in range(3)) * M / 2.0 ** S for r in range(3)]


@pytest.mark.parametrize("bd,D,matrix,fr", CASES)
def test_integer_model_against_float64(bd, D, matrix, fr):
    """The bound: the final floor((v + 1/2)) rounds by at most 1/2; the rounded coefficients move the sum by at most
    sum |c_i - exact_i| R_i / 2^S <= sum |c_i - exact_i| M / 2^S; the clip is 1-Lipschitz and applied to both sides.  Filtered chroma
    adds the rounding of Rf, Gf, Bf to D bits: at most 1/2 each, times |c_i| / 2^S."""
    rng = np.random.default_rng(bd * 100 + D + matrix + fr)
    k = coeffs(bd, D, matrix, fr)
    S, M, mx = k[11], (1 << D) - 1, (1 << bd) - 1
    q = quantisation(k, bd, D, matrix, fr)
    rgb = rng.integers(0, M + 1, (64, 512, 3), dtype=np.int64)
    rgb[0, :8] = [[0, 0, 0], [M, M, M], [M, 0, 0], [0, M, 0], [0, 0, M], [M, M, 0], [0, M, M], [M, 0, M]]
    got = IM.matrix_rows(k, rgb, rgb, bd)
    want = IM.float_yuv(rgb, bd, D, matrix, fr)
    worst = []
    for r in range(3):
        err = np.max(np.abs(got[r] - np.clip(want[r], 0, mx)))
        assert err <= 0.5 + q[r] + 1e-9, (r, err, q[r])
        worst.append(err)
    # 4:2:0 and 4:2:2 with the linear filter: the float side filters the unrounded R, G, B
    for cf in (1, 2):
        f = 3 if cf == 1 else 2
        xc, W = np.arange(256), 512
        xl, xm, xr = np.clip(2 * xc - 1, 0, W - 1), 2 * xc, np.clip(2 * xc + 1, 0, W - 1)
        h = (rgb[:, xl] + 2 * rgb[:, xm] + rgb[:, xr]).astype(np.float64)
        ff = (h[0::2] + h[1::2]) / 8.0 if cf == 1 else h / 4.0
        gotc = IM.matrix_rows(k, rgb, IM.filtered(rgb, cf, True), bd)[1:]
        wantc = IM.float_yuv(ff, bd, D, matrix, fr)[1:]
        for r in (1, 2):
            extra = sum(abs(c) for c in k[3 * r:3 * r + 3]) / 2.0 ** (S + 1)
            err = np.max(np.abs(gotc[r - 1] - np.clip(wantc[r - 1], 0, mx)))
            assert err <= 0.5 + q[r] + extra + 1e-9, (cf, r, err, q[r], extra, f)
            worst.append(err)
    print(f"B={bd} D={D} matrix={matrix} full={int(fr)} S={S}: max |int - float64| Y {worst[0]:.4f} Cb {worst[1]:.4f} Cr {worst[2]:.4f}, "
          f"filtered chroma {max(worst[3:]):.4f} LSB (quantisation {max(q):.5f})")
    if D == 8:
        assert max(worst[:3]) < 0.51


@pytest.mark.parametrize("bd,matrix,fr", list(itertools.product(DEPTHS, (1, 5, 9), (False, True))))
def test_round_trip_of_in_gamut_samples(bd, matrix, fr):
    """(Y, Cb, Cr) -> float64 R'G'B' at 16 bit, rounded -> import: exactly the triple, wherever the RGB was not clipped.  The same
    triples through the integer convert_model.rgb_int (U16): within 1; the count of differences is printed (a recorded figure)."""
    rng = np.random.default_rng(bd * 10 + matrix + fr)
    n, mx, M = 600_000, (1 << bd) - 1, 65535
    Y, U, V = [rng.integers(0, mx + 1, n, dtype=np.int64) for _ in range(3)]
    rgb = np.stack(CM.float_rgb(Y, U, V, bd, matrix, fr, 16), axis=-1)
    keep = np.all((rgb > 0) & (rgb < M), axis=-1)
    assert keep.sum() > 50_000
    Y, U, V, rgb = Y[keep], U[keep], V[keep], rgb[keep]
    k = coeffs(bd, 16, matrix, fr)
    back = IM.matrix_rows(k, np.rint(rgb).astype(np.int64), np.rint(rgb).astype(np.int64), bd)
    for name, a, b in zip("Y Cb Cr".split(), (Y, U, V), back):
        assert np.array_equal(a, b), (name, int(np.sum(a != b)))
    ri, D = CM.rgb_int([Y[None, :], U[None, :], V[None, :]], bd, 3, E.CONV_U16, matrix=matrix, full_range=fr)
    assert D == 16
    back_i = IM.matrix_rows(k, ri[0], ri[0], bd)
    diffs = 0
    for a, b in zip((Y, U, V), back_i):
        assert np.max(np.abs(a - b)) <= 1
        diffs += int(np.sum(a != b))
    print(f"B={bd} matrix={matrix} full={int(fr)}: {int(keep.sum())} in-gamut triples, exact through float64; "
          f"{diffs} samples differ (by 1) through the integer convert model")


def test_float_samples_map_back():
    v = np.arange(65536, dtype=np.int64)
    f32 = CM.out_samples(v, E.CONV_F32)
    got, D = IM.rgb_ints(np.stack([f32] * 3, -1)[None], "rgb", E.CONV_F32)
    assert D == 16 and np.array_equal(got[0, :, 0], v) and np.array_equal(got[0, :, 2], v)
    f16 = CM.out_samples(v, E.CONV_F16)
    got16, _ = IM.rgb_ints(np.stack([f16] * 3, -1)[None], "rgb", E.CONV_F16)
    err = np.abs(got16[0, :, 1] - v)
    assert err.max() <= 16
    print(f"F16 round trip: max error {int(err.max())} of 65535")
    odd = np.array([[[-1.0, np.nan, 2.0], [np.inf, -np.inf, 1.0], [0.0, 0.5, 1.0000001]]], np.float32)
    got, _ = IM.rgb_ints(odd, "rgb", E.CONV_F32)
    assert got.tolist() == [[[0, 0, 65535], [65535, 0, 65535], [0, 32768, 65535]]]
    u16, D = IM.rgb_ints(np.array([[[0, 1, 65535]]], np.uint16), "rgb", E.CONV_U16)
    assert D == 16 and u16.tolist() == [[[0, 1, 65535]]]
    # planar and rgba layouts address the same samples
    a = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    assert np.array_equal(IM.rgb_ints(a, "rgba", E.CONV_U8)[0], a[..., :3])
    assert np.array_equal(IM.rgb_ints(np.moveaxis(a[..., :3], -1, 0), "rgb_planar", E.CONV_U8)[0], a[..., :3])


@pytest.mark.parametrize("bd", (8, 10))
def test_chroma_siting_of_a_ramp(bd):
    """4:2:0 linear import then convert's linear up-sampling gives back the chroma of the ramp itself (its 4:4:4 import) within 1 LSB
    away from the edges: both sides use chroma_sample_loc_type 0.  A siting half a pixel off would miss by several LSB at this slope."""
    from openhevc_amd import frame as F
    W, H = 64, 16
    x = np.arange(W, dtype=np.int64)
    img = np.zeros((H, W, 3), np.uint16)
    img[..., 0] = (x * 1024)[None, :]
    img[..., 1] = 30000
    img[..., 2] = ((W - 1 - x) * 1024)[None, :]
    p1, p3 = F.pic_params(W, H, bit_depth=bd, chroma_format_idc=1), F.pic_params(W, H, bit_depth=bd, chroma_format_idc=3)
    sub = IM.import_picture(img, p1, "rgb", E.CONV_U16, chroma="linear")
    ref = IM.import_picture(img, p3, "rgb", E.CONV_U16)
    assert np.array_equal(sub[0], ref[0])                                    # luma always uses the pixel itself
    slope = np.abs(np.diff(ref[2][0].astype(np.int64))).mean()
    assert slope > 1.5 * (1 << (bd - 8))                                     # steep enough to tell the sitings apart
    for c in (1, 2):
        up = CM.upsample(sub[c], 1, True, W, H, bd)
        d = np.abs(up[:, 2:W - 2] - ref[c][:, 2:W - 2].astype(np.int64))
        assert d.max() <= 1, (c, int(d.max()))
    # the point form takes pixel (2x, 2y)
    pt = IM.import_picture(img, p1, "rgb", E.CONV_U16, chroma="nearest")
    assert np.array_equal(pt[1], ref[1][0::2, 0::2]) and np.array_equal(pt[2], ref[2][0::2, 0::2])


def test_model_replicates_the_window_edges():
    from openhevc_amd import frame as F
    p = F.pic_params(24, 16, bit_depth=10, chroma_format_idc=1)
    win = (4, 2, 2, 6)
    W, H = 18, 8
    rng = np.random.default_rng(5)
    img = rng.integers(0, 1024, W * H * 3 // 2).astype(np.uint16)
    pl = IM.import_picture(img, p, "planar", E.CONV_NATIVE, win)
    assert [a.shape for a in pl] == [(16, 24), (8, 12), (8, 12)]
    y = img[:W * H].reshape(H, W)
    assert np.array_equal(pl[0][2:10, 4:22], y)
    assert np.all(pl[0][:2, 4:22] == y[0]) and np.all(pl[0][10:, 4:22] == y[-1])
    assert np.all(pl[0][2:10, :4] == y[:, :1]) and np.all(pl[0][2:10, 22:] == y[:, -1:])
    assert np.all(pl[0][:2, :4] == y[0, 0]) and np.all(pl[0][10:, 22:] == y[-1, -1])
    back = CM.convert(pl, p, "planar", E.CONV_NATIVE, win)
    assert np.array_equal(back.ravel(), img)
