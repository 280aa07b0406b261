"""numpy model of oh_pics_import (include/ohevc_hip.h): YUV / RGB images -> the coded planes of a picture, bit for bit.

The integers of the RGB matrix come from oh_import_coeffs through ctypes (host only, no GPU), so the model and the kernel share them;
tests/test_import_host.py checks those integers against an independent float64 computation (float_coeffs) and the whole integer path
against the float64 H.273 equations (float_yuv).  Input: the image of ONE picture in the shape Engine.pics_convert gives per picture;
output: the coded planes (2-D integer arrays), the replicated margins around the window included."""
import numpy as np

from openhevc_amd import engine as E

import convert_model as CM

KR_KB = CM.KR_KB
shifts = CM.shifts


def plane_geometry(w, h, cf, window):
    """per plane: (coded width, coded height, x0, y0, window width, window height)"""
    left, right, top, bottom = window
    hs, vs = shifts(cf)
    W, H = w - left - right, h - top - bottom
    out = [(w, h, left, top, W, H)]
    if cf:
        out += [(w >> hs, h >> vs, left >> hs, top >> vs, W >> hs, H >> vs)] * 2
    return out


def replicate(win_planes, w, h, cf, window):
    """step 3: plane c's sample at coded (X, Y) is the window sample at the clamped position"""
    out = []
    for pl, (pw, ph, x0, y0, wc, hc) in zip(win_planes, plane_geometry(w, h, cf, window)):
        assert pl.shape == (hc, wc), (pl.shape, hc, wc)
        ys = np.clip(np.arange(ph) - y0, 0, hc - 1)
        xs = np.clip(np.arange(pw) - x0, 0, wc - 1)
        out.append(pl[ys[:, None], xs[None, :]])
    return out


def yuv_window_planes(image, bd, cf, fmt, sample, W, H):
    """step 1: a PLANAR / SEMIPLANAR image (any shape, W x H luma samples) -> the window's planes as stored samples"""
    v = np.asarray(image).ravel().astype(np.int64)
    hs, vs = shifts(cf)
    wc, hc = W >> hs, H >> vs
    semi = E.conv_format(fmt) == E.CONV_FORMATS["semiplanar"]
    planes = [v[:W * H].reshape(H, W)]
    if cf:
        rest = v[W * H:W * H + 2 * wc * hc]
        if semi:
            rest = rest.reshape(hc, wc, 2)
            planes += [rest[..., 0], rest[..., 1]]
        else:
            planes += [rest[:wc * hc].reshape(hc, wc), rest[wc * hc:].reshape(hc, wc)]
    elif semi:
        raise ValueError("a 4:0:0 picture has no semi-planar form")
    if bd == 8:
        return planes
    if sample == E.CONV_U8:
        return [p << (bd - 8) for p in planes]
    if sample != E.CONV_NATIVE:
        raise ValueError("YUV formats take NATIVE or U8")
    if semi:
        return [p >> (16 - bd) for p in planes]
    return [np.minimum(p, (1 << bd) - 1) for p in planes]


def rgb_ints(image, fmt, sample):
    """step 2, first half: an RGB image -> (H, W, 3) int64 of D bits, and D.  image: (3, H, W), (H, W, 3) or (H, W, 4) of uint8,
    uint16, float16 or float32"""
    a = np.asarray(image)
    f = E.conv_format(fmt)
    if f == E.CONV_FORMATS["rgb_planar"]:
        a = np.moveaxis(a, 0, -1)
    a = a[..., :3]
    if sample == E.CONV_U8:
        return a.astype(np.int64), 8
    if sample == E.CONV_U16:
        return a.astype(np.int64), 16
    x = a.astype(np.float32)                                  # f16 -> f32 is exact
    with np.errstate(invalid="ignore", over="ignore"):
        q = x * np.float32(65535)                             # one f32 multiplication, nearest even
        q = np.where(np.isnan(q), np.float32(0), np.minimum(np.maximum(q, np.float32(0)), np.float32(65535)))
    return np.rint(q).astype(np.int64), 16


def filtered(rgb, cf, linear):
    """the R, G, B the chroma rows read: (hc, wc, 3) at the chroma sites, rounded back to D bits"""
    H, W, _ = rgb.shape
    hs, vs = shifts(cf)
    if cf == 3:
        return rgb
    xc, yc = np.arange(W >> hs), np.arange(H >> vs)
    if not linear:
        return rgb[(yc << vs)[:, None], (xc << hs)[None, :]]
    xl, xm, xr = np.clip(2 * xc - 1, 0, W - 1), 2 * xc, np.clip(2 * xc + 1, 0, W - 1)
    h = rgb[:, xl] + 2 * rgb[:, xm] + rgb[:, xr]
    if vs:
        return (h[2 * yc] + h[2 * yc + 1] + 4) >> 3
    return (h + 2) >> 2


def matrix_rows(k, rgb, rgbf, bd):
    """step 2, second half: the integer rows of oh_import_coeffs on (.., 3) luma pixels and (.., 3) chroma-site pixels (None: no chroma)"""
    ry, gy, by, ru, gu, bu, rv, gv, bv, yoff, mid, S, D = [int(v) for v in k]
    rnd, mx = 1 << (S - 1), (1 << bd) - 1
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    out = [np.clip((ry * R + gy * G + by * B + (yoff << S) + rnd) >> S, 0, mx)]
    if rgbf is not None:
        R, G, B = rgbf[..., 0], rgbf[..., 1], rgbf[..., 2]
        out.append(np.clip((ru * R + gu * G + bu * B + (mid << S) + rnd) >> S, 0, mx))
        out.append(np.clip((rv * R + gv * G + bv * B + (mid << S) + rnd) >> S, 0, mx))
    return out


def rgb_window_planes(image, bd, cf, fmt, sample, matrix=1, full_range=False, chroma="linear"):
    rgb, D = rgb_ints(image, fmt, sample)
    k = E.import_coeffs(E.make_convert("rgb", sample, (0, 0, 0, 0), matrix, full_range, chroma), bd)
    assert k[12] == D
    return matrix_rows(k, rgb, filtered(rgb, cf, chroma == "linear") if cf else None, bd)


def import_picture(image, params, fmt, sample, window=(0, 0, 0, 0), matrix=1, full_range=False, chroma="linear"):
    """one image as Engine.pics_convert shapes it -> the coded planes of the picture, as the stored sample type"""
    bd, cf, w, h = params.bit_depth, params.chroma_format_idc, params.width, params.height
    W, H = w - window[0] - window[1], h - window[2] - window[3]
    if E.conv_format(fmt) <= E.CONV_FORMATS["semiplanar"]:
        win = yuv_window_planes(image, bd, cf, fmt, sample, W, H)
    else:
        win = rgb_window_planes(image, bd, cf, fmt, sample, matrix, full_range, chroma)
    dt = np.uint8 if bd == 8 else np.uint16
    return [p.astype(dt) for p in replicate(win, w, h, cf, window)]


# ---- the float64 side: what the integers are checked against ----
def scales(bd, full_range):
    """(yoff, ys, cs, mid)"""
    if full_range:
        return 0, (1 << bd) - 1, (1 << bd) - 1, 1 << (bd - 1)
    u = 1 << (bd - 8)
    return 16 * u, 219 * u, 224 * u, 1 << (bd - 1)


def float_coeffs(bd, D, matrix, full_range):
    """the nine exact (unrounded, unscaled by 2^S) coefficients per unit of a D-bit RGB integer, float64: rows y, u, v"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    yoff, ys, cs, mid = scales(bd, full_range)
    M = float((1 << D) - 1)
    y = [ys * kr / M, ys * kg / M, ys * kb / M]
    u = [-cs * kr / (2 * (1 - kb) * M), -cs * kg / (2 * (1 - kb) * M), cs / (2 * M)]
    v = [cs / (2 * M), -cs * kg / (2 * (1 - kr) * M), -cs * kb / (2 * (1 - kr) * M)]
    return y + u + v


def float_yuv(rgb, bd, D, matrix, full_range):
    """float64 H.273 equations on (.., 3) RGB of D bits: unrounded, unclipped Y, Cb, Cr in units of the bd-bit samples"""
    c = float_coeffs(bd, D, matrix, full_range)
    yoff, ys, cs, mid = scales(bd, full_range)
    R, G, B = [np.asarray(rgb[..., i], np.float64) for i in range(3)]
    return (c[0] * R + c[1] * G + c[2] * B + yoff, c[3] * R + c[4] * G + c[5] * B + mid, c[6] * R + c[7] * G + c[8] * B + mid)


def shift_bound_ok(k, D):
    """the rule that fixes S, in Python integers: every row's (|c0| + |c1| + |c2|) (2^D - 1) + (offset << S) + 2^(S-1) fits int32"""
    S, M = int(k[11]), (1 << D) - 1
    offs = (int(k[9]), int(k[10]), int(k[10]))
    return all(sum(abs(int(c)) for c in k[3 * r:3 * r + 3]) * M + (offs[r] << S) + (1 << (S - 1)) <= 2 ** 31 - 1 for r in range(3))


def coeffs_at(bd, D, matrix, full_range, S):
    """the rounding rules of §3g at a given shift, in Python (round half away from zero, as llround)"""
    kr, kb = KR_KB[matrix]
    yoff, ys, cs, mid = scales(bd, full_range)
    M = float((1 << D) - 1)

    def rnd(x):
        return int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)
    two = float(1 << S)
    ry, by = rnd(two * ys * kr / M), rnd(two * ys * kb / M)
    gy = rnd(two * ys / M) - ry - by
    bu = rv = rnd(two * cs / (2 * M))
    ru = rnd(-two * cs * kr / (2 * (1 - kb) * M))
    bv = rnd(-two * cs * kb / (2 * (1 - kr) * M))
    return (ry, gy, by, ru, -ru - bu, bu, rv, -rv - bv, bv, yoff, mid, S, D)
