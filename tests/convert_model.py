"""numpy model of oh_pics_convert (include/ohevc_hip.h): finished pictures -> YUV / RGB images, bit for bit.

The integers of the RGB matrix come from oh_convert_coeffs through ctypes (host only, no GPU), so the model and the kernel share them;
tests/test_convert_host.py checks those integers against the H.273 matrices.  Input: the picture's coded planes (2-D integer arrays,
e.g. HostPic.visible(c)); output: the image of ONE picture in the shape Engine.pics_convert gives per picture."""
import numpy as np

from openhevc_amd import engine as E

K_F32 = np.float32(1) / np.float32(65535)                    # the f32 nearest to 1 / 65535
KR_KB = {1: (0.2126, 0.0722), 5: (0.299, 0.114), 6: (0.299, 0.114), 9: (0.2627, 0.0593)}


def shifts(cf):
    return (1 if cf in (1, 2) else 0), (1 if cf == 1 else 0)


def crop(planes, cf, window):
    left, right, top, bottom = window
    hs, vs = shifts(cf)
    out = []
    for c, pl in enumerate(planes[:3 if cf else 1]):
        h, w = pl.shape
        sh, sv = (hs, vs) if c else (0, 0)
        out.append(pl[top >> sv:h - (bottom >> sv), left >> sh:w - (right >> sh)])
    return out


def yuv_image(planes, bd, cf, fmt, sample, window=(0, 0, 0, 0)):
    """PLANAR / SEMIPLANAR as a flat array of output samples"""
    p = [np.asarray(a).astype(np.int64) for a in crop(planes, cf, window)]
    semi = E.conv_format(fmt) == E.CONV_FORMATS["semiplanar"]
    if sample == E.CONV_U8 and bd > 8:
        p = [np.minimum((a + (1 << (bd - 9))) >> (bd - 8), 255) for a in p]
        dt = np.uint8
    elif sample in (E.CONV_U8, E.CONV_NATIVE):
        dt = np.uint8 if bd == 8 else np.uint16
        if semi and bd > 8:
            p = [a << (16 - bd) for a in p]
    else:
        raise ValueError("YUV formats take NATIVE or U8")
    if semi:
        cbcr = np.stack([p[1], p[2]], axis=-1)
        parts = [p[0].ravel(), cbcr.ravel()]
    else:
        parts = [a.ravel() for a in p]
    return np.concatenate(parts).astype(dt)


def _hfilter(C, rows, x):
    """h(j, x) for every luma row's chroma row j (rows) and luma column x: 2x scale"""
    wc = C.shape[1]
    Cr = C[rows]
    even = 2 * Cr[:, x >> 1]
    odd = Cr[:, np.maximum(x - 1, 0) >> 1] + Cr[:, np.minimum((x + 1) >> 1, wc - 1)]
    return np.where((x & 1)[None, :] == 1, odd, even)


def upsample(C, cf, linear, W, H, bd):
    """a coded chroma plane onto the coded luma grid (W x H); 4:0:0: the mid level"""
    if cf == 0:
        return np.full((H, W), 1 << (bd - 1), np.int64)
    C = np.asarray(C).astype(np.int64)
    if cf == 3:
        return C
    hs, vs = shifts(cf)
    x, y = np.arange(W), np.arange(H)
    if not linear:
        return C[(y >> vs)[:, None], (x >> hs)[None, :]]
    if cf == 2:
        return (_hfilter(C, y, x) + 1) >> 1
    hc = C.shape[0]
    j0 = y >> 1
    j1 = np.clip(j0 - 1 + 2 * (y & 1), 0, hc - 1)
    return (3 * _hfilter(C, j0, x) + _hfilter(C, j1, x) + 4) >> 3


def rgb_int(planes, bd, cf, sample, window=(0, 0, 0, 0), matrix=1, full_range=False, chroma="linear"):
    """(H, W, 3) integer R, G, B of D bits, and D"""
    cv = E.make_convert("rgb", sample, window, matrix, full_range, chroma)
    cy, crv, cgu, cgv, cbu, yoff, mid, S, D = E.convert_coeffs(cv, bd)
    Y = np.asarray(planes[0]).astype(np.int64)
    H, W = Y.shape
    lin = chroma == "linear"
    U = upsample(planes[1] if cf else None, cf, lin, W, H, bd)
    V = upsample(planes[2] if cf else None, cf, lin, W, H, bd)
    Y, U, V = [a[window[2]:H - window[3], window[0]:W - window[1]] for a in (Y, U, V)]
    dy = cy * (Y - yoff) + (1 << (S - 1))
    du, dv = U - mid, V - mid
    mx = (1 << D) - 1
    R = np.clip((dy + crv * dv) >> S, 0, mx)
    G = np.clip((dy + cgu * du + cgv * dv) >> S, 0, mx)
    B = np.clip((dy + cbu * du) >> S, 0, mx)
    return np.stack([R, G, B], axis=-1), D


def out_samples(v, sample):
    v = np.asarray(v)
    if sample == E.CONV_U8:
        return v.astype(np.uint8)
    if sample == E.CONV_U16:
        return v.astype(np.uint16)
    f = v.astype(np.float32) * K_F32                          # one f32 multiply
    return f if sample == E.CONV_F32 else f.astype(np.float16)


def rgb_image(planes, bd, cf, fmt, sample, window=(0, 0, 0, 0), matrix=1, full_range=False, chroma="linear"):
    """RGB_PLANAR (3, H, W), RGB (H, W, 3), RGBA (H, W, 4)"""
    rgb, D = rgb_int(planes, bd, cf, sample, window, matrix, full_range, chroma)
    f = E.conv_format(fmt)
    if f == E.CONV_FORMATS["rgb_planar"]:
        return out_samples(np.moveaxis(rgb, -1, 0), sample)
    if f == E.CONV_FORMATS["rgba"]:
        rgb = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), (1 << D) - 1, np.int64)], axis=-1)
    return out_samples(rgb, sample)


def convert(planes, params, fmt, sample, window=(0, 0, 0, 0), matrix=1, full_range=False, chroma="linear"):
    """one picture as Engine.pics_convert returns it per picture (YUV: (rows, W))"""
    bd, cf = params.bit_depth, params.chroma_format_idc
    W = params.width - window[0] - window[1]
    if E.conv_format(fmt) <= E.CONV_FORMATS["semiplanar"]:
        return yuv_image(planes, bd, cf, fmt, sample, window).reshape(-1, W)
    return rgb_image(planes, bd, cf, fmt, sample, window, matrix, full_range, chroma)


def float_rgb(Y, U, V, bd, matrix, full_range, D):
    """float64 evaluation of the H.273 equations for the integer samples Y and up-sampled U, V: R, G, B scaled to D bits, unrounded"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    if full_range:
        yoff, ys, cs = 0.0, (1 << bd) - 1.0, (1 << bd) - 1.0
    else:
        u = float(1 << (bd - 8))
        yoff, ys, cs = 16 * u, 219 * u, 224 * u
    mid = float(1 << (bd - 1))
    yn = (np.asarray(Y, np.float64) - yoff) / ys
    un = (np.asarray(U, np.float64) - mid) / cs
    vn = (np.asarray(V, np.float64) - mid) / cs
    r = yn + 2 * (1 - kr) * vn
    b = yn + 2 * (1 - kb) * un
    g = yn - 2 * kb * (1 - kb) / kg * un - 2 * kr * (1 - kr) / kg * vn
    mx = (1 << D) - 1
    return [np.clip(c * mx, 0, mx) for c in (r, g, b)]
