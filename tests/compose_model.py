"""numpy model of oh_pics_compose, int64 throughout and literal: the fill, then the layers one after the other, each
over the whole result of the ones before it.

A layer is a dict: "src", the source's coded planes (a list of 2-D arrays); "rect" = (sx, sy, w, h) in luma samples, None for the
whole source; "at" = (dx, dy); "opacity" 0 .. 256; "alpha", None or an (h, w) array of 0 .. 255 over the rectangle's luma samples."""
import numpy as np

ONE = 65280                                                                 # 255 * 256: the weight of an opaque sample


def shifts(cf, c):
    """(hshift, vshift) of plane c"""
    return (1 if c and cf in (1, 2) else 0, 1 if c and cf == 1 else 0)


def blend(dst, src, alpha, opacity):
    """(src w + dst (65280 - w) + 32640) // 65280 with w = alpha * opacity"""
    dst, src, w = np.asarray(dst, np.int64), np.asarray(src, np.int64), np.asarray(alpha, np.int64) * np.asarray(opacity, np.int64)
    return (src * w + dst * (ONE - w) + ONE // 2) // ONE


def chroma_alpha(cf, a00, a01, a10, a11):
    """the alpha of a chroma sample from the luma alphas a00 a01 (upper row) and a10 a11 (lower row) it covers"""
    a00, a01, a10, a11 = (np.asarray(a, np.int64) for a in (a00, a01, a10, a11))
    if cf == 1:
        return (a00 + a01 + a10 + a11 + 2) >> 2
    if cf == 2:
        return (a00 + a01 + 1) >> 1
    return a00


def plane_alpha(cf, c, alpha):
    """the alpha plane of plane c of a rectangle from its luma alpha plane"""
    a = np.asarray(alpha, np.int64)
    hs, vs = shifts(cf, c)
    if hs and vs:
        return chroma_alpha(1, a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2])
    if hs:
        return chroma_alpha(2, a[:, 0::2], a[:, 1::2], 0, 0)
    return a


def compose(dst_planes, params, layers, fill=None):
    """the coded planes of one destination after the call; dst_planes are not modified"""
    cf = params.chroma_format_idc
    out = []
    for c, d in enumerate(dst_planes):
        d = np.asarray(d).astype(np.int64)
        out.append(np.full_like(d, int(fill[c])) if fill is not None else d.copy())
    for l in layers:
        src = l["src"]
        rect = l.get("rect")
        if rect is None:
            rect = (0, 0, src[0].shape[1], src[0].shape[0])
        sx, sy, w, h = rect
        dx, dy = l.get("at", (0, 0))
        opacity, alpha = l.get("opacity", 256), l.get("alpha")
        for c in range(len(out)):
            hs, vs = shifts(cf, c)
            assert not (sx % (1 << hs) or w % (1 << hs) or dx % (1 << hs) or sy % (1 << vs) or h % (1 << vs) or dy % (1 << vs))
            px, py, pw, ph, qx, qy = sx >> hs, sy >> vs, w >> hs, h >> vs, dx >> hs, dy >> vs
            H, W = out[c].shape
            x0, x1, y0, y1 = max(qx, 0), min(qx + pw, W), max(qy, 0), min(qy + ph, H)     # the clip, destination plane samples
            if x0 >= x1 or y0 >= y1:
                continue
            s = np.asarray(src[c]).astype(np.int64)[py + y0 - qy:py + y1 - qy, px + x0 - qx:px + x1 - qx]
            if alpha is None:
                a = np.full((y1 - y0, x1 - x0), 255, np.int64)
            else:
                assert np.asarray(alpha).shape == (h, w)
                a = plane_alpha(cf, c, alpha)[y0 - qy:y1 - qy, x0 - qx:x1 - qx]
            out[c][y0:y1, x0:x1] = blend(out[c][y0:y1, x0:x1], s, a, opacity)
    return out
