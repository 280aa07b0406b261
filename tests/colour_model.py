"""numpy model of oh_pics_convert_colour (include/ohevc_hip.h), bit for bit, and the same stages in float64.

The integer model reads the tables and the misc integers of oh_colour_tables through ctypes (host only, no GPU), so the model and the
kernel share them; tests/test_colour_host.py checks those integers against the curves below and the model against float_pipeline.
Stage 0 (chroma placement, the H.273 matrix to 16 bit) is convert_model.rgb_int."""
import numpy as np

import convert_model as CM
from openhevc_amd import engine as E

FS = 1 << 30                                                  # full scale of linear light
PQ, HLG, SRGB = 16, 18, 13
SDR_VIDEO = (1, 6, 14, 15)
PRIMARIES = {1: ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)),          # BT.709
             9: ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)),          # BT.2020
             12: ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))}         # P3-D65
D65 = (0.3127, 0.3290)


# ---------------------------------------------------------------- the integer model ----------------------------------------------------------------
def nodes():
    """the node of every entry of a piecewise-logarithmic table (G, B), in units of 2^-30 of the full scale"""
    k = np.arange(E.COL_NP, dtype=np.int64)
    return np.where(k < 128, k, (64 + (k & 63)) << np.maximum((k >> 6) - 1, 0))


def src_curve(A, v):
    """stage 1: 16-bit codes through A"""
    A = np.asarray(A, np.int64)
    v = np.asarray(v, np.int64)
    i, f = v >> 4, v & 15
    return np.minimum(A[i] + (((A[i + 1] - A[i]) * f + 8) >> 4), FS)


def lut(T, l):
    """P(T, l) for 0 <= l <= 2^30"""
    T = np.asarray(T, np.int64)
    l = np.asarray(l, np.int64)
    e = np.frexp(np.maximum(l, 1).astype(np.float64))[1] - 1                # floor(log2 l), exact below 2^53
    s = np.maximum(e - 6, 0)
    k = (s << 6) + (l >> s)                                                 # l below 128: s = 0, k = l
    fr = l & ((1 << s) - 1)
    f12 = np.where(s <= 12, fr << np.maximum(12 - s, 0), fr >> np.maximum(s - 12, 0))
    return np.where(l < 128, T[np.minimum(l, 127)], T[k] + (((T[k + 1] - T[k]) * f12 + 2048) >> 12))


def stages(rgb16, col, tables=None):
    """(..., 3) integer R'G'B' of 16 bit -> (by_table, values): the 16-bit output codes, or linear light with 2^30 = full scale"""
    A, G, B, misc = tables if tables is not None else E.colour_tables(col)
    misc = [int(x) for x in misc]
    l = src_curve(A, rgb16)
    if misc[15]:
        if misc[12] == E.COL_NORM["luma"]:
            nrm = (misc[9] * l[..., 0] + misc[10] * l[..., 1] + misc[11] * l[..., 2] + (1 << 13)) >> 14
        else:
            nrm = l.max(axis=-1)
        g = lut(G, nrm)[..., None]
        l = (l * g + (1 << 19)) >> 20
    if misc[16]:
        M = np.array(misc[:9], np.int64).reshape(3, 3)
        l = np.clip(((l[..., None, :] * M).sum(axis=-1) + (1 << 19)) >> 20, 0, FS)
    if not misc[13]:
        return False, l
    return True, np.clip(lut(B, l), 0, 65535)


def k_linear(col, tables=None):
    misc = (tables if tables is not None else E.colour_tables(col))[3]
    return np.array([misc[14]], np.int32).view(np.float32)[0]


def out_samples(by_table, v, sample, K):
    """the values of stages() as output samples"""
    if by_table:
        if sample == E.CONV_U8:
            return ((v + 128) // 257).astype(np.uint8)
        return CM.out_samples(v, sample)
    if sample not in (E.CONV_F16, E.CONV_F32):
        raise ValueError("linear light takes float16 or float32")
    f = v.astype(np.float32) * np.float32(K)                  # one conversion, one f32 multiply
    if sample == E.CONV_F32:
        return f
    return np.where(f >= np.float32(65520), np.float32(65504), f).astype(np.float16)


def convert(planes, params, fmt, sample, col, window=(0, 0, 0, 0), matrix=1, full_range=False, chroma="linear", tables=None):
    """one picture as Engine.pics_convert(..., colour=col) returns it per picture: RGB_PLANAR (3, H, W), RGB (H, W, 3), RGBA (H, W, 4)"""
    tables = tables if tables is not None else E.colour_tables(col)
    rgb, D = CM.rgb_int(planes, params.bit_depth, params.chroma_format_idc, E.CONV_U16, window, matrix, full_range, chroma)
    assert D == 16
    by_table, v = stages(rgb, col, tables)
    K = k_linear(col, tables)
    out = out_samples(by_table, v, sample, K)
    f = E.conv_format(fmt)
    if f == E.CONV_FORMATS["rgb_planar"]:
        return np.ascontiguousarray(np.moveaxis(out, -1, 0))
    if f == E.CONV_FORMATS["rgba"]:
        if by_table:
            alpha = out_samples(True, np.full(out.shape[:2] + (1,), 65535, np.int64), sample, K)
        else:
            alpha = np.ones(out.shape[:2] + (1,), out.dtype)
        out = np.concatenate([out, alpha], axis=-1)
    return out


# ---------------------------------------------------------------- the curves in float64 ----------------------------------------------------------------
PQ_M1, PQ_M2 = 2610 / 16384, 2523 / 4096 * 128
PQ_C1, PQ_C2, PQ_C3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32


def pq_eotf(x):
    """ST 2084: signal -> luminance / 10000"""
    xp = np.power(np.maximum(np.asarray(x, np.float64), 0), 1 / PQ_M2)
    return np.power(np.maximum(xp - PQ_C1, 0) / (PQ_C2 - PQ_C3 * xp), 1 / PQ_M1)


def pq_inv(y):
    yp = np.power(np.maximum(np.asarray(y, np.float64), 0), PQ_M1)
    return np.power((PQ_C1 + PQ_C2 * yp) / (1 + PQ_C3 * yp), PQ_M2)


def hlg_inv_oetf(x):
    """BT.2100: signal -> scene linear, 1 at signal 1"""
    a = 0.17883277
    b, c = 1 - 4 * a, 0.5 - a * np.log(4 * a)
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.5, x * x / 3, (np.exp((x - c) / a) + b) / 12)


def srgb_eotf(x):
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.04045, x / 12.92, np.power((np.maximum(x, 0) + 0.055) / 1.055, 2.4))


def srgb_inv(l):
    l = np.asarray(l, np.float64)
    return np.where(l <= 0.0031308, 12.92 * l, 1.055 * np.power(np.maximum(l, 0), 1 / 2.4) - 0.055)


def source_curve(in_transfer, x):
    """E: signal -> linear light over the full scale"""
    if in_transfer == PQ:
        return pq_eotf(x)
    if in_transfer == HLG:
        return hlg_inv_oetf(x)
    if in_transfer == SRGB:
        return srgb_eotf(x)
    return np.power(np.maximum(np.asarray(x, np.float64), 0), 2.4)


def full_scale(col):
    return 10000.0 if col.in_transfer == PQ else float(col.src_peak)


def eetf_gain(nits, src_peak, dst_peak):
    """TM(nits) / nits of the BT.2390 EETF with black 0: 1 below the knee, the target peak from the source peak on"""
    nits = np.asarray(nits, np.float64)
    src_pq = pq_inv(src_peak / 10000)
    mx = pq_inv(dst_peak / 10000) / src_pq
    ks = 1.5 * mx - 0.5
    safe = np.maximum(nits, 1e-300)
    e1 = np.minimum(pq_inv(safe / 10000) / src_pq, 1)
    t = np.clip((e1 - ks) / (1 - ks), 0, 1)
    e2 = (2 * t**3 - 3 * t**2 + 1) * ks + (t**3 - 2 * t**2 + t) * (1 - ks) + (-2 * t**3 + 3 * t**2) * mx
    return np.where((nits <= 0) | (e1 <= ks), 1.0, 10000 * pq_eotf(e2 * src_pq) / safe)


def gain(col, x):
    """the factor of stage 2 at the norm x (over the full scale)"""
    x = np.asarray(x, np.float64)
    hlg = col.in_transfer == HLG
    src, Lfs = float(col.src_peak), full_scale(col)
    g = np.ones_like(x)
    gamma = 1.2 + 0.42 * np.log10(src / 1000) if hlg else 1.0
    if hlg:
        g = np.where(x > 0, np.power(np.maximum(x, 1e-300), gamma - 1), 0.0)
    if col.tone == E.COL_TONE["bt2390"]:
        g = g * eetf_gain(src * np.power(x, gamma) if hlg else Lfs * x, src, float(col.dst_peak))
    return np.minimum(g, 1.0)


def output_curve(col, x):
    """the OETF of stage 4 at x (1 = dst_peak)"""
    if col.out_transfer == E.COL_OUT["srgb"]:
        return srgb_inv(x)
    return np.power(np.maximum(np.asarray(x, np.float64), 0), 1 / 2.4)


def rgb_to_xyz(prim):
    P = np.array([[x / y, 1.0, (1 - x - y) / y] for x, y in PRIMARIES[prim]], np.float64).T
    W = np.array([D65[0] / D65[1], 1.0, (1 - D65[0] - D65[1]) / D65[1]])
    return P * np.linalg.solve(P, W)[None, :]


def float_pipeline(rgb16, col):
    """(..., 3) R'G'B' codes of 16 bit through the same stages in float64, no tables, no intermediate rounding: (by_table, values) —
    the unrounded 16-bit output code in [0, 65535], or linear light over the full scale in [0, 1]"""
    Lfs = full_scale(col)
    l = source_curve(col.in_transfer, np.asarray(rgb16, np.float64) / 65535)
    if col.in_transfer == HLG or col.tone == E.COL_TONE["bt2390"]:
        if col.norm == E.COL_NORM["luma"]:
            nrm = l @ rgb_to_xyz(col.in_primaries)[1]
        else:
            nrm = l.max(axis=-1)
        l = l * gain(col, nrm)[..., None]
    if col.in_primaries != col.out_primaries:
        l = l @ np.linalg.solve(rgb_to_xyz(col.out_primaries), rgb_to_xyz(col.in_primaries)).T
    l = np.clip(l, 0, 1)
    if col.out_transfer == E.COL_OUT["linear"]:
        return False, l
    return True, np.clip(65535 * output_curve(col, l * Lfs / float(col.dst_peak)), 0, 65535)
