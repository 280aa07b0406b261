"""numpy model of oh_pics_light_level (include/ohevc_hip.h), bit for bit.

Stage 0 (chroma placement, the H.273 matrix to 16 bit) is convert_model.rgb_int, stage 1 colour_model.src_curve; the table A and the
luminance weights come from oh_colour_tables through ctypes (host only, no GPU), so the model and the kernel share the integers.
The norm, the bins and the statistics are written out here."""
import numpy as np

import colour_model as M
import convert_model as CM
from openhevc_amd import engine as E

FS = 1 << 30
NBINS = 258
HLG = 18


def light_colour(in_transfer, in_primaries, src_peak):
    """the OhColour whose A and misc[9..11] the light-level pass uses.  Neither depends on src_peak; the engine builds HLG with 1000
    nits so that peaks outside what oh_pics_convert_colour takes for HLG are no obstacle"""
    pk = 1000.0 if in_transfer == HLG else float(src_peak)
    return E.make_colour(in_transfer, in_primaries, out="linear", out_primaries=in_primaries, tone="none", norm="luma", src_peak=pk,
                         dst_peak=100.0, white=pk)


_tables = {}


def tables(in_transfer, in_primaries=9, src_peak=1000.0):
    """(A, [wR, wG, wB]), computed once per combination"""
    key = (int(in_transfer), int(in_primaries), 1000.0 if in_transfer == HLG else float(src_peak))
    if key not in _tables:
        A, _, _, misc = E.colour_tables(light_colour(*key))
        _tables[key] = (A, [int(x) for x in misc[9:12]])
    return _tables[key]


def bin_of(v):
    """bin(v): 0 below 2^14; 1 + 16 (e - 14) + ((v >> (e - 4)) & 15) with e = floor(log2 v) above"""
    v = np.minimum(np.asarray(v, np.int64), FS)
    e = np.frexp(np.maximum(v, 1).astype(np.float64))[1] - 1                # exact below 2^53
    return np.where(v < (1 << 14), 0, 1 + 16 * (e - 14) + ((v >> np.maximum(e - 4, 0)) & 15))


def bin_upper(b):
    """the largest v of a bin"""
    if b == 0:
        return (1 << 14) - 1
    e, j = 14 + (b - 1) // 16, (b - 1) % 16
    return min(((17 + j) << (e - 4)) - 1, FS)


def norm_values(planes, params, in_transfer, in_primaries=9, norm="maxrgb", src_peak=1000.0, window=(0, 0, 0, 0), matrix=9,
                full_range=False, chroma="linear"):
    """(H, W) norms v of the window's pixels"""
    A, w = tables(in_transfer, in_primaries, src_peak)
    rgb, D = CM.rgb_int(planes, params.bit_depth, params.chroma_format_idc, E.CONV_U16, window, matrix, full_range, chroma)
    assert D == 16
    l = M.src_curve(A, rgb)
    if norm == "luma":
        return (w[0] * l[..., 0] + w[1] * l[..., 1] + w[2] * l[..., 2] + (1 << 13)) >> 14
    return l.max(axis=-1)


def stats(v):
    """the fields of OhLightLevel for the norms v"""
    v = np.asarray(v, np.int64)
    return dict(pixels=int(v.size), sum=int(v.sum()), max=int(v.max()), min=int(v.min()),
                hist=np.bincount(bin_of(v).ravel(), minlength=NBINS).astype(np.uint32))


def light_level(planes, params, in_transfer, **kw):
    """one picture as Engine.pics_light_level returns it per picture, as a dict"""
    return stats(norm_values(planes, params, in_transfer, **kw))


def percentile(lls, ppm):
    """oh_light_percentile over dicts of stats()"""
    total = sum(ll["pixels"] for ll in lls)
    hist = sum(ll["hist"].astype(np.int64) for ll in lls)
    cum = np.cumsum(hist)
    b = int(np.argmax(cum * 1000000 >= ppm * total))
    return min(bin_upper(b), max(ll["max"] for ll in lls))
