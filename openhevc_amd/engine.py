"""ctypes binding of libohevc_hip.so (include/ohevc_hip.h).  Plumbing only: no arithmetic here.

There is no CPU fallback: creating an Engine without the built library or without a GPU raises.
"""
import collections
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from . import frame as F
from .annexb import OhPictureHash

OH_N_PASSES = 6
PASS_NAMES = ("inter", "residual", "intra", "deblock_v", "deblock_h", "sao")

_lib = None
_torch_first = False


class EngineError(RuntimeError):
    code = None                                               # the OH_E_* code of the failed call, where one is known


def _check(rc, what, failed=None, text="{what} failed ({rc})"):
    """the return code of the library call `what`: where it failed (default: where it is not 0), EngineError(text) with .code set"""
    if rc != 0 if failed is None else failed:
        err = EngineError(text.format(what=what, rc=rc))
        err.code = rc
        raise err


def _enum(table, what, v, ints=None):
    """a name of table or its number -> the number.  ints None: any number passes as int(v); a range or a collection: the ints that
    do, which the ValueError of any other names as "lo .. hi" or as the sorted list"""
    if isinstance(v, str):
        if v not in table:
            raise ValueError(f"unknown {what} {v!r}: one of {sorted(table)}")
        return table[v]
    i = int(v)
    if ints is not None and i not in ints:
        raise ValueError(f"{what} {i}: {ints[0]} .. {ints[-1]}" if isinstance(ints, range) else f"{what} {v}: one of {sorted(ints)}")
    return i


def _ids(ids):
    """picture ids as a ctypes int array: as many entries as there are, one at least (the library takes no array without an address)"""
    return (C.c_int * max(len(ids), 1))(*ids)


class OhWindow(C.Structure):                                  # include/ohevc_hip.h
    _fields_ = [("left", C.c_int32), ("right", C.c_int32), ("top", C.c_int32), ("bottom", C.c_int32)]


OH_E_HIP, OH_E_ARG, OH_E_NOMEM, OH_E_UNSUPPORTED = -1, -2, -3, -4
CONV_FORMATS = {"planar": 0, "semiplanar": 1, "rgb_planar": 2, "rgb": 3, "rgba": 4}      # OH_CONV_PLANAR .. OH_CONV_RGBA
CONV_NATIVE, CONV_U8, CONV_U16, CONV_F16, CONV_F32 = range(5)                           # OH_CONV_NATIVE .. OH_CONV_F32
CONV_MAX_PICS, CONV_NCOEFFS = 64, 9
IMPORT_NCOEFFS = 13                                                                     # OH_IMPORT_NCOEFFS


class OhConvert(C.Structure):                                 # include/ohevc_hip.h
    _fields_ = [("format", C.c_int32), ("sample", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32),
                ("chroma_filter", C.c_int32), ("win", OhWindow)]


def conv_format(fmt):
    """a format name of CONV_FORMATS or its OH_CONV_* number -> the number"""
    return _enum(CONV_FORMATS, "format", fmt)


def make_convert(fmt, sample, window=(0, 0, 0, 0), matrix=1, full_range=False, chroma="linear"):
    """OhConvert for oh_pics_convert: window = (left, right, top, bottom) in luma samples, chroma "linear" or "nearest" """
    if chroma not in ("linear", "nearest"):
        raise ValueError(f"chroma must be 'linear' or 'nearest', not {chroma!r}")
    return OhConvert(conv_format(fmt), int(sample), int(matrix), int(bool(full_range)), 1 if chroma == "linear" else 0, OhWindow(*window))


class OhColour(C.Structure):                                  # include/ohevc_hip.h
    _fields_ = [("in_transfer", C.c_int32), ("in_primaries", C.c_int32), ("out_primaries", C.c_int32), ("out_transfer", C.c_int32),
                ("tone", C.c_int32), ("norm", C.c_int32), ("src_peak", C.c_float), ("dst_peak", C.c_float), ("white", C.c_float)]


COL_OUT = {"linear": 0, "srgb": 1, "gamma24": 2}                                        # OH_COL_LINEAR .. OH_COL_GAMMA24
COL_TONE = {"none": 0, "bt2390": 1}                                                     # OH_TONE_NONE, OH_TONE_BT2390
COL_NORM = {"maxrgb": 0, "luma": 1}                                                     # OH_NORM_MAXRGB, OH_NORM_LUMA
COL_NA, COL_NP, COL_NMISC = 4097, 1602, 20


def make_colour(in_transfer, in_primaries, out="srgb", out_primaries=1, tone="bt2390", norm="maxrgb", src_peak=1000.0, dst_peak=100.0,
                white=203.0):
    """OhColour for oh_pics_convert_colour: in_transfer / in_primaries / out_primaries are H.273 codes, out "srgb", "gamma24" or
    "linear", tone "bt2390" or "none", norm "maxrgb" or "luma" (HLG takes "luma"); the peaks and white in nits"""
    for name, v, d in (("out", out, COL_OUT), ("tone", tone, COL_TONE), ("norm", norm, COL_NORM)):
        if v not in d:
            raise ValueError(f"{name} must be one of {sorted(d)}, not {v!r}")
    return OhColour(int(in_transfer), int(in_primaries), int(out_primaries), COL_OUT[out], COL_TONE[tone], COL_NORM[norm],
                    float(src_peak), float(dst_peak), float(white))


def colour_tables(col):
    """oh_colour_tables (host only): (A, G, B, misc) as int32 arrays, exactly the integers the kernel receives"""
    A, G, B, misc = np.zeros(COL_NA, np.int32), np.zeros(COL_NP, np.int32), np.zeros(COL_NP, np.int32), np.zeros(COL_NMISC, np.int32)
    P = C.POINTER(C.c_int32)
    rc = lib().oh_colour_tables(C.byref(col), A.ctypes.data_as(P), G.ctypes.data_as(P), B.ctypes.data_as(P), misc.ctypes.data_as(P))
    _check(rc, "oh_colour_tables")
    return A, G, B, misc


LL_NBINS, LL_FULL = 258, 1 << 30                                                       # OH_LL_NBINS; full scale of linear light


class OhLightSpec(C.Structure):                               # include/ohevc_hip.h
    _fields_ = [("in_transfer", C.c_int32), ("in_primaries", C.c_int32), ("norm", C.c_int32), ("src_peak", C.c_float)]


class OhLightLevel(C.Structure):                              # include/ohevc_hip.h
    _fields_ = [("pixels", C.c_uint64), ("sum", C.c_uint64), ("max", C.c_uint32), ("min", C.c_uint32), ("hist", C.c_uint32 * LL_NBINS)]


class LightLevel:
    """the light-level statistics of one picture (OhLightLevel): pixels, sum, max, min of the norm v (2^30 = full scale) and hist, a
    numpy uint32 array of LL_NBINS counts; full_scale: the nits of 2^30 they were measured with (None: not known)"""
    __slots__ = ("pixels", "sum", "max", "min", "hist", "full_scale")

    def __init__(self, pixels, sum, max, min, hist, full_scale=None):
        self.pixels, self.sum, self.max, self.min = int(pixels), int(sum), int(max), int(min)
        self.hist = np.ascontiguousarray(hist, dtype=np.uint32)
        if self.hist.shape != (LL_NBINS,):
            raise ValueError(f"hist: {LL_NBINS} counts, not {self.hist.shape}")
        self.full_scale = None if full_scale is None else float(full_scale)

    def __repr__(self):
        return f"LightLevel(pixels={self.pixels}, sum={self.sum}, max={self.max}, min={self.min})"

    def as_struct(self):
        ll = OhLightLevel(self.pixels, self.sum, self.max, self.min)
        C.memmove(ll.hist, self.hist.ctypes.data, 4 * LL_NBINS)
        return ll


def light_bin(v):
    """oh_light_bin (host only): the histogram bin of a norm v, v clamped to 2^30"""
    return int(lib().oh_light_bin(int(v)))


def light_bin_upper(b):
    """oh_light_bin_upper (host only): the largest v of a bin"""
    return int(lib().oh_light_bin_upper(int(b)))


def light_percentile(lls, ppm=999900):
    """oh_light_percentile (host only): the pictures of lls (LightLevel) pooled as one scene -> the upper edge of the first bin at
    which ppm millionths of the pixels are reached, at most the largest max; in units of 2^-30 of the full scale"""
    lls = list(lls)
    arr = (OhLightLevel * max(len(lls), 1))(*[ll.as_struct() for ll in lls])
    v = C.c_uint32()
    rc = lib().oh_light_percentile(arr, len(lls), int(ppm), C.byref(v))
    _check(rc, "oh_light_percentile")
    return v.value


def light_nits(value, in_transfer, src_peak):
    """a norm value of the light-level pass in nits: 2^30 is 10000 nits for PQ (in_transfer 16), src_peak nits otherwise (HLG: of scene
    light, before the OOTF)"""
    return value / LL_FULL * (10000.0 if int(in_transfer) == 16 else float(src_peak))


def source_peak(in_transfer, lls=None, sei=None, ppm=999900, default=1000.0):
    """src_peak in nits for make_colour, from the first of these that is there: the measured percentile of lls (LightLevel of
    Engine.pics_light_level, pooled as one scene; other transfers than PQ scale by the full scale they were measured with, default
    where that is not known); the SEI's MaxCLL (sei: the dict of annexb.hdr_sei) when it is not zero; the mastering display's
    max_lum / 10000 when present and not zero; default.  A result at or below the display's dst_peak means the content fits the
    display: convert with tone="none" (OH_TONE_BT2390 refuses dst_peak >= src_peak)."""
    if lls:
        lls = list(lls)
        return light_nits(light_percentile(lls, ppm), in_transfer, lls[0].full_scale if lls[0].full_scale is not None else default)
    if sei:
        if sei.get("max_cll"):
            return float(sei["max_cll"])
        if sei.get("max_lum"):
            return sei["max_lum"] / 10000.0
    return float(default)


CMP_SSIM, CMP_NONE = 1, 0xFFFFFFFF                                                      # OH_CMP_SSIM, OH_CMP_NONE
CMP_TW, CMP_TH = 256, 32                                                                # OH_CMP_TW, OH_CMP_TH (csrc/kernels.h): the kernel's tile


class OhCompareSpec(C.Structure):                             # include/ohevc_hip.h
    _fields_ = [("win", OhWindow), ("flags", C.c_int32)]


class OhPlaneDiff(C.Structure):                               # include/ohevc_hip.h
    _fields_ = [("samples", C.c_uint64), ("differing", C.c_uint64), ("sad", C.c_uint64), ("sse", C.c_uint64), ("max_abs", C.c_uint32),
                ("first_x", C.c_uint32), ("first_y", C.c_uint32), ("ssim_windows", C.c_uint64), ("ssim_sum", C.c_int64)]


class OhCompare(C.Structure):                                 # include/ohevc_hip.h
    _fields_ = [("plane", OhPlaneDiff * 3)]


def compare_psnr(sse, samples, bit_depth):
    """oh_compare_psnr (host only): 10 log10(M^2 samples / sse) in dB, inf for sse 0, NaN for samples 0"""
    return float(lib().oh_compare_psnr(int(sse), int(samples), int(bit_depth)))


def compare_ssim_consts(bit_depth):
    """oh_compare_ssim_consts (host only): (c1, c2) of the SSIM windows at that bit depth"""
    c1, c2 = C.c_int64(), C.c_int64()
    _check(lib().oh_compare_ssim_consts(int(bit_depth), C.byref(c1), C.byref(c2)), "oh_compare_ssim_consts")
    return c1.value, c2.value


def compare_ssim_window(bit_depth, s1, s2, ss, s12):
    """oh_compare_ssim_window (host only): the Q30 value of one 8x8 window from its sums, by the function the kernel evaluates"""
    return int(lib().oh_compare_ssim_window(int(bit_depth), int(s1), int(s2), int(ss), int(s12)))


class PlaneDiff:
    """one plane of a compared pair (OhPlaneDiff): samples, differing, sad, sse, max_abs, first (None or (x, y) in plane-window
    coordinates), ssim_windows, ssim_sum (Q30); psnr, mse and ssim derive from them"""
    __slots__ = ("samples", "differing", "sad", "sse", "max_abs", "first", "ssim_windows", "ssim_sum", "bit_depth")

    def __init__(self, d, bit_depth):
        self.samples, self.differing, self.sad, self.sse, self.max_abs = int(d.samples), int(d.differing), int(d.sad), int(d.sse), int(d.max_abs)
        self.first = None if d.first_x == CMP_NONE else (int(d.first_x), int(d.first_y))
        self.ssim_windows, self.ssim_sum = int(d.ssim_windows), int(d.ssim_sum)
        self.bit_depth = int(bit_depth)

    def __repr__(self):
        return (f"PlaneDiff(samples={self.samples}, differing={self.differing}, sad={self.sad}, sse={self.sse}, max_abs={self.max_abs}, "
                f"first={self.first}, ssim_windows={self.ssim_windows}, ssim_sum={self.ssim_sum})")

    @property
    def psnr(self):
        return compare_psnr(self.sse, self.samples, self.bit_depth)

    @property
    def mse(self):
        return self.sse / self.samples if self.samples else None

    @property
    def ssim(self):
        return self.ssim_sum / self.ssim_windows / (1 << 30) if self.ssim_windows else None


class Compare:
    """a compared pair (OhCompare): plane, three PlaneDiff (those a 4:0:0 picture lacks are all zero)"""
    __slots__ = ("plane",)

    def __init__(self, o, bit_depth):
        self.plane = [PlaneDiff(o.plane[c], bit_depth) for c in range(3)]

    def __repr__(self):
        return f"Compare({self.plane})"


class OhResize(C.Structure):                                  # include/ohevc_hip.h
    _fields_ = [("filter", C.c_int32), ("win", OhWindow), ("width", C.c_int32), ("height", C.c_int32)]


RESIZE_FILTERS = {"bilinear": 0, "bicubic": 1}                                          # OH_RESIZE_BILINEAR, OH_RESIZE_BICUBIC
RESIZE_MAX_PICS, RESIZE_MAX_DOWN, RESIZE_MAX_UP = 64, 128, 16


def resize_filter(filt):
    """a filter name of RESIZE_FILTERS or its OH_RESIZE_* number -> the number"""
    return _enum(RESIZE_FILTERS, "filter", filt)


def resize_taps(src_extent, dst_extent, filter="bilinear", phase=2):
    """oh_resize_taps (host only): per sample of the resized axis (first source index inside the window, [integer coefficients]),
    the integers the kernels receive; phase 2: centred samples, 1: the co-sited chroma columns of 4:2:0 / 4:2:2"""
    f = resize_filter(filter)
    mt = lib().oh_resize_max_taps(src_extent, dst_extent, f)
    _check(mt, f"oh_resize_max_taps({src_extent}, {dst_extent}, {f})", mt < 1)
    n = max(dst_extent, 1)
    first, cnt, k = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, mt), np.int16)
    rc = lib().oh_resize_taps(src_extent, dst_extent, f, phase, first.ctypes.data_as(C.POINTER(C.c_int32)),
                              k.ctypes.data_as(C.POINTER(C.c_int16)), mt, cnt.ctypes.data_as(C.POINTER(C.c_int)))
    _check(rc, "oh_resize_taps")
    return [(int(first[x]), [int(v) for v in k[x, :cnt[x]]]) for x in range(dst_extent)]


COMPOSE_MAX_LAYERS, COMPOSE_FILL = 16, 1                                                # OH_COMPOSE_MAX_LAYERS, OH_COMPOSE_FILL
CPS_TW, CPS_TH = 64, 4                                                                  # OH_CPS_TW, OH_CPS_TH (csrc/kernels.h): the kernel's tile, 16-byte granules x rows


class OhLayer(C.Structure):                                   # include/ohevc_hip.h
    _fields_ = [("src_ids", C.POINTER(C.c_int32)), ("sx", C.c_int32), ("sy", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("dx", C.c_int32), ("dy", C.c_int32), ("opacity", C.c_int32), ("alpha", C.c_void_p),
                ("alpha_pixel_stride", C.c_int64), ("alpha_row_stride", C.c_int64), ("alpha_image_stride", C.c_int64)]


class OhCompose(C.Structure):                                 # include/ohevc_hip.h
    _fields_ = [("flags", C.c_int32), ("fill", C.c_int32 * 3), ("n_layers", C.c_int32), ("layers", C.POINTER(OhLayer))]


class Layer:
    """one layer of Engine.pics_compose: src, a finished picture's id for every destination or a list of one id per destination;
    rect = (sx, sy, w, h) of the source in luma samples (None: its whole coded size); at = (dx, dy), where the rectangle's top left
    goes in the destination (may be negative or reach beyond: clipped); opacity 0 .. 256; alpha, None or a torch uint8 tensor on the
    engine's device of shape (h, w), shared by the destinations, or (n, h, w), with any non-negative strides (rgba[..., 3] of an
    image works as it is): straight alpha, one value per luma sample of the rectangle"""
    __slots__ = ("src", "rect", "at", "opacity", "alpha")

    def __init__(self, src, rect=None, at=(0, 0), opacity=256, alpha=None):
        self.src, self.rect, self.at, self.opacity, self.alpha = src, rect, at, opacity, alpha


def compose_blend(dst, src, alpha, opacity):
    """oh_compose_blend (host only): (src w + dst (65280 - w) + 32640) / 65280 with w = alpha opacity, by the function the kernel evaluates"""
    return int(lib().oh_compose_blend(int(dst), int(src), int(alpha), int(opacity)))


def compose_chroma_alpha(chroma_format_idc, a00, a01, a10, a11):
    """oh_compose_chroma_alpha (host only): the alpha of a chroma sample from the luma alphas it covers"""
    return int(lib().oh_compose_chroma_alpha(int(chroma_format_idc), int(a00), int(a01), int(a10), int(a11)))


class OhReformat(C.Structure):                                # include/ohevc_hip.h
    _fields_ = [("depth", C.c_int32), ("chroma_down", C.c_int32), ("chroma_up", C.c_int32)]


RF_DEPTH = {"round": 0, "dither": 1}                                                    # OH_RF_ROUND, OH_RF_DITHER
RF_FILTERS = {"point": 0, "nearest": 0, "linear": 1}                                    # OH_RF_POINT, OH_RF_LINEAR
RF_SEG = 4096                                                                          # OH_RF_SEG (csrc/kernels.h): plane samples per workgroup segment


def reformat_quantise(sum, s, mode, x, y, bit_depth):
    """oh_reformat_quantise (host only): a weighted sum of source samples -> the destination sample of bit_depth bits, shifted down by s
    bits with one rounding (mode "round" or "dither", or its number) at place (x, y) of its plane, by the function the kernel evaluates"""
    return int(lib().oh_reformat_quantise(int(sum), int(s), _enum(RF_DEPTH, "depth mode", mode), int(x), int(y), int(bit_depth)))


class OhOrient(C.Structure):                                  # include/ohevc_hip.h
    _fields_ = [("orientation", C.c_int32), ("win", OhWindow)]


ORIENT_HFLIP, ORIENT_VFLIP, ORIENT_TRANSPOSE = 1, 2, 4                                  # OH_ORIENT_*: an orientation is any OR of these
ORIENTATIONS = {"identity": 0, "hflip": 1, "vflip": 2, "rot180": 3, "transpose": 4, "rot90": 5, "rot270": 6, "antitranspose": 7}
ORIENT_TILE = 64                                                                        # OH_OR_TILE (csrc/kernels.h): edge of the transposing kernel's tile


def orient_code(v):
    """a name of ORIENTATIONS ("rot90" is clockwise) or an int 0 .. 7 -> the int"""
    return _enum(ORIENTATIONS, "orientation", v, range(8))


def orient_then(first, second):
    """oh_orient_then (host only): the one orientation equal to applying first, then second"""
    return int(lib().oh_orient_then(orient_code(first), orient_code(second)))


def orient_inverse(o):
    """oh_orient_inverse (host only): the orientation that undoes o"""
    return int(lib().oh_orient_inverse(orient_code(o)))


def orient_size(o, width, height):
    """oh_orient_size (host only): (width, height) of the image of a width x height window: swapped under TRANSPOSE"""
    ow, oh = C.c_int(), C.c_int()
    _check(lib().oh_orient_size(orient_code(o), int(width), int(height), C.byref(ow), C.byref(oh)), "oh_orient_size")
    return ow.value, oh.value


def orientation_from_sei(hor_flip, ver_flip, anticlockwise_rotation):
    """oh_orient_from_sei (host only): the orientation a display-orientation SEI message recommends (annexb.display_orientation has
    its fields): the flips, then the anticlockwise rotation of the flipped picture, in units of 360 / 65536 degrees.  EngineError with
    code OH_E_UNSUPPORTED for an angle that is no quarter turn."""
    o = C.c_int()
    rc = lib().oh_orient_from_sei(int(hor_flip), int(ver_flip), int(anticlockwise_rotation), C.byref(o))
    _check(rc, f"oh_orient_from_sei({hor_flip}, {ver_flip}, {anticlockwise_rotation:#x})")
    return o.value


class OhWarp(C.Structure):                                    # include/ohevc_hip.h
    _fields_ = [("mode", C.c_int32), ("filter", C.c_int32), ("border", C.c_int32), ("fill", C.c_uint16 * 3), ("win", OhWindow),
                ("width", C.c_int32), ("height", C.c_int32), ("m", C.c_int64 * 9)]


WARP_MODES = {"affine": 0, "perspective": 1}                                            # OH_WARP_AFFINE, OH_WARP_PERSPECTIVE
WARP_FILTERS = {"nearest": 0, "bilinear": 1, "bicubic": 2}                              # OH_WARP_NEAREST .. OH_WARP_BICUBIC
WARP_BORDERS = {"replicate": 0, "constant": 1}                                          # OH_WARP_REPLICATE, OH_WARP_CONSTANT
WARP_TILE = (64, 16)                                                                    # WARP_TW, WARP_TH (csrc/warp_common.h): a workgroup's tile


def _warp_built(name, *args):
    """one of the C builders, which fill a whole OhWarp"""
    w = OhWarp()
    _check(getattr(lib(), name)(*args, C.byref(w)), name)
    return w


def warp_matrix(matrix, mode=None):
    """(mode, the nine int64 of OhWarp.m) from any form Engine.pics_warp takes: an OhWarp; 6 or 9 integers in the fixed-point layout
    of OhWarp.m (6: affine, m[6 .. 8] = 0, 0, 2^30); a float 2 x 3 or 3 x 3 numpy array, the inverse map (destination -> source) in luma
    samples.  A float array is rounded here and nowhere else: a 3 x 3 array is first divided by its [2][2] entry (which must not be
    0), then m[0 .. 5] = rint(65536 a) and m[6], m[7] = rint(2^30 a), m[8] = 2^30; rint is numpy's, halves to even, in float64.  mode
    None: affine for 6 numbers or 2 x 3, perspective for 9 or 3 x 3."""
    if isinstance(matrix, OhWarp):
        return (matrix.mode if mode is None else _enum(WARP_MODES, "mode", mode, WARP_MODES.values())), [int(v) for v in matrix.m]
    a = np.asarray(matrix)
    if a.dtype.kind == "f":
        if a.shape not in ((2, 3), (3, 3)):
            raise ValueError(f"a float matrix of shape {a.shape}: 2 x 3 or 3 x 3")
        a = a.astype(np.float64)
        if not np.isfinite(a).all():
            raise ValueError("a matrix with an entry that is not finite")
        if a.shape == (3, 3):
            if a[2, 2] == 0:
                raise ValueError("a 3 x 3 matrix whose [2][2] entry is 0")
            a = a / a[2, 2]
        m = [int(v) for v in np.rint(a[:2].reshape(-1) * 65536.0)]
        m += [int(np.rint(a[2, 0] * 2.0 ** 30)), int(np.rint(a[2, 1] * 2.0 ** 30)), 1 << 30] if a.shape == (3, 3) else [0, 0, 1 << 30]
        inferred = 1 if a.shape == (3, 3) else 0
    else:
        if a.dtype.kind not in "iu" or a.size not in (6, 9):
            raise ValueError("a matrix is an OhWarp, 6 or 9 integers, or a float 2 x 3 / 3 x 3 array")
        m = [int(v) for v in a.reshape(-1)]
        inferred = 1 if len(m) == 9 else 0
        m += [0, 0, 1 << 30] if len(m) == 6 else []
    if any(not -(1 << 63) <= v < 1 << 63 for v in m):
        raise ValueError("a coefficient does not fit int64")
    return (inferred if mode is None else _enum(WARP_MODES, "mode", mode, WARP_MODES.values())), m


def warp_identity():
    """oh_warp_identity (host only): the OhWarp of the identity map — affine, bilinear, replicate; width and height 0"""
    return _warp_built("oh_warp_identity")


def warp_translation(dx_q2, dy_q2):
    """oh_warp_translation (host only): destination (x, y) reads source (x + dx_q2 / 4, y + dy_q2 / 4): quarter samples, the
    convention of OhMotionVector"""
    return _warp_built("oh_warp_translation", int(dx_q2), int(dy_q2))


def warp_rotation(anticlockwise, centre_src, centre_dst, scale_q16=65536):
    """oh_warp_rotation (host only): an anticlockwise turn by `anticlockwise` units of 360 / 65536 degrees that carries the source
    position centre_src = (x, y) to the destination position centre_dst, both Q16 luma samples; scale_q16: source samples per
    destination sample"""
    return _warp_built("oh_warp_rotation", int(anticlockwise), int(centre_src[0]), int(centre_src[1]), int(centre_dst[0]), int(centre_dst[1]),
                       int(scale_q16))


def warp_then(first, second):
    """oh_warp_then (host only, affine maps): the one map equal to warping by first, then warping its image by second"""
    return _warp_built("oh_warp_then", C.byref(first), C.byref(second))


def warp_invert(fwd):
    """oh_warp_invert (host only, affine maps): a source -> destination map becomes the destination -> source map the service takes"""
    return _warp_built("oh_warp_invert", C.byref(fwd))


def warp_from_sei(hor_flip, ver_flip, anticlockwise_rotation, width, height):
    """oh_warp_from_sei (host only): (OhWarp, (image width, image height)) of a display-orientation SEI message at any angle
    (annexb.display_orientation has its fields) for pictures of width x height luma samples: the flips, then the anticlockwise
    rotation about the centre, into the rotated bounding box rounded up to even sizes.  The result is affine, bilinear, replicate."""
    w, ow, oh = OhWarp(), C.c_int(), C.c_int()
    rc = lib().oh_warp_from_sei(int(hor_flip), int(ver_flip), int(anticlockwise_rotation), int(width), int(height), C.byref(w), C.byref(ow), C.byref(oh))
    _check(rc, f"oh_warp_from_sei({hor_flip}, {ver_flip}, {anticlockwise_rotation:#x}, {width}, {height})")
    return w, (ow.value, oh.value)


def warp_paths(warp, bit_depth, chroma_format_idc, dst_width, dst_height):
    """oh_warp_paths (host only): (tiles that stage their taps in LDS, tiles that gather them from global memory) of a call with
    this OhWarp into destinations of dst_width x dst_height: the kernel's own predicate"""
    s, g = C.c_int64(), C.c_int64()
    rc = lib().oh_warp_paths(C.byref(warp), int(bit_depth), int(chroma_format_idc), int(dst_width), int(dst_height), C.byref(s), C.byref(g))
    _check(rc, "oh_warp_paths")
    return s.value, g.value


class OhFieldInfo(C.Structure):                               # include/ohevc_hip.h
    _fields_ = [("kind", C.c_int32), ("pair", C.c_int32), ("top_first", C.c_int32), ("repeat_first", C.c_int32), ("frames", C.c_int32)]


class OhDeinterlace(C.Structure):                             # include/ohevc_hip.h
    _fields_ = [("mode", C.c_int32), ("parity", C.c_int32), ("kept_first", C.c_int32)]


FieldInfo = collections.namedtuple("FieldInfo", "kind pair top_first repeat_first frames")
FIELD_FRAME, FIELD_TOP, FIELD_BOTTOM = 0, 1, 2                                          # FieldInfo.kind
DEINT_BOB, DEINT_BLEND, DEINT_LOWPASS5, DEINT_ADAPTIVE = 0, 1, 2, 3                     # OH_DEINT_*
DEINT_MODES = {"bob": DEINT_BOB, "blend": DEINT_BLEND, "lowpass5": DEINT_LOWPASS5, "adaptive": DEINT_ADAPTIVE}
DEINT_SEG = 4096                                                                        # OH_DI_SEG (csrc/kernels.h): samples of a row per workgroup


def field_info(pic_struct):
    """oh_field_info (host only): what a pic_struct of the picture timing SEI (annexb.pic_timing) says, H.265 Table D.2, as a
    FieldInfo: kind 0 frame / 1 top field / 2 bottom field; pair -1 / +1 where the field pairs with the previous / next picture in
    output order, else 0; top_first 1 / 0 where the message says which field of a frame is first, else -1; repeat_first; frames, how
    often a frame is shown (2 doubling, 3 tripling).  EngineError with code OH_E_ARG outside 0 .. 12."""
    fi = OhFieldInfo()
    _check(lib().oh_field_info(int(pic_struct), C.byref(fi)), f"oh_field_info({pic_struct})")
    return FieldInfo(fi.kind, fi.pair, fi.top_first, fi.repeat_first, fi.frames)


def deint_mode(v):
    """a name of DEINT_MODES or an int 0 .. 3 -> the int"""
    return _enum(DEINT_MODES, "deinterlacing mode", v, range(4))


def deint_adaptive(up, dn, a, b, pu, pd, nu, nd):
    """oh_deint_adaptive (host only): one missing sample of the adaptive mode from its window: up / dn seven kept samples of cur
    above and below (columns x - 3 .. x + 3), a / b the two samples at its own place before and after, pu / pd / nu / nd the samples
    above and below it in prev and next"""
    up, dn = [int(v) for v in up], [int(v) for v in dn]
    if len(up) != 7 or len(dn) != 7:
        raise ValueError("up and dn hold seven samples each")
    return int(lib().oh_deint_adaptive((C.c_int32 * 7)(*up), (C.c_int32 * 7)(*dn), int(a), int(b), int(pu), int(pd), int(nu), int(nd)))


FILTER_MAX_TAPS = 15                                                                    # OH_FILTER_MAX_TAPS


class OhFilterTaps(C.Structure):                              # include/ohevc_hip.h
    _fields_ = [("nh", C.c_int32), ("nv", C.c_int32), ("h", C.c_int16 * FILTER_MAX_TAPS), ("v", C.c_int16 * FILTER_MAX_TAPS)]


class OhFilter(C.Structure):                                  # include/ohevc_hip.h
    _fields_ = [("mode", C.c_int32), ("planes", C.c_int32), ("taps", OhFilterTaps * 2), ("amount", C.c_int32 * 2),
                ("threshold", C.c_int32 * 2)]


FILTER_CONVOLVE, FILTER_UNSHARP, FILTER_MEDIAN, FILTER_TEMPORAL = 0, 1, 2, 3             # OH_FILTER_*
FILTER_MODES = {"convolve": FILTER_CONVOLVE, "unsharp": FILTER_UNSHARP, "median": FILTER_MEDIAN, "temporal": FILTER_TEMPORAL}
FILTER_TW, FILTER_TH = 128, 32                                                          # OH_FLT_TW, OH_FLT_TH (csrc/kernels.h): a workgroup's tile


def filter_mode(v):
    """a name of FILTER_MODES or an int 0 .. 3 -> the int"""
    return _enum(FILTER_MODES, "filter mode", v, range(4))


def _filter_row(name, n):
    out = (C.c_int16 * FILTER_MAX_TAPS)()
    _check(getattr(lib(), name)(int(n), out), f"{name}({n})")
    return [int(v) for v in out[:n]]


def filter_binomial(n):
    """oh_filter_binomial (host only): row n - 1 of Pascal's triangle scaled to sum 256, n in {1, 3, 5, 7, 9}"""
    return _filter_row("oh_filter_binomial", n)


def filter_box(n):
    """oh_filter_box (host only): n equal taps of sum 256, n odd in 1 .. 15, the middle one taking the remainder of 256 / n"""
    return _filter_row("oh_filter_box", n)


def filter_taps(h, v):
    """an OhFilterTaps of the horizontal taps h and the vertical taps v; EngineError with code OH_E_ARG unless it is legal
    (oh_filter_taps_check: each axis an odd number of 1 .. 15 taps that sum to 256, their magnitudes to 512 at most)"""
    h, v = [int(k) for k in h], [int(k) for k in v]
    if not 1 <= len(h) <= FILTER_MAX_TAPS or not 1 <= len(v) <= FILTER_MAX_TAPS or any(not -32768 <= k <= 32767 for k in h + v):
        raise ValueError(f"{len(h)} x {len(v)} taps: 1 .. {FILTER_MAX_TAPS} int16 values on either axis")
    t = OhFilterTaps(len(h), len(v))
    t.h[:len(h)] = h
    t.v[:len(v)] = v
    _check(lib().oh_filter_taps_check(C.byref(t)), f"taps {h} x {v}", text="{what} are not legal ({rc})")
    return t


MOTION_MAX_RANGE, MOTION_MAX_CENTRE, MOTION_MAX_LAMBDA = 32, 4096, 4096                  # OH_MOTION_MAX_*


class OhMotionVector(C.Structure):                            # include/ohevc_hip.h
    _fields_ = [("x", C.c_int16), ("y", C.c_int16), ("sad", C.c_uint32), ("sad_centre", C.c_uint32)]


class OhMotionSearch(C.Structure):                            # include/ohevc_hip.h
    _fields_ = [("block", C.c_int32), ("range_x", C.c_int32), ("range_y", C.c_int32), ("subpel", C.c_int32), ("lam", C.c_int32),
                ("centres", C.POINTER(C.c_int16))]


MOTION_DTYPE = np.dtype([("x", np.int16), ("y", np.int16), ("sad", np.uint32), ("sad_centre", np.uint32)])     # OhMotionVector


def motion_blocks(width, height, block=16):
    """oh_motion_blocks (host only): (bw, bh), the blocks of `block` samples across and down a coded luma plane of width x height"""
    bw, bh = C.c_int(0), C.c_int(0)
    _check(lib().oh_motion_blocks(int(width), int(height), int(block), C.byref(bw), C.byref(bh)), f"oh_motion_blocks({width}, {height}, {block})")
    return bw.value, bh.value


def motion_field(field):
    """a field of vectors as a C-contiguous array of MOTION_DTYPE: a structured array as pics_motion returns it, or an integer array whose
    last axis holds (x, y)"""
    f = np.asarray(field)
    if f.dtype == MOTION_DTYPE:
        return np.ascontiguousarray(f)
    if f.dtype.names is not None or f.ndim < 1 or f.shape[-1] != 2 or f.dtype.kind not in "iu":
        raise ValueError("a field is an array of MOTION_DTYPE or an integer array of (x, y) pairs")
    if f.size and (f.min() < -32768 or f.max() > 32767):
        raise ValueError("a vector component is an int16")
    out = np.zeros(f.shape[:-1], dtype=MOTION_DTYPE)
    out["x"], out["y"] = f[..., 0], f[..., 1]
    return out


def motion_scale(coarse, block_c, s, grid, block_f):
    """oh_motion_scale (host only), coarse to fine: coarse, the (bhc, bwc) field of one pair searched with blocks of block_c on pictures
    reduced by the integer factor s (1, 2, 4, 8), becomes the int16 search centres (bh, bw, 2) of the grid = (bw, bh) of blocks of
    block_f on the full pictures: fine block (bx, by) takes the coarse block under it, its centre is (s mv + 2) >> 2 per component"""
    coarse = motion_field(coarse)
    if coarse.ndim != 2:
        raise ValueError(f"motion_scale: the field of one pair has the shape (bh, bw), not {coarse.shape}")
    bw, bh = int(grid[0]), int(grid[1])
    out = np.zeros((max(bh, 0), max(bw, 0), 2), dtype=np.int16)
    _check(lib().oh_motion_scale(coarse.ctypes.data_as(C.POINTER(OhMotionVector)), coarse.shape[1], coarse.shape[0], int(block_c), int(s), bw, bh,
                                      int(block_f), out.ctypes.data_as(C.POINTER(C.c_int16))), "oh_motion_scale")
    return out


HIST_BINS = 4096                                                                        # OH_HIST_BINS
LUT_DEPTHS = (8, 9, 10, 12)
LUT_ROWS, LUT_UNIT, HG_ROWS = 16, 16, 8                                                 # OH_LUT_ROWS, OH_LUT_UNIT, OH_HG_ROWS (csrc/kernels.h)


class OhPlaneHist(C.Structure):                               # include/ohevc_hip.h
    _fields_ = [("samples", C.c_uint64), ("sum", C.c_uint64), ("sum_sq", C.c_uint64), ("min", C.c_uint32), ("max", C.c_uint32),
                ("hist", C.c_uint32 * HIST_BINS)]


class OhHistogram(C.Structure):                               # include/ohevc_hip.h
    _fields_ = [("plane", OhPlaneHist * 3)]


class OhLut(C.Structure):                                     # include/ohevc_hip.h
    _fields_ = [("planes", C.c_int32), ("n_entries", C.c_int32), ("table", C.POINTER(C.c_uint16) * 3)]


class PlaneHist:
    """the code values of one plane of a picture (OhPlaneHist): samples, sum, sum_sq, min, max and hist, a numpy uint32 array of
    2^bit_depth counts; mean and variance derive from the integers and are None for a plane the picture lacks"""
    __slots__ = ("samples", "sum", "sum_sq", "min", "max", "hist")

    def __init__(self, samples, sum, sum_sq, min, max, hist):
        self.samples, self.sum, self.sum_sq, self.min, self.max = int(samples), int(sum), int(sum_sq), int(min), int(max)
        self.hist = np.ascontiguousarray(hist, dtype=np.uint32)
        if self.hist.ndim != 1 or self.hist.size > HIST_BINS:
            raise ValueError(f"hist: at most {HIST_BINS} counts in one dimension, not {self.hist.shape}")

    def __repr__(self):
        return f"PlaneHist(samples={self.samples}, sum={self.sum}, sum_sq={self.sum_sq}, min={self.min}, max={self.max})"

    @property
    def mean(self):
        return self.sum / self.samples if self.samples else None

    @property
    def variance(self):
        """the population variance, from the integers: (samples sum_sq - sum^2) / samples^2"""
        return (self.samples * self.sum_sq - self.sum * self.sum) / (self.samples * self.samples) if self.samples else None

    def as_struct(self):
        h = OhPlaneHist(self.samples, self.sum, self.sum_sq, self.min, self.max)
        C.memmove(h.hist, self.hist.ctypes.data, 4 * self.hist.size)
        return h


class Histogram:
    """the code values of one picture (OhHistogram): plane, three PlaneHist (those a 4:0:0 picture lacks are all zero)"""
    __slots__ = ("plane",)

    def __init__(self, o, bit_depth):
        self.plane = [PlaneHist(p.samples, p.sum, p.sum_sq, p.min, p.max, np.frombuffer(p.hist, dtype=np.uint32)[:1 << bit_depth].copy())
                      for p in o.plane]

    def __repr__(self):
        return f"Histogram({self.plane})"


def _hist_array(hists):
    """PlaneHist objects (or one) -> (a ctypes array of OhPlaneHist, their number)"""
    hists = [hists] if isinstance(hists, PlaneHist) else list(hists)
    return (OhPlaneHist * max(len(hists), 1))(*[h.as_struct() for h in hists]), len(hists)


def hist_percentile(hists, ppm):
    """oh_hist_percentile (host only): the PlaneHist of hists pooled -> the smallest value at or below which ppm millionths of the
    samples lie; 0 gives the minimum, 1000000 the maximum"""
    arr, n = _hist_array(hists)
    v = C.c_uint32()
    _check(lib().oh_hist_percentile(arr, n, int(ppm), C.byref(v)), "oh_hist_percentile")
    return v.value


def hist_distance(a, b):
    """oh_hist_distance (host only): the sum over all values of |a.hist - b.hist| of two PlaneHist, the scene-cut measure"""
    sad = C.c_uint64()
    _check(lib().oh_hist_distance(C.byref(a.as_struct()), C.byref(b.as_struct()), C.byref(sad)), "oh_hist_distance")
    return sad.value


def _lut_built(name, n_entries, *args):
    """a table builder of the library -> a numpy uint16 array of n_entries values"""
    out = np.zeros(max(int(n_entries), 1), dtype=np.uint16)
    _check(getattr(lib(), name)(*args, out.ctypes.data_as(C.POINTER(C.c_uint16))), name)
    return out


def _lut_entries(bit_depth):
    """the entries of a table indexed by samples of bit_depth bits; a depth no builder takes makes one entry, and the builder refuses"""
    return 1 << int(bit_depth) if int(bit_depth) in LUT_DEPTHS else 1


def lut_identity(bs, bd):
    """oh_lut_identity (host only): the table of a plain depth change from bs to bd bits, rounding to nearest"""
    return _lut_built("oh_lut_identity", _lut_entries(bs), int(bs), int(bd))


def lut_range(bs, bd, to_full, chroma=False):
    """oh_lut_range (host only): limited -> full range (to_full) or full -> limited, of luma or of chroma, from bs to bd bits"""
    return _lut_built("oh_lut_range", _lut_entries(bs), int(bs), int(bd), int(bool(to_full)), int(bool(chroma)))


def lut_linear(bs, bd, gain_q16, pivot_in=0, pivot_out=0):
    """oh_lut_linear (host only): (v - pivot_in) gain_q16 / 65536 + pivot_out, rounded and clamped to bd bits; 65536 is a gain of 1"""
    return _lut_built("oh_lut_linear", _lut_entries(bs), int(bs), int(bd), int(gain_q16), int(pivot_in), int(pivot_out))


def lut_stretch(hists, bit_depth, lo_ppm=0, hi_ppm=0):
    """oh_lut_stretch (host only): auto-levels from the pooled PlaneHist of hists: the lo_ppm percentile goes to 0, the value hi_ppm
    below the top to the maximum"""
    arr, n = _hist_array(hists)
    return _lut_built("oh_lut_stretch", _lut_entries(bit_depth), arr, n, int(lo_ppm), int(hi_ppm), int(bit_depth))


def lut_equalise(hists, bit_depth):
    """oh_lut_equalise (host only): the table that equalises the pooled PlaneHist of hists"""
    arr, n = _hist_array(hists)
    return _lut_built("oh_lut_equalise", _lut_entries(bit_depth), arr, n, int(bit_depth))


def lut_then(first, second):
    """oh_lut_then (host only): second[first[v]], two tables as one"""
    first, second = np.ascontiguousarray(first, dtype=np.uint16), np.ascontiguousarray(second, dtype=np.uint16)
    P = C.POINTER(C.c_uint16)
    return _lut_built("oh_lut_then", first.size, first.ctypes.data_as(P), first.size, second.ctypes.data_as(P), second.size)


class OhGrain(C.Structure):                                   # include/ohevc_hip.h
    _fields_ = [("planes", C.c_int32), ("blending", C.c_int32), ("log2_scale", C.c_int32), ("table", C.POINTER(C.c_uint32) * 3)]


GRAIN_BLENDINGS = {"additive": 0, "multiplicative": 1}                                  # OH_GRAIN_ADDITIVE, OH_GRAIN_MULTIPLICATIVE
GRAIN_ENTRIES = 256                                                                     # OH_GRAIN_ENTRIES
GRAIN_TILE = (256, 8)                                                                   # GRAIN_TW blocks of GRAIN_BLOCK: a workgroup's tile


class Grain:
    """what Engine.pics_grain adds (OhGrain): tables, a numpy uint32 array (3, 256) of sigma | fh << 8 | fv << 12 per plane and 8-bit
    block mean; planes, bit c set: plane c gets grain; blending, 0 additive or 1 multiplicative; log2_scale, 0 .. 15"""
    __slots__ = ("tables", "planes", "blending", "log2_scale")

    def __init__(self, tables, planes=7, blending=0, log2_scale=0):
        t = np.asarray(tables)
        if t.shape != (3, GRAIN_ENTRIES) or t.dtype.kind not in "iu" or (t.size and (t.min() < 0 or t.max() > 0xFFFFFFFF)):
            raise ValueError(f"grain: tables of shape {t.shape}, not (3, {GRAIN_ENTRIES}) entries of 32 bits")
        self.tables = np.ascontiguousarray(t, dtype=np.uint32)
        self.planes, self.blending, self.log2_scale = int(planes), _enum(GRAIN_BLENDINGS, "blending", blending), int(log2_scale)

    def __repr__(self):
        return f"Grain(planes={self.planes}, blending={self.blending}, log2_scale={self.log2_scale})"

    def as_struct(self, planes=None):
        """the OhGrain; it points into self.tables, which must outlive the call it is passed to"""
        g = OhGrain(self.planes if planes is None else int(planes), self.blending, self.log2_scale)
        for c in range(3):
            g.table[c] = self.tables[c].ctypes.data_as(C.POINTER(C.c_uint32))
        return g


def grain_hash(a, b, c, d):
    """oh_grain_hash (host only): H(a, b, c, d) of the film grain definition, four uint32 -> uint32"""
    return int(lib().oh_grain_hash(a & 0xFFFFFFFF, b & 0xFFFFFFFF, c & 0xFFFFFFFF, d & 0xFFFFFFFF))


def grain_pattern(fh, fv, parts=False):
    """oh_grain_pattern (host only): pattern (fh, fv), cut-offs 2 .. 14 in sixteenths of the band: a numpy int8 array (32, 32); parts:
    (coefficients int16, raw int16, pattern int8) instead"""
    c, r, p = np.zeros((32, 32), np.int16), np.zeros((32, 32), np.int16), np.zeros((32, 32), np.int8)
    I16 = C.POINTER(C.c_int16)
    _check(lib().oh_grain_pattern(int(fh), int(fv), c.ctypes.data_as(I16), r.ctypes.data_as(I16), p.ctypes.data_as(C.POINTER(C.c_int8))),
           "oh_grain_pattern")
    return (c, r, p) if parts else p


def make_grain(sigma, fh=8, fv=None, *, log2_scale=0, blending="additive", planes=7):
    """one entry for every intensity of every plane (oh_grain_uniform): sigma 0 .. 255, the horizontal and vertical cut-off fh, fv
    (2 .. 14; fv None: fh).  The standard deviation of the grain is about sigma / 2^log2_scale code values of an 8-bit picture."""
    t = np.zeros((3, GRAIN_ENTRIES), dtype=np.uint32)
    _check(lib().oh_grain_uniform(int(sigma), int(fh), int(fh if fv is None else fv), t[0].ctypes.data_as(C.POINTER(C.c_uint32))),
           "oh_grain_uniform")
    t[1:] = t[0]
    return Grain(t, planes, blending, log2_scale)


def grain_from_sei(sei):
    """oh_grain_from_sei (host only): the dict of annexb.film_grain (or an annexb.OhFilmGrainSei) -> the Grain of its tables, planes,
    blending and scale.  EngineError with code OH_E_UNSUPPORTED for a message outside the profile (model 0, up to three model values,
    cut-offs 2 .. 14, intervals that do not overlap), OH_E_ARG for a cancelled one.  The separate colour description is ignored."""
    from . import annexb as A
    if sei is None:
        raise ValueError("grain_from_sei: no message")
    s = sei if isinstance(sei, A.OhFilmGrainSei) else A.film_grain_to_struct(sei)
    t = np.zeros((3, GRAIN_ENTRIES), dtype=np.uint32)
    g = OhGrain()
    _check(lib().oh_grain_from_sei(C.byref(s), t.ctypes.data_as(C.c_void_p), C.byref(g)), "oh_grain_from_sei")
    return Grain(t, g.planes, g.blending, g.log2_scale)


def grain_block(seed, c, bx, by):
    """oh_grain_block (host only): (ox, oy, negate) of block (bx, by) of plane c of a picture with that seed"""
    ox, oy, neg = C.c_int(), C.c_int(), C.c_int()
    _check(lib().oh_grain_block(int(seed) & 0xFFFFFFFF, int(c), int(bx), int(by), C.byref(ox), C.byref(oy), C.byref(neg)), "oh_grain_block")
    return ox.value, oy.value, neg.value


def grain_seeds(seeds, n):
    """the seeds of n pictures as a numpy uint32 array: a sequence of n ints, or one int b, which stands for b + i (a run of POCs);
    every seed is taken modulo 2^32"""
    if hasattr(seeds, "__len__"):
        if len(seeds) != n:
            raise ValueError(f"seeds: {len(seeds)} for {n} pictures")
        return np.array([int(s) & 0xFFFFFFFF for s in seeds], dtype=np.uint32)
    return np.array([(int(seeds) + i) & 0xFFFFFFFF for i in range(n)], dtype=np.uint32)


class OhRemap(C.Structure):                                   # include/ohevc_hip.h
    _fields_ = [("in_bit_depth", C.c_int32), ("out_bit_depth", C.c_int32), ("pre", C.POINTER(C.c_uint16) * 3),
                ("coeff", (C.c_int32 * 3) * 3), ("log2_denom", C.c_int32), ("post", C.POINTER(C.c_uint16) * 3)]


REMAP_MAX_PIVOTS = 33                                                                   # OH_CRI_MAX_PIVOTS
REMAP_ROWS = 8                                                                          # OH_REMAP_ROWS: a workgroup's band of rows


def _remap_tables(what, tables, bit_depth):
    t = np.asarray(tables)
    entries = 1 << bit_depth if 0 <= bit_depth <= 16 else -1
    if t.shape != (3, entries) or t.dtype.kind not in "iu" or (t.size and (t.min() < 0 or t.max() > 0xFFFF)):
        raise ValueError(f"remap: {what} tables of shape {t.shape}, not (3, {entries}) entries of 16 bits")
    return np.ascontiguousarray(t, dtype=np.uint16)


class Remap:
    """what Engine.pics_colour_remap applies (OhRemap): pre, a numpy uint16 array (3, 2^in_bit_depth) of values 0 .. 2^out_bit_depth - 1;
    coeff, a numpy int32 array (3, 3) with log2_denom, its denominator's logarithm; post, a numpy uint16 array (3, 2^out_bit_depth)"""
    __slots__ = ("pre", "coeff", "log2_denom", "post", "in_bit_depth", "out_bit_depth")

    def __init__(self, pre, coeff, log2_denom, post, in_bit_depth, out_bit_depth=None):
        self.in_bit_depth = int(in_bit_depth)
        self.out_bit_depth = self.in_bit_depth if out_bit_depth is None else int(out_bit_depth)
        self.pre = _remap_tables("pre", pre, self.in_bit_depth)
        self.post = _remap_tables("post", post, self.out_bit_depth)
        k = np.asarray(coeff)
        if k.shape != (3, 3) or k.dtype.kind not in "iu" or abs(k).max() > 0x7FFFFFFF:
            raise ValueError(f"remap: coeff of shape {k.shape}, not (3, 3) integers of 32 bits")
        self.coeff = np.ascontiguousarray(k, dtype=np.int32)
        self.log2_denom = int(log2_denom)

    def __repr__(self):
        return f"Remap({self.in_bit_depth} -> {self.out_bit_depth} bit, coeff={self.coeff.tolist()}, log2_denom={self.log2_denom})"

    def as_struct(self):
        """the OhRemap; it points into self.pre and self.post, which must outlive the call it is passed to"""
        r = OhRemap(self.in_bit_depth, self.out_bit_depth)
        r.log2_denom = self.log2_denom
        for c in range(3):
            r.pre[c] = self.pre[c].ctypes.data_as(C.POINTER(C.c_uint16))
            r.post[c] = self.post[c].ctypes.data_as(C.POINTER(C.c_uint16))
            for i in range(3):
                r.coeff[c][i] = int(self.coeff[c, i])
        return r

    def luts(self):
        """oh_remap_luts (host only): where the matrix is diagonal, the three tables of 2^in_bit_depth entries that do the same plane by
        plane — for Engine.pics_lut(pids, list(remap.luts()), bit_depth=remap.out_bit_depth), at any chroma format.  EngineError with
        code OH_E_UNSUPPORTED for any other matrix"""
        out = np.zeros((3, 4096), dtype=np.uint16)
        r = self.as_struct()
        _check(lib().oh_remap_luts(C.byref(r), out.ctypes.data_as(C.c_void_p)), "oh_remap_luts")
        return out[:, :1 << self.in_bit_depth].copy()

    def sample(self, s):
        """oh_remap_sample (host only): the three output components of the source sample s"""
        r = self.as_struct()
        o = (C.c_uint16 * 3)()
        rc = lib().oh_remap_sample(C.byref(r), (C.c_uint16 * 3)(*[int(v) for v in s]), o)
        _check(rc, "oh_remap_sample", failed=rc != 1, text="{what} refused the remap")
        return tuple(o)


def remap_curve(in_bit_depth, out_bit_depth, pivots=()):
    """oh_remap_curve (host only): the piecewise-linear table of 2^in_bit_depth entries through pivots, up to 33 pairs (coded, target)
    with strictly increasing coded values; (0, 0) and (2^in - 1, 2^out - 1) are added where the pivots do not reach the ends"""
    pv = [(int(x), int(y)) for x, y in pivots]
    if any(not (0 <= x <= 0xFFFF and 0 <= y <= 0xFFFF) for x, y in pv):
        raise ValueError("remap_curve: a pivot is two values of 16 bits")
    n = len(pv)
    coded, target = (C.c_uint16 * max(n, 1))(*[x for x, _ in pv]), (C.c_uint16 * max(n, 1))(*[y for _, y in pv])
    out = np.zeros(1 << in_bit_depth if 0 <= in_bit_depth <= 12 else 1, dtype=np.uint16)
    _check(lib().oh_remap_curve(int(in_bit_depth), int(out_bit_depth), n, coded, target, out.ctypes.data_as(C.POINTER(C.c_uint16))),
           "oh_remap_curve")
    return out


def make_remap(pre, coeff, log2_denom, post, in_bit_depth, out_bit_depth=None):
    """a Remap from its parts.  pre / post: None (the curve without pivots: a rescaling from depth to depth), one table or list of
    pivots for all three components, or a sequence of three of these; a list of pivots goes through remap_curve.  coeff: None for the
    identity (2^log2_denom on the diagonal, so log2_denom up to 14: 2^15 is no coefficient), or three rows of three integers"""
    bi = int(in_bit_depth)
    bo = bi if out_bit_depth is None else int(out_bit_depth)

    def one(t, b):
        t = np.zeros(0) if t is None else np.asarray(t)
        return remap_curve(b, bo, t) if t.size == 0 or (t.ndim == 2 and t.shape[1] == 2) else t

    def three(t, b):
        # three of them: None, pivot lists (two dimensions) or tables (one dimension, and not the two entries of one pivot)
        apart = t is not None and len(t) == 3 and all(x is None or np.ndim(x) == 2 or (np.ndim(x) == 1 and len(x) != 2) for x in t)
        return np.stack([one(x, b) for x in (t if apart else [t] * 3)])

    k = np.eye(3, dtype=np.int64) << int(log2_denom) if coeff is None else coeff
    return Remap(three(pre, bi), k, log2_denom, three(post, bo), bi, bo)


def remap_from_sei(sei):
    """oh_remap_from_sei (host only): the dict of annexb.colour_remap (or an annexb.OhColourRemapSei) -> the Remap of its six curves and
    its matrix (absent: the identity).  EngineError with code OH_E_UNSUPPORTED for a depth other than 8, 9, 10 or 12, OH_E_ARG for a
    cancelled message or pivots that are no curve.  The signal info describes the result and changes no sample."""
    from . import annexb as A
    if sei is None:
        raise ValueError("remap_from_sei: no message")
    s = sei if isinstance(sei, A.OhColourRemapSei) else A.colour_remap_to_struct(sei)
    t = np.zeros((6, 4096), dtype=np.uint16)
    r = OhRemap()
    _check(lib().oh_remap_from_sei(C.byref(s), t.ctypes.data_as(C.c_void_p), C.byref(r)), "oh_remap_from_sei")
    k = [[r.coeff[c][i] for i in range(3)] for c in range(3)]
    return Remap(t[:3, :1 << r.in_bit_depth], k, r.log2_denom, t[3:, :1 << r.out_bit_depth], r.in_bit_depth, r.out_bit_depth)


class OhPacking(C.Structure):                                 # include/ohevc_hip.h
    _fields_ = [("arrangement", C.c_int32), ("quincunx", C.c_int32), ("flip", C.c_int32 * 2), ("grid_x", C.c_int32 * 2),
                ("grid_y", C.c_int32 * 2), ("content_interpretation", C.c_int32)]


PACK_ARRANGEMENTS = {"side_by_side": 3, "top_bottom": 4}      # OH_PACK_SIDE_BY_SIDE, OH_PACK_TOP_BOTTOM
PACK_MAX_PICS = 32                                            # OH_PK_MAX_PICS: packed pictures of one launch


class Packing:
    """what Engine.pics_unpack / pics_pack take (OhPacking): arrangement (3 side by side, 4 top-bottom), quincunx, flip (view 0, view 1:
    stored mirrored), grid ((x, y) of view 0, (x, y) of view 1, each 0 .. 15) and content_interpretation"""
    __slots__ = ("arrangement", "quincunx", "flip", "grid", "content_interpretation")

    def __init__(self, arrangement, quincunx=False, flip=(False, False), grid=((0, 0), (0, 0)), content_interpretation=0):
        self.arrangement = _enum(PACK_ARRANGEMENTS, "arrangement", arrangement)
        self.quincunx = bool(quincunx)
        self.flip = (bool(flip[0]), bool(flip[1]))
        self.grid = ((int(grid[0][0]), int(grid[0][1])), (int(grid[1][0]), int(grid[1][1])))
        self.content_interpretation = int(content_interpretation)

    def __repr__(self):
        return (f"Packing(arrangement={self.arrangement}, quincunx={self.quincunx}, flip={self.flip}, grid={self.grid}, "
                f"content_interpretation={self.content_interpretation})")

    def as_struct(self):
        pk = OhPacking(self.arrangement, int(self.quincunx))
        for v in range(2):
            pk.flip[v] = int(self.flip[v])
            pk.grid_x[v], pk.grid_y[v] = self.grid[v]
        pk.content_interpretation = self.content_interpretation
        return pk

    def view_size(self, params, full=True):
        """oh_packing_view_size (host only): the OhPicParams of a view of packed pictures of `params`, of full or half size"""
        pk, vp = self.as_struct(), F.OhPicParams()
        _check(lib().oh_packing_view_size(C.byref(pk), C.byref(params), int(bool(full)), C.byref(vp)), "oh_packing_view_size")
        return vp

    def views(self):
        """oh_packing_views (host only): (left, right), the constituent frames that are the left and the right view, or None where
        the content interpretation does not say"""
        pk, left, right = self.as_struct(), C.c_int(), C.c_int()
        return (left.value, right.value) if lib().oh_packing_views(C.byref(pk), C.byref(left), C.byref(right)) else None

    def sample(self, params, plane_samples, view, plane, x, y, full=True):
        """oh_packing_sample (host only): sample (x, y) of plane `plane` of view `view` from plane_samples, that plane of the packed
        picture as a numpy array (uint8 at 8 bit, else uint16)"""
        a = np.ascontiguousarray(plane_samples, dtype=np.uint8 if params.bit_depth == 8 else np.uint16)
        pk, out = self.as_struct(), C.c_int32()
        _check(lib().oh_packing_sample(C.byref(pk), C.byref(params), int(bool(full)), int(view), int(plane), int(x), int(y),
                                       a.ctypes.data_as(C.c_void_p), a.shape[1], C.byref(out)), "oh_packing_sample")
        return out.value

    def pack_sample(self, params, view0, view1, plane, x, y):
        """oh_packing_pack_sample (host only): sample (x, y) of plane `plane` of the packed picture of `params` from that plane of
        the two views, numpy arrays of one shape"""
        dt = np.uint8 if params.bit_depth == 8 else np.uint16
        a0, a1 = np.ascontiguousarray(view0, dtype=dt), np.ascontiguousarray(view1, dtype=dt)
        if a0.shape != a1.shape:
            raise ValueError("pack_sample: the planes of the two views are of one shape")
        pk, out = self.as_struct(), C.c_int32()
        _check(lib().oh_packing_pack_sample(C.byref(pk), C.byref(params), int(plane), int(x), int(y), a0.ctypes.data_as(C.c_void_p),
                                            a1.ctypes.data_as(C.c_void_p), a0.shape[1], C.byref(out)), "oh_packing_pack_sample")
        return out.value


def make_packing(arrangement, *, quincunx=False, flip=(False, False), grid=((0, 0), (0, 0)), content_interpretation=0):
    """a Packing from its parts.  arrangement: "side_by_side", "top_bottom" or the arrangement type (3, 4)"""
    return Packing(arrangement, quincunx, flip, grid, content_interpretation)


def packing_from_sei(sei):
    """oh_packing_from_sei (host only): the dict of annexb.frame_packing (or an annexb.OhFramePackingSei) -> the Packing.  EngineError
    with code OH_E_UNSUPPORTED and the reason for temporal interleaving, an arrangement type that HEVC does not define and field
    views; OH_E_ARG for a cancelled message."""
    from . import annexb as A
    if sei is None:
        raise ValueError("packing_from_sei: no message")
    s = sei if isinstance(sei, A.OhFramePackingSei) else A.frame_packing_to_struct(sei)
    pk = OhPacking()
    rc = lib().oh_packing_from_sei(C.byref(s), C.byref(pk))
    why = lib().oh_packing_unsupported(C.byref(s)).decode()
    _check(rc, "oh_packing_from_sei", text="{what} failed ({rc})" + (": " + why if why else ""))
    return Packing(pk.arrangement, pk.quincunx, tuple(pk.flip), ((pk.grid_x[0], pk.grid_y[0]), (pk.grid_x[1], pk.grid_y[1])),
                   pk.content_interpretation)


def convert_image_bytes(params, cv):
    """oh_convert_image_bytes (host only): bytes of one image, 0 when the combination is not valid"""
    return int(lib().oh_convert_image_bytes(C.byref(params), C.byref(cv)))


def convert_coeffs(cv, bit_depth):
    """oh_convert_coeffs (host only): (cy, crv, cgu, cgv, cbu, yoff, mid, S, D), the integers of an RGB conversion"""
    out = (C.c_int32 * CONV_NCOEFFS)()
    _check(lib().oh_convert_coeffs(C.byref(cv), bit_depth, out, CONV_NCOEFFS), "oh_convert_coeffs")
    return tuple(out)


def import_coeffs(cv, bit_depth):
    """oh_import_coeffs (host only): (ry, gy, by, ru, gu, bu, rv, gv, bv, yoff, mid, S, D), the integers of an RGB import"""
    out = (C.c_int32 * IMPORT_NCOEFFS)()
    _check(lib().oh_import_coeffs(C.byref(cv), bit_depth, out, IMPORT_NCOEFFS), "oh_import_coeffs")
    return tuple(out)


def lib_path():
    return os.path.join(F.PKG_DIR, "libohevc_hip.so")


def build():
    subprocess.check_call(["make", "-s", "-C", F.PKG_DIR, "libohevc_hip.so", "libohevc_host.so"])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(lib_path()):
            raise EngineError("libohevc_hip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        global _torch_first
        # torch's HIP libraries link the runtime as libamdhip64.so, this library as libamdhip64.so.7: loaded after this library, torch
        # brings a second HIP runtime that sees no GPU.  Loaded before it, both share torch's (what Engine.pics_convert needs).
        _torch_first = "torch" in sys.modules
        L = C.CDLL(lib_path())
        V, I, I64 = C.c_void_p, C.c_int, C.c_int64
        PP, IP, U16P = C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_uint16)
        WP, HP, MVP = C.POINTER(OhWarp), C.POINTER(OhPlaneHist), C.POINTER(OhMotionVector)
        L.oh_engine_create.argtypes = [PP, I]
        L.oh_engine_create_on_stream.argtypes = [PP, I, V]
        L.oh_pic_bytes.argtypes = [C.POINTER(F.OhPicParams)]
        L.oh_pic_bytes.restype = C.c_size_t
        L.oh_pic_wrap.argtypes = [V, C.POINTER(F.OhPicParams), V, V, C.c_size_t, C.POINTER(I)]
        L.oh_pic_final_half.argtypes = [V, I]
        L.oh_pic_set_final_half.argtypes = [V, I, I]
        L.oh_engine_destroy.argtypes = [V]
        L.oh_engine_destroy.restype = None
        L.oh_engine_last_error.argtypes = [V]
        L.oh_engine_last_error.restype = C.c_char_p
        L.oh_engine_sync.argtypes = [V]
        L.oh_pic_alloc.argtypes = [V, C.POINTER(F.OhPicParams), C.POINTER(I)]
        L.oh_pic_free.argtypes = [V, I]
        L.oh_pic_upload.argtypes = [V, I, C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t)]
        L.oh_pic_download.argtypes = [V, I, C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t)]
        L.oh_pic_download_window.argtypes = [V, I, C.POINTER(OhWindow), C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t)]
        L.oh_pic_download_start.argtypes = [V, I, C.POINTER(OhWindow), C.POINTER(C.c_void_p)]
        L.oh_download_finish.argtypes = [V, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ssize_t)]
        L.oh_pic_upsample_ctbs.argtypes = [V, I, I, C.c_void_p, I, C.POINTER(C.c_uint32), I]
        L.oh_pic_upsample_blocks.argtypes = [V, I, I, C.c_void_p, I, C.POINTER(OhWindow), C.POINTER(C.c_uint32), I]
        L.oh_upsample_blocks_defined.argtypes = [C.c_void_p, I, I, I, I, I, C.POINTER(I)]
        L.oh_pics_md5.argtypes = [V, C.POINTER(C.c_int), I, C.POINTER(C.c_uint8)]
        L.oh_pics_hash.argtypes = [V, C.POINTER(C.c_int), I, I, C.POINTER(OhPictureHash)]
        L.oh_pics_convert.argtypes = [V, C.POINTER(C.c_int), I, C.POINTER(OhConvert), V, C.c_size_t, C.c_size_t]
        L.oh_convert_image_bytes.argtypes = [C.POINTER(F.OhPicParams), C.POINTER(OhConvert)]
        L.oh_convert_image_bytes.restype = C.c_size_t
        L.oh_convert_coeffs.argtypes = [C.POINTER(OhConvert), I, C.POINTER(C.c_int32), I]
        L.oh_pics_import.argtypes = [V, C.POINTER(C.c_int), I, C.POINTER(OhConvert), V, C.c_size_t, C.c_size_t]
        L.oh_import_coeffs.argtypes = [C.POINTER(OhConvert), I, C.POINTER(C.c_int32), I]
        L.oh_pics_convert_colour.argtypes = [V, C.POINTER(C.c_int), I, C.POINTER(OhConvert), C.POINTER(OhColour), V, C.c_size_t, C.c_size_t]
        L.oh_colour_tables.argtypes = [C.POINTER(OhColour)] + [C.POINTER(C.c_int32)] * 4
        L.oh_pics_light_level.argtypes = [V, C.POINTER(C.c_int), I, C.POINTER(OhConvert), C.POINTER(OhLightSpec), C.POINTER(OhLightLevel)]
        L.oh_light_bin.argtypes = [C.c_uint32]
        L.oh_light_bin_upper.argtypes = [I]
        L.oh_light_bin_upper.restype = C.c_uint32
        L.oh_light_percentile.argtypes = [C.POINTER(OhLightLevel), I, C.c_uint32, C.POINTER(C.c_uint32)]
        L.oh_pics_compare.argtypes = [V, C.POINTER(C.c_int), C.POINTER(C.c_int), I, C.POINTER(OhCompareSpec), C.POINTER(OhCompare)]
        L.oh_compare_ssim_consts.argtypes = [I, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.oh_compare_ssim_window.argtypes = [I, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
        L.oh_compare_ssim_window.restype = C.c_int64
        L.oh_compare_psnr.argtypes = [C.c_uint64, C.c_uint64, I]
        L.oh_compare_psnr.restype = C.c_double
        L.oh_pics_compose.argtypes = [V, C.POINTER(C.c_int), I, C.POINTER(OhCompose)]
        L.oh_compose_blend.argtypes = [C.c_uint32] * 4
        L.oh_compose_blend.restype = C.c_uint32
        L.oh_compose_chroma_alpha.argtypes = [I] + [C.c_uint32] * 4
        L.oh_compose_chroma_alpha.restype = C.c_uint32
        L.oh_pics_reformat.argtypes = [V, C.POINTER(C.c_int), C.POINTER(C.c_int), I, C.POINTER(OhReformat)]
        L.oh_reformat_quantise.argtypes = [C.c_int32, I, I, I, I, I]
        L.oh_reformat_quantise.restype = C.c_int32
        L.oh_pics_orient.argtypes = [V, C.POINTER(C.c_int), C.POINTER(C.c_int), I, C.POINTER(OhOrient)]
        L.oh_orient_then.argtypes = [I, I]
        L.oh_orient_inverse.argtypes = [I]
        L.oh_orient_size.argtypes = [I, I, I, C.POINTER(I), C.POINTER(I)]
        L.oh_orient_from_sei.argtypes = [I, I, C.c_uint32, C.POINTER(I)]
        L.oh_pics_warp.argtypes = [V, IP, IP, I, WP]
        L.oh_warp_position.argtypes = [WP, I, I, I, I, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.oh_warp_cubic.argtypes = [I, C.POINTER(C.c_int16)]
        L.oh_warp_interp.argtypes = [C.POINTER(C.c_uint16), I, I, I, I]
        L.oh_warp_interp.restype = C.c_int32
        L.oh_warp_paths.argtypes = [WP, I, I, I, I, C.POINTER(I64), C.POINTER(I64)]
        L.oh_warp_identity.argtypes = [WP]
        L.oh_warp_translation.argtypes = [C.c_int32, C.c_int32, WP]
        L.oh_warp_then.argtypes = [WP, WP, WP]
        L.oh_warp_invert.argtypes = [WP, WP]
        L.oh_warp_rotation.argtypes = [C.c_uint32, I64, I64, I64, I64, C.c_int32, WP]
        L.oh_warp_from_sei.argtypes = [I, I, C.c_uint32, I, I, WP, IP, IP]
        L.oh_field_info.argtypes = [I, C.POINTER(OhFieldInfo)]
        L.oh_pics_weave.argtypes = [V, IP, IP, IP, I]
        L.oh_pics_separate.argtypes = [V, IP, IP, IP, I]
        L.oh_pics_deinterlace.argtypes = [V, IP, IP, IP, IP, I, C.POINTER(OhDeinterlace)]
        L.oh_deint_adaptive.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)] + [C.c_int32] * 6
        L.oh_deint_adaptive.restype = C.c_int32
        L.oh_pics_filter.argtypes = [V, IP, IP, IP, IP, I, C.POINTER(OhFilter)]
        L.oh_filter_taps_check.argtypes = [C.POINTER(OhFilterTaps)]
        L.oh_filter_binomial.argtypes = [I, C.POINTER(C.c_int16)]
        L.oh_filter_box.argtypes = [I, C.POINTER(C.c_int16)]
        L.oh_filter_unsharp.argtypes = [C.c_int32] * 5
        L.oh_filter_unsharp.restype = C.c_int32
        L.oh_filter_median9.argtypes = [C.POINTER(C.c_int32)]
        L.oh_filter_median9.restype = C.c_int32
        L.oh_filter_temporal.argtypes = [C.c_int32] * 6
        L.oh_filter_temporal.restype = C.c_int32
        L.oh_pics_histogram.argtypes = [V, IP, I, C.POINTER(OhWindow), C.POINTER(OhHistogram)]
        L.oh_hist_percentile.argtypes = [HP, I, C.c_uint32, C.POINTER(C.c_uint32)]
        L.oh_hist_distance.argtypes = [HP, HP, C.POINTER(C.c_uint64)]
        L.oh_pics_lut.argtypes = [V, IP, IP, I, C.POINTER(OhLut)]
        L.oh_lut_identity.argtypes = [I, I, U16P]
        L.oh_lut_range.argtypes = [I, I, I, I, U16P]
        L.oh_lut_linear.argtypes = [I, I, C.c_int32, C.c_int32, C.c_int32, U16P]
        L.oh_lut_stretch.argtypes = [HP, I, C.c_uint32, C.c_uint32, I, U16P]
        L.oh_lut_equalise.argtypes = [HP, I, I, U16P]
        L.oh_lut_then.argtypes = [U16P, I, U16P, I, U16P]
        U32, I32, U32P = C.c_uint32, C.c_int32, C.POINTER(C.c_uint32)
        L.oh_pics_grain.argtypes = [V, IP, IP, I, C.POINTER(OhGrain), U32P]
        L.oh_grain_hash.argtypes = [U32] * 4
        L.oh_grain_hash.restype = U32
        L.oh_grain_gauss.argtypes = [U32]
        L.oh_grain_gauss.restype = I32
        L.oh_grain_pattern.argtypes = [I, I, C.POINTER(C.c_int16), C.POINTER(C.c_int16), C.POINTER(C.c_int8)]
        L.oh_grain_uniform.argtypes = [I, I, I, U32P]
        L.oh_grain_from_sei.argtypes = [V, V, C.POINTER(OhGrain)]
        L.oh_grain_block.argtypes = [U32, I, I, I, IP, IP, IP]
        L.oh_grain_mean.argtypes = [U32, I, I]
        L.oh_grain_mean.restype = I32
        L.oh_grain_value.argtypes = [I32, I32, I, I]
        L.oh_grain_value.restype = I32
        L.oh_grain_smooth.argtypes = [I32] * 3
        L.oh_grain_smooth.restype = I32
        L.oh_grain_blend.argtypes = [I32, I32, I, I]
        L.oh_grain_blend.restype = I32
        RP = C.POINTER(OhRemap)
        L.oh_pics_colour_remap.argtypes = [V, IP, IP, I, RP]
        L.oh_remap_curve.argtypes = [I, I, I, U16P, U16P, U16P]
        L.oh_remap_sample.argtypes = [RP, U16P, U16P]
        L.oh_remap_from_sei.argtypes = [V, V, RP]
        L.oh_remap_luts.argtypes = [RP, V]
        PKP = C.POINTER(OhPacking)
        L.oh_pics_unpack.argtypes = [V, IP, IP, IP, I, PKP]
        L.oh_pics_pack.argtypes = [V, IP, IP, IP, I, PKP]
        L.oh_packing_from_sei.argtypes = [V, PKP]
        L.oh_packing_unsupported.argtypes = [V]
        L.oh_packing_unsupported.restype = C.c_char_p
        L.oh_packing_view_size.argtypes = [PKP, C.POINTER(F.OhPicParams), I, C.POINTER(F.OhPicParams)]
        L.oh_packing_sample.argtypes = [PKP, C.POINTER(F.OhPicParams), I, I, I, I, I, V, I, C.POINTER(I32)]
        L.oh_packing_pack_sample.argtypes = [PKP, C.POINTER(F.OhPicParams), I, I, I, V, V, I, C.POINTER(I32)]
        L.oh_packing_views.argtypes = [PKP, IP, IP]
        L.oh_motion_blocks.argtypes = [I, I, I, IP, IP]
        L.oh_pics_motion.argtypes = [V, IP, IP, I, C.POINTER(OhMotionSearch), MVP]
        L.oh_pics_motion_compensate.argtypes = [V, IP, IP, I, I, MVP]
        L.oh_motion_scale.argtypes = [MVP, I, I, I, I, I, I, I, C.POINTER(C.c_int16)]
        L.oh_motion_qpel.argtypes = [U16P, I, I, I]
        L.oh_motion_qpel.restype = C.c_int32
        L.oh_motion_epel.argtypes = [U16P, I, I, I]
        L.oh_motion_epel.restype = C.c_int32
        L.oh_motion_cost.argtypes = [C.c_uint32, I, I, I, I, I]
        L.oh_motion_cost.restype = C.c_uint64
        L.oh_pics_resize.argtypes = [V, C.POINTER(C.c_int), C.POINTER(C.c_int), I, C.POINTER(OhResize)]
        L.oh_resize_taps.argtypes = [I, I, I, I, C.POINTER(C.c_int32), C.POINTER(C.c_int16), I, C.POINTER(C.c_int)]
        L.oh_resize_max_taps.argtypes = [I, I, I]
        L.oh_frame_upload.argtypes = [V, C.POINTER(F.OhFrame), PP]
        L.oh_frames_upload.argtypes = [V, C.POINTER(C.POINTER(F.OhFrame)), I, PP]
        L.oh_frame_execute.argtypes = [V, V]
        L.oh_pic_upsample.argtypes = [V, C.c_int, C.c_int, V]
        L.oh_frames_execute.argtypes = [V, C.POINTER(C.c_void_p), C.c_int]
        L.oh_frame_free.argtypes = [V, V]
        L.oh_frame_release.argtypes = [V, V]
        L.oh_frame_download_bs.argtypes = [V, V, V, V, C.c_size_t]
        L.oh_frame_submit.argtypes = [V, C.POINTER(F.OhFrame)]
        L.oh_engine_profile.argtypes = [V, I]
        L.oh_engine_pass_times.argtypes = [V, C.POINTER(C.c_double), C.POINTER(C.c_uint64), I]
        L.oh_engine_intra_launch_times.argtypes = [V, C.POINTER(C.c_double), C.POINTER(C.c_uint64), I]
        L.oh_engine_host_times.argtypes = [V, C.POINTER(C.c_double), C.POINTER(C.c_uint64), I, I]
        L.oh_engine_memory.argtypes = [V, C.POINTER(C.c_uint64)]
        L.oh_engine_upload_bytes.argtypes = [V, I]
        L.oh_engine_upload_bytes.restype = C.c_uint64
        L.oh_engine_stream.argtypes = [V]
        L.oh_engine_stream.restype = V
        L.oh_host_alloc.argtypes = [C.c_size_t]
        L.oh_host_alloc.restype = V
        L.oh_host_free.argtypes = [V]
        L.oh_host_free.restype = None
        L.oh_pic_device_planes.argtypes = [V, I, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _lib = L
    return _lib


def upsample_blocks_defined(u, w_bl, h_bl, w_el, h_el, log2_ctb_size):
    """oh_upsample_blocks_defined (host only, no GPU): (True, -1) when the reference's CTB up-sampling path defines every CTB of the
    enhancement-layer picture, else (False, first CTB address that reads samples no call of its own wrote; -1: scale out of range)"""
    bad = C.c_int(-1)
    rc = lib().oh_upsample_blocks_defined(C.byref(u), w_bl, h_bl, w_el, h_el, log2_ctb_size, C.byref(bad))
    if rc < 0:
        raise EngineError(f"oh_upsample_blocks_defined: bad geometry ({rc})")
    return rc == 1, bad.value


class Engine:
    def __init__(self, device=0, stream=None):
        """stream: optional hipStream_t handle (int), e.g. torch.cuda.current_stream().cuda_stream"""
        self.L = lib()
        h = C.c_void_p()
        if stream is None:
            rc = self.L.oh_engine_create(C.byref(h), device)
        else:
            rc = self.L.oh_engine_create_on_stream(C.byref(h), device, C.c_void_p(stream))
        if rc != 0:
            raise EngineError(f"oh_engine_create(device={device}) failed with {rc}: no usable MI355X / HIP device")
        self.h = h
        self.device = device
        self._torch_stream = None
        self._params = {}                                     # picture id -> its OhPicParams (the image shapes of pics_convert)

    def _chk(self, rc, what):
        if rc != 0:
            _check(rc, f"{what} failed ({rc}): {self.L.oh_engine_last_error(self.h).decode()}", text="{what}")

    def close(self):
        if getattr(self, "h", None):
            self.L.oh_engine_destroy(self.h)
            self.h = None
            self._torch_stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self.L.oh_engine_sync(self.h), "oh_engine_sync")

    # ---- pictures ----
    def pic_alloc(self, params):
        pid = C.c_int(-1)
        self._chk(self.L.oh_pic_alloc(self.h, C.byref(params), C.byref(pid)), "oh_pic_alloc")
        self._params[pid.value] = F.OhPicParams.from_buffer_copy(params)
        return pid.value

    def pic_wrap(self, params, half0_ptr, half1_ptr, half_bytes):
        pid = C.c_int(-1)
        self._chk(self.L.oh_pic_wrap(self.h, C.byref(params), C.c_void_p(half0_ptr), C.c_void_p(half1_ptr), half_bytes,
                                     C.byref(pid)), "oh_pic_wrap")
        self._params[pid.value] = F.OhPicParams.from_buffer_copy(params)
        return pid.value

    def pic_final_half(self, pid):
        r = self.L.oh_pic_final_half(self.h, pid)
        if r < 0:
            raise EngineError(f"oh_pic_final_half({pid}) failed")
        return r

    def pic_set_final_half(self, pid, half):
        self._chk(self.L.oh_pic_set_final_half(self.h, pid, half), "oh_pic_set_final_half")

    def pic_free(self, pid):
        self._chk(self.L.oh_pic_free(self.h, pid), "oh_pic_free")
        self._params.pop(pid, None)

    @staticmethod
    def _plane_args(planes, params=None, window=(0, 0, 0, 0), pad=0):
        """(planes, their pointers, their row strides) as the plane calls take them: planes, a list of numpy planes, or with None
        zeroed planes that hold the window = (left, right, top, bottom) of a picture of params, their rows pad bytes longer"""
        if planes is None:
            dt = np.uint8 if params.bit_depth <= 8 else np.uint16
            W, H = params.width - window[0] - window[1], params.height - window[2] - window[3]
            planes = []
            for c in range(F.n_planes(params)):
                hs = 1 if c and params.chroma_format_idc in (1, 2) else 0
                vs = 1 if c and params.chroma_format_idc == 1 else 0
                planes.append(np.zeros((H >> vs, (W >> hs) + pad // dt().itemsize), dt))
        n = len(planes)
        d = (C.c_void_p * 3)(*[pl.ctypes.data for pl in planes] + [None] * (3 - n))
        s = (C.c_ssize_t * 3)(*[pl.strides[0] for pl in planes] + [0] * (3 - n))
        return planes, d, s

    def pic_upload(self, pid, hp):
        _, d, s = self._plane_args(hp.planes)
        self._chk(self.L.oh_pic_upload(self.h, pid, d, s), "oh_pic_upload")

    def pic_download(self, pid, params):
        hp = F.HostPic(params)
        _, d, s = self._plane_args(hp.planes)
        self._chk(self.L.oh_pic_download(self.h, pid, d, s), "oh_pic_download")
        return hp

    def pic_download_start(self, pid, left=0, right=0, top=0, bottom=0):
        """first half of the output fetch (oh_pic_download_start): the copies are enqueued behind the picture's batch; returns the handle
        oh_download_finish takes — on any thread, while this one keeps driving the engine"""
        d = C.c_void_p()
        win = OhWindow(left, right, top, bottom)
        self._chk(self.L.oh_pic_download_start(self.h, pid, C.byref(win), C.byref(d)), "oh_pic_download_start")
        return d

    def download_finish(self, handle, params, left=0, right=0, top=0, bottom=0, planes=True):
        """second half (oh_download_finish): waits for the copies, returns the packed planes; planes=False: hands no destination over
        (the call must return OH_E_ARG and still release the staging buffer) and returns the error code"""
        if not planes:
            return self.L.oh_download_finish(self.h, handle, None, None)
        out, d, s = self._plane_args(None, params, (left, right, top, bottom))
        self._chk(self.L.oh_download_finish(self.h, handle, d, s), "oh_download_finish")
        return out

    def pic_download_window(self, pid, params, left=0, right=0, top=0, bottom=0, pad=0):
        """the picture inside its conformance window as packed numpy planes (pad: extra bytes per destination row, to
        exercise pitches larger than the row)"""
        planes, d, s = self._plane_args(None, params, (left, right, top, bottom), pad)
        win = OhWindow(left, right, top, bottom)
        self._chk(self.L.oh_pic_download_window(self.h, pid, C.byref(win), d, s), "oh_pic_download_window")
        return [pl[:, :pl.shape[1] - pad // pl.itemsize] if pad else pl for pl in planes]

    def pics_md5(self, pids):
        """[[16-byte MD5 of plane 0, 1, 2]] of finished pictures, computed on the GPU (oh_pics_md5)"""
        n = len(pids)
        ids = _ids(pids)
        out = (C.c_uint8 * (48 * max(n, 1)))()
        self._chk(self.L.oh_pics_md5(self.h, ids, n, out), "oh_pics_md5")
        raw = bytes(out)
        return [[raw[48 * i + 16 * c:48 * i + 16 * c + 16] for c in range(3)] for i in range(n)]

    def pics_hash(self, pids, hash_type):
        """[(hash_type, [plane 0, 1, 2])] of finished pictures, computed on the GPU (oh_pics_hash): hash_type 0 MD5 (16-byte values),
        1 CRC, 2 checksum (ints) — the shape annexb.picture_hash gives for a decoded-picture-hash SEI"""
        n = len(pids)
        ids = _ids(pids)
        out = (OhPictureHash * max(n, 1))()
        self._chk(self.L.oh_pics_hash(self.h, ids, n, hash_type, out), "oh_pics_hash")
        if hash_type == 0:
            return [(0, [bytes(out[i].md5[c]) for c in range(3)]) for i in range(n)]
        return [(hash_type, list(out[i].crc if hash_type == 1 else out[i].checksum)) for i in range(n)]

    # ---- what the wrappers of the picture services share ----
    @staticmethod
    def _sized(params, width, height):
        """a copy of params with the size rounded up to the minimum coding block"""
        dp = F.OhPicParams.from_buffer_copy(params)
        mcb = 1 << dp.log2_min_cb_size
        dp.width, dp.height = -(-width // mcb) * mcb, -(-height // mcb) * mcb
        return dp

    def _alloc_like(self, params, n):
        """n fresh pictures of params; the ones already made are freed when an allocation fails"""
        out = []
        try:
            for _ in range(n):
                out.append(self.pic_alloc(params))
        except Exception:
            for made in out:
                self.pic_free(made)
            raise
        return out

    def _dsts(self, out, n, what, params):
        """the destinations of a call, (ids, the ones made for it): out listed, one for each of the n `what`, or without out n fresh
        pictures of params(), which raises where no picture can be made"""
        if out is None:
            out = self._alloc_like(params(), n)
            return out, out
        out = list(out)
        if len(out) != n:
            raise ValueError(f"out: {len(out)} pictures for {n} {what}")
        return out, []

    def _call(self, rc, what, made):
        """the return code of a service: a refusal frees the pictures made for the call and raises through _chk"""
        if rc != 0:
            for pid in made:
                self.pic_free(pid)
        self._chk(rc, what)

    def _image_call(self, call, what, pids, out, width, height, nothing):
        """a service that puts an image of width x height luma samples at the top left of its destinations: out, or fresh pictures of
        the sources' params with that size rounded up to the minimum coding block (nothing: the ValueError where none can be made).
        call(source ids, destination ids) is the library call `what`.  Returns (destination ids, dst_window), the window of the image"""
        def fitting():
            sp = self._pic_params(pids[0])
            if width < 1 or height < 1:
                raise ValueError(nothing)
            return self._sized(sp, width, height)

        out, made = self._dsts(out, len(pids), "sources", fitting)
        self._call(call(_ids(pids), _ids(out)), what, made)
        dp = self._pic_params(out[0])
        return out, (0, dp.width - width, 0, dp.height - height)

    @staticmethod
    def _around(n, prev, next):
        """the prev / next arrays of a call: None stays None (the library takes a null array), a None entry becomes -1"""
        around = []
        for name, ids in (("prev", prev), ("next", next)):
            if ids is not None:
                ids = [-1 if v is None else int(v) for v in ids]
                if len(ids) != n:
                    raise ValueError(f"{name}: {len(ids)} entries for {n} sources")
                ids = _ids(ids)
            around.append(ids)
        return around

    @contextlib.contextmanager
    def _torch_ordered(self, torch):
        """a library call that reads or writes torch's memory, ordered with torch both ways (torch None: nothing to order)"""
        dev = torch.device("cuda", self.device) if torch is not None else None
        cur = torch.cuda.current_stream(dev) if torch is not None else None
        if cur is None or (self.stream() or 0) == cur.cuda_stream:   # an engine created on torch's current stream: nothing to order
            yield
            return
        if self._torch_stream is None:
            self._torch_stream = torch.cuda.ExternalStream(self.stream() or 0, device=dev)
        es = self._torch_stream
        # the kernels that produce what the call reads are queued on torch's stream, and the allocator may hand out memory for what it
        # writes that a queued kernel still uses
        es.wait_stream(cur)
        yield
        # torch's stream waits for the call, so whatever torch does with the memory later (a free and a reuse included) is ordered
        # behind it.  No record_stream on the engine stream: the image usually outlives the engine, and the allocator would record
        # an event on the destroyed stream when the tensor is freed.
        cur.wait_stream(es)

    def pics_convert(self, pids, fmt, *, dtype=None, window=(0, 0, 0, 0), matrix=1, full_range=False, chroma="linear", out=None,
                     colour=None):
        """finished pictures -> one torch tensor on the engine's device (oh_pics_convert): fmt "planar" / "semiplanar" (N, rows, W),
        "rgb_planar" (N, 3, H, W), "rgb" / "rgba" (N, H, W, 3 | 4).  dtype: None (YUV: the stored samples, RGB: uint8), torch.uint8,
        torch.uint16 (YUV: the stored samples of a picture above 8 bit; an 8-bit picture has no uint16 YUV form and raises),
        torch.float16 or torch.float32.  window = (left, right, top, bottom), luma samples.  out: a preallocated contiguous tensor of
        that shape, dtype and device.  colour: an OhColour (make_colour) sends an RGB format through oh_pics_convert_colour: the
        source's transfer curve, tone curve, primaries and the output curve behind the matrix.  Ordered with torch both ways: the engine stream waits for torch's current
        stream before it writes, torch's current stream waits for the engine stream afterwards.  torch must have been imported before
        the first Engine was created (one HIP runtime)."""
        import torch
        if not _torch_first:
            raise EngineError("Engine.pics_convert: import torch before the first Engine is created (the engine must share torch's HIP "
                              "runtime to write into its tensors)")
        pids = list(pids)
        n = len(pids)
        fmt_i = conv_format(fmt)
        yuv = fmt_i <= CONV_FORMATS["semiplanar"]
        dev = torch.device("cuda", self.device)
        if n == 0:
            raise ValueError("pics_convert needs at least one picture (the image shape follows the pictures' params)")
        params = self._pic_params(pids[0])
        # YUV + uint16: the stored samples of a picture above 8 bit; an 8-bit picture has no uint16 YUV form (OH_E_UNSUPPORTED below)
        yuv16 = CONV_NATIVE if params.bit_depth > 8 else CONV_U16
        samples = {None: CONV_NATIVE if yuv else CONV_U8, torch.uint8: CONV_U8, torch.uint16: yuv16 if yuv else CONV_U16,
                   torch.float16: CONV_F16, torch.float32: CONV_F32}
        if dtype not in samples:
            raise ValueError(f"dtype {dtype}: one of uint8, uint16, float16, float32")
        sample = samples[dtype]
        cv = make_convert(fmt_i, sample, window, matrix, full_range, chroma)
        ib = convert_image_bytes(params, cv)
        if ib == 0:                                           # not a valid combination: the C call says why (and with which code)
            self._chk(self.L.oh_pics_convert(self.h, _ids(pids), n, C.byref(cv), None, 0, 0), "oh_pics_convert")
            raise EngineError("oh_pics_convert: invalid conversion")
        left, right, top, bottom = window
        W, H = params.width - left - right, params.height - top - bottom
        tdt = {CONV_U8: torch.uint8, CONV_U16: torch.uint16, CONV_F16: torch.float16, CONV_F32: torch.float32,
               CONV_NATIVE: torch.uint8 if params.bit_depth == 8 else torch.uint16}[sample]
        esz = torch.empty((), dtype=tdt).element_size()
        if yuv:
            shape = (n, ib // esz // W, W)
        elif fmt_i == CONV_FORMATS["rgb_planar"]:
            shape = (n, 3, H, W)
        else:
            shape = (n, H, W, 4 if fmt_i == CONV_FORMATS["rgba"] else 3)
        if out is None:
            out = torch.empty(shape, dtype=tdt, device=dev)
        elif tuple(out.shape) != shape or out.dtype != tdt or out.device != dev or not out.is_contiguous():
            raise ValueError(f"out: want a contiguous {tdt} tensor of shape {shape} on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        with self._torch_ordered(torch):
            if colour is None:
                self._chk(self.L.oh_pics_convert(self.h, _ids(pids), n, C.byref(cv), C.c_void_p(out.data_ptr()), ib,
                                                 out.numel() * esz), "oh_pics_convert")
            else:
                self._chk(self.L.oh_pics_convert_colour(self.h, _ids(pids), n, C.byref(cv), C.byref(colour),
                                                        C.c_void_p(out.data_ptr()), ib, out.numel() * esz), "oh_pics_convert_colour")
        return out

    def pics_import(self, images, fmt, *, out=None, bit_depth=None, chroma_format_idc=None, window=(0, 0, 0, 0), matrix=1, full_range=False,
                    chroma="linear"):
        """images on the engine's device -> finished engine pictures (oh_pics_import, the inverse of pics_convert): images is one
        contiguous torch tensor in the shape and dtype pics_convert returns for fmt — "planar" / "semiplanar" (N, rows, W),
        "rgb_planar" (N, 3, H, W), "rgb" / "rgba" (N, H, W, 3 | 4); uint8, uint16, float16 or float32 (YUV: uint8, or uint16 for the
        stored samples of pictures above 8 bit).  out: the pictures to fill, window = (left, right, top, bottom) of them in luma
        samples that the image fills (the image must have the window's size); the rest of their coded planes replicates the image's
        edges.  Without out, pictures of bit_depth / chroma_format_idc are allocated with the image size rounded up to the minimum
        coding block and the image at their top left.  matrix, full_range and chroma ("linear": the 1-2-1 filter of
        chroma_sample_loc_type 0, "nearest": the co-sited pixel) say how RGB becomes YCbCr.  Returns (picture ids, window), the window
        to pass to pics_convert / pic_download_window / pics_compare for the image.  Ordered with torch both ways: the engine stream
        waits for torch's current stream before it reads, torch's current stream waits for the engine stream afterwards, so the tensor
        may be freed or overwritten at once.  Does not wait on the host."""
        import torch
        if not _torch_first:
            raise EngineError("Engine.pics_import: import torch before the first Engine is created (the engine must share torch's HIP "
                              "runtime to read its tensors)")
        fmt_i = conv_format(fmt)
        yuv = fmt_i <= CONV_FORMATS["semiplanar"]
        dev = torch.device("cuda", self.device)
        if not isinstance(images, torch.Tensor) or images.device != dev or not images.is_contiguous():
            raise ValueError(f"images: want a contiguous torch tensor on {dev}")
        if images.dim() != (3 if yuv else 4) or images.shape[0] < 1:
            raise ValueError(f"images: shape {tuple(images.shape)} is not what pics_convert gives for format {fmt!r}")
        n = int(images.shape[0])

        def fitting():                                        # params of fresh pictures with the image at their top left, and its window
            nonlocal window
            if bit_depth is None or chroma_format_idc is None:
                raise ValueError("pics_import without out needs bit_depth and chroma_format_idc")
            cf = int(chroma_format_idc)
            if yuv:
                W = int(images.shape[2])
                rows = int(images.shape[1])
                # planar / semi-planar rows of W samples: H luma rows and 2 (W >> hs) (H >> vs) chroma samples
                num, den = {0: (1, 1), 1: (2, 3), 2: (1, 2), 3: (1, 3)}.get(cf, (0, 1))
                H = rows * num // den
            elif fmt_i == CONV_FORMATS["rgb_planar"]:
                H, W = int(images.shape[2]), int(images.shape[3])
            else:
                H, W = int(images.shape[1]), int(images.shape[2])
            if W < 1 or H < 1:
                raise ValueError(f"images: shape {tuple(images.shape)} holds no picture of chroma format {cf}")
            dp = self._sized(F.pic_params(8, 8, bit_depth=int(bit_depth), chroma_format_idc=cf), W, H)
            window = (0, dp.width - W, 0, dp.height - H)
            return dp

        pids, made = self._dsts(out, n, "images", fitting)
        if not made:
            window = tuple(int(v) for v in window)
        try:
            params = self._pic_params(pids[0])
            # YUV + uint16: the stored samples of a picture above 8 bit; an 8-bit picture has no uint16 YUV form (OH_E_UNSUPPORTED below)
            yuv16 = CONV_NATIVE if params.bit_depth > 8 else CONV_U16
            samples = {torch.uint8: CONV_U8, torch.uint16: yuv16 if yuv else CONV_U16, torch.float16: CONV_F16, torch.float32: CONV_F32}
            if images.dtype not in samples:
                raise ValueError(f"images: dtype {images.dtype}: one of uint8, uint16, float16, float32")
            sample = samples[images.dtype]
            if yuv and sample == CONV_U8 and params.bit_depth == 8:
                sample = CONV_NATIVE
            cv = make_convert(fmt_i, sample, window, matrix, full_range, chroma)
            esz = images.element_size()
            ib = convert_image_bytes(params, cv)
            ids = _ids(pids)
            if ib == 0:                                       # not a valid combination: the C call says why (and with which code)
                self._chk(self.L.oh_pics_import(self.h, ids, n, C.byref(cv), None, 0, 0), "oh_pics_import")
                raise EngineError("oh_pics_import: invalid import")
            if images[0].numel() * esz != ib:
                raise ValueError(f"images: {tuple(images.shape[1:])} {images.dtype} per image is {images[0].numel() * esz} bytes, the "
                                 f"window {window} of the pictures takes {ib}")
            with self._torch_ordered(torch):
                self._chk(self.L.oh_pics_import(self.h, ids, n, C.byref(cv), C.c_void_p(images.data_ptr()), ib, images.numel() * esz),
                          "oh_pics_import")
        except Exception:
            for pid in made:
                self.pic_free(pid)
            raise
        return pids, window

    def pics_light_level(self, pids, in_transfer, *, in_primaries=9, norm="maxrgb", src_peak=1000.0, window=(0, 0, 0, 0), matrix=9,
                         full_range=False, chroma="linear"):
        """light-level statistics of finished pictures, computed on the GPU (oh_pics_light_level): a LightLevel per picture over the
        norm ("maxrgb" or "luma") of every pixel's linear-light R, G, B, 2^30 = full scale (10000 nits for PQ, src_peak nits
        otherwise).  in_transfer / in_primaries / matrix are H.273 codes; window = (left, right, top, bottom), luma samples.  Waits
        for the engine stream."""
        if norm not in COL_NORM:
            raise ValueError(f"norm must be one of {sorted(COL_NORM)}, not {norm!r}")
        pids = list(pids)
        n = len(pids)
        cv = make_convert("rgb", CONV_U16, window, matrix, full_range, chroma)
        sp = OhLightSpec(int(in_transfer), int(in_primaries), COL_NORM[norm], float(src_peak))
        out = (OhLightLevel * max(n, 1))()
        self._chk(self.L.oh_pics_light_level(self.h, _ids(pids), n, C.byref(cv), C.byref(sp), out), "oh_pics_light_level")
        fs = 10000.0 if int(in_transfer) == 16 else float(src_peak)
        return [LightLevel(o.pixels, o.sum, o.max, o.min, np.frombuffer(o.hist, dtype=np.uint32).copy(), fs) for o in out[:n]]

    def pics_compare(self, a_pids, b_pids, *, window=(0, 0, 0, 0), ssim=True):
        """finished pictures compared pair by pair on the GPU (oh_pics_compare): a Compare per pair (a_pids[i], b_pids[i]) with a
        PlaneDiff per plane — differing samples, sad, sse, max_abs, the first differing sample and, with ssim, the SSIM sum over
        8x8 windows; window = (left, right, top, bottom), luma samples.  Waits for the engine stream."""
        a_pids, b_pids = list(a_pids), list(b_pids)
        n = len(a_pids)
        if len(b_pids) != n:
            raise ValueError(f"pics_compare: {n} pictures against {len(b_pids)}")
        sp = OhCompareSpec(OhWindow(*window), CMP_SSIM if ssim else 0)
        out = (OhCompare * max(n, 1))()
        self._chk(self.L.oh_pics_compare(self.h, _ids(a_pids), _ids(b_pids), n, C.byref(sp), out),
                  "oh_pics_compare")
        return [Compare(out[i], self._pic_params(a_pids[i]).bit_depth) for i in range(n)]

    def pics_resize(self, pids, size, *, window=(0, 0, 0, 0), filter="bilinear", out=None):
        """finished pictures -> resized engine pictures (oh_pics_resize): size = (width, height) of the image in luma samples, window =
        (left, right, top, bottom) of the sources in luma samples, filter "bilinear" or "bicubic" (anti-aliased when shrinking).
        out: destination pictures to reuse; None allocates pictures with the sources' params and the size rounded up to the minimum
        coding block.  Returns (destination ids, dst_window): the image is the top-left of each destination, dst_window the window to
        pass to pics_convert / pic_download_window for it.  Enqueued on the engine stream; does not wait."""
        pids = list(pids)
        n = len(pids)
        if n == 0:
            raise ValueError("pics_resize needs at least one picture (the destinations follow the pictures' params)")
        width, height = int(size[0]), int(size[1])
        rs = OhResize(resize_filter(filter), OhWindow(*window), width, height)
        return self._image_call(lambda src, dst: self.L.oh_pics_resize(self.h, src, dst, n, C.byref(rs)), "oh_pics_resize", pids, out, width, height,
                                f"size {size}: at least 1 x 1")

    def pics_reformat(self, pids, *, bit_depth=None, chroma_format_idc=None, depth="round", down="linear", up="linear", out=None):
        """finished pictures -> finished pictures of another bit depth and / or chroma format and the same size (oh_pics_reformat):
        depth "round" or "dither" (the ordered 4 x 4 dither) where bits go; down "point" or "linear" where chroma is sub-sampled
        further (the 1-2-1 filter of chroma_sample_loc_type 0), up "nearest" or "linear" where it is sub-sampled less.  out: destination
        pictures to reuse, of any depth and format; None allocates pictures with the sources' params, bit_depth / chroma_format_idc
        replaced where given.  Returns the destination ids.  Enqueued on the engine stream; does not wait."""
        pids = list(pids)
        n = len(pids)
        rf = OhReformat(_enum(RF_DEPTH, "depth mode", depth), _enum(RF_FILTERS, "down filter", down), _enum(RF_FILTERS, "up filter", up))
        if out is None and n == 0:
            return []

        def reformatted():
            dp = F.OhPicParams.from_buffer_copy(self._pic_params(pids[0]))
            if bit_depth is not None:
                dp.bit_depth = int(bit_depth)
            if chroma_format_idc is not None:
                dp.chroma_format_idc = int(chroma_format_idc)
            return dp

        out, made = self._dsts(out, n, "sources", reformatted)
        self._call(self.L.oh_pics_reformat(self.h, _ids(pids), _ids(out), n, C.byref(rf)),
                   "oh_pics_reformat", made)
        return out

    def pics_orient(self, pids, orientation, *, window=(0, 0, 0, 0), out=None):
        """finished pictures -> finished pictures that hold a window of them mirrored, turned or transposed (oh_pics_orient):
        orientation an int 0 .. 7 (any OR of ORIENT_HFLIP, ORIENT_VFLIP, ORIENT_TRANSPOSE; the transposition is applied first, then the
        horizontal, then the vertical flip) or "identity", "hflip", "vflip", "rot180", "transpose", "rot90" (clockwise), "rot270",
        "antitranspose"; window = (left, right, top, bottom) of the sources in luma samples.  out: destination pictures to reuse; None
        allocates pictures with the sources' params and the oriented size rounded up to the minimum coding block.  Returns
        (destination ids, dst_window) like pics_resize: the image is the top-left of each destination, the rest replicates its last
        column and row.  Enqueued on the engine stream; does not wait."""
        pids = list(pids)
        n = len(pids)
        if n == 0:
            raise ValueError("pics_orient needs at least one picture (the destinations follow the pictures' params)")
        code = orient_code(orientation)
        od = OhOrient(code, OhWindow(*window))
        sp = self._pic_params(pids[0])
        width, height = sp.width - od.win.left - od.win.right, sp.height - od.win.top - od.win.bottom
        if code & ORIENT_TRANSPOSE:
            width, height = height, width
        return self._image_call(lambda src, dst: self.L.oh_pics_orient(self.h, src, dst, n, C.byref(od)), "oh_pics_orient", pids, out, width, height,
                                f"window {tuple(window)} leaves nothing of {sp.width}x{sp.height}")

    def pics_warp(self, pids, matrix, size, *, mode=None, filter="bilinear", border="replicate", fill=(0, 0, 0), window=(0, 0, 0, 0), out=None):
        """finished pictures -> finished pictures resampled through an affine or perspective map (oh_pics_warp): matrix is the INVERSE
        map, destination -> source, in luma samples with (0, 0) the top-left sample of the window and of the image — an OhWarp (of
        which the map and, with mode None, the mode are taken: warp_rotation, warp_translation, warp_from_sei, ... build them), 6 or 9
        integers in the fixed-point layout of OhWarp.m, or a float 2 x 3 / 3 x 3 numpy array, which warp_matrix rounds to that layout
        (its docstring has the rounding).  size = (width, height) of the image in luma samples; mode "affine" / "perspective" or None
        (by the matrix's form); filter "nearest", "bilinear" or "bicubic" (no anti-aliasing: pics_resize scales down); border
        "replicate" or "constant" with fill = the code values per plane; window = (left, right, top, bottom) of the sources, outside
        of which nothing is read.  out: destination pictures to reuse; None allocates pictures with the sources' params and the size
        rounded up to the minimum coding block.  Returns (destination ids, dst_window) like pics_resize.  Enqueued on the engine
        stream; does not wait."""
        pids = list(pids)
        n = len(pids)
        if n == 0:
            raise ValueError("pics_warp needs at least one picture (the destinations follow the pictures' params)")
        width, height = int(size[0]), int(size[1])
        code, m = warp_matrix(matrix, mode)
        fill = [int(v) for v in fill]
        if len(fill) != 3 or any(not 0 <= v <= 0xFFFF for v in fill):
            raise ValueError(f"fill {tuple(fill)}: three code values")
        wp = OhWarp(code, _enum(WARP_FILTERS, "filter", filter, WARP_FILTERS.values()), _enum(WARP_BORDERS, "border", border, WARP_BORDERS.values()), (C.c_uint16 * 3)(*fill),
                    OhWindow(*window), width, height, (C.c_int64 * 9)(*m))
        return self._image_call(lambda src, dst: self.L.oh_pics_warp(self.h, src, dst, n, C.byref(wp)), "oh_pics_warp", pids, out, width, height,
                                f"size {size}: at least 1 x 1")

    def _of_height(self, pid, height):
        """the params of picture pid with another height; ValueError where oh_pic_alloc would refuse the height"""
        dp = F.OhPicParams.from_buffer_copy(self._pic_params(pid))
        mcb = 1 << dp.log2_min_cb_size
        if height < mcb or height % mcb:
            raise ValueError(f"a height of {height} is no multiple of the minimum coding block ({mcb}): no picture can hold it")
        dp.height = height
        return dp

    def pics_weave(self, top_pids, bottom_pids, *, out=None):
        """n pairs of finished fields -> n finished frames (oh_pics_weave): frame row 2y is row y of the top field, row 2y + 1 row y of
        the bottom field, in every plane.  out: destination pictures to reuse; None allocates pictures with the fields' params and
        twice their height.  Returns the destination ids.  Enqueued on the engine stream; does not wait."""
        top, bottom = list(top_pids), list(bottom_pids)
        n = len(top)
        if n == 0:
            raise ValueError("pics_weave needs at least one pair of fields (the destinations follow the fields' params)")
        if len(bottom) != n:
            raise ValueError(f"{n} top fields, {len(bottom)} bottom fields")
        out, made = self._dsts(out, n, "pairs of fields", lambda: self._of_height(top[0], 2 * self._pic_params(top[0]).height))
        self._call(self.L.oh_pics_weave(self.h, _ids(top), _ids(bottom), _ids(out), n), "oh_pics_weave", made)
        return out

    def pics_separate(self, pids, *, top=True, bottom=True, out=None):
        """n finished frames -> their fields (oh_pics_separate), the inverse of pics_weave: row y of the top field is frame row 2y, of
        the bottom field frame row 2y + 1.  top / bottom: which fields to make.  out: (top ids or None, bottom ids or None) to reuse;
        None allocates pictures with the frames' params and half their height (ValueError where no picture can have that height).
        Returns (top ids, bottom ids), None for a side that was not asked for.  Enqueued on the engine stream; does not wait."""
        pids = list(pids)
        n = len(pids)
        if n == 0:
            raise ValueError("pics_separate needs at least one picture (the destinations follow the pictures' params)")
        if not top and not bottom:
            raise ValueError("pics_separate: neither field asked for")
        made = []
        if out is None:                                       # the fields of both sides in one run: made or freed together
            height = self._pic_params(pids[0]).height
            if height % 2:
                raise ValueError(f"a frame of {height} rows has no two fields of one height")
            made = self._alloc_like(self._of_height(pids[0], height // 2), n * (bool(top) + bool(bottom)))
            sides = [made[:n] if top else None, made[-n:] if bottom else None]
        else:
            sides = list(out)
            if len(sides) != 2 or (sides[0] is None) != (not top) or (sides[1] is None) != (not bottom):
                raise ValueError("out: a pair (top ids, bottom ids) with None for the side that is not asked for")
            sides = [None if s is None else self._dsts(s, n, "sources", None)[0] for s in sides]
        self._call(self.L.oh_pics_separate(self.h, _ids(pids), _ids(sides[0]) if top else None, _ids(sides[1]) if bottom else None, n),
                   "oh_pics_separate", made)
        return sides[0], sides[1]

    def pics_deinterlace(self, pids, mode="adaptive", *, keep="top", kept_first=True, prev=None, next=None, out=None):
        """finished pictures whose rows alternate between two fields -> finished progressive pictures (oh_pics_deinterlace; the exact
        definitions are in include/ohevc_hip.h).  mode: "bob", "blend", "lowpass5", "adaptive" or DEINT_*; keep: "top" (rows 0, 2, ...
        are kept, parity 0) or "bottom" (parity 1), or the parity itself; kept_first: the kept field is the earlier one of its frame
        (adaptive only); prev / next: the pictures before and after each one in time (adaptive only), lists that may hold None, which
        like prev=None / next=None stands for the picture itself.  out: destination pictures to reuse; None allocates pictures with
        the sources' params.  Returns the destination ids.  Enqueued on the engine stream; does not wait."""
        pids = list(pids)
        n = len(pids)
        if n == 0:
            raise ValueError("pics_deinterlace needs at least one picture (the destinations follow the pictures' params)")
        if keep in ("top", "bottom"):
            parity = int(keep == "bottom")
        elif keep in (0, 1):
            parity = int(keep)
        else:
            raise ValueError(f"keep {keep!r}: 'top' (0) or 'bottom' (1)")
        dd = OhDeinterlace(deint_mode(mode), parity, int(bool(kept_first)))
        around = self._around(n, prev, next)
        out, made = self._dsts(out, n, "sources", lambda: self._pic_params(pids[0]))
        self._call(self.L.oh_pics_deinterlace(self.h, around[0], _ids(pids), around[1], _ids(out), n, C.byref(dd)), "oh_pics_deinterlace", made)
        return out

    def pics_filter(self, pids, mode, *, luma=None, chroma=None, amount=64, threshold=0, planes=7, prev=None, next=None, out=None):
        """finished pictures -> finished filtered pictures of the same params (oh_pics_filter; the exact definitions are in
        include/ohevc_hip.h).  mode: "convolve", "unsharp", "median", "temporal" or FILTER_*; luma / chroma: (h, v) tap lists of the
        luma plane and of both chroma planes (convolve, unsharp), None the binomial 3 x 3; amount (unsharp, in 1/64) and threshold
        (unsharp, temporal): an int for both classes or a pair (luma, chroma); planes: bit c set filters plane c, clear copies it;
        prev / next: the pictures before and after each one in time (temporal only), lists that may hold None, which like prev=None /
        next=None stands for the picture itself.  out: destination pictures to reuse; None allocates pictures with the sources'
        params.  Returns the destination ids.  Enqueued on the engine stream; does not wait."""
        pids = list(pids)
        n = len(pids)
        if n == 0:
            raise ValueError("pics_filter needs at least one picture (the destinations follow the pictures' params)")
        ff = OhFilter(filter_mode(mode), int(planes))
        for q, taps in enumerate((luma, chroma)):
            h, v = (filter_binomial(3), filter_binomial(3)) if taps is None else taps
            ff.taps[q] = filter_taps(h, v)
        for name, val, arr in (("amount", amount, ff.amount), ("threshold", threshold, ff.threshold)):
            pair = tuple(val) if hasattr(val, "__len__") else (val, val)
            if len(pair) != 2:
                raise ValueError(f"{name}: an int or a pair (luma, chroma)")
            arr[0], arr[1] = int(pair[0]), int(pair[1])
        around = self._around(n, prev, next)
        out, made = self._dsts(out, n, "sources", lambda: self._pic_params(pids[0]))
        self._call(self.L.oh_pics_filter(self.h, around[0], _ids(pids), around[1], _ids(out), n, C.byref(ff)), "oh_pics_filter", made)
        return out

    def pics_motion(self, cur, ref, block=16, range=(8, 8), subpel=2, lam=0, centres=None):
        """block-matching motion search between finished pictures on the GPU (oh_pics_motion; the exact definition is in
        include/ohevc_hip.h): per pair (cur[i], ref[i]) and luma block of `block` samples the vector, in HEVC's quarter samples, that
        predicts the block of cur from ref with the smallest (cost, d, y, x), cost = SAD + ((lam d) >> 2).  range = (x, y) integer
        samples either side of the centre, subpel 0 integer / 1 half / 2 quarter, centres: None or the int16 (cx, cy) per pair and block,
        shape (n, bh, bw, 2).  Returns a numpy structured array of shape (n, bh, bw) with the fields x, y, sad, sad_centre.  Waits for
        the engine stream."""
        cur, ref = list(cur), list(ref)
        n = len(cur)
        if len(ref) != n:
            raise ValueError(f"pics_motion: {n} pictures against {len(ref)}")
        ms = OhMotionSearch(int(block), int(range[0]), int(range[1]), int(subpel), int(lam))
        bw = bh = 0
        if n and cur[0] in self._params and int(block) in (8, 16):
            p = self._pic_params(cur[0])
            bw, bh = motion_blocks(p.width, p.height, block)
        if centres is not None:
            c = np.asarray(centres)
            if c.shape != (n, bh, bw, 2) or c.dtype.kind not in "iu":
                raise ValueError(f"pics_motion: centres of shape {c.shape}, not {(n, bh, bw, 2)} integers")
            if c.size and (c.min() < -32768 or c.max() > 32767):
                raise ValueError("pics_motion: a centre component is an int16")
            c = np.ascontiguousarray(c, dtype=np.int16)
            # without pairs there is nothing to read, but a non-null pointer all the same
            ms.centres = (c if c.size else np.zeros(2, np.int16)).ctypes.data_as(C.POINTER(C.c_int16))
        out = np.zeros((n, bh, bw), dtype=MOTION_DTYPE)
        buf = out if out.size else np.zeros(1, dtype=MOTION_DTYPE)
        self._chk(self.L.oh_pics_motion(self.h, _ids(cur), _ids(ref), n, C.byref(ms), buf.ctypes.data_as(C.POINTER(OhMotionVector))), "oh_pics_motion")
        return out

    def pics_motion_compensate(self, ref, field, block=16, out=None):
        """finished pictures -> their motion-compensated predictions, finished pictures of the same params (oh_pics_motion_compensate;
        the exact definition is in include/ohevc_hip.h): luma block (bx, by) of destination i is ref[i] displaced by field[i, by, bx]
        with HEVC's luma interpolation, its chroma by the same vector with the chroma interpolation.  field: what pics_motion returned,
        or an integer array (n, bh, bw, 2) of (x, y) in quarter luma samples.  out: destination pictures to reuse; None allocates
        pictures with the sources' params.  Returns the destination ids.  Enqueued on the engine stream; does not wait; the field may
        be changed at once."""
        ref = list(ref)
        n = len(ref)
        if n == 0:
            raise ValueError("pics_motion_compensate needs at least one picture (the destinations follow the pictures' params)")
        f = motion_field(field)
        if int(block) in (8, 16):
            p = self._pic_params(ref[0])
            bw, bh = motion_blocks(p.width, p.height, block)
            if f.shape != (n, bh, bw):
                raise ValueError(f"pics_motion_compensate: a field of shape {f.shape}, not {(n, bh, bw)}")
        out, made = self._dsts(out, n, "sources", lambda: self._pic_params(ref[0]))
        buf = f if f.size else np.zeros(1, dtype=MOTION_DTYPE)
        self._call(self.L.oh_pics_motion_compensate(self.h, _ids(ref), _ids(out), n, int(block), buf.ctypes.data_as(C.POINTER(OhMotionVector))),
                   "oh_pics_motion_compensate", made)
        return out

    def pics_histogram(self, pids, *, window=(0, 0, 0, 0)):
        """the code values of finished pictures counted on the GPU (oh_pics_histogram): a Histogram per picture with a PlaneHist per
        plane — samples, sum, sum_sq, min, max, mean, variance and hist, the uint32 counts of the 2^bit_depth values; window = (left,
        right, top, bottom), luma samples.  Waits for the engine stream."""
        pids = list(pids)
        n = len(pids)
        win = OhWindow(*window)
        out = (OhHistogram * max(n, 1))()
        self._chk(self.L.oh_pics_histogram(self.h, _ids(pids), n, C.byref(win), out), "oh_pics_histogram")
        return [Histogram(out[i], self._pic_params(pids[i]).bit_depth) for i in range(n)]

    def pics_lut(self, pids, tables, *, planes=None, bit_depth=None, out=None):
        """finished pictures -> finished pictures of the same size and chroma format whose samples went through a table
        (oh_pics_lut): dst = table[src].  tables: one array of 2^(source bit depth) values, which goes to every selected plane, or a
        sequence of up to three, one per plane, where None means that the plane is copied; planes: bit c set sends plane c through its
        table (None: every plane that has one).  out: destination pictures to reuse, of any bit depth that holds the tables' values;
        None allocates pictures with the sources' params, bit_depth replaced where given.  Returns the destination ids.  Enqueued on
        the engine stream; does not wait; the tables may be changed at once."""
        pids = list(pids)
        n = len(pids)
        one = not isinstance(tables, (list, tuple)) or len(tables) > 3 or any(t is not None and not hasattr(t, "__len__") for t in tables)
        per_plane = [tables] * 3 if one else (list(tables) + [None] * 3)[:3]
        per_plane = [None if t is None else np.asarray(t) for t in per_plane]
        if any(t is not None and (t.ndim != 1 or (t.size and (t.min() < 0 or t.max() > 0xFFFF))) for t in per_plane):
            raise ValueError("pics_lut: a table has one dimension and values of 16 bits")
        per_plane = [None if t is None else np.ascontiguousarray(t, dtype=np.uint16) for t in per_plane]
        sizes = {t.size for t in per_plane if t is not None}
        if len(sizes) > 1:
            raise ValueError(f"pics_lut: tables of {sorted(sizes)} entries in one call")
        if planes is None:
            planes = sum(1 << c for c, t in enumerate(per_plane) if t is not None)
        # without any table (every plane copied) the entries are those of the sources' depth, which the library asks for all the same
        lut = OhLut(int(planes), sizes.pop() if sizes else 1 << self._pic_params(pids[0]).bit_depth if n else 0)
        for c, t in enumerate(per_plane):
            if t is not None:
                lut.table[c] = t.ctypes.data_as(C.POINTER(C.c_uint16))
        if out is None and n == 0:
            return []

        def with_depth():
            dp = F.OhPicParams.from_buffer_copy(self._pic_params(pids[0]))
            if bit_depth is not None:
                dp.bit_depth = int(bit_depth)
            return dp

        out, made = self._dsts(out, n, "sources", with_depth)
        self._call(self.L.oh_pics_lut(self.h, _ids(pids), _ids(out), n, C.byref(lut)), "oh_pics_lut", made)
        return out

    def pics_grain(self, pids, grain, seeds, *, planes=None, out=None):
        """finished pictures -> finished pictures of the same params with synthesised film grain added (oh_pics_grain; the exact
        definition is in include/ohevc_hip.h).  grain: what grain_from_sei or make_grain returned; seeds: one int per picture, or one
        int b for b, b + 1, ... — the pictures' POCs, so that a picture gets the same grain however often it is shown; planes: bit c
        set adds grain to plane c, clear copies it (None: the grain's own planes).  out: destination pictures to reuse; None allocates
        pictures with the sources' params.  Returns the destination ids.  Enqueued on the engine stream; does not wait; the grain and
        the seeds may be changed at once."""
        pids = list(pids)
        n = len(pids)
        if not isinstance(grain, Grain):
            raise ValueError("pics_grain: grain is what grain_from_sei or make_grain returns")
        sd = grain_seeds(seeds, n)
        g = grain.as_struct(planes)
        if out is None and n == 0:
            return []
        out, made = self._dsts(out, n, "sources", lambda: self._pic_params(pids[0]))
        buf = sd if sd.size else np.zeros(1, dtype=np.uint32)   # without pictures there is nothing to read, but a non-null pointer all the same
        self._call(self.L.oh_pics_grain(self.h, _ids(pids), _ids(out), n, C.byref(g), buf.ctypes.data_as(C.POINTER(C.c_uint32))),
                   "oh_pics_grain", made)
        return out

    def pics_colour_remap(self, pids, remap, *, out=None):
        """finished 4:4:4 pictures of remap.in_bit_depth -> finished 4:4:4 pictures of the same size at remap.out_bit_depth, every
        sample through the pre tables, the matrix and the post tables (oh_pics_colour_remap; the exact definition is in
        include/ohevc_hip.h).  remap: what remap_from_sei or make_remap returned.  out: destination pictures to reuse; None allocates
        pictures with the sources' params at the output depth.  Returns the destination ids.  Enqueued on the engine stream; does not
        wait; the remap may be changed at once.  Other chroma formats: pics_reformat first, or pics_lut with remap.luts() where the
        matrix is diagonal."""
        pids = list(pids)
        n = len(pids)
        if not isinstance(remap, Remap):
            raise ValueError("pics_colour_remap: remap is what remap_from_sei or make_remap returns")
        r = remap.as_struct()
        if out is None and n == 0:
            return []

        def at_output_depth():
            dp = F.OhPicParams.from_buffer_copy(self._pic_params(pids[0]))
            dp.bit_depth = remap.out_bit_depth
            return dp

        out, made = self._dsts(out, n, "sources", at_output_depth)
        self._call(self.L.oh_pics_colour_remap(self.h, _ids(pids), _ids(out), n, C.byref(r)), "oh_pics_colour_remap", made)
        return out

    def pics_unpack(self, pids, packing, full=True, out=None, *, views=(True, True)):
        """finished frame-packed pictures -> the two views of each as finished pictures (oh_pics_unpack; the exact definition is in
        include/ohevc_hip.h).  packing: what packing_from_sei or make_packing returned.  full: views of the packed pictures' size,
        up-sampled on the phase of the grid positions (quincunx: interpolated on the lattice), else the stored halves.  views: which
        of the two to make.  out: (view 0 ids or None, view 1 ids or None) to reuse — their size picks the mode, `full` is not read;
        None allocates pictures of packing.view_size.  Returns (view 0 ids, view 1 ids), None for a view that was not asked for.
        Enqueued on the engine stream; does not wait."""
        pids = list(pids)
        n = len(pids)
        if not isinstance(packing, Packing):
            raise ValueError("pics_unpack: packing is what packing_from_sei or make_packing returns")
        if n == 0:
            raise ValueError("pics_unpack needs at least one picture (the destinations follow the pictures' params)")
        pk = packing.as_struct()
        made = []
        if out is None:
            want = [bool(views[0]), bool(views[1])]
            if not any(want):
                raise ValueError("pics_unpack: neither view asked for")
            made = self._alloc_like(packing.view_size(self._pic_params(pids[0]), full), n * sum(want))
            sides = [made[:n] if want[0] else None, made[-n:] if want[1] else None]
        else:
            sides = list(out)
            if len(sides) != 2 or (sides[0] is None and sides[1] is None):
                raise ValueError("out: a pair (view 0 ids, view 1 ids) with None for a view that is not asked for")
            sides = [None if s is None else self._dsts(s, n, "sources", None)[0] for s in sides]
        self._call(self.L.oh_pics_unpack(self.h, _ids(pids), None if sides[0] is None else _ids(sides[0]),
                                         None if sides[1] is None else _ids(sides[1]), n, C.byref(pk)), "oh_pics_unpack", made)
        return sides[0], sides[1]

    def pics_pack(self, v0, v1, packing, out=None):
        """two lists of finished views -> finished frame-packed pictures (oh_pics_pack): half-size views are placed in their halves
        with the flips applied, the exact inverse of pics_unpack(full=False); with quincunx sampling full-size views are
        point-sampled on the lattice.  out: destination pictures to reuse; None allocates pictures of the views' params and
        twice their coded size on the packed axis (with quincunx: their size) — a packed size whose half is no whole number of
        minimum coding blocks needs out=, the halves are then the top-left windows of the views.  Returns the destination ids.  Enqueued on the engine stream; does not wait."""
        v0, v1 = list(v0), list(v1)
        n = len(v0)
        if not isinstance(packing, Packing):
            raise ValueError("pics_pack: packing is what packing_from_sei or make_packing returns")
        if len(v1) != n:
            raise ValueError(f"pics_pack: {n} pictures of view 0, {len(v1)} of view 1")
        if n == 0:
            raise ValueError("pics_pack needs at least one pair (the destinations follow the pictures' params)")
        pk = packing.as_struct()

        def packed():
            vp = F.OhPicParams.from_buffer_copy(self._pic_params(v0[0]))
            if not packing.quincunx:
                if packing.arrangement == PACK_ARRANGEMENTS["side_by_side"]:
                    vp.width *= 2
                else:
                    vp.height *= 2
            return vp

        out, made = self._dsts(out, n, "pairs", packed)
        self._call(self.L.oh_pics_pack(self.h, _ids(v0), _ids(v1), _ids(out), n, C.byref(pk)), "oh_pics_pack", made)
        return out

    def pics_compose(self, dst, layers, *, fill=None):
        """finished pictures composed in place on the GPU (oh_pics_compose): dst, the destination ids (identical params); layers, a
        list of at most COMPOSE_MAX_LAYERS Layer applied in order, source over destination with straight alpha in code values; fill,
        None or the (Y, Cb, Cr) sample values every coded plane starts from instead of what the destination holds (a 4:0:0 picture
        reads the first only).  Without fill only the bounding box of the layers is touched.  Ordered with torch both ways like
        pics_import: the engine stream waits for torch's current stream before it reads the alpha tensors, torch's current stream waits
        for the engine stream afterwards, so they may be freed or overwritten at once.  Returns the destination ids; does not wait on
        the host."""
        dst = list(dst)
        layers = list(layers)
        n = len(dst)
        keep = []                                             # what the C structures point at
        ol = (OhLayer * max(len(layers), 1))()
        torch = None
        if any(l.alpha is not None for l in layers):
            import torch
            if not _torch_first:
                raise EngineError("Engine.pics_compose: import torch before the first Engine is created (the engine must share torch's "
                                  "HIP runtime to read its tensors)")
        elif _torch_first:
            import torch
        dev = torch.device("cuda", self.device) if torch is not None else None
        for k, l in enumerate(layers):
            src = list(l.src) if isinstance(l.src, (list, tuple)) else [int(l.src)] * n
            if len(src) != n:
                raise ValueError(f"layer {k}: {len(src)} sources for {n} destinations")
            ids = _ids(src)
            keep.append(ids)
            if l.rect is None:
                sp = self._pic_params(src[0]) if n else None
                rect = (0, 0, sp.width, sp.height) if n else (0, 0, 0, 0)
            else:
                rect = tuple(int(v) for v in l.rect)
            o = ol[k]
            o.src_ids = C.cast(ids, C.POINTER(C.c_int32))
            o.sx, o.sy, o.w, o.h = rect
            o.dx, o.dy = int(l.at[0]), int(l.at[1])
            o.opacity = int(l.opacity)
            if l.alpha is not None:
                t = l.alpha
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != dev or t.dim() not in (2, 3):
                    raise ValueError(f"layer {k}: alpha: want a torch uint8 tensor of shape (h, w) or (n, h, w) on {dev}")
                if tuple(t.shape[-2:]) != (rect[3], rect[2]) or (t.dim() == 3 and t.shape[0] != n):
                    raise ValueError(f"layer {k}: alpha of shape {tuple(t.shape)} for {n} rectangles of {rect[2]} x {rect[3]}")
                st = t.stride()
                if any(s < 0 for s in st):
                    raise ValueError(f"layer {k}: alpha with negative strides {st}")
                keep.append(t)
                o.alpha = t.data_ptr()
                o.alpha_pixel_stride, o.alpha_row_stride = st[-1], st[-2]
                o.alpha_image_stride = st[0] if t.dim() == 3 else 0
        cp = OhCompose(COMPOSE_FILL if fill is not None else 0, (C.c_int32 * 3)(*([int(v) for v in fill] + [0, 0])[:3] if fill is not None else (0, 0, 0)),
                       len(layers), ol)
        with self._torch_ordered(torch):                      # the alpha planes are torch's
            self._chk(self.L.oh_pics_compose(self.h, _ids(dst), n, C.byref(cp)), "oh_pics_compose")
        return dst

    def _pic_params(self, pid):
        p = self._params.get(pid)
        if p is None:
            raise EngineError(f"picture {pid} was not allocated through this Engine object")
        return p

    def pic_device_planes(self, pid):
        p = (C.c_void_p * 3)()
        st, w, h = (C.c_int32 * 3)(), (C.c_int32 * 3)(), (C.c_int32 * 3)()
        self._chk(self.L.oh_pic_device_planes(self.h, pid, p, st, w, h), "oh_pic_device_planes")
        return [(p[c], st[c], w[c], h[c]) for c in range(3)]

    def pic_upsample(self, dst_pid, src_pid, u):
        """SHVC inter-layer reference: resample picture src_pid into dst_pid (u: frame.upsample_setup)"""
        self._chk(self.L.oh_pic_upsample(self.h, dst_pid, src_pid, C.byref(u)), "oh_pic_upsample")

    def memory(self):
        """oh_engine_memory: what the engine holds for work lists (arenas alive, their bytes, free in the pool, staging buffers, their bytes, deferred lists)"""
        out = (C.c_uint64 * 6)()
        self._chk(self.L.oh_engine_memory(self.h, out), "oh_engine_memory")
        return dict(zip(("arenas", "arena_bytes", "arenas_free", "stages", "stage_bytes", "deferred"), map(int, out)))

    # ---- work lists ----
    def pic_upsample_ctbs(self, dst_pid, src_pid, u, log2_ctb_size, ctb_addrs):
        a = (C.c_uint32 * max(len(ctb_addrs), 1))(*ctb_addrs)
        self._chk(self.L.oh_pic_upsample_ctbs(self.h, dst_pid, src_pid, C.byref(u), log2_ctb_size, a, len(ctb_addrs)), "oh_pic_upsample_ctbs")

    def pic_upsample_blocks(self, dst_pid, src_pid, u, log2_ctb_size, ctb_addrs=None, el_conf_win=None):
        """the reference's CTB up-sampling path (oh_pic_upsample_blocks) for the listed CTBs, all when ctb_addrs is None;
        el_conf_win: (left, right, top, bottom) of the enhancement layer's conformance window (only an empty one is covered).
        Raises EngineError (OH_E_UNSUPPORTED) where the reference's output is not defined (upsample_blocks_defined)."""
        a = None if ctb_addrs is None else (C.c_uint32 * max(len(ctb_addrs), 1))(*ctb_addrs)
        w = None if el_conf_win is None else C.byref(OhWindow(*el_conf_win))
        self._chk(self.L.oh_pic_upsample_blocks(self.h, dst_pid, src_pid, C.byref(u), log2_ctb_size, w, a, 0 if a is None else len(ctb_addrs)),
                  "oh_pic_upsample_blocks")

    def frame_upload(self, frame):
        df = C.c_void_p()
        self._chk(self.L.oh_frame_upload(self.h, C.byref(frame), C.byref(df)), "oh_frame_upload")
        return df

    def frames_upload(self, frames):
        """n work lists, one set of preparation launches (oh_frames_upload); returns the device frames"""
        n = len(frames)
        fs = (C.POINTER(F.OhFrame) * n)(*[C.pointer(f) for f in frames])
        out = (C.c_void_p * n)()
        self._chk(self.L.oh_frames_upload(self.h, fs, n, out), "oh_frames_upload")
        return [C.c_void_p(out[i]) for i in range(n)]

    def frame_execute(self, df):
        self._chk(self.L.oh_frame_execute(self.h, df), "oh_frame_execute")
        self.n_batches = getattr(self, "n_batches", 0) + 1

    def frames_execute(self, dfs):
        """one launch per pass over all the (mutually independent) pictures in dfs"""
        arr = (C.c_void_p * len(dfs))(*[d.value if isinstance(d, C.c_void_p) else d for d in dfs])
        self.n_batches = getattr(self, "n_batches", 0) + (len(dfs) + 31) // 32
        self._chk(self.L.oh_frames_execute(self.h, arr, len(dfs)), "oh_frames_execute")

    def frame_download_bs(self, df, params):
        """(vertical, horizontal) boundary-strength grids of an uploaded work list as the deblock pass reads them"""
        n = F.bs_size(params)
        v, h = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self._chk(self.L.oh_frame_download_bs(self.h, df, v.ctypes.data, h.ctypes.data, n), "oh_frame_download_bs")
        return v, h

    def frame_free(self, df):
        self._chk(self.L.oh_frame_free(self.h, df), "oh_frame_free")

    def frame_release(self, df):
        """stream-ordered free (no host wait): call after the last execute of df was enqueued"""
        self._chk(self.L.oh_frame_release(self.h, df), "oh_frame_release")

    def frame_submit(self, frame):
        self._chk(self.L.oh_frame_submit(self.h, C.byref(frame)), "oh_frame_submit")

    # ---- profiling ----
    def profile(self, enable):
        self._chk(self.L.oh_engine_profile(self.h, int(enable)), "oh_engine_profile")

    def pass_times(self, reset=False):
        ms = (C.c_double * OH_N_PASSES)()
        n = C.c_uint64()
        self._chk(self.L.oh_engine_pass_times(self.h, ms, C.byref(n), int(reset)), "oh_engine_pass_times")
        return dict(zip(PASS_NAMES, list(ms))), n.value

    def intra_launch_times(self, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        self._chk(self.L.oh_engine_intra_launch_times(self.h, C.byref(ms), C.byref(n), int(reset)), "oh_engine_intra_launch_times")
        return ms.value, n.value

    HOST_TIME_NAMES = ("upload", "upload_count_loops", "upload_arena", "upload_wait_for_staging_buffer", "upload_memcpy_to_pinned",
                       "upload_enqueue", "execute", "execute_wait_for_preparation", "release")

    def host_times(self, reset=False):
        """{slot: (milliseconds, calls)} of host wall time inside the hand-over path (include/ohevc_hip.h: OhHostTime)"""
        n = len(self.HOST_TIME_NAMES)
        ms, calls = (C.c_double * n)(), (C.c_uint64 * n)()
        self._chk(self.L.oh_engine_host_times(self.h, ms, calls, n, int(reset)), "oh_engine_host_times")
        return {k: (ms[i], calls[i]) for i, k in enumerate(self.HOST_TIME_NAMES)}

    def upload_bytes(self, reset=False):
        return int(self.L.oh_engine_upload_bytes(self.h, int(reset)))

    def stream(self):
        return self.L.oh_engine_stream(self.h)


def remap_frame(frame, id_map):
    """copy of an OhFrame header whose picture ids are translated through id_map (host id -> engine id)"""
    g = F.OhFrame()
    C.memmove(C.byref(g), C.byref(frame), C.sizeof(F.OhFrame))
    g.cur_pic = id_map[frame.cur_pic]
    for i in range(F.OH_MAX_REFS):
        r = frame.ref_pics[i]
        g.ref_pics[i] = id_map.get(r, -1)
    return g
