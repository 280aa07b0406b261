"""ctypes view of include/ohevc_annexb.h (libohevc_host.so): access-unit splitter, NAL scan, NAL unescape, picture-hash SEI, HDR SEIs, display-orientation SEI, picture timing SEI, film grain SEI, colour remapping SEI, frame packing SEI."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
END_NOT_FOUND = -100


class OhAuScanner(C.Structure):
    _fields_ = [("state64", C.c_uint64), ("frame_start_found", C.c_int32), ("reserved", C.c_int32)]


class OhNal(C.Structure):
    _fields_ = [("offset", C.c_size_t), ("size", C.c_size_t), ("type", C.c_int32), ("layer_id", C.c_int32), ("temporal_id", C.c_int32),
                ("first_slice_segment_in_pic", C.c_int32)]


class OhPictureHash(C.Structure):
    _fields_ = [("present", C.c_int32), ("hash_type", C.c_int32), ("md5", (C.c_uint8 * 16) * 3), ("crc", C.c_uint32 * 3), ("checksum", C.c_uint32 * 3)]


class OhHdrSei(C.Structure):
    _fields_ = [("has_mastering", C.c_int32), ("primaries", (C.c_uint16 * 2) * 3), ("white", C.c_uint16 * 2), ("max_lum", C.c_uint32),
                ("min_lum", C.c_uint32), ("has_cll", C.c_int32), ("max_cll", C.c_uint16), ("max_fall", C.c_uint16),
                ("has_alt_transfer", C.c_int32), ("preferred_transfer", C.c_int32)]


class OhDisplayOrientation(C.Structure):
    _fields_ = [("present", C.c_int32), ("cancel", C.c_int32), ("hor_flip", C.c_int32), ("ver_flip", C.c_int32),
                ("anticlockwise_rotation", C.c_uint32), ("persistence", C.c_int32)]


class OhPicTiming(C.Structure):
    _fields_ = [("present", C.c_int32), ("pic_struct", C.c_int32), ("source_scan_type", C.c_int32), ("duplicate_flag", C.c_int32)]


FG_MAX_INTERVALS, FG_MAX_VALUES = 256, 6                       # OH_FG_MAX_INTERVALS, OH_FG_MAX_VALUES


class OhFilmGrainSei(C.Structure):
    _fields_ = [("present", C.c_int32), ("cancel", C.c_int32), ("model_id", C.c_int32), ("separate_colour_description", C.c_int32),
                ("bit_depth_luma_minus8", C.c_int32), ("bit_depth_chroma_minus8", C.c_int32), ("full_range", C.c_int32),
                ("colour_primaries", C.c_int32), ("transfer_characteristics", C.c_int32), ("matrix_coeffs", C.c_int32),
                ("blending_mode_id", C.c_int32), ("log2_scale_factor", C.c_int32), ("comp_model_present", C.c_int32 * 3),
                ("num_intensity_intervals_minus1", C.c_int32 * 3), ("num_model_values_minus1", C.c_int32 * 3), ("persistence", C.c_int32),
                ("lower", (C.c_uint8 * FG_MAX_INTERVALS) * 3), ("upper", (C.c_uint8 * FG_MAX_INTERVALS) * 3),
                ("value", ((C.c_int32 * FG_MAX_VALUES) * FG_MAX_INTERVALS) * 3)]


CRI_MAX_PIVOTS = 33                                            # OH_CRI_MAX_PIVOTS


class OhColourRemapSei(C.Structure):
    _fields_ = [("present", C.c_int32), ("cancel", C.c_int32), ("id", C.c_uint32), ("persistence", C.c_int32),
                ("video_signal_info_present", C.c_int32), ("full_range", C.c_int32), ("primaries", C.c_int32),
                ("transfer_function", C.c_int32), ("matrix_coefficients", C.c_int32),
                ("input_bit_depth", C.c_int32), ("output_bit_depth", C.c_int32), ("pre_lut_num_val_minus1", C.c_int32 * 3),
                ("pre_lut_coded_value", (C.c_uint16 * CRI_MAX_PIVOTS) * 3), ("pre_lut_target_value", (C.c_uint16 * CRI_MAX_PIVOTS) * 3),
                ("matrix_present", C.c_int32), ("log2_matrix_denom", C.c_int32), ("coeffs", (C.c_int32 * 3) * 3),
                ("post_lut_num_val_minus1", C.c_int32 * 3),
                ("post_lut_coded_value", (C.c_uint16 * CRI_MAX_PIVOTS) * 3), ("post_lut_target_value", (C.c_uint16 * CRI_MAX_PIVOTS) * 3)]


_FP_FLAGS = ("spatial_flipping", "frame0_flipped", "field_views", "current_frame_is_frame0", "frame0_self_contained", "frame1_self_contained")
_FP_GRID = ("frame0_grid_position_x", "frame0_grid_position_y", "frame1_grid_position_x", "frame1_grid_position_y")


class OhFramePackingSei(C.Structure):
    _fields_ = ([("present", C.c_int32), ("cancel", C.c_int32), ("id", C.c_uint32), ("arrangement_type", C.c_int32),
                 ("quincunx_sampling", C.c_int32), ("content_interpretation_type", C.c_int32)] +
                [(k, C.c_int32) for k in _FP_FLAGS + _FP_GRID] +
                [("reserved_byte", C.c_int32), ("persistence", C.c_int32), ("upsampled_aspect_ratio", C.c_int32)])


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(_HERE, "libohevc_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make -C openhevc_amd` (or __graft_entry__.build())")
        L = C.CDLL(path)
        L.oh_au_scanner_init.argtypes = [C.POINTER(OhAuScanner)]
        L.oh_au_scanner_init.restype = None
        L.oh_au_find_frame_end.argtypes = [C.POINTER(OhAuScanner), C.c_char_p, C.c_size_t]
        L.oh_au_find_frame_end.restype = C.c_long
        L.oh_annexb_split.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t]
        L.oh_annexb_split.restype = C.c_long
        L.oh_annexb_nal_units.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(OhNal), C.c_size_t]
        L.oh_annexb_nal_units.restype = C.c_long
        L.oh_nal_unescape.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_int32)]
        L.oh_nal_unescape.restype = C.c_long
        L.oh_sei_picture_hash.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(OhPictureHash)]
        L.oh_sei_picture_hash.restype = C.c_int
        L.oh_sei_hdr.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(OhHdrSei)]
        L.oh_sei_hdr.restype = C.c_int
        L.oh_sei_display_orientation.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(OhDisplayOrientation)]
        L.oh_sei_display_orientation.restype = C.c_int
        L.oh_sei_pic_timing.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(OhPicTiming)]
        L.oh_sei_pic_timing.restype = C.c_int
        L.oh_sei_film_grain.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(OhFilmGrainSei)]
        L.oh_sei_film_grain.restype = C.c_int
        L.oh_sei_colour_remap.argtypes = [C.c_char_p, C.c_size_t, C.c_int64, C.POINTER(OhColourRemapSei)]
        L.oh_sei_colour_remap.restype = C.c_int
        L.oh_sei_frame_packing.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(OhFramePackingSei)]
        L.oh_sei_frame_packing.restype = C.c_int
        _lib = L
    return _lib


def split(data):
    """[(start, end)] of the access units of an Annex-B buffer (oh_annexb_split)"""
    L = lib()
    cap = 64
    while True:
        off = (C.c_size_t * cap)()
        n = L.oh_annexb_split(data, len(data), off, cap)
        if n >= 0:
            return [(off[i], off[i + 1]) for i in range(n)]
        cap = -n + 1


def nal_units(buf):
    """[(offset, size, type, layer_id, temporal_id, first_slice_segment_in_pic)]"""
    L = lib()
    cap = 64
    while True:
        arr = (OhNal * cap)()
        n = L.oh_annexb_nal_units(buf, len(buf), arr, cap)
        if n < 0:
            raise ValueError("no start code where one is due")
        if n <= cap:
            return [(u.offset, u.size, u.type, u.layer_id, u.temporal_id, u.first_slice_segment_in_pic) for u in arr[:n]]
        cap = n


def unescape(nal):
    """(rbsp bytes, [positions of the bytes before each dropped emulation-prevention byte], bytes consumed)"""
    L = lib()
    dst = C.create_string_buffer(max(len(nal), 1))
    n = C.c_size_t()
    ns = C.c_int32()
    cap = len(nal) // 3 + 1
    pos = (C.c_int32 * cap)()
    used = L.oh_nal_unescape(nal, len(nal), dst, C.byref(n), pos, cap, C.byref(ns))
    return dst.raw[:n.value], list(pos[:ns.value]), used


def picture_hash(nal):
    """None, or (hash_type, [three digests / values]) of the decoded-picture-hash message of one SEI NAL unit"""
    h = OhPictureHash()
    r = lib().oh_sei_picture_hash(nal, len(nal), C.byref(h))
    if r < 0:
        raise ValueError("malformed SEI NAL unit")
    if not r:
        return None
    if h.hash_type == 0:
        return 0, [bytes(h.md5[c]) for c in range(3)]
    return h.hash_type, list(h.crc if h.hash_type == 1 else h.checksum)


def hdr_sei(nal):
    """None, or a dict of what the HDR messages of one prefix SEI NAL unit carry (oh_sei_hdr): "primaries" ([(x, y)] * 3), "white",
    "max_lum", "min_lum" (raw: 0.00002 for the chromaticities, 0.0001 cd/m2 for the luminances) from a mastering display colour volume;
    "max_cll", "max_fall" (cd/m2, 0 unknown) from a content light level; "preferred_transfer" from alternative transfer
    characteristics.  Keys of messages the unit does not hold are absent."""
    h = OhHdrSei()
    r = lib().oh_sei_hdr(nal, len(nal), C.byref(h))
    if r < 0:
        raise ValueError("malformed SEI NAL unit")
    if not r:
        return None
    d = {}
    if h.has_mastering:
        d.update(primaries=[(h.primaries[c][0], h.primaries[c][1]) for c in range(3)], white=(h.white[0], h.white[1]),
                 max_lum=int(h.max_lum), min_lum=int(h.min_lum))
    if h.has_cll:
        d.update(max_cll=int(h.max_cll), max_fall=int(h.max_fall))
    if h.has_alt_transfer:
        d["preferred_transfer"] = int(h.preferred_transfer)
    return d


def display_orientation(nal):
    """None, or a dict of the display-orientation message (payload type 47) of one prefix SEI NAL unit (oh_sei_display_orientation):
    "cancel", "hor_flip", "ver_flip" (bool), "anticlockwise_rotation" (0 .. 65535, units of 360 / 65536 degrees), "persistence"; the
    fields behind "cancel" are False / 0 in a cancelled message.  engine.orientation_from_sei turns the flips and the rotation into
    an orientation of Engine.pics_orient where the rotation is a multiple of a quarter turn; engine.warp_from_sei turns them into the
    map and the image size of Engine.pics_warp at any angle."""
    d = OhDisplayOrientation()
    r = lib().oh_sei_display_orientation(nal, len(nal), C.byref(d))
    if r < 0:
        raise ValueError("malformed SEI NAL unit")
    if not r:
        return None
    return dict(cancel=bool(d.cancel), hor_flip=bool(d.hor_flip), ver_flip=bool(d.ver_flip),
                anticlockwise_rotation=int(d.anticlockwise_rotation), persistence=bool(d.persistence))


def pic_timing(nal, frame_field_info_present=True):
    """None, or a dict of the picture timing message (payload type 1) of one prefix SEI NAL unit (oh_sei_pic_timing): "pic_struct",
    "source_scan_type", "duplicate_flag" as ints.  frame_field_info_present is the VUI flag of the stream's SPS, which the caller
    knows; without it the message holds none of the three and they are -1.  engine.field_info says what a pic_struct means."""
    d = OhPicTiming()
    r = lib().oh_sei_pic_timing(nal, len(nal), int(bool(frame_field_info_present)), C.byref(d))
    if r < 0:
        raise ValueError("malformed SEI NAL unit")
    if not r:
        return None
    return dict(pic_struct=int(d.pic_struct), source_scan_type=int(d.source_scan_type), duplicate_flag=int(d.duplicate_flag))


def film_grain_struct(nal):
    """None, or the OhFilmGrainSei of the film grain characteristics message (payload type 19) of one prefix SEI NAL unit"""
    g = OhFilmGrainSei()
    r = lib().oh_sei_film_grain(nal, len(nal), C.byref(g))
    if r < 0:
        raise ValueError("malformed SEI NAL unit")
    return g if r else None


def film_grain(nal):
    """None, or a dict of the film grain characteristics message (payload type 19) of one prefix SEI NAL unit (oh_sei_film_grain),
    every field as coded: "cancel" (bool; a cancelled message holds nothing else), "model_id", "colour" (None, or a dict of
    "bit_depth_luma", "bit_depth_chroma", "full_range", "colour_primaries", "transfer_characteristics", "matrix_coeffs" where the
    separate colour description is present), "blending_mode_id", "log2_scale_factor", "persistence" (bool) and "components": three
    entries, None for a component without a model, else a list of (lower, upper, [model values]) per intensity interval.
    engine.grain_from_sei turns the dict into what Engine.pics_grain takes."""
    g = film_grain_struct(nal)
    if g is None:
        return None
    if g.cancel:
        return dict(cancel=True)
    colour = None
    if g.separate_colour_description:
        colour = dict(bit_depth_luma=8 + g.bit_depth_luma_minus8, bit_depth_chroma=8 + g.bit_depth_chroma_minus8,
                      full_range=bool(g.full_range), colour_primaries=int(g.colour_primaries),
                      transfer_characteristics=int(g.transfer_characteristics), matrix_coeffs=int(g.matrix_coeffs))
    comps = []
    for c in range(3):
        if not g.comp_model_present[c]:
            comps.append(None)
            continue
        nv = g.num_model_values_minus1[c] + 1
        comps.append([(int(g.lower[c][i]), int(g.upper[c][i]), [int(g.value[c][i][j]) for j in range(nv)])
                      for i in range(g.num_intensity_intervals_minus1[c] + 1)])
    return dict(cancel=False, model_id=int(g.model_id), colour=colour, blending_mode_id=int(g.blending_mode_id),
                log2_scale_factor=int(g.log2_scale_factor), components=comps, persistence=bool(g.persistence))


def film_grain_to_struct(d):
    """the OhFilmGrainSei that film_grain would have read the dict d from"""
    g = OhFilmGrainSei()
    g.present = 1
    if d.get("cancel"):
        g.cancel = 1
        return g
    g.model_id = int(d.get("model_id", 0))
    colour = d.get("colour")
    if colour:
        g.separate_colour_description = 1
        g.bit_depth_luma_minus8, g.bit_depth_chroma_minus8 = int(colour["bit_depth_luma"]) - 8, int(colour["bit_depth_chroma"]) - 8
        g.full_range = int(bool(colour["full_range"]))
        g.colour_primaries, g.transfer_characteristics = int(colour["colour_primaries"]), int(colour["transfer_characteristics"])
        g.matrix_coeffs = int(colour["matrix_coeffs"])
    g.blending_mode_id, g.log2_scale_factor = int(d.get("blending_mode_id", 0)), int(d.get("log2_scale_factor", 0))
    g.persistence = int(bool(d.get("persistence", False)))
    comps = list(d.get("components", ()))
    if len(comps) > 3:
        raise ValueError("film grain: at most three components")
    for c, iv in enumerate(comps):
        if iv is None:
            continue
        iv = list(iv)
        if not 1 <= len(iv) <= FG_MAX_INTERVALS:
            raise ValueError(f"film grain: component {c} has {len(iv)} intervals (1 .. {FG_MAX_INTERVALS})")
        nv = {len(v) for _, _, v in iv}
        if len(nv) != 1 or not 1 <= min(nv) <= FG_MAX_VALUES:
            raise ValueError(f"film grain: the intervals of component {c} have one number of model values, 1 .. {FG_MAX_VALUES}")
        g.comp_model_present[c] = 1
        g.num_intensity_intervals_minus1[c], g.num_model_values_minus1[c] = len(iv) - 1, nv.pop() - 1
        for i, (lo, hi, vals) in enumerate(iv):
            if not (0 <= int(lo) <= 255 and 0 <= int(hi) <= 255):
                raise ValueError("film grain: the bounds of an interval are 0 .. 255")
            g.lower[c][i], g.upper[c][i] = int(lo), int(hi)
            for j, v in enumerate(vals):
                g.value[c][i][j] = int(v)
    return g


def colour_remap_struct(nal, id=None):
    """None, or the OhColourRemapSei of the colour remapping information message (payload type 142) of one prefix SEI NAL unit: the
    last one of the unit, or with id the last one whose colour_remap_id is id"""
    r = OhColourRemapSei()
    rc = lib().oh_sei_colour_remap(nal, len(nal), -1 if id is None else int(id), C.byref(r))
    if rc < 0:
        raise ValueError("malformed SEI NAL unit")
    return r if rc else None


def colour_remap(nal, id=None):
    """None, or a dict of the colour remapping information message (payload type 142) of one prefix SEI NAL unit
    (oh_sei_colour_remap), every field as coded: "id", "cancel" (bool; a cancelled message holds nothing else), "persistence" (bool),
    "signal" (None, or a dict of "full_range", "primaries", "transfer_function", "matrix_coefficients"), "input_bit_depth",
    "output_bit_depth", "pre" and "post": three lists of (coded, target) pivots, empty where num_val_minus1 is 0, and "matrix": None, or
    (log2_matrix_denom, three rows of three coefficients).  id: None takes the last message of the unit, a number the last one with that
    colour_remap_id.  engine.remap_from_sei turns the dict into what Engine.pics_colour_remap takes."""
    r = colour_remap_struct(nal, id)
    if r is None:
        return None
    if r.cancel:
        return dict(id=int(r.id), cancel=True)
    signal = None
    if r.video_signal_info_present:
        signal = dict(full_range=bool(r.full_range), primaries=int(r.primaries), transfer_function=int(r.transfer_function),
                      matrix_coefficients=int(r.matrix_coefficients))

    def pivots(nm1, coded, target):
        return [[(int(coded[c][i]), int(target[c][i])) for i in range(nm1[c] + 1 if nm1[c] else 0)] for c in range(3)]

    matrix = (int(r.log2_matrix_denom), [[int(r.coeffs[c][i]) for i in range(3)] for c in range(3)]) if r.matrix_present else None
    return dict(id=int(r.id), cancel=False, persistence=bool(r.persistence), signal=signal, input_bit_depth=int(r.input_bit_depth),
                output_bit_depth=int(r.output_bit_depth), pre=pivots(r.pre_lut_num_val_minus1, r.pre_lut_coded_value, r.pre_lut_target_value),
                matrix=matrix, post=pivots(r.post_lut_num_val_minus1, r.post_lut_coded_value, r.post_lut_target_value))


def colour_remap_to_struct(d):
    """the OhColourRemapSei that colour_remap would have read the dict d from"""
    r = OhColourRemapSei()
    r.present, r.id = 1, int(d.get("id", 0))
    if d.get("cancel"):
        r.cancel = 1
        return r
    r.persistence = int(bool(d.get("persistence", False)))
    signal = d.get("signal")
    if signal:
        r.video_signal_info_present = 1
        r.full_range = int(bool(signal["full_range"]))
        r.primaries, r.transfer_function = int(signal["primaries"]), int(signal["transfer_function"])
        r.matrix_coefficients = int(signal["matrix_coefficients"])
    r.input_bit_depth, r.output_bit_depth = int(d["input_bit_depth"]), int(d["output_bit_depth"])
    for key, nm1, coded, target in (("pre", r.pre_lut_num_val_minus1, r.pre_lut_coded_value, r.pre_lut_target_value),
                                    ("post", r.post_lut_num_val_minus1, r.post_lut_coded_value, r.post_lut_target_value)):
        curves = list(d.get(key) or ((), (), ()))
        if len(curves) != 3:
            raise ValueError(f"colour remap: {key} has three curves")
        for c, pv in enumerate(curves):
            pv = list(pv)
            if len(pv) == 1 or len(pv) > CRI_MAX_PIVOTS:
                raise ValueError(f"colour remap: {key}[{c}] has {len(pv)} pivots (none, or 2 .. {CRI_MAX_PIVOTS}: num_val_minus1 of 0 codes none)")
            nm1[c] = max(len(pv) - 1, 0)
            for i, (x, y) in enumerate(pv):
                if not (0 <= int(x) <= 0xFFFF and 0 <= int(y) <= 0xFFFF):
                    raise ValueError("colour remap: a pivot is two values of 16 bits")
                coded[c][i], target[c][i] = int(x), int(y)
    matrix = d.get("matrix")
    if matrix is not None:
        r.matrix_present = 1
        r.log2_matrix_denom = int(matrix[0])
        for c in range(3):
            for i in range(3):
                r.coeffs[c][i] = int(matrix[1][c][i])
    return r


def frame_packing_struct(nal):
    """None, or the OhFramePackingSei of the last frame packing arrangement message (payload type 45) of one prefix SEI NAL unit"""
    r = OhFramePackingSei()
    rc = lib().oh_sei_frame_packing(nal, len(nal), C.byref(r))
    if rc < 0:
        raise ValueError("malformed SEI NAL unit")
    return r if rc else None


def frame_packing(nal):
    """None, or a dict of the frame packing arrangement message (payload type 45) of one prefix SEI NAL unit (oh_sei_frame_packing),
    every field as coded: "id", "cancel" (bool; a cancelled message holds nothing else but "upsampled_aspect_ratio"),
    "arrangement_type" (3 side by side, 4 top-bottom, 5 temporal interleaving), "quincunx_sampling" (bool),
    "content_interpretation_type", the flags "spatial_flipping", "frame0_flipped", "field_views", "current_frame_is_frame0",
    "frame0_self_contained", "frame1_self_contained" (bool), "grid": ((frame0 x, y), (frame1 x, y)), zeros where the message does not
    code them, "reserved_byte", "persistence" (bool) and "upsampled_aspect_ratio" (bool).  engine.packing_from_sei turns the dict into
    what Engine.pics_unpack / pics_pack take."""
    r = frame_packing_struct(nal)
    if r is None:
        return None
    if r.cancel:
        return dict(id=int(r.id), cancel=True, upsampled_aspect_ratio=bool(r.upsampled_aspect_ratio))
    d = dict(id=int(r.id), cancel=False, arrangement_type=int(r.arrangement_type), quincunx_sampling=bool(r.quincunx_sampling),
             content_interpretation_type=int(r.content_interpretation_type))
    for k in _FP_FLAGS:
        d[k] = bool(getattr(r, k))
    d["grid"] = ((int(r.frame0_grid_position_x), int(r.frame0_grid_position_y)), (int(r.frame1_grid_position_x), int(r.frame1_grid_position_y)))
    d.update(reserved_byte=int(r.reserved_byte), persistence=bool(r.persistence), upsampled_aspect_ratio=bool(r.upsampled_aspect_ratio))
    return d


def frame_packing_to_struct(d):
    """the OhFramePackingSei that frame_packing would have read the dict d from"""
    r = OhFramePackingSei()
    r.present, r.id = 1, int(d.get("id", 0))
    r.upsampled_aspect_ratio = int(bool(d.get("upsampled_aspect_ratio", False)))
    if d.get("cancel"):
        r.cancel = 1
        return r
    r.arrangement_type = int(d["arrangement_type"])
    r.quincunx_sampling = int(bool(d.get("quincunx_sampling", False)))
    r.content_interpretation_type = int(d.get("content_interpretation_type", 0))
    for k in _FP_FLAGS:
        setattr(r, k, int(bool(d.get(k, False))))
    grid = d.get("grid", ((0, 0), (0, 0)))
    for k, v in zip(_FP_GRID, (grid[0][0], grid[0][1], grid[1][0], grid[1][1])):
        if not 0 <= int(v) <= 15:
            raise ValueError("frame packing: a grid position is a value of 4 bits")
        setattr(r, k, int(v))
    r.reserved_byte = int(d.get("reserved_byte", 0))
    r.persistence = int(bool(d.get("persistence", False)))
    return r
