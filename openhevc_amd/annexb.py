"""ctypes view of include/ohevc_annexb.h (libohevc_host.so): access-unit splitter, NAL scan, NAL unescape, picture-hash SEI, HDR SEIs, display-orientation SEI, picture timing SEI."""
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
