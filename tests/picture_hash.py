"""Host models of the decoded-picture-hash SEI's CRC and checksum (H.265 Annex D; HM calcCRC / calcChecksum) over whole coded planes,
and a ctypes view of the stream writer's oh_stream_add_hash (include/ohevc_stream.h).  TEST INFRASTRUCTURE."""
import binascii
import ctypes as C

import numpy as np

from openhevc_amd import frame as F


def packed(plane):
    """the plane's rows packed: one byte per sample (uint8), two low byte first (uint16)"""
    return np.ascontiguousarray(plane).astype(plane.dtype.newbyteorder("<"), copy=False).tobytes()


def crc_annex_d(data):
    """the bitwise register of Annex D, transcribed: 0xFFFF, every message bit MSB first, then 16 zero bits"""
    crc = 0xFFFF
    for byte in data:
        for bit_idx in range(8):
            msb = (crc >> 15) & 1
            bit = (byte >> (7 - bit_idx)) & 1
            crc = (((crc << 1) + bit) & 0xFFFF) ^ (msb * 0x1021)
    for _ in range(16):
        msb = (crc >> 15) & 1
        crc = ((crc << 1) & 0xFFFF) ^ (msb * 0x1021)
    return crc


def crc(plane):
    """the same value from the standard library: CRC-16/AUG-CCITT = crc_hqx with initial value 0x1D0F"""
    return binascii.crc_hqx(packed(plane), 0x1D0F)


def checksum_loop(plane, bit_depth):
    """Annex D checksum, transcribed"""
    s = 0
    h, w = plane.shape
    for y in range(h):
        for x in range(w):
            mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
            v = int(plane[y, x])
            s = (s + ((v & 0xFF) ^ mask)) & 0xFFFFFFFF
            if bit_depth > 8:
                s = (s + ((v >> 8) ^ mask)) & 0xFFFFFFFF
    return s


def checksum(plane, bit_depth):
    """the same, vectorised: exact sum in 64 bits, then mod 2^32"""
    v = np.asarray(plane).astype(np.uint64)
    h, w = v.shape
    x = np.arange(w, dtype=np.uint64)[None, :]
    y = np.arange(h, dtype=np.uint64)[:, None]
    mask = (x & 0xFF) ^ (y & 0xFF) ^ (x >> 8) ^ (y >> 8)
    s = int(((v & 0xFF) ^ mask).sum(dtype=np.uint64))
    if bit_depth > 8:
        s += int(((v >> 8) ^ mask).sum(dtype=np.uint64))
    return s & 0xFFFFFFFF


def picture_hash(planes, bit_depth, hash_type):
    """(hash_type, [three values]) of a picture's coded planes as annexb.picture_hash reads them from an SEI (absent planes: 0)"""
    import hashlib
    vals = []
    for c in range(3):
        if c >= len(planes):
            vals.append(bytes(16) if hash_type == 0 else 0)
        elif hash_type == 0:
            vals.append(hashlib.md5(packed(planes[c])).digest())
        elif hash_type == 1:
            vals.append(crc(planes[c]))
        else:
            vals.append(checksum(planes[c], bit_depth))
    return hash_type, vals


def host_pic_hash(hp, p, hash_type):
    return picture_hash([hp.visible(c) for c in range(F.n_planes(p))], p.bit_depth, hash_type)


def payload(hash_type, vals):
    """one picture's three values as the SEI carries them (CRC and checksum big-endian)"""
    if hash_type == 0:
        return b"".join(vals)
    return b"".join(int(v).to_bytes(2 if hash_type == 1 else 4, "big") for v in vals)


def add_hash(data, aus, hash_type, values):
    """the stream with a picture-hash SEI of hash_type behind every picture; values: per picture (decode order) three plane values"""
    import streamgen
    H = F.host()
    H.oh_stream_add_hash.argtypes = [C.POINTER(streamgen.OhStream), C.c_int, C.c_char_p, C.POINTER(streamgen.OhStream)]
    H.oh_stream_free.argtypes = [C.POINTER(streamgen.OhStream)]
    st = streamgen.OhStream()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    off = (C.c_size_t * (len(aus) + 1))(*([a for a, _ in aus] + [aus[-1][1]]))
    st.data, st.size, st.n_pictures, st.au_offset = C.cast(buf, C.POINTER(C.c_uint8)), len(data), len(aus), C.cast(off, C.POINTER(C.c_size_t))
    out = streamgen.OhStream()
    blob = b"".join(payload(hash_type, v) for v in values)
    rc = H.oh_stream_add_hash(C.byref(st), hash_type, blob, C.byref(out))
    if rc:
        raise ValueError(f"oh_stream_add_hash refused hash_type {hash_type} ({rc})")
    res = bytes(C.string_at(out.data, out.size))
    res_aus = [(out.au_offset[i], out.au_offset[i + 1]) for i in range(out.n_pictures)]
    H.oh_stream_free(C.byref(out))
    return res, res_aus


def sei_hashes(data, aus):
    """per access unit: annexb.picture_hash of its suffix SEI NAL unit (None: no such message)"""
    from openhevc_amd import annexb as A
    out = []
    for a, b in aus:
        au = data[a:b]
        found = None
        for off, size, t, *_ in A.nal_units(au):
            if t == 40:
                found = A.picture_hash(au[off:off + size])
        out.append(found)
    return out
