"""The HDR SEI reader (include/ohevc_annexb.h: oh_sei_hdr; annexb.hdr_sei) on hand-assembled NAL byte strings and on a written
stream with the SEI NAL unit inserted into every access unit — no GPU, no reference needed."""
import ctypes as C
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgen                                                            # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402

SC3, SC4 = b"\x00\x00\x01", b"\x00\x00\x00\x01"
PPS, SEI_P, SEI_S = 34, 39, 40
# BT.2020 primaries in the order the message codes them (G, B, R), D65, in units of 0.00002
PRIM = [(8500, 39850), (6550, 2300), (35400, 14600)]
WHITE = (15635, 16450)
MAX_LUM, MIN_LUM = 10000000, 50                                             # 1000 and 0.005 cd/m2
MAX_CLL, MAX_FALL = 1000, 400


def nal(nut, payload=b"", layer=0, tid=0):
    return bytes([(nut << 1) | (layer >> 5), ((layer & 31) << 3) | (tid + 1)]) + payload


def escape(b):
    out, zeros = bytearray(), 0
    for v in b:
        if zeros >= 2 and v <= 3:
            out.append(3)
            zeros = 0
        out.append(v)
        zeros = zeros + 1 if v == 0 else 0
    return bytes(out)


def msg(ptype, payload):
    head = b"\xff" * (ptype // 255) + bytes([ptype % 255])
    return head + b"\xff" * (len(payload) // 255) + bytes([len(payload) % 255]) + payload


def mastering():
    p = b"".join(struct.pack(">HH", x, y) for x, y in PRIM) + struct.pack(">HH", *WHITE) + struct.pack(">II", MAX_LUM, MIN_LUM)
    assert len(p) == 24 and p[16:] == bytes.fromhex("0098968000000032")
    return msg(137, p)


def cll():
    return msg(144, struct.pack(">HH", MAX_CLL, MAX_FALL))


def alt(t=18):
    return msg(147, bytes([t]))


MASTERING = dict(primaries=PRIM, white=WHITE, max_lum=MAX_LUM, min_lum=MIN_LUM)
CLL = dict(max_cll=MAX_CLL, max_fall=MAX_FALL)
ALL = dict(MASTERING, **CLL, preferred_transfer=18)


def raw(n):
    h = A.OhHdrSei()
    return A.lib().oh_sei_hdr(n, len(n), C.byref(h)), h


def test_mastering_display_with_an_emulation_prevention_byte():
    n = nal(SEI_P, escape(mastering() + b"\x80"))
    assert b"\x00\x00\x03\x00\x32" in n                                     # 00 00 00 32 of min_lum cannot stand in a NAL unit
    assert A.hdr_sei(n) == MASTERING
    rc, h = raw(n)
    assert rc == 1 and h.has_mastering == 1 and h.has_cll == 0 and h.has_alt_transfer == 0
    assert (h.max_lum, h.min_lum) == (MAX_LUM, MIN_LUM)


def test_content_light_level_and_alternative_transfer():
    assert A.hdr_sei(nal(SEI_P, escape(cll() + b"\x80"))) == CLL
    assert A.hdr_sei(nal(SEI_P, escape(alt(18) + b"\x80"))) == dict(preferred_transfer=18)
    assert A.hdr_sei(nal(SEI_P, escape(msg(144, b"\x00\x00\x00\x00") + alt(16) + b"\x80"))) == dict(max_cll=0, max_fall=0, preferred_transfer=16)
    rc, h = raw(nal(SEI_P, escape(cll() + alt(18) + b"\x80")))
    assert rc == 2 and (h.has_mastering, h.has_cll, h.has_alt_transfer) == (0, 1, 1)


def test_all_three_behind_a_payload_type_128_message():
    """0x80 in front of the end is payloadType 128 (structure of pictures), not the trailing bits"""
    sop = msg(128, b"\x12\x34\x56")
    assert sop[0] == 0x80
    n = nal(SEI_P, escape(sop + mastering() + cll() + alt() + b"\x80"))
    assert A.hdr_sei(n) == ALL and raw(n)[0] == 3
    # payloads longer than their fields (extension bytes) are read by their fields
    long137 = msg(137, mastering()[2:] + b"\x55\x66")
    assert A.hdr_sei(nal(SEI_P, escape(long137 + b"\x80"))) == MASTERING


def test_unrelated_messages_with_long_type_and_size_are_skipped():
    """a payloadType above 255 (one 0xFF byte) and a payloadSize of 0xFF + 45: 300 bytes that look like HDR messages"""
    decoy = b"\xff" + bytes([137]) + b"\xff" + bytes([45]) + (bytes([144, 4, 9, 9, 9, 9]) * 50)
    assert len(decoy) == 4 + 300
    n = nal(SEI_P, escape(decoy + cll() + b"\x80"))
    assert A.hdr_sei(n) == CLL
    assert A.hdr_sei(nal(SEI_P, escape(decoy + b"\x80"))) is None
    assert raw(nal(SEI_P, escape(decoy + b"\x80")))[0] == 0
    assert A.hdr_sei(nal(SEI_P, escape(msg(5, b"\x01\x02\x03") + b"\x80"))) is None
    # the picture-hash reader walks the same messages
    digest = bytes(range(1, 17))
    both = nal(SEI_P, escape(decoy + cll() + msg(256, b"\x00" + digest * 3) + b"\x80"))
    assert A.hdr_sei(both) == CLL and A.picture_hash(both) == (0, [digest] * 3)


def test_suffix_sei_is_ignored():
    n = nal(SEI_S, escape(mastering() + cll() + alt() + b"\x80"))
    assert raw(n)[0] == 0 and A.hdr_sei(n) is None
    h = raw(n)[1]
    assert (h.has_mastering, h.has_cll, h.has_alt_transfer, h.max_lum, h.max_cll) == (0, 0, 0, 0, 0)


def test_truncated_payloads_and_other_nal_units_are_malformed():
    whole = mastering() + cll() + alt()
    assert raw(nal(SEI_P, escape(whole[:-1])))[0] == -1                      # 147 announces one byte and the unit ends
    assert raw(nal(SEI_P, escape(mastering()[:20])))[0] == -1                # runs past the unit
    assert raw(nal(SEI_P, escape(msg(137, mastering()[2:25]) + b"\x80")))[0] == -1     # 23 bytes: shorter than its fields
    assert raw(nal(SEI_P, escape(msg(144, b"\x03\xe8\x01") + b"\x80")))[0] == -1
    assert raw(nal(SEI_P, escape(msg(147, b"") + b"\x80")))[0] == -1
    assert raw(nal(SEI_P, escape(cll() + msg(147, b"") + b"\x80")))[0] == -1
    rc, h = raw(nal(SEI_P, escape(cll() + msg(147, b"") + b"\x80")))
    assert (h.has_cll, h.max_cll) == (0, 0)                                 # nothing of a malformed unit is reported
    assert raw(nal(PPS, escape(whole + b"\x80")))[0] == -1
    assert raw(nal(SEI_P)[:2])[0] == -1
    with pytest.raises(ValueError):
        A.hdr_sei(nal(PPS, escape(whole + b"\x80")))
    with pytest.raises(ValueError):
        A.hdr_sei(nal(SEI_P, escape(whole[:-1])))


def test_sei_in_front_of_the_first_slice_of_every_access_unit_of_a_written_stream():
    data, aus = streamgen.write_stream(64, 64, 137, n_pictures=5, gop=2)
    before = A.split(data)
    assert len(before) == 5
    out = bytearray()
    for k, (a, b) in enumerate(before):
        au = data[a:b]
        units = A.nal_units(au)
        first = next(u for u in units if u[5])
        at = first[0] - 3                                                   # the three-byte start code of the first slice segment
        if at > 0 and au[at - 1] == 0:
            at -= 1                                                         # its zero_byte
        sei = nal(SEI_P, escape(mastering() + msg(144, struct.pack(">HH", MAX_CLL + k, MAX_FALL)) + alt() + b"\x80"))
        out += au[:at] + SC4 + sei + au[at:]
    out = bytes(out)
    after = A.split(out)
    assert len(after) == len(before)
    for k, (a, b) in enumerate(after):
        au = out[a:b]
        units = A.nal_units(au)
        assert sum(1 for u in units if u[5]) == 1
        found = [A.hdr_sei(au[off:off + size]) for off, size, t, *_ in units if t == SEI_P]
        assert found == [dict(ALL, max_cll=MAX_CLL + k)], k
