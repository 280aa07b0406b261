"""The display-orientation SEI reader (include/ohevc_annexb.h: oh_sei_display_orientation; annexb.display_orientation) on
hand-assembled NAL byte strings and on a written stream with the SEI NAL unit spliced into every access unit — no GPU, no reference
needed.  The message: cancel u(1); unless cancelled hor_flip u(1), ver_flip u(1), anticlockwise_rotation u(16), persistence u(1) — 20
bits, then the alignment bits 1000."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgen                                                            # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402

SC4 = b"\x00\x00\x00\x01"
PPS, SEI_P, SEI_S = 34, 39, 40
TYPE = 47


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


def payload(hor_flip=0, ver_flip=0, rotation=0, persistence=0, cancel=0):
    if cancel:
        return bytes([0xC0])                                                # the flag, then the alignment bits 1000000
    bits = (hor_flip << 22) | (ver_flip << 21) | (rotation << 5) | (persistence << 4) | 0x8
    return bits.to_bytes(3, "big")


def orientation(**kw):
    return msg(TYPE, payload(**kw))


def fields(hor_flip=0, ver_flip=0, rotation=0, persistence=0, cancel=0):
    return dict(cancel=bool(cancel), hor_flip=bool(hor_flip), ver_flip=bool(ver_flip), anticlockwise_rotation=rotation,
                persistence=bool(persistence))


def raw(n):
    d = A.OhDisplayOrientation()
    return A.lib().oh_sei_display_orientation(n, len(n), C.byref(d)), d


def test_full_message():
    assert payload(1, 0, 0x4000, 1) == bytes([0x48, 0x00, 0x18]) and payload(0, 1, 0xFFFF, 0) == bytes([0x3F, 0xFF, 0xE8])
    for kw in (dict(hor_flip=1, ver_flip=0, rotation=0x4000, persistence=1), dict(hor_flip=0, ver_flip=1, rotation=0xFFFF, persistence=0),
               dict(hor_flip=1, ver_flip=1, rotation=0x8001, persistence=1), dict(rotation=0xC000)):
        n = nal(SEI_P, escape(orientation(**kw) + b"\x80"))
        assert A.display_orientation(n) == fields(**kw), kw
        rc, d = raw(n)
        assert rc == 1 and d.present == 1 and d.cancel == 0
        assert (d.hor_flip, d.ver_flip, d.anticlockwise_rotation, d.persistence) == (kw.get("hor_flip", 0), kw.get("ver_flip", 0),
                                                                                     kw["rotation"], kw.get("persistence", 0))
    # a payload longer than its fields (extension bytes) is read by its fields
    long47 = msg(TYPE, payload(1, 1, 0x4000, 0) + b"\x55\x66")
    assert A.display_orientation(nal(SEI_P, escape(long47 + b"\x80"))) == fields(1, 1, 0x4000, 0)


def test_cancelled_message():
    n = nal(SEI_P, escape(orientation(cancel=1) + b"\x80"))
    assert A.display_orientation(n) == fields(cancel=1)
    rc, d = raw(n)
    assert rc == 1 and (d.present, d.cancel, d.hor_flip, d.ver_flip, d.anticlockwise_rotation, d.persistence) == (1, 1, 0, 0, 0, 0)
    # the bits behind a set cancel flag are not fields
    assert A.display_orientation(nal(SEI_P, escape(msg(TYPE, b"\xff\xff\xff") + b"\x80"))) == fields(cancel=1)


def test_behind_an_unrelated_message_with_long_type_and_size():
    """a payloadType above 255 (one 0xFF byte) and a payloadSize of 0xFF + 45: 300 bytes that look like display orientations"""
    decoy = b"\xff" + bytes([TYPE]) + b"\xff" + bytes([45]) + (bytes([TYPE, 3, 0x7f, 0xff, 0xf8]) * 60)
    assert len(decoy) == 4 + 300
    n = nal(SEI_P, escape(decoy + orientation(hor_flip=1, rotation=0x4000) + b"\x80"))
    assert A.display_orientation(n) == fields(hor_flip=1, rotation=0x4000)
    assert A.display_orientation(nal(SEI_P, escape(decoy + b"\x80"))) is None and raw(nal(SEI_P, escape(decoy + b"\x80")))[0] == 0
    assert A.display_orientation(nal(SEI_P, escape(msg(5, b"\x01\x02\x03") + b"\x80"))) is None
    # the other readers walk the same messages
    both = nal(SEI_P, escape(msg(144, b"\x03\xe8\x01\x90") + orientation(ver_flip=1) + b"\x80"))
    assert A.display_orientation(both) == fields(ver_flip=1) and A.hdr_sei(both) == dict(max_cll=1000, max_fall=400)


def test_rotation_zero_and_emulation_prevention():
    """rotation 0 with both flips clear: the payload is 00 00 08 (00 00 18 with persistence) — two zero bytes, but the byte behind them
    carries the alignment bit, so the message's own bytes never need an emulation-prevention byte.  One is needed where a message in
    front of it ends the run: its payload 00 00 01 is written 00 00 03 01, and the orientation behind it is found where it lies after
    the unit was unescaped."""
    assert payload() == b"\x00\x00\x08" and payload(persistence=1) == b"\x00\x00\x18"
    for pers in (0, 1):
        body = orientation(persistence=pers) + b"\x80"
        assert escape(body) == body
        assert A.display_orientation(nal(SEI_P, body)) == fields(persistence=pers)
    body = msg(5, b"\x00\x00\x01\x00\x00\x00") + orientation() + b"\x80"
    n = nal(SEI_P, escape(body))
    assert len(n) == 2 + len(body) + 2 and b"\x00\x00\x03\x01\x00\x00\x03\x00" in n
    assert A.display_orientation(n) == fields()
    n = nal(SEI_P, escape(msg(5, b"\x00\x00\x01\x00\x00\x00") + orientation(hor_flip=1, ver_flip=1, rotation=0x8000, persistence=1) + b"\x80"))
    assert A.display_orientation(n) == fields(1, 1, 0x8000, 1)


def test_suffix_sei_is_ignored():
    n = nal(SEI_S, escape(orientation(hor_flip=1, rotation=0x4000) + b"\x80"))
    rc, d = raw(n)
    assert rc == 0 and A.display_orientation(n) is None
    assert (d.present, d.cancel, d.hor_flip, d.ver_flip, d.anticlockwise_rotation, d.persistence) == (0, 0, 0, 0, 0, 0)


def test_truncated_payloads_and_other_nal_units_are_malformed():
    whole = orientation(hor_flip=1, rotation=0x4000)
    assert raw(nal(SEI_P, escape(whole[:-1])))[0] == -1                      # announces three bytes and the unit ends
    assert raw(nal(SEI_P, escape(msg(TYPE, payload(1, 0, 0x4000)[:2]) + b"\x80")))[0] == -1      # two bytes: shorter than its fields
    assert raw(nal(SEI_P, escape(msg(TYPE, b"\x40") + b"\x80")))[0] == -1    # not cancelled, one byte
    assert raw(nal(SEI_P, escape(msg(TYPE, b"") + b"\x80")))[0] == -1        # not even the cancel flag
    rc, d = raw(nal(SEI_P, escape(whole + msg(TYPE, b"\x40") + b"\x80")))
    assert rc == -1 and (d.present, d.hor_flip, d.anticlockwise_rotation) == (0, 0, 0)   # nothing of a malformed unit is reported
    assert raw(nal(PPS, escape(whole + b"\x80")))[0] == -1
    assert raw(nal(SEI_P)[:2])[0] == -1
    with pytest.raises(ValueError):
        A.display_orientation(nal(PPS, escape(whole + b"\x80")))
    with pytest.raises(ValueError):
        A.display_orientation(nal(SEI_P, escape(whole[:-1])))


def test_sei_in_front_of_the_first_slice_of_every_access_unit_of_a_written_stream():
    data, aus = streamgen.write_stream(64, 64, 47, n_pictures=4, gop=2)
    before = A.split(data)
    assert len(before) == 4
    out = bytearray()
    for k, (a, b) in enumerate(before):
        au = data[a:b]
        units = A.nal_units(au)
        first = next(u for u in units if u[5])
        at = first[0] - 3                                                   # the three-byte start code of the first slice segment
        if at > 0 and au[at - 1] == 0:
            at -= 1                                                         # its zero_byte
        sei = nal(SEI_P, escape(orientation(hor_flip=k & 1, ver_flip=k >> 1, rotation=k << 14, persistence=1) + b"\x80"))
        out += au[:at] + SC4 + sei + au[at:]
    out = bytes(out)
    after = A.split(out)
    assert len(after) == len(before)
    for k, (a, b) in enumerate(after):
        au = out[a:b]
        units = A.nal_units(au)
        assert sum(1 for u in units if u[5]) == 1
        found = [A.display_orientation(au[off:off + size]) for off, size, t, *_ in units if t == SEI_P]
        assert found == [fields(k & 1, k >> 1, k << 14, 1)], k
