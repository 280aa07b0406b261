"""The frame packing arrangement SEI reader (include/ohevc_annexb.h: oh_sei_frame_packing; annexb.frame_packing) on hand-assembled NAL
byte strings — no GPU, no reference needed.  The message, MSB first: frame_packing_arrangement_id ue(v), cancel u(1); unless cancelled
arrangement_type u(7), quincunx_sampling u(1), content_interpretation_type u(6), six flags u(1) each, four grid positions u(4) each only
where quincunx_sampling is 0 and the type is not 5, reserved_byte u(8), persistence u(1); then upsampled_aspect_ratio u(1) and the
alignment bits 1 0 .. 0.  What the reference's parser keeps of a message (hevc_sei.c:52-75, cross-read, not run): present = !cancel,
arrangement_type, quincunx_subsampling and content_interpretation_type, the values of exactly these bit positions."""
import ctypes as C

import numpy as np
import pytest

from openhevc_amd import annexb as A

SEI_P, SEI_S = 39, 40
TYPE = 45
FLAGS = ("spatial_flipping", "frame0_flipped", "field_views", "current_frame_is_frame0", "frame0_self_contained", "frame1_self_contained")


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


class Bits:
    def __init__(self):
        self.s = ""

    def u(self, n, v):
        assert 0 <= v < 1 << n
        self.s += format(v, f"0{n}b") if n else ""
        return self

    def ue(self, k):
        z = (k + 1).bit_length() - 1
        self.s += "0" * z + format(k + 1, "b")
        return self

    def aligned(self):
        s = self.s + "1"
        s += "0" * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big")


def fields(d, grid_coded=None):
    """the bits of the dict that annexb.frame_packing returns; grid_coded: whether the grid positions are written, against the rule"""
    b = Bits().ue(d["id"]).u(1, int(d["cancel"]))
    if not d["cancel"]:
        b.u(7, d["arrangement_type"]).u(1, int(d["quincunx_sampling"])).u(6, d["content_interpretation_type"])
        for k in FLAGS:
            b.u(1, int(d[k]))
        coded = not d["quincunx_sampling"] and d["arrangement_type"] != 5
        if coded if grid_coded is None else grid_coded:
            for x, y in d["grid"]:
                b.u(4, x).u(4, y)
        b.u(8, d["reserved_byte"]).u(1, int(d["persistence"]))
    return b.u(1, int(d["upsampled_aspect_ratio"]))


def payload(d):
    return fields(d).aligned()


def packing(arrangement_type=3, quincunx=False, cit=1, flags=(), grid=((0, 0), (0, 0)), id=0, reserved_byte=0, persistence=True, uar=False):
    d = dict(id=id, cancel=False, arrangement_type=arrangement_type, quincunx_sampling=quincunx, content_interpretation_type=cit)
    for k in FLAGS:
        d[k] = k in flags
    d.update(grid=tuple(tuple(g) for g in grid), reserved_byte=reserved_byte, persistence=persistence, upsampled_aspect_ratio=uar)
    return d


def cancelled(id=0, uar=False):
    return dict(id=id, cancel=True, upsampled_aspect_ratio=uar)


def unit(*dicts, nut=SEI_P):
    return nal(nut, escape(b"".join(msg(TYPE, payload(d)) for d in dicts) + b"\x80"))


def raw(n):
    r = A.OhFramePackingSei()
    return A.lib().oh_sei_frame_packing(n, len(n), C.byref(r)), r


def is_zero(r):
    return bytes(r) == bytes(C.sizeof(r))


def reference_keeps(p):
    """what decode_nal_sei_frame_packing_arrangement leaves in the context after the payload p, read from its bits alone"""
    s = "".join(format(v, "08b") for v in p)
    z = s.index("1")
    at = 2 * z + 1                                            # get_ue_golomb
    present = s[at] == "0"
    at += 1
    if not present:
        return dict(present=False)
    return dict(present=True, arrangement_type=int(s[at:at + 7], 2), quincunx=int(s[at + 7]), content_interpretation_type=int(s[at + 8:at + 14], 2))


def check_against_reference(d):
    got = A.frame_packing(unit(d))
    ref = reference_keeps(payload(d))
    assert ref["present"] == (not got["cancel"])
    if ref["present"]:
        assert (got["arrangement_type"], int(got["quincunx_sampling"]), got["content_interpretation_type"]) == \
            (ref["arrangement_type"], ref["quincunx"], ref["content_interpretation_type"])


def test_every_field_comes_back_as_coded():
    rng = np.random.default_rng(45)
    for trial in range(200):
        flags = [k for k in FLAGS if rng.integers(2)]
        d = packing(int(rng.integers(0, 128)), bool(rng.integers(2)), int(rng.integers(0, 64)), flags,
                    [[int(v) for v in rng.integers(0, 16, 2)] for _ in range(2)], int(rng.integers(0, 1000)), int(rng.integers(0, 256)),
                    bool(rng.integers(2)), bool(rng.integers(2)))
        if d["quincunx_sampling"] or d["arrangement_type"] == 5:
            d["grid"] = ((0, 0), (0, 0))                      # not coded: reported as 0
        assert A.frame_packing(unit(d)) == d, d
        check_against_reference(d)


@pytest.mark.parametrize("flag", FLAGS)
def test_each_flag_alone(flag):
    d = packing(4, flags=(flag,))
    got = A.frame_packing(unit(d))
    assert got == d and [k for k in FLAGS if got[k]] == [flag]


def test_both_branches_of_the_grid_condition():
    grid = ((1, 2), (3, 4))
    coded = packing(3, grid=grid, reserved_byte=0xA5, persistence=True, uar=True)
    assert A.frame_packing(unit(coded)) == coded
    # the same fields without the sixteen bits: quincunx sampling, and temporal interleaving
    for d in (packing(3, quincunx=True, reserved_byte=0xA5, uar=True), packing(5, reserved_byte=0xA5, uar=True)):
        assert len(fields(d).s) == len(fields(coded).s) - 16
        got = A.frame_packing(unit(d))
        assert got == d and got["grid"] == ((0, 0), (0, 0)) and got["reserved_byte"] == 0xA5 and got["upsampled_aspect_ratio"]
        check_against_reference(d)
    # sixteen bits written where the rule has none are read as the reserved byte, persistence and what follows: the rule is the reader's
    d = packing(3, quincunx=True, grid=((0xC, 0x3), (0x8, 0x0)), reserved_byte=0x11)
    n = nal(SEI_P, escape(msg(TYPE, fields(d, grid_coded=True).aligned()) + b"\x80"))
    got = A.frame_packing(n)
    assert got["grid"] == ((0, 0), (0, 0)) and got["reserved_byte"] == 0xC3 and got["persistence"] is True


def test_cancel_and_long_ids():
    for id in (0, 1, 254, 255, 256, 65535, 2 ** 31, 2 ** 32 - 1):
        d = cancelled(id, uar=bool(id & 1))
        assert A.frame_packing(unit(d)) == d
        check_against_reference(d)
        d = packing(4, id=id, grid=((4, 12), (15, 1)))
        assert len(Bits().ue(id).s) > 8 or id < 255
        assert A.frame_packing(unit(d)) == d
    rc, r = raw(unit(cancelled(7)))
    assert rc == 1 and r.present == 1 and r.cancel == 1 and r.id == 7 and r.arrangement_type == 0
    # an id of 2^32 does not fit; 33 leading zeros are no ue(v)
    for bits in (Bits().ue(2 ** 32).u(1, 1).u(1, 0), Bits().u(33, 0).u(1, 1).u(34, 0)):
        rc, r = raw(nal(SEI_P, escape(msg(TYPE, bits.aligned()) + b"\x80")))
        assert rc == -1 and is_zero(r)


def test_the_last_of_two_messages_counts():
    a, b = packing(3, grid=((0, 0), (8, 0)), id=1), packing(4, quincunx=True, cit=2, id=2)
    assert A.frame_packing(unit(a, b)) == b
    assert A.frame_packing(unit(b, a)) == a
    assert A.frame_packing(unit(a, cancelled(1))) == cancelled(1)
    # another message type around it, and the suffix SEI, where the message does not count
    n = nal(SEI_P, escape(msg(137, bytes(24)) + msg(TYPE, payload(a)) + msg(144, bytes(4)) + b"\x80"))
    assert A.frame_packing(n) == a
    assert A.frame_packing(unit(a, nut=SEI_S)) is None
    rc, r = raw(nal(SEI_P, escape(msg(144, bytes(4)) + b"\x80")))
    assert rc == 0 and is_zero(r)
    rc, r = raw(nal(32, b"\x00" * 8))
    assert rc == -1 and is_zero(r)


def test_emulation_prevention_inside_the_payload():
    # id 0, type 0 .. : a payload with runs of zero bytes: reserved byte 0, grid positions 0
    d = packing(0, cit=0, grid=((0, 0), (0, 0)), reserved_byte=0, persistence=False)
    p = payload(d)
    assert b"\x00\x00\x00" in p
    n = unit(d)
    assert b"\x00\x00\x03" in n and len(n) > 2 + 2 + len(p) + 1
    assert A.frame_packing(n) == d
    d = packing(3, reserved_byte=0x40)                        # 00 00 01 inside the payload: flags and grid 0, then 01 of the reserved byte
    assert b"\x00\x00\x03\x01" in unit(d)
    assert A.frame_packing(unit(d)) == d


def test_truncation():
    d = packing(3, grid=((4, 12), (9, 9)), id=300, reserved_byte=0x5A)
    p = payload(d)
    nbits = len(fields(d).s)
    for cut in range(len(p)):
        # a payload cut to `cut` bytes, its size byte saying so: the last field lies past its end
        rc, r = raw(nal(SEI_P, escape(msg(TYPE, p[:cut]) + b"\x80")))
        assert (rc, is_zero(r)) == ((1, False) if cut * 8 >= nbits else (-1, True)), cut
    whole = unit(d)
    for cut in range(len(whole) - 1):                         # without the trailing bits alone the message is still whole
        rc, r = raw(whole[:cut])                              # the unit cut: the message runs past it, or there is none yet
        assert rc in (-1, 0) and is_zero(r), cut
    # a cancelled message needs its two flags only
    assert raw(nal(SEI_P, escape(msg(TYPE, Bits().ue(0).u(1, 1).u(1, 1).aligned()) + b"\x80")))[0] == 1
    assert raw(nal(SEI_P, escape(msg(TYPE, b"") + b"\x80")))[0] == -1


def test_struct_round_trip():
    for d in (packing(3, flags=("spatial_flipping", "frame0_flipped"), grid=((0, 8), (8, 0)), cit=2, id=9, reserved_byte=3, uar=True),
              packing(4, quincunx=True), cancelled(5, True)):
        s = A.frame_packing_to_struct(d)
        r = A.frame_packing_struct(unit(d))
        assert bytes(s) == bytes(r)
    with pytest.raises(ValueError):
        A.frame_packing_to_struct(packing(3, grid=((16, 0), (0, 0))))
    with pytest.raises(ValueError):
        A.frame_packing(nal(SEI_P, escape(msg(TYPE, b"") + b"\x80")))
