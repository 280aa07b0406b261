"""The film grain characteristics SEI reader (include/ohevc_annexb.h: oh_sei_film_grain; annexb.film_grain) on hand-assembled NAL byte
strings and on a written stream with the SEI NAL unit spliced into every access unit — no GPU, no reference needed.  The message, MSB
first: cancel u(1); unless cancelled model_id u(2), separate_colour_description_present u(1) [bit depths u(3) u(3), full range u(1),
primaries, transfer, matrix u(8) each], blending_mode_id u(2), log2_scale_factor u(4), comp_model_present[3] u(1) each; per present
component num_intensity_intervals_minus1 u(8), num_model_values_minus1 u(3), per interval lower u(8), upper u(8) and the model values
se(v); persistence u(1); then the alignment bits 1 0 .. 0."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streamgen                                                            # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402

SC4 = b"\x00\x00\x00\x01"
PPS, SEI_P, SEI_S = 34, 39, 40
TYPE = 19


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

    def se(self, v):
        k = 2 * v - 1 if v > 0 else -2 * v                                  # codeNum
        z = (k + 1).bit_length() - 1
        self.s += "0" * z + format(k + 1, "b")
        return self

    def aligned(self):
        s = self.s + "1"
        s += "0" * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big")


def payload(d):
    """the payload bytes of the dict that annexb.film_grain returns"""
    return fields(d).aligned()


def fields(d):
    b = Bits()
    if d.get("cancel"):
        return b.u(1, 1)
    b.u(1, 0).u(2, d["model_id"]).u(1, int(d["colour"] is not None))
    if d["colour"] is not None:
        c = d["colour"]
        b.u(3, c["bit_depth_luma"] - 8).u(3, c["bit_depth_chroma"] - 8).u(1, int(c["full_range"]))
        b.u(8, c["colour_primaries"]).u(8, c["transfer_characteristics"]).u(8, c["matrix_coeffs"])
    b.u(2, d["blending_mode_id"]).u(4, d["log2_scale_factor"])
    for comp in d["components"]:
        b.u(1, int(comp is not None))
    for comp in d["components"]:
        if comp is None:
            continue
        b.u(8, len(comp) - 1).u(3, len(comp[0][2]) - 1)
        for lo, hi, vals in comp:
            b.u(8, lo).u(8, hi)
            for v in vals:
                b.se(v)
    return b.u(1, int(d["persistence"]))


def grain(components, model_id=0, colour=None, blending=0, scale=0, persistence=False):
    return dict(cancel=False, model_id=model_id, colour=colour, blending_mode_id=blending, log2_scale_factor=scale,
                components=components, persistence=persistence)


BT709 = dict(bit_depth_luma=10, bit_depth_chroma=9, full_range=True, colour_primaries=1, transfer_characteristics=13, matrix_coeffs=6)
FULL = grain([[(16, 63, [40, 6, 10]), (64, 127, [30, 8, 8]), (128, 235, [12, 14, 2])],
              [(0, 255, [20, 5, 5])],
              [(10, 20, [255, 2, 14]), (200, 250, [0, 14, 2])]], colour=BT709, blending=1, scale=5, persistence=True)


def unit(d, nut=SEI_P):
    return nal(nut, escape(msg(TYPE, payload(d)) + b"\x80"))


def raw(n):
    g = A.OhFilmGrainSei()
    return A.lib().oh_sei_film_grain(n, len(n), C.byref(g)), g


def is_zero(g):
    return bytes(g) == bytes(C.sizeof(g))


def test_bit_writer():
    assert Bits().se(0).s == "1" and Bits().se(1).s == "010" and Bits().se(-1).s == "011" and Bits().se(2).s == "00100"
    assert Bits().se(-3).s == "00111" and Bits().u(1, 1).aligned() == b"\xc0"
    # cancel 0, model 0, no description, blending 0, scale 2, components 1 0 0, 1 interval, 1 value, 0 .. 255, se(4), persistence 1
    assert payload(grain([[(0, 255, [4])], None, None], scale=2, persistence=True)) == bytes([0x00, 0xa0, 0x00, 0x00, 0xff, 0x11, 0x80])


def test_full_message_with_three_components():
    n = unit(FULL)
    assert A.film_grain(n) == FULL
    rc, g = raw(n)
    assert rc == 1 and (g.present, g.cancel, g.model_id, g.separate_colour_description) == (1, 0, 0, 1)
    assert (g.bit_depth_luma_minus8, g.bit_depth_chroma_minus8, g.full_range) == (2, 1, 1)
    assert (g.colour_primaries, g.transfer_characteristics, g.matrix_coeffs) == (1, 13, 6)
    assert (g.blending_mode_id, g.log2_scale_factor, g.persistence) == (1, 5, 1)
    assert list(g.comp_model_present) == [1, 1, 1] and list(g.num_intensity_intervals_minus1) == [2, 0, 1]
    assert list(g.num_model_values_minus1) == [2, 2, 2]
    assert (g.lower[0][2], g.upper[0][2], list(g.value[0][2])) == (128, 235, [12, 14, 2, 0, 0, 0])
    assert (g.lower[2][1], g.upper[2][1], list(g.value[2][1])) == (200, 250, [0, 14, 2, 0, 0, 0])
    assert g.lower[0][3] == 0 and g.upper[1][1] == 0 and list(g.value[1][1]) == [0] * 6     # nothing behind what was coded
    # a payload longer than its fields (extension bytes) is read by its fields
    assert A.film_grain(nal(SEI_P, escape(msg(TYPE, payload(FULL) + b"\x55\x66") + b"\x80"))) == FULL
    # the dict goes back into the struct that was read
    assert bytes(A.film_grain_to_struct(FULL)) == bytes(g)


@pytest.mark.parametrize("nv", [1, 2, 3, 6])
def test_one_component_and_the_number_of_model_values(nv):
    vals = [17, 9, 3, -2, 100000, -100000][:nv]
    for c in range(3):
        comps = [None] * 3
        comps[c] = [(5, 9, vals), (10, 10, [v + 1 for v in vals])]
        d = grain(comps, scale=15, blending=3, model_id=3)
        assert A.film_grain(unit(d)) == d, (c, nv)


def test_negative_and_extreme_model_values():
    for vals in ([-1, -2, -3], [0, 0, 0], [-255, 255], [2 ** 31 - 1], [-(2 ** 31 - 1)], [-(2 ** 31)], [65535, -65536, 1]):
        d = grain([None, [(0, 0, vals)], None])
        assert A.film_grain(unit(d)) == d, vals
    # se(v) codes of 32 leading zeros: -2^31 fits an int32, 2^31 does not; 33 leading zeros are no code
    head = Bits().u(1, 0).u(2, 0).u(1, 0).u(2, 0).u(4, 0).u(3, 4).u(8, 0).u(3, 0).u(8, 1).u(8, 2)
    fits, over, long = Bits(), Bits(), Bits()
    fits.s = head.s + "0" * 32 + "1" + format(1, "032b") + "1"              # codeNum 2^32: -2^31
    over.s = head.s + "0" * 32 + "1" + format(0, "032b") + "1"              # codeNum 2^32 - 1: 2^31
    long.s = head.s + "0" * 33 + "1" + format(0, "033b") + "1"
    assert A.film_grain(nal(SEI_P, escape(msg(TYPE, fits.aligned()) + b"\x80")))["components"][0] == [(1, 2, [-(2 ** 31)])]
    for bad in (over, long):
        rc, g = raw(nal(SEI_P, escape(msg(TYPE, bad.aligned()) + b"\x80")))
        assert rc == -1 and is_zero(g)


def test_colour_description_present_and_absent():
    comps = [[(0, 255, [10])], None, None]
    with_c, without = grain(comps, colour=BT709), grain(comps)
    assert len(payload(with_c)) == len(payload(without)) + 4                # 31 bits more
    assert A.film_grain(unit(with_c)) == with_c and A.film_grain(unit(without)) == without
    assert A.film_grain(unit(without))["colour"] is None


def test_cancelled_message():
    assert payload(dict(cancel=True)) == b"\xc0"
    n = unit(dict(cancel=True))
    assert A.film_grain(n) == dict(cancel=True)
    rc, g = raw(n)
    assert rc == 1 and (g.present, g.cancel) == (1, 1)
    g.present = g.cancel = 0
    assert is_zero(g)
    # the bits behind a set cancel flag are not fields
    assert A.film_grain(nal(SEI_P, escape(msg(TYPE, b"\xff\xff\xff") + b"\x80"))) == dict(cancel=True)


def test_payload_that_needs_emulation_prevention():
    """bounds 0 / 0 and model values 0 make runs of zero bytes in the payload, which the NAL unit carries with 03 bytes between them;
    the reader works on the unescaped bytes"""
    d = grain([[(0, 0, [32, 8, 8])], None, None])                           # 00 00 behind 24 bits of head, then se(32): 000000 1000000
    d0 = grain([[(0, 0, [0]), (0, 0, [0]), (0, 0, [0])], [(0, 0, [0])], None])
    for dd in (d, d0):
        p = payload(dd)
        body = msg(TYPE, p) + b"\x80"
        assert b"\x00\x00" in p and b"\x00\x00\x03" in escape(body) and len(escape(body)) > len(body)
        assert A.film_grain(nal(SEI_P, escape(body))) == dd
    # behind a message whose payload ends a zero run
    n = nal(SEI_P, escape(msg(5, b"\x00\x00\x01\x00\x00\x00") + msg(TYPE, payload(FULL)) + b"\x80"))
    assert b"\x00\x00\x03\x01" in n and A.film_grain(n) == FULL


def test_suffix_sei_is_passed_over_and_other_messages_are_not_grain():
    rc, g = raw(unit(FULL, SEI_S))
    assert rc == 0 and is_zero(g) and A.film_grain(unit(FULL, SEI_S)) is None
    assert A.film_grain(nal(SEI_P, escape(msg(47, b"\x48\x00\x18") + b"\x80"))) is None
    both = nal(SEI_P, escape(msg(144, b"\x03\xe8\x01\x90") + msg(TYPE, payload(FULL)) + b"\x80"))
    assert A.film_grain(both) == FULL and A.hdr_sei(both) == dict(max_cll=1000, max_fall=400)


def test_of_two_messages_the_last_counts():
    first, last = grain([[(0, 255, [50, 4, 4])], [(0, 255, [9])], None], scale=3), grain([None, None, [(7, 8, [1, 2])]])
    n = nal(SEI_P, escape(msg(TYPE, payload(first)) + msg(TYPE, payload(last)) + b"\x80"))
    assert A.film_grain(n) == last
    rc, g = raw(n)
    assert rc == 1 and list(g.comp_model_present) == [0, 0, 1] and g.lower[0][0] == 0 and g.upper[0][0] == 0 and g.value[0][0][0] == 0
    n = nal(SEI_P, escape(msg(TYPE, payload(first)) + msg(TYPE, payload(dict(cancel=True))) + b"\x80"))
    assert A.film_grain(n) == dict(cancel=True)


def test_truncated_at_every_byte_length():
    """the payload cut to every shorter length, with its size byte made to fit, and the unit cut to every shorter length"""
    for d in (FULL, grain([[(0, 255, [1])], None, None], persistence=True)):
        p = payload(d)
        assert len(fields(d).s) % 8 and len(p) == len(fields(d).s) // 8 + 1     # the last byte holds a field: no shorter payload is whole
        for k in range(len(p)):
            rc, g = raw(nal(SEI_P, escape(msg(TYPE, p[:k]) + b"\x80")))
            assert rc == -1 and is_zero(g), k
        whole = nal(SEI_P, msg(TYPE, p))                                    # no zero runs in these: escaping changes nothing
        if escape(whole[2:]) == whole[2:]:
            for k in range(len(whole)):
                assert raw(whole[:k])[0] == -1, k                           # announces more bytes than the unit has
    assert raw(nal(PPS, escape(msg(TYPE, payload(FULL)) + b"\x80")))[0] == -1
    with pytest.raises(ValueError):
        A.film_grain(nal(PPS, escape(msg(TYPE, payload(FULL)) + b"\x80")))
    with pytest.raises(ValueError):
        A.film_grain(nal(SEI_P, escape(msg(TYPE, payload(FULL)[:-1]) + b"\x80")))
    # a malformed message behind a good one: nothing of the unit is reported
    rc, g = raw(nal(SEI_P, escape(msg(TYPE, payload(FULL)) + msg(TYPE, b"\x00") + b"\x80")))
    assert rc == -1 and is_zero(g)


def test_more_than_six_model_values_is_malformed():
    b = Bits().u(1, 0).u(2, 0).u(1, 0).u(2, 0).u(4, 0).u(3, 4).u(8, 0).u(3, 6).u(8, 0).u(8, 255)
    for _ in range(7):
        b.se(1)
    rc, g = raw(nal(SEI_P, escape(msg(TYPE, b.u(1, 0).aligned()) + b"\x80")))
    assert rc == -1 and is_zero(g)
    b7 = Bits().u(1, 0).u(2, 0).u(1, 0).u(2, 0).u(4, 0).u(3, 4).u(8, 0).u(3, 7).u(8, 0).u(8, 255)
    for _ in range(8):
        b7.se(1)
    assert raw(nal(SEI_P, escape(msg(TYPE, b7.u(1, 0).aligned()) + b"\x80")))[0] == -1


def test_256_intervals():
    d = grain([[(i, i, [i, 2 + i % 13]) for i in range(256)], None, None])
    p = payload(d)
    assert len(p) > 255                                                     # the payload size takes an 0xFF byte
    assert A.film_grain(nal(SEI_P, escape(msg(TYPE, p) + b"\x80"))) == d


def test_sei_in_front_of_the_first_slice_of_every_access_unit_of_a_written_stream():
    data, aus = streamgen.write_stream(64, 64, 47, n_pictures=4, gop=2)
    before = A.split(data)
    assert len(before) == 4

    def of(k):
        return grain([[(0, 127, [10 + k, 4 + k]), (128, 255, [k, 2])],
                      None, [(k, 200 + k, [k])] if k & 1 else None], scale=k, persistence=bool(k & 2))

    out = bytearray()
    for k, (a, b) in enumerate(before):
        au = data[a:b]
        units = A.nal_units(au)
        first = next(u for u in units if u[5])
        at = first[0] - 3                                                   # the three-byte start code of the first slice segment
        if at > 0 and au[at - 1] == 0:
            at -= 1                                                         # its zero_byte
        out += au[:at] + SC4 + unit(of(k)) + au[at:]
    out = bytes(out)
    after = A.split(out)
    assert len(after) == len(before)
    for k, (a, b) in enumerate(after):
        au = out[a:b]
        units = A.nal_units(au)
        assert sum(1 for u in units if u[5]) == 1
        found = [A.film_grain(au[off:off + size]) for off, size, t, *_ in units if t == SEI_P]
        assert found == [of(k)], k
