"""The colour remapping information SEI reader (include/ohevc_annexb.h: oh_sei_colour_remap; annexb.colour_remap) on hand-assembled NAL
byte strings — no GPU, no reference needed.  The message, MSB first: colour_remap_id ue(v), cancel u(1); unless cancelled persistence
u(1), video_signal_info_present u(1) [full range u(1), primaries, transfer function, matrix coefficients u(8) each], input and output
bit depth u(8) each; per component pre_lut_num_val_minus1 u(8) and, above 0, that many plus one pairs of coded u(vi) and target u(vo);
matrix_present u(1) [log2_matrix_denom u(4), nine se(v)]; per component post_lut_num_val_minus1 u(8) and its pairs u(vo), u(vo); then the
alignment bits 1 0 .. 0.  vi = ((input depth + 7) >> 3) << 3, vo likewise."""
import ctypes as C

import numpy as np
import pytest

from openhevc_amd import annexb as A

SEI_P, SEI_S = 39, 40
TYPE = 142


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

    def se(self, v):
        return self.ue(2 * v - 1 if v > 0 else -2 * v)

    def aligned(self):
        s = self.s + "1"
        s += "0" * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big")


def width(bd):
    return ((bd + 7) >> 3) << 3


def fields(d, num_val_minus1=None):
    """the bits of the dict that annexb.colour_remap returns; num_val_minus1: written in place of every count (for the refusals)"""
    b = Bits().ue(d["id"])
    if d.get("cancel"):
        return b.u(1, 1)
    b.u(1, 0).u(1, int(d["persistence"])).u(1, int(d["signal"] is not None))
    if d["signal"] is not None:
        s = d["signal"]
        b.u(1, int(s["full_range"])).u(8, s["primaries"]).u(8, s["transfer_function"]).u(8, s["matrix_coefficients"])
    b.u(8, d["input_bit_depth"]).u(8, d["output_bit_depth"])
    vi, vo = width(d["input_bit_depth"]), width(d["output_bit_depth"])

    def curves(key, vc):
        for pv in d[key]:
            assert len(pv) != 1
            b.u(8, max(len(pv) - 1, 0) if num_val_minus1 is None else num_val_minus1)
            for x, y in pv:
                b.u(vc, x).u(vo, y)

    curves("pre", vi)
    b.u(1, int(d["matrix"] is not None))
    if d["matrix"] is not None:
        b.u(4, d["matrix"][0])
        for row in d["matrix"][1]:
            for k in row:
                b.se(k)
    curves("post", vo)
    return b


def payload(d):
    return fields(d).aligned()


def remap(bi, bo, pre=((), (), ()), matrix=None, post=((), (), ()), id=0, signal=None, persistence=False):
    return dict(id=id, cancel=False, persistence=persistence, signal=signal, input_bit_depth=bi, output_bit_depth=bo,
                pre=[list(p) for p in pre], matrix=matrix, post=[list(p) for p in post])


def unit(*dicts, nut=SEI_P):
    return nal(nut, escape(b"".join(msg(TYPE, payload(d)) for d in dicts) + b"\x80"))


def raw(n, id=-1):
    r = A.OhColourRemapSei()
    return A.lib().oh_sei_colour_remap(n, len(n), id, C.byref(r)), r


def is_zero(r):
    return bytes(r) == bytes(C.sizeof(r))


def pivots(rng, bi, bo, n):
    xs = np.sort(rng.choice(np.arange(1 << bi), n, replace=False))
    return [(int(x), int(y)) for x, y in zip(xs, rng.integers(0, 1 << bo, n))]


BT2020 = dict(full_range=True, primaries=9, transfer_function=16, matrix_coefficients=9)
_rng = np.random.default_rng(142)
FULL = remap(10, 8, pre=[pivots(_rng, 10, 8, 33) for _ in range(3)], matrix=(14, [[16000, -300, 5], [-32768, 32767, 0], [1, -1, -32767]]),
             post=[pivots(_rng, 8, 8, 33) for _ in range(3)], id=7, signal=BT2020, persistence=True)


def test_bit_writer():
    assert Bits().ue(0).s == "1" and Bits().ue(1).s == "010" and Bits().ue(2).s == "011" and Bits().ue(3).s == "00100"
    assert Bits().se(0).s == "1" and Bits().se(1).s == "010" and Bits().se(-1).s == "011" and Bits().se(2).s == "00100"
    assert width(8) == 8 and width(9) == 16 and width(16) == 16
    # id 0 (1), not cancelled, no persistence, no signal info: 1000; depths 8, 8; three counts of 0; no matrix; three counts of 0
    assert payload(remap(8, 8)) == bytes([0x80, 0x80, 0x80, 0, 0, 0, 0, 0, 0x04])      # 69 bits, then the one


def test_full_message():
    """10 -> 8 bit, 33 pivots on every curve, a matrix with the extreme coefficients, the signal info"""
    d = A.colour_remap(unit(FULL))
    assert d == FULL
    assert all(len(p) == 33 for p in d["pre"] + d["post"]) and d["matrix"][1][1] == [-32768, 32767, 0]
    r = A.colour_remap_struct(unit(FULL))
    assert (r.present, r.cancel, r.id, r.persistence, r.video_signal_info_present, r.full_range) == (1, 0, 7, 1, 1, 1)
    assert (r.primaries, r.transfer_function, r.matrix_coefficients, r.input_bit_depth, r.output_bit_depth) == (9, 16, 9, 10, 8)
    assert list(r.pre_lut_num_val_minus1) == [32] * 3 and list(r.post_lut_num_val_minus1) == [32] * 3
    assert (r.matrix_present, r.log2_matrix_denom) == (1, 14) and [list(row) for row in r.coeffs] == FULL["matrix"][1]
    assert r.pre_lut_coded_value[2][32] == FULL["pre"][2][32][0] and r.post_lut_target_value[1][0] == FULL["post"][1][0][1]


@pytest.mark.parametrize("bi", range(8, 17))
@pytest.mark.parametrize("bo", range(8, 17))
def test_depths_and_field_widths(bi, bo):
    """the coded values of a curve take 8 bits at a depth of 8 and 16 bits above; the largest values of each width come back"""
    Mi, Mo = (1 << bi) - 1, (1 << bo) - 1
    d = remap(bi, bo, pre=[[(0, Mo), (Mi, 0)], [], [(1, 1), (2, Mo), (Mi, Mo)]], matrix=(0, [[1, 0, 0], [0, 1, 0], [0, 0, 1]]),
              post=[[], [(0, 0), (Mo, Mo)], [(Mo - 1, 5), (Mo, 6)]])
    assert A.colour_remap(unit(d)) == d
    bits = len(fields(d).s)
    assert bits == 1 + 3 + 16 + 24 + 5 * width(bi) + 5 * width(bo) + 1 + 4 + 3 * 3 + 6 * 1 + 24 + 8 * width(bo)


def test_absent_parts():
    """no signal info, no matrix, num_val_minus1 0 on every curve: what is absent is 0"""
    d = remap(12, 12, id=3)
    assert A.colour_remap(unit(d)) == d
    r = A.colour_remap_struct(unit(d))
    assert (r.video_signal_info_present, r.full_range, r.primaries, r.matrix_present, r.log2_matrix_denom) == (0, 0, 0, 0, 0)
    assert not any(any(row) for row in r.coeffs) and not any(r.pre_lut_num_val_minus1) and not any(r.post_lut_num_val_minus1)
    with_matrix = remap(8, 10, matrix=(15, [[0, 0, 0]] * 3))
    assert A.colour_remap(unit(with_matrix))["matrix"] == (15, [[0, 0, 0]] * 3)


@pytest.mark.parametrize("k", [0, 1, -1, 255, -256, 32767, -32767, -32768, 65535, 2 ** 31 - 1, -2 ** 31])
def test_coefficients(k):
    """every coefficient as coded, also outside what the service takes"""
    rows = [[k, -k if k != -2 ** 31 else k, 0], [1, k, -1], [0, 0, k]]
    d = remap(8, 8, matrix=(5, rows))
    assert A.colour_remap(unit(d))["matrix"] == (5, rows)


def test_cancelled():
    n = nal(SEI_P, escape(msg(TYPE, Bits().ue(9).u(1, 1).aligned()) + b"\x80"))
    assert A.colour_remap(n) == dict(id=9, cancel=True)
    rc, r = raw(n)
    assert rc == 1 and (r.present, r.cancel, r.id) == (1, 1, 9)
    r.present = r.cancel = r.id = 0
    assert is_zero(r)                                                       # nothing else is set
    assert A.colour_remap(unit(dict(id=9, cancel=True))) == dict(id=9, cancel=True)


def test_emulation_prevention():
    """a payload with runs of zero bytes: 16-bit pivots of small values"""
    d = remap(10, 10, pre=[[(0, 0), (1, 0), (2, 1), (3, 2)], [], []], post=[[], [], [(0, 0), (256, 0), (512, 3)]])
    n = unit(d)
    assert n.count(b"\x00\x00\x03") >= 4 and len(n) > len(nal(SEI_P, msg(TYPE, payload(d)) + b"\x80"))
    assert A.colour_remap(n) == d


def test_suffix_sei_is_passed_over():
    rc, r = raw(unit(FULL, nut=SEI_S))
    assert rc == 0 and is_zero(r) and A.colour_remap(unit(FULL, nut=SEI_S)) is None
    other = nal(SEI_P, escape(msg(19, b"\x80") + b"\x80"))                  # a cancelled film grain message: no colour remapping
    assert A.colour_remap(other) is None


def test_ids_select_among_messages():
    a, b, c = remap(10, 10, id=1, persistence=True), remap(10, 8, id=2, pre=[[(0, 5), (1023, 250)], [], []]), remap(8, 8, id=1)
    n = unit(a, b, c)
    assert A.colour_remap(n) == c and A.colour_remap(n, id=-1) == c         # the last one
    assert A.colour_remap(n, id=2) == b and A.colour_remap(n, id=1) == c    # the last one of that id
    assert A.colour_remap(unit(a, b), id=1) == a
    assert A.colour_remap(n, id=3) is None and A.colour_remap(n, id=2 ** 40) is None
    rc, r = raw(n, 3)
    assert rc == 0 and is_zero(r)
    big = remap(8, 8, id=2 ** 32 - 2)                                       # the largest ue(v) of 32 bits
    assert A.colour_remap(unit(a, big), id=2 ** 32 - 2) == big
    # another message in front and behind
    n = nal(SEI_P, escape(msg(137, bytes(24)) + msg(TYPE, payload(b)) + msg(144, bytes(4)) + b"\x80"))
    assert A.colour_remap(n, id=2) == b


def test_truncation_at_every_length():
    """the unit cut to every shorter length, and the payload cut to every shorter length inside a whole unit: -1 and zeroed output"""
    for d in (FULL, remap(8, 8), remap(9, 16, matrix=(1, [[7, 8, 9]] * 3), signal=BT2020)):
        n = unit(d)
        assert raw(n)[0] == 1
        for k in range(len(n) - 1):                                         # without its last byte, the trailing bits, the message is whole
            rc, r = raw(n[:k])
            assert rc == -1 and is_zero(r), (k, len(n))
        p = payload(d)
        assert len(fields(d).s) % 8 != 0                                    # the last byte holds a field
        for k in range(len(p)):
            rc, r = raw(nal(SEI_P, escape(msg(TYPE, p[:k]) + b"\x80")))
            assert rc == -1 and is_zero(r), (k, len(p))


def test_a_malformed_message_of_another_id_spoils_the_unit():
    bad = nal(SEI_P, escape(msg(TYPE, payload(remap(8, 8, id=1))) + msg(TYPE, payload(remap(8, 8, id=2))[:4]) + b"\x80"))
    rc, r = raw(bad, 1)
    assert rc == -1 and is_zero(r)
    with pytest.raises(ValueError, match="malformed"):
        A.colour_remap(bad, id=1)


@pytest.mark.parametrize("what", ["num_val 33", "num_val 255", "depth 7", "depth 17", "depth 0 out", "depth 255 out", "ue 33 zeros",
                                  "se 33 zeros", "ue too large", "not an SEI", "message past the unit"])
def test_refusals(what):
    if what.startswith("num_val"):
        d = remap(8, 8, pre=[[(i, i) for i in range(34)]] + [[]] * 2)
        n = nal(SEI_P, escape(msg(TYPE, fields(d, int(what.split()[1])).aligned()) + b"\x80"))
    elif what.startswith("depth"):
        v = int(what.split()[1])
        head = Bits().ue(0).u(1, 0).u(1, 0).u(1, 0)
        head = head.u(8, 8).u(8, v) if what.endswith("out") else head.u(8, v).u(8, 8)
        n = nal(SEI_P, escape(msg(TYPE, head.u(64, 0).aligned()) + b"\x80"))
    elif what == "ue 33 zeros":
        b = Bits()
        b.s = "0" * 33 + "1" + "0" * 33
        n = nal(SEI_P, escape(msg(TYPE, b.u(64, 0).aligned()) + b"\x80"))
    elif what == "ue too large":                                            # 32 zeros: codeNum 2^32 - 1 + 1 does not fit 32 bits
        b = Bits()
        b.s = "0" * 32 + "1" + "0" * 31 + "1"
        n = nal(SEI_P, escape(msg(TYPE, b.u(64, 0).aligned()) + b"\x80"))
        ok = Bits()
        ok.s = "0" * 32 + "1" + "0" * 32                                    # codeNum 2^32 - 1 fits
        assert raw(nal(SEI_P, escape(msg(TYPE, ok.u(1, 1).aligned()) + b"\x80")))[1].id == 2 ** 32 - 1
    elif what == "se 33 zeros":
        b = Bits().ue(0).u(1, 0).u(1, 0).u(1, 0).u(8, 8).u(8, 8).u(24, 0).u(1, 1).u(4, 0)
        b.s += "0" * 33 + "1" + "0" * 33
        n = nal(SEI_P, escape(msg(TYPE, b.u(64, 0).u(64, 0).aligned()) + b"\x80"))
    elif what == "not an SEI":
        n = nal(34, escape(msg(TYPE, payload(FULL)) + b"\x80"))
    else:
        p = payload(remap(8, 8))
        n = nal(SEI_P, escape(bytes([TYPE, len(p) + 2]) + p + b"\x80"))      # the trailing bits are one byte
    rc, r = raw(n)
    assert rc == -1 and is_zero(r)
    with pytest.raises(ValueError, match="malformed"):
        A.colour_remap(n)


def test_se_value_that_does_not_fit():
    """se(v) codes around the ends of int32_t: codeNum 2^32 - 1 is the value 2^31, which does not fit; codeNum 2^32 is -2^31, which does"""
    def with_code(k):
        b = Bits().ue(0).u(1, 0).u(1, 0).u(1, 0).u(8, 8).u(8, 8).u(24, 0).u(1, 1).u(4, 0).ue(k)
        for _ in range(8):
            b.se(0)
        return nal(SEI_P, escape(msg(TYPE, b.u(24, 0).aligned()) + b"\x80"))
    assert A.colour_remap(with_code(2 ** 32))["matrix"][1][0][0] == -2 ** 31
    assert A.colour_remap(with_code(2 ** 32 - 2))["matrix"][1][0][0] == -2 ** 31 + 1
    assert A.colour_remap(with_code(2 ** 32 - 3))["matrix"][1][0][0] == 2 ** 31 - 1
    for k in (2 ** 32 - 1, 2 ** 32 + 1, 2 ** 33 - 2):
        rc, r = raw(with_code(k))
        assert rc == -1 and is_zero(r)


def test_round_trip_dict_struct_dict():
    for d in (FULL, remap(8, 8), remap(12, 9, matrix=(3, [[-1, 2, -3], [4, -5, 6], [-7, 8, -9]]), post=[[(0, 1), (5, 0)], [], []]),
              dict(id=4, cancel=True)):
        s = A.colour_remap_to_struct(d)
        assert bytes(s) == bytes(A.colour_remap_struct(unit(d)))            # the struct that the reader fills
        n = unit(d)
        assert A.colour_remap(n) == d
    with pytest.raises(ValueError):
        A.colour_remap_to_struct(remap(8, 8, pre=[[(1, 1)], [], []]))       # one pivot cannot be coded
    with pytest.raises(ValueError):
        A.colour_remap_to_struct(remap(8, 8, pre=[[(i, i) for i in range(34)], [], []]))
