"""Fields and deinterlacing without a GPU: the numpy model the GPU tests compare against (tests/deinterlace_model.py) held against
independent restatements, the host-only functions of include/ohevc_hip.h (oh_deint_adaptive, oh_field_info) against the model and the
table, what the GPU tests' random planes make the model do, the picture timing SEI reader (include/ohevc_annexb.h: oh_sei_pic_timing) on
hand-assembled NAL units, and the names of the Python layer."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deinterlace_model as DM                                              # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402


# ---------------- the model against restatements ----------------
def reference_row_walk(src):
    """the reference's deinterlace_bottom_field (imgconvert.c:352-379) restated: five row cursors m2, m1, 0, p1, p2 that start on rows
    0, 0, 1, 2, 3; per step the row under m1 is copied, the next row is filtered from the five cursors, then m2, m1, 0 take the places
    of 0, p1, p2 and p1, p2 move down two rows; the last pair filters with 0 standing in for p1 and p2.  8 bit, the top field kept."""
    src = np.asarray(src).astype(int)
    height, width = src.shape
    dst = np.zeros_like(src)

    def line(m2, m1, c0, p1, p2):
        row = np.empty(width, int)
        for x in range(width):
            total = -src[m2, x]
            total += src[m1, x] << 2
            total += src[c0, x] << 1
            total += src[p1, x] << 2
            total += -src[p2, x]
            row[x] = min(max((total + 4) >> 3, 0), 255)                      # the crop table
        return row
    m2, m1, c0, p1, p2 = 0, 0, 1, 2, 3
    out = 0
    y = 0
    while y < height - 2:
        dst[out] = src[m1]
        out += 1
        dst[out] = line(m2, m1, c0, p1, p2)
        m2, m1, c0 = c0, p1, p2
        p1 += 2
        p2 += 2
        out += 1
        y += 2
    dst[out] = src[m1]
    out += 1
    dst[out] = line(m2, m1, c0, c0, c0)
    return dst


@pytest.mark.parametrize("w,h", ((8, 8), (12, 16)))
def test_lowpass5_is_the_reference_row_walk(w, h):
    rng = np.random.default_rng(w * h)
    for k in range(8):
        src = rng.integers(0, 256, (h, w), dtype=np.uint8)
        if k == 1:
            src[::2] = 255                                                  # clips on the way
            src[1::4] = 0
        assert np.array_equal(DM.lowpass5_plane(src, 0, 8), reference_row_walk(src)), k
    assert np.array_equal(DM.deinterlace([src], DM.LOWPASS5, 0, 8)[0], reference_row_walk(src).astype(np.uint8))


def test_blend_and_bob_against_numpy_expressions():
    rng = np.random.default_rng(7)
    for bd, (h, w) in itertools.product((8, 10), ((4, 8), (8, 16), (16, 24))):
        src = rng.integers(0, 1 << bd, (h, w)).astype(np.int64)
        pad = np.pad(src, ((1, 1), (0, 0)), mode="edge")
        assert np.array_equal(DM.blend_plane(src), (pad[:-2] + 2 * pad[1:-1] + pad[2:] + 2) >> 2)
        for parity in (0, 1):
            kept = src[parity::2]                                           # the mirrored neighbours of a missing row are kept rows
            above = kept if parity == 0 else np.concatenate((kept[:1], kept[:-1]))
            below = np.concatenate((kept[1:], kept[-1:])) if parity == 0 else kept
            want = src.copy()
            want[1 - parity::2] = (above + below + 1) >> 1
            assert np.array_equal(DM.bob_plane(src, parity), want), (bd, h, w, parity)
            assert np.array_equal(DM.bob_plane(src, parity)[parity::2], kept)
            assert np.array_equal(DM.lowpass5_plane(src, parity, bd)[parity::2], kept)


def test_weave_and_separate_model():
    rng = np.random.default_rng(3)
    t, b = rng.integers(0, 256, (4, 6), dtype=np.uint8), rng.integers(0, 256, (4, 6), dtype=np.uint8)
    d = DM.weave_plane(t, b)
    assert d.shape == (8, 6) and np.array_equal(d[0::2], t) and np.array_equal(d[1::2], b)
    t2, b2 = DM.separate_plane(d)
    assert np.array_equal(t2, t) and np.array_equal(b2, b)


def test_adaptive_passes_a_still_scene_through():
    rng = np.random.default_rng(11)
    for bd, (h, w) in itertools.product((8, 10), ((4, 8), (8, 16))):
        c = rng.integers(0, 1 << bd, (h, w))
        for parity, kf in itertools.product((0, 1), (0, 1)):
            assert np.array_equal(DM.adaptive_plane(c, c, c, parity, kf), c), (bd, h, w, parity, kf)
    # and does not where the scene moves
    assert not np.array_equal(DM.adaptive_plane(c, c, rng.integers(0, 1 << bd, c.shape), 0, 0), c)


def test_lowpass5_clips_both_ways():
    for bd in (8, 10, 12):
        M = (1 << bd) - 1
        for parity in (0, 1):
            y = 3 - parity                                                  # a missing row with all four neighbours inside
            high = np.full((8, 4), M)
            high[[y - 2, y + 2]] = 0                                        # (4 M + 2 M + 4 M + 4) >> 3 = (10 M + 4) >> 3 > M
            low = np.zeros((8, 4), int)
            low[[y - 2, y + 2]] = M                                         # (-2 M + 4) >> 3 < 0
            assert (10 * M + 4) >> 3 > M and (-2 * M + 4) >> 3 < 0
            assert (DM.lowpass5_plane(high, parity, bd)[y] == M).all() and (DM.lowpass5_plane(low, parity, bd)[y] == 0).all()


# ---------------- oh_deint_adaptive against the model ----------------
def _host(L, up, dn, rest):
    return L.oh_deint_adaptive((C.c_int32 * 7)(*up), (C.c_int32 * 7)(*dn), *rest)


def test_adaptive_function_against_the_model_on_random_windows():
    L = E.lib()
    seen_j, seen_o = set(), set()
    for bd in (8, 10, 12):
        rng = np.random.default_rng(1000 + bd)
        v = rng.integers(0, 1 << bd, (7000, 20)).tolist()
        # windows near an edge: up and dn equal but for a shift, so that the slanted directions win
        for k in range(0, 7000, 5):
            s = (k // 5) % 5 - 2
            for i in range(7):
                v[k][7 + i] = v[k][min(max(i + 2 * s, 0), 6)]
        for row in v:
            want, js, oc, _ = DM.adaptive_sample(row[:7], row[7:14], *row[14:])
            assert _host(L, row[:7], row[7:14], row[14:]) == want, (bd, row)
            seen_j.add(js)
            seen_o.add(oc)
    assert seen_j == {-2, -1, 0, 1, 2} and seen_o == {-1, 0, 1}
    assert E.deint_adaptive(v[0][:7], v[0][7:14], *v[0][14:]) == DM.adaptive_sample(v[0][:7], v[0][7:14], *v[0][14:])[0]
    with pytest.raises(ValueError):
        E.deint_adaptive([0] * 6, [0] * 7, 0, 0, 0, 0, 0, 0)


def test_adaptive_function_on_windows_of_extremes():
    """every up / dn window made of 0 and M (2^14), the six temporal samples running through their 64 patterns beside them; then every
    temporal pattern beside sixteen windows, at 12 bit"""
    L = E.lib()
    M = 255
    for k in range(1 << 14):
        up = [M * (k >> i & 1) for i in range(7)]
        dn = [M * (k >> (7 + i) & 1) for i in range(7)]
        rest = [M * ((k * 37 + (k >> 6)) >> i & 1) for i in range(6)]
        want = DM.adaptive_sample(up, dn, *rest)[0]
        assert _host(L, up, dn, rest) == want and 0 <= want <= M, (up, dn, rest)
    M = 4095
    for t, k in itertools.product(range(64), range(16)):
        up = [M * (k & 1), M * (k >> 1 & 1), M * (k & 1), M * (k >> 1 & 1), 0, M, M * (k & 1)]
        dn = [M * (k >> 2 & 1), M * (k >> 3 & 1), M, M * (k >> 2 & 1), M * (k >> 3 & 1), 0, M * (k >> 2 & 1)]
        rest = [M * (t >> i & 1) for i in range(6)]
        want = DM.adaptive_sample(up, dn, *rest)[0]
        assert _host(L, up, dn, rest) == want and 0 <= want <= M, (up, dn, rest)


# ---------------- what the GPU tests' planes make the model do ----------------
@pytest.mark.parametrize("w,h", ((16, 8), (24, 16)))
@pytest.mark.parametrize("bd", (8, 10))
def test_gpu_test_planes_cover_every_branch_of_adaptive(bd, w, h):
    """the luma planes of tests/test_gpu_deinterlace.py (random_triplet) take each of the five j*, each clamp outcome and each of the
    three diff terms as the strict maximum, over the four combinations of parity and kept_first: so that a change of seed cannot hollow
    the GPU test out"""
    P, Cu, N = (pic[0] for pic in DM.random_triplet(bd, w, h, 0))
    assert np.array_equal(DM.random_triplet(bd, w, h, 1)[1][0], Cu)            # the luma planes do not depend on the chroma format
    js, oc, wh = {}, {}, {}
    for parity, kf in itertools.product((0, 1), (0, 1)):
        _, j, o, t = DM.adaptive_plane(P, Cu, N, parity, kf, detail=True)
        miss = np.arange(h) % 2 != parity
        for d, arr in ((js, j), (oc, o), (wh, t)):
            for v in arr[miss].ravel().tolist():
                d[v] = d.get(v, 0) + 1
    assert all(js.get(v, 0) >= 1 for v in (-2, -1, 0, 1, 2)), js
    assert all(oc.get(v, 0) >= 1 for v in (-1, 0, 1)), oc
    assert all(wh.get(v, 0) >= 1 for v in (0, 1, 2)), wh
    assert sum(js.values()) == 4 * (h // 2) * w


# ---------------- oh_field_info ----------------
TABLE_D2 = {  # pic_struct: (kind, pair, top_first, repeat_first, frames)
    0: (0, 0, -1, 0, 1), 1: (1, 0, -1, 0, 1), 2: (2, 0, -1, 0, 1), 3: (0, 0, 1, 0, 1), 4: (0, 0, 0, 0, 1), 5: (0, 0, 1, 1, 1),
    6: (0, 0, 0, 1, 1), 7: (0, 0, -1, 0, 2), 8: (0, 0, -1, 0, 3), 9: (1, -1, -1, 0, 1), 10: (2, -1, -1, 0, 1), 11: (1, 1, -1, 0, 1),
    12: (2, 1, -1, 0, 1)}


def test_field_info():
    L = E.lib()
    for s, want in TABLE_D2.items():
        fi = E.OhFieldInfo()
        assert L.oh_field_info(s, C.byref(fi)) == 0
        assert (fi.kind, fi.pair, fi.top_first, fi.repeat_first, fi.frames) == want, s
        got = E.field_info(s)
        assert tuple(got) == want and got.kind == want[0] and got.frames == want[4]
    fi = E.OhFieldInfo(7, 7, 7, 7, 7)
    for bad in (13, 14, 15, -1, 1 << 20):
        assert L.oh_field_info(bad, C.byref(fi)) == E.OH_E_ARG, bad
        with pytest.raises(E.EngineError) as ei:
            E.field_info(bad)
        assert ei.value.code == E.OH_E_ARG
    assert L.oh_field_info(3, None) == E.OH_E_ARG
    assert (fi.kind, fi.pair, fi.top_first, fi.repeat_first, fi.frames) == (7, 7, 7, 7, 7)
    assert (E.FIELD_FRAME, E.FIELD_TOP, E.FIELD_BOTTOM) == (0, 1, 2)


# ---------------- the picture timing SEI ----------------
PPS, SEI_P, SEI_S = 34, 39, 40
TYPE = 1


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


def timing(pic_struct, scan=0, dup=0, tail=b""):
    """pic_struct u(4), source_scan_type u(2), duplicate_flag u(1), then one bit of whatever follows (here the alignment bit)"""
    return msg(TYPE, bytes([(pic_struct << 4) | (scan << 2) | (dup << 1) | 1]) + tail)


def raw(n, flag=1):
    d = A.OhPicTiming()
    return A.lib().oh_sei_pic_timing(n, len(n), flag, C.byref(d)), d


def test_pic_timing_every_pic_struct():
    for s, scan, dup in itertools.product(range(13), range(3), (0, 1)):
        n = nal(SEI_P, escape(timing(s, scan, dup) + b"\x80"))
        assert A.pic_timing(n) == dict(pic_struct=s, source_scan_type=scan, duplicate_flag=dup), (s, scan, dup)
        rc, d = raw(n)
        assert rc == 1 and (d.present, d.pic_struct, d.source_scan_type, d.duplicate_flag) == (1, s, scan, dup)
        assert tuple(E.field_info(A.pic_timing(n)["pic_struct"])) == TABLE_D2[s]
    # the HRD fields that may follow are not read
    n = nal(SEI_P, escape(timing(9, 1, 1, tail=b"\x12\x34\x56\x78") + b"\x80"))
    assert A.pic_timing(n) == dict(pic_struct=9, source_scan_type=1, duplicate_flag=1)
    # reserved values come out as coded; oh_field_info refuses them
    assert A.pic_timing(nal(SEI_P, escape(timing(15, 3, 1) + b"\x80"))) == dict(pic_struct=15, source_scan_type=3, duplicate_flag=1)


def test_pic_timing_without_frame_field_info():
    for body in (timing(11, 1, 1), msg(TYPE, b"\x12\x34"), msg(TYPE, b"")):
        n = nal(SEI_P, escape(body + b"\x80"))
        assert A.pic_timing(n, frame_field_info_present=False) == dict(pic_struct=-1, source_scan_type=-1, duplicate_flag=-1)
        rc, d = raw(n, 0)
        assert rc == 1 and (d.present, d.pic_struct, d.source_scan_type, d.duplicate_flag) == (1, -1, -1, -1)


def test_pic_timing_suffix_sei_is_passed_over():
    n = nal(SEI_S, escape(timing(11) + b"\x80"))
    rc, d = raw(n)
    assert rc == 0 and A.pic_timing(n) is None
    assert (d.present, d.pic_struct, d.source_scan_type, d.duplicate_flag) == (0, 0, 0, 0)
    assert A.pic_timing(nal(SEI_P, escape(msg(5, b"\x01\x02\x03") + b"\x80"))) is None


def test_pic_timing_last_of_two_counts_and_other_readers_walk_the_same_messages():
    n = nal(SEI_P, escape(timing(11, 0, 1) + timing(10, 1, 0) + b"\x80"))
    assert A.pic_timing(n) == dict(pic_struct=10, source_scan_type=1, duplicate_flag=0)
    both = nal(SEI_P, escape(msg(144, b"\x03\xe8\x01\x90") + timing(2) + b"\x80"))
    assert A.pic_timing(both)["pic_struct"] == 2 and A.hdr_sei(both) == dict(max_cll=1000, max_fall=400)


def test_pic_timing_behind_a_message_that_needs_emulation_prevention():
    body = msg(5, b"\x00\x00\x01\x00\x00\x00") + timing(12, 2, 1) + b"\x80"
    n = nal(SEI_P, escape(body))
    assert len(n) == 2 + len(body) + 2 and b"\x00\x00\x03\x01\x00\x00\x03\x00" in n
    assert A.pic_timing(n) == dict(pic_struct=12, source_scan_type=2, duplicate_flag=1)
    # pic_struct 0, interlaced, no duplicate: the payload byte is 0x01, behind a size byte of 1 — never two zero bytes in front of it
    assert escape(timing(0)) == timing(0)


def test_pic_timing_malformed():
    whole = timing(11, 1, 0, tail=b"\x55")
    assert raw(nal(SEI_P, escape(whole[:-1])))[0] == -1                      # announces two bytes and the unit ends
    assert raw(nal(SEI_P, escape(msg(TYPE, b"") + b"\x80")))[0] == -1        # the flag is set and the payload is empty
    rc, d = raw(nal(SEI_P, escape(timing(11) + msg(TYPE, b"") + b"\x80")))
    assert rc == -1 and (d.present, d.pic_struct) == (0, 0)                  # nothing of a malformed unit is reported
    assert raw(nal(PPS, escape(whole + b"\x80")))[0] == -1
    assert raw(nal(SEI_P)[:2])[0] == -1
    with pytest.raises(ValueError):
        A.pic_timing(nal(PPS, escape(whole + b"\x80")))
    with pytest.raises(ValueError):
        A.pic_timing(nal(SEI_P, escape(whole[:-1])))


# ---------------- names and constants ----------------
def test_names_and_constants():
    assert (E.DEINT_BOB, E.DEINT_BLEND, E.DEINT_LOWPASS5, E.DEINT_ADAPTIVE) == (DM.BOB, DM.BLEND, DM.LOWPASS5, DM.ADAPTIVE) == (0, 1, 2, 3)
    assert E.DEINT_MODES == {"bob": 0, "blend": 1, "lowpass5": 2, "adaptive": 3}
    assert E.deint_mode("lowpass5") == 2 and E.deint_mode(3) == 3
    for bad in ("yadif", 4, -1):
        with pytest.raises(ValueError):
            E.deint_mode(bad)
    assert E.DEINT_SEG > 0 and E.DEINT_SEG % 16 == 0
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openhevc_amd", "csrc", "kernels.h")).read()
    assert f"OH_DI_SEG = {E.DEINT_SEG} " in src
    assert C.sizeof(E.OhDeinterlace) == 12 and C.sizeof(E.OhFieldInfo) == 20 and C.sizeof(A.OhPicTiming) == 16
    for name in ("pics_weave", "pics_separate", "pics_deinterlace"):
        assert callable(getattr(E.Engine, name))
    assert E.FieldInfo._fields == ("kind", "pair", "top_first", "repeat_first", "frames")
