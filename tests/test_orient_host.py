"""The host-only arithmetic of the picture orientation (include/ohevc_hip.h: oh_orient_then, oh_orient_inverse, oh_orient_size,
oh_orient_from_sei) and the numpy model the GPU tests compare against (tests/orient_model.py) — no GPU needed."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orient_model as OM                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

S = np.arange(15, dtype=np.uint16).reshape(3, 5) * 7 + 1                    # asymmetric: 5 wide, 3 high, every sample its own


def test_model_against_numpy():
    want = {0: S, 1: S[:, ::-1], 2: S[::-1], 3: np.rot90(S, 2), 4: S.T, 5: np.rot90(S, -1), 6: np.rot90(S, 1), 7: np.rot90(S, 2).T}
    for o, w in want.items():
        got = OM.orient_plane(S, o)
        assert got.shape == w.shape and np.array_equal(got, w), o
    images = [OM.orient_plane(S, o).tobytes() + bytes(OM.orient_plane(S, o).shape) for o in range(8)]
    assert len(set(images)) == 8


def test_names_and_constants():
    assert (E.ORIENT_HFLIP, E.ORIENT_VFLIP, E.ORIENT_TRANSPOSE) == (OM.HFLIP, OM.VFLIP, OM.TRANSPOSE) == (1, 2, 4)
    assert E.ORIENTATIONS == {"identity": 0, "hflip": 1, "vflip": 2, "rot180": 3, "transpose": 4, "rot90": 5, "rot270": 6, "antitranspose": 7}
    assert np.array_equal(OM.orient_plane(S, E.orient_code("rot90")), np.rot90(S, -1))       # clockwise
    assert E.orient_code("rot270") == 6 and E.orient_code(3) == 3
    for bad in ("rot45", 8, -1):
        with pytest.raises(ValueError):
            E.orient_code(bad)
    assert E.ORIENT_TILE > 0


def test_then_all_pairs():
    """oh_orient_then(a, b) is the one orientation whose image of S is b's image of a's image of S; the eight images are distinct, so
    the model yields exactly one answer per pair"""
    images = [OM.orient_plane(S, o) for o in range(8)]
    L = E.lib()
    for a, b in itertools.product(range(8), range(8)):
        twice = OM.orient_plane(images[a], b)
        match = [o for o in range(8) if images[o].shape == twice.shape and np.array_equal(images[o], twice)]
        assert len(match) == 1
        assert L.oh_orient_then(a, b) == match[0] == E.orient_then(a, b), (a, b)
    for a in range(8):
        assert sorted(E.orient_then(a, b) for b in range(8)) == list(range(8))
        assert sorted(E.orient_then(b, a) for b in range(8)) == list(range(8))
    for bad in ((8, 0), (0, 8), (-1, 3), (3, -1), (1 << 20, 0)):
        assert L.oh_orient_then(*bad) == -1
    assert E.orient_then("hflip", "vflip") == 3 and E.orient_then("rot90", "rot90") == 3 and E.orient_then("rot90", "rot270") == 0


def test_inverse():
    L = E.lib()
    for a in range(8):
        inv = L.oh_orient_inverse(a)
        assert 0 <= inv <= 7 and E.orient_inverse(a) == inv
        assert E.orient_then(a, inv) == 0 and E.orient_then(inv, a) == 0
        assert np.array_equal(OM.orient_plane(OM.orient_plane(S, a), inv), S)
    assert [E.orient_inverse(a) for a in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]
    assert L.oh_orient_inverse(8) == -1 and L.oh_orient_inverse(-1) == -1


def test_size():
    L = E.lib()
    for o in range(8):
        assert E.orient_size(o, 5, 3) == ((3, 5) if o & 4 else (5, 3)) == OM.orient_plane(S, o).shape[::-1]
    ow, oh = C.c_int(-7), C.c_int(-7)
    for bad in ((8, 5, 3), (-1, 5, 3), (0, 0, 3), (0, 5, 0), (4, -2, 3)):
        assert L.oh_orient_size(*bad, C.byref(ow), C.byref(oh)) == E.OH_E_ARG
    assert L.oh_orient_size(0, 5, 3, None, C.byref(oh)) == E.OH_E_ARG and L.oh_orient_size(0, 5, 3, C.byref(ow), None) == E.OH_E_ARG
    assert (ow.value, oh.value) == (-7, -7)
    with pytest.raises(E.EngineError):
        E.orient_size(0, 0, 3)


def test_from_sei():
    """the flips first, then k quarter turns anticlockwise of the flipped picture"""
    L = E.lib()
    images = [OM.orient_plane(S, o) for o in range(8)]
    seen = set()
    for hf, vf, k in itertools.product((0, 1), (0, 1), range(4)):
        want = S
        if hf:
            want = want[:, ::-1]
        if vf:
            want = want[::-1]
        want = np.rot90(want, k)
        o = C.c_int(-1)
        assert L.oh_orient_from_sei(hf, vf, k << 14, C.byref(o)) == 0
        assert 0 <= o.value <= 7 and np.array_equal(images[o.value], want), (hf, vf, k)
        assert E.orientation_from_sei(hf, vf, k << 14) == o.value
        seen.add(o.value)
    assert seen == set(range(8))
    o = C.c_int(-1)
    for rot in (0x2000, 1, 0x4001, 0xFFFF, 0x3FFF):
        assert L.oh_orient_from_sei(0, 0, rot, C.byref(o)) == E.OH_E_UNSUPPORTED, rot
    for bad in ((2, 0, 0), (0, 2, 0), (-1, 0, 0), (0, -1, 0x4000), (0, 0, 0x10000), (1, 1, 0x14000)):
        assert L.oh_orient_from_sei(*bad, C.byref(o)) == E.OH_E_ARG, bad
    assert L.oh_orient_from_sei(0, 0, 0, None) == E.OH_E_ARG
    assert o.value == -1
    with pytest.raises(E.EngineError) as ei:
        E.orientation_from_sei(0, 0, 0x2000)
    assert ei.value.code == E.OH_E_UNSUPPORTED
