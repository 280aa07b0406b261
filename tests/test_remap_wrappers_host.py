"""Engine.pics_colour_remap follows the rule that the Python wrappers of the picture-to-picture services share (the technique of
tests/test_grain_wrappers_host.py): the destinations are `out`, or pictures made for the call — with the sources' params at the remap's
output depth — that are freed again when an allocation fails or the library refuses.  The Engine here is made without a library call;
its pic_alloc, pic_free and the library function are stand-ins that record what they get — no GPU, nothing preloaded.  Also what
make_remap takes for its tables, and what the wrappers refuse themselves, before any allocation."""
import ctypes as C
import types

import numpy as np
import pytest

from openhevc_amd import frame as F
from openhevc_amd.engine import Engine, EngineError, OhRemap, Remap, make_remap, remap_curve, remap_from_sei

N = 3
SRC = [1, 2, 3]                                                # pictures of 24 x 16, 10 bit, 4:4:4


class Rig:
    """an Engine whose pictures are counted: alloc_fails_at: the allocation (from 1) that raises; rc: what the library function answers"""

    def __init__(self, alloc_fails_at=None, rc=0):
        e = self.e = object.__new__(Engine)
        e.h, e.device, e._torch_stream = None, 0, None
        e._params = {pid: F.pic_params(24, 16, bit_depth=10, chroma_format_idc=3) for pid in SRC + list(range(50, 53))}
        self.made, self.freed, self.calls, self.remaps = [], [], 0, []

        def pic_alloc(params):
            if alloc_fails_at == len(self.made) + 1:
                raise EngineError("oh_pic_alloc failed (-2): no memory")
            pid = 100 + len(self.made)
            self.made.append(pid)
            e._params[pid] = F.OhPicParams.from_buffer_copy(params)
            return pid

        def pic_free(pid):
            self.freed.append(pid)
            e._params.pop(pid, None)

        def library_call(h, src, dst, n, rp):
            self.calls += 1
            r = C.cast(rp, C.POINTER(OhRemap)).contents
            self.remaps.append(dict(depths=(r.in_bit_depth, r.out_bit_depth), log2_denom=r.log2_denom,
                                    coeff=[[r.coeff[c][i] for i in range(3)] for c in range(3)],
                                    pre=[np.ctypeslib.as_array(r.pre[c], (1 << r.in_bit_depth,)).copy() for c in range(3)],
                                    post=[np.ctypeslib.as_array(r.post[c], (1 << r.out_bit_depth,)).copy() for c in range(3)],
                                    src=list(src), dst=list(dst), n=n))
            return rc

        e.pic_alloc, e.pic_free = pic_alloc, pic_free
        e.L = types.SimpleNamespace(oh_engine_last_error=lambda h: b"refused", oh_pics_colour_remap=library_call)


REMAP = make_remap(None, [[1, 2, 3], [4, 5, 6], [7, 8, -9]], 4, None, 10, 8)


def test_failed_allocation_frees_what_it_made():
    rig = Rig(alloc_fails_at=3)
    with pytest.raises(EngineError, match="oh_pic_alloc"):
        rig.e.pics_colour_remap(SRC, REMAP)
    assert rig.made == [100, 101] and sorted(rig.freed) == rig.made and rig.calls == 0


def test_refusal_frees_the_fresh_pictures():
    rig = Rig(rc=-4)
    with pytest.raises(EngineError, match="oh_pics_colour_remap") as err:
        rig.e.pics_colour_remap(SRC, REMAP)
    assert err.value.code == -4 and rig.calls == 1
    assert len(rig.made) == N and sorted(rig.freed) == rig.made


def test_fresh_pictures_have_the_output_depth_and_the_remap_arrives():
    rig = Rig()
    ids = rig.e.pics_colour_remap(SRC, REMAP)
    assert ids == rig.made and len(ids) == N and rig.freed == [] and rig.calls == 1
    p = rig.e._params[ids[0]]
    assert (p.width, p.height, p.bit_depth, p.chroma_format_idc) == (24, 16, 8, 3)      # the sources' params at the output depth
    assert rig.e._params[SRC[0]].bit_depth == 10                                        # which stay as they were
    r = rig.remaps[0]
    assert (r["depths"], r["log2_denom"], r["coeff"], r["src"], r["dst"], r["n"]) == ((10, 8), 4, [[1, 2, 3], [4, 5, 6], [7, 8, -9]], SRC, ids, N)
    assert all(np.array_equal(t, remap_curve(10, 8)) for t in r["pre"]) and all(np.array_equal(t, np.arange(256)) for t in r["post"])


@pytest.mark.parametrize("rc", [0, -2])
def test_given_out_is_never_freed(rc):
    rig = Rig(rc=rc)
    if rc:
        with pytest.raises(EngineError, match="oh_pics_colour_remap"):
            rig.e.pics_colour_remap(SRC, REMAP, out=[50, 51, 52])
    else:
        assert rig.e.pics_colour_remap(SRC, REMAP, out=[50, 51, 52]) == [50, 51, 52]
    assert rig.made == [] and rig.freed == [] and rig.calls == 1


def test_no_pictures():
    rig = Rig()
    assert rig.e.pics_colour_remap([], REMAP) == [] and rig.calls == 0
    assert rig.e.pics_colour_remap([], REMAP, out=[]) == [] and rig.calls == 1 and rig.remaps[0]["n"] == 0      # the library checks the struct


def test_make_remap_tables():
    """None, one table or pivot list for all three components, or three of them"""
    ramp = np.arange(256)
    r = make_remap(None, None, 5, None, 8)
    assert (r.in_bit_depth, r.out_bit_depth, r.log2_denom) == (8, 8, 5) and r.coeff.tolist() == [[32, 0, 0], [0, 32, 0], [0, 0, 32]]
    assert all(np.array_equal(t, ramp) for t in list(r.pre) + list(r.post)) and r.pre.dtype == np.uint16 and r.coeff.dtype == np.int32
    pv = [(0, 255), (255, 0)]
    r = make_remap(pv, None, 0, [None, ramp[::-1], [(10, 20), (30, 5)]], 8)
    assert all(np.array_equal(t, ramp[::-1]) for t in r.pre) and np.array_equal(r.post[0], ramp) and np.array_equal(r.post[1], ramp[::-1])
    assert np.array_equal(r.post[2], remap_curve(8, 8, [(10, 20), (30, 5)]))
    r = make_remap(np.tile(ramp, (4, 1)).reshape(-1) >> 2, None, 0, np.stack([ramp, ramp, ramp[::-1]]), 10, 8)
    assert r.pre.shape == (3, 1024) and r.post.shape == (3, 256) and r.post[2, 0] == 255
    r = make_remap([[(1, 2), (3, 4)], [(5, 6), (7, 8)], [(9, 10), (11, 12)]], None, 0, [[(1, 2), (3, 4), (5, 6)]] * 3, 8)
    assert r.pre[1, 5] == 6 and r.pre[2, 11] == 12 and r.post[0, 5] == 6
    three_pivots = make_remap([(1, 2), (3, 4), (5, 6)], None, 0, None, 8)           # three pivots of one curve, not three curves
    assert all(np.array_equal(t, remap_curve(8, 8, [(1, 2), (3, 4), (5, 6)])) for t in three_pivots.pre)
    s = r.as_struct()
    assert (s.in_bit_depth, s.out_bit_depth, s.log2_denom, s.pre[1][5], s.coeff[2][2]) == (8, 8, 0, 6, 1)


def test_what_the_wrappers_refuse_themselves():
    rig = Rig()
    ramp = np.arange(256)
    bad = [lambda: rig.e.pics_colour_remap(SRC, REMAP.pre),                             # tables are no Remap
           lambda: rig.e.pics_colour_remap(SRC, None),
           lambda: rig.e.pics_colour_remap(SRC, REMAP, out=[50, 51]),
           lambda: Remap(np.zeros((3, 255), int), np.eye(3, dtype=int), 0, np.zeros((3, 256), int), 8),
           lambda: Remap(np.zeros((2, 256), int), np.eye(3, dtype=int), 0, np.zeros((3, 256), int), 8),
           lambda: Remap(np.zeros((3, 256)), np.eye(3, dtype=int), 0, np.zeros((3, 256), int), 8),          # floats
           lambda: Remap(np.full((3, 256), -1), np.eye(3, dtype=int), 0, np.zeros((3, 256), int), 8),
           lambda: Remap(np.full((3, 256), 65536), np.eye(3, dtype=int), 0, np.zeros((3, 256), int), 8),
           lambda: Remap(np.zeros((3, 256), int), np.eye(3, dtype=int), 0, np.zeros((3, 256), int), 8, 10),  # post of 256 entries at 10 bit
           lambda: Remap(np.zeros((3, 256), int), np.eye(2, dtype=int), 0, np.zeros((3, 256), int), 8),
           lambda: Remap(np.zeros((3, 256), int), np.eye(3), 0, np.zeros((3, 256), int), 8),                 # a float matrix
           lambda: Remap(np.zeros((3, 256), int), np.eye(3, dtype=np.int64) << 40, 0, np.zeros((3, 256), int), 8),
           lambda: make_remap(ramp[:100], None, 0, None, 8),
           lambda: remap_from_sei(None)]
    for call in bad:
        with pytest.raises((ValueError, TypeError)):
            call()
    assert rig.made == [] and rig.freed == [] and rig.calls == 0


def test_what_the_library_refuses_frees_the_fresh_pictures():
    """the wrapper leaves the depths, log2_denom, the coefficients' range and the entries to the library: its refusal frees what was made"""
    rig = Rig(rc=-2)
    r = Remap(np.full((3, 1024), 4095), np.full((3, 3), 40000), 16, np.zeros((3, 256), int), 10, 8)
    with pytest.raises(EngineError, match="oh_pics_colour_remap"):
        rig.e.pics_colour_remap(SRC, r)
    assert rig.calls == 1 and rig.remaps[0]["log2_denom"] == 16 and rig.remaps[0]["coeff"][1][1] == 40000
    assert len(rig.made) == N and sorted(rig.freed) == rig.made
