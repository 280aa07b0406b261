"""Engine.pics_grain follows the rule that the Python wrappers of the picture-to-picture services share (the technique of
tests/test_warp_wrappers_host.py): the destinations are `out`, or pictures made for the call that are freed again when an allocation
fails or the library refuses.  The Engine here is made without a library call; its pic_alloc, pic_free and the library function are
stand-ins that record what they get — no GPU, nothing preloaded.  Also the seeds a call may take, the texts of the blending enum, and
what the wrapper refuses itself, before any allocation."""
import ctypes as C
import types

import numpy as np
import pytest

from openhevc_amd import frame as F
from openhevc_amd.engine import (GRAIN_BLENDINGS, Engine, EngineError, Grain, OhGrain, grain_from_sei, grain_seeds, make_grain)

N = 3
SRC = [1, 2, 3]                                                # pictures of 24 x 16


class Rig:
    """an Engine whose pictures are counted: alloc_fails_at: the allocation (from 1) that raises; rc: what the library function answers"""

    def __init__(self, alloc_fails_at=None, rc=0):
        e = self.e = object.__new__(Engine)
        e.h, e.device, e._torch_stream = None, 0, None
        e._params = {pid: F.pic_params(24, 16) for pid in SRC + list(range(50, 53))}
        self.made, self.freed, self.calls, self.grains = [], [], 0, []

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

        def library_call(h, src, dst, n, gp, seeds):
            self.calls += 1
            g = C.cast(gp, C.POINTER(OhGrain)).contents
            self.grains.append(dict(planes=g.planes, blending=g.blending, log2_scale=g.log2_scale,
                                    tables=[np.ctypeslib.as_array(g.table[c], (256,)).copy() for c in range(3)],
                                    seeds=[seeds[i] for i in range(n)], src=list(src), dst=list(dst), n=n))
            return rc

        e.pic_alloc, e.pic_free = pic_alloc, pic_free
        e.L = types.SimpleNamespace(oh_engine_last_error=lambda h: b"refused", oh_pics_grain=library_call)


def test_failed_allocation_frees_what_it_made():
    rig = Rig(alloc_fails_at=3)
    with pytest.raises(EngineError, match="oh_pic_alloc"):
        rig.e.pics_grain(SRC, make_grain(10), 0)
    assert rig.made == [100, 101] and sorted(rig.freed) == rig.made and rig.calls == 0


def test_refusal_frees_the_fresh_pictures():
    rig = Rig(rc=-2)
    with pytest.raises(EngineError, match="oh_pics_grain") as err:
        rig.e.pics_grain(SRC, make_grain(10), 0)
    assert err.value.code == -2 and rig.calls == 1
    assert len(rig.made) == N and sorted(rig.freed) == rig.made


def test_fresh_pictures_are_returned_and_the_grain_arrives():
    rig = Rig()
    grain = make_grain(33, 4, 12, log2_scale=6, blending="multiplicative", planes=5)
    ids = rig.e.pics_grain(SRC, grain, [9, 8, 7])
    assert ids == rig.made and len(ids) == N and rig.freed == [] and rig.calls == 1
    g = rig.grains[0]
    assert (g["planes"], g["blending"], g["log2_scale"], g["seeds"], g["src"], g["dst"], g["n"]) == (5, 1, 6, [9, 8, 7], SRC, ids, N)
    assert all((t == 33 | 4 << 8 | 12 << 12).all() for t in g["tables"])
    assert rig.e._params[ids[0]].width == 24 and rig.e._params[ids[0]].height == 16      # the sources' params
    rig.e.pics_grain(SRC, grain, 5, planes=2)                   # planes of the call, not of the grain
    assert rig.grains[1]["planes"] == 2 and grain.planes == 5


@pytest.mark.parametrize("rc", [0, -2])
def test_given_out_is_never_freed(rc):
    rig = Rig(rc=rc)
    if rc:
        with pytest.raises(EngineError, match="oh_pics_grain"):
            rig.e.pics_grain(SRC, make_grain(10), 0, out=[50, 51, 52])
    else:
        assert rig.e.pics_grain(SRC, make_grain(10), 0, out=[50, 51, 52]) == [50, 51, 52]
    assert rig.made == [] and rig.freed == [] and rig.calls == 1


def test_seeds():
    """a sequence is taken as it is, one int b stands for b + i; both modulo 2^32"""
    assert list(grain_seeds([5, 5, 2 ** 32 + 1, -1], 4)) == [5, 5, 1, 0xFFFFFFFF] and grain_seeds([], 0).size == 0
    assert list(grain_seeds(7, 3)) == [7, 8, 9] and list(grain_seeds(0xFFFFFFFE, 4)) == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1]
    assert list(grain_seeds(np.array([3, 4], np.int64), 2)) == [3, 4] and grain_seeds(1, 2).dtype == np.uint32
    with pytest.raises(ValueError):
        grain_seeds([1, 2], 3)
    rig = Rig()
    rig.e.pics_grain(SRC, make_grain(1), 40)
    rig.e.pics_grain(SRC, make_grain(1), (40, 40, 41))
    assert rig.grains[0]["seeds"] == [40, 41, 42] and rig.grains[1]["seeds"] == [40, 40, 41]
    assert rig.e.pics_grain([], make_grain(1), []) == [] and rig.e.pics_grain([], make_grain(1), 3) == [] and rig.calls == 2
    assert rig.e.pics_grain([], make_grain(1), 3, out=[]) == [] and rig.calls == 3 and rig.grains[2]["n"] == 0


def test_enum_texts_and_grain_objects():
    assert GRAIN_BLENDINGS == {"additive": 0, "multiplicative": 1}
    assert make_grain(1, blending="additive").blending == 0 and make_grain(1, blending=1).blending == 1
    with pytest.raises(ValueError, match="blending"):
        make_grain(1, blending="overlay")
    t = np.zeros((3, 256), np.int64)
    t[1, 5] = 0xFFFFFFFF
    g = Grain(t, 3, "multiplicative", 4)
    assert g.tables.dtype == np.uint32 and g.tables[1, 5] == 0xFFFFFFFF and (g.planes, g.blending, g.log2_scale) == (3, 1, 4)
    s = g.as_struct()
    assert (s.planes, s.blending, s.log2_scale) == (3, 1, 4) and s.table[1][5] == 0xFFFFFFFF and g.as_struct(6).planes == 6
    for bad in (np.zeros((2, 256)), np.zeros((3, 255), int), np.zeros((3, 256)), np.full((3, 256), -1), np.full((3, 256), 1 << 32)):
        with pytest.raises(ValueError):
            Grain(bad)
    d = dict(cancel=False, model_id=0, colour=None, blending_mode_id=1, log2_scale_factor=2, persistence=True,
             components=[[(0, 255, [10])], None, None])
    g = grain_from_sei(d)
    assert (g.planes, g.blending, g.log2_scale) == (1, 1, 2) and (g.tables[0] == 10 | 8 << 8 | 8 << 12).all() and not g.tables[1:].any()


def test_what_the_wrapper_refuses_itself():
    rig = Rig()
    grain = make_grain(10)
    bad = [lambda: rig.e.pics_grain(SRC, grain.tables, 0),                                  # tables are no Grain
           lambda: rig.e.pics_grain(SRC, None, 0),
           lambda: rig.e.pics_grain(SRC, grain, [1, 2]),                                    # two seeds for three pictures
           lambda: rig.e.pics_grain(SRC, grain, "poc"),
           lambda: rig.e.pics_grain(SRC, grain, 0, out=[50, 51])]
    for call in bad:
        with pytest.raises((ValueError, TypeError)):
            call()
    assert rig.made == [] and rig.freed == [] and rig.calls == 0


def test_what_the_library_refuses_frees_the_fresh_pictures():
    """the wrapper leaves planes, log2_scale and the entries to the library: its refusal frees what was made"""
    rig = Rig(rc=-2)
    with pytest.raises(EngineError, match="oh_pics_grain"):
        rig.e.pics_grain(SRC, make_grain(10, log2_scale=16), 0, planes=9)
    assert rig.calls == 1 and rig.grains[0]["planes"] == 9 and rig.grains[0]["log2_scale"] == 16
    assert len(rig.made) == N and sorted(rig.freed) == rig.made
