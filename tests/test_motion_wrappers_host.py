"""Engine.pics_motion_compensate follows the rule that the Python wrappers of the picture-to-picture services share (the technique of
tests/test_engine_wrappers_host.py): the destinations are `out`, or pictures made for the call that are freed again when an allocation
fails or the library refuses.  The Engine here is made without a library call; its pic_alloc, pic_free and the library function are
stand-ins that record ids — no GPU, nothing preloaded.  Also what the wrappers refuse themselves, before any allocation."""
import types

import numpy as np
import pytest

from openhevc_amd import frame as F
from openhevc_amd.engine import MOTION_DTYPE, Engine, EngineError

N = 3
REF = [1, 2, 3]                                                # pictures of 24 x 16: 2 x 1 blocks of 16, 3 x 2 of 8


class Rig:
    """an Engine whose pictures are counted: alloc_fails_at: the allocation (from 1) that raises; rc: what the library function answers"""

    def __init__(self, alloc_fails_at=None, rc=0):
        e = self.e = object.__new__(Engine)
        e.h, e.device, e._torch_stream = None, 0, None
        e._params = {pid: F.pic_params(24, 16) for pid in REF + list(range(50, 53))}
        self.made, self.freed, self.calls, self.blocks = [], [], 0, []

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

        def library_call(h, ref, dst, n, block, field):
            self.calls += 1
            self.blocks.append(block)
            return rc

        e.pic_alloc, e.pic_free = pic_alloc, pic_free
        e.L = types.SimpleNamespace(oh_engine_last_error=lambda h: b"refused", oh_pics_motion_compensate=library_call)


def field(block=16, n=N):
    return np.zeros((n, 1, 2) if block == 16 else (n, 2, 3), dtype=MOTION_DTYPE)


def test_failed_allocation_frees_what_it_made():
    rig = Rig(alloc_fails_at=3)
    with pytest.raises(EngineError, match="oh_pic_alloc"):
        rig.e.pics_motion_compensate(REF, field())
    assert rig.made == [100, 101] and sorted(rig.freed) == rig.made and rig.calls == 0


def test_refusal_frees_the_fresh_pictures():
    rig = Rig(rc=-1)
    with pytest.raises(EngineError, match="oh_pics_motion_compensate") as err:
        rig.e.pics_motion_compensate(REF, field())
    assert err.value.code == -1 and rig.calls == 1
    assert len(rig.made) == N and sorted(rig.freed) == rig.made


@pytest.mark.parametrize("block", (8, 16))
def test_fresh_pictures_are_returned(block):
    rig = Rig()
    assert rig.e.pics_motion_compensate(REF, field(block), block=block) == rig.made
    assert len(rig.made) == N and rig.freed == [] and rig.calls == 1 and rig.blocks == [block]


@pytest.mark.parametrize("rc", [0, -1])
def test_given_out_is_never_freed(rc):
    rig = Rig(rc=rc)
    if rc:
        with pytest.raises(EngineError, match="oh_pics_motion_compensate"):
            rig.e.pics_motion_compensate(REF, field(), out=[50, 51, 52])
    else:
        assert rig.e.pics_motion_compensate(REF, field(), out=[50, 51, 52]) == [50, 51, 52]
    assert rig.made == [] and rig.freed == [] and rig.calls == 1


def test_wrong_out_length_is_refused_before_any_allocation():
    rig = Rig()
    with pytest.raises(ValueError, match=f"out: {N - 1} pictures for {N}"):
        rig.e.pics_motion_compensate(REF, field(), out=[50, 51])
    assert rig.made == [] and rig.freed == [] and rig.calls == 0


def test_what_the_wrapper_refuses_itself():
    rig = Rig()
    with pytest.raises(ValueError, match="a field of shape"):
        rig.e.pics_motion_compensate(REF, field(8), block=16)             # the grid of another block size
    with pytest.raises(ValueError, match="a field of shape"):
        rig.e.pics_motion_compensate(REF, field(16, n=2))
    with pytest.raises(ValueError, match="at least one picture"):
        rig.e.pics_motion_compensate([], field(16, n=0))
    with pytest.raises(ValueError, match="int16"):
        rig.e.pics_motion_compensate(REF, np.full((N, 1, 2, 2), 40000))
    assert rig.made == [] and rig.freed == [] and rig.calls == 0
    # (x, y) pairs in place of a structured field
    assert rig.e.pics_motion_compensate(REF, np.zeros((N, 1, 2, 2), dtype=np.int64)) == rig.made and rig.calls == 1


def test_a_block_size_the_library_refuses_frees_the_fresh_pictures():
    """the wrapper leaves the block size to the library: its refusal frees what was made"""
    rig = Rig(rc=-1)
    with pytest.raises(EngineError, match="oh_pics_motion_compensate"):
        rig.e.pics_motion_compensate(REF, field(), block=12)
    assert rig.calls == 1 and rig.blocks == [12] and len(rig.made) == N and sorted(rig.freed) == rig.made
