"""What the Python wrappers of the picture-to-picture services (openhevc_amd/engine.py) share: the destinations of a call are `out`, or
pictures made for it that are freed again when an allocation fails or the library refuses.  The Engine here is made without a library
call; its pic_alloc, pic_free and the one library function a wrapper calls are stand-ins that record ids — no GPU, nothing preloaded."""
import types

import numpy as np
import pytest

from openhevc_amd import frame as F
from openhevc_amd.engine import Engine, EngineError

N = 3
SRC = [1, 2, 3]                                               # frames of 16 x 16, also the top fields of weave
BOTTOM = [4, 5, 6]


class Rig:
    """an Engine whose pictures are counted: alloc_fails_at: the allocation (from 1) that raises; rc: what the library function answers"""

    def __init__(self, name, alloc_fails_at=None, rc=0):
        e = self.e = object.__new__(Engine)
        e.h, e.device, e._torch_stream = None, 0, None
        e._params = {pid: F.pic_params(16, 16) for pid in SRC + BOTTOM + list(range(50, 53)) + list(range(70, 73))}
        self.made, self.freed, self.calls = [], [], 0

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

        def library_call(*args):
            self.calls += 1
            return rc

        e.pic_alloc, e.pic_free = pic_alloc, pic_free
        e.L = types.SimpleNamespace(oh_engine_last_error=lambda h: b"refused", **{name: library_call})


# name of the library function, the call with the destinations `out`, and what a given `out` of k pictures per list looks like
def _given(k):
    return list(range(50, 50 + k))


SERVICES = {
    "resize": ("oh_pics_resize", lambda e, out: e.pics_resize(SRC, (8, 8), out=out), _given),
    "reformat": ("oh_pics_reformat", lambda e, out: e.pics_reformat(SRC, bit_depth=10, out=out), _given),
    "orient": ("oh_pics_orient", lambda e, out: e.pics_orient(SRC, "rot90", out=out), _given),
    "weave": ("oh_pics_weave", lambda e, out: e.pics_weave(SRC, BOTTOM, out=out), _given),
    "separate": ("oh_pics_separate", lambda e, out: e.pics_separate(SRC, out=out), lambda k: (_given(k), list(range(70, 70 + k)))),
    "separate_top": ("oh_pics_separate", lambda e, out: e.pics_separate(SRC, bottom=False, out=out), lambda k: (_given(k), None)),
    "deinterlace": ("oh_pics_deinterlace", lambda e, out: e.pics_deinterlace(SRC, "adaptive", prev=[None, 1, 2], out=out), _given),
    "filter": ("oh_pics_filter", lambda e, out: e.pics_filter(SRC, "temporal", next=[2, 3, None], out=out), _given),
    "lut": ("oh_pics_lut", lambda e, out: e.pics_lut(SRC, np.arange(256, dtype=np.uint16), out=out), _given),
    "motion_compensate": ("oh_pics_motion_compensate", lambda e, out: e.pics_motion_compensate(SRC, np.zeros((N, 1, 1, 2), np.int16), out=out),
                          _given),
    "warp": ("oh_pics_warp", lambda e, out: e.pics_warp(SRC, [65536, 0, 0, 0, 65536, 0], (8, 8), out=out), _given),
}
ALL = pytest.mark.parametrize("service", sorted(SERVICES))


@ALL
def test_failed_allocation_frees_what_it_made(service):
    name, call, _ = SERVICES[service]
    rig = Rig(name, alloc_fails_at=3)
    with pytest.raises(EngineError, match="oh_pic_alloc"):
        call(rig.e, None)
    assert rig.made == [100, 101] and sorted(rig.freed) == rig.made and rig.calls == 0


@ALL
def test_refusal_frees_the_fresh_pictures(service):
    name, call, _ = SERVICES[service]
    rig = Rig(name, rc=-1)
    with pytest.raises(EngineError, match=name) as err:
        call(rig.e, None)
    assert err.value.code == -1 and rig.calls == 1
    assert len(rig.made) == (2 * N if service == "separate" else N) and sorted(rig.freed) == rig.made


@ALL
def test_fresh_pictures_are_returned(service):
    name, call, _ = SERVICES[service]
    rig = Rig(name)
    got = call(rig.e, None)
    ids = got[0] if service in ("resize", "orient", "warp") else got
    if service.startswith("separate"):
        ids = ids[0] + (ids[1] or [])
    assert ids == rig.made and rig.freed == [] and rig.calls == 1


@ALL
@pytest.mark.parametrize("rc", [0, -1])
def test_given_out_is_never_freed(service, rc):
    name, call, given = SERVICES[service]
    rig = Rig(name, rc=rc)
    if rc:
        with pytest.raises(EngineError, match=name):
            call(rig.e, given(N))
    else:
        call(rig.e, given(N))
    assert rig.made == [] and rig.freed == [] and rig.calls == 1


@ALL
def test_wrong_out_length_is_refused_before_any_allocation(service):
    name, call, given = SERVICES[service]
    rig = Rig(name)
    with pytest.raises(ValueError, match=f"out: {N - 1} pictures for {N}"):
        call(rig.e, given(N - 1))
    assert rig.made == [] and rig.freed == [] and rig.calls == 0
