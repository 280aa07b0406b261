"""Engine.pics_warp follows the rule that the Python wrappers of the picture-to-picture services share (the technique of
tests/test_motion_wrappers_host.py): the destinations are `out`, or pictures made for the call that are freed again when an allocation
fails or the library refuses.  The Engine here is made without a library call; its pic_alloc, pic_free and the library function are
stand-ins that record what they get — no GPU, nothing preloaded.  Also the forms a matrix may take, the rounding of a float matrix, and
what the wrapper refuses itself, before any allocation."""
import ctypes as C
import types

import numpy as np
import pytest

from openhevc_amd import frame as F
from openhevc_amd.engine import Engine, EngineError, OhWarp, warp_matrix

N = 3
SRC = [1, 2, 3]                                                # pictures of 24 x 16
ONE, ONE30 = 1 << 16, 1 << 30
IDENT = [ONE, 0, 0, 0, ONE, 0, 0, 0, ONE30]


class Rig:
    """an Engine whose pictures are counted: alloc_fails_at: the allocation (from 1) that raises; rc: what the library function answers"""

    def __init__(self, alloc_fails_at=None, rc=0):
        e = self.e = object.__new__(Engine)
        e.h, e.device, e._torch_stream = None, 0, None
        e._params = {pid: F.pic_params(24, 16) for pid in SRC + list(range(50, 53))}
        self.made, self.freed, self.calls, self.warps = [], [], 0, []

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

        def library_call(h, src, dst, n, wp):
            self.calls += 1
            w = C.cast(wp, C.POINTER(OhWarp)).contents
            self.warps.append(dict(mode=w.mode, filter=w.filter, border=w.border, fill=list(w.fill), size=(w.width, w.height), m=list(w.m),
                                   win=(w.win.left, w.win.right, w.win.top, w.win.bottom), src=list(src), dst=list(dst), n=n))
            return rc

        e.pic_alloc, e.pic_free = pic_alloc, pic_free
        e.L = types.SimpleNamespace(oh_engine_last_error=lambda h: b"refused", oh_pics_warp=library_call)


def test_failed_allocation_frees_what_it_made():
    rig = Rig(alloc_fails_at=3)
    with pytest.raises(EngineError, match="oh_pic_alloc"):
        rig.e.pics_warp(SRC, IDENT, (24, 16))
    assert rig.made == [100, 101] and sorted(rig.freed) == rig.made and rig.calls == 0


def test_refusal_frees_the_fresh_pictures():
    rig = Rig(rc=-2)
    with pytest.raises(EngineError, match="oh_pics_warp") as err:
        rig.e.pics_warp(SRC, IDENT, (24, 16))
    assert err.value.code == -2 and rig.calls == 1
    assert len(rig.made) == N and sorted(rig.freed) == rig.made


def test_fresh_pictures_are_returned_with_the_image_window():
    rig = Rig()
    ids, win = rig.e.pics_warp(SRC, IDENT, (20, 10), filter="bicubic", border="constant", fill=(1, 2, 3), window=(2, 2, 0, 4))
    assert ids == rig.made and len(ids) == N and rig.freed == [] and rig.calls == 1
    assert win == (0, 4, 0, 6)                                  # 20 x 10 inside 24 x 16: the size rounded up to the minimum coding block
    w = rig.warps[0]
    assert (w["mode"], w["filter"], w["border"], w["fill"], w["size"], w["win"]) == (1, 2, 1, [1, 2, 3], (20, 10), (2, 2, 0, 4))
    assert w["m"] == IDENT and w["src"] == SRC and w["dst"] == ids and w["n"] == N


@pytest.mark.parametrize("rc", [0, -4])
def test_given_out_is_never_freed(rc):
    rig = Rig(rc=rc)
    if rc:
        with pytest.raises(EngineError, match="oh_pics_warp"):
            rig.e.pics_warp(SRC, IDENT, (24, 16), out=[50, 51, 52])
    else:
        assert rig.e.pics_warp(SRC, IDENT, (16, 8), out=[50, 51, 52]) == ([50, 51, 52], (0, 8, 0, 8))
    assert rig.made == [] and rig.freed == [] and rig.calls == 1


def test_matrix_forms():
    """an OhWarp, 6 or 9 integers, a float 2 x 3 or 3 x 3 array; the mode follows the form unless it is given"""
    assert warp_matrix(IDENT) == (1, IDENT) and warp_matrix(IDENT[:6]) == (0, IDENT) and warp_matrix(IDENT, "affine") == (0, IDENT)
    assert warp_matrix(np.array(IDENT[:6]).reshape(2, 3)) == (0, IDENT) and warp_matrix(IDENT[:6], 1) == (1, IDENT)
    w = OhWarp()
    w.mode = 1
    w.m[:] = [5, 4, 3, 2, 1, 0, -1, -2, 77]
    assert warp_matrix(w) == (1, [5, 4, 3, 2, 1, 0, -1, -2, 77]) and warp_matrix(w, "affine")[0] == 0
    assert warp_matrix(np.eye(2, 3)) == (0, IDENT) and warp_matrix(np.eye(3)) == (1, IDENT)
    # the rounding: numpy's rint of the float64 product, halves to even; a 3 x 3 array is divided by its [2][2] entry first
    a = np.array([[0.5 + 2.0 ** -17, -1.25, 3.0 + 2.5 * 2.0 ** -16], [1.0 / 3.0, 2.0 ** -16 * 1.5, -7.75]])
    assert warp_matrix(a) == (0, [32768, -81920, 196610, 21845, 2, -507904, 0, 0, ONE30])
    p = np.array([[2.0, 0.0, 4.0], [0.0, 2.0, -6.0], [2.0 ** -9, -(2.0 ** -10), 2.0]])
    assert warp_matrix(p) == (1, [ONE, 0, 2 * ONE, 0, ONE, -3 * ONE, 1 << 20, -(1 << 19), ONE30])
    assert warp_matrix(-p) == warp_matrix(p)                    # the same projective map
    rig = Rig()
    rig.e.pics_warp(SRC, p, (24, 16))
    rig.e.pics_warp(SRC, p[:2] / 2.0, (24, 16))
    rig.e.pics_warp(SRC, w, (24, 16), mode="affine")
    assert [x["mode"] for x in rig.warps] == [1, 0, 0] and rig.warps[1]["m"] == [ONE, 0, 2 * ONE, 0, ONE, -3 * ONE, 0, 0, ONE30]


def test_what_the_wrapper_refuses_itself():
    rig = Rig()
    bad = [lambda: rig.e.pics_warp([], IDENT, (24, 16)),                                    # no picture
           lambda: rig.e.pics_warp(SRC, IDENT[:7], (24, 16)),                               # seven numbers
           lambda: rig.e.pics_warp(SRC, np.eye(3, 2), (24, 16)),                            # a float matrix of another shape
           lambda: rig.e.pics_warp(SRC, np.array([[1.0, 0, 0], [0, np.nan, 0]]), (24, 16)),
           lambda: rig.e.pics_warp(SRC, np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 0]]), (24, 16)),   # [2][2] is 0
           lambda: rig.e.pics_warp(SRC, [1 << 63, 0, 0, 0, 1, 0], (24, 16)),                # beyond int64
           lambda: rig.e.pics_warp(SRC, "identity", (24, 16)),
           lambda: rig.e.pics_warp(SRC, IDENT, (24, 16), mode="projective"),
           lambda: rig.e.pics_warp(SRC, IDENT, (24, 16), filter="lanczos"),
           lambda: rig.e.pics_warp(SRC, IDENT, (24, 16), filter=3),
           lambda: rig.e.pics_warp(SRC, IDENT, (24, 16), border="mirror"),
           lambda: rig.e.pics_warp(SRC, IDENT, (24, 16), fill=(0, 0)),
           lambda: rig.e.pics_warp(SRC, IDENT, (24, 16), fill=(0, 0, 70000)),
           lambda: rig.e.pics_warp(SRC, IDENT, (0, 16)),                                    # nothing to allocate for
           lambda: rig.e.pics_warp(SRC, IDENT, (24, 16), out=[50, 51])]
    for call in bad:
        with pytest.raises((ValueError, OverflowError)):
            call()
    assert rig.made == [] and rig.freed == [] and rig.calls == 0


def test_a_map_the_library_refuses_frees_the_fresh_pictures():
    """the wrapper leaves the coefficients' bounds to the library: its refusal frees what was made"""
    rig = Rig(rc=-2)
    with pytest.raises(EngineError, match="oh_pics_warp"):
        rig.e.pics_warp(SRC, [1 << 40, 0, 0, 0, ONE, 0], (24, 16))
    assert rig.calls == 1 and rig.warps[0]["m"][0] == 1 << 40 and len(rig.made) == N and sorted(rig.freed) == rig.made
