"""-m gpu: oh_pics_motion and Engine.pics_motion on the MI355X against the numpy model of tests/motion_model.py, every field of every
OhMotionVector bit for bit: the cases of motion_model.search_cases() (four sizes, three bit depths, both block sizes, ranges from 0 to
32, integer / half / quarter vectors, three lambdas, centres null, near and wholly outside, noise, a planted displacement, pictures on
which every candidate ties, a picture against itself), a batch of more than one launch, a two-level pyramid next to oh_pics_resize, and
the argument rules.  What the cases reach is asserted on the CPU by tests/test_motion_host.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import motion_model as MM                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

CASES = MM.search_cases()
GROUPS = sorted({c["name"] for c in CASES})
FIELDS = ("x", "y", "sad", "sad_centre")


def params(w, h, bd, cf=0):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def put(eng, p, planes):
    """the id of an uploaded picture with these coded planes"""
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        hp.visible(c)[...] = planes[c]
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == E.MOTION_DTYPE, what
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:4], got[f].ravel()[:8], want[f].ravel()[:8])


@pytest.mark.parametrize("group", GROUPS)
def test_cases(group):
    """every case of the group: cur and ref uploaded (one picture where cur is ref), searched, compared with the model's field"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for i, c in enumerate(CASES):
        if c["name"] != group:
            continue
        cur, ref, centres, field, want, _ = MM.case_result(i, c)
        p = params(c["w"], c["h"], c["bd"])
        ic = put(eng, p, [cur])
        ir = ic if c["content"] == "same" else put(eng, p, [ref])
        got = eng.pics_motion([ic], [ir], block=c["block"], range=c["range"], subpel=c["subpel"], lam=c["lam"],
                              centres=None if centres is None else centres[None])
        same(got[0], want, MM.case_id(c))
        if c["content"] == "planted":                               # what the host test asserts of the model holds for the GPU's field
            inner = MM.interior(c["w"], c["h"], c["block"], c["range"])
            assert not got[0]["sad"][inner].any() and np.array_equal(MM.field_xy(got[0])[inner], field[inner])
        if c["content"] == "opposed":
            M = (1 << c["bd"]) - 1
            assert (got[0]["sad"] % M == 0).all() and np.array_equal(MM.field_xy(got[0]), 4 * centres.astype(np.int64))
        for pid in {ic, ir}:
            eng.pic_free(pid)
    eng.close()


def test_batch_of_more_than_one_launch():
    """70 pairs of 16 x 8 in one call (OH_CONV_MAX_PICS is 64): five pictures, each used in many pairs and some as both members of one,
    centres of their own per pair; every pair equals the model, which is computed once per distinct (cur, ref, centres)"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    bd, w, h, block = 10, 16, 8, 8
    p = params(w, h, bd)
    planes = [MM.noise(bd, w, h, 4000 + k) for k in range(5)]
    ids = [put(eng, p, [v]) for v in planes]
    n = 70
    pairs = [(k % 5, (k * 3 + k // 5) % 5) for k in range(n)]
    assert any(a == b for a, b in pairs) and len(set(pairs)) > 10
    cen = np.stack([MM.random_centres(w, h, block, 6, 4100 + k % 3) for k in range(n)])
    got = eng.pics_motion([ids[a] for a, _ in pairs], [ids[b] for _, b in pairs], block=block, range=(3, 2), subpel=2, lam=7, centres=cen)
    assert got.shape == (n, 1, 2)
    memo = {}
    for k, (a, b) in enumerate(pairs):
        key = (a, b, k % 3)
        if key not in memo:
            memo[key] = MM.search(planes[a], planes[b], bd, block, (3, 2), 2, 7, cen[k])
        same(got[k], memo[key], ("pair", k))
    # without centres, and nothing written to the pictures
    got = eng.pics_motion([ids[0]] * 65, [ids[1]] * 65, block=16, range=(1, 0), subpel=1)
    want = MM.search(planes[0], planes[1], bd, 16, (1, 0), 1, 0)
    for k in (0, 63, 64):
        same(got[k], want, ("repeat", k))
    for k in range(5):
        assert np.array_equal(eng.pic_download(ids[k], p).visible(0), planes[k])
    eng.close()


def test_chroma_is_not_searched():
    """a 4:2:0 pair whose chroma planes are unrelated gives the field of its luma planes, also from a picture that a service finished"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    bd, w, h = 8, 24, 16
    p = params(w, h, bd, 1)
    a, b = MM.random_planes(bd, w, h, 1, 61), MM.random_planes(bd, w, h, 1, 62)
    ia, ib = put(eng, p, a), put(eng, p, b)
    want = MM.search(a[0], b[0], bd, 16, (3, 2), 2, 0)
    same(eng.pics_motion([ia], [ib], range=(3, 2))[0], want, "4:2:0")
    out = eng.pics_filter([ib], "median", planes=0)                 # a copy, made by a picture service: finished in half 0
    assert eng.pic_final_half(out[0]) == 0
    same(eng.pics_motion([ia], out, range=(3, 2))[0], want, "a service's destination")
    eng.close()


def test_pyramid():
    """oh_pics_resize by two, a coarse search, motion_scale, a fine search with range 2 around the scaled centres: equal to the model run
    on the downloaded pictures, level by level"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for bd in (8, 10):
        w, h = 144, 80
        p, ps = params(w, h, bd), params(w // 2, h // 2, bd)
        ref = MM.smooth(bd, w, h, 7000 + bd)
        cur = np.roll(ref, (3, -9), axis=(0, 1))                    # cur(x, y) = ref(x + 9, y - 3): beyond what the fine range alone reaches
        ic, ir = put(eng, p, [cur]), put(eng, p, [ref])
        small, _ = eng.pics_resize([ic, ir], (w // 2, h // 2))
        coarse = eng.pics_motion([small[0]], [small[1]], block=8, range=(8, 8), subpel=2, lam=4)
        grid = E.motion_blocks(w, h, 16)
        centres = E.motion_scale(coarse[0], 8, 2, grid, 16)
        fine = eng.pics_motion([ic], [ir], block=16, range=(2, 2), subpel=2, lam=4, centres=centres[None])
        sc, sr = (np.array(eng.pic_download(pid, ps).visible(0)) for pid in small)
        want_coarse = MM.search(sc, sr, bd, 8, (8, 8), 2, 4)
        same(coarse[0], want_coarse, ("coarse", bd))
        want_centres = MM.motion_scale(want_coarse, 8, 2, grid, 16)
        assert np.array_equal(centres, want_centres) and np.abs(want_centres).max() > 2
        same(fine[0], MM.search(cur, ref, bd, 16, (2, 2), 2, 4, want_centres), ("fine", bd))
    eng.close()


def test_errors_leave_out_untouched():
    """every OH_E_ARG rule of ohevc_hip.h through the raw C call, out untouched behind each refusal; n == 0 is fine with ms checked all
    the same; the limits themselves are inside"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    arg = E.OH_E_ARG
    bd, w, h = 10, 24, 16
    p = params(w, h, bd)
    a, b = put(eng, p, [MM.noise(bd, w, h, 1)]), put(eng, p, [MM.noise(bd, w, h, 2)])
    small, deep, colour = put(eng, params(16, 16, bd), [MM.noise(bd, 16, 16, 3)]), put(eng, params(w, h, 8), [MM.noise(8, w, h, 4)]), \
        put(eng, params(w, h, bd, 1), MM.random_planes(bd, w, h, 1, 5))
    keep = []
    mark = 0x5A

    def ids(v):
        if v is None:
            return None
        arr = (C.c_int * max(len(v), 1))(*v)
        keep.append(arr)
        return arr

    def search(cur=(a, a), ref=(b, b), n=2, block=8, rx=3, ry=2, subpel=2, lam=7, centres=None, e_null=False, ms_null=False, out_null=False):
        ms = E.OhMotionSearch(block, rx, ry, subpel, lam)
        if centres is not None:
            cen = np.ascontiguousarray(centres, dtype=np.int16)
            keep.append(cen)
            ms.centres = cen.ctypes.data_as(C.POINTER(C.c_int16))
        out = np.full(2 * 6 * 3, mark, dtype=np.uint32)            # room for two pairs of 3 x 2 blocks
        rc = L.oh_pics_motion(None if e_null else eng.h, ids(cur), ids(ref), n, None if ms_null else C.byref(ms),
                              None if out_null else out.ctypes.data_as(C.POINTER(E.OhMotionVector)))
        if rc != 0:
            assert (out == mark).all(), "a refused call wrote into out"
        return rc

    assert search(e_null=True) == arg and search(ms_null=True) == arg and search(out_null=True) == arg
    assert search(cur=None) == arg and search(ref=None) == arg and search(n=-1) == arg
    assert search(cur=(a, 999)) == arg and search(ref=(777, b)) == arg                                  # unknown pictures
    assert search(ref=(b, small)) == arg and search(cur=(deep, a)) == arg and search(ref=(colour, b)) == arg    # params differ
    for block in (0, 4, 12, 32, -8):
        assert search(block=block) == arg and search(cur=(), ref=(), n=0, block=block) == arg, block
    for r in (-1, 33, 1 << 20):
        assert search(rx=r) == arg and search(ry=r) == arg and search(cur=None, ref=None, n=0, ry=r) == arg, r
    for s in (-1, 3):
        assert search(subpel=s) == arg and search(cur=(), ref=(), n=0, subpel=s) == arg, s
    for lam in (-1, 4097, 1 << 30):
        assert search(lam=lam) == arg and search(cur=(), ref=(), n=0, lam=lam) == arg, lam
    zero = np.zeros((2, 2, 3, 2), np.int16)
    for where in ((0, 0, 0, 0), (1, 1, 2, 1)):                       # the first and the last component the call reads
        for v in (4097, -4097, 32767, -32768):
            cen = zero.copy()
            cen[where] = v
            assert search(centres=cen) == arg, (where, v)
    # inside the rules: the limits themselves, and n == 0
    cen = zero.copy()
    cen[0, 0, 0] = (4096, -4096)
    cen[1, 1, 2] = (-4096, 4096)
    assert search(centres=cen, rx=32, ry=32, lam=4096) == 0 and search(rx=0, ry=0, subpel=0, lam=0, block=16) == 0
    assert search(cur=(a, a), ref=(a, a)) == 0
    assert search(cur=(), ref=(), n=0) == 0 and search(cur=None, ref=None, n=0) == 0
    # the wrapper: lists of different lengths, centres of another shape
    with pytest.raises(ValueError):
        eng.pics_motion([a], [a, b])
    with pytest.raises(ValueError):
        eng.pics_motion([a], [b], block=8, centres=np.zeros((1, 1, 2, 2), np.int16))
    with pytest.raises(E.EngineError) as err:
        eng.pics_motion([a], [b], block=12)
    assert err.value.code == arg
    assert eng.pics_motion([], []).shape == (0, 0, 0)
    eng.close()
