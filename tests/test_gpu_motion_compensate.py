"""-m gpu: oh_pics_motion_compensate and Engine.pics_motion_compensate on the MI355X against the numpy model of tests/motion_model.py,
every coded plane of every destination bit for bit: chroma formats 0 to 3, bit depths 8 and 10 (12 at 4:2:0), both block sizes, four
sizes; a zero field (a copy), one constant vector per fraction class, random vectors near and at the scale of +-32768 where every read
clamps, the field a search returned; more than one launch; sources that a service finished; the calls next to oh_pics_hash and
oh_pics_convert; the composition the service exists for, compensation of prev and next onto cur in front of the temporal filter; and the
argument rules."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import filter_model as FM                                                   # noqa: E402
import motion_model as MM                                                   # noqa: E402
import picture_hash as PH                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = [(0, 8), (0, 10), (1, 8), (1, 10), (1, 12), (2, 8), (2, 10), (3, 8), (3, 10)]      # (chroma_format_idc, bit depth)


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def put(eng, p, planes):
    """the id of an uploaded picture with these coded planes"""
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        hp.visible(c)[...] = planes[c]
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid


def planes_of(eng, pid, p):
    got = eng.pic_download(pid, p)
    return [np.array(got.visible(c)) for c in range(F.n_planes(p))]


def verify(eng, pid, p, want, what=None):
    got = planes_of(eng, pid, p)
    assert len(want) == len(got)
    for c in range(len(got)):
        assert got[c].shape == want[c].shape, (what, c)
        assert np.array_equal(got[c], want[c]), (what, c, np.argwhere(got[c] != want[c])[:4])


def grid_field(w, h, block, vec):
    bw, bh = MM.blocks(w, h, block)
    return np.broadcast_to(np.asarray(vec, dtype=np.int64), (bh, bw, 2)).copy()


@pytest.mark.parametrize("cf,bd", FORMATS, ids=[f"cf{cf}-{bd}bit" for cf, bd in FORMATS])
def test_every_fraction_class(cf, bd):
    """24 x 16 (blocks of 16 cut at the right edge) and 16 x 8: a zero field copies; then one constant vector per pair of eighth-sample
    fractions of 4:2:0 chroma, which takes luma through its 16 classes four times, with whole parts of either sign"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for (w, h), block in (((24, 16), 16), ((16, 8), 8)):
        p = params(w, h, bd, cf)
        src = MM.random_planes(bd, w, h, cf, 100 * bd + 10 * cf + block)
        sid = put(eng, p, src)
        dst = eng.pic_alloc(p)
        assert eng.pics_motion_compensate([sid], grid_field(w, h, block, (0, 0))[None], block=block, out=[dst]) == [dst]
        assert eng.pic_final_half(dst) == 0
        verify(eng, dst, p, src, "zero field")
        vectors = MM.class_vectors()
        assert {(x & 7, y & 7) for x, y in vectors} == set(itertools.product(range(8), repeat=2))
        for vec in vectors:
            field = grid_field(w, h, block, vec)
            eng.pics_motion_compensate([sid], field[None], block=block, out=[dst])
            verify(eng, dst, p, MM.compensate(src, cf, bd, field, block), (w, h, block, vec))
    eng.close()


@pytest.mark.parametrize("w,h", MM.SIZES, ids=[f"{w}x{h}" for w, h in MM.SIZES])
def test_random_fields(w, h):
    """per size, format and block size: vectors within a few samples, one per block; vectors over the whole int16 range, where nearly
    every read clamps; the extremes themselves"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for k, (cf, bd) in enumerate(FORMATS):
        for block in (8, 16):
            if (k + block // 8) % 2 and (w, h) == MM.SIZES[-1]:
                continue                                            # the largest size takes every other combination
            p = params(w, h, bd, cf)
            seed = 1000 * w + 10 * k + block
            src = MM.random_planes(bd, w, h, cf, seed)
            sid = put(eng, p, src)
            near = MM.random_field(w, h, block, -40, 40, seed + 1)
            far = MM.random_field(w, h, block, -32768, 32767, seed + 2)
            far.reshape(-1, 2)[0] = (-32768, 32767)
            far.reshape(-1, 2)[-1] = (32767, -32768)
            out = eng.pics_motion_compensate([sid, sid], np.stack([near, far]), block=block)
            assert len(out) == 2 and sid not in out and all(eng.pic_final_half(pid) == 0 for pid in out)
            verify(eng, out[0], p, MM.compensate(src, cf, bd, near, block), (cf, bd, block, "near"))
            verify(eng, out[1], p, MM.compensate(src, cf, bd, far, block), (cf, bd, block, "far"))
            for pid in out + [sid]:
                eng.pic_free(pid)
    eng.close()


def test_the_field_of_a_search():
    """search, then compensate with what came back (the structured array as it is): the prediction equals the model's, and its luma
    differs from cur by exactly the SADs the search reported"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for bd, block, cf in ((8, 16, 1), (10, 8, 3)):
        w, h = 72, 40
        p = params(w, h, bd, cf)
        ref = [MM.smooth(bd, s[1], s[0], 300 + bd + c) for c, s in enumerate(MM.plane_shapes(w, h, cf))]
        truth = MM.random_field(w, h, block, -11, 11, 310 + bd)
        cur = MM.compensate(ref, cf, bd, truth, block)
        ic, ir = put(eng, p, cur), put(eng, p, ref)
        field = eng.pics_motion([ic], [ir], block=block, range=(3, 3), subpel=2)
        out = eng.pics_motion_compensate([ir], field, block=block)
        want = MM.compensate(ref, cf, bd, field[0], block)
        verify(eng, out[0], p, want, (bd, block))
        diff = np.abs(want[0].astype(np.int64) - cur[0].astype(np.int64))
        for by, bx in np.ndindex(field[0].shape):
            x0, y0, bw_, bh_ = MM.rect(w, h, block, bx, by)
            assert diff[y0:y0 + bh_, x0:x0 + bw_].sum() == field[0]["sad"][by, bx], (bx, by)
    eng.close()


def test_more_than_one_launch_and_service_made_sources():
    """70 pictures of 16 x 8 in one call (OH_CONV_MAX_PICS is 64), each with a field of its own, from three sources of which one was
    finished by oh_pics_filter; the destinations are given"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    bd, cf, w, h, block = 10, 1, 16, 8, 8
    p = params(w, h, bd, cf)
    planes = [MM.random_planes(bd, w, h, cf, 800 + k) for k in range(3)]
    ids = [put(eng, p, v) for v in planes]
    made = eng.pics_filter([ids[2]], "median")
    assert eng.pic_final_half(made[0]) == 0
    planes[2] = FM.filter_pic(planes[2], FM.MEDIAN, bd)
    ids[2] = made[0]
    n = 70
    fields = np.stack([MM.random_field(w, h, block, -64, 64, 900 + k) for k in range(n)])
    dst = [eng.pic_alloc(p) for _ in range(n)]
    assert eng.pics_motion_compensate([ids[k % 3] for k in range(n)], fields, block=block, out=dst) == dst
    for k in range(n):
        verify(eng, dst[k], p, MM.compensate(planes[k % 3], cf, bd, fields[k], block), k)
    eng.close()


def test_next_to_hash_and_convert():
    """the destination hashes and converts like any picture, with no wait in between"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for bd in (8, 10):
        w, h, block = 24, 16, 16
        p = params(w, h, bd, 3)
        src = MM.random_planes(bd, w, h, 3, 40 + bd)
        sid = put(eng, p, src)
        field = MM.random_field(w, h, block, -30, 30, 50 + bd)
        out = eng.pics_motion_compensate([sid], field[None], block=block)
        want = MM.compensate(src, 3, bd, field, block)
        for ht in (1, 2):
            assert eng.pics_hash(out, ht)[0] == PH.picture_hash(want, bd, ht), (bd, ht)
        img = eng.pics_convert(out, "planar").cpu().numpy()
        assert img.shape == (1, 48, 24) and np.array_equal(img[0], np.concatenate(want)), bd
    eng.close()


def test_motion_compensated_temporal_filter():
    """what the service exists for: prev and next are searched against cur and compensated onto it, then oh_pics_filter TEMPORAL averages
    where the compensated neighbours agree with cur — equal to filter_model.filter_pic on the model's compensated planes, and it
    averages where the filter on the neighbours as they are keeps cur"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for bd, cf, block in ((8, 1, 16), (10, 2, 8)):
        w, h = 72, 40
        p = params(w, h, bd, cf)
        shapes = MM.plane_shapes(w, h, cf)
        base = [MM.smooth(bd, s[1] + 16, s[0] + 16, 600 + bd + c) for c, s in enumerate(shapes)]
        hs, vs = int(cf in (1, 2)), int(cf == 1)

        def view(dx, dy):                                           # the scene panned by (dx, dy) luma samples (multiples of 2)
            return [np.ascontiguousarray(b[8 + (dy >> (vs if c else 0)):, 8 + (dx >> (hs if c else 0)):][:s[0], :s[1]])
                    for c, (b, s) in enumerate(zip(base, shapes))]
        rng = np.random.default_rng(610 + bd)
        M = (1 << bd) - 1

        def noisy(planes):                                          # grain of -1 .. 1: nine of them stay within the threshold below
            return [np.clip(v.astype(np.int64) + rng.integers(-1, 2, v.shape), 0, M).astype(v.dtype) for v in planes]
        prev, cur, nxt = noisy(view(-4, 2)), view(0, 0), noisy(view(4, -2))
        ids = [put(eng, p, v) for v in (prev, cur, nxt)]
        fields = eng.pics_motion([ids[1], ids[1]], [ids[0], ids[2]], block=block, range=(6, 4), subpel=0)
        comp = eng.pics_motion_compensate([ids[0], ids[2]], fields, block=block)
        thr = (9, 9)
        out = eng.pics_filter([ids[1]], "temporal", threshold=thr, prev=[comp[0]], next=[comp[1]])
        mp = MM.compensate(prev, cf, bd, MM.search(cur[0], prev[0], bd, block, (6, 4), 0), block)
        mn = MM.compensate(nxt, cf, bd, MM.search(cur[0], nxt[0], bd, block, (6, 4), 0), block)
        verify(eng, comp[0], p, mp, "prev onto cur")
        verify(eng, comp[1], p, mn, "next onto cur")
        want = FM.filter_pic(cur, FM.TEMPORAL, bd, threshold=thr, prev=mp, nxt=mn)
        verify(eng, out[0], p, want, (bd, cf))
        # in whole blocks none of whose reads clamp the compensated neighbours are cur plus grain, so the filter averages there,
        # while on the neighbours as they are it finds motion everywhere and keeps cur
        plain = FM.filter_pic(cur, FM.TEMPORAL, bd, threshold=thr, prev=prev, nxt=nxt)
        inner = (slice(16, -16), slice(16, -16))
        assert np.abs(mp[0][inner].astype(np.int64) - cur[0][inner]).max() == 1 and np.abs(mn[0][inner].astype(np.int64) - cur[0][inner]).max() == 1
        assert np.array_equal(plain[0][inner], cur[0][inner]) and not np.array_equal(want[0][inner], cur[0][inner])
    eng.close()


def test_errors_write_nothing():
    """every OH_E_ARG rule of ohevc_hip.h through the raw C call: refused on the host, and behind each refusal the checksums of all
    pictures in play have not moved; n == 0 is fine; then calls inside the rules succeed"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    arg = E.OH_E_ARG
    bd = 10
    seeds = itertools.count(500, 10)

    def some(p, k=2):
        seed = next(seeds)
        return [put(eng, p, MM.random_planes(p.bit_depth, p.width, p.height, p.chroma_format_idc, seed + i)) for i in range(k)]
    p = params(32, 16, bd, 1)
    src, dst = some(p), some(p)
    small, deep, full = some(params(16, 16, bd, 1)), some(params(32, 16, 8, 1)), some(params(32, 16, bd, 3))
    watched = src + dst + small + deep + full

    def sums():
        return [eng.pics_hash([pid], 2) for pid in watched]
    before = sums()
    keep = []
    vecs = (E.OhMotionVector * 16)()                                # two pictures of 4 x 2 blocks of 8

    def ids(v):
        if v is None:
            return None
        a = (C.c_int * max(len(v), 1))(*v)
        keep.append(a)
        return a

    def comp(s=src, d=dst, n=2, block=8, field=vecs, e_null=False):
        rc = L.oh_pics_motion_compensate(None if e_null else eng.h, ids(s), ids(d), n, block, field)
        if rc != 0:
            assert sums() == before, "a refused call wrote into a picture"
        return rc

    assert comp(e_null=True) == arg and comp(field=None) == arg and comp(s=None) == arg and comp(d=None) == arg and comp(n=-1) == arg
    assert comp(s=[src[0], 999]) == arg and comp(d=[999, dst[1]]) == arg                                # unknown pictures
    assert comp(s=[src[0], small[0]]) == arg and comp(d=[dst[0], small[0]]) == arg                      # params differ
    assert comp(d=deep) == arg and comp(d=full) == arg and comp(d=small) == arg
    assert comp(d=[dst[0], dst[0]]) == arg and comp(d=src) == arg and comp(d=[src[1], dst[0]]) == arg   # twice; also a source
    for block in (0, 4, 12, 32, -16):
        assert comp(block=block) == arg and comp(s=[], d=[], n=0, block=block) == arg, block
    eng.sync()
    assert sums() == before
    assert comp(s=[], d=[], n=0) == 0 and comp(s=None, d=None, n=0) == 0 and comp(s=None, d=None, n=0, block=16) == 0
    eng.sync()
    assert sums() == before
    # inside the rules: a source twice; any int16 and any sad in the field
    for i in range(16):
        vecs[i].x, vecs[i].y, vecs[i].sad, vecs[i].sad_centre = (-32768, 32767, 0xFFFFFFFF, 7) if i % 2 else (5, -9, 0, 0)
    assert comp(s=[src[0], src[0]]) == 0
    eng.sync()
    after = sums()
    assert [i for i in range(len(watched)) if after[i] != before[i]] == [watched.index(pid) for pid in dst]
    s0 = planes_of(eng, src[0], p)
    field = np.array([[(-32768, 32767) if (4 * by + bx) % 2 else (5, -9) for bx in range(4)] for by in range(2)])
    verify(eng, dst[0], p, MM.compensate(s0, 1, bd, field, 8), "inside the rules")
    with pytest.raises(E.EngineError) as err:
        eng.pics_motion_compensate(src, np.zeros((2, 2, 4), dtype=E.MOTION_DTYPE), block=8, out=src)
    assert err.value.code == arg
    eng.close()
