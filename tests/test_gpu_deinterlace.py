"""-m gpu: oh_pics_weave / oh_pics_separate / oh_pics_deinterlace and their Engine methods on the MI355X against the numpy model of
tests/deinterlace_model.py, every coded plane of every destination bit for bit: fields to frames and back at every chroma format and
two bit depths, every mode with both parities and both kept_first, the still scene, the segment seam, the clipping planes, a batch of
more than one launch, the finished halves, the calls next to oh_pics_hash and oh_pics_convert, from the SEI's bytes to the woven frame,
and the argument rules."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import deinterlace_model as DM                                              # noqa: E402
import picture_hash as PH                                                   # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = [(16, 8), (24, 16)]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]
MODES = (DM.BOB, DM.BLEND, DM.LOWPASS5, DM.ADAPTIVE)


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def host_pic(p, planes):
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        hp.visible(c)[...] = planes[c]
    return hp


def random_planes(p, rng):
    dt = np.uint8 if p.bit_depth == 8 else np.uint16
    return [rng.integers(0, 1 << p.bit_depth, s, dtype=dt) for s in DM.plane_shapes(p.width, p.height, p.chroma_format_idc)]


def put(eng, p, planes):
    """the id of an uploaded picture with these coded planes"""
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, host_pic(p, planes))
    return pid


def verify(eng, pid, p, want, what=None):
    got = eng.pic_download(pid, p)
    assert len(want) == F.n_planes(p)
    for c in range(F.n_planes(p)):
        assert got.visible(c).shape == want[c].shape, (what, c)
        assert np.array_equal(got.visible(c), want[c]), (what, c, np.argwhere(got.visible(c) != want[c])[:4])


@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("bd", (8, 10))
def test_weave_and_separate(bd, w, h):
    """fields of w x h into frames of w x 2h and back, chroma formats 0 .. 3; one side alone"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(bd * 100 + w)
    eng = Engine(0)
    for cf in range(4):
        fp, Fp = params(w, h, bd, cf), params(w, 2 * h, bd, cf)
        t, b = random_planes(fp, rng), random_planes(fp, rng)
        tid, bid = put(eng, fp, t), put(eng, fp, b)
        frames = eng.pics_weave([tid], [bid])
        assert len(frames) == 1 and frames[0] not in (tid, bid)
        dp = eng._pic_params(frames[0])
        assert (dp.width, dp.height, dp.bit_depth, dp.chroma_format_idc) == (w, 2 * h, bd, cf)
        verify(eng, frames[0], Fp, DM.weave(t, b), ("weave", cf))
        assert eng.pic_final_half(frames[0]) == 0
        tops, bottoms = eng.pics_separate(frames)
        dp = eng._pic_params(tops[0])
        assert (dp.width, dp.height, dp.bit_depth, dp.chroma_format_idc) == (w, h, bd, cf)
        verify(eng, tops[0], fp, t, ("separate, top", cf))
        verify(eng, bottoms[0], fp, b, ("separate, bottom", cf))
        assert DM.separate(DM.weave(t, b))[0][0].tobytes() == t[0].tobytes()
        only_t, none = eng.pics_separate(frames, bottom=False)
        assert none is None
        verify(eng, only_t[0], fp, t, ("top alone", cf))
        none, only_b = eng.pics_separate(frames, top=False)
        assert none is None
        verify(eng, only_b[0], fp, b, ("bottom alone", cf))
        # into pictures that exist: the fields swapped give the frame with its rows swapped in pairs
        eng.pics_weave([bid], [tid], out=frames)
        verify(eng, frames[0], Fp, DM.weave(b, t), ("weave into out", cf))
        for pid in [tid, bid] + frames + tops + bottoms + only_t + only_b:
            eng.pic_free(pid)
    eng.close()


@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("bd", (8, 10))
def test_every_mode(bd, w, h):
    """4 modes x 2 parities x 2 kept_first x chroma formats 0 .. 3 on independent random prev / cur / next (the planes whose branch
    coverage tests/test_deinterlace_host.py asserts); at 4:2:0, 16 x 8 has chroma planes of 4 rows: both edge rules at once"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for cf in range(4):
        p = params(w, h, bd, cf)
        P, Cu, N = DM.random_triplet(bd, w, h, cf)
        ids = [put(eng, p, v) for v in (P, Cu, N)]
        dst = eng.pic_alloc(p)
        for mode, parity, kf in itertools.product(MODES, (0, 1), (0, 1)):
            out = eng.pics_deinterlace([ids[1]], mode, keep=parity, kept_first=kf, prev=[ids[0]], next=[ids[2]], out=[dst])
            assert out == [dst]
            verify(eng, dst, p, DM.deinterlace(Cu, mode, parity, bd, kf, P, N), (cf, mode, parity, kf))
        fresh = eng.pics_deinterlace([ids[1]], "bob", keep="bottom")
        assert fresh[0] not in ids + [dst] and eng.pic_final_half(fresh[0]) == 0
        verify(eng, fresh[0], p, DM.deinterlace(Cu, DM.BOB, 1, bd), (cf, "fresh"))
        for pid in ids + [dst] + fresh:
            eng.pic_free(pid)
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_units_of_row_pairs(bd):
    """the vertical filters take four pairs of rows per workgroup and carry rows from pair to pair: 16 x 24 at 4:2:0 has 12 pairs of
    luma rows (three whole units) and 6 of chroma rows (a whole unit and half of one); 16 x 8 at 4:2:2 a single unit in every plane"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(24 + bd)
    eng = Engine(0)
    for w, h, cf in ((16, 24, 1), (16, 8, 2), (16, 40, 0)):
        p = params(w, h, bd, cf)
        P, Cu, N = (random_planes(p, rng) for _ in range(3))
        ids = [put(eng, p, v) for v in (P, Cu, N)]
        dst = eng.pic_alloc(p)
        for mode, parity in itertools.product(MODES, (0, 1)):
            eng.pics_deinterlace([ids[1]], mode, keep=parity, kept_first=parity, prev=[ids[0]], next=[ids[2]], out=[dst])
            verify(eng, dst, p, DM.deinterlace(Cu, mode, parity, bd, parity, P, N), (h, cf, mode, parity))
    eng.close()


def test_adaptive_still_scene_and_missing_neighbours():
    """prev == cur == next gives cur; prev=None / next=None and None entries equal passing cur"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for bd, cf in ((8, 1), (10, 2)):
        p = params(24, 16, bd, cf)
        P, Cu, N = DM.random_triplet(bd, 24, 16, cf)
        ip, ic, inx = (put(eng, p, v) for v in (P, Cu, N))
        for parity, kf in itertools.product((0, 1), (0, 1)):
            kw = dict(keep=parity, kept_first=kf)
            still = eng.pics_deinterlace([ic], "adaptive", prev=[ic], next=[ic], **kw)
            verify(eng, still[0], p, Cu, ("still", bd, parity, kf))
            bare = eng.pics_deinterlace([ic], "adaptive", **kw)
            verify(eng, bare[0], p, Cu, ("no neighbours", bd, parity, kf))
            # two pictures in one call: the first has no prev, the second no next
            got = eng.pics_deinterlace([ic, ic], "adaptive", prev=[None, ip], next=[inx, None], **kw)
            verify(eng, got[0], p, DM.deinterlace(Cu, DM.ADAPTIVE, parity, bd, kf, Cu, N), ("prev None", bd, parity, kf))
            verify(eng, got[1], p, DM.deinterlace(Cu, DM.ADAPTIVE, parity, bd, kf, P, Cu), ("next None", bd, parity, kf))
            same = eng.pics_deinterlace([ic, ic], "adaptive", prev=[ic, ip], next=[inx, ic], **kw)
            assert eng.pics_hash(same, 2) == eng.pics_hash(got, 2)
            for pid in still + bare + got + same:
                eng.pic_free(pid)
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_segment_seam(bd):
    """DEINT_SEG + 8 samples wide, 8 rows, 4:2:0: the luma rows take two workgroups, the seven-column window of ADAPTIVE crosses the seam
    from either side, the last granule of the 8-bit luma rows (and of the chroma rows at either depth) is partial"""
    from openhevc_amd.engine import Engine
    w, h = E.DEINT_SEG + 8, 8
    gs = 16 if bd == 8 else 8
    assert (w // 2) % gs and (bd != 8 or w % gs)
    rng = np.random.default_rng(4104 + bd)
    eng = Engine(0)
    p = params(w, h, bd, 1)
    P, Cu, N = (random_planes(p, rng) for _ in range(3))
    ids = [put(eng, p, v) for v in (P, Cu, N)]
    dst = eng.pic_alloc(p)
    for mode, parity, kf in ((DM.LOWPASS5, 0, 1), (DM.ADAPTIVE, 1, 0)):
        eng.pics_deinterlace([ids[1]], mode, keep=parity, kept_first=kf, prev=[ids[0]], next=[ids[2]], out=[dst])
        want = DM.deinterlace(Cu, mode, parity, bd, kf, P, N)
        verify(eng, dst, p, want, (mode, parity))
        if mode == DM.ADAPTIVE:                                             # the samples next to the seam are not all straight ones
            _, js, _, _ = DM.adaptive_plane(P[0][:, E.DEINT_SEG - 8:E.DEINT_SEG + 8], Cu[0][:, E.DEINT_SEG - 8:E.DEINT_SEG + 8],
                                            N[0][:, E.DEINT_SEG - 8:E.DEINT_SEG + 8], parity, kf, detail=True)
            assert (js[1 - parity::2, 4:12] != 0).any()
    # fields of that width: the row copy across the seam
    fp = params(w, 8, bd, 1)
    t, b = random_planes(fp, rng), random_planes(fp, rng)
    tid, bid = put(eng, fp, t), put(eng, fp, b)
    frames = eng.pics_weave([tid], [bid])
    verify(eng, frames[0], params(w, 16, bd, 1), DM.weave(t, b), "weave")
    tops, bottoms = eng.pics_separate(frames)
    verify(eng, tops[0], fp, t, "top")
    verify(eng, bottoms[0], fp, b, "bottom")
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_clipping_and_constant_planes(bd):
    """the two planes that push LOWPASS5 above M and below 0, and planes of all 0 and all M in every mode"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    M = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    p = params(16, 8, bd, 1)
    shapes = DM.plane_shapes(16, 8, 1)
    dst = eng.pic_alloc(p)
    for parity in (0, 1):
        y = 3 - parity
        high = [np.full(s, M, dt) for s in shapes]
        low = [np.zeros(s, dt) for s in shapes]
        high[0][[y - 2, y + 2]] = 0
        low[0][[y - 2, y + 2]] = M
        for name, planes, edge in (("high", high, M), ("low", low, 0)):
            pid = put(eng, p, planes)
            eng.pics_deinterlace([pid], "lowpass5", keep=parity, out=[dst])
            want = DM.deinterlace(planes, DM.LOWPASS5, parity, bd)
            assert (want[0][y] == edge).all()
            verify(eng, dst, p, want, (name, parity))
            eng.pic_free(pid)
    for value in (0, M):
        flat = [np.full(s, value, dt) for s in shapes]
        other = [np.full(s, M - value, dt) for s in shapes]
        pid, oid = put(eng, p, flat), put(eng, p, other)
        for mode, parity in itertools.product(MODES, (0, 1)):
            eng.pics_deinterlace([pid], mode, keep=parity, prev=[oid], next=[oid], out=[dst])
            verify(eng, dst, p, DM.deinterlace(flat, mode, parity, bd, 1, other, other), (value, mode, parity))
    eng.close()


def test_more_than_one_launch():
    """CONV_MAX_PICS + 1 pictures of 16 x 8 in one call, each with its own content, a mix of real and None prev entries; and as many
    pairs of fields woven in one call"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(65)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 1
    p = params(16, 8, 10, 1)
    planes = [random_planes(p, rng) for _ in range(n)]
    ids = [put(eng, p, v) for v in planes]
    prev = [None if i % 3 == 0 else ids[i - 1] for i in range(n)]
    nxt = [ids[i + 1] if i + 1 < n else None for i in range(n)]
    out = eng.pics_deinterlace(ids, "adaptive", keep="bottom", kept_first=False, prev=prev, next=nxt)
    assert len(out) == n and len(set(out)) == n and not set(out) & set(ids)
    for i in range(n):
        want = DM.deinterlace(planes[i], DM.ADAPTIVE, 1, 10, 0, planes[i] if prev[i] is None else planes[i - 1],
                              planes[i + 1] if i + 1 < n else planes[i])
        verify(eng, out[i], p, want, ("batch", i))
    frames = eng.pics_weave(ids, ids[1:] + ids[:1])
    Fp = params(16, 16, 10, 1)
    for i in (0, 1, n - 2, n - 1):
        verify(eng, frames[i], Fp, DM.weave(planes[i], planes[(i + 1) % n]), ("weave", i))
    eng.close()


def test_state_and_halves():
    """sources whose finished half is half 1 are read there; destinations whose finished half was 1 get half 0 written and marked; a
    destination reused via out="""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(12)
    eng = Engine(0)
    p = params(32, 16, 10, 1)
    a, b = random_planes(p, rng), random_planes(p, rng)
    ia = put(eng, p, a)
    half = eng.L.oh_pic_bytes(C.byref(p)) // 2
    mem = torch.zeros(2 * half, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    own = eng.pic_wrap(p, mem.data_ptr() + half, mem.data_ptr(), half)      # its half 0 is the upper block
    eng.pic_upload(own, host_pic(p, b))                                     # b in the upper block
    twin = eng.pic_wrap(p, mem.data_ptr(), mem.data_ptr() + half, half)     # the same memory: half 1 holds b, half 0 zeros
    eng.pic_set_final_half(twin, 1)
    assert eng.pic_final_half(twin) == 1
    dst = eng.pic_alloc(p)
    eng.pic_upload(dst, host_pic(p, random_planes(p, rng)))
    eng.pic_set_final_half(dst, 1)
    assert eng.pics_deinterlace([twin], "adaptive", prev=[ia], next=[twin], out=[dst]) == [dst]
    assert eng.pic_final_half(dst) == 0
    verify(eng, dst, p, DM.deinterlace(b, DM.ADAPTIVE, 0, 10, 1, a, b), "cur and next in half 1")
    eng.pic_set_final_half(dst, 1)
    eng.pics_deinterlace([ia], "adaptive", prev=[twin], next=[twin], keep="bottom", out=[dst])
    eng.pics_deinterlace([twin], "blend", out=[dst])                        # back to back, no wait between: the second call's result stays
    assert eng.pic_final_half(dst) == 0
    verify(eng, dst, p, DM.deinterlace(b, DM.BLEND, 0, 10), "second call")
    # fields: a frame in half 1 separated, fields in half 1 woven
    fp = params(32, 8, 10, 1)
    tops, bottoms = eng.pics_separate([twin])
    tb = DM.separate(b)
    verify(eng, tops[0], fp, tb[0], "separate from half 1")
    verify(eng, bottoms[0], fp, tb[1], "separate from half 1")
    eng.pic_set_final_half(dst, 1)
    assert eng.pics_weave(bottoms, tops, out=[dst]) == [dst] and eng.pic_final_half(dst) == 0
    verify(eng, dst, p, DM.weave(tb[1], tb[0]), "weave into a reused destination")
    eng.close()


def test_next_to_hash_and_convert():
    """the result hashes like the model on the host, and converts: 4:4:4 planar is the model's planes one below the other"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for bd in (8, 10):
        p = params(24, 16, bd, 3)
        P, Cu, N = DM.random_triplet(bd, 24, 16, 3)
        ids = [put(eng, p, v) for v in (P, Cu, N)]
        for mode in MODES:
            out = eng.pics_deinterlace([ids[1]], mode, prev=[ids[0]], next=[ids[2]])
            want = DM.deinterlace(Cu, mode, 0, bd, 1, P, N)
            for ht in (1, 2):
                assert eng.pics_hash(out, ht)[0] == PH.picture_hash(want, bd, ht), (bd, mode, ht)
            img = eng.pics_convert(out, "planar").cpu().numpy()
            assert img.shape == (1, 48, 24) and np.array_equal(img[0], np.concatenate(want)), (bd, mode)
            eng.pic_free(out[0])
    eng.close()


def test_from_the_sei_to_the_woven_frame():
    """two picture timing messages (pic_struct 11: a top field paired with the next picture; 10: a bottom field paired with the previous
    one) -> annexb.pic_timing -> field_info -> which picture is the top field of pics_weave"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(1110)
    eng = Engine(0)
    fp, Fp = params(24, 16, 10, 1), params(24, 32, 10, 1)
    first, second = random_planes(fp, rng), random_planes(fp, rng)
    pics = [(put(eng, fp, first), first), (put(eng, fp, second), second)]           # in output order

    def sei(pic_struct):
        return bytes([39 << 1, 1, 1, 1, (pic_struct << 4) | 1]) + b"\x80"           # interlaced source, no duplicate
    for structs in ((11, 10), (12, 9)):
        info = [E.field_info(A.pic_timing(sei(s))["pic_struct"]) for s in structs]
        assert [i.pair for i in info] == [1, -1] and {i.kind for i in info} == {E.FIELD_TOP, E.FIELD_BOTTOM}
        top = next(pc for pc, i in zip(pics, info) if i.kind == E.FIELD_TOP)
        bottom = next(pc for pc, i in zip(pics, info) if i.kind == E.FIELD_BOTTOM)
        frames = eng.pics_weave([top[0]], [bottom[0]])
        want = DM.weave(top[1], bottom[1])
        verify(eng, frames[0], Fp, want, structs)
        assert np.array_equal(want[0][0::2], (first if structs[0] == 11 else second)[0])
        eng.pic_free(frames[0])
    eng.close()


def test_errors_write_nothing():
    """every OH_E_ARG and OH_E_UNSUPPORTED rule of ohevc_hip.h through the raw C calls: refused on the host, and behind each refusal the
    checksums of all pictures in play are fetched and have not moved; n == 0 is fine; then the calls inside the rules succeed"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)

    def some(p, k=2):
        return [put(eng, p, random_planes(p, rng)) for _ in range(k)]
    fp, Fp = params(32, 16, 10, 1), params(32, 32, 10, 1)
    tops, bots, frames = some(fp), some(fp), some(Fp)
    more_fields = some(fp, 4)
    wide_f, tall_f = some(params(48, 32, 10, 1)), some(params(32, 48, 10, 1))          # frames of another width / not twice the height
    deep_f, full_f = some(params(32, 32, 8, 1)), some(params(32, 32, 10, 3))           # another bit depth / chroma format
    odd_field = put(eng, F.pic_params(32, 16, bit_depth=10, chroma_format_idc=1, log2_ctb_size=5), random_planes(fp, rng))   # a field with other params
    cur, dst, prv = some(Fp), some(Fp), some(Fp)
    deep_d, full_d = some(params(32, 32, 8, 1)), some(params(32, 32, 10, 3))
    watched = tops + bots + frames + more_fields + wide_f + tall_f + deep_f + full_f + [odd_field] + cur + dst + prv + deep_d + full_d
    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED

    def sums():
        return [eng.pics_hash([pid], 2) for pid in watched]
    before = sums()
    keep = []

    def ids(v):
        if v is None:
            return None
        a = (C.c_int * max(len(v), 1))(*v)
        keep.append(a)
        return a

    def refused_writes_nothing(rc):
        """behind every refused call: a download of the checksums of every picture in play"""
        if rc != 0:
            assert sums() == before, "a refused call wrote into a picture"
        return rc

    def weave(t=tops, b=bots, d=frames, n=2, e_null=False):
        return refused_writes_nothing(L.oh_pics_weave(None if e_null else eng.h, ids(t), ids(b), ids(d), n))

    def separate(s=frames, t=tops, b=bots, n=2, e_null=False):
        return refused_writes_nothing(L.oh_pics_separate(None if e_null else eng.h, ids(s), ids(t), ids(b), n))

    def deint(c=cur, d=dst, pv=None, nx=None, n=2, mode=3, parity=0, kf=1, d_null=False, e_null=False):
        dd = E.OhDeinterlace(mode, parity, kf)
        return refused_writes_nothing(L.oh_pics_deinterlace(None if e_null else eng.h, ids(pv), ids(c), ids(nx), ids(d), n,
                                                            None if d_null else C.byref(dd)))

    # weave
    assert weave(e_null=True) == arg and weave(t=None) == arg and weave(b=None) == arg and weave(d=None) == arg and weave(n=-1) == arg
    assert weave(t=[tops[0], 999]) == arg and weave(b=[-1, bots[1]]) == arg and weave(d=[frames[0], 999]) == arg       # unknown pictures
    assert weave(b=[bots[0], odd_field]) == arg and weave(t=[odd_field, tops[1]]) == arg                                # params differ inside the fields
    assert weave(d=[frames[0], wide_f[0]]) == arg                                                                       # inside the frames
    assert weave(d=wide_f) == arg and weave(d=tall_f) == arg and weave(d=more_fields[:2]) == arg                       # width; height not twice
    assert weave(d=[frames[0], frames[0]]) == arg                                                                       # a destination twice
    assert weave(t=frames, b=frames, d=frames) == arg and weave(t=more_fields[:2], b=more_fields[2:], d=more_fields[:2]) == arg   # source and destination
    assert weave(d=deep_f) == uns and weave(d=full_f) == uns
    assert "oh_pics_reformat" in L.oh_engine_last_error(eng.h).decode()
    # separate
    assert separate(e_null=True) == arg and separate(s=None) == arg and separate(n=-1) == arg
    assert separate(t=None, b=None) == arg                                                                              # both destination lists null
    assert separate(s=[frames[0], 999]) == arg and separate(t=[tops[0], 999]) == arg and separate(b=[999, bots[0]]) == arg
    assert separate(s=[frames[0], wide_f[0]]) == arg and separate(b=[bots[0], odd_field]) == arg and separate(t=[odd_field, tops[1]], b=None) == arg
    assert separate(s=wide_f) == arg and separate(s=tall_f) == arg and separate(s=tops, t=more_fields[:2], b=more_fields[2:]) == arg
    assert separate(t=[tops[0], tops[0]]) == arg and separate(t=tops, b=[bots[0], tops[1]]) == arg                     # twice, across both lists
    assert separate(t=[tops[0], tops[0]], b=None) == arg
    assert separate(s=more_fields[:2], t=more_fields[:2], b=None) == arg and separate(s=frames, t=tops, b=[bots[0], frames[1]]) == arg
    assert separate(s=deep_f) == uns and separate(s=full_f, b=None) == uns
    # deinterlace
    assert deint(e_null=True) == arg and deint(d_null=True) == arg and deint(c=None) == arg and deint(d=None) == arg and deint(n=-1) == arg
    assert deint(c=[cur[0], 999]) == arg and deint(d=[999, dst[1]]) == arg and deint(pv=[prv[0], 999]) == arg and deint(nx=[777, -1]) == arg
    assert deint(pv=[-2, prv[1]]) == arg and deint(nx=[prv[0], -5]) == arg                                             # below -1
    assert deint(c=[cur[0], tops[0]]) == arg and deint(d=[dst[0], tops[0]]) == arg and deint(pv=[tops[0], -1]) == arg  # params differ
    assert deint(d=deep_d) == arg and deint(d=full_d) == arg and deint(nx=[-1, full_d[0]]) == arg                      # depth, format: a params difference
    assert deint(d=[dst[0], dst[0]]) == arg and deint(d=cur) == arg and deint(d=[cur[1], dst[0]]) == arg                # twice; also a source
    assert deint(pv=[dst[1], -1]) == arg and deint(nx=[-1, dst[0]]) == arg                                             # a destination among prev / next
    for mode in (-1, 4, 1 << 20):
        assert deint(mode=mode) == arg and deint(c=[], d=[], n=0, mode=mode) == arg, mode
    for v in (-1, 2, 7):
        assert deint(parity=v) == arg and deint(kf=v) == arg and deint(mode=1, parity=v) == arg and deint(mode=0, kf=v) == arg, v
    eng.sync()
    assert sums() == before, "a refused call wrote into a picture"
    # n == 0
    assert weave(t=[], b=[], d=[], n=0) == 0 and weave(t=None, b=None, d=None, n=0) == 0
    assert separate(s=[], t=[], b=[], n=0) == 0 and deint(c=[], d=[], n=0) == 0 and deint(c=None, d=None, n=0) == 0
    eng.sync()
    assert sums() == before
    # inside the rules; prev / next are not even looked at by the other modes; a source twice is fine
    for mode in (0, 1, 2):
        assert deint(mode=mode, pv=[999, -7], nx=[dst[0], tops[0]]) == 0, mode
    assert deint(pv=[prv[0], -1], nx=None) == 0 and deint(c=[cur[0], cur[0]], pv=[cur[0], cur[1]], nx=[prv[1], prv[1]]) == 0
    assert separate() == 0 and separate(t=None) == 0 and separate(b=None, s=[frames[0], frames[0]]) == 0
    assert weave(t=bots, b=tops) == 0 and weave(t=[tops[0], tops[0]], b=[tops[0], bots[1]]) == 0
    eng.sync()
    after = sums()
    changed = [i for i in range(len(watched)) if after[i] != before[i]]
    assert changed == [watched.index(pid) for pid in tops + bots + frames + dst]
    eng.close()
