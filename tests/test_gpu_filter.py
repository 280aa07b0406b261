"""-m gpu: oh_pics_filter and Engine.pics_filter on the MI355X against the numpy model of tests/filter_model.py, every coded plane of
every destination bit for bit: every mode at every chroma format and two bit depths, the plane mask, the seams between the kernel's
tiles, the extreme planes, a batch of more than one launch, the finished halves, the calls next to oh_pics_hash, oh_pics_convert and
oh_pics_resize, and the argument rules.  Which branches these planes reach is asserted on the CPU by tests/test_filter_host.py."""
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
import picture_hash as PH                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZE_IDS = [f"{w}x{h}" for w, h in FM.SIZES]
MODES = (FM.CONVOLVE, FM.UNSHARP, FM.MEDIAN, FM.TEMPORAL)
BIG = dict(luma=(FM.LOBES15, FM.SKEW15), chroma=(FM.SKEW15, FM.LOBES15))     # the largest radius on both axes in both classes


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def host_pic(p, planes):
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        hp.visible(c)[...] = planes[c]
    return hp


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


def mode_cases(bd):
    """(name, mode, keyword arguments) of every case but TEMPORAL's"""
    cases = [(name, FM.CONVOLVE, dict(luma=luma, chroma=chroma)) for name, luma, chroma in FM.CONVOLVE_SETS]
    cases += [("unsharp " + name, FM.UNSHARP, kw) for name, kw in FM.unsharp_cases(bd)]
    return cases + [("median", FM.MEDIAN, dict())]


@pytest.mark.parametrize("w,h", FM.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("bd", FM.DEPTHS)
def test_every_mode(bd, w, h):
    """CONVOLVE with binomial 3, 5 and 9, a box 7 x 3, skewed 3 x 1 and 15 x 15 sets with negative lobes; UNSHARP with amounts of
    either sign, with and without threshold; MEDIAN; TEMPORAL on related_triplet with prev and next of their own, then without; chroma
    formats 0 .. 3.  At 4:2:0, 16 x 8 has chroma planes of 8 x 4: a radius of 7 clamps on both sides at once."""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for cf in range(4):
        p = params(w, h, bd, cf)
        src = FM.random_planes(bd, w, h, cf, FM.source_seed(bd, w, h, cf))
        sid = put(eng, p, src)
        dst = eng.pic_alloc(p)
        for name, mode, kw in mode_cases(bd):
            assert eng.pics_filter([sid], mode, out=[dst], **kw) == [dst]
            verify(eng, dst, p, FM.filter_pic(src, mode, bd, **kw), (cf, name))
        P, Cu, N = FM.related_triplet(bd, w, h, cf)
        ids = [put(eng, p, v) for v in (P, Cu, N)]
        for thr in FM.temporal_thresholds(bd):
            eng.pics_filter([ids[1]], "temporal", threshold=thr, prev=[ids[0]], next=[ids[2]], out=[dst])
            verify(eng, dst, p, FM.filter_pic(Cu, FM.TEMPORAL, bd, threshold=thr, prev=P, nxt=N), (cf, "temporal", thr))
        thr = FM.temporal_thresholds(bd)[0]
        # two pictures in one call: the first has no prev (an entry of -1), the second no next; then null arrays
        got = eng.pics_filter([ids[1], ids[1]], "temporal", threshold=thr, prev=[None, ids[0]], next=[ids[2], None])
        verify(eng, got[0], p, FM.filter_pic(Cu, FM.TEMPORAL, bd, threshold=thr, nxt=N), (cf, "prev -1"))
        verify(eng, got[1], p, FM.filter_pic(Cu, FM.TEMPORAL, bd, threshold=thr, prev=P), (cf, "next -1"))
        bare = eng.pics_filter([ids[1]], FM.TEMPORAL, threshold=thr)
        assert bare[0] not in ids + [sid, dst] + got and eng.pic_final_half(bare[0]) == 0
        verify(eng, bare[0], p, Cu, (cf, "no neighbours"))
        half = eng.pics_filter([ids[1]], FM.TEMPORAL, threshold=thr, next=[ids[2]])
        verify(eng, half[0], p, FM.filter_pic(Cu, FM.TEMPORAL, bd, threshold=thr, nxt=N), (cf, "prev null"))
        default = eng.pics_filter([sid], "convolve")                         # the default taps: binomial 3 x 3
        verify(eng, default[0], p, FM.filter_pic(src, FM.CONVOLVE, bd), (cf, "default taps"))
        for pid in ids + [sid, dst] + got + bare + half + default:
            eng.pic_free(pid)
    eng.close()


@pytest.mark.parametrize("mode", MODES)
def test_plane_mask(mode):
    """every value of planes: the planes not selected equal the source; a 4:0:0 picture ignores the chroma bits"""
    from openhevc_amd.engine import Engine
    bd, w, h = 10, 24, 16
    eng = Engine(0)
    kw = dict(luma=(FM.box(5), FM.SKEW3), chroma=(FM.SKEW3, FM.box(3)), amount=(100, -40), threshold=(2, 30))
    for cf in (1, 3, 0):
        p = params(w, h, bd, cf)
        P, Cu, N = FM.related_triplet(bd, w, h, cf, seed=77 + cf)
        ids = [put(eng, p, v) for v in (P, Cu, N)]
        dst = eng.pic_alloc(p)
        for planes in range(8):
            eng.pic_upload(dst, host_pic(p, P))                              # something else than the result in every plane
            eng.pics_filter([ids[1]], mode, planes=planes, prev=[ids[0]], next=[ids[2]], out=[dst], **kw)
            want = FM.filter_pic(Cu, mode, bd, planes=planes, prev=P, nxt=N, **kw)
            for c in range(len(Cu)):
                assert np.array_equal(want[c], Cu[c]) == (not planes >> c & 1) or mode == FM.TEMPORAL, (planes, c)
            verify(eng, dst, p, want, (cf, planes))
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_tile_seams(bd):
    """The kernel's units are a tile of FILTER_TW = 128 samples across and FILTER_TH = 32 rows.  A 4:2:0 picture whose chroma planes are
    one 16-byte granule wider and four rows taller than a tile (coded sizes are multiples of 8): the chroma planes take 2 x 2 tiles, the
    luma planes 3 x 3, the last tile of a row one (chroma) or two (luma) granules wide; every mode at the largest radius, so that
    windows cross every seam from both sides and the last rows clamp inside a tile of four (chroma) or eight (luma) rows"""
    from openhevc_amd.engine import Engine
    gs = 16 if bd == 8 else 8
    w, h = 2 * (E.FILTER_TW + gs), 2 * (E.FILTER_TH + 4)
    eng = Engine(0)
    p = params(w, h, bd, 1)
    P, Cu, N = FM.related_triplet(bd, w, h, 1, seed=300 + bd)
    ids = [put(eng, p, v) for v in (P, Cu, N)]
    dst = eng.pic_alloc(p)
    cases = [("convolve", FM.CONVOLVE, BIG), ("unsharp", FM.UNSHARP, dict(amount=(200, -64), threshold=(3, 1), **BIG)),
             ("convolve 9 x 5", FM.CONVOLVE, dict(luma=(FM.binomial(9), FM.binomial(5)), chroma=(FM.binomial(5), FM.binomial(9)))),
             ("median", FM.MEDIAN, dict()), ("temporal", FM.TEMPORAL, dict(threshold=FM.temporal_thresholds(bd)[0]))]
    for name, mode, kw in cases:
        eng.pics_filter([ids[1]], mode, prev=[ids[0]], next=[ids[2]], out=[dst], **kw)
        verify(eng, dst, p, FM.filter_pic(Cu, mode, bd, prev=P, nxt=N, **kw), name)
    # a width that is no multiple of the granule: the last granule of the chroma rows (at 8 bit of the luma rows too) is partial
    w2 = w + 8
    assert (w2 // 2) % gs and (bd != 8 or w2 % gs)
    p2 = params(w2, 8, bd, 1)
    src = FM.random_planes(bd, w2, 8, 1, 9)
    sid = put(eng, p2, src)
    for name, mode, kw in cases[:4]:
        out = eng.pics_filter([sid], mode, **kw)
        verify(eng, out[0], p2, FM.filter_pic(src, mode, bd, **kw), (name, "partial granule"))
    eng.close()


@pytest.mark.parametrize("bd", (8, 12))
def test_extremes(bd):
    """planes of all 0, all M and checkerboards of 0 / M with 15-tap sets whose magnitudes sum to 512 on both axes, UNSHARP at amount
    512, MEDIAN, and TEMPORAL between a checkerboard and its inverse at the smallest and the largest threshold"""
    from openhevc_amd.engine import Engine
    M = (1 << bd) - 1
    w, h, cf = 40, 24, 1
    eng = Engine(0)
    p = params(w, h, bd, cf)
    planes = FM.extreme_planes(bd, w, h, cf)
    ids = {name: put(eng, p, v) for name, v in planes}
    dst = eng.pic_alloc(p)
    for name, src in planes:
        for what, mode, kw in (("convolve", FM.CONVOLVE, BIG), ("convolve, skew both", FM.CONVOLVE, dict(luma=(FM.SKEW15, FM.SKEW15), chroma=(FM.LOBES15, FM.LOBES15))),
                               ("unsharp", FM.UNSHARP, dict(amount=512, threshold=0, **BIG)), ("unsharp, soft", FM.UNSHARP, dict(amount=-64, threshold=(M, 0), **BIG)),
                               ("median", FM.MEDIAN, dict())):
            eng.pics_filter([ids[name]], mode, out=[dst], **kw)
            verify(eng, dst, p, FM.filter_pic(src, mode, bd, **kw), (name, what))
    by_name = dict(planes)
    for a, b, c in (("checker", "checker'", "zeros"), ("full", "zeros", "checker"), ("zeros", "full", "full")):
        for thr in (0, 9 * M - 1, 9 * M):
            eng.pics_filter([ids[a]], "temporal", threshold=thr, prev=[ids[b]], next=[ids[c]], out=[dst])
            verify(eng, dst, p, FM.filter_pic(by_name[a], FM.TEMPORAL, bd, threshold=thr, prev=by_name[b], nxt=by_name[c]), (a, b, c, thr))
    eng.close()


def test_more_than_one_launch():
    """CONV_MAX_PICS + 1 pictures of 16 x 8 in one call, each with its own content: TEMPORAL with a mix of real and None neighbours,
    and UNSHARP"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 1
    bd = 10
    p = params(16, 8, bd, 1)
    planes = [FM.random_planes(bd, 16, 8, 1, 1000 + i) for i in range(n)]
    for i in range(1, n, 2):                                                 # every other picture close to the one before it
        planes[i] = [np.clip(a.astype(np.int64) + (i % 3) - 1, 0, 1023).astype(a.dtype) for a in planes[i - 1]]
    ids = [put(eng, p, v) for v in planes]
    prev = [None if i % 3 == 0 else ids[i - 1] for i in range(n)]
    nxt = [ids[i + 1] if i + 1 < n else None for i in range(n)]
    out = eng.pics_filter(ids, "temporal", threshold=(9, 18), prev=prev, next=nxt)
    assert len(out) == n and len(set(out)) == n and not set(out) & set(ids)
    for i in range(n):
        want = FM.filter_pic(planes[i], FM.TEMPORAL, bd, threshold=(9, 18), prev=None if prev[i] is None else planes[i - 1],
                             nxt=planes[i + 1] if i + 1 < n else None)
        verify(eng, out[i], p, want, ("temporal", i))
    kw = dict(luma=(FM.binomial(5), FM.SKEW3), chroma=(FM.SKEW3, FM.binomial(5)), amount=96, threshold=2)
    eng.pics_filter(ids, "unsharp", out=out, **kw)
    for i in (0, 1, n - 2, n - 1):
        verify(eng, out[i], p, FM.filter_pic(planes[i], FM.UNSHARP, bd, **kw), ("unsharp", i))
    eng.close()


def test_state_and_halves():
    """sources whose finished half is half 1 are read there; destinations whose finished half was 1 get half 0 written and marked; two
    calls into one destination back to back"""
    from openhevc_amd.engine import Engine
    bd = 10
    eng = Engine(0)
    p = params(32, 16, bd, 1)
    a, b = FM.random_planes(bd, 32, 16, 1, 1), FM.random_planes(bd, 32, 16, 1, 2)
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
    eng.pic_upload(dst, host_pic(p, FM.random_planes(bd, 32, 16, 1, 3)))
    eng.pic_set_final_half(dst, 1)
    M = 1023
    assert eng.pics_filter([twin], "temporal", threshold=9 * M, prev=[ia], next=[twin], out=[dst]) == [dst]
    assert eng.pic_final_half(dst) == 0
    verify(eng, dst, p, FM.filter_pic(b, FM.TEMPORAL, bd, threshold=9 * M, prev=a, nxt=b), "src and next in half 1")
    eng.pic_set_final_half(dst, 1)
    eng.pics_filter([ia], "median", out=[dst])
    eng.pics_filter([twin], "convolve", luma=(FM.box(7), FM.box(3)), out=[dst])       # back to back, no wait between: the second call's result stays
    assert eng.pic_final_half(dst) == 0
    verify(eng, dst, p, FM.filter_pic(b, FM.CONVOLVE, bd, luma=(FM.box(7), FM.box(3))), "second call")
    eng.close()


def test_next_to_hash_convert_and_resize():
    """the result hashes like the model on the host and converts (4:4:4 planar is the model's planes one below the other) with no wait
    in between; oh_pics_resize followed by UNSHARP in one stream equals UNSHARP of the downloaded resized picture"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    for bd in (8, 10):
        p = params(24, 16, bd, 3)
        P, Cu, N = FM.related_triplet(bd, 24, 16, 3)
        ids = [put(eng, p, v) for v in (P, Cu, N)]
        thr = FM.temporal_thresholds(bd)[0]
        for mode, kw in ((FM.CONVOLVE, dict(luma=(FM.binomial(9), FM.SKEW3))), (FM.UNSHARP, dict(amount=128, threshold=1)), (FM.MEDIAN, dict()),
                         (FM.TEMPORAL, dict(threshold=thr))):
            out = eng.pics_filter([ids[1]], mode, prev=[ids[0]], next=[ids[2]], **kw)
            want = FM.filter_pic(Cu, mode, bd, prev=P, nxt=N, **kw)
            for ht in (1, 2):
                assert eng.pics_hash(out, ht)[0] == PH.picture_hash(want, bd, ht), (bd, mode, ht)
            img = eng.pics_convert(out, "planar").cpu().numpy()
            assert img.shape == (1, 48, 24) and np.array_equal(img[0], np.concatenate(want)), (bd, mode)
            eng.pic_free(out[0])
        # a picture down-scaled and sharpened: both calls enqueued, nothing waited for in between
        big = params(96, 64, bd, 1)
        src = FM.random_planes(bd, 96, 64, 1, 40 + bd)
        sid = put(eng, big, src)
        small, _ = eng.pics_resize([sid], (48, 32))
        sharp = eng.pics_filter(small, "unsharp", amount=(96, 48), threshold=(2, 1))
        sp = params(48, 32, bd, 1)
        mid = eng.pic_download(small[0], sp)
        resized = [np.array(mid.visible(c)) for c in range(3)]
        assert not np.array_equal(resized[0], src[0][:32, :48])
        verify(eng, sharp[0], sp, FM.filter_pic(resized, FM.UNSHARP, bd, amount=(96, 48), threshold=(2, 1)), ("resize, unsharp", bd))
    eng.close()


def test_errors_write_nothing():
    """every OH_E_ARG rule of ohevc_hip.h through the raw C call: refused on the host, and behind each refusal the checksums of all
    pictures in play are fetched and have not moved; n == 0 is fine; the fields a mode does not read are not checked; then the calls
    inside the rules succeed"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    bd = 10
    M = (1 << bd) - 1

    seeds = itertools.count(500, 10)

    def some(p, k=2):
        seed = next(seeds)
        return [put(eng, p, FM.random_planes(p.bit_depth, p.width, p.height, p.chroma_format_idc, seed + i)) for i in range(k)]
    p = params(32, 16, bd, 1)
    src, dst, prv = some(p), some(p), some(p)
    small, deep, full = some(params(16, 16, bd, 1)), some(params(32, 16, 8, 1)), some(params(32, 16, bd, 3))
    odd = put(eng, F.pic_params(32, 16, bit_depth=bd, chroma_format_idc=1, log2_ctb_size=5), FM.random_planes(bd, 32, 16, 1, 99))
    watched = src + dst + prv + small + deep + full + [odd]
    arg = E.OH_E_ARG

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

    def spec(mode=1, planes=7, luma=None, chroma=None, amount=(64, 64), threshold=(0, 0)):
        f = E.OhFilter(mode, planes)
        for q, t in enumerate((luma, chroma)):
            if t is None:
                t = (3, 3, [64, 128, 64], [64, 128, 64])
            f.taps[q].nh, f.taps[q].nv = t[0], t[1]
            f.taps[q].h[:len(t[2])] = t[2]
            f.taps[q].v[:len(t[3])] = t[3]
        f.amount[0], f.amount[1] = amount
        f.threshold[0], f.threshold[1] = threshold
        return f

    def filt(s=src, d=dst, pv=None, nx=None, n=2, f_null=False, e_null=False, **kw):
        f = spec(**kw)
        rc = L.oh_pics_filter(None if e_null else eng.h, ids(pv), ids(s), ids(nx), ids(d), n, None if f_null else C.byref(f))
        if rc != 0:
            assert sums() == before, "a refused call wrote into a picture"
        return rc

    T = E.FILTER_TEMPORAL
    assert filt(e_null=True) == arg and filt(f_null=True) == arg and filt(s=None) == arg and filt(d=None) == arg and filt(n=-1) == arg
    assert filt(s=[src[0], 999]) == arg and filt(d=[999, dst[1]]) == arg                                                 # unknown pictures
    assert filt(mode=T, pv=[prv[0], 999]) == arg and filt(mode=T, nx=[777, -1]) == arg
    assert filt(mode=T, pv=[-2, prv[1]]) == arg and filt(mode=T, nx=[prv[0], -5]) == arg                                 # below -1
    assert filt(s=[src[0], small[0]]) == arg and filt(d=[dst[0], small[0]]) == arg and filt(d=[dst[0], odd]) == arg      # params differ
    assert filt(d=deep) == arg and filt(d=full) == arg and filt(d=small) == arg
    assert filt(mode=T, pv=[small[0], -1]) == arg and filt(mode=T, nx=[-1, full[0]]) == arg and filt(mode=T, pv=[odd, odd]) == arg
    assert filt(d=[dst[0], dst[0]]) == arg and filt(d=src) == arg and filt(d=[src[1], dst[0]]) == arg                    # twice; also a source
    assert filt(mode=T, pv=[dst[1], -1]) == arg and filt(mode=T, nx=[-1, dst[0]]) == arg                                 # a destination among prev / next
    for mode in (-1, 4, 1 << 20):
        assert filt(mode=mode) == arg and filt(s=[], d=[], n=0, mode=mode) == arg, mode
    for planes in (-1, 8, 1 << 16):
        for mode in range(4):
            assert filt(mode=mode, planes=planes) == arg, (mode, planes)
    bad_taps = [(2, 1, [128, 128], [256]), (1, 0, [256], []), (17, 1, [256], [256]), (3, 1, [64, 128, 63], [256]), (1, 3, [256], [64, 128, 65]),
                (3, 3, [-129, 514, -129], [64, 128, 64]), (3, 3, [64, 128, 64], [-200, 456, 0])]
    for t in bad_taps:
        for mode in (0, 1):
            assert filt(mode=mode, luma=t) == arg and filt(mode=mode, chroma=t) == arg, (mode, t)
            assert filt(mode=mode, chroma=t, planes=1) == arg and filt(mode=mode, luma=t, planes=6) == arg                # whatever planes says
    for v in (-65, 513, 1 << 20, -(1 << 20)):
        assert filt(amount=(v, 0)) == arg and filt(amount=(0, v)) == arg and filt(amount=(0, v), planes=1) == arg, v
    for v in (-1, M + 1, 1 << 30):
        assert filt(threshold=(v, 0)) == arg and filt(threshold=(0, v)) == arg, v
    for v in (-1, 9 * M + 1, 1 << 30):
        assert filt(mode=T, threshold=(v, 0)) == arg and filt(mode=T, threshold=(0, v), planes=1) == arg, v
    eng.sync()
    assert sums() == before, "a refused call wrote into a picture"
    # n == 0
    assert filt(s=[], d=[], n=0) == 0 and filt(s=None, d=None, n=0) == 0 and filt(s=None, d=None, n=0, mode=T) == 0
    eng.sync()
    assert sums() == before
    # inside the rules.  What a mode does not read is not checked: prev / next outside TEMPORAL, amount and threshold in CONVOLVE,
    # taps and amount in MEDIAN and TEMPORAL, the threshold in MEDIAN; a source twice is fine; the limits themselves are inside
    junk = (16, -3, [999] * 15, [-999] * 15)
    for mode in (0, 1, 2):
        assert filt(mode=mode, pv=[999, -7], nx=[dst[0], small[0]]) == 0, mode
    assert filt(mode=0, amount=(9999, -9999), threshold=(-5, 1 << 30)) == 0
    assert filt(mode=2, luma=junk, chroma=junk, amount=(9999, -9999), threshold=(-5, 1 << 30)) == 0
    assert filt(mode=T, luma=junk, chroma=junk, amount=(9999, -9999), threshold=(9 * M, 0)) == 0
    assert filt(mode=1, amount=(-64, 512), threshold=(M, 0)) == 0 and filt(mode=T, threshold=(M + 1, 9 * M)) == 0
    assert filt(mode=T, pv=[prv[0], -1], nx=None) == 0 and filt(mode=T, s=[src[0], src[0]], pv=[src[0], src[1]], nx=[prv[1], prv[1]]) == 0
    assert filt(planes=0) == 0
    eng.sync()
    after = sums()
    changed = [i for i in range(len(watched)) if after[i] != before[i]]
    assert changed == [watched.index(pid) for pid in dst]
    verify(eng, dst[0], p, [np.array(eng.pic_download(src[0], p).visible(c)) for c in range(3)], "planes 0 is a copy")
    eng.close()
