"""-m gpu: oh_pics_reformat / Engine.pics_reformat on the MI355X against the numpy model of tests/reformat_model.py, every coded plane of
every destination bit for bit: all pairs of chroma formats at six pairs of bit depths, the seam of the kernel's segments, the single
rounding of a filter and a depth change together, batches of more than one launch set, the finished halves, the call next to
oh_pics_import, oh_pics_compose and oh_pics_compare, and the argument rules."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compose_model as PM                                                  # noqa: E402
import picture_hash as PH                                                   # noqa: E402
import reformat_model as RM                                                 # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DEPTH_NAMES = {RM.ROUND: "round", RM.DITHER: "dither"}
FILTER_NAMES = {RM.POINT: "point", RM.LINEAR: "linear"}


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def random_pic(p, rng, top=None):
    """random samples with 0 and the maximum (or top) in every plane"""
    hp = F.HostPic(p)
    top = (1 << p.bit_depth) - 1 if top is None else top
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        v[...] = rng.integers(0, top + 1, v.shape, dtype=v.dtype)
        flat = rng.permutation(v.size)
        v.reshape(-1)[flat[:4]] = (0, top, top, 0)
        v[-1, -1], v[0, 0] = top, 0
    return hp


def new(eng, p, rng, top=None):
    """(id, HostPic) of an uploaded picture"""
    hp = random_pic(p, rng, top)
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid, hp


def coded(hp):
    return [hp.visible(c) for c in range(len(hp.planes))]


def model(hp, dp, depth=RM.ROUND, down=RM.LINEAR, up=RM.LINEAR):
    sp = hp.params
    return RM.reformat(coded(hp), sp.bit_depth, sp.chroma_format_idc, dp.bit_depth, dp.chroma_format_idc, depth, down, up)


def verify(eng, pid, dp, want, what=None):
    got = eng.pic_download(pid, dp)
    assert len(want) == F.n_planes(dp)
    for c in range(F.n_planes(dp)):
        assert np.array_equal(got.visible(c), want[c]), (what, c, np.argwhere(got.visible(c) != want[c])[:4])


def check(eng, srcs, dst_ids, dp, depth=RM.ROUND, down=RM.LINEAR, up=RM.LINEAR, what=None):
    """one call on [(id, HostPic)] into dst_ids against the model"""
    ids = [s[0] for s in srcs]
    assert eng.pics_reformat(ids, depth=DEPTH_NAMES[depth], down=FILTER_NAMES[down], up=FILTER_NAMES[up], out=dst_ids) == list(dst_ids)
    for (_, hp), d in zip(srcs, dst_ids):
        verify(eng, d, dp, model(hp, dp, depth, down, up), what)
        assert eng.pic_final_half(d) == 0


def direction(scf, dcf):
    """-1 chroma is sub-sampled further, 1 less, 0 neither (or no chroma on one side)"""
    if not scf or not dcf or scf == dcf:
        return 0
    return -1 if dcf < scf else 1


DEPTH_PAIRS = [(8, 8), (8, 10), (10, 8), (12, 8), (10, 12), (9, 10)]
SIZES = [(16, 8), (24, 16)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("sbd,dbd", DEPTH_PAIRS, ids=[f"{a}to{b}" for a, b in DEPTH_PAIRS])
def test_all_format_pairs(sbd, dbd, w, h):
    """the sixteen pairs of chroma formats at one pair of depths: both depth modes, and both filters of the direction that applies (the
    other field set to the other value: it must not matter).  24 wide: 12-byte 8-bit chroma rows, no whole granule; 16 x 8: the clamps
    of j1 and k2 in every class of row and column"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(sbd * 100 + dbd + w)
    eng = Engine(0)
    srcs = [new(eng, params(w, h, sbd, cf), rng) for cf in range(4)]
    dps = [params(w, h, dbd, cf) for cf in range(4)]
    dsts = [eng.pic_alloc(dp) for dp in dps]
    for scf, dcf, depth in itertools.product(range(4), range(4), (RM.ROUND, RM.DITHER)):
        d = direction(scf, dcf)
        for filt in ((RM.LINEAR,) if d == 0 else (RM.POINT, RM.LINEAR)):
            down, up = (filt, 1 - filt) if d < 0 else (1 - filt, filt)
            check(eng, [srcs[scf]], [dsts[dcf]], dps[dcf], depth, down, up, what=(scf, dcf, depth, down, up))
    eng.close()


@pytest.mark.parametrize("scf,dcf", [(1, 3), (3, 1)], ids=["420to444", "444to420"])
def test_segment_seam(scf, dcf):
    """a picture 8 luma samples wider than the kernel's segment, 10 -> 8 bit with the linear filter and the dither: the filter's halo
    and the dither's phase across the seam, in luma and in the chroma plane that is up-sampled (its destination row has the seam) or
    sub-sampled (its source row has it)"""
    from openhevc_amd.engine import Engine
    w, h = E.RF_SEG + 8, 8
    rng = np.random.default_rng(scf)
    eng = Engine(0)
    src = new(eng, params(w, h, 10, scf), rng)
    dp = params(w, h, 8, dcf)
    dst = eng.pic_alloc(dp)
    check(eng, [src], [dst], dp, RM.DITHER, RM.LINEAR, RM.LINEAR, what="seam")
    want = model(src[1], dp, RM.DITHER)
    seam = E.RF_SEG // 2 if dcf == 1 else E.RF_SEG                           # in destination chroma columns
    assert want[1].shape[1] > seam and want[0].shape[1] > E.RF_SEG
    eng.close()


@pytest.mark.parametrize("depth", (RM.ROUND, RM.DITHER), ids=["round", "dither"])
def test_filter_and_depth_round_once(depth):
    """4:4:4 12 bit -> 4:2:0 8 bit at 64 x 64: f = 3 and k = 4 make one rounding at s = 7, which rounding twice would not equal"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(70 + depth)
    eng = Engine(0)
    src = new(eng, params(64, 64, 12, 3), rng)
    dp = params(64, 64, 8, 1)
    dst = eng.pic_alloc(dp)
    check(eng, [src], [dst], dp, depth, what="s = 7")
    want = model(src[1], dp, depth)
    mid = RM.reformat(coded(src[1]), 12, 3, 12, 1, depth)                   # the filter alone, then the depth alone: two roundings
    twice = RM.reformat(mid, 12, 1, 8, 1, depth)
    assert any(not np.array_equal(a, b) for a, b in zip(want[1:], twice[1:]))
    eng.close()


def test_more_than_one_launch_set():
    """65 pictures of 16 x 8 in one call, each with its own content: 4:2:0 8 bit -> 4:4:4 10 bit and back down with the dither"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(65)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 1
    sp, dp = params(16, 8, 8, 1), params(16, 8, 10, 3)
    srcs = [new(eng, sp, rng) for _ in range(n)]
    ids = eng.pics_reformat([s[0] for s in srcs], bit_depth=10, chroma_format_idc=3)
    assert len(ids) == n and len(set(ids)) == n and not set(ids) & {s[0] for s in srcs}
    for (_, hp), d in zip(srcs, ids):
        verify(eng, d, dp, model(hp, dp), "up")
    back = [eng.pic_alloc(sp) for _ in range(n)]
    eng.pics_reformat(ids, depth="dither", down="linear", out=back)
    for (_, hp), d in zip(srcs, back):
        wide = F.HostPic(dp)
        for c, pl in enumerate(model(hp, dp)):
            wide.visible(c)[...] = pl
        verify(eng, d, sp, model(wide, sp, RM.DITHER), "down")
    eng.close()


def test_state_and_halves():
    """a source whose finished half is half 1 is read there; a destination that oh_pic_wrap made, and one whose finished half was 1:
    half 0 is written and becomes the finished one; two calls back to back into the same destinations leave the second"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(12)
    eng = Engine(0)
    sp, dp = params(64, 32, 10, 1), params(64, 32, 8, 3)
    a, b = new(eng, sp, rng), random_pic(sp, rng)
    # a source whose finished half is half 1: uploads go to half 0, so b is uploaded through a picture wrapped over the same memory with
    # the halves swapped
    half = eng.L.oh_pic_bytes(C.byref(sp)) // 2
    mem = torch.zeros(2 * half, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    own = eng.pic_wrap(sp, mem.data_ptr() + half, mem.data_ptr(), half)     # its half 0 is the upper block, its half 1 the lower
    eng.pic_upload(own, b)                                                  # b in the upper block
    twin = eng.pic_wrap(sp, mem.data_ptr(), mem.data_ptr() + half, half)    # the same memory: half 1 holds b, half 0 zeros
    eng.pic_set_final_half(twin, 1)
    assert eng.pic_final_half(twin) == 1
    # destinations: one wrapped, one allocated whose finished half is 1
    dhalf = eng.L.oh_pic_bytes(C.byref(dp)) // 2
    dmem = torch.full((2 * dhalf,), 0x55, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    dw = eng.pic_wrap(dp, dmem.data_ptr(), dmem.data_ptr() + dhalf, dhalf)
    da = eng.pic_alloc(dp)
    eng.pic_upload(da, random_pic(dp, rng))
    eng.pic_set_final_half(da, 1)
    eng.pic_set_final_half(dw, 1)
    assert eng.pics_reformat([twin, a[0]], depth="dither", out=[dw, da]) == [dw, da]
    assert eng.pic_final_half(dw) == 0 and eng.pic_final_half(da) == 0
    verify(eng, dw, dp, model(b, dp, RM.DITHER), "finished half 1 of the source, wrapped destination")
    verify(eng, da, dp, model(a[1], dp, RM.DITHER), "allocated destination")
    assert (dmem[dhalf:] == 0x55).all()                                     # half 1 of the wrapped destination: untouched
    # back to back, no wait between: the second call's result stays
    eng.pics_reformat([a[0], twin], depth="round", up="nearest", out=[dw, da])
    eng.pics_reformat([twin, a[0]], depth="round", up="linear", out=[dw, da])
    verify(eng, dw, dp, model(b, dp, RM.ROUND), "second call")
    verify(eng, da, dp, model(a[1], dp, RM.ROUND), "second call")
    assert eng.pic_final_half(dw) == 0 and eng.pic_final_half(da) == 0
    eng.close()


def test_equals_import_of_the_8_bit_image():
    """8 -> 10 bit of a picture is oh_pics_import of its planar 8-bit image into a 10-bit picture: the same checksums"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(810)
    eng = Engine(0)
    for cf in (1, 2, 3, 0):
        sp, dp = params(48, 24, 8, cf), params(48, 24, 10, cf)
        pid, hp = new(eng, sp, rng)
        image = np.concatenate([pl.reshape(-1) for pl in coded(hp)]).astype(np.uint8).reshape(1, -1, 48)
        imp, win = eng.pics_import(torch.from_numpy(image).to(DEV), "planar", bit_depth=10, chroma_format_idc=cf)
        assert win == (0, 0, 0, 0)
        ref = eng.pics_reformat([pid], bit_depth=10)
        sums = eng.pics_hash(ref + imp, 2)
        assert sums[0] == sums[1] == PH.picture_hash(model(hp, dp), 10, 2), cf
    eng.close()


def test_compose_after_reformat():
    """an 8-bit 4:4:4 layer onto 10-bit 4:2:0 destinations: refused as it is, composed after the reformat, equal to the models chained"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(44)
    eng = Engine(0)
    p, pl8, pl = params(96, 48, 10, 1), params(32, 16, 8, 3), params(32, 16, 10, 1)
    dst, logo = new(eng, p, rng), new(eng, pl8, rng)
    with pytest.raises(E.EngineError) as ei:
        eng.pics_compose([dst[0]], [E.Layer(logo[0], None, (20, 10), 200)])
    assert ei.value.code == E.OH_E_UNSUPPORTED
    verify(eng, dst[0], p, coded(dst[1]), "refused: untouched")
    fit = eng.pics_reformat([logo[0]], bit_depth=10, chroma_format_idc=1)
    eng.pics_compose([dst[0]], [E.Layer(fit[0], None, (20, 10), 200)])
    want = PM.compose(coded(dst[1]), p, [{"src": model(logo[1], pl), "at": (20, 10), "opacity": 200}])
    verify(eng, dst[0], p, want, "composed")
    eng.close()


def test_compare_after_a_round_trip():
    """10 -> 8 -> 10 bit with rounding moves a sample by at most 2 of the 10-bit scale (k = 2: half a step of 4), apart from the clamp
    at the top — 1022 and 1023 round to 256, which 8 bits do not hold, and come back as 1020 —, which the model predicts"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(1082)
    eng = Engine(0)
    p, p8 = params(64, 32, 10, 1), params(64, 32, 8, 1)
    for top, bound in ((1021, 2), (1023, 3)):
        pid, hp = new(eng, p, rng, top)
        down = eng.pics_reformat([pid], bit_depth=8)
        back = eng.pics_reformat(down, bit_depth=10)
        low = F.HostPic(p8)
        for c, pl in enumerate(model(hp, p8)):
            low.visible(c)[...] = pl
        want = model(low, p)
        verify(eng, back[0], p, want, "round trip")
        cmp = eng.pics_compare([pid], back, ssim=False)[0]
        for c in range(3):
            figure = int(np.abs(want[c] - coded(hp)[c].astype(np.int64)).max())
            print(f"top {top} plane {c}: max_abs {cmp.plane[c].max_abs}, the model's {figure}")
            assert cmp.plane[c].max_abs == figure == bound, (top, c)
    eng.close()


def test_argument_errors_write_nothing():
    """every OH_E_ARG rule of ohevc_hip.h through the raw C call: refused on the host, the destinations' checksums stay; n == 0 is fine"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)
    sp, dp = params(32, 16, 10, 1), params(32, 16, 8, 3)
    src = [new(eng, sp, rng)[0] for _ in range(2)]
    dst = [new(eng, dp, rng)[0] for _ in range(2)]
    other_s, other_d = new(eng, params(32, 16, 10, 2), rng)[0], new(eng, params(32, 16, 9, 3), rng)[0]
    wide, tall = new(eng, params(40, 16, 8, 3), rng)[0], new(eng, params(32, 24, 8, 3), rng)[0]
    wide2, tall2 = new(eng, params(40, 16, 8, 3), rng)[0], new(eng, params(32, 24, 8, 3), rng)[0]
    same = [new(eng, sp, rng)[0] for _ in range(2)]                         # destinations of the sources' kind
    watched = dst + [other_d, wide, tall, wide2, tall2] + same + src

    def sums():
        return [eng.pics_hash([pid], 2) for pid in watched]

    before = sums()
    keep = []

    def ids(v):
        a = (C.c_int * max(len(v), 1))(*v)
        keep.append(a)
        return a

    def call(s=src, d=dst, n=None, rf=(0, 1, 1), rf_null=False, e_null=False):
        r = E.OhReformat(*rf)
        return L.oh_pics_reformat(None if e_null else eng.h, ids(s) if s is not None else None, ids(d) if d is not None else None,
                                  len(s or d or []) if n is None else n, None if rf_null else C.byref(r))

    arg = E.OH_E_ARG
    assert call(e_null=True) == arg and call(rf_null=True) == arg and call(s=None, n=2) == arg and call(d=None, n=2) == arg   # null arguments
    assert call(n=-1) == arg
    assert call(s=[src[0], 999]) == arg and call(d=[dst[0], 999]) == arg and call(s=[-1, src[1]]) == arg     # unknown pictures
    assert call(s=[src[0], other_s]) == arg and call(d=[dst[0], other_d]) == arg                            # params differ among themselves
    assert call(d=[wide, wide2]) == arg and call(d=[tall, tall2]) == arg                                    # another width, another height
    assert call(d=[dst[0], dst[0]]) == arg                                                                  # a destination twice
    assert call(s=src, d=[same[0], src[0]]) == arg and call(s=src, d=[src[1], same[1]]) == arg and call(s=src, d=src) == arg   # source and destination
    for rf in ((2, 1, 1), (-1, 1, 1), (0, 2, 1), (0, -1, 0), (0, 1, 2), (1, 0, -1), (1 << 20, 0, 0)):
        assert call(rf=rf) == arg, rf                                                                       # enum values outside their lists
        assert call(s=[], d=[], n=0, rf=rf) == arg, rf                                                      # also with nothing to do
    eng.sync()
    assert sums() == before, "a refused call wrote into a picture"
    assert call(s=[], d=[], n=0) == 0 and call(s=None, d=None, n=0) == 0                                    # n == 0
    eng.sync()
    assert sums() == before
    for rf in itertools.product((0, 1), (0, 1), (0, 1)):                                                    # every value inside the lists
        assert call(rf=rf) == 0, rf
    assert call(s=[src[0], src[0]], d=same) == 0                                                            # a source twice is fine
    eng.sync()
    after = sums()
    assert after[0] != before[0] and after[1] != before[1] and after[2:7] == before[2:7] and after[9:] == before[9:]
    eng.close()


def test_nothing_to_do():
    """n == 0 gives OH_OK and no pictures, with and without destinations given"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    assert eng.pics_reformat([], bit_depth=8) == [] and eng.pics_reformat([], out=[]) == []
    with pytest.raises(ValueError):
        eng.pics_reformat([], depth="floyd")
    eng.close()
