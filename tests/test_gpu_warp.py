"""-m gpu: oh_pics_warp / Engine.pics_warp on the MI355X against the numpy model of tests/warp_model.py, every coded plane of every
destination bit for bit: identity and translations at every filter, chroma format and border, the eight orientations against
oh_pics_orient, rotation and scale, both kernel paths (the staged box and the gather from global memory, told apart by the kernel's
own predicate oh_warp_paths), perspective maps down to the smallest denominator, windows, the layout of the destinations, batches of
more than one launch, the call next to oh_pics_convert and oh_pics_compare, from the SEI's bytes to the samples, and the refusals."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import warp_model as WM                                                     # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

WHOLE = (0, 0, 0, 0)
ONE, ONE30 = WM.ONE, WM.ONE30
FILTERS = (WM.NEAREST, WM.BILINEAR, WM.BICUBIC)
SIZES = ((16, 8), (24, 16), (72, 40))                                       # the last: more than one 64 x 16 tile both ways, partial tiles


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def random_pic(p, rng, columns=False):
    """random samples with 0 and the maximum in every plane; columns: columns alternate between 0 and the maximum"""
    hp = F.HostPic(p)
    top = (1 << p.bit_depth) - 1
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        if columns:
            v[...] = (np.arange(v.shape[1]) & 1)[None, :] * top
        else:
            v[...] = rng.integers(0, top + 1, v.shape, dtype=v.dtype)
            v[-1, -1], v[0, 0] = top, 0
    return hp


def new(eng, p, rng, **kw):
    hp = random_pic(p, rng, **kw)
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid, hp


def coded(hp):
    return [hp.visible(c) for c in range(len(hp.planes))]


def fills(bd):
    top = (1 << bd) - 1
    return (top // 3, top, 5)


def verify(eng, pid, dp, want, what=None):
    got = eng.pic_download(pid, dp)
    assert len(want) == F.n_planes(dp)
    for c in range(F.n_planes(dp)):
        assert np.array_equal(got.visible(c), want[c]), (what, c, np.argwhere(got.visible(c) != want[c])[:4])


def check(eng, src, m, size, mode=0, filt=1, border=0, fill=(0, 0, 0), window=WHOLE, out=None, what=None):
    """one call on (id, HostPic) against the model; the destination is out or made by the call and freed again"""
    pid, hp = src
    m = [int(v) for v in m.m] if isinstance(m, E.OhWarp) else m
    ids, win = eng.pics_warp([pid], m, size, mode=mode, filter=filt, border=border, fill=fill, window=window, out=None if out is None else [out])
    dp = eng._pic_params(ids[0])
    assert win == (0, dp.width - size[0], 0, dp.height - size[1])
    if out is None:
        assert (dp.width, dp.height) == (-(-size[0] // 8) * 8, -(-size[1] // 8) * 8)
    want = WM.warp(coded(hp), hp.params, window, m, size, dp, mode=mode, filt=filt, border=border, fill=fill)
    verify(eng, ids[0], dp, want, what)
    assert eng.pic_final_half(ids[0]) == 0
    if out is None:
        eng.pic_free(ids[0])
    return want


def paths(m, size, dp, mode=0, filt=1):
    w = E.warp_identity()
    w.mode, w.filter, w.width, w.height = mode, filt, size[0], size[1]
    for k, v in enumerate(m):
        w.m[k] = v
    return E.warp_paths(w, dp.bit_depth, dp.chroma_format_idc, dp.width, dp.height)


@pytest.mark.parametrize("bd", (8, 10))
def test_identity_and_integer_translations(bd):
    """all filters, chroma formats 0 .. 3, both borders (12 bit once); a translation by 2^20 samples, where every tap is border"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(bd)
    eng = Engine(0)
    for cf, (w, h) in itertools.product(range(4), SIZES):
        depth = 12 if (bd, cf, w) == (10, 1, 24) else bd
        src = new(eng, params(w, h, depth, cf), rng)
        for filt in FILTERS:
            got = check(eng, src, WM.IDENTITY, (w, h), filt=filt, what=("identity", cf, w, filt))
            assert all(np.array_equal(a, b) for a, b in zip(got, coded(src[1])))
            for (dx, dy), border in itertools.product(((12, -8), (-20, 4), (4 << 20, 0), (0, -(4 << 20))), (0, 1)):
                want = check(eng, src, WM.translation(dx, dy), (w, h), filt=filt, border=border, fill=fills(depth), what=(cf, w, filt, dx, dy, border))
                if abs(dx) + abs(dy) > 1 << 20 and border:
                    assert all((want[c] == fills(depth)[c]).all() for c in range(len(want)))
        eng.pic_free(src[0])
    eng.close()


def test_orientations_against_pics_orient():
    """the eight orientations as exact integer maps equal oh_pics_orient at every filter: all fractions are zero"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(8)
    eng = Engine(0)
    for cf, bd, (w, h) in ((0, 8, (24, 16)), (3, 10, (72, 40)), (3, 8, (16, 8))):
        src = new(eng, params(w, h, bd, cf), rng)
        for o in range(8):
            m, size = WM.orient_map(o, w, h)
            ref, rwin = eng.pics_orient([src[0]], o)
            dp = eng._pic_params(ref[0])
            want = coded(eng.pic_download(ref[0], dp))
            for filt in FILTERS:
                ids, win = eng.pics_warp([src[0]], m, size, mode="affine", filter=filt)
                assert win == rwin
                verify(eng, ids[0], dp, want, (cf, o, filt))
                eng.pic_free(ids[0])
            eng.pic_free(ref[0])
    eng.close()


@pytest.mark.parametrize("cf,bd", ((1, 10), (2, 8)))
def test_rotation_and_scale(cf, bd):
    """30 degrees and an angle with an odd code, scale 3/4 and 3/2, each filter, both borders with a fill; a quarter-sample translation"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(30 + bd)
    eng = Engine(0)
    for w, h in SIZES[1:]:
        src = new(eng, params(w, h, bd, cf), rng)
        centre = ((w - 1) << 15, (h - 1) << 15)
        for code, scale in itertools.product((5461, 12345), (49152, 98304)):
            m = list(E.warp_rotation(code, centre, centre, scale).m)
            for filt, border in itertools.product(FILTERS, (0, 1)):
                check(eng, src, m, (w, h), filt=filt, border=border, fill=fills(bd), what=(w, code, scale, filt, border))
        for filt, border in itertools.product(FILTERS, (0, 1)):
            check(eng, src, list(E.warp_translation(5, -3).m), (w, h), filt=filt, border=border, fill=fills(bd), what=("quarter", w, filt, border))
        eng.pic_free(src[0])
    eng.close()


def test_both_kernel_paths():
    """8 : 1 (136 x 72 into 16 x 8, and 520 x 136 into a whole tile of 64 x 16, whose box cannot be staged), 1 : 8 (16 x 8 into
    128 x 64), and a shear whose whole tiles gather while its partial tiles stage: both paths in one launch.  oh_warp_paths, the
    kernel's own predicate, says which paths ran: a path nobody ran is not tested"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(81)
    eng = Engine(0)
    ran = [0, 0]
    down = [8 * ONE, 0, 7 << 15, 0, 8 * ONE, 7 << 15, 0, 0, ONE30]
    up = [ONE // 8, 0, -(7 << 12), 0, ONE // 8, -(7 << 12), 0, 0, ONE30]
    shear = [ONE, 12 * ONE, -(150 << 16), 2 * ONE, ONE, -(40 << 16), 0, 0, ONE30]
    for cf, bd in ((1, 10), (3, 8)):
        cases = (((136, 72), down, (16, 8)), ((520, 136), down, (64, 16)), ((16, 8), up, (128, 64)), ((72, 40), shear, (72, 40)))
        for (sw, sh), m, size in cases:
            src = new(eng, params(sw, sh, bd, cf), rng)
            for filt in FILTERS:
                check(eng, src, m, size, filt=filt, what=(cf, sw, filt))
                st, ga = paths(m, size, params(size[0], size[1], bd, cf), filt=filt)
                ran[0] += st
                ran[1] += ga
                if (sw, m) == (520, down):
                    assert st == 0 and ga > 0                   # the whole tile at 8 : 1 cannot be staged
                if m is up:
                    assert ga == 0 and st > 0
                if m is shear:
                    assert st > 0 and ga > 0                    # both in one launch
            eng.pic_free(src[0])
    assert ran[0] > 0 and ran[1] > 0
    eng.close()


def test_perspective():
    """a keystone whose denominator falls to just above 2^20 at the image's last corner, on columns that alternate between 0 and the
    maximum; a perspective map with m6 = m7 = 0 and m8 = 2^30 equals the affine result"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(20)
    eng = Engine(0)
    w, h = 72, 40
    k = (ONE30 - (1 << 20) - 7) // (w - 1 + h - 1)
    low = ONE30 - k * (w - 1 + h - 1)
    assert 1 << 20 <= low < (1 << 20) + 128
    key = [ONE // 4, 0, 3 << 10, 0, ONE // 4, 1 << 10, -k, -k, ONE30]        # the numerator shrinks as the denominator does
    mild = [ONE, ONE // 8, -(2 << 16), -ONE // 16, ONE, 1 << 16, -(1 << 21), 3 << 20, ONE30 + 12345]
    for cf, bd in ((1, 10), (3, 8)):
        src = new(eng, params(w, h, bd, cf), rng, columns=True)
        noise = new(eng, params(w, h, bd, cf), rng)
        for m, filt, border in itertools.product((key, mild), FILTERS, (0, 1)):
            for s in (src, noise):
                check(eng, s, m, (w, h), mode=1, filt=filt, border=border, fill=fills(bd), what=(cf, m is key, filt, border))
        centre = ((w - 1) << 15, (h - 1) << 15)
        rot = list(E.warp_rotation(7001, centre, centre, 60000).m)
        for filt in FILTERS:
            a = check(eng, noise, rot, (w, h), mode=0, filt=filt)
            b = check(eng, noise, rot, (w, h), mode=1, filt=filt)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        below = key[:8] + [ONE30 - 128]                                       # the corner's denominator below 2^20
        with pytest.raises(E.EngineError) as err:
            eng.pics_warp([src[0]], below, (w, h))
        assert err.value.code == E.OH_E_ARG
        eng.pic_free(src[0])
        eng.pic_free(noise[0])
    eng.close()


def test_window():
    """a window with odd 4:2:0 chroma offsets in random content (its outside differs from its edge): replicate uses the window's edge,
    constant the fill; the model sees only the window"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(6)
    eng = Engine(0)
    for (w, h), window in (((24, 16), (2, 4, 2, 6)), ((72, 40), (6, 2, 10, 2))):
        assert (window[0] >> 1) & 1 and (window[2] >> 1) & 1
        src = new(eng, params(w, h, 10, 1), rng)
        iw, ih = w - window[0] - window[1], h - window[2] - window[3]
        for m in (WM.translation(-12, -8), WM.translation(9, 7), list(E.warp_rotation(3000, (0, 0), (0, 0), 70000).m)):
            for filt, border in itertools.product(FILTERS, (0, 1)):
                check(eng, src, m, (iw, ih), filt=filt, border=border, fill=fills(10), window=window, what=(w, filt, border))
        eng.pic_free(src[0])
    eng.close()


def test_layout_and_batches():
    """destinations larger than the image (the replicated rest), OH_CONV_MAX_PICS + 1 pictures in one call, half 0 finished"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(65)
    eng = Engine(0)
    for bd, cf in ((8, 1), (10, 3)):
        src = new(eng, params(16, 8, bd, cf), rng)
        dp = params(32, 24, bd, cf)
        dst = eng.pic_alloc(dp)
        eng.pic_upload(dst, random_pic(dp, rng))
        eng.pic_set_final_half(dst, 1)
        m = list(E.warp_rotation(2000, (15 << 15, 7 << 15), (15 << 15, 7 << 15)).m)
        want = check(eng, src, m, (16, 8), filt=2, out=dst)
        assert eng.pic_final_half(dst) == 0
        assert np.array_equal(want[0][:, 16:], np.repeat(want[0][:, 15:16], 16, axis=1)) and np.array_equal(want[0][8:], np.repeat(want[0][7:8], 16, axis=0))
    n = E.CONV_MAX_PICS + 1
    sp = params(16, 8, 10, 1)
    srcs = [new(eng, sp, rng) for _ in range(n)]
    m = list(E.warp_rotation(60000, (15 << 15, 7 << 15), (15 << 15, 7 << 15)).m)
    ids, win = eng.pics_warp([s[0] for s in srcs], m, (16, 8), mode="affine", filter="bicubic", border="constant", fill=fills(10))
    assert len(set(ids)) == n and not set(ids) & {s[0] for s in srcs} and win == WHOLE
    for (_, hp), d in zip(srcs, ids):
        verify(eng, d, sp, WM.warp(coded(hp), sp, WHOLE, m, (16, 8), sp, filt=2, border=1, fill=fills(10)), "batch")
        assert eng.pic_final_half(d) == 0
    eng.close()


def test_next_to_convert_compare_and_the_sei():
    """results feed pics_convert and pics_compare; from the SEI's bytes through warp_from_sei to the samples"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(47)
    eng = Engine(0)
    p = params(24, 16, 8, 3)
    pid, hp = new(eng, p, rng)
    rgb = eng.pics_convert([pid], "rgb_planar")
    m, size = WM.orient_map(3, 24, 16)
    ids, win = eng.pics_warp([pid], m, size, mode="affine", filter="bicubic")
    assert torch.equal(eng.pics_convert(ids, "rgb_planar", window=win), torch.rot90(rgb, 2, (2, 3)).contiguous())
    back, _ = eng.pics_warp(ids, m, size, mode="affine", filter="nearest")
    cmp = eng.pics_compare([pid], back, ssim=False)[0]
    assert [cmp.plane[c].differing for c in range(3)] == [0, 0, 0]
    assert eng.pics_compare([pid], ids, ssim=False)[0].plane[0].differing > 0
    p10 = params(24, 16, 10, 1)
    src = new(eng, p10, rng)
    for hf, vf, rot in itertools.product((0, 1), (0, 1), (0, 1 << 14, 5461, 40001)):
        bits = (hf << 22) | (vf << 21) | (rot << 5) | (1 << 4) | 0x8
        nal = bytes([39 << 1, 1, 47, 3]) + bits.to_bytes(3, "big") + b"\x80"
        d = A.display_orientation(nal)
        assert d["anticlockwise_rotation"] == rot and d["hor_flip"] == bool(hf) and d["ver_flip"] == bool(vf)
        wp, size = E.warp_from_sei(d["hor_flip"], d["ver_flip"], d["anticlockwise_rotation"], 24, 16)
        want = check(eng, src, wp, size, border=1, fill=fills(10), what=(hf, vf, rot))
        if rot == 1 << 14:
            luma = src[1].visible(0)
            luma = luma[:, ::-1] if hf else luma
            luma = luma[::-1] if vf else luma
            assert np.array_equal(want[0][:size[1], :size[0]], np.rot90(luma, 1))
    eng.close()


def test_refusals_write_nothing():
    """every OH_E_ARG and OH_E_UNSUPPORTED rule of ohevc_hip.h through the raw C call: the watched pictures' checksums stay; n == 0 is
    fine after the OhWarp was checked; then the plain call succeeds and a source listed twice is fine"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)
    sp = params(32, 16, 10, 1)
    src = [new(eng, sp, rng)[0] for _ in range(2)]
    dst = [new(eng, params(32, 32, 10, 1), rng)[0] for _ in range(2)]
    other_s, other_d = new(eng, params(32, 16, 10, 3), rng)[0], new(eng, params(32, 24, 10, 1), rng)[0]
    deep = [new(eng, params(32, 32, 8, 1), rng)[0] for _ in range(2)]
    full = [new(eng, params(32, 32, 10, 3), rng)[0] for _ in range(2)]
    same = [new(eng, sp, rng)[0] for _ in range(2)]                           # the sources' params: room for the image
    watched = dst + [other_d] + deep + full + src + same
    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    before = [eng.pics_hash([pid], 2) for pid in watched]
    keep = []

    def ids(v):
        a = (C.c_int * max(len(v), 1))(*v)
        keep.append(a)
        return a

    def call(s=src, d=dst, n=None, m=WM.IDENTITY, size=(32, 16), mode=0, filt=1, border=0, fill=(0, 0, 0), win=WHOLE, w_null=False, e_null=False):
        wp = E.OhWarp(mode, filt, border, (C.c_uint16 * 3)(*fill), E.OhWindow(*win), size[0], size[1], (C.c_int64 * 9)(*m))
        return L.oh_pics_warp(None if e_null else eng.h, ids(s) if s is not None else None, ids(d) if d is not None else None,
                              len(s or d or []) if n is None else n, None if w_null else C.byref(wp))

    def with_m(k, v):
        m = list(WM.IDENTITY)
        m[k] = v
        return m

    assert call(e_null=True) == arg and call(w_null=True) == arg and call(s=None, n=2) == arg and call(d=None, n=2) == arg and call(n=-1) == arg
    assert call(s=[src[0], 999]) == arg and call(d=[dst[0], 999]) == arg and call(s=[-1, src[1]]) == arg      # unknown pictures
    assert call(s=[src[0], other_s]) == arg and call(d=[dst[0], other_d]) == arg                             # params differ among themselves
    assert call(d=[dst[0], dst[0]]) == arg                                                                   # a destination twice
    assert call(s=[src[0], same[0]], d=same) == arg and call(d=src) == arg                                   # source and destination
    for win in ((32, 0, 0, 0), (16, 16, 0, 0), (0, 0, 8, 8), (-2, 0, 0, 0), (1, 1, 0, 0), (0, 0, 1, 1)):
        assert call(win=win) == arg, win                                                                     # empty, negative or odd windows
    for size in ((0, 16), (32, 0), (-2, 16), (34, 16), (32, 34), (31, 16), (32, 15), (40, 16)):
        assert call(size=size) == arg, size                                                                  # the image
    for kw in (dict(mode=2), dict(mode=-1), dict(filt=3), dict(filt=-1), dict(border=2), dict(border=-1)):
        assert call(**kw) == arg and call(s=[], d=[], n=0, **kw) == arg, kw                                  # also with nothing to do
    assert call(border=1, fill=(1024, 0, 0)) == arg and call(border=1, fill=(0, 0, 1024)) == arg             # a fill above 10 bit
    for k, v in ((0, (1 << 22) + 1), (1, -(1 << 22) - 1), (3, (1 << 22) + 1), (4, -(1 << 22) - 1), (2, (1 << 36) + 1), (5, -(1 << 36) - 1)):
        assert call(m=with_m(k, v)) == arg and call(m=with_m(k, v), mode=1) == arg, k
    for k, v in ((6, (1 << 26) + 1), (7, -(1 << 26) - 1), (8, 0), (8, -5), (8, (1 << 36) + 1)):
        assert call(m=with_m(k, v), mode=1) == arg, k
    assert call(m=with_m(6, -(ONE30 - (1 << 20) + 31) // 31), mode=1) == arg                                 # the denominator at corner (31, 0)
    assert call(m=with_m(7, -(ONE30 - (1 << 20) + 31) // 31), mode=1, size=(32, 32)) == arg                  # at corner (0, 31)
    assert call(d=deep) == uns and call(d=full) == uns                                                       # another depth, another format
    assert "oh_pics_reformat" in L.oh_engine_last_error(eng.h).decode()
    eng.sync()
    assert [eng.pics_hash([pid], 2) for pid in watched] == before, "a refused call wrote into a picture"
    assert call(s=[], d=[], n=0) == 0 and call(s=None, d=None, n=0) == 0
    for k, v in ((6, (1 << 26) + 1), (8, 0)):
        assert call(m=with_m(k, v), mode=0) == 0, k                                                          # the affine mode ignores m[6 .. 8]
    assert call(border=0, fill=(4096, 0, 0)) == 0                                                            # the fill is read with OH_WARP_CONSTANT only
    assert call(s=[src[0], src[0]]) == 0                                                                     # a source twice is fine
    eng.sync()
    after = [eng.pics_hash([pid], 2) for pid in watched]
    assert [i for i in range(len(watched)) if after[i] != before[i]] == [0, 1]
    eng.close()
