"""-m gpu: oh_pics_orient / Engine.pics_orient on the MI355X against the numpy model of tests/orient_model.py, every coded plane of every
destination bit for bit: all orientations at every chroma format and two bit depths with and without a window, the smallest image, the
seam of the transposing kernel's tiles, larger destinations, round trips, batches of more than one launch, the finished halves, the call
next to oh_pics_convert and oh_pics_compare, from the SEI's bytes to the samples, and the argument rules."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import orient_model as OM                                                   # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
WHOLE = (0, 0, 0, 0)


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def random_pic(p, rng):
    """random samples with 0 and the maximum in every plane"""
    hp = F.HostPic(p)
    top = (1 << p.bit_depth) - 1
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        v[...] = rng.integers(0, top + 1, v.shape, dtype=v.dtype)
        v[-1, -1], v[0, 0] = top, 0
    return hp


def new(eng, p, rng):
    """(id, HostPic) of an uploaded picture"""
    hp = random_pic(p, rng)
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid, hp


def coded(hp):
    return [hp.visible(c) for c in range(len(hp.planes))]


def model(hp, o, dp, window=WHOLE):
    return OM.orient(coded(hp), hp.params, window, o, dp)


def verify(eng, pid, dp, want, what=None):
    got = eng.pic_download(pid, dp)
    assert len(want) == F.n_planes(dp)
    for c in range(F.n_planes(dp)):
        assert np.array_equal(got.visible(c), want[c]), (what, c, np.argwhere(got.visible(c) != want[c])[:4])


def image_size(p, o, window=WHOLE):
    w, h = p.width - window[0] - window[1], p.height - window[2] - window[3]
    return (h, w) if o & 4 else (w, h)


def check_fresh(eng, src, o, window=WHOLE, what=None):
    """one call on (id, HostPic) into pictures the call allocates, against the model; returns the destination's id"""
    pid, hp = src
    sp = hp.params
    ids, win = eng.pics_orient([pid], o, window=window)
    iw, ih = image_size(sp, o, window)
    dp = eng._pic_params(ids[0])
    assert (dp.width, dp.height) == (-(-iw // 8) * 8, -(-ih // 8) * 8) and (dp.bit_depth, dp.chroma_format_idc) == (sp.bit_depth, sp.chroma_format_idc)
    assert win == (0, dp.width - iw, 0, dp.height - ih)
    verify(eng, ids[0], dp, model(hp, o, dp, window), what)
    assert eng.pic_final_half(ids[0]) == 0
    return ids[0]


SIZES = [(16, 8), (24, 16)]
# (left, right, top, bottom): source and destination granules unaligned to each other, 4:2:0 chroma offsets odd.  16 x 8 has no room for a
# bottom of 6 behind a top of 2 (that window is empty: test_errors_write_nothing), so it keeps the offsets and gives up rows at the bottom
WINDOWS = {(16, 8): (2, 4, 2, 2), (24, 16): (2, 4, 2, 6)}


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("bd", (8, 10))
def test_all_orientations(bd, w, h):
    """8 orientations x chroma formats 0, 1, 3 (and 2 for orientations 0 .. 3) with the whole picture and with a window: 24 u8 samples are
    a row and a half of granules"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(bd * 100 + w)
    eng = Engine(0)
    for cf in range(4):
        src = new(eng, params(w, h, bd, cf), rng)
        for o, window in itertools.product(range(4 if cf == 2 else 8), (WHOLE, WINDOWS[(w, h)])):
            pid = check_fresh(eng, src, o, window, what=(cf, o, window))
            eng.pic_free(pid)
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_smallest_image(bd):
    """2 x 2 luma (1 x 1 chroma at 4:2:0) out of a 16 x 16 picture into 8 x 8 destinations: everything but one sample per chroma plane is
    replication"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(22 + bd)
    eng = Engine(0)
    window = (6, 8, 4, 10)
    for cf in (1, 3, 0):
        src = new(eng, params(16, 16, bd, cf), rng)
        for o in range(8):
            pid = check_fresh(eng, src, o, window, what=(cf, o))
            dp = eng._pic_params(pid)
            assert (dp.width, dp.height) == (8, 8)
            if cf == 1:
                got = eng.pic_download(pid, dp)
                assert all(len(np.unique(got.visible(c))) == 1 for c in (1, 2))
            eng.pic_free(pid)
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_tile_seam(bd):
    """partial tiles on both axes and unequal counts of tiles per axis, in luma and in chroma, orientations 4 .. 7 and 1.  The 4:2:0
    picture of (ORIENT_TILE + 8) x (ORIENT_TILE + 24) passes the tile edge in luma only and has as many tiles across as down, so a
    picture of twice (ORIENT_TILE + 8) x twice (2 ORIENT_TILE + 24) runs beside it, whose chroma planes pass the edge as well"""
    from openhevc_amd.engine import Engine
    T = E.ORIENT_TILE
    rng = np.random.default_rng(64 + bd)
    eng = Engine(0)
    small, big = params(T + 8, T + 24, bd, 1), params(2 * (T + 8), 2 * (2 * T + 24), bd, 1)
    assert small.width > T and small.height > T and small.width % T and small.height % T
    for c in (0, 1):
        pw, ph = F.plane_dims(big, c)
        assert pw > T and ph > T and pw % T and ph % T and -(-pw // T) != -(-ph // T), c
    for p in (small, big):
        src = new(eng, p, rng)
        for o in (4, 5, 6, 7, 1):
            eng.pic_free(check_fresh(eng, src, o, what=(p.width, o)))
        eng.pic_free(check_fresh(eng, src, 6, (2, 4, 2, 6), what=(p.width, "window")))
    eng.close()


def test_larger_destinations():
    """a 16 x 8 image transposed into 32 x 24 destinations: the replicated columns and rows"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(3224)
    eng = Engine(0)
    for bd, cf in ((8, 1), (10, 3)):
        src = new(eng, params(16, 8, bd, cf), rng)
        dp = params(32, 24, bd, cf)
        dst = eng.pic_alloc(dp)
        for o in (4, 5, 6, 7, 0, 3):
            ids, win = eng.pics_orient([src[0]], o, out=[dst])
            iw, ih = image_size(src[1].params, o)
            assert ids == [dst] and win == (0, 32 - iw, 0, 24 - ih)
            want = model(src[1], o, dp)
            verify(eng, dst, dp, want, (bd, cf, o))
            assert np.array_equal(want[0][:, iw:], np.repeat(want[0][:, iw - 1:iw], 32 - iw, axis=1))
            assert np.array_equal(want[0][ih:], np.repeat(want[0][ih - 1:ih], 24 - ih, axis=0))
    eng.close()


def test_round_trips():
    """a then orient_inverse(a) gives the source's checksum; a then b equals one call with orient_then(a, b): all pairs, 24 x 16 4:4:4"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(2416)
    eng = Engine(0)
    p = params(24, 16, 8, 3)
    pid, hp = new(eng, p, rng)
    want = eng.pics_hash([pid], 2)[0]
    first = {a: eng.pics_orient([pid], a) for a in range(8)}
    for a in range(8):
        ids, win = first[a]
        back, bwin = eng.pics_orient(ids, E.orient_inverse(a), window=win)
        assert bwin == WHOLE and eng.pics_hash(back, 2)[0] == want, a
        eng.pic_free(back[0])
    for a, b in itertools.product(range(8), range(8)):
        ids, win = first[a]
        two, win2 = eng.pics_orient(ids, b, window=win)
        one, win1 = eng.pics_orient([pid], E.orient_then(a, b))
        assert win1 == win2 and eng.pics_hash(two, 2) == eng.pics_hash(one, 2), (a, b)
        eng.pic_free(two[0])
        eng.pic_free(one[0])
    eng.close()


def test_more_than_one_launch():
    """CONV_MAX_PICS + 1 pictures of 16 x 8 in one call, each with its own content, a quarter turn clockwise"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(65)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 1
    sp = params(16, 8, 10, 1)
    srcs = [new(eng, sp, rng) for _ in range(n)]
    ids, win = eng.pics_orient([s[0] for s in srcs], "rot90")
    assert len(ids) == n and len(set(ids)) == n and not set(ids) & {s[0] for s in srcs} and win == (0, 0, 0, 0)
    dp = eng._pic_params(ids[0])
    assert (dp.width, dp.height) == (8, 16)
    for (_, hp), d in zip(srcs, ids):
        verify(eng, d, dp, model(hp, 5, dp), "batch")
        assert np.array_equal(model(hp, 5, dp)[0], np.rot90(hp.visible(0), -1))
    eng.close()


def test_state_and_halves():
    """a source whose finished half is half 1 is read there; a destination that oh_pic_wrap made, and one whose finished half was 1:
    half 0 is written and becomes the finished one; two calls back to back into the same destinations leave the second"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(12)
    eng = Engine(0)
    sp, dp = params(64, 32, 10, 1), params(32, 64, 10, 1)
    a, b = new(eng, sp, rng), random_pic(sp, rng)
    half = eng.L.oh_pic_bytes(C.byref(sp)) // 2
    mem = torch.zeros(2 * half, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    own = eng.pic_wrap(sp, mem.data_ptr() + half, mem.data_ptr(), half)     # its half 0 is the upper block, its half 1 the lower
    eng.pic_upload(own, b)                                                  # b in the upper block
    twin = eng.pic_wrap(sp, mem.data_ptr(), mem.data_ptr() + half, half)    # the same memory: half 1 holds b, half 0 zeros
    eng.pic_set_final_half(twin, 1)
    assert eng.pic_final_half(twin) == 1
    dhalf = eng.L.oh_pic_bytes(C.byref(dp)) // 2
    dmem = torch.full((2 * dhalf,), 0x55, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    dw = eng.pic_wrap(dp, dmem.data_ptr(), dmem.data_ptr() + dhalf, dhalf)
    da = eng.pic_alloc(dp)
    eng.pic_upload(da, random_pic(dp, rng))
    eng.pic_set_final_half(da, 1)
    eng.pic_set_final_half(dw, 1)
    assert eng.pics_orient([twin, a[0]], 5, out=[dw, da])[0] == [dw, da]
    assert eng.pic_final_half(dw) == 0 and eng.pic_final_half(da) == 0
    verify(eng, dw, dp, model(b, 5, dp), "finished half 1 of the source, wrapped destination")
    verify(eng, da, dp, model(a[1], 5, dp), "allocated destination")
    assert (dmem[dhalf:] == 0x55).all()                                     # half 1 of the wrapped destination: untouched
    eng.pics_orient([a[0], twin], 6, out=[dw, da])                          # back to back, no wait between: the second call's result stays
    eng.pics_orient([twin, a[0]], 7, out=[dw, da])
    verify(eng, dw, dp, model(b, 7, dp), "second call")
    verify(eng, da, dp, model(a[1], 7, dp), "second call")
    assert eng.pic_final_half(dw) == 0 and eng.pic_final_half(da) == 0
    eng.close()


def test_next_to_convert_and_compare():
    """4:4:4: planar RGB of the oriented picture is torch.rot90 / flip of the RGB of the source; a picture against its hflip of hflip
    has no differing sample"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(444)
    eng = Engine(0)
    p = params(24, 16, 8, 3)
    pid, hp = new(eng, p, rng)
    rgb = eng.pics_convert([pid], "rgb_planar")
    turned = {1: lambda t: torch.flip(t, (3,)), 2: lambda t: torch.flip(t, (2,)), 3: lambda t: torch.rot90(t, 2, (2, 3)),
              4: lambda t: t.transpose(2, 3), 5: lambda t: torch.rot90(t, -1, (2, 3)), 6: lambda t: torch.rot90(t, 1, (2, 3)),
              7: lambda t: torch.rot90(t, 2, (2, 3)).transpose(2, 3)}
    for o, f in turned.items():
        ids, win = eng.pics_orient([pid], o)
        got = eng.pics_convert(ids, "rgb_planar", window=win)
        assert got.shape == f(rgb).shape and torch.equal(got, f(rgb).contiguous()), o
        eng.pic_free(ids[0])
    for p2 in (params(24, 16, 10, 1), p):
        pid2, _ = new(eng, p2, rng)
        once, _ = eng.pics_orient([pid2], "hflip")
        twice, _ = eng.pics_orient(once, "hflip")
        cmp = eng.pics_compare([pid2], twice, ssim=False)[0]
        assert [cmp.plane[c].differing for c in range(3)] == [0, 0, 0]
        cmp = eng.pics_compare([pid2], once, ssim=False)[0]
        assert cmp.plane[0].differing > 0
    eng.close()


def test_from_the_sei_to_the_samples():
    """message bytes -> annexb.display_orientation -> orientation_from_sei -> pics_orient, against numpy's flips and rot90"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(47)
    eng = Engine(0)
    pid, hp = new(eng, params(24, 16, 10, 3), rng)
    for hf, vf, k in itertools.product((0, 1), (0, 1), range(4)):
        bits = (hf << 22) | (vf << 21) | ((k << 14) << 5) | (1 << 4) | 0x8
        nal = bytes([39 << 1, 1, 47, 3]) + bits.to_bytes(3, "big") + b"\x80"
        d = A.display_orientation(nal)
        assert d == dict(cancel=False, hor_flip=bool(hf), ver_flip=bool(vf), anticlockwise_rotation=k << 14, persistence=True)
        o = E.orientation_from_sei(d["hor_flip"], d["ver_flip"], d["anticlockwise_rotation"])
        ids, win = eng.pics_orient([pid], o)
        dp = eng._pic_params(ids[0])
        got = eng.pic_download_window(ids[0], dp, *win)
        for c in range(3):
            want = hp.visible(c)
            if hf:
                want = want[:, ::-1]
            if vf:
                want = want[::-1]
            assert np.array_equal(got[c], np.rot90(want, k)), (hf, vf, k, c)
        eng.pic_free(ids[0])
    eng.close()


def test_errors_write_nothing():
    """every OH_E_ARG and OH_E_UNSUPPORTED rule of ohevc_hip.h through the raw C call: refused on the host, the watched pictures'
    checksums stay; n == 0 is fine; then every orientation succeeds, and a source listed twice is fine"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)
    sp = params(32, 16, 10, 1)
    src = [new(eng, sp, rng)[0] for _ in range(2)]
    dst = [new(eng, params(32, 32, 10, 1), rng)[0] for _ in range(2)]       # holds the image of every orientation
    flat = [new(eng, sp, rng)[0] for _ in range(2)]                         # 32 x 16: too low for a transposed 32 x 16
    narrow = [new(eng, params(24, 32, 10, 1), rng)[0] for _ in range(2)]    # too narrow for orientations 0 .. 3
    other_s, other_d = new(eng, params(32, 16, 10, 3), rng)[0], new(eng, params(32, 24, 10, 1), rng)[0]
    deep = [new(eng, params(32, 32, 8, 1), rng)[0] for _ in range(2)]       # another bit depth
    full = [new(eng, params(32, 32, 10, 3), rng)[0] for _ in range(2)]      # another chroma format
    s422 = [new(eng, params(32, 16, 10, 2), rng)[0] for _ in range(2)]
    d422 = [new(eng, params(32, 32, 10, 2), rng)[0] for _ in range(2)]
    small = new(eng, params(16, 8, 10, 1), rng)[0]
    watched = dst + flat + narrow + [other_d] + deep + full + d422 + src + s422
    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED

    def sums():
        return [eng.pics_hash([pid], 2) for pid in watched]

    before = sums()
    keep = []

    def ids(v):
        a = (C.c_int * max(len(v), 1))(*v)
        keep.append(a)
        return a

    def call(s=src, d=dst, n=None, o=0, win=WHOLE, o_null=False, e_null=False):
        od = E.OhOrient(o, E.OhWindow(*win))
        return L.oh_pics_orient(None if e_null else eng.h, ids(s) if s is not None else None, ids(d) if d is not None else None,
                                len(s or d or []) if n is None else n, None if o_null else C.byref(od))

    assert call(e_null=True) == arg and call(o_null=True) == arg and call(s=None, n=2) == arg and call(d=None, n=2) == arg   # null arguments
    assert call(n=-1) == arg
    assert call(s=[src[0], 999]) == arg and call(d=[dst[0], 999]) == arg and call(s=[-1, src[1]]) == arg     # unknown pictures
    assert call(s=[src[0], other_s]) == arg and call(d=[dst[0], other_d]) == arg                            # params differ among themselves
    assert call(d=[dst[0], dst[0]]) == arg                                                                  # a destination twice
    assert call(d=[flat[0], src[0]]) == arg and call(d=[src[1], flat[1]]) == arg and call(d=src) == arg      # source and destination
    for o in (8, -1, 16, 1 << 20):
        assert call(o=o) == arg, o                                                                          # orientations outside 0 .. 7
        assert call(s=[], d=[], n=0, o=o) == arg, o                                                         # also with nothing to do
    for win in ((32, 0, 0, 0), (16, 16, 0, 0), (0, 0, 8, 8), (0, 0, 0, 16), (-2, 0, 0, 0), (1, 1, 0, 0), (0, 0, 1, 1), (3, 1, 0, 0), (0, 0, 2, 1)):
        assert call(win=win) == arg and call(win=win, o=5) == arg, win                                      # empty, negative or odd windows
    assert call(s=[small], d=[dst[0]], win=(2, 4, 2, 6)) == arg                                             # 16 x 8: nothing left of the rows
    for o in range(4, 8):
        assert call(d=flat, o=o) == arg, o                                                                  # the image is taller than the destinations
    for o in range(4):
        assert call(d=narrow, o=o) == arg, o                                                                # wider
        assert call(d=narrow, o=o, win=(0, 6, 0, 0)) == arg, o                                              # still two samples too wide
    for o in range(8):
        assert call(d=deep, o=o) == uns and call(d=full, o=o) == uns, o                                     # another depth, another format
    assert "oh_pics_reformat" in eng.L.oh_engine_last_error(eng.h).decode()
    for o in range(4, 8):
        assert call(s=s422, d=d422, o=o) == uns, o                                                          # 4:2:2 transposed
        assert "4:2:0 or 4:4:4" in eng.L.oh_engine_last_error(eng.h).decode()
    eng.sync()
    assert sums() == before, "a refused call wrote into a picture"
    assert call(s=[], d=[], n=0) == 0 and call(s=None, d=None, n=0) == 0 and call(s=[], d=[], n=0, o=7) == 0     # n == 0
    eng.sync()
    assert sums() == before
    for o in range(8):                                                                                      # every orientation inside the list
        assert call(o=o) == 0, o
    for o in range(4):
        assert call(s=s422, d=d422, o=o) == 0, o                                                            # 4:2:2 without a transposition
        assert call(d=narrow, o=o, win=(0, 8, 0, 0)) == 0, o                                                # the window that fits
    assert call(s=[src[0], src[0]], d=flat) == 0                                                            # a source twice is fine
    eng.sync()
    after = sums()
    changed = [i for i in range(len(watched)) if after[i] != before[i]]
    assert changed == [watched.index(p) for p in dst + flat + narrow + d422]
    eng.close()
