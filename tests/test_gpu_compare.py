"""-m gpu: oh_pics_compare / Engine.pics_compare on the MI355X against the numpy model of tests/compare_model.py, every field of every
plane bit for bit (the SSIM sum included: no tolerance anywhere): chroma formats, bit depths, windows and leftover columns and rows,
the kernel's tile boundaries, calls of more than one launch, repeated calls, pictures that oh_pics_resize made, and the argument
rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compare_model as CM                                                  # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

Q = 1 << 30


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def random_pic(p, rng):
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        v[...] = rng.integers(0, 1 << p.bit_depth, v.shape, dtype=v.dtype)
    return hp


def filled(p, fn):
    """a picture whose plane c is fn(c, shape), an integer array"""
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        v[...] = fn(c, v.shape)
    return hp


def up(eng, p, hp):
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid


def coded(hp, p):
    return [hp.visible(c) for c in range(F.n_planes(p))]


def same(got, want):
    """every field of the three PlaneDiff of a Compare against the model's dicts"""
    return all(getattr(got.plane[c], k) == want[c][k] for c in range(3) for k in CM.FIELDS)


def check(eng, p, pairs, **kw):
    """pairs: [((id a, HostPic a), (id b, HostPic b))] in one call against the model; returns the Compare list"""
    got = eng.pics_compare([a[0] for a, _ in pairs], [b[0] for _, b in pairs], **kw)
    assert len(got) == len(pairs)
    for i, (a, b) in enumerate(pairs):
        want = CM.compare(coded(a[1], p), coded(b[1], p), p, kw.get("window", (0, 0, 0, 0)), kw.get("ssim", True))
        assert same(got[i], want), (i, kw, got[i], want)
    return got


FORMATS = [(8, 1), (10, 1), (10, 2), (12, 3), (8, 0)]                       # bit depth, chroma_format_idc


@pytest.mark.parametrize("bd,cf", FORMATS, ids=[f"{b}b_cf{c}" for b, c in FORMATS])
def test_formats_equal_the_model(bd, cf):
    """96 x 40, five pairs in one call: random against random, a picture against itself (the same id twice), against a copy with +-1
    noise, all-zero against all-maximum, a ramp against its reverse; with and without SSIM"""
    from openhevc_amd.engine import Engine
    p = params(96, 40, bd, cf)
    top = (1 << bd) - 1
    rng = np.random.default_rng(bd * 7 + cf)
    eng = Engine(0)
    r0, r1 = random_pic(p, rng), random_pic(p, rng)
    noisy = filled(p, lambda c, s: np.clip(r0.visible(c).astype(np.int64) + rng.integers(-1, 2, s), 0, top))
    zero, full = filled(p, lambda c, s: 0), filled(p, lambda c, s: top)
    ramp = filled(p, lambda c, s: (np.arange(s[0] * s[1]) % (top + 1)).reshape(s))
    rev = filled(p, lambda c, s: (np.arange(s[0] * s[1])[::-1] % (top + 1)).reshape(s))
    pics = [(up(eng, p, hp), hp) for hp in (r0, r1, noisy, zero, full, ramp, rev)]
    pairs = [(pics[0], pics[1]), (pics[0], pics[0]), (pics[0], pics[2]), (pics[3], pics[4]), (pics[5], pics[6])]
    got = check(eng, p, pairs)
    bare = check(eng, p, pairs, ssim=False)
    n_pl = F.n_planes(p)
    for i in range(len(pairs)):
        for c in range(3):
            g, b = got[i].plane[c], bare[i].plane[c]
            assert b.ssim_windows == 0 and b.ssim_sum == 0 and b.ssim is None
            assert all(getattr(g, k) == getattr(b, k) for k in ("samples", "differing", "sad", "sse", "max_abs", "first"))
            if c >= n_pl:                                                   # 4:0:0: the planes the picture lacks
                assert all(getattr(g, k) == CM.ABSENT[k] for k in CM.FIELDS)
    for c in range(n_pl):
        g = got[1].plane[c]                                                 # identical
        assert g.sse == g.sad == g.differing == g.max_abs == 0 and g.first is None
        assert g.ssim_windows > 0 and g.ssim_sum == g.ssim_windows << 30 and g.ssim == 1.0 and g.psnr == float("inf")
        g = got[3].plane[c]                                                 # zero against maximum
        assert g.sse == g.samples * top * top and g.max_abs == top and g.differing == g.samples and g.first == (0, 0)
        assert g.psnr == 0.0 and g.mse == top * top
        assert got[2].plane[c].max_abs == 1 and got[2].plane[c].ssim_sum < got[1].plane[c].ssim_sum
    eng.close()


def test_leftovers_and_windows():
    """a 70 x 38 picture inside coded planes of 72 x 40 (coded sizes are multiples of the minimum coding block): its windows
    (2, 4, 2, 6) and (0, 66, 0, 36), the second a 4 x 2 image without an SSIM window, and the whole of it, where luma (70 x 38) and
    chroma (35 x 19) leave columns and rows over; differences in the leftovers alone; a 4:4:4 12-bit window at odd offsets"""
    from openhevc_amd.engine import Engine
    p = params(72, 40, 10, 1)
    rng = np.random.default_rng(70)
    eng = Engine(0)
    a, b = random_pic(p, rng), random_pic(p, rng)
    pa, pb = (up(eng, p, a), a), (up(eng, p, b), b)
    whole = (0, 2, 0, 2)
    for win, size in (((2, 4 + 2, 2, 6 + 2), 64 * 30), ((0, 66 + 2, 0, 36 + 2), 4 * 2), (whole, 70 * 38)):
        got = check(eng, p, [(pa, pb), (pb, pb)], window=win)
        assert got[0].plane[0].samples == size and got[0].plane[1].samples == size // 4
        check(eng, p, [(pa, pb)], window=win, ssim=False)
    small = eng.pics_compare([pa[0]], [pb[0]], window=(0, 68, 0, 38))[0]
    assert [small.plane[c].ssim_windows for c in range(3)] == [0, 0, 0] and small.plane[0].ssim is None
    # b2 = a but for samples in the columns and rows that the 4 x 4 blocks of the whole-picture window leave over
    b2 = a.copy()
    for c, spots in ((0, ((69, 5), (3, 37))), (1, ((34, 2), (1, 18))), (2, ((32, 16),))):
        for x, y in spots:
            b2.visible(c)[y, x] ^= 1
    got = check(eng, p, [(pa, (up(eng, p, b2), b2))], window=whole)[0]
    assert [got.plane[c].first for c in range(3)] == [(69, 5), (34, 2), (32, 16)]
    assert [got.plane[c].sse for c in range(3)] == [2, 2, 1]
    assert [(got.plane[c].ssim_windows, got.plane[c].ssim_sum) for c in range(3)] == [(128, 128 << 30), (21, 21 << 30), (21, 21 << 30)]
    eng.close()
    p = params(72, 40, 12, 3)                                               # 4:4:4: odd offsets are aligned
    eng = Engine(0)
    a, b = random_pic(p, np.random.default_rng(71)), random_pic(p, np.random.default_rng(72))
    pa, pb = (up(eng, p, a), a), (up(eng, p, b), b)
    for win in ((1, 2, 3, 2), (3, 0, 1, 0), (1, 3, 3, 1)):                  # 69 x 35, 69 x 39, 68 x 36
        check(eng, p, [(pa, pb), (pa, pa)], window=win)
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_tile_boundaries(bd):
    """three tile columns and a remainder, three tile rows and a remainder, in every plane (4:4:4): two equal pictures but for one
    sample, at the four corners of an interior tile and at the last sample of the window; then several differing samples"""
    from openhevc_amd.engine import Engine
    TW, TH = E.CMP_TW, E.CMP_TH
    w, h = 3 * TW + 40, 3 * TH + 8
    p = params(w, h, bd, 3)
    rng = np.random.default_rng(bd)
    eng = Engine(0)
    a = random_pic(p, rng)
    pa = (up(eng, p, a), a)
    spots = [(TW, TH), (2 * TW - 1, TH), (TW, 2 * TH - 1), (2 * TW - 1, 2 * TH - 1), (w - 1, h - 1)]
    pairs = []
    for x, y in spots:
        b = a.copy()
        for c in range(3):
            b.visible(c)[y, x] ^= 1 << c
        pairs.append((pa, (up(eng, p, b), b)))
    got = check(eng, p, pairs)
    for (x, y), g, (_, (_, b)) in zip(spots, got, pairs):
        for c in range(3):
            d = g.plane[c]
            assert d.differing == 1 and d.first == (x, y) and d.max_abs == 1 << c and d.sse == 1 << 2 * c
            q = CM.window_values(a.visible(c), b.visible(c), bd)
            covering = (1 + (4 <= x < w - 4)) * (1 + (4 <= y < h - 4))      # the 8 x 8 windows at stride 4 over (x, y)
            assert int((q != Q).sum()) == covering and covering in (1, 2, 4)
            assert d.ssim_sum == int(q.sum()) < d.ssim_windows << 30
    # several samples, the raster-first of them in another tile than the rest, another one in every plane
    b = a.copy()
    firsts = [(2 * TW + 7, 3), (TW - 1, TH + 1), (w - 1, 0)]
    for c in range(3):
        for x, y in [firsts[c], (5, firsts[c][1] + 1), (TW, 2 * TH), (w - 2, h - 1), (0, h - 1)]:
            b.visible(c)[y, x] ^= 3
    pb = (up(eng, p, b), b)
    g = check(eng, p, [(pa, pb)])[0]
    assert [g.plane[c].first for c in range(3)] == firsts and all(g.plane[c].differing == 5 for c in range(3))
    g = check(eng, p, [(pa, pb)], window=(2, 0, 1, 0), ssim=False)[0]       # the samples the window keeps, keyed in its coordinates
    assert [g.plane[c].first for c in range(3)] == [(x - 2, y - 1) if y else (5 - 2, 0) for x, y in firsts]
    eng.close()


def test_more_pairs_than_one_launch_and_no_accumulation():
    """70 different pairs of 32 x 16 — every picture the first member of one pair and the second of the next: two launches; the same
    pairs in two calls; the same call again"""
    from openhevc_amd.engine import Engine
    p = params(32, 16, 10, 1)
    rng = np.random.default_rng(70)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 6
    pics = []
    for _ in range(n):
        hp = random_pic(p, rng)
        pics.append((up(eng, p, hp), hp))
    pairs = [(pics[i], pics[(i + 1) % n]) for i in range(n)]
    one = check(eng, p, pairs)
    ia, ib = [a[0] for a, _ in pairs], [b[0] for _, b in pairs]
    two = eng.pics_compare(ia[:33], ib[:33]) + eng.pics_compare(ia[33:], ib[33:])
    again = eng.pics_compare(ia, ib)
    for i in range(n):
        for other in (two, again):
            assert all(getattr(one[i].plane[c], k) == getattr(other[i].plane[c], k) for c in range(3) for k in CM.FIELDS), i
    assert len({x.plane[0].sse for x in one}) > 60 and len({x.plane[0].ssim_sum for x in one}) > 60      # the pairs do differ
    assert eng.pics_compare([], []) == []
    eng.close()


def test_with_the_other_picture_services():
    """a rendition against its source: 200 x 136 resized to 100 x 68 and back with oh_pics_resize, compared with the original, equals
    the model on the downloaded pictures; a 1:1 resize is an identical picture"""
    from openhevc_amd.engine import Engine
    p = params(200, 136, 10, 1)
    eng = Engine(0)
    src = random_pic(p, np.random.default_rng(5))
    # low-pass content: noise alone has nothing a half-size rendition keeps
    for c in range(3):
        v = src.visible(c)
        yy, xx = np.mgrid[0:v.shape[0], 0:v.shape[1]]
        v[...] = np.clip(512 + 300 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0) + (v.astype(np.int64) - 512) // 16, 0, 1023)
    pid = up(eng, p, src)
    small, swin = eng.pics_resize([pid], (100, 68))
    back, bwin = eng.pics_resize(small, (200, 136), window=swin)
    assert bwin == (0, 0, 0, 0)
    got = eng.pics_compare([pid], back)[0]
    hb = eng.pic_download(back[0], p)
    want = CM.compare(coded(src, p), coded(hb, p), p)
    assert same(got, want), (got, want)
    for c in range(3):
        d = got.plane[c]
        assert d.differing > 0 and 0.0 < d.ssim < 1.0 and 20.0 < d.psnr < 100.0
    copy, cwin = eng.pics_resize([pid], (200, 136))
    got = eng.pics_compare(copy, [pid], window=cwin)[0]
    for c in range(3):
        d = got.plane[c]
        assert d.differing == d.sse == d.sad == d.max_abs == 0 and d.first is None and d.ssim_sum == d.ssim_windows << 30
    eng.close()


def test_argument_errors_leave_out_untouched():
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    p = params(64, 32, 10, 1)
    rng = np.random.default_rng(1)
    hps = [random_pic(p, rng) for _ in range(3)]
    pids = [up(eng, p, hp) for hp in hps]
    p8, pbig = params(64, 32, 8, 1), params(72, 40, 10, 1)
    other8, otherbig = up(eng, p8, random_pic(p8, rng)), up(eng, pbig, random_pic(pbig, rng))
    out = (E.OhCompare * 3)()
    C.memset(out, 0xA5, C.sizeof(out))
    guard = bytes(out)

    def ids(v):
        return (C.c_int * max(len(v), 1))(*v)

    def call(a, b, sp, out_p=out, n=None):
        return L.oh_pics_compare(eng.h, ids(a) if a is not None else None, ids(b) if b is not None else None,
                                 len(a or b or []) if n is None else n, C.byref(sp) if sp is not None else None, out_p)

    def spec(win=(0, 0, 0, 0), flags=E.CMP_SSIM):
        return E.OhCompareSpec(E.OhWindow(*win), flags)

    arg = E.OH_E_ARG
    A, B = pids[:2], pids[1:]
    assert call(A, B, None) == arg
    assert call(A, B, spec(), None) == arg
    assert call(None, B, spec()) == arg and call(A, None, spec()) == arg
    assert call([pids[0], 999], B, spec()) == arg and call(A, [999, pids[0]], spec()) == arg      # unknown picture in either list
    assert call(A, [pids[1], other8], spec()) == arg and call([other8, pids[0]], B, spec()) == arg  # 8 bit against 10 bit
    assert call([other8], [other8], spec()) == 0                                                   # (fine among themselves)
    C.memset(out, 0xA5, C.sizeof(out))
    assert call(A, [otherbig, pids[2]], spec()) == arg and call([pids[0]], [otherbig], spec()) == arg   # 64 x 32 against 72 x 40
    for win in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (32, 32, 0, 0), (0, 0, 16, 16), (0, 0, -2, 0), (64, 0, 0, 0)):
        assert call(A, B, spec(win)) == arg, win                                                   # misaligned and empty windows
    for flags in (2, 3, 4, -1, 1 << 31 - 1):
        assert call(A, B, spec(flags=flags)) == arg, flags
    assert call(A, B, spec(), n=-1) == arg
    assert bytes(out) == guard, "a refused call wrote into out"
    assert call([], [], spec()) == 0 and call(None, None, spec(), n=0) == 0 and bytes(out) == guard      # n == 0: nothing to do
    assert call(A, B, spec((2, 2, 2, 2), 0)) == 0
    for i in range(2):
        got, want = E.Compare(out[i], 10), CM.compare(coded(hps[i], p), coded(hps[i + 1], p), p, (2, 2, 2, 2), ssim=False)
        assert same(got, want), i
    assert bytes(out[2]) == guard[2 * C.sizeof(E.OhCompare):]               # two pairs, two results
    eng.close()
