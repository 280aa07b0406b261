"""-m gpu: oh_pics_lut / Engine.pics_lut on the MI355X against the numpy model of tests/levels_model.py, every coded plane of every
destination bit for bit: the chroma formats and bit depths with a random table per plane at 72 x 40 and 136 x 72 (picture sizes are
multiples of 8; these have plane rows that are no whole units of 16 samples and more row groups than one), five pairs of depths, the
plane masks, tables with fixed ends and the inverted ramp, lut_identity beside oh_pics_reformat, range conversion there and back,
more than one launch, the round trip through oh_pics_histogram and lut_equalise, untouched sources, and the argument rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import levels_model as LM                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = [(8, 1), (10, 1), (10, 2), (12, 3), (8, 0)]
SIZES = [(72, 40), (136, 72)]
DEPTH_PAIRS = [(8, 8), (8, 10), (10, 8), (12, 12), (10, 12)]


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def shapes(p):
    return [F.plane_dims(p, c)[::-1] for c in range(F.n_planes(p))]


def planes_of(kind, p, rng):
    third = (1 << p.bit_depth) // 3
    return [LM.content(kind, s, p.bit_depth, rng, start=c * third) for c, s in enumerate(shapes(p))]


def put(eng, p, planes):
    hp = F.HostPic(p)
    for c, pl in enumerate(planes):
        hp.visible(c)[...] = pl
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid


def with_depth(p, bd):
    dp = F.OhPicParams.from_buffer_copy(p)
    dp.bit_depth = bd
    return dp


def verify(eng, pid, dp, want, what=None):
    got = eng.pic_download(pid, dp)
    assert len(want) == F.n_planes(dp)
    for c in range(F.n_planes(dp)):
        assert got.visible(c).dtype == want[c].dtype
        assert np.array_equal(got.visible(c), want[c]), (what, c, np.argwhere(got.visible(c) != want[c])[:4])


def random_tables(sbd, dbd, rng):
    return [rng.integers(0, 1 << dbd, 1 << sbd).astype(np.uint16) for _ in range(3)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("bd,cf", FORMATS, ids=[f"{bd}bit_cf{cf}" for bd, cf in FORMATS])
def test_formats_random_tables(bd, cf, w, h):
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(bd + cf + w)
    eng = Engine(0)
    p = params(w, h, bd, cf)
    tabs = random_tables(bd, bd, rng)
    pics = [planes_of(k, p, rng) for k in ("random", "ramp", "top")]
    ids = [put(eng, p, pl) for pl in pics]
    out = eng.pics_lut(ids, tabs)
    assert len(out) == 3 and not set(out) & set(ids)
    for pl, d in zip(pics, out):
        verify(eng, d, p, LM.apply(pl, tabs, 7, bd), (bd, cf))
        assert eng.pic_final_half(d) == 0
    one = eng.pics_lut(ids[:1], tabs[1])                                    # one table for every plane
    verify(eng, one[0], p, LM.apply(pics[0], [tabs[1]] * 3, 7, bd), "one table")
    eng.close()


@pytest.mark.parametrize("sbd,dbd", DEPTH_PAIRS, ids=[f"{a}to{b}" for a, b in DEPTH_PAIRS])
def test_depth_pairs_ends_and_inversion(sbd, dbd):
    """random tables across a pair of depths; a table that holds 0 at index 0 and the destination's maximum at the last index; the
    inverted ramp of lut_linear; and lut_identity, which is oh_pics_reformat with rounding"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(sbd * 16 + dbd)
    eng = Engine(0)
    Ms, Md = (1 << sbd) - 1, (1 << dbd) - 1
    for cf, (w, h) in ((1, (72, 40)), (3, (24, 16))):
        sp = params(w, h, sbd, cf)
        dp = with_depth(sp, dbd)
        pics = [planes_of(k, sp, rng) for k in ("random", "ramp")]
        ids = [put(eng, sp, pl) for pl in pics]
        tabs = random_tables(sbd, dbd, rng)
        ends = [t.copy() for t in tabs]
        for t in ends:
            t[0], t[Ms] = 0, Md
        inverted = E.lut_linear(sbd, dbd, -65536 * (Md + 1) // (Ms + 1), 0, Md)
        assert inverted[0] == Md and np.all(np.diff(inverted.astype(np.int64)) <= 0)
        for what, tt in (("random", tabs), ("ends", ends), ("inverted", [inverted] * 3)):
            out = eng.pics_lut(ids, tt, bit_depth=dbd)
            for pl, d in zip(pics, out):
                verify(eng, d, dp, LM.apply(pl, tt, 7, dbd), (what, cf))
                eng.pic_free(d)
        ident = E.lut_identity(sbd, dbd)
        a, b = eng.pics_lut(ids, ident, bit_depth=dbd), eng.pics_reformat(ids, bit_depth=dbd, depth="round")
        for x, y, pl in zip(a, b, pics):
            verify(eng, x, dp, LM.apply(pl, [ident] * 3, 7, dbd), "identity")
            got = eng.pic_download(y, dp)
            verify(eng, x, dp, [got.visible(c) for c in range(3)], "reformat")
        for c in eng.pics_compare(a, b, ssim=False):
            assert all(c.plane[k].differing == 0 and c.plane[k].samples for k in range(3))
    eng.close()


@pytest.mark.parametrize("mask", (1, 6, 7, 0, 2))
def test_plane_masks(mask):
    """an unselected plane equals the source; with every table given, and with None for the planes that are copied"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(mask)
    eng = Engine(0)
    for bd, cf in ((10, 1), (8, 3)):
        p = params(72, 40, bd, cf)
        pl = planes_of("random", p, rng)
        pid = put(eng, p, pl)
        tabs = random_tables(bd, bd, rng)
        want = LM.apply(pl, tabs, mask, bd)
        for c in range(3):
            assert np.array_equal(want[c], pl[c]) == (not mask >> c & 1)
        verify(eng, eng.pics_lut([pid], tabs, planes=mask)[0], p, want, ("mask", mask))
        verify(eng, eng.pics_lut([pid], [t if mask >> c & 1 else None for c, t in enumerate(tabs)])[0], p, want, ("None", mask))
    g = params(72, 40, 8, 0)                                                # 4:0:0: bits 1 and 2 and their tables are ignored
    pl = planes_of("random", g, rng)
    t = random_tables(8, 8, rng)[0]
    verify(eng, eng.pics_lut([put(eng, g, pl)], [t, None, None], planes=mask)[0], g, LM.apply(pl, [t], mask, 8), "4:0:0")
    eng.close()


def test_range_to_limited_and_back():
    """full -> limited -> full with lut_range, luma and chroma tables: equal to the model's chain and to the one pass with lut_then;
    it moves a sample by at most one code (limited range has fewer codes than full range, so it cannot be the identity:
    tests/test_levels_host.py).  Limited -> full -> limited of a legal-range picture is the picture"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(16235)
    eng = Engine(0)
    for bd in (8, 10):
        k = 1 << (bd - 8)
        p = params(136, 72, bd, 1)
        lim = [E.lut_range(bd, bd, False, False)] + [E.lut_range(bd, bd, False, True)] * 2
        full = [E.lut_range(bd, bd, True, False)] + [E.lut_range(bd, bd, True, True)] * 2
        pl = planes_of("random", p, rng)
        pid = put(eng, p, pl)
        there = eng.pics_lut([pid], lim)
        back = eng.pics_lut(there, full)
        mid = LM.apply(pl, lim, 7, bd)
        verify(eng, there[0], p, mid, "to limited")
        verify(eng, back[0], p, LM.apply(mid, full, 7, bd), "and back")
        assert mid[0].min() == 16 * k and mid[0].max() == 235 * k and mid[1].min() == 16 * k and mid[1].max() <= 240 * k
        once = eng.pics_lut([pid], [E.lut_then(a, b) for a, b in zip(lim, full)])
        cmp = eng.pics_compare(back + [pid], once + back, ssim=False)
        assert all(cmp[0].plane[c].differing == 0 for c in range(3))
        assert all(cmp[1].plane[c].max_abs == 1 for c in range(3))
        legal = [rng.integers(16 * k, (235 if c == 0 else 240) * k + 1, s).astype(pl[0].dtype) for c, s in enumerate(shapes(p))]
        lid = put(eng, p, legal)
        again = eng.pics_lut(eng.pics_lut([lid], full), lim)
        verify(eng, again[0], p, legal, "limited -> full -> limited")
    eng.close()


def test_more_than_one_launch_and_sources_untouched():
    """70 pictures of 32 x 16 in one call, 10 -> 8 bit, each with its own content; the sources keep their checksums"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(70)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 6
    sp = params(32, 16, 10, 1)
    dp = with_depth(sp, 8)
    pics = [planes_of("random", sp, rng) for _ in range(n)]
    ids = [put(eng, sp, pl) for pl in pics]
    before = eng.pics_hash(ids, 2)
    tabs = random_tables(10, 8, rng)
    out = eng.pics_lut(ids, tabs, bit_depth=8)
    assert len(out) == n and len(set(out)) == n and not set(out) & set(ids)
    tabs_used = [t.copy() for t in tabs]
    for t in tabs:                                                          # the call has copied them
        t[...] = 0
    for pl, d in zip(pics, out):
        verify(eng, d, dp, LM.apply(pl, tabs_used, 7, 8), "70")
    assert eng.pics_hash(ids, 2) == before
    reuse = eng.pics_lut(ids[:2], tabs_used, out=out[:2])                    # destinations given, twice in a row
    assert reuse == out[:2]
    verify(eng, out[1], dp, LM.apply(pics[1], tabs_used, 7, 8), "reused")
    assert eng.pics_lut([], tabs_used) == [] and eng.pics_lut([], tabs_used, out=[]) == []
    eng.close()


def test_equalise_round_trip():
    """histogram -> lut_equalise -> pics_lut -> histogram: the tables and the second histograms are the model's"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(77)
    eng = Engine(0)
    for bd, cf in ((8, 1), (10, 3)):
        M = (1 << bd) - 1
        p = params(136, 72, bd, cf)
        dt = np.uint16 if bd > 8 else np.uint8
        pics = [[np.minimum(rng.geometric(8.0 / M, s) + M // 8, M).astype(dt) for s in shapes(p)] for _ in range(2)]     # skewed, dark
        ids = [put(eng, p, pl) for pl in pics]
        h = eng.pics_histogram(ids)
        mh = [LM.histogram(pl, cf) for pl in pics]
        tabs, want_tabs = [], []
        for c in range(3):                                                  # the two pictures pooled, plane by plane
            tabs.append(E.lut_equalise([x.plane[c] for x in h], bd))
            want_tabs.append(LM.lut_equalise([x[c] for x in mh], bd))
            assert np.array_equal(tabs[c], want_tabs[c]), c
        out = eng.pics_lut(ids, tabs)
        h2 = eng.pics_histogram(out)
        for pl, d, g in zip(pics, out, h2):
            want = LM.apply(pl, want_tabs, 7, bd)
            verify(eng, d, p, want, "equalised")
            w2 = LM.histogram(want, cf)
            for c in range(3):
                assert np.array_equal(g.plane[c].hist, w2[c].hist[:M + 1]) and (g.plane[c].sum, g.plane[c].sum_sq) == (w2[c].sum, w2[c].sum_sq)
        assert max(g.plane[0].max for g in h2) == M and min(g.plane[0].min for g in h2) == 0
        st = E.lut_stretch([x.plane[0] for x in h], bd, 1000, 1000)
        assert np.array_equal(st, LM.lut_stretch([x[0] for x in mh], 1000, 1000, bd))
        verify(eng, eng.pics_lut(ids[:1], [st, None, None])[0], p, LM.apply(pics[0], [st] * 3, 1, bd), "stretched luma")
    eng.close()


def test_argument_errors_write_nothing():
    """every OH_E_ARG rule of ohevc_hip.h through the raw C call: refused on the host, the pictures' checksums stay; n == 0 is fine"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)
    sp = params(32, 16, 10, 1)
    dp8 = with_depth(sp, 8)

    def some(p):
        return put(eng, p, planes_of("random", p, rng))

    src, dst, dst8 = [some(sp), some(sp)], [some(sp), some(sp)], [some(dp8), some(dp8)]
    other_s, other_d = some(params(32, 16, 10, 2)), some(params(32, 16, 9, 1))
    wide, wide2, tall, tall2 = some(params(40, 16, 10, 1)), some(params(40, 16, 10, 1)), some(params(32, 24, 10, 1)), some(params(32, 24, 10, 1))
    cf3 = [some(params(32, 16, 10, 3)), some(params(32, 16, 10, 3))]
    watched = src + dst + dst8 + [other_s, other_d, wide, wide2, tall, tall2] + cf3

    def sums():
        return [eng.pics_hash([pid], 2) for pid in watched]

    before = sums()
    keep = []
    P16 = C.POINTER(C.c_uint16)
    good10 = [np.arange(1024, dtype=np.uint16)[::-1].copy() for _ in range(3)]
    good8 = [(t >> 2).astype(np.uint16) for t in good10]

    def call(s=src, d=dst, n=None, planes=7, n_entries=1024, tabs=good10, lut_null=False, e_null=False):
        lut = E.OhLut(planes, n_entries)
        for c, t in enumerate(tabs):
            if t is not None:
                lut.table[c] = t.ctypes.data_as(P16)
        sa = (C.c_int * max(len(s), 1))(*s) if s is not None else None
        da = (C.c_int * max(len(d), 1))(*d) if d is not None else None
        keep.extend((lut, sa, da, tabs))
        return L.oh_pics_lut(None if e_null else eng.h, sa, da, len(s or d or []) if n is None else n, None if lut_null else C.byref(lut))

    arg = E.OH_E_ARG
    assert call(e_null=True) == arg and call(lut_null=True) == arg and call(s=None, n=2) == arg and call(d=None, n=2) == arg   # null arguments
    assert call(n=-1) == arg
    assert call(s=[src[0], 999]) == arg and call(d=[dst[0], 999]) == arg and call(s=[-1, src[1]]) == arg                      # unknown pictures
    assert call(s=[src[0], other_s]) == arg and call(d=[dst[0], other_d]) == arg                            # params differ among themselves
    assert call(d=[wide, wide2]) == arg and call(d=[tall, tall2]) == arg and call(d=cf3) == arg             # width, height, chroma format
    assert call(d=[dst[0], dst[0]]) == arg                                                                  # a destination twice
    assert call(d=[dst[0], src[0]]) == arg and call(d=[src[1], dst[1]]) == arg and call(d=src) == arg        # source and destination
    for planes in (-1, 8, 15, 1 << 20):
        assert call(planes=planes) == arg and call(s=[], d=[], n=0, planes=planes) == arg, planes
    for n_entries in (0, 256, 1023, 1025, 4096, -1024):
        assert call(n_entries=n_entries) == arg, n_entries
    assert call(s=dst8, d=src, n_entries=1024, tabs=good10) == arg                                          # 8-bit sources take 256 entries
    for c in range(3):
        assert call(tabs=[t if k != c else None for k, t in enumerate(good10)]) == arg, c                   # no table for a selected plane
    high = [t.copy() for t in good10]
    high[2][1023] = 1024
    assert call(tabs=high) == arg                                                                           # an entry above Md, 10 bit
    assert call(d=dst8, tabs=good10) == arg and call(d=dst8, tabs=good8[:2] + [good10[2]]) == arg           # ... and above 255
    for planes in (0, 1, 3, 5, 6):
        assert call(d=dst8, tabs=good8, planes=planes) == arg, planes                                       # a plane copied across depths
    eng.sync()
    assert sums() == before, "a refused call wrote into a picture"
    assert call(s=[], d=[], n=0) == 0 and call(s=None, d=None, n=0) == 0 and call(s=[], d=[], n=0, n_entries=5, tabs=[None] * 3) == 0    # n == 0
    eng.sync()
    assert sums() == before
    assert call(d=dst8, tabs=good8) == 0                                                                    # every rule kept
    assert call(planes=5, tabs=[good10[0], None, good10[2]]) == 0                                           # an unselected plane needs no table ...
    assert call(planes=2, tabs=[high[2], good10[1], high[2]]) == 0                                          # ... and its table is not read
    assert call(s=[src[0], src[0]], d=dst) == 0                                                             # a source twice is fine
    eng.sync()
    after = sums()
    assert after[:2] == before[:2] and all(after[i] != before[i] for i in range(2, 6)) and after[6:] == before[6:]
    with pytest.raises(E.EngineError) as ei:
        eng.pics_lut(src, good10, planes=8)
    assert ei.value.code == arg
    with pytest.raises(E.EngineError) as ei:                                # destinations made for a refused call are freed again
        eng.pics_lut(src, good10, bit_depth=8)
    assert ei.value.code == arg
    with pytest.raises(ValueError):
        eng.pics_lut(src, [good10[0], good8[1][:256]])
    eng.close()
