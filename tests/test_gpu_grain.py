"""-m gpu: oh_pics_grain / Engine.pics_grain on the MI355X against the numpy model of tests/grain_model.py, every coded plane of every
destination bit for bit: the chroma formats and bit depths at 72 x 40 and 136 x 72 (chroma blocks cut by the right and bottom edge,
rows that are no whole granules, several rows of blocks) with an interval table per plane, three pictures of different content and
seed; planes wider than a workgroup's tile of 256 samples, whose last tile is one block or a block cut to 4 samples; one block and one edge; a table with gaps on a ramp; sigma 0; both blendings at black and white; log2_scale 0 and 15; the plane
masks; seeds; more than one launch; untouched sources; out= reuse; a message parsed from bytes; and the argument rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grain_model as GM                                                    # noqa: E402
import levels_model as LM                                                   # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = [(8, 1), (10, 1), (10, 2), (12, 3), (8, 0)]
SIZES = [(72, 40), (136, 72)]


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def shapes(p):
    return [F.plane_dims(p, c)[::-1] for c in range(F.n_planes(p))]


def planes_of(kind, p, rng):
    third = (1 << p.bit_depth) // 3
    return [LM.content(kind, s, p.bit_depth, rng, start=c * third) for c, s in enumerate(shapes(p))]


def flat(p, value):
    dt = np.uint16 if p.bit_depth > 8 else np.uint8
    return [np.full(s, value, dtype=dt) for s in shapes(p)]


def put(eng, p, planes):
    hp = F.HostPic(p)
    for c, pl in enumerate(planes):
        hp.visible(c)[...] = pl
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid


def get(eng, pid, p):
    got = eng.pic_download(pid, p)
    return [got.visible(c).copy() for c in range(F.n_planes(p))]


def verify(eng, pid, p, want, what=None):
    got = get(eng, pid, p)
    assert len(want) == len(got)
    for c in range(len(got)):
        assert got[c].dtype == want[c].dtype
        assert np.array_equal(got[c], want[c]), (what, c, np.argwhere(got[c] != want[c])[:4])


def interval_tables(rng):
    """per plane a table of a few intervals with their own sigma and cut-offs, and gaps between some"""
    t = np.zeros((3, 256), dtype=np.uint32)
    for c in range(3):
        edges = sorted(int(v) for v in rng.choice(np.arange(1, 255), 7, replace=False))
        for k, (lo, hi) in enumerate(zip([0] + edges, edges + [256])):
            if k % 4 != 3:                                                  # every fourth interval is a gap
                t[c, lo:hi] = GM.entry(int(rng.integers(1, 256)), int(rng.integers(2, 15)), int(rng.integers(2, 15)))
    return t


def model(pics, p, grain, seeds, mask=None):
    return [GM.apply(pl, p.bit_depth, grain.tables, s, grain.planes if mask is None else mask, grain.blending, grain.log2_scale)
            for pl, s in zip(pics, seeds)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("bd,cf", FORMATS, ids=[f"{bd}bit_cf{cf}" for bd, cf in FORMATS])
def test_formats_interval_tables(bd, cf, w, h):
    rng = np.random.default_rng(bd + cf + w)
    eng = E.Engine(0)
    p = params(w, h, bd, cf)
    grain = E.Grain(interval_tables(rng), 7, 0, 3)
    pics = [planes_of(k, p, rng) for k in ("random", "ramp", "top")]
    seeds = [7, 0xFFFFFFFF, 123456789]
    ids = [put(eng, p, pl) for pl in pics]
    out = eng.pics_grain(ids, grain, seeds)
    assert len(out) == 3 and not set(out) & set(ids)
    for pl, d, want in zip(pics, out, model(pics, p, grain, seeds)):
        verify(eng, d, p, want, (bd, cf))
        assert eng.pic_final_half(d) == 0
    assert any(not np.array_equal(a, b) for a, b in zip(get(eng, out[1], p), pics[1]))      # grain was added
    uni = E.make_grain(40, 3, 12, log2_scale=1)
    one = eng.pics_grain(ids[:1], uni, 5)
    verify(eng, one[0], p, model(pics[:1], p, uni, [5])[0], "uniform")
    eng.close()


WIDE = [(520, 24, 8, 1), (520, 24, 10, 2), (776, 16, 12, 3), (264, 8, 8, 0)]


@pytest.mark.parametrize("w,h,bd,cf", WIDE, ids=[f"{w}x{h}_{bd}bit_cf{cf}" for w, h, bd, cf in WIDE])
def test_planes_wider_than_a_workgroups_tile(w, h, bd, cf):
    """planes of more than one tile of GRAIN_TILE[0] = 256 samples across: a tile's outer columns are smoothed with the block of the
    next tile, whose descriptor the workgroup makes itself from that block's samples.  520 = 2 x 256 + 8 (the third tile holds one
    block); its 4:2:0 and 4:2:2 chroma planes are 260 wide: the block beside the first tile is cut to 4 samples by the right edge, and
    the 4:2:0 chroma height of 12 cuts the last row of blocks to 4 rows; 776 = 3 x 256 + 8 in all three planes.  Random content with
    an interval table, so that the blocks either side of a tile edge differ in sigma and pattern, and a ramp"""
    TW = E.GRAIN_TILE[0]
    rng = np.random.default_rng(w + bd)
    eng = E.Engine(0)
    p = params(w, h, bd, cf)
    assert all(s[1] > TW for s in shapes(p)) and any(s[1] % TW in (4, 8) for s in shapes(p))
    grain = E.Grain(interval_tables(rng), 7, 0, 1)
    # blocks of random levels with a little noise: neighbouring blocks fall into different intervals
    pics = [planes_of("random", p, rng), planes_of("ramp", p, rng)]
    M = (1 << bd) - 1
    pics.append([np.clip(np.kron(rng.integers(0, M + 1, ((s[0] + 7) // 8, (s[1] + 7) // 8)), np.ones((8, 8), dtype=np.int64))[:s[0], :s[1]] +
                         rng.integers(-3, 4, s), 0, M).astype(pl.dtype) for s, pl in zip(shapes(p), pics[0])])
    seeds = [1, 2, 3]
    ids = [put(eng, p, pl) for pl in pics]
    out = eng.pics_grain(ids, grain, seeds)
    want = model(pics, p, grain, seeds)
    for d, wp in zip(out, want):
        verify(eng, d, p, wp, (w, h, bd, cf))
    # the smoothing across every tile edge did something in the model, so the comparison above saw it
    for c, s in enumerate(shapes(p)):
        g = GM.unsmoothed(pics[2][c], c, bd, grain.tables[c], seeds[2], grain.log2_scale)
        for x in range(TW, s[1], TW):
            assert not np.array_equal(GM.smoothed(g)[:, x - 1:x + 1], g[:, x - 1:x + 1]), (c, x)
    uni = E.make_grain(255, 14, 14)
    verify(eng, eng.pics_grain(ids[:1], uni, 9)[0], p, model(pics[:1], p, uni, [9])[0], "uniform")
    eng.close()


@pytest.mark.parametrize("bd,cf", [(8, 1), (10, 3)])
def test_one_block_and_one_edge(bd, cf):
    """8 x 8: one block, no edge to smooth (4:2:0: chroma blocks of 4 x 4); 16 x 8: one edge"""
    rng = np.random.default_rng(88 + bd)
    eng = E.Engine(0)
    grain = E.make_grain(200, 14, 14, log2_scale=2)
    for w in (8, 16):
        p = params(w, 8, bd, cf)
        pl = planes_of("random", p, rng)
        out = eng.pics_grain([put(eng, p, pl)], grain, [w])
        verify(eng, out[0], p, model([pl], p, grain, [w])[0], w)
        if w == 8:                                                          # without an edge the smoothing changes nothing
            verify(eng, out[0], p, GM.apply(pl, bd, grain.tables, 8, 7, 0, 2, smooth=False), "unsmoothed")
    eng.close()


def test_gaps_on_a_ramp():
    """a table with gaps on the ramp picture: a block whose mean lies in a gap is unchanged except for its one column next to a
    neighbour in its row that has grain"""
    eng = E.Engine(0)
    bd = 8
    p = params(136, 72, bd, 0)
    ramp = planes_of("ramp", p, np.random.default_rng(0))
    t = np.zeros((3, 256), dtype=np.uint32)
    t[0, 40:90] = GM.entry(120, 5, 9)
    t[0, 150:200] = GM.entry(200, 12, 4)
    grain = E.Grain(t, 1, 0, 1)
    out = eng.pics_grain([put(eng, p, ramp)], grain, [3])
    got = get(eng, out[0], p)[0]
    verify(eng, out[0], p, model([ramp], p, grain, [3])[0], "gaps")
    src = ramp[0]
    in_gap = grained = touched = 0
    for by in range(9):
        means = [GM.mean8(src[8 * by:8 * by + 8, 8 * bx:8 * bx + 8], bd) for bx in range(17)]
        has = [bool(t[0, m] & 255) for m in means]
        for bx in range(17):
            blk = (slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
            if has[bx]:
                grained += 1
                assert not np.array_equal(got[blk], src[blk])
                continue
            in_gap += 1
            same = got[blk] == src[blk]
            assert same[:, 1:7].all(), (bx, by)
            assert same[:, 0].all() or (bx > 0 and has[bx - 1]), (bx, by)
            assert same[:, 7].all() or (bx < 16 and has[bx + 1]), (bx, by)
            touched += int(not same.all())
    assert in_gap > 20 and grained > 20 and touched > 2
    eng.close()


def test_sigma_zero_is_a_copy():
    rng = np.random.default_rng(4)
    eng = E.Engine(0)
    for bd, cf in ((8, 1), (10, 2)):
        p = params(72, 40, bd, cf)
        pl = planes_of("random", p, rng)
        pid = put(eng, p, pl)
        verify(eng, eng.pics_grain([pid], E.make_grain(0, 5, 5), 1)[0], p, pl, "sigma 0")
        verify(eng, eng.pics_grain([pid], E.Grain(np.zeros((3, 256), np.uint32)), 1)[0], p, pl, "entry 0")
        # sigma 0 needs no legal cut-offs: such an entry names no pattern
        verify(eng, eng.pics_grain([pid], E.Grain(np.full((3, 256), 0xFF00, np.uint32)), 1)[0], p, pl, "sigma 0, cut-offs 15")
    eng.close()


@pytest.mark.parametrize("blending", ["additive", "multiplicative"])
@pytest.mark.parametrize("log2_scale", [0, 15])
def test_blendings_clip_at_black_and_white(blending, log2_scale):
    eng = E.Engine(0)
    rng = np.random.default_rng(log2_scale)
    for bd, cf in ((8, 1), (12, 1)):
        M = (1 << bd) - 1
        p = params(72, 40, bd, cf)
        grain = E.make_grain(255, 9, 7, log2_scale=log2_scale, blending=blending)
        pics = [flat(p, 0), flat(p, M), flat(p, 1), flat(p, M - 1), planes_of("random", p, rng)]
        ids = [put(eng, p, pl) for pl in pics]
        out = eng.pics_grain(ids, grain, 100)
        want = model(pics, p, grain, [100 + i for i in range(5)])
        for i, d in enumerate(out):
            verify(eng, d, p, want[i], (blending, log2_scale, bd, i))
        if log2_scale == 0:
            assert want[1][0].max() == M and want[1][0].min() < M and want[0][0].min() == 0     # clipped at both ends
            assert (want[0][0].max() > 0) == (blending == "additive")       # multiplicative grain leaves black black
        else:
            assert all(np.array_equal(a, b) for a, b in zip(want[4], pics[4]))   # 255 * 127 * 16 / 2^20 rounds to 0
    eng.close()


@pytest.mark.parametrize("mask", (1, 6, 7, 0, 2))
def test_plane_masks(mask):
    rng = np.random.default_rng(mask)
    eng = E.Engine(0)
    grain = E.make_grain(90, 4, 11, log2_scale=1)
    for bd, cf in ((10, 1), (8, 3)):
        p = params(72, 40, bd, cf)
        pl = planes_of("random", p, rng)
        pid = put(eng, p, pl)
        want = model([pl], p, grain, [9], mask)[0]
        for c in range(3):
            assert np.array_equal(want[c], pl[c]) == (not mask >> c & 1)
        verify(eng, eng.pics_grain([pid], grain, [9], planes=mask)[0], p, want, ("mask", mask))
    g = params(72, 40, 8, 0)                                                # 4:0:0: bits 1 and 2 are ignored
    pl = planes_of("random", g, rng)
    verify(eng, eng.pics_grain([put(eng, g, pl)], grain, [9], planes=mask)[0], g, model([pl], g, grain, [9], mask)[0], "4:0:0")
    eng.close()


def test_seeds():
    """the same seed gives the same picture, another seed another one; one int stands for a run of seeds"""
    rng = np.random.default_rng(6)
    eng = E.Engine(0)
    p = params(136, 72, 10, 1)
    pl = planes_of("random", p, rng)
    pid = put(eng, p, pl)
    grain = E.make_grain(60, 8, 8, log2_scale=2)
    a, b, c = eng.pics_grain([pid, pid, pid], grain, [41, 41, 42])
    ga, gb, gc = get(eng, a, p), get(eng, b, p), get(eng, c, p)
    assert all(np.array_equal(x, y) for x, y in zip(ga, gb)) and all(not np.array_equal(x, y) for x, y in zip(ga, gc))
    run = eng.pics_grain([pid, pid], grain, 41)
    verify(eng, run[0], p, ga, "41")
    verify(eng, run[1], p, gc, "42")
    wrap = eng.pics_grain([pid, pid], grain, 0xFFFFFFFF)                    # the run wraps at 2^32
    verify(eng, wrap[1], p, model([pl], p, grain, [0])[0], "wrapped")
    eng.close()


def test_more_than_one_launch_sources_untouched_and_out():
    """70 pictures of 32 x 16 in one call, each with its own content and seed; the sources keep their checksums; out= is reused"""
    rng = np.random.default_rng(70)
    eng = E.Engine(0)
    n = E.CONV_MAX_PICS + 6
    p = params(32, 16, 10, 1)
    pics = [planes_of("random", p, rng) for _ in range(n)]
    ids = [put(eng, p, pl) for pl in pics]
    before = eng.pics_hash(ids, 2)
    grain = E.Grain(interval_tables(rng), 7, 0, 2)
    seeds = [int(v) for v in rng.integers(0, 1 << 32, n)]
    out = eng.pics_grain(ids, grain, seeds)
    assert len(out) == n and len(set(out)) == n and not set(out) & set(ids)
    used = E.Grain(grain.tables.copy(), 7, 0, 2)
    grain.tables[...] = 0                                                   # the call has copied them
    for pl, d, want in zip(pics, out, model(pics, p, used, seeds)):
        verify(eng, d, p, want, "70")
    assert eng.pics_hash(ids, 2) == before
    reuse = eng.pics_grain(ids[:2], used, [5, 6], out=out[:2])              # destinations given, twice in a row
    reuse = eng.pics_grain(ids[:2], used, [7, 8], out=out[:2])
    assert reuse == out[:2]
    verify(eng, out[1], p, model(pics[1:2], p, used, [8])[0], "reused")
    assert eng.pics_grain([], used, []) == [] and eng.pics_grain([], used, 0, out=[]) == []
    eng.close()


def test_a_message_parsed_from_bytes():
    """SEI bytes -> annexb.film_grain -> grain_from_sei -> pics_grain: luma in two intervals, Cr in one, Cb copied"""
    import test_film_grain_sei as S
    d = S.grain([[(0, 99, [60, 4, 12]), (130, 255, [35, 9, 9])], None, [(0, 255, [80, 10])]], scale=3, persistence=True)
    read = A.film_grain(S.unit(d))
    assert read == d
    grain = E.grain_from_sei(read)
    assert (grain.planes, grain.blending, grain.log2_scale) == (5, 0, 3) and np.array_equal(grain.tables, GM.from_sei(d)[1])
    rng = np.random.default_rng(19)
    eng = E.Engine(0)
    p = params(136, 72, 10, 1)
    pics = [planes_of(k, p, rng) for k in ("random", "ramp")]
    out = eng.pics_grain([put(eng, p, pl) for pl in pics], grain, 16)       # POC 16 and 17
    for pl, dst, want in zip(pics, out, model(pics, p, grain, [16, 17])):
        verify(eng, dst, p, want, "sei")
        assert np.array_equal(want[1], pl[1]) and not np.array_equal(want[2], pl[2])
    eng.close()


def test_argument_errors_write_nothing():
    """every OH_E_ARG rule of ohevc_hip.h through the raw C call: refused on the host, the pictures' checksums stay; n == 0 is fine"""
    eng = E.Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)
    sp = params(32, 16, 10, 1)

    def some(p):
        return put(eng, p, planes_of("random", p, rng))

    src, dst = [some(sp), some(sp)], [some(sp), some(sp)]
    other_s, other_d = some(params(32, 16, 10, 2)), some(params(32, 16, 9, 1))
    dst8 = [some(params(32, 16, 8, 1)), some(params(32, 16, 8, 1))]
    wide = [some(params(40, 16, 10, 1)), some(params(40, 16, 10, 1))]
    mono = [some(params(32, 16, 10, 0)), some(params(32, 16, 10, 0)), some(params(32, 16, 10, 0)), some(params(32, 16, 10, 0))]
    watched = src + dst + dst8 + wide + mono + [other_s, other_d]

    def sums():
        return [eng.pics_hash([pid], 2) for pid in watched]

    before = sums()
    keep = []
    P32 = C.POINTER(C.c_uint32)
    good = [GM.uniform(50, 8, 8) for _ in range(3)]

    def call(s=src, d=dst, n=None, planes=7, blending=0, log2_scale=0, tabs=good, g_null=False, e_null=False, seeds_null=False):
        g = E.OhGrain(planes, blending, log2_scale)
        for c, t in enumerate(tabs):
            if t is not None:
                g.table[c] = t.ctypes.data_as(P32)
        sa = (C.c_int * max(len(s), 1))(*s) if s is not None else None
        da = (C.c_int * max(len(d), 1))(*d) if d is not None else None
        sd = (C.c_uint32 * 4)(1, 2, 3, 4)
        keep.extend((g, sa, da, tabs, sd))
        return L.oh_pics_grain(None if e_null else eng.h, sa, da, len(s or d or []) if n is None else n, None if g_null else C.byref(g),
                               None if seeds_null else sd)

    arg = E.OH_E_ARG
    assert call(e_null=True) == arg and call(g_null=True) == arg and call(seeds_null=True) == arg                            # null arguments
    assert call(s=None, n=2) == arg and call(d=None, n=2) == arg and call(n=-1) == arg
    assert call(s=[src[0], 999]) == arg and call(d=[dst[0], 999]) == arg and call(s=[-1, src[1]]) == arg                      # unknown pictures
    assert call(s=[src[0], other_s]) == arg and call(d=[dst[0], other_d]) == arg                            # params differ among themselves
    assert call(d=dst8) == arg and call(d=wide) == arg and call(d=mono[:2]) == arg                          # ... and between the sides
    assert call(d=[dst[0], dst[0]]) == arg                                                                  # a destination twice
    assert call(d=[dst[0], src[0]]) == arg and call(d=[src[1], dst[1]]) == arg and call(d=src) == arg        # source and destination
    for planes in (-1, 8, 15, 1 << 20):
        assert call(planes=planes) == arg and call(s=[], d=[], n=0, planes=planes) == arg, planes
    for blending in (-1, 2, 3):
        assert call(blending=blending) == arg and call(s=[], d=[], n=0, blending=blending) == arg, blending
    for ls in (-1, 16, 100):
        assert call(log2_scale=ls) == arg and call(s=[], d=[], n=0, log2_scale=ls) == arg, ls
    for c in range(3):
        assert call(tabs=[t if k != c else None for k, t in enumerate(good)]) == arg, c                     # no table for a selected plane
    for e in (GM.entry(1, 1, 8), GM.entry(1, 8, 15), GM.entry(255, 0, 0), GM.entry(1, 15, 15), 1, 1 << 16 | GM.entry(1, 8, 8), 0xFFFFFFFF):
        bad = [t.copy() for t in good]
        bad[1][77] = e
        assert call(tabs=bad) == arg, hex(e)                                                                # an entry that names no pattern
    eng.sync()
    assert sums() == before, "a refused call wrote into a picture"
    assert call(s=[], d=[], n=0) == 0 and call(s=None, d=None, n=0) == 0 and call(s=[], d=[], n=0, tabs=[None] * 3) == 0      # n == 0
    eng.sync()
    assert sums() == before
    bad = [t.copy() for t in good]
    bad[1][77] = 1
    assert call(planes=5, tabs=[good[0], None, good[2]]) == 0                                               # an unselected plane needs no table ...
    assert call(planes=5, tabs=bad) == 0                                                                    # ... and its table is not read
    assert call(s=mono[:2], d=mono[2:], tabs=[good[0], None, None]) == 0                                    # planes the format lacks need none
    assert call(s=[src[0], src[0]], d=dst) == 0                                                             # a source twice is fine
    sigma0 = [np.full(256, 0xFF00, np.uint32)] * 3
    assert call(tabs=sigma0) == 0                                                                           # sigma 0 asks for no pattern
    eng.sync()
    after = sums()
    assert after[:2] == before[:2] and after[2] != before[2] and after[4:8] == before[4:8] and after[8:10] == before[8:10]
    assert after[10] != before[10] and after[12:] == before[12:]
    with pytest.raises(E.EngineError) as ei:
        eng.pics_grain(src, E.make_grain(5), 0, planes=8)
    assert ei.value.code == arg
    with pytest.raises(E.EngineError) as ei:
        eng.pics_grain(src, E.make_grain(5), 0, out=dst8)
    assert ei.value.code == arg
    eng.close()
