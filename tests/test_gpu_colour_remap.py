"""-m gpu: oh_pics_colour_remap / Engine.pics_colour_remap on the MI355X against the numpy model of tests/remap_model.py, every coded
plane of every destination bit for bit: eight pairs of bit depths at 72 x 40 and 136 x 72 (rows that are no whole granules at 8 bit,
more than one band of rows) with random tables over the full output range and a random matrix with negative entries, so that the
gathers reach every part of each table and both clips occur, three pictures of different content per call; 520 x 24, where a band has
more units than the workgroup has lanes; the smallest picture; the identity; a diagonal matrix against
oh_pics_lut with Remap.luts() on the same pictures, and through oh_pics_lut on a 4:2:0 picture; extreme coefficients at d = 0 and 15;
more than one launch; untouched sources; out= reuse; a message parsed from bytes; and the argument rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import levels_model as LM                                                   # noqa: E402
import remap_model as RM                                                    # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = [(8, 8), (8, 10), (10, 8), (10, 10), (12, 12), (9, 12), (12, 9), (12, 8)]
SIZES = [(72, 40), (136, 72)]


def params(w, h, bd, cf=3):
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


def get(eng, pid, p):
    got = eng.pic_download(pid, p)
    return [got.visible(c).copy() for c in range(F.n_planes(p))]


def verify(eng, pid, p, want, what=None):
    got = get(eng, pid, p)
    assert len(want) == len(got)
    for c in range(len(got)):
        assert got[c].dtype == want[c].dtype
        assert np.array_equal(got[c], want[c]), (what, c, np.argwhere(got[c] != want[c])[:4])


def random_remap(rng, bi, bo, d):
    pre, post = RM.random_tables(rng, bi, bo)
    return E.Remap(pre, RM.random_matrix(rng, d), d, post, bi, bo)


def model(pl, r, counts=None):
    return RM.apply(pl, r.pre, r.coeff, r.log2_denom, r.post, r.in_bit_depth, r.out_bit_depth, counts)


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("bi,bo", PAIRS, ids=[f"{bi}to{bo}" for bi, bo in PAIRS])
def test_depth_pairs(bi, bo, w, h):
    rng = np.random.default_rng(100 * bi + bo + w)
    eng = E.Engine(0)
    sp, dp = params(w, h, bi), params(w, h, bo)
    assert h > E.REMAP_ROWS                                                 # more than one band of rows
    r = random_remap(rng, bi, bo, 11)
    pics = [planes_of(k, sp, rng) for k in ("random", "ramp", "top")]       # noise, a ramp, flat at Mi
    ids = [put(eng, sp, pl) for pl in pics]
    out = eng.pics_colour_remap(ids, r)
    assert len(out) == 3 and not set(out) & set(ids)
    counts = []
    for pl, d in zip(pics, out):
        q = eng._pic_params(d)
        assert (q.width, q.height, q.bit_depth, q.chroma_format_idc) == (w, h, bo, 3)
        verify(eng, d, dp, model(pl, r, counts), (bi, bo))
        assert eng.pic_final_half(d) == 0
    assert counts[0][0] > 0 and counts[0][1] > 0                            # both clips occurred on the noise
    eng.close()


@pytest.mark.parametrize("w,h", [(520, 24), (1032, 16)])
@pytest.mark.parametrize("bi,bo", [(10, 10), (8, 12)])
def test_more_units_in_a_band_than_lanes(bi, bo, w, h):
    """520 x 24: 33 units a row, 264 in a band of REMAP_ROWS = 8 rows for 256 lanes, so a lane's loop runs more than once, for a few
    lanes only; three bands.  The band height that was measured to be best divides every coded height (a multiple of the minimum
    coding block of 8), so no picture has a cut band; at 16 rows this one's second band was 8 rows.  1032 x 16: 65 units a row, 520 in
    a band: every lane's loop runs twice and a few lanes' three times"""
    assert 256 < (w + 15) // 16 * E.REMAP_ROWS and h > E.REMAP_ROWS
    rng = np.random.default_rng(bi + bo)
    eng = E.Engine(0)
    sp, dp = params(w, h, bi), params(w, h, bo)
    r = random_remap(rng, bi, bo, 7)
    pics = [planes_of(k, sp, rng) for k in ("random", "ramp")]
    out = eng.pics_colour_remap([put(eng, sp, pl) for pl in pics], r)
    for pl, d in zip(pics, out):
        verify(eng, d, dp, model(pl, r), (bi, bo))
    eng.close()


@pytest.mark.parametrize("bi,bo", [(8, 8), (10, 12), (12, 8)])
def test_smallest_picture(bi, bo):
    rng = np.random.default_rng(8 + bi)
    eng = E.Engine(0)
    sp, dp = params(8, 8, bi), params(8, 8, bo)
    r = random_remap(rng, bi, bo, 3)
    pl = planes_of("random", sp, rng)
    verify(eng, eng.pics_colour_remap([put(eng, sp, pl)], r)[0], dp, model(pl, r), "8x8")
    eng.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_identity_is_a_copy(bd):
    rng = np.random.default_rng(bd)
    eng = E.Engine(0)
    p = params(72, 40, bd)
    pics = [planes_of(k, p, rng) for k in ("random", "ramp")]
    ids = [put(eng, p, pl) for pl in pics]
    for d in (0, 9, 14):                                                    # 2^15 is no coefficient
        out = eng.pics_colour_remap(ids, E.make_remap(None, None, d, None, bd))
        for pl, dst in zip(pics, out):
            verify(eng, dst, p, pl, ("identity", d))
    # the identity matrix between tables that are not: the path without the matrix, against the model
    r = random_remap(rng, bd, bd, 6)
    r = E.Remap(r.pre, np.eye(3, dtype=np.int64) << 6, 6, r.post, bd)
    verify(eng, eng.pics_colour_remap(ids[:1], r)[0], p, model(pics[0], r), "identity matrix")
    eng.close()


@pytest.mark.parametrize("bi,bo", [(8, 8), (10, 8), (8, 12), (12, 12)])
def test_diagonal_matrix_equals_pics_lut(bi, bo):
    """a check against the existing kernel, independent of the model: the remap with a diagonal matrix and oh_pics_lut with
    Remap.luts() give the same 4:4:4 pictures; and Remap.luts() through oh_pics_lut on a 4:2:0 picture equals the model"""
    rng = np.random.default_rng(10 * bi + bo)
    eng = E.Engine(0)
    sp, dp = params(136, 72, bi), params(136, 72, bo)
    pre, post = RM.random_tables(rng, bi, bo)
    r = E.Remap(pre, np.diag([700, -3, 1500]), 9, post, bi, bo)
    pics = [planes_of(k, sp, rng) for k in ("random", "ramp")]
    ids = [put(eng, sp, pl) for pl in pics]
    a = eng.pics_colour_remap(ids, r)
    b = eng.pics_lut(ids, list(r.luts()), bit_depth=bo)
    for x, y in zip(a, b):
        verify(eng, x, dp, get(eng, y, dp), "lut")
    s420, d420 = params(136, 72, bi, 1), params(136, 72, bo, 1)
    pl = planes_of("random", s420, rng)
    out = eng.pics_lut([put(eng, s420, pl)], list(r.luts()), bit_depth=bo)
    k = r.luts()
    dt = np.uint16 if bo > 8 else np.uint8
    verify(eng, out[0], d420, [k[c][pl[c]].astype(dt) for c in range(3)], "4:2:0")
    # the model on full planes of the same samples: plane c depends on plane c alone
    want = RM.luts(r.pre, r.coeff, r.log2_denom, r.post, bi, bo)
    assert np.array_equal(k, want)
    eng.close()


@pytest.mark.parametrize("d", [0, 15])
@pytest.mark.parametrize("bi,bo", [(12, 12), (8, 12), (12, 8)])
def test_extreme_coefficients(bi, bo, d):
    """rows of +-32767 / -32768 on tables that hold Mo: the sums reach 3 * 32768 * 4095 either way"""
    rng = np.random.default_rng(d + bi)
    eng = E.Engine(0)
    sp, dp = params(72, 40, bi), params(72, 40, bo)
    pre, post = RM.random_tables(rng, bi, bo)
    pre[:, ::2] = (1 << bo) - 1
    pics = [planes_of(k, sp, rng) for k in ("random", "zero")]
    ids = [put(eng, sp, pl) for pl in pics]
    for k in ([[32767] * 3, [-32768] * 3, [32767, -32768, 32767]], [[-32768, 32767, 0], [1, -1, 1], [32767, 32767, -32768]]):
        r = E.Remap(pre, k, d, post, bi, bo)
        for pl, dst in zip(pics, eng.pics_colour_remap(ids, r)):
            verify(eng, dst, dp, model(pl, r), (d, k))
    eng.close()


def test_more_than_one_launch_sources_untouched_and_out():
    """65 pictures of 72 x 40 in one call, each with its own content; the sources keep their checksums; out= is reused"""
    rng = np.random.default_rng(65)
    eng = E.Engine(0)
    n = E.CONV_MAX_PICS + 1
    sp, dp = params(72, 40, 10), params(72, 40, 8)
    pics = [planes_of("random", sp, rng) for _ in range(n)]
    ids = [put(eng, sp, pl) for pl in pics]
    before = eng.pics_hash(ids, 2)
    r = random_remap(rng, 10, 8, 12)
    out = eng.pics_colour_remap(ids, r)
    assert len(out) == n and len(set(out)) == n and not set(out) & set(ids)
    used = E.Remap(r.pre.copy(), r.coeff.copy(), r.log2_denom, r.post.copy(), 10, 8)
    r.pre[...] = 0                                                          # the call has copied them
    r.post[...] = 0
    for pl, d in zip(pics, out):
        verify(eng, d, dp, model(pl, used), "65")
    assert eng.pics_hash(ids, 2) == before
    other = random_remap(rng, 10, 8, 2)
    reuse = eng.pics_colour_remap(ids[:2], used, out=out[:2])               # destinations given, twice in a row with other tables
    reuse = eng.pics_colour_remap(ids[:2], other, out=out[:2])
    assert reuse == out[:2]
    verify(eng, out[1], dp, model(pics[1], other), "reused")
    assert eng.pics_colour_remap([], used) == [] and eng.pics_colour_remap([], used, out=[]) == []
    eng.close()


def test_a_message_parsed_from_bytes():
    """SEI bytes -> annexb.colour_remap -> remap_from_sei -> pics_colour_remap, 10 -> 8 bit, the message of one id among two"""
    import test_colour_remap_sei as S
    rng = np.random.default_rng(142)
    d = S.remap(10, 8, pre=[RM.random_pivots(rng, 10, 8, 33), [], [(100, 30), (900, 220)]],
                matrix=(8, [[300, -60, 20], [-40, 280, 10], [5, -100, 350]]),
                post=[[], RM.random_pivots(rng, 8, 8, 9), [(0, 255), (255, 0)]], id=2, signal=S.BT2020)
    n = S.unit(S.remap(10, 10, id=1), d)
    read = A.colour_remap(n, id=2)
    assert read == d and A.colour_remap(n, id=1)["output_bit_depth"] == 10
    r = E.remap_from_sei(read)
    for c in range(3):
        assert np.array_equal(r.pre[c], RM.curve(10, 8, d["pre"][c])) and np.array_equal(r.post[c], RM.curve(8, 8, d["post"][c]))
    eng = E.Engine(0)
    sp, dp = params(136, 72, 10), params(136, 72, 8)
    pics = [planes_of(k, sp, rng) for k in ("random", "ramp")]
    out = eng.pics_colour_remap([put(eng, sp, pl) for pl in pics], r)
    for pl, dst in zip(pics, out):
        verify(eng, dst, dp, model(pl, r), "sei")
    eng.close()


def test_argument_errors_write_nothing():
    """every OH_E_ARG and OH_E_UNSUPPORTED rule of ohevc_hip.h through the raw C call: refused on the host, the destinations still hold
    what was uploaded and every picture keeps its checksum; n == 0 is fine"""
    eng = E.Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)
    sp, dp = params(32, 16, 10), params(32, 16, 8)
    uploaded = {}

    def some(p):
        pl = planes_of("random", p, rng)
        pid = put(eng, p, pl)
        uploaded[pid] = (p, pl)
        return pid

    src, dst = [some(sp), some(sp)], [some(dp), some(dp)]
    src9, dst10 = some(params(32, 16, 9)), [some(sp), some(sp)]
    wide = [some(params(40, 16, 8)), some(params(40, 16, 8))]
    tall = [some(params(32, 24, 8)), some(params(32, 24, 8))]
    s420, s422, s400 = [some(params(32, 16, 10, 1)) for _ in range(2)], [some(params(32, 16, 10, 2)) for _ in range(2)], \
        [some(params(32, 16, 10, 0)) for _ in range(2)]
    d420 = [some(params(32, 16, 8, 1)) for _ in range(2)]
    watched = list(uploaded)

    def sums():
        return [eng.pics_hash([pid], 2) for pid in watched]

    before = sums()
    keep = []
    P16 = C.POINTER(C.c_uint16)
    pre_ok, post_ok = RM.random_tables(rng, 10, 8)
    ident = [[4, 0, 0], [0, 4, 0], [0, 0, 4]]

    def call(s=src, d=dst, n=None, bi=10, bo=8, pre=pre_ok, post=post_ok, coeff=ident, log2_denom=2, r_null=False, e_null=False,
             no_pre=None, no_post=None):
        r = E.OhRemap(bi, bo)
        r.log2_denom = log2_denom
        pre, post = np.ascontiguousarray(pre, dtype=np.uint16), np.ascontiguousarray(post, dtype=np.uint16)
        for c in range(3):
            if c != no_pre:
                r.pre[c] = pre[c].ctypes.data_as(P16)
            if c != no_post:
                r.post[c] = post[c].ctypes.data_as(P16)
            for i in range(3):
                r.coeff[c][i] = coeff[c][i]
        sa = (C.c_int * max(len(s), 1))(*s) if s is not None else None
        da = (C.c_int * max(len(d), 1))(*d) if d is not None else None
        keep.extend((r, sa, da, pre, post))
        return L.oh_pics_colour_remap(None if e_null else eng.h, sa, da, len(s or d or []) if n is None else n, None if r_null else C.byref(r))

    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    assert call(e_null=True) == arg and call(r_null=True) == arg                                           # null arguments
    assert call(s=None, n=2) == arg and call(d=None, n=2) == arg and call(n=-1) == arg
    assert call(s=[src[0], 999]) == arg and call(d=[dst[0], 999]) == arg and call(s=[-1, src[1]]) == arg    # unknown pictures
    assert call(s=[src[0], src9]) == arg and call(d=[dst[0], wide[0]]) == arg                               # params differ on one side
    assert call(d=[dst[0], dst[0]]) == arg                                                                  # a destination twice
    assert call(d=[dst10[0], src[0]], bo=10, post=np.zeros((3, 1024))) == arg and call(d=src, bo=10, post=np.zeros((3, 1024))) == arg
    assert call(d=wide) == arg and call(d=tall) == arg                                                      # sizes that differ
    assert call(d=dst10) == arg and call(s=dst10, bi=10, bo=8, d=src) == arg                                # a picture depth other than the struct's
    assert call(s=[src9, src9]) == arg and call(bi=8, pre=pre_ok[:, :256]) == arg
    big = np.zeros((3, 1 << 16))
    for bd in (0, 7, 11, 13, 14, 16, -1):                                                                   # struct depths, with and without pictures
        assert call(bi=bd, pre=big) == arg and call(bo=bd, post=big) == arg, bd
        assert call(s=[], d=[], n=0, bi=bd, pre=big) == arg and call(s=[], d=[], n=0, bo=bd, post=big) == arg, bd
    for c in range(3):
        assert call(no_pre=c) == arg and call(no_post=c) == arg and call(s=[], d=[], n=0, no_post=c) == arg  # a null table
        for table, v, where in (("pre", 256, 1023), ("pre", 65535, 0), ("post", 256, 255), ("post", 4095, 17)):
            bad = (pre_ok if table == "pre" else post_ok).copy()
            bad[c, where] = v
            assert call(**{table: bad}) == arg, (c, table, v)                                               # an entry above Mo
    for k in (32768, -32769, 1 << 20, -(1 << 31)):
        for c, i in ((0, 0), (1, 2), (2, 1)):
            bad = [row[:] for row in ident]
            bad[c][i] = k
            assert call(coeff=bad) == arg and call(s=[], d=[], n=0, coeff=bad) == arg, (k, c, i)            # a coefficient outside int16
    for ld in (-1, 16, 100):
        assert call(log2_denom=ld) == arg and call(s=[], d=[], n=0, log2_denom=ld) == arg, ld
    # chroma formats other than 4:4:4 on either side
    assert call(s=s420, d=d420) == uns and call(s=s422) == uns and call(s=s400) == uns and call(d=d420) == uns
    assert b"oh_pics_reformat first, or oh_remap_luts with oh_pics_lut where the matrix is diagonal" in L.oh_engine_last_error(eng.h)
    eng.sync()
    assert sums() == before, "a refused call wrote into a picture"
    for pid in dst + dst10 + d420:                                                                          # the destinations still hold what was uploaded
        verify(eng, pid, *uploaded[pid], "refused")
    assert call(s=[], d=[], n=0) == 0 and call(s=None, d=None, n=0) == 0                                    # n == 0
    eng.sync()
    assert sums() == before
    assert call(coeff=[[32767, -32768, 0]] * 3, log2_denom=15) == 0 and call(log2_denom=0) == 0             # the ends of the domains
    assert call(s=[src[0], src[0]]) == 0                                                                    # a source twice is fine
    eng.sync()
    after = sums()
    assert after[:2] == before[:2] and after[2] != before[2] and after[3] != before[3] and after[4:] == before[4:]
    with pytest.raises(E.EngineError) as ei:
        eng.pics_colour_remap(src, E.make_remap(None, None, 16, None, 10, 8))
    assert ei.value.code == arg
    with pytest.raises(E.EngineError) as ei:
        eng.pics_colour_remap(s420, E.make_remap(None, None, 0, None, 10, 8))
    assert ei.value.code == uns
    with pytest.raises(E.EngineError) as ei:
        eng.pics_colour_remap(src, E.make_remap(None, None, 0, None, 10, 8), out=dst10)
    assert ei.value.code == arg
    eng.close()
