"""-m gpu: oh_pics_unpack / oh_pics_pack (Engine.pics_unpack / pics_pack) on the MI355X against the numpy model of
tests/packing_model.py, every coded plane of every destination bit for bit.  Packed 80 x 24 (halves of 40 samples: two and a half
granules at 8 bit, so the seam lies inside a granule; top-bottom halves of 12 rows in views of 16 coded rows, whose last rows replicate)
and 136 x 72 (side-by-side halves of 68 samples in views of 72 coded columns), chroma formats 0 .. 3 at 8 and 10 bit and 4:4:4 at
12 bit, both arrangements, half size, full size and quincunx, all four flip combinations, grid positions that see all 16 phases, on
noise, a ramp and two views of different flat levels; the smallest picture, where each view is narrower than the filter; one view
alone; more pictures than one launch takes; untouched sources; out= reuse; a descriptor parsed from bytes; pack then unpack; and the
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
import packing_model as M                                                   # noqa: E402
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(80, 24), (136, 72)]
FORMATS = [(8, 0), (8, 1), (8, 2), (8, 3), (10, 0), (10, 1), (10, 2), (10, 3), (12, 3)]
FLIPS = list(itertools.product((False, True), repeat=2))
# (x, y) of view 0, (x, y) of view 1; the component on the packed axis takes the values 0, 8, 4, 12, 1, 10, 3, 14, 5, 7 in both
# arrangements: every residue mod 8, so that a plane that is not sub-sampled sees all 16 phases (tests/test_packing_model.py)
GRIDS = [((0, 0), (8, 8)), ((8, 8), (0, 0)), ((4, 4), (12, 12)), ((1, 1), (10, 10)), ((3, 3), (14, 14)), ((5, 5), (7, 7))]
ARRS = [M.SBS, M.TB]


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def shapes(p):
    return [F.plane_dims(p, c)[::-1] for c in range(F.n_planes(p))]


def content(kind, p, rng, arr=M.SBS):
    dt = np.uint8 if p.bit_depth == 8 else np.uint16
    top = (1 << p.bit_depth) - 1
    out = []
    for c, (h, w) in enumerate(shapes(p)):
        if kind == "noise":
            a = rng.integers(0, top + 1, (h, w))
        elif kind == "ramp":
            y, x = np.mgrid[0:h, 0:w]
            a = (x * 7 + y * 13 + c * 50) % (top + 1)
        else:                                                 # two views of different flat levels: the seam shows any tap across it
            a = np.full((h, w), top // 5 + c)
            if arr == M.SBS:
                a[:, w // 2:] = top - 3 * c
            else:
                a[h // 2:, :] = top - 3 * c
        out.append(a.astype(dt))
    return out


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
        assert got[c].shape == want[c].shape, (what, c, got[c].shape, want[c].shape)
        assert np.array_equal(got[c], want[c]), (what, c, np.argwhere(got[c] != want[c])[:4])


def want_view(pk, planes, p, v, full):
    """the coded planes of view v by the model, and the view's params"""
    vp = pk.view_size(p, full)
    sbs = pk.arrangement == M.SBS
    out = []
    for c, pl in enumerate(planes):
        win = M.unpack_plane(pl, pk.arrangement, v, flip=pk.flip[v], g=pk.grid[v][0 if sbs else 1], quincunx=pk.quincunx, full=full, plane=c,
                             chroma_format_idc=p.chroma_format_idc, bit_depth=p.bit_depth)
        hs, vs = M.shifts(p.chroma_format_idc, c)
        out.append(M.coded(win, vp.height >> vs, vp.width >> hs).astype(pl.dtype))
    return out, vp


def windows(pk, p, planes, full):
    """the windows of a view's coded planes"""
    out = []
    for c, pl in enumerate(planes):
        hs, vs = M.shifts(p.chroma_format_idc, c)
        w, h = M.view_size(p.width, p.height, pk.arrangement, full)[:2]
        out.append(pl[:h >> vs, :w >> hs])
    return out


def check_unpack(eng, p, pk, full, pics, ids, what):
    v0, v1 = eng.pics_unpack(ids, pk, full)
    assert len(v0) == len(v1) == len(ids) and not set(v0 + v1) & set(ids)
    for pl, a, b in zip(pics, v0, v1):
        for v, pid in ((0, a), (1, b)):
            want, vp = want_view(pk, pl, p, v, full)
            q = eng._pic_params(pid)
            assert (q.width, q.height, q.bit_depth, q.chroma_format_idc) == (vp.width, vp.height, p.bit_depth, p.chroma_format_idc)
            verify(eng, pid, vp, want, (what, v))
            assert eng.pic_final_half(pid) == 0
    for pid in v0 + v1:
        eng.pic_free(pid)


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("bd,cf", FORMATS, ids=[f"{bd}bit-cf{cf}" for bd, cf in FORMATS])
def test_unpack_against_the_model(bd, cf, w, h):
    rng = np.random.default_rng(1000 * bd + 10 * cf + w)
    eng = E.Engine(0)
    p = params(w, h, bd, cf)
    for arr in ARRS:
        pics = [content(k, p, rng, arr) for k in ("noise", "ramp", "flat")]
        ids = [put(eng, p, pl) for pl in pics]
        for i, flip in enumerate(FLIPS):
            check_unpack(eng, p, E.make_packing(arr, flip=flip), False, pics, ids, ("half", arr, flip))
            check_unpack(eng, p, E.make_packing(arr, flip=flip, grid=GRIDS[i]), True, pics, ids, ("full", arr, flip, GRIDS[i]))
            check_unpack(eng, p, E.make_packing(arr, flip=flip, quincunx=True), True, pics, ids, ("quincunx", arr, flip))
            check_unpack(eng, p, E.make_packing(arr, flip=flip, quincunx=True), False, pics, ids, ("quincunx half", arr, flip))
        for grid in GRIDS[4:] + [tuple(tuple(int(v) for v in rng.integers(0, 16, 2)) for _ in range(2))]:
            check_unpack(eng, p, E.make_packing(arr, grid=grid), True, pics, ids, ("full", arr, grid))
    eng.close()


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("bd,cf", [(8, 1), (10, 2), (12, 3), (8, 0)], ids=["8bit-cf1", "10bit-cf2", "12bit-cf3", "8bit-cf0"])
def test_pack_against_the_model_and_back(bd, cf, w, h):
    """views -> oh_pics_pack -> the model's packed planes; -> oh_pics_unpack -> the views' windows again (with quincunx: on the lattice)"""
    rng = np.random.default_rng(7 * bd + cf + h)
    eng = E.Engine(0)
    p = params(w, h, bd, cf)
    for arr, quincunx in itertools.product(ARRS, (False, True)):
        vp = E.make_packing(arr, quincunx=quincunx).view_size(p, quincunx)
        views = [[content(k, vp, rng) for k in ("noise", "ramp")] for _ in range(2)]         # [view][picture][plane], whole coded planes
        vids = [[put(eng, vp, pl) for pl in views[v]] for v in range(2)]
        for flip in FLIPS:
            pk = E.make_packing(arr, quincunx=quincunx, flip=flip)
            # out=: the packed size, whose halves are windows of the views' coded planes where they are no whole coding blocks
            out = eng.pics_pack(vids[0], vids[1], pk, out=[eng.pic_alloc(p) for _ in vids[0]])
            for i, pid in enumerate(out):
                win = [windows(pk, p, views[v][i], quincunx) for v in range(2)]
                want = [M.pack_plane(win[0][c], win[1][c], arr, flip=flip, quincunx=quincunx).astype(win[0][c].dtype) for c in range(len(win[0]))]
                verify(eng, pid, p, want, ("pack", arr, quincunx, flip))
                assert eng.pic_final_half(pid) == 0
            back = eng.pics_unpack(out, pk, quincunx)
            for v in range(2):
                for i, pid in enumerate(back[v]):
                    got = windows(pk, p, get(eng, pid, vp), quincunx)
                    for c, g in enumerate(got):
                        src = windows(pk, p, views[v][i], quincunx)[c]
                        Y, X = np.mgrid[0:g.shape[0], 0:g.shape[1]]
                        on = ((X ^ Y ^ v) & 1) == 0 if quincunx else np.ones(g.shape, bool)
                        assert np.array_equal(g[on], src[on]), ("back", arr, quincunx, flip, v, c)
            for pid in out + back[0] + back[1]:
                eng.pic_free(pid)
    eng.close()


@pytest.mark.parametrize("bd,cf", [(8, 1), (10, 3), (8, 0)])
def test_smallest_picture(bd, cf):
    """8 x 8: a view holds 4 luma and 2 chroma samples on the packed axis, fewer than the filter has taps, so every output clamps taps
    at both ends; the half size rounds up to the full size, which is then what views of 8 x 8 mean"""
    rng = np.random.default_rng(bd + cf)
    eng = E.Engine(0)
    p = params(8, 8, bd, cf)
    for arr in ARRS:
        pics = [content(k, p, rng, arr) for k in ("noise", "flat")]
        ids = [put(eng, p, pl) for pl in pics]
        for flip, grid in zip(FLIPS, GRIDS):
            check_unpack(eng, p, E.make_packing(arr, flip=flip, grid=grid), True, pics, ids, ("8x8 full", arr, flip, grid))
            check_unpack(eng, p, E.make_packing(arr, flip=flip, quincunx=True), True, pics, ids, ("8x8 quincunx", arr, flip))
            # packing without quincunx takes the 8 x 8 views as halves: their top-left 4 x 8 (8 x 4) windows
            pk = E.make_packing(arr, flip=flip)
            out = eng.pics_pack([ids[0]], [ids[1]], pk, out=[eng.pic_alloc(p)])
            win = [windows(pk, p, pics[v], False) for v in range(2)]
            verify(eng, out[0], p, [M.pack_plane(win[0][c], win[1][c], arr, flip=flip).astype(pics[0][c].dtype) for c in range(len(pics[0]))], "8x8 pack")
            eng.pic_free(out[0])
    eng.close()


def test_one_view_alone():
    rng = np.random.default_rng(5)
    eng = E.Engine(0)
    p = params(80, 24, 10, 1)
    for arr in ARRS:
        pk = E.make_packing(arr, flip=(True, False), grid=((3, 9), (12, 6)))
        pics = [content(k, p, rng, arr) for k in ("noise", "ramp")]
        ids = [put(eng, p, pl) for pl in pics]
        for full in (False, True):
            for v in range(2):
                got = eng.pics_unpack(ids, pk, full, views=(v == 0, v == 1))
                assert got[1 - v] is None and len(got[v]) == 2
                for pl, pid in zip(pics, got[v]):
                    want, vp = want_view(pk, pl, p, v, full)
                    verify(eng, pid, vp, want, ("alone", arr, full, v))
                # the same into pictures that exist, through out=
                again = eng.pics_unpack(ids[::-1], pk, out=(got[v], None) if v == 0 else (None, got[v]))
                assert again[v] == got[v] and again[1 - v] is None
                for pl, pid in zip(pics[::-1], got[v]):
                    verify(eng, pid, vp, want_view(pk, pl, p, v, full)[0], ("alone, out=", arr, full, v))
    with pytest.raises(ValueError):
        eng.pics_unpack(ids, pk, views=(False, False))
    eng.close()


def test_more_pictures_than_one_launch():
    rng = np.random.default_rng(33)
    eng = E.Engine(0)
    p = params(24, 16, 8, 1)
    n = E.PACK_MAX_PICS + 3
    pk = E.make_packing("side_by_side", flip=(False, True), grid=((0, 0), (8, 0)))
    pics = [content("noise", p, rng) for _ in range(n)]
    ids = [put(eng, p, pl) for pl in pics]
    check_unpack(eng, p, pk, True, pics, ids, "35 pictures")
    halves = eng.pics_unpack(ids, pk, False)                  # halves of 12 columns in views of 16
    out = eng.pics_pack(halves[0], halves[1], pk, out=[eng.pic_alloc(p) for _ in ids])
    for pl, pid in zip(pics, out):
        verify(eng, pid, p, pl, "35 pictures, packed again")
    eng.close()


def test_sources_stay_and_out_is_reused():
    rng = np.random.default_rng(77)
    eng = E.Engine(0)
    p = params(136, 72, 10, 2)
    pk = E.make_packing("top_bottom", grid=((0, 4), (0, 12)), flip=(True, True))
    pics = [content(k, p, rng, M.TB) for k in ("noise", "ramp")]
    ids = [put(eng, p, pl) for pl in pics]
    before = [eng.pics_hash([pid], 2) for pid in ids]
    v0, v1 = eng.pics_unpack(ids, pk, True)
    eng.sync()
    assert [eng.pics_hash([pid], 2) for pid in ids] == before
    for pl, pid in zip(pics, ids):
        verify(eng, pid, p, pl, "source")
    # the views made above as destinations of another descriptor, and the packed pictures as destinations of pack
    pk2 = E.make_packing("top_bottom", quincunx=True)
    got = eng.pics_unpack(ids, pk2, out=(v1, v0))
    assert got == (v1, v0)
    for pl, a, b in zip(pics, v1, v0):
        for v, pid in ((0, a), (1, b)):
            want, vp = want_view(pk2, pl, p, v, True)
            verify(eng, pid, vp, want, ("out=", v))
    spare = [eng.pic_alloc(p) for _ in ids]
    assert eng.pics_pack(v1, v0, pk2, out=spare) == spare
    for pl, pid in zip(pics, spare):                          # the lattice of the interpolated views is the packed picture again
        verify(eng, pid, p, pl, "packed into out=")
    # without out= the packed pictures are twice the views' coded size on the packed axis, with quincunx the views' size
    made = eng.pics_pack(v1, v0, pk2)
    q = eng._pic_params(made[0])
    assert (q.width, q.height) == (136, 72)
    verify(eng, made[1], p, pics[1], "packed into fresh pictures")
    hv = eng.pics_unpack(ids, E.make_packing("side_by_side"), False)
    q = eng._pic_params(eng.pics_pack(hv[0], hv[1], E.make_packing("side_by_side"))[0])
    assert (q.width, q.height) == (144, 72)                   # halves of 68 in views of 72 coded columns
    with pytest.raises(ValueError):
        eng.pics_unpack(ids, pk2, out=(v1[:1], v0))
    with pytest.raises(ValueError):
        eng.pics_pack(v1, v0[:1], pk2)
    eng.close()


def test_a_descriptor_parsed_from_bytes():
    """SEI bytes -> annexb.frame_packing -> packing_from_sei -> pics_unpack: side by side, frame 0 mirrored, frame 1 one full-resolution
    sample to the right of frame 0, frame 1 the left view"""
    import test_frame_packing_sei as S
    d = S.packing(3, cit=2, flags=("spatial_flipping", "frame0_flipped", "frame0_self_contained"), grid=((0, 5), (8, 5)), id=3)
    n = S.unit(S.packing(4, quincunx=True, id=1), d)
    read = A.frame_packing(n)
    assert read == d
    pk = E.packing_from_sei(read)
    assert (pk.arrangement, pk.quincunx, pk.flip, pk.grid, pk.views()) == (3, False, (True, False), ((0, 5), (8, 5)), (1, 0))
    rng = np.random.default_rng(45)
    eng = E.Engine(0)
    p = params(136, 72, 10, 1)
    pics = [content(k, p, rng) for k in ("noise", "ramp")]
    ids = [put(eng, p, pl) for pl in pics]
    check_unpack(eng, p, pk, True, pics, ids, "sei")
    check_unpack(eng, p, pk, False, pics, ids, "sei, halves")
    eng.close()


def test_argument_errors_write_nothing():
    """every OH_E_ARG and OH_E_UNSUPPORTED rule of ohevc_hip.h through the raw C calls: refused on the host, the destinations still
    hold what was uploaded and every picture keeps its checksum; n == 0 is fine"""
    eng = E.Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)
    uploaded = {}

    def some(p):
        pl = content("noise", p, rng)
        pid = put(eng, p, pl)
        uploaded[pid] = (p, pl)
        return pid

    def two(w, h, bd=10, cf=1):
        return [some(params(w, h, bd, cf)) for _ in range(2)]

    src = two(32, 16)
    half, half_b, full, full_b = two(16, 16), two(16, 16), two(32, 16), two(32, 16)
    tb_half = two(32, 8)
    other = two(24, 16)                                         # neither size
    bd8, cf3 = two(16, 16, 8), two(16, 16, 10, 3)
    odd = two(40, 24)
    odd422 = two(24, 8, 10, 2)
    w36 = [some(params(40, 16, 10, 1)) for _ in range(2)]
    watched = list(uploaded)

    def sums():
        return [eng.pics_hash([pid], 2) for pid in watched]

    before = sums()
    keep = []

    def ids_of(x):
        if x is None:
            return None
        a = (C.c_int * max(len(x), 1))(*x)
        keep.append(a)
        return a

    def desc(arr=3, quincunx=0, flip=(0, 0), gx=(0, 0), gy=(0, 0)):
        pk = E.OhPacking(arr, quincunx)
        for v in range(2):
            pk.flip[v], pk.grid_x[v], pk.grid_y[v] = flip[v], gx[v], gy[v]
        keep.append(pk)
        return pk

    def unpack(s=src, a=half, b=half_b, n=None, pk=None, e_null=False, pk_null=False):
        pk = desc() if pk is None else pk
        return L.oh_pics_unpack(None if e_null else eng.h, ids_of(s), ids_of(a), ids_of(b), len(s or a or b or []) if n is None else n,
                                None if pk_null else C.byref(pk))

    def pack(a=half, b=half_b, d=src, n=None, pk=None, e_null=False, pk_null=False):
        pk = desc() if pk is None else pk
        return L.oh_pics_pack(None if e_null else eng.h, ids_of(a), ids_of(b), ids_of(d), len(d or a or b or []) if n is None else n,
                              None if pk_null else C.byref(pk))

    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    # null arguments, a negative n
    assert unpack(e_null=True) == arg and unpack(pk_null=True) == arg and unpack(s=None, n=2) == arg and unpack(a=None, b=None, n=2) == arg
    assert unpack(n=-1) == arg and pack(n=-1) == arg
    assert pack(e_null=True) == arg and pack(pk_null=True) == arg and pack(a=None, n=2) == arg and pack(b=None, n=2) == arg and pack(d=None, n=2) == arg
    # the descriptor, with and without pictures
    for pk in (desc(arr=5), desc(arr=0), desc(arr=2), desc(quincunx=2), desc(flip=(0, 2)), desc(flip=(-1, 0)), desc(gx=(16, 0)), desc(gy=(0, -1))):
        assert unpack(pk=pk) == arg and pack(pk=pk) == arg
        assert unpack(s=[], a=[], b=[], n=0, pk=pk) == arg and pack(a=[], b=[], d=[], n=0, pk=pk) == arg
    # unknown pictures, params that differ on one side, a picture on both sides, a destination twice
    assert unpack(s=[src[0], 999]) == arg and unpack(a=[half[0], 999]) == arg and unpack(b=[-1, half_b[1]]) == arg
    assert unpack(s=[src[0], odd[0]]) == arg and unpack(a=[half[0], full[0]]) == arg and unpack(b=full) == arg
    assert unpack(a=[half[0], half[0]]) == arg and unpack(b=half) == arg and unpack(a=src, b=None) == arg
    assert pack(d=[src[0], src[0]]) == arg and pack(a=src, b=full, pk=desc(quincunx=1)) == arg and pack(b=[half_b[0], full[0]]) == arg
    # views of neither size.  (A half that is no whole number of chroma samples cannot reach the engine: a picture's sides are multiples
    # of the minimum coding block of 8; tests/test_packing_math_host.py has that refusal of oh_packing_view_size)
    assert unpack(a=other, b=None) == arg and pack(a=other, b=two(24, 16)) == arg
    assert unpack(a=tb_half, b=None) == arg and unpack(a=half, b=None, pk=desc(arr=4)) == arg           # the other arrangement's halves
    assert b"half size" in L.oh_engine_last_error(eng.h)
    assert pack(a=half, b=half_b, pk=desc(quincunx=1)) == arg                                           # quincunx packs full-size views
    # another bit depth or chroma format; full-size views without quincunx
    assert unpack(a=bd8, b=None) == uns and unpack(a=cf3, b=None) == uns and pack(a=bd8, b=two(16, 16, 8)) == uns
    assert pack(a=full, b=full_b) == uns
    assert b"oh_pics_resize" in L.oh_engine_last_error(eng.h)
    eng.sync()
    assert sums() == before, "a refused call wrote into a picture"
    for pid in half + half_b + full + full_b + src:
        verify(eng, pid, *uploaded[pid], "refused")
    # n == 0
    assert unpack(s=[], a=[], b=[], n=0) == 0 and unpack(s=None, a=None, b=half, n=0) == 0 and pack(a=None, b=None, d=None, n=0) == 0
    eng.sync()
    assert sums() == before
    # what is fine: 4:2:2 top-bottom at a height of 8, a width of 40, a source twice, one view
    assert unpack(s=odd422, a=two(24, 8, 10, 2), b=None, pk=desc(arr=4)) == 0
    assert unpack(s=w36, a=two(24, 16), b=two(24, 16)) == 0                                             # halves of 20 in views of 24
    assert unpack(s=[src[0], src[0]], a=None, b=half_b) == 0 and unpack(a=full, b=full_b, pk=desc(gx=(15, 15))) == 0
    assert pack(a=full, b=full_b, pk=desc(quincunx=1)) == 0
    eng.sync()
    p = params(32, 16, 10, 1)
    with pytest.raises(E.EngineError) as ei:
        eng.pics_pack(full, full_b, E.make_packing(3), out=[eng.pic_alloc(p), eng.pic_alloc(p)])
    assert ei.value.code == uns
    with pytest.raises(E.EngineError) as ei:
        eng.pics_unpack(src, E.make_packing(4), out=(half, None))
    assert ei.value.code == arg
    with pytest.raises(ValueError):
        eng.pics_unpack(src, "side_by_side")
    eng.close()
