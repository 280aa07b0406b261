"""GPU parity (-m gpu) of the SAO pass on DIRECTED parameters: the work lists are the synthetic generator's (or hold no block at all),
but every OhSaoCtb entry is overwritten, so that each edge class meets each edge_flags value, each band position occurs, every mix of
types per plane occurs and every width of a row group (1, 2, 4, 8 lanes of sao_kernel share a picture row) is run — with content on
which SAO really changes samples.  The expected picture is the CPU oracle's (pinned to the reference in tests/test_oracle_*.py).

Every case first proves on the oracle's result alone that it is not vacuous: the picture filtered with the directed entries is compared
with the picture of the same list with SAO off, and at least 90 % of the CTBs with a type, in every plane, must hold a changed sample.  The seeds of the synthetic pictures are ones for which the oracle meets this (found on the CPU)."""
import ctypes as C

import numpy as np
import pytest

from openhevc_amd import frame as F
from oracle_lib import host_pic_array, oracle
from test_gpu_parity import assert_same, run_both

pytestmark = pytest.mark.gpu

SAO_DT = np.dtype([("offset_val", "<i2", (3, 5)), ("band_position", "u1", (3,)), ("eo_class", "u1", (3,)), ("type_idx", "u1", (3,)), ("edge_flags", "u1")])
assert SAO_DT.itemsize == C.sizeof(F.OhSaoCtb)


@pytest.fixture(scope="module")
def eng():
    from openhevc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def offset_limit(bd):
    """largest SaoOffsetVal magnitude of the bit depth (7.4.9.3.2 with log2_sao_offset_scale at its maximum)"""
    return ((1 << (min(bd, 10) - 5)) - 1) << (bd - min(bd, 10))


class Directed:
    """a deep copy of a work list whose SAO entries are this object's numpy records (.sao, raster order of CTBs)"""

    def __init__(self, f):
        self.fc = F.FrameCopy(f)
        self.p = p = self.fc.frame.p
        lc = p.log2_ctb_size
        self.ctbw, self.ctbh = (p.width + (1 << lc) - 1) >> lc, (p.height + (1 << lc) - 1) >> lc
        self.sao = np.zeros(self.ctbw * self.ctbh, SAO_DT)
        self.fc.frame.sao = C.cast(self.sao.ctypes.data, C.POINTER(F.OhSaoCtb))
        self.frame = self.fc.frame

    def offsets(self, rng, i, c, mag=None):
        """four non-zero offsets, signs drawn, magnitudes up to the bit depth's limit (`mag`: all at that magnitude)"""
        lim = offset_limit(self.p.bit_depth)
        m = rng.integers(1, lim + 1, 4) if mag is None else np.full(4, mag)
        self.sao["offset_val"][i, c, 1:] = m * rng.choice([-1, 1], 4)

    def ctb_rect(self, i, c):
        lc, hs, vs = self.p.log2_ctb_size, F.hshift(self.p, c), F.vshift(self.p, c)
        pw, ph = F.plane_dims(self.p, c)
        x0, y0 = ((i % self.ctbw) << lc) >> hs, ((i // self.ctbw) << lc) >> vs
        return x0, y0, min(x0 + ((1 << lc) >> hs), pw), min(y0 + ((1 << lc) >> vs), ph)


def empty_list(p):
    """a work list without any block: the picture passes through the in-loop filters as it was uploaded"""
    rec = F.Recorder(p)
    refs = (C.c_int32 * F.OH_MAX_REFS)(*([0, 1] + [-1] * (F.OH_MAX_REFS - 2)))
    F.host().oh_rec_begin(rec.h, 2, refs, F.OH_MAX_REFS)
    d = Directed(F.host().oh_rec_finish(rec.h).contents)
    rec.close()
    return d


def synth_list(p, st, seed, **knobs):
    rec = F.Recorder(p)
    d = Directed(rec.synth(F.synth_params(st, seed, **knobs), 2, [0, 1]))
    rec.close()
    return d


def noise_pics(p, seed, amp=3, clip_rows=False, full_range=False):
    """the pictures of one case: the current one holds noise of +-amp levels around mid-grey, so that local minima, maxima, both kinds
    of corners and flat runs (the five edge categories) all occur.  clip_rows: some rows lie at 0 and some at the maximum, so that
    the clip to the sample range acts.  full_range: uniform samples (every band occurs, and the clip acts at both ends)."""
    rng = np.random.default_rng(seed)
    pics = {0: F.HostPic(p), 1: F.HostPic(p), 2: F.HostPic(p)}
    mx = (1 << p.bit_depth) - 1
    for c, pl in enumerate(pics[2].planes):
        if full_range:
            a = rng.integers(0, mx + 1, pl.shape)
            a[rng.integers(0, 8, pl.shape) == 0] = 0
            a[rng.integers(0, 8, pl.shape) == 0] = mx
        else:
            a = (1 << (p.bit_depth - 1)) + rng.integers(-amp, amp + 1, pl.shape)
            if clip_rows:
                a[3::11] = 0
                a[7::11] = mx
        pl[...] = a.astype(pl.dtype)
    return pics


def oracle_picture(frame, pics):
    got = {k: v.copy() for k, v in pics.items()}
    assert oracle().oh_or_frame(C.byref(frame), host_pic_array(got)) == 0
    return got[frame.cur_pic]


def assert_not_vacuous(d, pics, want, tag, classes=False):
    """on the oracle's pictures alone: with the directed entries (`want`) against the same list with SAO off everywhere"""
    types = d.sao["type_idx"].copy()
    d.sao["type_idx"][...] = 0
    before = oracle_picture(d.frame, pics)
    d.sao["type_idx"][...] = types
    sides = {k: set() for k in range(4)}                    # per edge class: the CTB sides (first / last row / column) with a changed sample
    for c in range(len(want.planes)):
        chg = before.visible(c) != want.visible(c)
        on = hit = 0
        for i in range(len(d.sao)):
            x0, y0, x1, y1 = d.ctb_rect(i, c)
            if types[i, c] == 0:
                assert not chg[y0:y1, x0:x1].any(), f"{tag}: plane {c} CTB {i} has no type and changed"
                continue
            t = chg[y0:y1, x0:x1]
            on += 1
            hit += bool(t.any())
            if types[i, c] == 2:
                k = int(d.sao["eo_class"][i, c])
                sides[k] |= {s for s, m in (("top", t[0]), ("bottom", t[-1]), ("left", t[:, 0]), ("right", t[:, -1])) if m.any()}
        assert on == 0 or hit >= 0.9 * on, f"{tag}: plane {c}: SAO changed samples in only {hit} of {on} CTBs with a type"
    if classes:
        for k in range(4):
            assert sides[k] == {"top", "bottom", "left", "right"}, f"{tag}: class {k} changed samples only on the sides {sorted(sides[k])} of its CTBs"


def check(eng, d, pics, tag, classes=False):
    want, got = run_both(eng, d.p, d.frame, pics)
    assert_not_vacuous(d, pics, want, tag, classes)
    assert_same(want, got, tag)


# ---- every eo_class x every edge_flags value ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("rot", [0, 17])
def test_every_class_meets_every_edge_flags_value(eng, bd, rot):
    """4:4:4, 16x16 CTBs (not the stale-column configuration), 512x504: 32 x 32 CTBs, the last row partial.  CTB i holds pair number
    (i + rot) % 1024 of (class, flags); with rot = 17 the pairs stand on other CTBs, those on the picture's borders included.  The
    chroma planes hold the pairs of other classes."""
    p = F.pic_params(512, 504, bit_depth=bd, chroma_format_idc=3, log2_ctb_size=4)
    d = empty_list(p)
    assert len(d.sao) == 1024
    rng = np.random.default_rng(100 + rot + bd)
    for i in range(1024):
        k = (i + rot) % 1024
        d.sao["edge_flags"][i] = k & 255
        for c in range(3):
            d.sao["type_idx"][i, c] = 2
            d.sao["eo_class"][i, c] = ((k >> 8) + c) & 3
            d.offsets(rng, i, c)
    for c in range(3):
        assert len({(int(s["eo_class"][c]), int(s["edge_flags"])) for s in d.sao}) == 1024
    check(eng, d, noise_pics(p, 7 + rot, clip_rows=bd == 10), f"class x flags, {bd} bit, rotated by {rot}", classes=True)


# ---- row groups of 1, 2, 4 and 8 lanes ----------------------------------------------------------------------------------------
FLAG_SET = [0, 0, 1, 2, 4, 8, 0x10, 0x20, 0x40, 0x80, 0x0f, 0xf0, 0xff, 0x35, 0xca, 0]


def direct_mixed(d, seed, band_position=None):
    """mostly edge CTBs of rotating classes, a band and an off CTB in between; flags from FLAG_SET and drawn"""
    rng = np.random.default_rng(seed)
    mid_band = 15                                          # bands 15..18 hold mid-grey and what lies a few levels around it
    for i in range(len(d.sao)):
        d.sao["edge_flags"][i] = FLAG_SET[i % len(FLAG_SET)] if i % 3 else rng.integers(0, 256)
        for c in range(3):
            t = (2, 2, 1, 2, 2, 0, 2)[(i + 2 * c) % 7]
            d.sao["type_idx"][i, c] = t
            d.sao["eo_class"][i, c] = (i + c + i // d.ctbw) & 3
            d.sao["band_position"][i, c] = mid_band if band_position is None else band_position
            d.offsets(rng, i, c)


GROUP_CASES = [(w, h, lc, chroma, bd) for (w, h) in ((136, 88),) for lc in (4, 5, 6) for chroma in (0, 1, 2, 3) for bd in ((8, 10)[(lc + chroma) & 1],)] + [
    (264, 200, 5, 1, 8), (264, 200, 6, 2, 10), (264, 200, 4, 3, 10),
    (8, 8, 4, 3, 8), (24, 24, 5, 1, 8), (40, 56, 6, 2, 10),                    # a single CTB
    (136, 24, 5, 1, 10), (264, 16, 4, 2, 8), (200, 64, 6, 3, 8),               # one row of CTBs
    (24, 88, 4, 1, 8), (24, 200, 5, 2, 10), (56, 200, 6, 1, 8),                # one column of CTBs
]


@pytest.mark.parametrize("w,h,lc,chroma,bd", GROUP_CASES)
def test_row_groups_of_every_width(eng, w, h, lc, chroma, bd):
    """CTB widths of 8, 16, 32 and 64 samples in some plane: 1, 2, 4 and 8 lanes share a row and hand each other the columns x - 1 and
    x + 8.  Luma widths are 8 mod 16, so a subsampled plane ends inside a lane's eight samples.  Deblocking is on (all strengths 0)."""
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc)
    d = empty_list(p)
    direct_mixed(d, w + h + lc)
    check(eng, d, noise_pics(p, lc * 10 + chroma, clip_rows=bool(chroma & 1)), f"{w}x{h} ctb {1 << lc} chroma {chroma} {bd} bit")


@pytest.mark.parametrize("w,h,chroma,bd,st,seed", [(136, 88, 1, 8, 0, 691), (264, 200, 2, 10, 0, 819), (200, 136, 1, 10, 2, 755), (96, 16, 2, 8, 0, 2001), (96, 32, 1, 8, 0, 651)])
def test_stale_columns_with_directed_flags(eng, w, h, chroma, bd, st, seed):
    """16x16 CTBs with subsampled chroma on pictures whose chroma edges deblocking really filters (intra blocks): the column x + 8 of a
    chroma CTB is read as the reference's driver saw it, here under directed classes and flags"""
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=4)
    d = synth_list(p, st, seed, intra_pct=40)
    direct_mixed(d, w + h)
    for i in range(len(d.sao)):                             # edge everywhere in chroma
        d.sao["type_idx"][i, 1:] = 2
    rng = np.random.default_rng(w)
    pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
    check(eng, d, pics, f"stale columns {w}x{h} chroma {chroma} {bd} bit")


# ---- band ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd,chroma,lc", [(8, 1, 4), (10, 3, 4), (12, 2, 5), (10, 1, 6)])
def test_every_band_position(eng, bd, chroma, lc):
    """band_position 0..31 in every plane (29..31 wrap around to bands 0..2), all four offsets at the bit depth's limit with both
    signs, on full-range content with samples at 0 and at the maximum: the clip acts at both ends"""
    w, h = (136, 88) if lc == 4 else (264, 200) if lc == 5 else (520, 264)
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc)
    d = empty_list(p)
    assert len(d.sao) >= 32
    rng = np.random.default_rng(bd)
    for i in range(len(d.sao)):
        for c in range(3):
            d.sao["type_idx"][i, c] = 1
            d.sao["band_position"][i, c] = (i + 11 * c) & 31
            d.offsets(rng, i, c, mag=offset_limit(bd))
    for c in range(F.n_planes(p)):
        assert set(d.sao["band_position"][:, c]) == set(range(32))
    check(eng, d, noise_pics(p, bd, full_range=True), f"band positions, {bd} bit")


# ---- the nine mixes of types per plane ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,lc,chroma,bd", [(264, 200, 5, 1, 10), (136, 88, 4, 2, 8), (264, 200, 6, 3, 8)])
def test_types_are_per_plane(eng, w, h, lc, chroma, bd):
    """luma off with chroma edge, luma band with chroma off, ... : CTB i holds mix i % 9 of (luma type, chroma type); an off plane is
    copied, whatever the other planes of the CTB do"""
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc)
    d = empty_list(p)
    direct_mixed(d, w)
    assert len(d.sao) >= 9
    for i in range(len(d.sao)):
        d.sao["type_idx"][i, 0] = (i % 9) // 3
        d.sao["type_idx"][i, 1:] = (i % 9) % 3
    check(eng, d, noise_pics(p, w + lc), f"type mixes {w}x{h} chroma {chroma}")


# ---- PCM / bypass restore -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,lc,chroma,bd,seed", [(200, 136, 6, 2, 8, 2000), (200, 136, 5, 2, 10, 1105), (264, 200, 5, 1, 10, 1169), (136, 88, 4, 3, 8, 2018)])
def test_pcm_and_bypass_samples_are_restored(eng, w, h, lc, chroma, bd, seed):
    """pcm_loop_filter_disable and transquant_bypass_enable with is_pcm set: the samples of those blocks are put back after SAO in
    CTBs of every type (4:2:2 included, whose row-copy length is the quirk described in sao.hip)"""
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc, pcm_loop_filter_disable=1, transquant_bypass_enable=1)
    d = synth_list(p, 2, seed, pcm_pct=15, bypass_pct=15, intra_pct=30)
    assert d.frame.is_pcm and np.frombuffer(C.string_at(d.frame.is_pcm, (w >> p.log2_min_pu_size) * (h >> p.log2_min_pu_size)), np.uint8).any()
    direct_mixed(d, h, band_position=None)
    rng = np.random.default_rng(lc)
    for i in range(len(d.sao)):                             # full-range content: bands all over
        d.sao["band_position"][i] = rng.integers(0, 32, 3)
        d.sao["type_idx"][i] = (i % 3, (i + 1) % 3, (i + 2) % 3)
    pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
    check(eng, d, pics, f"pcm / bypass {w}x{h} chroma {chroma}")


# ---- a batch ------------------------------------------------------------------------------------------------------------------
def test_batch_with_and_without_sao_parameters(eng):
    """oh_frames_execute on four pictures of one geometry (16x16 CTBs, 4:2:0) with different SAO entries: one has no SAO parameters
    at all (the engine runs it in a sub-batch that skips the pass), one was decoded in tile scan (OhFrame.sao_pending)"""
    from openhevc_amd.engine import remap_frame
    p = F.pic_params(136, 88, bit_depth=8, chroma_format_idc=1, log2_ctb_size=4)
    rng = np.random.default_rng(3)
    refs = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng)}
    ids = {k: eng.pic_alloc(p) for k in refs}
    for k, hp in refs.items():
        eng.pic_upload(ids[k], hp)
    ds, want, curs, dfs = [], [], [], []
    for n in range(4):
        d = synth_list(p, 0 if n & 1 else 2, 1200 + n, intra_pct=40)
        direct_mixed(d, 77 * n)
        if n == 1:
            d.frame.sao = C.cast(None, C.POINTER(F.OhSaoCtb))
        if n == 2:                                          # 3 x 2 tiles: the filter calls follow the tile scan
            tid = (C.c_int32 * len(d.sao))(*[(i // d.ctbw >= 3) * 3 + min(i % d.ctbw // 3, 2) for i in range(len(d.sao))])
            d.pending = np.zeros(len(d.sao), np.uint8)
            H = F.host()
            H.oh_sao_pending_driver.argtypes = [C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_uint8)]
            H.oh_sao_pending_driver(tid, d.ctbw, d.ctbh, d.pending.ctypes.data_as(C.POINTER(C.c_uint8)))
            d.frame.sao_pending = d.pending.ctypes.data_as(C.POINTER(C.c_uint8))
        cur = F.HostPic(p, rng=rng)
        want.append(oracle_picture(d.frame, {0: refs[0], 1: refs[1], 2: cur}))
        cid = eng.pic_alloc(p)
        eng.pic_upload(cid, cur)
        curs.append(cid)
        ds.append(d)
        dfs.append(eng.frame_upload(remap_frame(d.frame, {0: ids[0], 1: ids[1], 2: cid})))
    assert ds[2].pending.any() and not want[0].equal(want[2])
    eng.frames_execute(dfs)
    eng.sync()
    for n in range(4):
        assert_same(want[n], eng.pic_download(curs[n], p), f"batched picture {n}")
    for df in dfs:
        eng.frame_free(df)
    for v in list(ids.values()) + curs:
        eng.pic_free(v)
