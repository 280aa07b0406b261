"""The directed intra work lists of tests/directed_intra.py held against their own claims on the CPU: every family holds the
combinations it promises, the oracle's decision counters (oracle.h: OH_CNT_I_*) show that the branches the lists are there for are
reached, every list keeps the contract — and, where the reference is present, the checker equals the reference's own
hpc.intra_pred[] slots on every list of every family."""
import collections
import ctypes as C

import numpy as np
import pytest

import directed_intra as DI
from openhevc_amd import frame as F
from oracle_lib import have_ref_flags, host_pic_array, oracle, oracle_counters, plane_ptrs, ref_flags


def run_oracle(dl):
    pics = dl.pictures()
    assert oracle().oh_or_frame(C.byref(dl.frame), host_pic_array(pics)) == 0
    return pics[2]


def counters_over(lists):
    oracle_counters()
    for dl in lists:
        run_oracle(dl)
    return oracle_counters()["intra"]


def show(name, lists, cnt):
    print(f"{name}: {sum(len(dl.blks) for dl in lists)} blocks in {len(lists)} pictures; counters {dict(cnt)}")


SUBSTITUTION = ("sub_left", "sub_up_left", "sub_up", "sub_up_right", "sub_none", "fill_left", "fill_up_left", "fill_up", "fill_up_right")


@pytest.mark.parametrize("chroma,bd", DI.F_FULL + DI.F_CUT)
def test_matrix_holds_every_size_mode_flags_once(chroma, bd):
    lists = DI.build_f(chroma, bd)
    assert len({id(dl) for dl in lists}) == len(lists)
    got = collections.Counter(DI.f_triples(lists))
    want = DI.f_matrix(chroma, (chroma, bd) in DI.F_FULL)
    assert set(got) == set(want) and max(got.values()) == 1 and len(want) == len(set(want))
    for pt, sizes in ((0, (2, 3, 4, 5)), (1, DI.chroma_sizes(chroma))):
        for log2 in sizes:
            modes = set(range(35)) if (chroma, bd) in DI.F_FULL or log2 < 5 else set(DI.CUT_MODES_32)
            assert {(m, a) for t, l2, m, a in got if (t, l2) == (pt, log2)} == {(m, a) for m in modes for a in range(32)}
    assert all(dl.p.width <= DI.MAX_DIM and dl.p.height <= DI.MAX_DIM and DI.check_contract(dl) for dl in lists)
    assert all(DI.zscan_avail(dl.p, b.c, b.x, b.y, b.n) == DI.ALL5 for dl in lists for b in dl.blks if isinstance(b.tag, tuple))
    if chroma == 2:
        lower = [b for dl in lists for b in dl.blks if b.tag == "lower"]
        assert len(lower) == sum(t[0] for t in want) and all(b.avail & DI.U and not b.avail & DI.UR for b in lower)
    kinds = collections.Counter(b.tu.recipe.split(" ")[0] if b.tu is not None else "none" for dl in lists for b in dl.blks)
    assert min(kinds["none"], kinds["small"], kinds["DC"]) > len(want) // 4
    per_part = [len(DI.build_f(chroma, bd, k)) for k in range(DI.F_PARTS[(chroma, bd)])]
    assert max(per_part) <= 14, per_part
    cnt = counters_over(lists)
    show(f"F chroma {chroma} {bd} bit", lists, cnt)
    for k in SUBSTITUTION + ("filt_none", "filt_3tap", "dc_edge", "projected", "clip10_low", "clip10_high", "clip26_low", "clip26_high"):
        assert cnt[k] > 0, k


def saturating(b):
    """the block's residual drives every sample to 0 or to the maximum whatever was predicted (make_res kinds 2 .. 5)"""
    return b.tu is not None and b.tu.recipe.split(" ")[0] in ("DC", "bypass")


def test_every_triple_shows_its_prediction_in_some_format():
    """a saturating residual hides the prediction from the comparison: every (plane type, size, mode, flags) that two or more formats
    hold has a format in which its residual does not saturate, and on the oracle's picture that block is not constant there unless
    its prediction is (DC / planar / substituted edges may be); within a format two thirds of the matrix are visible"""
    seen, formats = collections.defaultdict(list), collections.Counter()
    for chroma, bd in DI.F_FULL + DI.F_CUT:
        lists = DI.build_f(chroma, bd)
        blks = [b for dl in lists for b in dl.blks if isinstance(b.tag, tuple)]
        assert 3 * sum(not saturating(b) for b in blks) >= 2 * len(blks) - 3
        for b in blks:
            seen[b.tag].append(not saturating(b))
    assert all(any(v) for v in seen.values() if len(v) >= 2)
    assert all(len(v) >= 2 for t, v in seen.items())         # every triple is in two formats or more
    # on the oracle: a visible angular block that gathers its row and its column from noise is not constant, a saturated one is
    n_vis = n_sat = 0
    for dl in DI.build_f(1, 8, 0):
        out = run_oracle(dl)
        for b in dl.blks:
            spread = np.ptp(out.planes[b.c][b.y:b.y + b.n, b.x:b.x + b.n])
            if saturating(b):
                n_sat += 1
                assert spread == 0, b
            elif b.mode >= 2 and b.avail & DI.U and b.avail & DI.L:
                n_vis += 1
                assert spread > 0, b
    assert n_vis > 50 and n_sat > 50


@pytest.mark.parametrize("family", ["G", "H", "K"])
def test_enumerated_families_carry_no_saturating_residual(family):
    """in G, H and K every combination is enumerated once: none of their blocks may hide its prediction behind the residual"""
    if family == "G":
        lists = [dl for cf, bd in DI.G_FORMATS for w in DI.G_KINDS for dl in DI.build_g(cf, bd, w)]
    elif family == "H":
        lists = [dl for bd in DI.H_DEPTHS for dl in [x for v in DI.H_VARIANTS for x in DI.build_h_thr(bd, v)] + DI.build_h_thr(bd, "strong", 3, 1) +
                 DI.build_h_thr(bd, "strong", 1, 1) + DI.build_h_clip(bd)]
    else:
        lists = DI.build_k8(8, 3) + DI.build_k8(8, 4) + [dl for cf, bd in DI.K_FORMATS for dl in DI.build_k_big(cf, bd) + DI.build_k_edge(cf, bd)]
    kinds = collections.Counter(b.tu.recipe if b.tu is not None else "none" for dl in lists for b in dl.blks)
    assert set(kinds) == {"none", "small random"} and min(kinds.values()) > sum(kinds.values()) // 4, kinds
    assert not any(saturating(b) for dl in lists for b in dl.blks)


@pytest.mark.parametrize("chroma,bd", DI.G_FORMATS)
def test_edge_lists_hold_every_cut(chroma, bd):
    lists = {what: DI.build_g(chroma, bd, what) for what in DI.G_KINDS}
    cuts = DI.g_cuts(lists["tr"] + lists["bl"])
    for c in ([0, 1] if chroma else [0]):
        for log2 in ((2, 3, 4, 5) if c == 0 else DI.chroma_sizes(chroma)):
            n = 1 << log2
            for what, values in (("tr", DI.cut_values(chroma, c, n)), ("bl", DI.cut_values_v(chroma, c, n))):
                assert cuts.get((what, log2, c), set()) == set(values), (what, log2, c)
                sub = 1 if c and (chroma == 1 or (chroma == 2 and what == "tr")) else 0
                assert set(values) == set(range(4 if sub else 8, n, 4 if sub else 8))      # every multiple of 4 a plane's size allows
    for what in ("tr", "bl"):
        for dl in lists[what]:
            pw, ph = F.plane_dims(dl.p, dl.blks[0].c)
            for b in dl.blks:
                assert ((pw - b.x - b.n) if what == "tr" else (ph - b.y - b.n)) == b.edge[2] and b.avail & (DI.UR if what == "tr" else DI.BL)
        modes = {b.mode for dl in lists[what] for b in dl.blks}
        # a run is cut inside an 8x8 block only in a subsampled plane (the slot path); 16x16 and 32x32 take a wave each
        assert modes == set(DI.G_MODES) and {b.log2 for dl in lists[what] for b in dl.blks} >= \
            ({3, 4, 5} if chroma == 1 or (chroma == 2 and what == "tr") else {4, 5})
    # x = 0 / y = 0: every subset of what the position allows, with every mode
    at_x0 = {(b.c > 0, b.log2, b.mode, b.avail) for dl in lists["origin"] for b in dl.blks if b.x == 0 and b.y > 0}
    at_y0 = {(b.c > 0, b.log2, b.mode, b.avail) for dl in lists["origin"] for b in dl.blks if b.y == 0 and b.x > 0}
    for c in ([0, 1] if chroma else [0]):
        for log2 in ((2, 3, 4, 5) if c == 0 else DI.chroma_sizes(chroma)):
            assert {(bool(c), log2, m, a) for m in DI.G_MODES for a in (0, DI.U, DI.UR, DI.U | DI.UR)} <= at_x0
            assert {(bool(c), log2, m, a) for m in DI.G_MODES for a in (0, DI.L, DI.BL, DI.L | DI.BL)} <= at_y0
    assert {(dl.p.width, dl.p.height) for dl in lists["tiny"]} == {(8, 8), (16, 8), (8, 16)}
    every = [dl for ls in lists.values() for dl in ls]
    assert any(dl.p.width % 16 == 8 for dl in every) and any(dl.p.height % 16 == 8 for dl in every)
    assert all(DI.check_contract(dl) for dl in every)
    cnt = counters_over(every)
    show(f"G chroma {chroma} {bd} bit", every, cnt)
    assert cnt["tr_partial"] >= sum(len(dl.blks) for dl in lists["tr"]) and cnt["bl_partial"] >= sum(len(dl.blks) for dl in lists["bl"])
    assert cnt["projected"] > 0 and cnt["sub_none"] > 0


@pytest.mark.parametrize("bd", DI.H_DEPTHS)
def test_threshold_lists_sit_on_the_limit(bd):
    lim = 1 << (bd - 5)
    strong, plain, off = (DI.build_h_thr(bd, v) for v in ("strong", "plain", "disabled"))
    want_pairs = {(t, l) for t in (lim - 1, lim, lim + 1) for l in (lim - 1, lim, lim + 1)}
    per_flags, signs = collections.defaultdict(set), set()
    outcome = collections.Counter()
    for dl in strong:
        for b in dl.blks:
            t, l, st, sl = DI.h_measure(dl, b)               # from the samples of the picture, not from what the builder meant
            per_flags[b.avail].add((t, l))
            signs |= {("t", st), ("l", sl)}
            outcome["tl_" + "pf"[t >= lim] + "pf"[l >= lim]] += 1
        assert DI.check_contract(dl)
    assert set(per_flags) == set(DI.H_FLAGS) and all(s == want_pairs for s in per_flags.values())
    assert signs == {("t", 1), ("t", -1), ("l", 1), ("l", -1)}
    for lists, reached in ((strong, True), (plain, True), (off, False)):
        cnt = counters_over(lists)
        show(f"H thresholds {bd} bit {lists[0].name.split(' ')[-5]}", lists, cnt)
        for k in ("tl_pp", "tl_pf", "tl_fp", "tl_ff"):
            assert cnt[k] == (outcome[k] if reached else 0), (k, cnt[k], outcome[k])
        assert cnt["filt_strong"] == (outcome["tl_pp"] if lists is strong else 0)
        assert cnt["filt_none"] == (0 if reached else 72)
    # no block's output is constant: the prediction, and with it the smoothing decision, shows in the picture
    for dl in strong + plain + off:
        out = run_oracle(dl)
        assert all(np.ptp(out.planes[b.c][b.y:b.y + b.n, b.x:b.x + b.n]) > 0 for b in dl.blks), dl.name
    # strong_intra_smoothing matters on exactly the blocks with t < lim and l < lim
    for a, b_ in zip(strong, plain):
        pa, pb = run_oracle(a), run_oracle(b_)
        assert pa.equal(run_oracle(a))
        for b in a.blks:
            t, l, _, _ = DI.h_measure(a, b)
            same = np.array_equal(pa.planes[0][b.y:b.y + 32, b.x:b.x + 32], pb.planes[0][b.y:b.y + 32, b.x:b.x + 32])
            assert same == (not (t < lim and l < lim)), (a.name, b)
        cover = np.zeros(pa.planes[0].shape, bool)
        for b in a.blks:
            cover[b.y:b.y + 32, b.x:b.x + 32] = True
        assert np.array_equal(pa.planes[0][~cover], pb.planes[0][~cover]) and all(np.array_equal(pa.planes[c], pb.planes[c]) for c in (1, 2))
    # the same neighbourhoods in chroma: 3-tap only in 4:4:4, no smoothing in 4:2:0
    c444, c420 = DI.build_h_thr(bd, "strong", 3, 1), DI.build_h_thr(bd, "strong", 1, 1)
    cnt = counters_over(c444)
    assert cnt["filt_3tap"] == 72 and cnt["filt_strong"] == 0
    cnt = counters_over(c420)
    assert cnt["filt_none"] == 72
    for dl in c444 + c420:
        assert {DI.h_measure(dl, b)[:2] for b in dl.blks} == want_pairs


@pytest.mark.parametrize("bd", DI.H_DEPTHS)
def test_clip_lists_reach_both_ends(bd):
    lists = DI.build_h_clip(bd)
    assert collections.Counter((b.log2, b.mode, b.edge) for dl in lists for b in dl.blks) == \
        collections.Counter((l2, m, arr) for l2 in (2, 3, 4) for m in (1, 10, 26) for arr in range(8))
    cnt = counters_over(lists)
    show(f"H clip {bd} bit", lists, cnt)
    for k in ("clip10_low", "clip10_high", "clip10_none", "clip26_low", "clip26_high", "clip26_none", "dc_edge"):
        assert cnt[k] > 0, k
    # low: edge 0, other edge 0, corner max; high: edge max, other edge max, corner 0 -> one arrangement each, n samples: 4 + 8 + 16
    assert cnt["clip26_low"] == cnt["clip10_low"] == cnt["clip26_high"] == cnt["clip10_high"] == 28
    assert all(DI.check_contract(dl) for dl in lists)


def test_occupancy_lists_hold_the_stated_counts():
    seen, mixed, geometries = set(), 0, set()
    for chroma, bd in DI.J_FORMATS:
        lists = DI.build_j(chroma, bd)
        for dl in lists:
            assert DI.check_contract(dl)
            lc = dl.p.log2_ctb_size
            geometries.add((lc, dl.p.width >> lc, dl.p.height >> lc))
            cover = [np.zeros(F.plane_dims(dl.p, c)[::-1], np.int32) for c in range(3)]
            for b in dl.blks:
                cover[b.c][b.y:b.y + b.n, b.x:b.x + b.n] += 1
                assert b.avail == DI.zscan_avail(dl.p, b.c, b.x, b.y, b.n)       # true flags
            assert all((cv == 1).all() for cv in cover)                           # fully covered, once
            for _, _, small, large in DI.occupancy(dl):
                seen.add(small)
                mixed += bool(small and large)
            assert dl.frame.n_levels >= (dl.p.width >> lc)                       # the CTUs of a row wait for each other
        kinds = collections.Counter(b.tu.recipe.split(" ")[0] if b.tu is not None else "none" for dl in lists for b in dl.blks)
        assert kinds["bypass"] > sum(kinds.values()) // 4 and {b.mode for dl in lists for b in dl.blks} == set(DI.J_MODES)
        cnt = counters_over(lists)
        show(f"J chroma {chroma} {bd} bit", lists, cnt)
    assert set(DI.J_OCCUPANCY) <= seen, sorted(seen)
    assert mixed >= 20
    assert geometries == {(lc, w, h) for lc in (4, 5, 6) for w, h in ((1, 1), (4, 1), (3, 3))}


# cip_top_start is left out: with realisable flags it cannot happen.  A left-side flag survives the re-derivation only if a cell of
# its run is intra, and a block that is not aligned to the min-PU grid (no re-derivation) has its own, intra, PU to its left.
CIP = ("cip_no_left", "cip_x0_zero", "cip_up_sweep", "cip_corner", "cip_flag_cleared")


def test_cip_lists_hold_every_mask():
    k8 = DI.build_k8(8, 3)
    full = collections.Counter(b.mask for dl in k8 for b in dl.blks if b.avail == DI.ALL5)
    assert set(full) == set(range(512)) and max(full.values()) == 1
    for s in DI.K_SUBSETS:
        assert len({b.mask for dl in k8 for b in dl.blks if b.avail == s}) == 128
    assert {b.mode for dl in k8 for b in dl.blks} == set(DI.K_MODES)
    for dl in k8[:3]:                                         # the map says what the mask says
        m = dl.is_intra
        for b in dl.blks:
            for i, (X, Y, w, h) in enumerate(DI.k_groups(dl.p, b)):
                assert m[Y >> 2, X >> 2] == (b.mask >> i) & 1, (b, i)
    k8b = DI.build_k8(8, 4)
    assert k8b[0].p.log2_min_pu_size == 3 and k8[0].p.log2_min_pu_size == 2
    every = k8 + k8b
    for chroma, bd in DI.K_FORMATS:
        big, edge = DI.build_k_big(chroma, bd), DI.build_k_edge(chroma, bd)
        assert {(b.c > 0, b.log2) for dl in big for b in dl.blks} == {(False, 4), (False, 5), (True, 2), (True, 3), (True, 4)}
        assert any(b.x == 0 and b.y > 0 for dl in edge for b in dl.blks) and any(b.y == 0 and b.x > 0 for dl in edge for b in dl.blks)
        every += big + edge
    assert all(dl.p.constrained_intra_pred and DI.check_contract(dl) for dl in every)
    for name, lists in (("K 8x8", k8), ("K all", every)):
        cnt = counters_over(lists)
        show(name, lists, cnt)
        for k in CIP:
            assert cnt[k] > 0 or (k == "cip_x0_zero" and lists is k8), k
        assert cnt["cip_top_start"] == 0


def test_a_wrong_flag_and_a_race_are_caught():
    """the contract checker itself: an unrealisable flag, a read of a block recorded later and an overlap are refused"""
    p = DI.params(64, 64, 1, 8)
    for blks in ([DI.Blk(0, 3, 2, DI.UR, x=8, y=8)],                       # up-right of the bottom-right quarter follows it
                 [DI.Blk(0, 3, 2, DI.L, x=8, y=0), DI.Blk(0, 3, 2, 0, x=0, y=0)],
                 [DI.Blk(0, 3, 2, 0, x=8, y=8), DI.Blk(0, 4, 2, 0, x=0, y=0)]):
        with pytest.raises(AssertionError):
            DI.record_intra("bad", p, blks, seed=1)
    assert DI.zscan_avail(p, 0, 8, 8, 8) == DI.L | DI.UL | DI.U and DI.zscan_avail(p, 0, 0, 8, 8) == DI.U | DI.UR
    assert DI.zscan_avail(p, 0, 32, 32, 32) == DI.L | DI.UL | DI.U and DI.zscan_avail(p, 1, 4, 4, 4) == DI.L | DI.UL | DI.U


def test_zscan_avail_equals_the_recorder_on_fully_recorded_pictures():
    """on a picture that is covered in decode order, "precedes in z-scan and inside the picture" (zscan_avail) is what the recorder's
    map of recorded blocks gives (oh_rec_avail): every block of every J list"""
    lib = F.host()
    n = 0
    for chroma, bd in DI.J_FORMATS:
        for dl in DI.build_j(chroma, bd):
            rec = F.Recorder(dl.p)
            lib.oh_rec_begin(rec.h, 2, (C.c_int32 * F.OH_MAX_REFS)(*([-1] * F.OH_MAX_REFS)), F.OH_MAX_REFS)
            for b in dl.blks:
                rect = DI.luma_rect(dl.p, b.c, b.x, b.y, b.n)
                assert lib.oh_rec_avail(rec.h, *rect) == DI.zscan_avail(dl.p, b.c, b.x, b.y, b.n), (dl.name, b)
                lib.oh_rec_mark_decoded(rec.h, *rect)
                n += 1
            rec.close()
    assert n > 10000


def ref_lists():
    out = [(f"F-{cf}-{bd}", lambda cf=cf, bd=bd: DI.build_f(cf, bd)) for cf, bd in DI.F_FULL + DI.F_CUT]
    out += [(f"G-{cf}-{bd}", lambda cf=cf, bd=bd: [dl for w in DI.G_KINDS for dl in DI.build_g(cf, bd, w)]) for cf, bd in DI.G_FORMATS]
    out += [(f"H-{bd}", lambda bd=bd: [dl for v in DI.H_VARIANTS for dl in DI.build_h_thr(bd, v)] + DI.build_h_thr(bd, "strong", 3, 1) +
             DI.build_h_thr(bd, "strong", 1, 1) + DI.build_h_clip(bd)) for bd in DI.H_DEPTHS]
    out += [(f"J-{cf}-{bd}", lambda cf=cf, bd=bd: DI.build_j(cf, bd)) for cf, bd in DI.J_FORMATS]
    out += [("K-8x8", lambda: DI.build_k8(8, 3) + DI.build_k8(8, 4))]
    out += [(f"K-{cf}-{bd}", lambda cf=cf, bd=bd: DI.build_k_big(cf, bd) + DI.build_k_edge(cf, bd)) for cf, bd in DI.K_FORMATS]
    return out


def ref_run(dl):
    """the list through the reference's kernels (oracle/ref_harness.c::ref_frame: blocks re-sorted into decode order, intra_pred[]
    slots, residual added after each block), the candidate flags taken from the items"""
    pics = dl.pictures()
    cur = pics[2]
    d, s = plane_ptrs(cur)
    d2, _ = plane_ptrs(cur.copy())
    refs = ((C.c_void_p * 3) * 2)()
    for i in range(2):
        for c, pl in enumerate(pics[i].planes):
            refs[i][c] = pl.ctypes.data
    ref_flags().ref_set_item_flags(1)
    assert ref_flags().ref_frame(C.byref(dl.frame), d, s, C.cast(refs, C.c_void_p), 2, s, d2) == 0
    return cur


@pytest.mark.skipif(not have_ref_flags(), reason="reference tree / oracle/_ref/libohevc_ref_flags.so not present")
@pytest.mark.parametrize("name,build", ref_lists(), ids=[n for n, _ in ref_lists()])
def test_checker_equals_the_reference_slots(name, build):
    from test_gpu_directed import assert_same_named
    n = 0
    for dl in build():
        assert_same_named(dl, ref_run(dl), run_oracle(dl))
        n += 1
    assert n
