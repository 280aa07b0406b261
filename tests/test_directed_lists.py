"""The directed work lists of tests/directed.py held against their own claims on the CPU: the numpy transform model equals the
checker on every residual block, the residual set reaches the clips it is there for, the inter families hold every combination
they promise, the graded weights leave the output in range — and, where the reference is present, the checker's inter pass equals
a composition of the reference's own slots PU by PU on the A, B and C lists."""
import ctypes as C

import numpy as np
import pytest

import directed as D
from openhevc_amd import frame as F
from oracle_lib import have_ref, host_pic_array, i16p, oracle, ref


def oracle_idct(b, bd, dst=False):
    a = np.ascontiguousarray(b, dtype=np.int16).copy()
    if dst:
        oracle().oh_or_idct_4x4_luma(bd, i16p(a))
    else:
        oracle().oh_or_idct(bd, i16p(a), int(np.log2(a.shape[0])))
    return a


def pixels(pred, res, bd):
    return np.clip(pred + res, 0, (1 << bd) - 1)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_transform_model_equals_the_checker_on_every_block(bd):
    for n in (4, 8, 16, 32):
        for dst in ((False, True) if n == 4 else (False,)):
            for recipe, b in D.e_blocks(n, bd, dst):
                r, _, _ = D.idct_model(b, bd, dst)
                assert np.array_equal(r, oracle_idct(b, bd, dst)), (bd, n, dst, recipe)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_residual_set_reaches_the_clips(bd, n):
    """per (bit depth, size): a dense block shows a missing first clip in the final picture, the sign-aligned blocks hit the first
    clip, and the second clip is hit exactly in the cells where it can be; there, wrapping the kept residual instead of clipping it
    changes the intra picture (DC prediction without neighbours = mid grey)"""
    blocks = D.e_blocks(n, bd)
    mid = 1 << (bd - 1)
    e1 = [b for r, b in blocks if r.startswith("e1")]
    e2 = [b for r, b in blocks if r.startswith("e2")]
    assert len(e1) >= 8 and len(e2) == 16
    changed = sum(not np.array_equal(pixels(mid, D.idct_model(b, bd)[0], bd), pixels(mid, D.idct_model(b, bd, clip1=False)[0], bd)) for b in e1)
    hits1 = sum(D.idct_model(b, bd)[1] for b in e2)
    hits2 = sum(D.idct_model(b, bd)[2] for b in e2)
    print(f"{bd} bit {n}x{n}: first clip removed changes {changed}/{len(e1)} e1 pictures; e2 first-clip hits {hits1}, second-clip hits {hits2}")
    assert changed >= 1
    assert hits1 > 0
    if (bd, n) in D.SECOND_CLIP_CELLS:
        assert hits2 > 0
        wrapped = sum(not np.array_equal(pixels(mid, D.idct_model(b, bd)[0], bd), pixels(mid, D.wrap16(D.idct_model(b, bd, clip2=False)[0]), bd))
                      for b in e2)
        print(f"{bd} bit {n}x{n}: wrapping the kept residual changes {wrapped}/{len(e2)} e2 intra pictures")
        assert wrapped >= 1
    else:
        assert hits2 == 0


@pytest.mark.parametrize("chroma,bd", D.E_FORMATS)
def test_residual_lists_hold_every_block_twice(chroma, bd):
    lists = D.build_e(chroma, bd)
    tus = [t for dl in lists for t in dl.tus]
    assert sum(t.intra for t in tus) * 2 == len(tus) == len(D.e_items(chroma, bd))
    for n in (4, 8, 16, 32):
        want = {r for r, _ in D.e_blocks(n, bd)}
        for intra in (False, True):
            got = {t.recipe for t in tus if t.kind == F.TU_IDCT and t.log2 == int(np.log2(n)) and t.intra == intra}
            assert got == want, (n, intra)
    kinds = {(t.kind, t.flags) for t in tus if t.log2 == 2}
    assert {(F.TU_DST4, 0), (F.TU_SKIP, F.TUF_ROTATE), (F.TU_BYPASS, F.TUF_RDPCM | F.TUF_RDPCM_VER), (F.TU_SKIP, F.TUF_RDPCM)} <= kinds
    if chroma == 3:
        assert any(t.c and t.log2 == 5 for t in tus)          # chroma 32x32
    for dl in lists:                                          # no two blocks of a plane overlap
        for c in range(F.n_planes(dl.p)):
            w, h = F.plane_dims(dl.p, c)
            cover = np.zeros((h, w), np.int32)
            for t in dl.tus:
                if t.c == c:
                    cover[t.y:t.y + (1 << t.log2), t.x:t.x + (1 << t.log2)] += 1
            assert cover.max() <= 1, dl.name


def no_overlap(dl):
    cover = np.zeros((dl.p.height // 4, dl.p.width // 4), np.int32)
    for u in dl.pus:
        cover[u.y // 4:(u.y + u.h) // 4, u.x // 4:(u.x + u.w) // 4] += 1
    return cover.max() <= 1


@pytest.mark.parametrize("chroma,bd", D.A_FULL + D.A_CUT)
def test_matrix_holds_every_shape_kind_fraction(chroma, bd):
    full = (chroma, bd) in D.A_FULL
    lists = D.build_a(chroma, bd, full)
    assert len({id(dl) for dl in lists}) == len(lists)
    shapes = D.SHAPES_ALL if full else D.SHAPES_CUT
    got = D.a_triples(lists)
    want = {(w, h, k, fx, fy) for w, h in shapes for k in D.KINDS for fx in range(8) for fy in range(8)}
    assert want <= got
    assert {(w, h, "list1 of " + k, fx, fy) for w, h in shapes for k in ("bi", "wbi") for fx in range(8) for fy in range(8)} <= got
    n = sum(len(dl.pus) for dl in lists)
    assert n == len(shapes) * len(D.KINDS) * 64
    assert all(no_overlap(dl) and dl.p.width <= D.MAX_DIM and dl.p.height <= D.MAX_DIM for dl in lists)
    assert all(abs(v >> 2) <= 8 for dl in lists for u in dl.pus for mv in u.mv for v in mv)
    print(f"A chroma {chroma} {bd} bit: {n} PUs in {len(lists)} pictures")


@pytest.mark.parametrize("chroma,bd", D.B_FORMATS)
def test_border_lists_hold_every_zone_and_crossing(chroma, bd):
    lists = D.build_b(chroma, bd)
    pairs = D.b_pairs(lists)
    want = {(z, str(c)) for z, c in D.B_VARIANTS}
    assert len(want) == 65
    for size in D.B_SIZES:
        assert pairs[size] == want, size
    assert all(no_overlap(dl) for dl in lists)
    # every 8x8 position on the 4-sample grid is used
    for width, height in D.B_SIZES:
        pos = {(u.x, u.y) for dl in lists if (dl.p.width, dl.p.height) == (width, height) for u in dl.pus}
        assert pos == {(x, y) for x in range(0, width - 7, 4) for y in range(0, height - 7, 4)}
    # the vectors do what the variant says (luma window = block displaced by mv >> 2, 3 samples before, 4 after)
    for dl in lists[::7]:
        for u in dl.pus:
            zone, arg = u.note[4:u.note.index("]")].split(" ", 1)
            mv = u.mv[1 if u.kind == "uni1" else 0]
            x0, x1 = u.x + (mv[0] >> 2) - 3, u.x + (mv[0] >> 2) + u.w + 3
            y0, y1 = u.y + (mv[1] >> 2) - 3, u.y + (mv[1] >> 2) + u.h + 3
            if zone in ("left", "top_left", "bottom_left"):
                assert (x1 <= -64) if arg == "outside" else (-x0 == int(arg)), u
            if zone in ("right", "top_right", "bottom_right"):
                assert (x0 >= dl.p.width + 64) if arg == "outside" else (x1 - (dl.p.width - 1) == int(arg)), u
            if zone in ("top", "top_left", "top_right"):
                assert (y1 <= -64) if arg == "outside" else (-y0 == int(arg)), u
            if zone in ("bottom", "bottom_left", "bottom_right"):
                assert (y0 >= dl.p.height + 64) if arg == "outside" else (y1 - (dl.p.height - 1) == int(arg)), u
    fracs = {(mv[0] & 3, mv[1] & 3) for dl in lists for u in dl.pus for mv in u.mv}
    assert {(fx & 3, fy & 3) for fx, fy in D.B_FRACS} <= fracs
    assert {u.kind for dl in lists for u in dl.pus} == {"uni0", "uni1", "bi"}
    print(f"B chroma {chroma} {bd} bit: {sum(len(dl.pus) for dl in lists)} PUs in {len(lists)} lists")


@pytest.mark.parametrize("chroma,bd", D.D_FORMATS)
def test_occupancy_lists_hold_every_pattern(chroma, bd):
    pats = D.d_patterns(D.build_d(chroma, bd))
    for h in (8, 4):
        assert {n for hh, n, _ in pats if hh == h} == set(range(1, 9))
        assert {(h, 4, pat) for pat in range(16)} <= pats
        assert {(h, 1, 0), (h, 1, 1)} <= pats


def run_oracle_inter(dl):
    pics = dl.pictures()
    assert oracle().oh_or_pass_inter(C.byref(dl.frame), host_pic_array(pics)) == 0
    return pics


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_graded_weights_leave_the_output_in_range(bd):
    """on the checker's result every graded entry x kind leaves at least 25 % of its PUs' luma samples strictly inside (0, max)"""
    dl, = D.build_c(1, bd)
    out = run_oracle_inter(dl)[2].visible(0)
    mx = (1 << bd) - 1
    shares = {}
    for u in dl.pus:
        e = int(u.note[len("[C: entry "):-1])
        blk = out[u.y:u.y + u.h, u.x:u.x + u.w]
        s = shares.setdefault((e, u.kind), [0, 0])
        s[0] += int(np.count_nonzero((blk > 0) & (blk < mx)))
        s[1] += blk.size
    assert len(shares) == 12 * 3
    for (e, kind), (inside, total) in sorted(shares.items()):
        print(f"{bd} bit entry {e} {kind}: {100 * inside / total:.1f} % inside (0, max)")
    for (e, kind), (inside, total) in shares.items():
        if e < len(D.GRADED):
            assert inside >= 0.25 * total, (bd, e, kind, inside, total)


def m2_lists():
    out = []
    for chroma, bd in D.A_FULL:
        out.append((f"A-{chroma}-{bd}", lambda chroma=chroma, bd=bd: D.build_a(chroma, bd, True)))
    for chroma, bd in D.B_FORMATS:
        out.append((f"B-{chroma}-{bd}", lambda chroma=chroma, bd=bd: D.build_b(chroma, bd)))
    for chroma, bd in D.C_FORMATS:
        out.append((f"C-{chroma}-{bd}", lambda chroma=chroma, bd=bd: D.build_c(chroma, bd)))
    return out


@pytest.mark.skipif(not have_ref(), reason="reference tree / oracle/_ref not present")
@pytest.mark.parametrize("name,build", m2_lists(), ids=[n for n, _ in m2_lists()])
def test_checker_inter_pass_equals_the_reference_slots(name, build):
    """oh_or_pass_inter on the directed lists == every PU composed from the reference's own slots (directed.expected_pu), all planes"""
    r = ref()
    n = 0
    for dl in build():
        before = dl.pictures()
        got = run_oracle_inter(dl)[2]
        for u in dl.pus:
            for c, bx, by, want in D.expected_pu(r, dl.p, u, before):
                have = got.visible(c)[by:by + want.shape[0], bx:bx + want.shape[1]]
                assert np.array_equal(have, want), f"{dl.name}: plane {c} of {u}"
            n += 1
    assert n
