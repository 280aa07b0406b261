"""GPU parity (-m gpu) on the directed extreme-value work lists of tests/directed.py: the HIP engine must reproduce the CPU
checker bit for bit on every list of the five families (fraction x shape x kind matrix, borders and clamping, full-range weights,
wave occupancy, residual extremes).  The in-loop filters are off, so a picture is the output of mc_kernel / residual_kernel /
the intra pass; a difference is reported with the PU or transform block that wrote the sample."""
import ctypes as C
import gc

import numpy as np
import pytest

import directed as D
from oracle_lib import host_pic_array, oracle

pytestmark = pytest.mark.gpu

BATCH = 32


@pytest.fixture(scope="module")
def eng():
    from openhevc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def assert_same_named(dl, want, got):
    for c in range(len(want.planes)):
        a, b = want.visible(c), got.visible(c)
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            x, y = int(xs[0]), int(ys[0])
            raise AssertionError(f"{dl.name}: plane {c} differs at {len(ys)} samples, first (x={x}, y={y}): oracle {a[y, x]} "
                                 f"engine {b[y, x]}; written by {dl.item_at(c, x, y)}")


def check_lists(eng, lists):
    """every list through the engine (uploaded and executed in batches, the references of one geometry uploaded once) and through
    the checker; returns the number of lists compared"""
    from openhevc_amd.engine import remap_frame
    groups = {}
    for dl in lists:
        groups.setdefault((dl.p.width, dl.p.height, dl.seed), []).append(dl)
    n = 0
    for group in groups.values():
        p = group[0].p
        base = group[0].pictures()
        ref_ids = [eng.pic_alloc(p) for _ in range(2)]
        cur_ids, dfs = [], []
        try:
            for k in range(2):
                eng.pic_upload(ref_ids[k], base[k])
            for i in range(0, len(group), BATCH):
                chunk = group[i:i + BATCH]
                cur_ids = [eng.pic_alloc(p) for _ in chunk]
                for cid in cur_ids:
                    eng.pic_upload(cid, base[2])
                dfs = eng.frames_upload([remap_frame(dl.frame, {0: ref_ids[0], 1: ref_ids[1], 2: cid}) for dl, cid in zip(chunk, cur_ids)])
                eng.frames_execute(dfs)
                eng.sync()
                for dl, cid in zip(chunk, cur_ids):
                    want = {0: base[0], 1: base[1], 2: base[2].copy()}
                    assert oracle().oh_or_frame(C.byref(dl.frame), host_pic_array(want)) == 0
                    assert_same_named(dl, want[2], eng.pic_download(cid, p))
                    n += 1
                for df in dfs:
                    eng.frame_free(df)
                for cid in cur_ids:
                    eng.pic_free(cid)
                cur_ids, dfs = [], []
        finally:
            for df in dfs:
                eng.frame_free(df)
            for pid in ref_ids + cur_ids:
                eng.pic_free(pid)
    return n


A_CASES = [(cf, bd, part) for cf, bd in D.A_FULL + D.A_CUT for part in range(D.A_PARTS[(cf, bd) in D.A_FULL])]
B_CASES = [(cf, bd, size, part) for cf, bd in D.B_FORMATS for size in D.B_SIZES for part in range(D.B_PARTS[size])]
E_CASES = [(cf, bd, part) for cf, bd in D.E_FORMATS for part in range(D.E_PARTS)]


@pytest.mark.parametrize("chroma,bd,part", A_CASES)
def test_fraction_shape_kind_matrix(eng, chroma, bd, part):
    """A: every (shape, kind, fraction) triple, shuffled so that a wave mixes them; all 24 shapes for 4:2:0 at 8 and 10 bit.  The
    matrix of a format is dealt to several cases (tests/test_directed_lists.py asserts that together they hold every triple)."""
    lists = D.build_a(chroma, bd, (chroma, bd) in D.A_FULL, part)
    assert lists and check_lists(eng, lists) == len(lists)


@pytest.mark.parametrize("chroma,bd,size,part", B_CASES, ids=[f"{cf}-{bd}-{w}x{h}-{k}" for cf, bd, (w, h), k in B_CASES])
def test_borders_and_clamping(eng, chroma, bd, size, part):
    """B: windows across every edge and corner by 1 .. 8 samples, wholly outside, and the int16 extremes of the vector, in
    pictures from 8x8 (chroma planes 4 wide: every window on the clamped path) to 64x64"""
    lists = D.build_b(chroma, bd, size, part)
    assert lists and check_lists(eng, lists) == len(lists)


@pytest.mark.parametrize("chroma,bd", D.C_FORMATS)
def test_full_range_weights(eng, chroma, bd):
    """C: weights -128 .. 255, offsets -128 .. 127, denominators 0 .. 7 (luma and chroma different) on uni L0, uni L1 and bi PUs"""
    assert check_lists(eng, D.build_c(chroma, bd)) == 1


@pytest.mark.parametrize("chroma,bd", D.D_FORMATS)
def test_wave_occupancy(eng, chroma, bd):
    """D: 1 .. 8 jobs, every uni / bi pattern of four: dead quarters of a wave and the ballot that skips the second list"""
    lists = D.build_d(chroma, bd)
    assert check_lists(eng, lists) == len(lists)


@pytest.mark.parametrize("chroma,bd,part", E_CASES)
def test_residual_extremes(eng, chroma, bd, part):
    """E: dense, sign-aligned, single- and two-coefficient saturating blocks through IDCT / DST / skip / bypass (rdpcm, rotation),
    each added at once and kept as the residual of a DC intra block"""
    lists = D.build_e(chroma, bd, part)
    assert lists and check_lists(eng, lists) == len(lists)


def test_matrix_with_pinned_lists(eng):
    """one A case (4:2:2 10 bit, part 0) with every array in page-locked memory (OH_FRAME_PINNED): pulled by the GPU from where they lie"""
    from openhevc_amd import frame as F
    lists = D.build_a.__wrapped__(2, 10, False, 0, eng.L)
    assert all(dl.frame.flags & F.OH_FRAME_PINNED for dl in lists)
    assert check_lists(eng, lists) == len(lists)
    del lists
    gc.collect()


def test_residual_extremes_with_pinned_lists(eng):
    """one E case (4:2:0 12 bit, part 0) with pinned lists"""
    from openhevc_amd import frame as F
    lists = D.build_e.__wrapped__(1, 12, 0, eng.L)
    assert all(dl.frame.flags & F.OH_FRAME_PINNED for dl in lists)
    assert check_lists(eng, lists) == len(lists)
    del lists
    gc.collect()
