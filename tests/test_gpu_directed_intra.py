"""GPU parity (-m gpu) on the directed intra work lists of tests/directed_intra.py: the HIP engine must reproduce the CPU checker
bit for bit on every list of the five families (flags x mode x size x plane, picture edges, thresholds, occupancy and chains,
constrained intra prediction) — with the form of the intra pass the engine chooses for the picture, and with each form forced.
The in-loop filters are off, so a picture is the output of the intra pass; a difference is reported with the block that wrote
the sample: size, plane, mode, flags, residual, recipe."""
import gc

import pytest

import directed_intra as DI
from forced_engine import forced_engine
from test_gpu_directed import check_lists, eng  # noqa: F401  (eng: the module-scoped engine fixture)

pytestmark = pytest.mark.gpu

F_CASES = [(cf, bd, part) for cf, bd in DI.F_FULL + DI.F_CUT for part in range(DI.F_PARTS[(cf, bd)])]
G_CASES = [(cf, bd, what) for cf, bd in DI.G_FORMATS for what in DI.G_KINDS]
H_CASES = [(bd, kind) for bd in DI.H_DEPTHS for kind in ("strong", "plain", "disabled", "chroma444", "chroma420", "clip")]
K_CASES = ([("8x8", 1, 8, part) for part in range(4)] + [("8x8 min cb 16", 1, 8, None)] +
           [("large", cf, bd, part) for cf, bd in DI.K_FORMATS for part in range(3)] + [("edge", cf, bd, None) for cf, bd in DI.K_FORMATS])


def h_lists(bd, kind):
    if kind == "clip":
        return DI.build_h_clip(bd)
    if kind.startswith("chroma"):
        return DI.build_h_thr(bd, "strong", 3 if kind == "chroma444" else 1, 1)
    return DI.build_h_thr(bd, kind)


def k_lists(kind, chroma, bd, part):
    if kind == "8x8":
        return DI.build_k8(bd, 3, part)
    if kind == "8x8 min cb 16":
        return DI.build_k8(bd, 4)
    return DI.build_k_big(chroma, bd, part) if kind == "large" else DI.build_k_edge(chroma, bd)


@pytest.mark.parametrize("chroma,bd,part", F_CASES)
def test_flags_mode_size_plane_matrix(eng, chroma, bd, part):
    """F: every (size, mode, flag subset) in luma and in chroma, each block alone in its cell on extreme-mixed noise, residuals none /
    small / saturating; the matrix of a format is dealt to several cases (tests/test_directed_intra_lists.py asserts that together
    they hold every triple once)"""
    lists = DI.build_f(chroma, bd, part)
    assert lists and check_lists(eng, lists) == len(lists)


@pytest.mark.parametrize("chroma,bd,what", G_CASES)
def test_picture_edges(eng, chroma, bd, what):
    """G: up-right / bottom-left runs cut by the picture's edge at every possible length, blocks at x = 0 and y = 0 with every flag
    subset the position allows, pictures of 8x8, 16x8 and 8x16"""
    lists = DI.build_g(chroma, bd, what)
    assert lists and check_lists(eng, lists) == len(lists)


@pytest.mark.parametrize("bd,kind", H_CASES)
def test_thresholds(eng, bd, kind):
    """H: 32x32 blocks whose edges sit one below, on and one above the limit of the strong smoothing, on gathered and on substituted
    ends, with the strong smoothing on, off and all smoothing disabled, and the same edges in chroma; modes 1 / 10 / 26 on edges
    that drive the boundary filter's clip both ways"""
    lists = h_lists(bd, kind)
    assert lists and check_lists(eng, lists) == len(lists)


@pytest.mark.parametrize("chroma,bd", DI.J_FORMATS)
def test_occupancy_and_chains(eng, chroma, bd):
    """J: CTUs of 16 / 32 / 64 fully covered by quadtrees of chaining blocks, 1 .. 9 and more small blocks to a sub-level beside
    large ones, neighbours driven to 0 and to the maximum"""
    lists = DI.build_j(chroma, bd)
    assert check_lists(eng, lists) == len(lists)


@pytest.mark.parametrize("kind,chroma,bd,part", K_CASES, ids=[f"{k}-{cf}-{bd}-{part}" for k, cf, bd, part in K_CASES])
def test_constrained_intra_pred_masks(eng, kind, chroma, bd, part):
    """K: every mask of intra / inter groups around an 8x8 block, picked masks around larger and chroma blocks, blocks at x = 0 and
    y = 0, 4x4 and 8x8 min PUs"""
    lists = k_lists(kind, chroma, bd, part)
    assert lists and check_lists(eng, lists) == len(lists)


def test_matrix_with_pinned_lists(eng):
    """one F case (4:2:0 8 bit, part 0) with every array in page-locked memory (OH_FRAME_PINNED)"""
    from openhevc_amd import frame as F
    lists = DI.build_f.__wrapped__(1, 8, 0, eng.L)
    assert all(dl.frame.flags & F.OH_FRAME_PINNED for dl in lists)
    assert check_lists(eng, lists) == len(lists)
    del lists
    gc.collect()


def test_cip_masks_with_pinned_lists(eng):
    """one K case (8x8 masks, part 0) with pinned lists"""
    from openhevc_amd import frame as F
    lists = DI.build_k8.__wrapped__(8, 3, 0, eng.L)
    assert all(dl.frame.flags & F.OH_FRAME_PINNED for dl in lists)
    assert check_lists(eng, lists) == len(lists)
    del lists
    gc.collect()


# ---- each form of the pass forced (an engine reads its switches when it is created: tests/forced_engine.py) ----
FORCED = {
    "F": lambda: [DI.build_f(1, 10, 0), DI.build_f(3, 8, 0)],
    "G": lambda: [DI.build_g(cf, bd, w) for cf, bd in DI.G_FORMATS for w in DI.G_KINDS],
    "H": lambda: ([DI.build_h_thr(bd, v) for bd in DI.H_DEPTHS for v in DI.H_VARIANTS] +
                  [DI.build_h_thr(bd, "strong", cf, 1) for bd in DI.H_DEPTHS for cf in (3, 1)] + [DI.build_h_clip(bd) for bd in DI.H_DEPTHS]),
    "J": lambda: [DI.build_j(cf, bd) for cf, bd in DI.J_FORMATS],
    "K": lambda: [DI.build_k8(8, 3)],
}


def run_forced(family, **switches):
    with forced_engine(**switches) as e:
        for lists in FORCED[family]():
            assert lists and check_lists(e, lists) == len(lists)


@pytest.mark.parametrize("family", list(FORCED))
@pytest.mark.parametrize("mode", ["dag", "direct"])
def test_forced_forms(mode, family):
    """part 0 of F for 4:2:0 10 bit and 4:4:4 8 bit, all of G, H and J and K's 8x8 masks through the staged form (a workgroup per CTU,
    the CTU in LDS) and through the direct form (a wave per CTU on the picture in HBM), whatever the engine would choose"""
    run_forced(family, OHEVC_INTRA_MODE=mode)


@pytest.mark.parametrize("waves,phases", [(2, 2), (8, 8)])
def test_chains_under_wave_layouts(waves, phases):
    """J with the sub-levels of a CTU dealt to 2 and to 8 waves"""
    run_forced("J", OHEVC_INTRA_WAVES=waves, OHEVC_INTRA_PHASES=phases)


@pytest.mark.parametrize("res_lds", [0, 1])
def test_chains_with_residuals_staged_or_not(res_lds):
    """J through the staged form with the residuals read from HBM and staged in LDS"""
    run_forced("J", OHEVC_INTRA_MODE="dag", OHEVC_INTRA_RES_LDS=res_lds)
