"""The identities of the frame packing definition, on tests/packing_model.py alone — no library, no GPU: unpacking the halves of what
pack made gives the views back under every flip combination, and the quincunx interpolation of what pack sampled reproduces the views on
the lattice."""
import itertools

import numpy as np
import pytest

import packing_model as M

ARRS = (M.SBS, M.TB)
FLIPS = list(itertools.product((False, True), repeat=2))


@pytest.mark.parametrize("arr", ARRS)
@pytest.mark.parametrize("flip", FLIPS)
def test_unpack_half_of_pack_is_identity(arr, flip):
    rng = np.random.default_rng(arr * 4 + flip[0] * 2 + flip[1])
    for h, w in ((6, 10), (1, 1), (7, 3)):
        views = [rng.integers(0, 1024, (h, w)) for _ in range(2)]
        packed = M.pack_plane(views[0], views[1], arr, flip=flip)
        assert packed.shape == ((h, 2 * w) if arr == M.SBS else (2 * h, w))
        for v in range(2):
            assert np.array_equal(M.unpack_plane(packed, arr, v, flip=flip[v], full=False), views[v])
        # and the other way round: packing the halves of a packed plane gives it back
        p = rng.integers(0, 1024, packed.shape)
        halves = [M.unpack_plane(p, arr, v, flip=flip[v], full=False) for v in range(2)]
        assert np.array_equal(M.pack_plane(halves[0], halves[1], arr, flip=flip), p)
    if flip == (False, False):
        return
    # a flip is seen: the packed plane differs from the unflipped one
    a = np.arange(24).reshape(4, 6)
    assert not np.array_equal(M.pack_plane(a, a, arr, flip=flip), M.pack_plane(a, a, arr))


@pytest.mark.parametrize("arr", ARRS)
@pytest.mark.parametrize("flip", FLIPS)
def test_quincunx_unpack_of_pack_keeps_the_lattice(arr, flip):
    rng = np.random.default_rng(100 + arr * 4 + flip[0] * 2 + flip[1])
    for H, W in ((8, 12), (2, 2), (6, 4)):
        views = [rng.integers(0, 256, (H, W)) for _ in range(2)]
        packed = M.pack_plane(views[0], views[1], arr, flip=flip, quincunx=True)
        assert packed.shape == (H, W)
        Y, X = np.mgrid[0:H, 0:W]
        for v in range(2):
            full = M.unpack_plane(packed, arr, v, flip=flip[v], quincunx=True)
            on = ((X ^ Y ^ v) & 1) == 0
            assert full.shape == (H, W) and np.array_equal(full[on], views[v][on])
            # the half-size form is C_v itself, and frame 0 holds the sample (0, 0)
            half = M.unpack_plane(packed, arr, v, flip=flip[v], quincunx=True, full=False)
            assert np.array_equal(half, M.constituent(packed, arr, v, flip[v]))
            if v == 0:
                assert half[0, 0] == views[0][0, 0]
            # every other sample is the rounded mean of its lattice neighbours: of a flat view the level itself
        flat = [np.full((H, W), 77), np.full((H, W), 200)]
        packed = M.pack_plane(flat[0], flat[1], arr, flip=flip, quincunx=True)
        for v in range(2):
            assert np.array_equal(M.unpack_plane(packed, arr, v, flip=flip[v], quincunx=True), flat[v])


def test_quincunx_interpolation_by_hand():
    # side by side, view 0, a 2 x 4 plane: lattice (0,0) (2,0) (1,1) (3,1); C_0 = [[a, b], [c, d]]
    a, b, c, d = 10, 20, 30, 41
    packed = np.array([[a, b, 0, 0], [c, d, 0, 0]])
    full = M.unpack_plane(packed, M.SBS, 0, quincunx=True)
    assert full[0, 0] == a and full[0, 2] == b and full[1, 1] == c and full[1, 3] == d
    # (1, 0): L = a, R = b, U outside -> D = c, D = c
    assert full[0, 1] == (a + b + c + c + 2) >> 2
    # (3, 0): L = b, R outside -> L = b, U outside -> D = d
    assert full[0, 3] == (b + b + d + d + 2) >> 2
    # (0, 1): L outside -> R = c, U = a, D outside -> U = a
    assert full[1, 0] == (c + c + a + a + 2) >> 2


def test_full_size_filter_keeps_flat_levels_and_the_seam():
    # two views of different flat levels: every phase sums to 64, so each view stays flat whatever the grid position — a tap across
    # the seam, or a clamp to the wrong half, would show
    for arr in ARRS:
        packed = M.pack_plane(np.full((6, 5), 100), np.full((6, 5), 900), arr)
        for v, level in ((0, 100), (1, 900)):
            for g in range(16):
                for plane, cf in ((0, 1), (1, 1), (1, 3)):
                    out = M.unpack_plane(packed, arr, v, g=g, plane=plane, chroma_format_idc=cf, bit_depth=10)
                    assert out.shape == packed.shape[:1] + (10,) if arr == M.SBS else (12, 5)
                    assert (out == level).all()


def test_all_sixteen_phases_occur():
    for kind in range(3):                                     # over the grid positions, two neighbouring outputs see every phase
        assert set(int(v) for g in range(16) for v in M.positions(2, g, kind) & 15) == set(range(16))
    # the grid positions of the GPU tests (tests/test_gpu_packing.py: GRIDS) see every phase on a plane that is not sub-sampled; the
    # pairs the issue names, (0, 8), (8, 0) and (4, 12), give the phases 0, 4, 8 and 12 alone
    assert set(int(v) for g in (0, 8, 4, 12) for v in M.positions(2, g, 0) & 15) == {0, 4, 8, 12}
    assert set(int(v) for g in (0, 8, 4, 12, 1, 10, 3, 14, 5, 7) for v in M.positions(2, g, 0) & 15) == set(range(16))
