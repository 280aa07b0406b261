"""The host helpers of the colour remapping service through ctypes (include/ohevc_hip.h: oh_remap_curve, oh_remap_from_sei,
oh_remap_luts, oh_remap_sample) against the numpy model of tests/remap_model.py, which a first test holds to plain loops over Python
ints — no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import remap_model as RM                                                    # noqa: E402
import test_colour_remap_sei as S                                           # noqa: E402  its bit writer
from openhevc_amd import annexb as A                                        # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

PAIRS = [(bi, bo) for bi in RM.DEPTHS for bo in RM.DEPTHS]
U16P = C.POINTER(C.c_uint16)


def test_model_against_python_ints():
    """curve, sample, picture and luts of the numpy model on a few hundred samples"""
    rng = np.random.default_rng(1)
    for bi, bo in [(8, 8), (10, 8), (8, 12), (12, 9)]:
        for n in (0, 1, 2, 33):
            pv = RM.random_pivots(rng, bi, bo, n)
            assert RM.curve(bi, bo, pv).tolist() == RM.curve_ints(bi, bo, pv)
        pre, post = RM.random_tables(rng, bi, bo)
        for d in (0, 7, 15):
            k = RM.random_matrix(rng, d)
            s = rng.integers(0, 1 << bi, (3, 10, 10))
            counts = []
            got = RM.apply(list(s), pre, k, d, post, bi, bo, counts)
            want = [RM.sample_ints(s[:, y, x], pre, k, d, post, bi, bo) for y in range(10) for x in range(10)]
            assert [tuple(int(got[c][y, x]) for c in range(3)) for y in range(10) for x in range(10)] == want
            assert got[0].dtype == (np.uint16 if bo > 8 else np.uint8)
            diag = np.diag(np.diag(k))
            assert RM.luts(pre, k, d, post, bi, bo) is None
            assert RM.luts(pre, diag, d, post, bi, bo).tolist() == RM.luts_ints(pre, diag, d, post, bi, bo)
    # hand-computed: pre and post the identity at 8 bit, d = 2: (1 + 6 + 9 + 2) >> 2 = 4; (4 + 10 + 18 + 2) >> 2 = 8; (7 + 16 - 27 + 2) >> 2 = -1 -> 0
    ident = np.tile(np.arange(256), (3, 1))
    assert RM.sample_ints((1, 2, 3), ident, [[1, 2, 3], [4, 5, 6], [7, 8, -9]], 2, ident, 8, 8) == (4, 8, 0)
    assert RM.curve_ints(8, 8, [(0, 0), (4, 2)])[:5] == [0, 1, 1, 2, 2]                  # (y t + 2) // 4: 0, 0.75 -> 1 (2 t + 2) // 4
    assert RM.curve(8, 10, ()).tolist() == [(1023 * v + 127) // 255 for v in range(256)]


@pytest.mark.parametrize("bi,bo", PAIRS, ids=[f"{bi}to{bo}" for bi, bo in PAIRS])
def test_curve_against_model(bi, bo):
    rng = np.random.default_rng(100 * bi + bo)
    Mi, Mo = (1 << bi) - 1, (1 << bo) - 1
    cases = [RM.random_pivots(rng, bi, bo, n) for n in (1, 2, 3, 7, 32, 33, 33)]
    cases += [[], [(0, Mo), (Mi, 0)], [(Mi // 2, Mo)], [(0, 0)], [(Mi, Mo)], [(Mi - 1, 0), (Mi, Mo)], [(i, Mo - i) for i in range(33)]]
    for pv in cases:
        assert np.array_equal(E.remap_curve(bi, bo, pv), RM.curve(bi, bo, pv)), pv


def test_curve_refusals():
    for bad in ([(5, 1), (5, 2)], [(6, 1), (5, 2)], [(256, 0)], [(0, 256)], [(i, 0) for i in range(34)]):
        with pytest.raises(E.EngineError) as err:
            E.remap_curve(8, 8, bad)
        assert err.value.code == E.OH_E_ARG
    for bi, bo in ((7, 8), (8, 11), (16, 8), (8, 16)):
        with pytest.raises(E.EngineError):
            E.remap_curve(bi, bo)
    with pytest.raises(ValueError):
        E.remap_curve(8, 8, [(-1, 0)])


def sei_case(rng, bi, bo, matrix):
    pre = [RM.random_pivots(rng, bi, bo, n) for n in (33, 0, 2)]
    post = [RM.random_pivots(rng, bo, bo, n) for n in (0, 5, 33)]
    return S.remap(bi, bo, pre=pre, matrix=matrix, post=post, id=1, signal=S.BT2020)


@pytest.mark.parametrize("bi,bo", PAIRS, ids=[f"{bi}to{bo}" for bi, bo in PAIRS])
def test_from_sei_parsed_from_bytes(bi, bo):
    rng = np.random.default_rng(7 * bi + bo)
    rows = [[9000, -1200, 300], [-32768, 32767, 1], [0, -5, 16384]]
    for matrix in (None, (13, rows)):
        d = A.colour_remap(S.unit(sei_case(rng, bi, bo, matrix)))
        for r in (E.remap_from_sei(d), E.remap_from_sei(A.colour_remap_to_struct(d))):
            assert (r.in_bit_depth, r.out_bit_depth) == (bi, bo)
            assert r.pre.shape == (3, 1 << bi) and r.post.shape == (3, 1 << bo)
            for c in range(3):
                assert np.array_equal(r.pre[c], RM.curve(bi, bo, d["pre"][c]))
                assert np.array_equal(r.post[c], RM.curve(bo, bo, d["post"][c]))
            assert r.log2_denom == (13 if matrix else 0) and r.coeff.tolist() == (rows if matrix else [[1, 0, 0], [0, 1, 0], [0, 0, 1]])


def test_from_sei_refusals():
    with pytest.raises(ValueError):
        E.remap_from_sei(None)
    with pytest.raises(E.EngineError) as err:
        E.remap_from_sei(dict(id=0, cancel=True))
    assert err.value.code == E.OH_E_ARG
    for bi, bo in ((11, 8), (8, 16), (14, 14)):
        with pytest.raises(E.EngineError) as err:
            E.remap_from_sei(S.remap(bi, bo))
        assert err.value.code == E.OH_E_UNSUPPORTED
    for bad in (S.remap(8, 8, pre=[[(3, 0), (3, 1)], [], []]), S.remap(10, 8, post=[[], [], [(0, 0), (256, 1)]]),
                S.remap(10, 8, pre=[[], [(0, 256), (1, 0)], []]), S.remap(8, 10, pre=[[(0, 0), (256, 1)], [], []])):
        with pytest.raises(E.EngineError) as err:
            E.remap_from_sei(bad)
        assert err.value.code == E.OH_E_ARG
    s = A.OhColourRemapSei()                                                # present 0
    with pytest.raises(E.EngineError):
        E.remap_from_sei(s)


@pytest.mark.parametrize("bi,bo", PAIRS, ids=[f"{bi}to{bo}" for bi, bo in PAIRS])
def test_luts(bi, bo):
    rng = np.random.default_rng(31 * bi + bo)
    pre, post = RM.random_tables(rng, bi, bo)
    for d, diag in ((0, (1, 1, 1)), (0, (3, 0, -1)), (15, (32767, -32768, 20000)), (6, (64, 100, 17))):
        k = np.diag(diag)
        r = E.Remap(pre, k, d, post, bi, bo)
        got = r.luts()
        assert got.shape == (3, 1 << bi) and got.dtype == np.uint16
        assert np.array_equal(got, RM.luts(pre, k, d, post, bi, bo))
    for c, i in ((0, 1), (2, 0), (1, 2)):
        k = np.diag([4, 4, 4])
        k[c, i] = -1
        with pytest.raises(E.EngineError) as err:
            E.Remap(pre, k, 2, post, bi, bo).luts()
        assert err.value.code == E.OH_E_UNSUPPORTED
    with pytest.raises(E.EngineError) as err:
        E.Remap(pre, np.diag([1, 1, 40000]), 2, post, bi, bo).luts()
    assert err.value.code == E.OH_E_ARG


@pytest.mark.parametrize("bi,bo", PAIRS, ids=[f"{bi}to{bo}" for bi, bo in PAIRS])
def test_sample_against_model(bi, bo):
    """10^4 random triples; the matrix is such that results fall below 0 and above Mo: both clips occur"""
    rng = np.random.default_rng(53 * bi + bo)
    pre, post = RM.random_tables(rng, bi, bo)
    n = 10000
    s = rng.integers(0, 1 << bi, (3, n)).astype(np.uint16)
    s[:, :3] = [[0, (1 << bi) - 1, 0xFFFF]] * 3                             # the ends, and a sample above Mi (looked up by its low bits)
    fn = E.lib().oh_remap_sample
    for d in (0, 9, 15):
        k = RM.random_matrix(rng, d)
        r = E.Remap(pre, k, d, post, bi, bo)
        st = r.as_struct()
        counts = []
        want = np.stack(RM.apply(list(s), pre, k, d, post, bi, bo, counts))
        low, high = counts[0]
        assert low > 0 and high > 0, (low, high)
        got = np.zeros((n, 3), dtype=np.uint16)
        sin = np.ascontiguousarray(s.T)
        ps, pg = sin.ctypes.data, got.ctypes.data
        for j in range(n):
            assert fn(C.byref(st), C.cast(ps + 6 * j, U16P), C.cast(pg + 6 * j, U16P)) == 1
        assert np.array_equal(got.T, want)
    assert E.Remap(pre, k, d, post, bi, bo).sample(s[:, 5]) == tuple(int(v) for v in want[:, 5])
