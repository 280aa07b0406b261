"""The host-only helpers of the picture comparison (include/ohevc_hip.h: oh_compare_ssim_consts, oh_compare_ssim_window,
oh_compare_psnr) against tests/compare_model.py — no GPU needed.  oh_compare_ssim_window is the function the kernel evaluates
(csrc/compare_common.h), so this pins the formula bit for bit."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compare_model as CM                                                  # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402

DEPTHS = (8, 9, 10, 12)
Q = 1 << 30


def sums(a, b):
    """(s1, s2, ss, s12) of 8x8 windows a, b: int64 arrays of (n, 8, 8)"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    return a.sum(axis=(1, 2)), b.sum(axis=(1, 2)), (a * a + b * b).sum(axis=(1, 2)), (a * b).sum(axis=(1, 2))


def lib_windows(bd, s1, s2, ss, s12):
    f = E.lib().oh_compare_ssim_window
    return np.array([f(bd, int(s1[i]), int(s2[i]), int(ss[i]), int(s12[i])) for i in range(len(s1))], dtype=np.int64)


def test_consts_equal_the_model():
    for bd in DEPTHS:
        assert E.compare_ssim_consts(bd) == CM.ssim_consts(bd), bd
    assert E.compare_ssim_consts(8) == (416, 235963)
    for bd in (0, 7, 11, 16):
        with pytest.raises(E.EngineError):
            E.compare_ssim_consts(bd)


@pytest.mark.parametrize("bd", DEPTHS)
def test_window_equals_the_model_on_random_windows(bd):
    """100 000 reachable sum tuples: the sums of two random 8x8 windows; and 20 000 more from a window and a noisy copy of it (the
    high-SSIM end, which independent windows do not reach)"""
    rng = np.random.default_rng(bd)
    n, m, top = 100000, 20000, (1 << bd) - 1
    a = rng.integers(0, top + 1, (n + m, 8, 8))
    b = rng.integers(0, top + 1, (n + m, 8, 8))
    amp = rng.integers(1, 1 << (bd - 2), (m, 1, 1))
    b[n:] = np.clip(a[n:] + rng.integers(-1, 2, (m, 8, 8)) * amp, 0, top)
    s = sums(a, b)
    want = CM.ssim_window(bd, *s)
    got = lib_windows(bd, *s)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert want.min() < Q // 2 < want.max() <= Q


@pytest.mark.parametrize("bd", DEPTHS)
def test_window_extremes(bd):
    top = (1 << bd) - 1
    zero, full = np.zeros((1, 8, 8), np.int64), np.full((1, 8, 8), top, np.int64)
    board = ((np.add.outer(np.arange(8), np.arange(8)) & 1) * top)[None].astype(np.int64)
    cases = [(zero, zero), (full, full), (zero, full), (full, zero), (board, top - board)]
    for k, (a, b) in enumerate(cases):
        s = sums(a, b)
        want = int(CM.ssim_window(bd, *s)[0])
        assert E.compare_ssim_window(bd, *(int(v[0]) for v in s)) == want, (bd, k)
        if k < 2:
            assert want == Q
    s = sums(board, top - board)                                            # negative covariance: a negative window value
    assert E.compare_ssim_window(bd, *(int(v[0]) for v in s)) < 0


@pytest.mark.parametrize("bd", DEPTHS)
def test_identical_windows_give_one_exactly(bd):
    rng = np.random.default_rng(100 + bd)
    a = rng.integers(0, 1 << bd, (2000, 8, 8))
    a[:200] = rng.integers(0, 1 << bd, (200, 1, 1))                         # flat windows: zero variance
    s = sums(a, a)
    assert np.all(lib_windows(bd, *s) == Q)
    assert np.all(CM.ssim_window(bd, *s) == Q)


def test_psnr():
    for bd in DEPTHS:
        M = (1 << bd) - 1
        for sse, samples in ((1, 1), (7, 3840 * 2160), (123456789, 8294400), (M * M * 4096, 4096), (2 ** 50, 2 ** 26)):
            want = 10 * math.log10(M * M * samples / sse)
            assert E.compare_psnr(sse, samples, bd) == pytest.approx(want, rel=1e-14, abs=1e-12), (bd, sse, samples)
        assert E.compare_psnr(0, 100, bd) == math.inf
        assert math.isnan(E.compare_psnr(5, 0, bd)) and math.isnan(E.compare_psnr(0, 0, bd))
        assert E.compare_psnr(M * M * 64, 64, bd) == 0.0                    # zero against maximum


def test_model_on_a_hand_made_plane():
    """the model itself: counts, first, leftovers and the window count on a plane small enough to check by hand"""
    a = np.zeros((9, 14), np.int64)
    b = a.copy()
    b[8, 13] = 3                                                            # in the leftover row and column
    b[2, 5] = 1
    d = CM.plane_diff(a, b, 8)
    assert d["samples"] == 126 and d["differing"] == 2 and d["sad"] == 4 and d["sse"] == 10 and d["max_abs"] == 3
    assert d["first"] == (5, 2) and d["ssim_windows"] == 2 * 1
    q = CM.window_values(a, b, 8)
    assert q.shape == (1, 2) and np.all(q < Q)                              # both windows cover (5, 2)
    b[2, 5] = 0
    d = CM.plane_diff(a, b, 8)
    assert d["first"] == (13, 8) and d["ssim_sum"] == 2 * Q                 # the leftovers take no part in SSIM
    assert CM.plane_diff(a[:2, :4], b[:2, :4], 8)["ssim_windows"] == 0


def test_python_constants_equal_the_headers():
    """the kernel's tile, from which the GPU test derives its shapes, and the flag values"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "openhevc_amd", "csrc", "kernels.h")).read() + open(os.path.join(root, "include", "ohevc_hip.h")).read()

    def const(name):
        return int(re.search(r"\b" + name + r"\s*=\s*(0x[0-9A-Fa-f]+|\d+)", txt).group(1), 0)

    assert (E.CMP_TW, E.CMP_TH) == (const("OH_CMP_TW"), const("OH_CMP_TH"))
    assert (E.CMP_SSIM, E.CMP_NONE, E.CONV_MAX_PICS) == (const("OH_CMP_SSIM"), const("OH_CMP_NONE"), const("OH_CONV_MAX_PICS"))
    assert E.CMP_TW % 4 == 0 and E.CMP_TH % 4 == 0
