"""The up-sampler of tests/packing_model.py held to the CPU checker's restatement of the reference's arithmetic: the unrounded sums S of a
side-by-side row without flip equal the int16 output of the checker's horizontal slots in their x2 variant, which uses phases 0 and 8
with the taps centred as the reference centres them.  This pins the tables and the tap alignment of the model.

  g = 0   p = 8 X: index X >> 1, phase 8 (X & 1) — the x2 slot at EL column X.
  g = 8   p = 8 (X - 1): the x2 slot at EL column X - 1; the slot is handed the row one sample to the left, so that its column X + 1
          is the model's X and X = 0 (index -1, phase 8, every tap left of the centre clamped) is covered too.

The slots do not clamp: the row lies in a buffer whose margins replicate its first and last sample, which is what the clamp of the
definition reads.  Chroma: the 4-tap slot against a chroma plane that is not sub-sampled on the packed axis (4:4:4; p = 8 X - g) at
g = 0 and 8, and against a sub-sampled one (4:2:0; p = (16 X - g + 1) >> 1) at g = 0; at g = 8 a sub-sampled chroma plane has the
phases 12 and 4, which the x2 slot does not have."""
import ctypes as C

import numpy as np
import pytest

import packing_model as M
from openhevc_amd import frame as F
from oracle_lib import i16p, off_u8p, oracle

N, ROWS, MARGIN = 37, 5, 16


def slot_sums(c, g, chroma):
    """the x2 slot over the rows of c (uint8, N samples each) for the model's outputs 0 .. 2 N - 1 at grid position g (0 or 8)"""
    n = c.shape[1]
    buf = np.empty((c.shape[0], n + 2 * MARGIN), np.uint8)
    buf[:, MARGIN:MARGIN + n] = c
    buf[:, :MARGIN] = c[:, :1]
    buf[:, MARGIN + n:] = c[:, -1:]
    u = F.upsample_setup(64, 64, 128, 128, (0, 0, 0, 0))
    assert u.idx == F.OH_UP_X2
    shift = g // 8                                            # columns the slot's output leads the model's by
    w = 2 * n + shift
    got = np.zeros((c.shape[0], w), np.int16)
    f = oracle().oh_or_up_cr_h if chroma else oracle().oh_or_up_luma_h
    f(F.OH_UP_X2, 8, i16p(got), w, off_u8p(buf, MARGIN - shift), buf.shape[1], 0, 0, w, c.shape[0], w + 2, C.byref(u))
    return got[:, shift:].astype(np.int64)


@pytest.mark.parametrize("g", [0, 8])
def test_luma_sums(g):
    rng = np.random.default_rng(g)
    for c in (rng.integers(0, 256, (ROWS, N)).astype(np.uint8), np.full((1, 3), 255, np.uint8), np.arange(8, dtype=np.uint8)[None, :] * 30):
        want = slot_sums(c, g, False)
        assert np.array_equal(M.filter_sums(c, g, 0, False), want)
        # the same through unpack_plane: a side-by-side plane whose left half is c, no flip
        packed = np.concatenate([c, 255 - c], axis=1)
        assert np.array_equal(M.unpack_plane(packed, M.SBS, 0, g=g, plane=0, chroma_format_idc=1), np.clip((want + 32) >> 6, 0, 255))


@pytest.mark.parametrize("g,kind", [(0, 0), (8, 0), (0, 1)])
def test_chroma_sums(g, kind):
    rng = np.random.default_rng(10 + g + kind)
    for c in (rng.integers(0, 256, (ROWS, N)).astype(np.uint8), np.full((1, 2), 255, np.uint8)):
        want = slot_sums(c, g, True)
        assert np.array_equal(M.filter_sums(c, g, kind, True), want)
        packed = np.concatenate([c, 255 - c], axis=1)
        got = M.unpack_plane(packed, M.SBS, 0, g=g, plane=1, chroma_format_idc=1 if kind else 3)
        assert np.array_equal(got, np.clip((want + 32) >> 6, 0, 255))


def test_vertical_chroma_phases_at_g0():
    """at g = 0 the vertical positions of sub-sampled chroma have the phases 14 and 6: the reference's own x2 chroma phases"""
    p = M.positions(16, 0, 2)
    assert [int(v) for v in p[:2] & 15] == [14, 6] and set(int(v) for v in p & 15) == {14, 6}
    assert [int(v) for v in p[:4] >> 4] == [-1, 0, 0, 1]
