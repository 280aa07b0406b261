"""-m gpu: oh_pics_histogram / Engine.pics_histogram on the MI355X against the numpy model of tests/levels_model.py, every field of every
plane bit for bit: the chroma formats and bit depths with contents that reach bin 0, the top bin, every bin and one bin only; windows
that leave 70 x 38 and 131 x 67 samples (picture sizes are multiples of 8, so these are windows of 72 x 40 and 136 x 72 pictures; an odd
width needs a format without horizontal sub-sampling) with plane rows that are no whole granules and start inside an odd granule; a
flat plane of more than 2^17 samples; noise over many workgroups; more than one launch; a second call; a resized picture; the same sums
by oh_pics_compare; and the argument rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import levels_model as LM                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = [(8, 1), (10, 1), (10, 2), (12, 3), (8, 0)]


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def shapes(p):
    return [F.plane_dims(p, c)[::-1] for c in range(F.n_planes(p))]


def planes_of(kind, p, rng):
    """the planes of a picture of one kind of content; the ramps of the three planes start a third of the range apart, so that every
    bin is hit in some plane even where a plane has fewer samples than bins"""
    third = (1 << p.bit_depth) // 3
    return [LM.content(kind, s, p.bit_depth, rng, start=c * third) for c, s in enumerate(shapes(p))]


def put(eng, p, planes):
    hp = F.HostPic(p)
    for c, pl in enumerate(planes):
        hp.visible(c)[...] = pl
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid


def same(got, want, bd, what=None):
    """an Engine Histogram against the model's three PlaneHist"""
    for c in range(3):
        g, w = got.plane[c], want[c]
        assert g.hist.shape == (1 << bd,) and g.hist.dtype == np.uint32
        assert not w.hist[1 << bd:].any()
        assert np.array_equal(g.hist, w.hist[:1 << bd]), (what, c, np.argwhere(g.hist != w.hist[:1 << bd])[:4])
        assert (g.samples, g.sum, g.sum_sq, g.min, g.max) == w.fields(), (what, c)
        if w.samples:
            assert g.mean == w.sum / w.samples and g.variance == (w.samples * w.sum_sq - w.sum ** 2) / w.samples ** 2
        else:
            assert g.mean is None and g.variance is None


@pytest.mark.parametrize("bd,cf", FORMATS, ids=[f"{bd}bit_cf{cf}" for bd, cf in FORMATS])
def test_formats_and_contents(bd, cf):
    """96 x 40, one call: random, all zero, all M, a ramp through every bin, and random values that leave bins empty"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(bd * 10 + cf)
    eng = Engine(0)
    p = params(96, 40, bd, cf)
    kinds = ("random", "zero", "top", "ramp", "sparse")
    pics = [planes_of(k, p, rng) for k in kinds]
    got = eng.pics_histogram([put(eng, p, pl) for pl in pics])
    for k, pl, g in zip(kinds, pics, got):
        same(g, LM.histogram(pl, cf), bd, k)
    M = (1 << bd) - 1
    assert got[1].plane[0].hist[0] == 96 * 40 and got[2].plane[0].hist[M] == 96 * 40 and got[0].plane[0].min == 0 and got[0].plane[0].max == M
    if cf == 0:
        assert got[0].plane[1].samples == 0 and not got[0].plane[2].hist.any()
    eng.close()


# (picture, format, window (left, right, top, bottom)): what the window leaves and where its chroma rows start
WINDOWS = [((72, 40), (8, 1), (2, 0, 2, 0)),        # 70 x 38 from chroma column 1: 35 bytes of a chroma row
           ((72, 40), (10, 1), (0, 2, 0, 2)),       # 70 x 38 at the origin: rows of 140 and 70 bytes
           ((136, 72), (8, 1), (38, 28, 4, 30)),    # 70 x 38; chroma from column 19: 3 bytes into granule 1
           ((136, 72), (10, 2), (18, 48, 3, 31)),   # 70 x 38; chroma from column 9: 2 bytes into granule 1
           ((136, 72), (12, 3), (3, 2, 5, 0)),      # 131 x 67 in all three planes
           ((136, 72), (8, 0), (5, 0, 0, 5)),       # 131 x 67, luma alone
           ((136, 72), (10, 3), (9, 126, 71, 0)),   # one sample wide, one high: one granule, from inside granule 1
           ((136, 72), (8, 1), (0, 0, 0, 0))]       # the whole picture: 9 row groups of 8 in luma


@pytest.mark.parametrize("size,fmt,window", WINDOWS, ids=[f"{s[0]}x{s[1]}_{f[0]}bit_cf{f[1]}_{'_'.join(map(str, w))}" for s, f, w in WINDOWS])
def test_windows_and_leftovers(size, fmt, window):
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(sum(window) + fmt[0])
    eng = Engine(0)
    p = params(*size, *fmt)
    pics = [planes_of(k, p, rng) for k in ("random", "flat", "ramp")]
    got = eng.pics_histogram([put(eng, p, pl) for pl in pics], window=window)
    for pl, g in zip(pics, got):
        want = LM.histogram(pl, fmt[1], window)
        same(g, want, fmt[0], window)
        assert want[0].samples == (size[0] - window[0] - window[1]) * (size[1] - window[2] - window[3])
    eng.close()


def test_flat_plane_beyond_narrow_counters():
    """1040 x 136: 141440 equal luma samples, more than 2^17 — the whole count arrives in one bin through the combined runs"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(3)
    eng = Engine(0)
    for bd in (8, 10):
        p = params(1040, 136, bd, 1)
        pl = planes_of("flat", p, rng)
        got = eng.pics_histogram([put(eng, p, pl)])[0]
        same(got, LM.histogram(pl, 1), bd, "flat")
        v = (1 << bd) // 2
        assert got.plane[0].hist[v] == 1040 * 136 > 1 << 17 and got.plane[0].variance == 0.0 and got.plane[0].mean == v
    eng.close()


def test_noise_over_many_workgroups():
    """520 x 264 of noise at 8 bit: 33 luma workgroups add into every one of the 256 bins of one result; and runs inside a granule
    next to noise: a picture whose samples repeat in runs of 1 .. 40"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(4)
    eng = Engine(0)
    p = params(520, 264, 8, 1)
    noise = planes_of("random", p, rng)
    runs = []
    for s in shapes(p):
        n = s[0] * s[1]
        lengths = rng.integers(1, 41, n // 8)
        runs.append(np.repeat(rng.integers(0, 256, lengths.size), lengths)[:n].astype(np.uint8).reshape(s))
    got = eng.pics_histogram([put(eng, p, noise), put(eng, p, runs)])
    same(got[0], LM.histogram(noise, 1), 8, "noise")
    same(got[1], LM.histogram(runs, 1), 8, "runs")
    assert 264 > 4 * E.HG_ROWS and got[0].plane[0].hist.min() > 0
    eng.close()


def test_more_than_one_launch_and_a_second_call():
    """70 pictures of 32 x 16 in one call, each with its own content: two launches; the same call again gives the same (every call
    starts from zero), and a call on other pictures of another depth is not disturbed by what the first left"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(70)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 6
    p = params(32, 16, 10, 1)
    pics = [planes_of("random", p, rng) for _ in range(n)]
    ids = [put(eng, p, pl) for pl in pics]
    for turn in range(2):
        got = eng.pics_histogram(ids)
        assert len(got) == n
        for pl, g in zip(pics, got):
            same(g, LM.histogram(pl, 1), 10, turn)
    p8 = params(32, 16, 8, 3)
    one = planes_of("top", p8, rng)
    same(eng.pics_histogram([put(eng, p8, one)])[0], LM.histogram(one, 3), 8, "after")
    assert eng.pics_histogram([]) == []
    eng.close()


def test_resized_picture_and_compare():
    """a picture that oh_pics_resize made, counted over the image's window: equal to the model on the downloaded planes; and the
    sums by existing GPU code: against an all-zero picture oh_pics_compare gives sad == sum, sse == sum_sq, max_abs == max"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(9)
    eng = Engine(0)
    p = params(64, 48, 10, 1)
    src = put(eng, p, planes_of("random", p, rng))
    out, win = eng.pics_resize([src], (150, 90), filter="bicubic")
    dp = eng._pic_params(out[0])
    hp = eng.pic_download(out[0], dp)
    got = eng.pics_histogram(out, window=win)[0]
    same(got, LM.histogram([hp.visible(c) for c in range(3)], 1, win), 10, "resized")
    assert got.plane[0].samples == 150 * 90
    zero = put(eng, dp, planes_of("zero", dp, rng))
    cmp = eng.pics_compare(out, [zero], window=win, ssim=False)[0]
    for c in range(3):
        g = got.plane[c]
        assert (cmp.plane[c].sad, cmp.plane[c].sse, cmp.plane[c].max_abs, cmp.plane[c].samples) == (g.sum, g.sum_sq, g.max, g.samples), c
    eng.close()


def test_argument_errors_leave_out_untouched():
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    rng = np.random.default_rng(2)
    p = params(32, 16, 10, 1)
    a, b = (put(eng, p, planes_of("random", p, rng)) for _ in range(2))
    other = put(eng, params(32, 16, 8, 1), planes_of("random", params(32, 16, 8, 1), rng))
    out = (E.OhHistogram * 2)()
    C.memset(out, 0x55, C.sizeof(out))
    keep = []

    def call(ids=(a, b), n=None, win=(0, 0, 0, 0), win_null=False, out_null=False, e_null=False):
        arr = (C.c_int * max(len(ids), 1))(*ids) if ids is not None else None
        w = E.OhWindow(*win)
        keep.extend((arr, w))
        return L.oh_pics_histogram(None if e_null else eng.h, arr, len(ids or []) if n is None else n, None if win_null else C.byref(w),
                                   None if out_null else out)

    arg = E.OH_E_ARG
    assert call(e_null=True) == arg and call(win_null=True) == arg and call(out_null=True) == arg and call(ids=None, n=2) == arg
    assert call(n=-1) == arg
    assert call(ids=(a, 999)) == arg and call(ids=(-1, b)) == arg                                          # unknown pictures
    assert call(ids=(a, other)) == arg                                                                     # params differ
    for win in ((32, 0, 0, 0), (16, 16, 0, 0), (0, 0, 8, 8), (-2, 0, 0, 0), (0, 0, 0, -2)):                   # empty, or negative
        assert call(win=win) == arg, win
    for win in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):                                    # not multiples of 2 x 2
        assert call(win=win) == arg, win
    assert bytes(out) == b"\x55" * C.sizeof(out), "a refused call wrote into out"
    assert call(ids=(), n=0) == 0 and call(ids=None, n=0) == 0                                             # n == 0
    assert bytes(out) == b"\x55" * C.sizeof(out)
    assert call() == 0 and out[0].plane[0].samples == 32 * 16 and out[1].plane[2].samples == 16 * 8
    assert call(ids=(a, a)) == 0 and bytes(out[0]) == bytes(out[1])                                        # a picture twice is fine
    with pytest.raises(E.EngineError) as ei:
        eng.pics_histogram([a], window=(2, 0, 1, 0))
    assert ei.value.code == arg
    eng.close()
