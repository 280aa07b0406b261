"""-m gpu: oh_pics_light_level / Engine.pics_light_level on the MI355X against the numpy model of tests/light_model.py, every field of
OhLightLevel bit for bit: chroma formats, bit depths, transfers, norms, ranges, windows, segment and row-group boundaries, calls of
more than one launch, repeated calls, the table caches beside oh_pics_convert_colour's, the way from a measurement to a tone-mapped
image, and the argument rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import colour_model as M                                                    # noqa: E402
import light_model as LM                                                    # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

FS = 1 << 30
FIELDS = ("pixels", "sum", "max", "min")


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def fill(p, how, rng):
    """a picture of uniform random codes over the whole sample range, a luma ramp through every code with neutral chroma, all zero or
    all maximum (the fills of test_gpu_colour.py)"""
    hp = F.HostPic(p)
    top = (1 << p.bit_depth) - 1
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        if how == "random":
            v[...] = rng.integers(0, top + 1, v.shape, dtype=v.dtype)
        elif how == "ramp":
            v[...] = (np.arange(v.size) % (top + 1)).reshape(v.shape) if c == 0 else 1 << (p.bit_depth - 1)
        else:
            v[...] = 0 if how == "zero" else top
    return hp


def upload(eng, p, hows, rng):
    pids, hps = [], []
    for how in hows:
        hp = fill(p, how, rng)
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        pids.append(pid)
        hps.append(hp)
    return pids, hps


def coded(hp, p):
    return [hp.visible(c) for c in range(F.n_planes(p))]


def same(got, want):
    """every field of a LightLevel against the model's dict"""
    return all(getattr(got, k) == want[k] for k in FIELDS) and got.hist.dtype == np.uint32 and np.array_equal(got.hist, want["hist"])


def check(eng, pids, hps, p, transfer, **kw):
    got = eng.pics_light_level(pids, transfer, **kw)
    assert len(got) == len(pids)
    for i, hp in enumerate(hps):
        want = LM.light_level(coded(hp, p), p, transfer, **kw)
        assert same(got[i], want), (i, transfer, kw, got[i], {k: want[k] for k in FIELDS})
        assert int(got[i].hist.sum()) == got[i].pixels
    return got


FORMATS = [(8, 1), (10, 1), (10, 2), (12, 3), (8, 0)]                       # bit depth, chroma_format_idc
TRANSFERS = (16, 18, 13, 1)


def combos():
    """30 of the 640 combinations: every format meets every transfer, both norms, both chroma filters, both ranges and both matrices"""
    out = []
    for i in range(30):
        bd, cf = FORMATS[i % 5]
        out.append((bd, cf, TRANSFERS[i % 4], ("maxrgb", "luma")[(i // 2) % 2], ("linear", "nearest")[(i // 3) % 2], bool((i // 5) % 2),
                    (9, 1)[(i // 7) % 2]))
    return out


@pytest.mark.parametrize("bd,cf,transfer,norm,chroma,full,matrix", combos(),
                         ids=[f"{c[0]}b_cf{c[1]}_t{c[2]}_{c[3]}_{c[4]}_{'full' if c[5] else 'limited'}_m{c[6]}" for c in combos()])
def test_formats_equal_the_model(bd, cf, transfer, norm, chroma, full, matrix):
    """96 x 40: random, ramp, all-zero and all-maximum pictures in one call"""
    from openhevc_amd.engine import Engine
    p = params(96, 40, bd, cf)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random", "ramp", "zero", "max"), np.random.default_rng(bd * 7 + cf))
    check(eng, pids, hps, p, transfer, in_primaries=9 if matrix == 9 else 1, norm=norm, src_peak=1000.0 if transfer == 18 else 100.0,
          matrix=matrix, full_range=full, chroma=chroma)
    eng.close()


@pytest.mark.parametrize("bd,cf", FORMATS, ids=[f"{b}b_cf{c}" for b, c in FORMATS])
def test_full_range_pq_maximum_lands_in_the_last_bin(bd, cf):
    from openhevc_amd.engine import Engine
    p = params(96, 40, bd, cf)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("max", "zero"), np.random.default_rng(0))
    got = check(eng, pids, hps, p, 16, norm="maxrgb", full_range=True)
    assert got[0].hist[257] == got[0].pixels == 96 * 40 and got[0].max == got[0].min == FS and got[0].sum == 96 * 40 * FS
    if cf == 0:                                                             # with chroma, Cb = Cr = 0 is a saturated green, not black
        assert got[1].hist[0] == got[1].pixels and got[1].max == 0 and got[1].sum == 0
    assert got[0].full_scale == 10000.0
    eng.close()


def test_windows():
    """a 70 x 38 picture inside coded planes of 72 x 40 (coded sizes are multiples of the minimum coding block): the windows
    (2, 4, 2, 6) and (0, 66, 0, 36) of that picture, the second a 4 x 2 image"""
    from openhevc_amd.engine import Engine
    p = params(72, 40, 10, 1)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random", "ramp"), np.random.default_rng(70))
    for win, size in (((2, 4 + 2, 2, 6 + 2), 64 * 30), ((0, 66 + 2, 0, 36 + 2), 4 * 2), ((0, 2, 0, 2), 70 * 38)):
        for chroma in ("linear", "nearest"):
            got = check(eng, pids, hps, p, 16, window=win, chroma=chroma, norm="luma")
            assert got[0].pixels == size
    eng.close()
    p = params(72, 40, 12, 3)                                               # 4:4:4: odd offsets are aligned
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random",), np.random.default_rng(71))
    check(eng, pids, hps, p, 18, window=(1, 3, 3, 1), src_peak=1000.0)
    eng.close()


@pytest.mark.parametrize("w,h", [(4352, 24), (48, 72)], ids=["4352x24_segments", "48x72_row_groups"])
def test_segment_and_row_group_boundaries(w, h):
    """4352 columns cross every power-of-two segment width up to 4096; 72 rows take more row groups than one workgroup handles"""
    from openhevc_amd.engine import Engine
    p = params(w, h, 10, 1)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random", "ramp"), np.random.default_rng(w))
    check(eng, pids, hps, p, 16, norm="maxrgb")
    check(eng, pids, hps, p, 16, norm="luma", window=(2, 0, 2, 0))
    eng.close()


def test_more_pictures_than_one_launch_and_no_accumulation():
    """70 different pictures of 32 x 16: two launches; the same pictures in two calls; the same call again"""
    from openhevc_amd.engine import Engine
    p = params(32, 16, 10, 1)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 6
    pids, hps = upload(eng, p, ("random",) * n, np.random.default_rng(70))
    one = check(eng, pids, hps, p, 16)
    two = eng.pics_light_level(pids[:33], 16) + eng.pics_light_level(pids[33:], 16)
    again = eng.pics_light_level(pids, 16)
    for i in range(n):
        for other in (two, again):
            assert all(getattr(one[i], k) == getattr(other[i], k) for k in FIELDS) and np.array_equal(one[i].hist, other[i].hist), i
    assert len({x.sum for x in one}) > 60                                   # the pictures do differ
    assert eng.pics_light_level([], 16) == []
    eng.close()


def test_table_caches_do_not_disturb_each_other():
    """light level with PQ, a colour conversion with the HLG pipeline, light level with sRGB, the HLG conversion again and PQ again:
    each equals its model"""
    from openhevc_amd.engine import Engine
    p = params(200, 136, 10, 1)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random", "ramp"), np.random.default_rng(3))
    hlg = E.make_colour(18, 9, out="gamma24", tone="bt2390", norm="luma", src_peak=1000, dst_peak=100)
    tabs = E.colour_tables(hlg)

    def conv():
        g = eng.pics_convert(pids, "rgb_planar", dtype=torch.uint16, matrix=9, colour=hlg).cpu().numpy()
        for i, hp in enumerate(hps):
            assert np.array_equal(g[i], M.convert(coded(hp, p), p, "rgb_planar", E.CONV_U16, hlg, matrix=9, tables=tabs)), i

    check(eng, pids, hps, p, 16)
    conv()
    check(eng, pids, hps, p, 13, in_primaries=1, matrix=1, src_peak=80.0, norm="luma")
    conv()
    check(eng, pids, hps, p, 16)
    check(eng, pids, hps, p, 18, src_peak=300.0)                            # HLG below the colour path's 400 nits, with maxRGB
    conv()
    eng.close()


def test_measured_peak_drives_the_tone_curve():
    """decode -> measure -> make_colour(src_peak = measured) -> pics_convert, no host copy of a picture: a PQ scene whose luma stays
    below code 600 of 1023"""
    from openhevc_amd.engine import Engine
    p = params(200, 136, 10, 1)
    rng = np.random.default_rng(9)
    eng = Engine(0)
    pids, hps = [], []
    for _ in range(3):
        hp = F.HostPic(p)
        hp.visible(0)[...] = rng.integers(64, 601, hp.visible(0).shape)
        for c in (1, 2):
            hp.visible(c)[...] = rng.integers(480, 545, hp.visible(c).shape)
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        pids.append(pid)
        hps.append(hp)
    lls = check(eng, pids, hps, p, 16)
    want_lls = [LM.light_level(coded(hp, p), p, 16) for hp in hps]
    peak = E.source_peak(16, lls, sei=dict(max_cll=4000))
    assert peak == E.light_nits(LM.percentile(want_lls, 999900), 16, 0)
    assert 100.0 < peak < 1000.0                                            # far below the MaxCLL the stream claims
    col = E.make_colour(16, 9, tone="bt2390", src_peak=peak, dst_peak=100)
    tabs = E.colour_tables(col)
    g = eng.pics_convert(pids, "rgb", dtype=torch.uint8, matrix=9, colour=col).cpu().numpy()
    for i, hp in enumerate(hps):
        assert np.array_equal(g[i], M.convert(coded(hp, p), p, "rgb", E.CONV_U8, col, matrix=9, tables=tabs)), i
    eng.close()


def test_argument_errors_leave_out_untouched():
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    p = params(64, 32, 10, 1)
    pids, hps = upload(eng, p, ("random", "random"), np.random.default_rng(1))
    other, _ = upload(eng, params(64, 32, 8, 1), ("random",), np.random.default_rng(2))
    out = (E.OhLightLevel * 3)()
    C.memset(out, 0xA5, C.sizeof(out))
    guard = bytes(out)

    def call(ids, cv, sp, out_p=out):
        return L.oh_pics_light_level(eng.h, (C.c_int * max(len(ids), 1))(*ids), len(ids), C.byref(cv) if cv is not None else None,
                                     C.byref(sp) if sp is not None else None, out_p)

    def spec(**kw):
        sp = E.OhLightSpec(16, 9, E.COL_NORM["maxrgb"], 1000.0)
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    cv = E.make_convert("rgb", E.CONV_U16, matrix=9)
    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    assert call(pids, None, spec()) == arg
    assert call(pids, cv, None) == arg
    assert call(pids, cv, spec(), None) == arg
    assert call([pids[0], 999], cv, spec()) == arg                          # unknown picture
    assert call(pids + other, cv, spec()) == arg                            # params differ
    assert call(pids, E.make_convert("rgb", E.CONV_U16, (1, 0, 0, 0), matrix=9), spec()) == arg      # misaligned window
    assert call(pids, E.make_convert("rgb", E.CONV_U16, (0, 0, 1, 0), matrix=9), spec()) == arg
    assert call(pids, E.make_convert("rgb", E.CONV_U16, (32, 32, 0, 0), matrix=9), spec()) == arg    # empty window
    assert call(pids, E.make_convert("rgb", E.CONV_U16, (0, 0, -2, 0), matrix=9), spec()) == arg
    for kw in (dict(norm=2), dict(norm=-1), dict(src_peak=0.0), dict(src_peak=-5.0), dict(src_peak=float("nan")), dict(src_peak=float("inf"))):
        assert call(pids, cv, spec(**kw)) == arg, kw
    for kw in (dict(in_transfer=2), dict(in_transfer=17), dict(in_primaries=5), dict(in_primaries=0)):
        assert call(pids, cv, spec(**kw)) == uns, kw
    for m in (0, 2, 4, 10):
        assert call(pids, E.make_convert("rgb", E.CONV_U16, matrix=m), spec()) == uns, m
    assert bytes(out) == guard, "a refused call wrote into out"
    assert call([], cv, spec()) == 0 and bytes(out) == guard                # n == 0: nothing to do
    # format and sample are not read; HLG takes maxRGB and any peak; every listed transfer and primaries code is taken
    odd = E.make_convert("planar", E.CONV_NATIVE, matrix=9)
    odd.format, odd.sample = 77, -3
    assert call(pids, odd, spec()) == 0
    for i, hp in enumerate(hps):
        assert same(E.LightLevel(out[i].pixels, out[i].sum, out[i].max, out[i].min, np.frombuffer(out[i].hist, dtype=np.uint32)),
                    LM.light_level(coded(hp, p), p, 16)), i
    assert bytes(out[2]) == guard[2 * C.sizeof(E.OhLightLevel):]            # two pictures, two results
    for t in (16, 18, 13, 1, 6, 14, 15):
        for pr in (1, 9, 12):
            assert call(pids, cv, spec(in_transfer=t, in_primaries=pr, norm=t % 2, src_peak=12000.0 if t == 18 else 150.0)) == 0, (t, pr)
    eng.close()
