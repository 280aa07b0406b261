"""Keeps the structured test content honest, on the CPU: the pictures of content.STRUCTURED_CASES must drive the ORACLE through the
content-dependent branches of the luma deblocking filter and of the intra smoothing that uniform noise almost never reaches
(oh_or_counters, oracle.h).  tests/test_gpu_structured.py then compares the engine with the oracle on the very same pictures.
The thresholds are conditions on the content, not measurements of the code: a case that misses one gets other knobs or seeds.

Counters, both seeds together, vertical / horizontal edges (luma segments with bs > 0); the 48 noise cases of
test_gpu_parity.py together give 170 980 segments, 18 479 filtered (11 %), 1 691 strong, 13 filtered next to a PCM / bypass block
and no strong one:

    case                     segments    filter on      strong   strong next to PCM / bypass
    i8_sis                  2268/2180    2165/2064     518/550   -          (33 strongly smoothed 32x32 intra blocks)
    i10_sis                 2268/2180    2165/2063     634/677   -          (35)
    b8                      2920/2966    2720/2783     177/159   -
    b12 (136x88)              434/404      393/384       31/35   -
    b8_ctb16_one_row (96x16)    80/40        68/34        10/3   -
    b10_sparse_lists        1834/1860    1192/1223       36/64   -
    b8_pcm_bypass           1800/1798    1664/1711     253/278   17/20
    b10_pcm_bypass          1953/1993    1815/1867     185/155   43/19
    b8_422_pcm_bypass         765/724      706/636     131/109   15/20
    b10_422_pcm_bypass      1109/1097     981/1014       64/85   10/32
    all 19 cases          28010/27463  25292/25104   3222/3111   85/91
"""
import ctypes as C

import numpy as np
import pytest

import content as K
from openhevc_amd import frame as F
from oracle_lib import have_ref, host_pic_array, oracle, oracle_counters


def run_case(case):
    """oracle pictures of both seeds and the counters they left behind"""
    p = K.structured_params(case)
    rec = F.Recorder(p)
    oracle_counters()
    out = []
    for seed in K.STRUCTURED_SEEDS:
        f, pics = K.structured_picture(case, rec, seed)
        assert oracle().oh_or_frame(C.byref(f), host_pic_array(pics)) == 0
        out.append(pics[2])
    cnt = oracle_counters()
    rec.close()
    return out, cnt


@pytest.mark.parametrize("case", K.STRUCTURED_CASES, ids=K.STRUCTURED_IDS)
def test_structured_case_reaches_the_filter_branches(case):
    name, w, h = case[0], case[1], case[2]
    _, cnt = run_case(case)
    v, hz = cnt["v"], cnt["h"]
    msg = f"{name}: vertical {v} horizontal {hz} strongly smoothed 32x32 intra blocks {cnt['intra_strong_32']}"
    print(msg)                                               # lines_px_clipped and strong_tc2_hits: shown, no threshold
    for d in (v, hz):
        assert d["segments"] > 0 and 2 * d["filter_on"] >= d["segments"], msg
        assert d["filter_on"] == d["strong"] + d["normal"], msg
        assert d["nd_p"] >= 1 and d["nd_q"] >= 1 and d["lines_skipped"] >= 1, msg
        if h >= 128:
            assert d["strong"] >= 8, msg
    assert v["strong"] + hz["strong"] >= 1, msg
    if "pcm" in name:
        assert v["filter_on_pcm"] + hz["filter_on_pcm"] >= 100, msg
        assert v["strong_pcm"] + hz["strong_pcm"] >= 8 and v["strong_pcm"] >= 1 and hz["strong_pcm"] >= 1, msg
    else:
        assert v["filter_on_pcm"] + hz["filter_on_pcm"] == 0, msg
    if "sis" in name:
        assert case[8]["split_pct"] <= 20 and cnt["intra_strong_32"] >= 15, msg


def test_counters_leave_the_pictures_alone_and_reset():
    """the same picture twice gives the same samples and the same counts; a read with reset clears them"""
    case = K.case_named("b8_422_pcm_bypass")
    a, ca = run_case(case)
    b, cb = run_case(case)
    assert ca == cb and all(x.equal(y) for x, y in zip(a, b))
    again = oracle_counters()
    assert again["intra_strong_32"] == 0 and not any(again["v"].values()) and not any(again["h"].values())


@pytest.mark.parametrize("case", [c for c in K.STRUCTURED_CASES if "pcm" in c[0]], ids=[n for n in K.STRUCTURED_IDS if "pcm" in n])
def test_pcm_and_bypass_flags_matter_where_the_filter_is_on(case):
    """the same lists with pcm_loop_filter_disable = transquant_bypass_enable = 0 in a copy of their parameters filter the PCM and
    bypass blocks too: luma differs from the real result — also with SAO off on both sides, so that its restore step, which
    reads the same flags, is not what differs"""
    p = K.structured_params(case)
    rec = F.Recorder(p)
    for seed in K.STRUCTURED_SEEDS:
        f, pics = K.structured_picture(case, rec, seed)
        got = []
        for pcm, sao in ((1, 1), (0, 1), (1, 0), (0, 0)):
            g = F.OhFrame()
            C.memmove(C.byref(g), C.byref(f), C.sizeof(F.OhFrame))
            g.p.pcm_loop_filter_disable = g.p.transquant_bypass_enable = pcm
            g.p.sao_enabled = sao
            mine = {k: v.copy() for k, v in pics.items()}
            assert oracle().oh_or_frame(C.byref(g), host_pic_array(mine)) == 0
            got.append(mine[2].visible(0).copy())
        assert not np.array_equal(got[0], got[1]), (case[0], seed)
        assert not np.array_equal(got[2], got[3]), (case[0], seed, "deblocking alone")
    rec.close()


@pytest.mark.skipif(not have_ref(), reason="reference tree / oracle/_ref not present")
@pytest.mark.parametrize("name", ["b10_pcm_bypass", "b12"])
def test_structured_picture_through_reference_kernels(name):
    """the oracle's own paths on this content against the reference's kernels and drivers (ref_frame), as
    test_whole_picture_through_reference_kernels does on noise"""
    from test_oracle_picture_vs_ref import ref_frame
    case = K.case_named(name)
    p = K.structured_params(case)
    rec = F.Recorder(p)
    for seed in K.STRUCTURED_SEEDS:
        f, pics = K.structured_picture(case, rec, seed)
        want = {k: v.copy() for k, v in pics.items()}
        assert oracle().oh_or_frame(C.byref(f), host_pic_array(want)) == 0
        assert ref_frame(rec, f, pics) == 0
        for c in range(F.n_planes(p)):
            assert np.array_equal(want[2].visible(c), pics[2].visible(c)), (name, seed, c)
    rec.close()
