"""GPU parity (-m gpu) on low-activity pictures, where the deblocking filter actually filters.  The pictures of
tests/test_gpu_parity.py are uniform noise: there d0 + d3 < beta holds for about a tenth of the luma segments, the strong filter is
rare and never runs next to a PCM / bypass block.  Here the references come from content.zoned_picture and the work lists carry
small residuals and flat PCM blocks (content.STRUCTURED_CASES); tests/test_structured_content.py shows on the CPU, from the
oracle's decision counters, that these pictures reach those branches.  The engine must reproduce the oracle bit for bit."""
import ctypes as C

import numpy as np
import pytest

import content as K
from openhevc_amd import frame as F
from oracle_lib import host_pic_array, oracle
from test_gpu_parity import assert_same, eng, run_both  # noqa: F401  (eng: the module-scoped engine fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.STRUCTURED_CASES, ids=K.STRUCTURED_IDS)
def test_structured_picture_parity(eng, case):  # noqa: F811
    p = K.structured_params(case)
    rec = F.Recorder(p)
    for seed in K.STRUCTURED_SEEDS:
        f, pics = K.structured_picture(case, rec, seed)
        want, got = run_both(eng, p, f, pics)
        assert_same(want, got, f"{case[0]} seed {seed}")
    rec.close()


PINNED = ("b10_pcm_bypass", "b12", "b10_444", "b10_tiles")


@pytest.mark.parametrize("name", PINNED)
def test_structured_pinned_lists(eng, name):  # noqa: F811
    """the same kind of list with every array in page-locked memory and the strengths packed four to the byte (OH_FRAME_PINNED)"""
    case = K.case_named(name)
    p = K.structured_params(case)
    rec = F.Recorder(p)
    f, pics = K.structured_picture(case, rec, 41, synth_seed=4100)
    fc = F.FrameCopy(f, pinned_by=eng.L)
    assert fc.frame.flags & F.OH_FRAME_PINNED
    want, got = run_both(eng, p, fc.frame, pics)
    assert_same(want, got, f"{name} pinned")
    del fc
    rec.close()


def test_structured_batch(eng):  # noqa: F811
    """oh_frames_execute: 9 pictures of 136x88 10-bit, I and B mixed, shared structured references, the residual scale varying
    from picture to picture: one launch per pass over all of them, each against the oracle"""
    from openhevc_amd.engine import remap_frame
    p = F.pic_params(136, 88, bit_depth=10)
    rec = F.Recorder(p)
    rng = np.random.default_rng(12)
    refs = {0: K.zoned_picture(p, rng), 1: K.zoned_picture(p, rng)}
    ids = {k: eng.pic_alloc(p) for k in refs}
    for k, hp in refs.items():
        eng.pic_upload(ids[k], hp)
    dfs, want, cur_ids = [], [], []
    for i in range(9):
        st = 0 if i % 4 == 1 else 2
        f = rec.synth(F.synth_params(st, 9300 + i, intra_pct=10 + 5 * (i % 7), coeff_shift=1 + i % 4, pcm_flat=1), 2, [0, 1])
        cur = F.HostPic(p, rng=rng)
        pics = {0: refs[0].copy(), 1: refs[1].copy(), 2: cur.copy()}
        assert oracle().oh_or_frame(C.byref(f), host_pic_array(pics)) == 0
        want.append(pics[2])
        cid = eng.pic_alloc(p)
        eng.pic_upload(cid, cur)
        cur_ids.append(cid)
        dfs.append(eng.frame_upload(remap_frame(f, {0: ids[0], 1: ids[1], 2: cid})))
    eng.frames_execute(dfs)
    eng.sync()
    try:
        for i in range(9):
            assert_same(want[i], eng.pic_download(cur_ids[i], p), f"structured batch picture {i}")
    finally:
        for df in dfs:
            eng.frame_free(df)
        for v in list(ids.values()) + cur_ids:
            eng.pic_free(v)
        rec.close()


def test_structured_reference_chain(eng):  # noqa: F811
    """P, B, B on the device starting from one structured picture: the second and third predict from filtered, low-activity
    DECODED pictures, which never leave HBM"""
    from openhevc_amd.engine import remap_frame
    p = F.pic_params(264, 200)
    rec = F.Recorder(p)
    rng = np.random.default_rng(2)
    host = {0: K.zoned_picture(p, rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng), 3: F.HostPic(p, rng=rng)}
    ids = {k: eng.pic_alloc(p) for k in host}
    for k, hp in host.items():
        eng.pic_upload(ids[k], hp)
    arr = host_pic_array(host)
    try:
        for cur, refs in ((1, [0]), (2, [0, 1]), (3, [1, 2])):
            f = rec.synth(F.synth_params(1 if len(refs) == 1 else 2, 520 + cur, coeff_shift=4, pcm_flat=1), cur, refs)
            assert oracle().oh_or_frame(C.byref(f), arr) == 0
            eng.frame_submit(remap_frame(f, ids))
            eng.sync()
            assert_same(host[cur], eng.pic_download(ids[cur], p), f"structured chain picture {cur}")
    finally:
        for v in ids.values():
            eng.pic_free(v)
        rec.close()


def test_structured_random_configurations(eng):  # noqa: F811
    """the parameter draws of test_random_configurations over 20 small pictures, with small residuals (coeff_shift 2..4), flat PCM
    blocks and structured references"""
    seed, count = 20261018, 20
    rng = np.random.default_rng(seed)
    for it in range(count):
        chroma = int(rng.choice([0, 1, 1, 1, 2, 3]))
        bd = int(rng.choice([8, 8, 10, 10, 12]))
        lc = int(rng.choice([4, 5, 6]))
        w, h = 8 * int(rng.integers(2, 34)), 8 * int(rng.integers(2, 26))
        st = int(rng.choice([0, 1, 2, 2, 2]))
        pcm, byp, cip = bool(rng.integers(0, 3) == 0), bool(rng.integers(0, 3) == 0), bool(rng.integers(0, 3) == 0)
        p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc,
                         pcm_loop_filter_disable=int(pcm), transquant_bypass_enable=int(byp), constrained_intra_pred=int(cip),
                         strong_intra_smoothing=int(rng.integers(0, 2)), intra_smoothing_disabled=int(rng.integers(0, 4) == 0),
                         sao=int(rng.integers(0, 4) != 0), deblock=int(rng.integers(0, 4) != 0),
                         cb_qp_offset=int(rng.integers(-4, 5)), cr_qp_offset=int(rng.integers(-4, 5)))
        knobs = dict(intra_pct=int(rng.integers(0, 80)), skip_pct=int(rng.integers(0, 70)), bi_pct=int(rng.integers(0, 100)),
                     frac_mv_pct=int(rng.integers(0, 101)), mv_range=int(rng.choice([8, 64, 300, 3000])),
                     cbf_pct=int(rng.integers(10, 100)), weighted_pct=int(rng.choice([0, 0, 30, 100])),
                     split_pct=int(rng.integers(10, 90)), tskip_pct=int(rng.choice([0, 0, 30])),
                     pcm_pct=int(rng.choice([0, 15])) if pcm else 0, bypass_pct=int(rng.choice([0, 15])) if byp else 0,
                     sao_pct=int(rng.integers(0, 101)), vary_deblock_offsets=int(rng.integers(0, 2)),
                     sparse_pct=int(rng.choice([0, 0, 50, 100])), scaling_list=int(rng.integers(0, 2)),
                     ccp_pct=int(rng.choice([0, 50])) if chroma == 3 else 0, bs_from_motion=int(rng.integers(0, 3) == 0),
                     coeff_shift=int(rng.choice([2, 3, 4])), pcm_flat=1)
        rec = F.Recorder(p)
        f = rec.synth(F.synth_params(st, 556000 + it, **knobs), 2, [0, 1] if st else [])
        prng = np.random.default_rng(it)
        pics = {0: K.zoned_picture(p, prng), 1: K.zoned_picture(p, prng), 2: F.HostPic(p, rng=prng)}
        want, got = run_both(eng, p, f, pics)
        assert_same(want, got, f"structured random configuration {it}: {w}x{h} {bd} bit chroma {chroma} ctb {1 << lc} slice {st} "
                               f"pcm {pcm} bypass {byp} cip {cip} knobs {knobs}")
        rec.close()


@pytest.mark.parametrize("flavour", ["no_filters", "deblock_only", "sao_only"])
def test_structured_pass_switches(eng, flavour):  # noqa: F811
    """each in-loop filter switched off per picture, on content where the one left on has work to do"""
    p = F.pic_params(264, 200, sao=int(flavour == "sao_only"), deblock=int(flavour == "deblock_only"))
    rec = F.Recorder(p)
    f = rec.synth(F.synth_params(2, 78, coeff_shift=4, pcm_flat=1), 2, [0, 1])
    rng = np.random.default_rng(6)
    pics = {0: K.zoned_picture(p, rng), 1: K.zoned_picture(p, rng), 2: F.HostPic(p, rng=rng)}
    want, got = run_both(eng, p, f, pics)
    assert_same(want, got, f"structured {flavour}")
    rec.close()
