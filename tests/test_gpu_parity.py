"""GPU parity (-m gpu): the HIP engine, called through its C ABI (libohevc_hip.so), must
reproduce the CPU oracle bit for bit on the same seeded work lists, and the reference-recorded
MD5s of tests/golden/."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from forced_engine import forced_engine
from openhevc_amd import frame as F
from oracle_lib import host_pic_array, oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from openhevc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def run_both(eng, p, frame, pics):
    """pics: {host id: HostPic}; returns (oracle result, engine result) for frame.cur_pic"""
    from openhevc_amd.engine import remap_frame
    ids = {}
    for hid, hp in pics.items():
        ids[hid] = eng.pic_alloc(p)
        eng.pic_upload(ids[hid], hp)
    try:
        eng.frame_submit(remap_frame(frame, ids))
        eng.sync()
        got = eng.pic_download(ids[frame.cur_pic], p)
    finally:
        for v in ids.values():
            eng.pic_free(v)
    want_pics = {k: v.copy() for k, v in pics.items()}
    assert oracle().oh_or_frame(C.byref(frame), host_pic_array(want_pics)) == 0
    return want_pics[frame.cur_pic], got


def sent_by_upload(eng, p, frame):
    """the bytes of work list that one hand-over of `frame` (cur_pic 2, references 0 and 1) sends to the GPU"""
    from openhevc_amd.engine import remap_frame
    ids = {k: eng.pic_alloc(p) for k in (0, 1, 2)}
    before = eng.upload_bytes()
    eng.frame_free(eng.frame_upload(remap_frame(frame, ids)))
    for v in ids.values():
        eng.pic_free(v)
    return eng.upload_bytes() - before


def assert_same(want, got, tag):
    for c in range(len(want.planes)):
        a, b = want.visible(c), got.visible(c)
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError(f"{tag}: plane {c} differs at {len(ys)} samples, first (x={xs[0]}, y={ys[0]}): "
                                 f"oracle {a[ys[0], xs[0]]} engine {b[ys[0], xs[0]]}")


CASES = [
    # name, w, h, bd, chroma, log2_ctb, slice_type, knobs
    ("i8", 416, 240, 8, 1, 6, 0, {}),
    ("p8", 416, 240, 8, 1, 6, 1, {}),
    ("b8", 416, 240, 8, 1, 6, 2, {}),
    ("b8_weighted", 416, 240, 8, 1, 6, 2, {"weighted_pct": 50}),
    ("b8_ctb16", 200, 136, 8, 1, 4, 2, {"intra_pct": 30}),
    ("i10", 264, 200, 10, 1, 5, 0, {}),
    ("b10", 264, 200, 10, 1, 6, 2, {"weighted_pct": 25}),
    ("b12", 136, 88, 12, 1, 5, 2, {}),
    ("i8_444", 136, 88, 8, 3, 6, 0, {}),
    ("b10_444", 136, 88, 10, 3, 5, 2, {}),
    ("i8_mono", 128, 64, 8, 0, 6, 0, {}),
    ("i8_422", 136, 88, 8, 2, 6, 0, {}),
    ("b10_422", 200, 136, 10, 2, 5, 2, {"weighted_pct": 25, "intra_pct": 25}),
    ("b8_422_pcm_bypass", 200, 136, 8, 2, 6, 2, {"pcm_pct": 12, "bypass_pct": 12, "intra_pct": 30}),
    ("b8_tskip", 200, 136, 8, 1, 6, 2, {"tskip_pct": 40, "intra_pct": 30}),
    ("b8_pcm_bypass", 264, 200, 8, 1, 6, 2, {"pcm_pct": 12, "bypass_pct": 12, "intra_pct": 30, "vary_deblock_offsets": 1}),
    ("b10_pcm_bypass", 264, 200, 10, 1, 5, 2, {"pcm_pct": 12, "bypass_pct": 12, "intra_pct": 30}),
    ("b8_farmv", 128, 72, 8, 1, 6, 2, {"mv_range": 2000, "skip_pct": 80}),
    ("b8_dense", 416, 240, 8, 1, 6, 2, {"split_pct": 85, "cbf_pct": 95, "skip_pct": 0}),
    ("tiny", 8, 8, 8, 1, 4, 0, {}),
    # constrained_intra_pred_flag = 1 (hevcpred_template.c:116-249): half the CUs intra, PCM CUs count as intra
    ("b8_cip", 264, 200, 8, 1, 6, 2, {"intra_pct": 50}),
    ("b10_cip_pcm", 200, 136, 10, 1, 5, 2, {"intra_pct": 60, "pcm_pct": 10, "split_pct": 70}),
    ("b8_444_cip", 136, 88, 8, 3, 5, 2, {"intra_pct": 40}),
    ("b10_422_cip", 200, 136, 10, 2, 6, 2, {"intra_pct": 50}),
    # sparse residual hand-off: quantised levels + QP (+ scaling lists), de-quantised on the GPU (hevc_cabac.c:1478-1494, 1818-1841)
    ("b8_sparse", 416, 240, 8, 1, 6, 2, {"sparse_pct": 70}),
    ("b10_sparse_lists", 264, 200, 10, 1, 5, 2, {"sparse_pct": 100, "scaling_list": 1, "tskip_pct": 25, "intra_pct": 30}),
    ("i12_444_sparse_lists", 136, 88, 12, 3, 5, 0, {"sparse_pct": 100, "scaling_list": 1}),
    # cross-component prediction (4:4:4 range extension, hevc.c:1319-1365): chroma residual += (scale * luma residual) >> 3
    ("b8_444_ccp", 200, 136, 8, 3, 5, 2, {"ccp_pct": 60, "intra_pct": 30}),
    ("i10_444_ccp_sparse", 136, 88, 10, 3, 6, 0, {"ccp_pct": 80, "sparse_pct": 60, "tskip_pct": 20}),
    ("b10_bs_from_motion", 416, 240, 10, 1, 6, 2, {"bs_from_motion": 1, "intra_pct": 25}),
    ("p8_bs_from_motion_ctb16", 200, 136, 8, 1, 4, 1, {"bs_from_motion": 1, "vary_deblock_offsets": 1}),
    ("i8_422_bs_from_motion", 416, 240, 8, 2, 5, 0, {"bs_from_motion": 1}),
    # 16x16 CTBs with subsampled chroma: the SAO of a CTB sees the first chroma column of its right neighbour before the horizontal-edge
    # deblocking reached it (the reference's driver order, oracle.c: g_pre_h; deblock.hip / sao.hip: sao_stale); 1 and 2 CTB rows are special
    ("i10_422_ctb16", 136, 88, 10, 2, 4, 0, {"sao_pct": 90}),
    ("b8_ctb16_sao", 264, 200, 8, 1, 4, 2, {"sao_pct": 90, "intra_pct": 30}),
    ("b8_ctb16_one_row", 96, 16, 8, 1, 4, 2, {"sao_pct": 90, "intra_pct": 30}),
    ("i10_ctb16_two_rows", 96, 32, 10, 1, 4, 0, {"sao_pct": 90}),
    ("b10_ctb16_slices", 264, 200, 10, 1, 4, 2, dict(n_slices=9, sao_pct=80, slice_knobs=F.SYNTH_NO_LF_ACROSS_SLICES | F.SYNTH_DEBLOCK_OFF_SLICES)),
    # several slices / tiles (pinned through the reference's own drivers in tests/test_oracle_picture_vs_ref.py): SAO restore flags
    # (sao_edge_filter[1]), boundary strengths gated at slice / tile edges, per-slice deblocking off / offsets, neighbour availability
    ("b8_slices_lf_off", 416, 240, 8, 1, 5, 2, dict(n_slices=6, sao_pct=80, slice_knobs=F.SYNTH_NO_LF_ACROSS_SLICES | F.SYNTH_SLICE_OFFSETS)),
    ("b10_slices_deblock_off", 264, 200, 10, 1, 5, 2, dict(n_slices=9, sao_pct=80, slice_knobs=F.SYNTH_NO_LF_ACROSS_SLICES | F.SYNTH_DEBLOCK_OFF_SLICES)),
    ("i8_slices", 264, 200, 8, 1, 6, 0, dict(n_slices=5, sao_pct=80, slice_knobs=F.SYNTH_NO_LF_ACROSS_SLICES | F.SYNTH_SLICE_OFFSETS)),
    ("b8_tiles_lf_off", 416, 240, 8, 1, 5, 2, dict(tile_cols=3, tile_rows=2, sao_pct=80, slice_knobs=F.SYNTH_NO_LF_ACROSS_TILES)),
    ("b10_tiles_slices", 832, 480, 10, 1, 6, 2, dict(tile_cols=2, tile_rows=3, sao_pct=80, slice_knobs=F.SYNTH_NO_LF_ACROSS_TILES | F.SYNTH_SLICE_PER_TILE |
                                                      F.SYNTH_NO_LF_ACROSS_SLICES | F.SYNTH_SLICE_OFFSETS)),
    ("i8_444_tiles", 200, 136, 8, 3, 5, 0, dict(tile_cols=2, tile_rows=2, sao_pct=80, slice_knobs=F.SYNTH_SLICE_PER_TILE | F.SYNTH_NO_LF_ACROSS_SLICES)),
    ("b8_slices_bs_from_motion", 416, 240, 8, 1, 5, 2, dict(n_slices=6, bs_from_motion=1, sao_pct=80, slice_knobs=F.SYNTH_NO_LF_ACROSS_SLICES | F.SYNTH_DEBLOCK_OFF_SLICES)),
    ("p10_422_tiles_bs_from_motion", 416, 240, 10, 2, 5, 1, dict(tile_cols=3, tile_rows=2, bs_from_motion=1, slice_knobs=F.SYNTH_NO_LF_ACROSS_TILES | F.SYNTH_SLICE_PER_TILE)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_picture_parity(eng, case):
    name, w, h, bd, chroma, lc, st, knobs = case
    pcm = "pcm" in name
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc,
                     pcm_loop_filter_disable=int(pcm), transquant_bypass_enable=int(pcm), constrained_intra_pred=int("cip" in name),
                     cb_qp_offset=2 if "weighted" in name else 0, cr_qp_offset=-3 if "weighted" in name else 0)
    rec = F.Recorder(p)
    for seed in range(2):
        f = rec.synth(F.synth_params(st, 3000 + seed, **knobs), 2, [0, 1])
        rng = np.random.default_rng(seed)
        pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
        want, got = run_both(eng, p, f, pics)
        assert_same(want, got, f"{name} seed {seed}")
    rec.close()


PINNED_CASES = ("i8", "b8_weighted", "b8_ctb16", "b12", "b10_444", "i8_mono", "b8_422_pcm_bypass", "tiny", "b10_cip_pcm", "b10_sparse_lists",
                "i10_444_ccp_sparse", "b10_bs_from_motion", "b10_ctb16_slices", "b10_tiles_slices")


# the two other forms of hand-over, both staged: ordinary memory with packed grids (a copy with no packing jobs), pinned memory with
# byte grids (packed out of pinned memory) — on the smallest pictures that reach every optional segment of the arena
OTHER_FORM_CASES = ("tiny", "b8_ctb16", "b8_422_pcm_bypass", "b10_sparse_lists")
FORMS = {"pinned_packed": (True, True), "pageable_packed": (False, True), "pinned_bytes": (True, False), "pageable_bytes": (False, False)}
PINNED_PARAMS = [pytest.param(c, "pinned_packed", id=c[0]) for c in CASES if c[0] in PINNED_CASES] + \
                [pytest.param(c, form, id=f"{c[0]}-{form}") for c in CASES if c[0] in OTHER_FORM_CASES for form in ("pageable_packed", "pinned_bytes")]


@pytest.mark.parametrize("case,form", PINNED_PARAMS)
def test_pinned_lists_are_pulled_by_the_gpu(eng, case, form):
    """OH_FRAME_PINNED: the same pictures with every array of the work list in page-locked memory from oh_host_alloc (boundary strengths
    packed four to the byte): no staging copy on the host — prep_pull reads the arrays over PCIe from where they lie (odd sizes, tails
    and every optional array included).  The forms in between (pageable_packed, pinned_bytes) are staged like an ordinary list; whatever
    the form, the same bytes of a list cross PCIe."""
    name, w, h, bd, chroma, lc, st, knobs = case
    pcm = "pcm" in name
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc,
                     pcm_loop_filter_disable=int(pcm), transquant_bypass_enable=int(pcm), constrained_intra_pred=int("cip" in name),
                     cb_qp_offset=2 if "weighted" in name else 0, cr_qp_offset=-3 if "weighted" in name else 0)
    rec = F.Recorder(p)
    f = rec.synth(F.synth_params(st, 4100, **knobs), 2, [0, 1])
    pinned, packed = FORMS[form]
    fc = F.FrameCopy(f, pinned_by=eng.L if pinned else None, pack_bs=packed)
    assert bool(fc.frame.flags & F.OH_FRAME_PINNED) == pinned
    assert bool(fc.frame.flags & F.OH_FRAME_BS_PACKED) == (packed and bool(f.vertical_bs))
    rng = np.random.default_rng(41)
    pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
    before = eng.upload_bytes()
    want, got = run_both(eng, p, fc.frame, pics)
    assert_same(want, got, f"{name} {form}")
    sent = eng.upload_bytes() - before
    del fc
    if form != "pinned_packed":                       # copy_bytes does not depend on the form: all four send the same bytes
        for other, (opin, opack) in FORMS.items():
            oc = F.FrameCopy(f, pinned_by=eng.L if opin else None, pack_bs=opack)
            assert sent_by_upload(eng, p, oc.frame) == sent, f"{name}: {other} and {form} send different bytes"
            del oc
    rec.close()


@pytest.mark.parametrize("flavour", ["no_filters", "deblock_only", "sao_only"])
def test_pass_switches(eng, flavour):
    """each in-loop filter can be switched off per picture (slice_deblocking_filter_disabled /
    sao disabled): the remaining passes still match"""
    p = F.pic_params(264, 200, sao=int(flavour == "sao_only"), deblock=int(flavour == "deblock_only"))
    rec = F.Recorder(p)
    f = rec.synth(F.synth_params(2, 77), 2, [0, 1])
    rng = np.random.default_rng(5)
    pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
    want, got = run_both(eng, p, f, pics)
    assert_same(want, got, flavour)
    rec.close()


def test_golden_pictures(eng):
    """the engine reproduces MD5s whose in-loop filter stage was produced by the reference's own
    ff_hevc_hls_filters driver (tests/golden/make_golden.py)"""
    from test_golden import build_case, load_picture_cases, md5_planes
    from openhevc_amd.engine import remap_frame
    gold = load_picture_cases()
    for case in gold["cases"]:
        f, pics, rec = build_case(case)
        p = f.p
        ids = {k: eng.pic_alloc(p) for k in pics}
        for k, hp in pics.items():
            eng.pic_upload(ids[k], hp)
        eng.frame_submit(remap_frame(f, ids))
        got = eng.pic_download(ids[2], p)
        for v in ids.values():
            eng.pic_free(v)
        assert md5_planes(got) == gold["expected"][case[0]]["final"], case[0]
        rec.close()


def test_output_fetch_in_two_halves(eng):
    """oh_pic_download_start / oh_download_finish: started on the engine's thread behind the picture's passes, finished on ANOTHER thread while
    this one keeps handing pictures over; the planes are those of oh_pic_download_window; a finish without destination planes returns
    OH_E_ARG and gives the staging buffer back (the next fetch works)"""
    import threading
    from openhevc_amd.engine import remap_frame
    p = F.pic_params(416, 240, bit_depth=10)
    rec = F.Recorder(p)
    rng = np.random.default_rng(8)
    host = {k: F.HostPic(p, rng=rng) for k in range(4)}
    ids = {k: eng.pic_alloc(p) for k in host}
    for k in (0, 1):
        eng.pic_upload(ids[k], host[k])
    fa = F.FrameCopy(rec.synth(F.synth_params(2, 801), 2, [0, 1]))
    fb = F.FrameCopy(rec.synth(F.synth_params(2, 802), 3, [0, 1]))
    eng.frame_submit(remap_frame(fa.frame, ids))
    h = eng.pic_download_start(ids[2], left=8, right=16, top=4, bottom=8)       # enqueued behind picture 2's passes
    got = {}
    t = threading.Thread(target=lambda: got.setdefault("win", eng.download_finish(h, p, left=8, right=16, top=4, bottom=8)))
    t.start()
    for _ in range(20):                                       # meanwhile this thread keeps the engine busy with other pictures
        eng.frame_submit(remap_frame(fb.frame, ids))
    t.join()
    eng.sync()
    want = eng.pic_download_window(ids[2], p, left=8, right=16, top=4, bottom=8)
    for c in range(3):
        assert np.array_equal(want[c], got["win"][c]), c
    full = eng.pic_download(ids[2], p)
    assert np.array_equal(want[0], full.visible(0)[4:240 - 8, 8:416 - 16])
    h2 = eng.pic_download_start(ids[2])
    assert eng.download_finish(h2, p, planes=False) == -2     # OH_E_ARG; the buffer is free again:
    again = eng.download_finish(eng.pic_download_start(ids[2]), p)
    assert np.array_equal(again[0], full.visible(0))
    for v in ids.values():
        eng.pic_free(v)
    rec.close()


def test_submit_and_forget_keeps_the_engines_memory_bounded():
    """a decoder hands one work list per picture to oh_frame_submit and forgets it: over a long stream the device arenas, the pinned
    staging buffers and the deferred lists level off (stream-ordered release into the pools), and the last picture is still right"""
    from openhevc_amd.engine import Engine, remap_frame
    e = Engine(0)
    p = F.pic_params(416, 240)
    rec = F.Recorder(p)
    rng = np.random.default_rng(3)
    host = {k: F.HostPic(p, rng=rng) for k in range(3)}
    ids = {k: e.pic_alloc(p) for k in host}
    for k in (0, 1):
        e.pic_upload(ids[k], host[k])
    lists = [F.FrameCopy(rec.synth(F.synth_params(2 if k % 4 else 0, 700 + k), 2, [0, 1])) for k in range(6)]
    seen = []
    for n in range(400):
        e.frame_submit(remap_frame(lists[n % len(lists)].frame, ids))
        if n % 32 == 31:
            e.sync()                                           # (a decoder that shows its pictures waits for the engine now and then; without any wait
                                                               #  the host runs ahead and the pool grows to its cap of 512 arenas instead)
        if n in (99, 199, 399):
            seen.append(e.memory())
    e.sync()
    m = e.memory()
    assert m["deferred"] == 0 and all(s["deferred"] == 0 for s in seen), seen
    assert all(s["arenas"] <= 40 and s["stages"] <= 48 for s in seen) and seen[2]["arenas"] <= seen[0]["arenas"] + 2, seen     # no arena per picture
    got = e.pic_download(ids[2], p)
    want = {k: v.copy() for k, v in host.items()}
    assert oracle().oh_or_frame(C.byref(lists[399 % len(lists)].frame), host_pic_array(want)) == 0
    assert_same(want[2], got, "picture 400")
    e.close()
    rec.close()


def test_reference_chain_and_reexecute(eng):
    """a picture decoded by the engine is used as reference by the next one without leaving HBM;
    executing an uploaded work list twice gives the same picture (coefficients are not consumed)"""
    from openhevc_amd.engine import remap_frame
    p = F.pic_params(416, 240)
    rec = F.Recorder(p)
    rng = np.random.default_rng(1)
    host = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p), 2: F.HostPic(p), 3: F.HostPic(p)}
    ids = {k: eng.pic_alloc(p) for k in host}
    eng.pic_upload(ids[0], host[0])
    arr = host_pic_array(host)
    plan = [(1, 0, [0]), (2, 1, [0, 1]), (3, 2, [1, 2])]          # (cur, slice_type idx, refs): I? no: P, B, B chain
    for cur, st, refs in plan:
        f = rec.synth(F.synth_params(1 if len(refs) == 1 else 2, 500 + cur), cur, refs)
        assert oracle().oh_or_frame(C.byref(f), arr) == 0
        df = eng.frame_upload(remap_frame(f, ids))
        eng.frame_execute(df)
        first = eng.pic_download(ids[cur], p)
        eng.frame_execute(df)
        again = eng.pic_download(ids[cur], p)
        eng.pic_upload(ids[cur], F.HostPic(p))        # an upload in between must not confuse which half is final
        eng.frame_execute(df)
        third = eng.pic_download(ids[cur], p)
        eng.frame_free(df)
        assert_same(host[cur], first, f"chain pic {cur}")
        assert_same(first, again, f"re-execute pic {cur}")
        assert_same(first, third, f"upload + re-execute pic {cur}")
    for v in ids.values():
        eng.pic_free(v)
    rec.close()


def test_1080p_b_and_i_pictures(eng):
    """BASELINE config[1] geometry: 1920x1080 Main 8-bit 4:2:0 (1080 is not a CTB multiple)"""
    p = F.pic_params(1920, 1080)
    rec = F.Recorder(p)
    rng = np.random.default_rng(9)
    refs = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng)}
    for st, seed in ((0, 1), (2, 2)):
        f = rec.synth(F.synth_params(st, seed), 2, [0, 1])
        pics = dict(refs)
        pics[2] = F.HostPic(p)
        want, got = run_both(eng, p, f, pics)
        assert_same(want, got, f"1080p slice_type {st}")
    rec.close()


@pytest.mark.parametrize("name,w,h,bd,chroma,seeds", [
    ("480p_main8", 832, 480, 8, 1, ((0, 19), (2, 20))),                 # BASELINE configs[0] geometry (BQMall_832x480 class; the stream itself is not available offline)
    ("2160p_main8", 3840, 2160, 8, 1, ((0, 24), (2, 25))),              # BASELINE configs[2]: 4K Main 8-bit
    ("2160p_main10", 3840, 2160, 10, 1, ((0, 21), (2, 22))),            # BASELINE configs[3] geometry, the bench workload
    ("4320p_444_10bit", 7680, 4320, 10, 3, ((2, 23), (0, 26))),          # BASELINE configs[4] geometry (range extension 4:4:4): B and I picture
])
def test_full_size_pictures(eng, name, w, h, bd, chroma, seeds):
    """BASELINE.json's full sizes, bit-exact against the oracle (a 4K picture costs the oracle ~0.3 s, the 8K 4:4:4 one a
    few seconds): the benchmark stream's own generator knobs"""
    from openhevc_amd import parallel as P
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma)
    rec = F.Recorder(p)
    rng = np.random.default_rng(31)
    refs = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng)}
    for st, seed in seeds:
        f = rec.synth(F.synth_params(st, seed, **P.default_synth_knobs()), 2, [0, 1])
        pics = dict(refs)
        pics[2] = F.HostPic(p)
        want, got = run_both(eng, p, f, pics)
        assert_same(want, got, f"{name} slice_type {st}")
    rec.close()


def test_malformed_work_lists_fail_on_the_host(eng):
    from openhevc_amd.engine import EngineError, remap_frame
    p = F.pic_params(128, 72)
    rec = F.Recorder(p)
    f = rec.synth(F.synth_params(2, 3), 2, [0, 1])
    ids = {k: eng.pic_alloc(p) for k in (0, 1, 2)}
    good = remap_frame(f, ids)
    # reference slot pointing at a picture that does not exist
    bad = remap_frame(f, ids)
    bad.ref_pics[0] = 99
    with pytest.raises(EngineError):
        eng.frame_submit(bad)
    # current picture used as its own reference
    bad = remap_frame(f, ids)
    bad.ref_pics[1] = ids[2]
    with pytest.raises(EngineError):
        eng.frame_submit(bad)
    # coefficient pool shorter than the TUs claim
    bad = remap_frame(f, ids)
    bad.n_coeff = 8
    with pytest.raises(EngineError):
        eng.frame_submit(bad)
    eng.frame_submit(good)
    eng.sync()
    # sparse records: a position outside the block, a matrix without scaling lists, a record running out of the pool
    fs = rec.synth(F.synth_params(2, 4, sparse_pct=100), 2, [0, 1])
    words = np.ctypeslib.as_array(fs.sparse, shape=(int(fs.n_sparse),)).copy()
    first = int(fs.tu_sparse[0])
    for mutate in ("position", "matrix", "count"):
        w = words.copy()
        if mutate == "position":
            w[first + 1] = (w[first + 1] & 0xffff0000) | 0x7fff
        elif mutate == "matrix":
            w[first] = (w[first] & 0x00ffffff) | (2 << 24)
        else:
            w[first] = (w[first] & 0xffff0000) | 0xffff
        bad = remap_frame(fs, ids)
        bad.sparse = w.ctypes.data_as(C.POINTER(C.c_uint32))
        with pytest.raises(EngineError):
            eng.frame_submit(bad)
    eng.frame_submit(remap_frame(fs, ids))
    eng.sync()
    # a work list uploaded to one engine cannot be executed by another (picture ids are per engine)
    from openhevc_amd.engine import Engine
    other = Engine(0)
    df = eng.frame_upload(remap_frame(f, ids))
    with pytest.raises(EngineError):
        other.frames_execute([df])
    eng.frame_free(df)
    other.close()
    for v in ids.values():
        eng.pic_free(v)
    rec.close()


def test_unordered_coefficient_pool(eng):
    """A work list whose coefficient blocks are NOT stored CTU by CTU (legal for the C ABI, never
    produced by the recorder): the intra kernel cannot stage a CTU's residual span in LDS and takes
    its slow path; results must not change."""
    p = F.pic_params(416, 240)
    rec = F.Recorder(p)
    f = rec.synth(F.synth_params(0, 31, cbf_pct=80), 2, [0, 1])
    n_tu = int(f.n_tu)
    tus = [(f.tu[i].coeff_off, 1 << (2 * f.tu[i].log2_size)) for i in range(n_tu)]
    src = np.ctypeslib.as_array(f.coeffs, shape=(int(f.n_coeff),)).copy()
    perm = np.random.default_rng(4).permutation(n_tu)
    dst = np.zeros_like(src)
    new_tu = (F.OhTu * n_tu)()
    C.memmove(new_tu, f.tu, C.sizeof(F.OhTu) * n_tu)
    pos = 0
    for i in perm:
        off, n2 = tus[i]
        dst[pos:pos + n2] = src[off:off + n2]
        new_tu[i].coeff_off = pos
        pos += n2
    g = F.OhFrame()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(F.OhFrame))
    g.tu = C.cast(new_tu, C.POINTER(F.OhTu))
    g.coeffs = dst.ctypes.data_as(C.POINTER(C.c_int16))
    rng = np.random.default_rng(0)
    pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
    want, got = run_both(eng, p, g, pics)
    assert_same(want, got, "unordered coefficient pool")
    rec.close()


@pytest.mark.parametrize("n,w,h,bd", [(5, 416, 240, 8), (35, 136, 88, 10)])
def test_batched_pictures(eng, n, w, h, bd):
    """oh_frames_execute: n independent pictures (I and B mixed, different numbers of wavefront levels,
    shared references) run as one launch per pass — each must equal the oracle's picture.  35 > the
    kernels' batch size: the engine splits the call."""
    from openhevc_amd.engine import remap_frame
    p = F.pic_params(w, h, bit_depth=bd)
    rec = F.Recorder(p)
    rng = np.random.default_rng(11)
    refs = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng)}
    ids = {k: eng.pic_alloc(p) for k in refs}
    for k, hp in refs.items():
        eng.pic_upload(ids[k], hp)
    dfs, want, cur_ids = [], [], []
    for i in range(n):
        st = 0 if i % 4 == 1 else 2
        f = rec.synth(F.synth_params(st, 9100 + i, intra_pct=10 + 5 * (i % 7)), 2, [0, 1])
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
    for i in range(n):
        assert_same(want[i], eng.pic_download(cur_ids[i], p), f"batched picture {i}")
    for df in dfs:
        eng.frame_free(df)
    for v in list(ids.values()) + cur_ids:
        eng.pic_free(v)
    rec.close()


def test_shvc_upsample_pictures(eng):
    """oh_pic_upsample against the MD5s recorded from the reference's
    upsample_base_layer_frame slot, and the resampled picture used as a reference by a B picture"""
    from test_golden import load_upsample_cases, md5_planes, upsample_inputs
    from openhevc_amd.engine import EngineError, remap_frame
    gold = load_upsample_cases()
    for case in gold["cases"]:
        u, bl, pe = upsample_inputs(case)
        b_id, e_id = eng.pic_alloc(bl.params), eng.pic_alloc(pe)
        eng.pic_upload(b_id, bl)
        eng.pic_upsample(e_id, b_id, u)
        eng.sync()
        got = eng.pic_download(e_id, pe)
        assert md5_planes(got) == gold["expected"][case[0]], case[0]
        if case[0] == "x2":                                 # inter-layer prediction: the EL picture predicts from it
            rec = F.Recorder(pe)
            f = rec.synth(F.synth_params(2, 4242), 2, [0, 1])
            rng = np.random.default_rng(3)
            other, cur = F.HostPic(pe, rng=rng), F.HostPic(pe, rng=rng)
            o_id, c_id = eng.pic_alloc(pe), eng.pic_alloc(pe)
            eng.pic_upload(o_id, other)
            eng.pic_upload(c_id, cur)
            eng.frame_submit(remap_frame(f, {0: e_id, 1: o_id, 2: c_id}))
            eng.sync()
            pics = {0: got.copy(), 1: other.copy(), 2: cur.copy()}
            assert oracle().oh_or_frame(C.byref(f), host_pic_array(pics)) == 0
            assert_same(pics[2], eng.pic_download(c_id, pe), "EL picture predicted from the up-sampled BL picture")
            eng.pic_free(o_id)
            eng.pic_free(c_id)
            rec.close()
        eng.pic_free(b_id)
        eng.pic_free(e_id)
    # on-demand granularity: a list of CTBs (what ff_upsample_block marks in is_upsampled[]) gives the whole-picture samples inside
    # those CTBs and leaves every other sample alone; all CTBs = the whole picture — for 64, 32 and 16 sample CTBs
    for case in gold["cases"]:
        u, bl, pe = upsample_inputs(case)
        if u.win_left or u.win_right or u.win_top or u.win_bottom:
            b_id, e_id = eng.pic_alloc(bl.params), eng.pic_alloc(pe)
            with pytest.raises(EngineError):                # the reference's own CTB path differs from its whole-picture slot there
                eng.pic_upsample_ctbs(e_id, b_id, u, 6, [0])
            eng.pic_free(b_id)
            eng.pic_free(e_id)
            continue
        b_id, whole, part = eng.pic_alloc(bl.params), eng.pic_alloc(pe), eng.pic_alloc(pe)
        eng.pic_upload(b_id, bl)
        eng.pic_upsample(whole, b_id, u)
        want = eng.pic_download(whole, pe)
        for lc in (6, 5, 4):
            ctb = 1 << lc
            cw, ch = (pe.width + ctb - 1) >> lc, (pe.height + ctb - 1) >> lc
            rng = np.random.default_rng(lc)
            some = sorted(rng.choice(cw * ch, size=max(1, cw * ch // 3), replace=False).tolist())
            blank = F.HostPic(pe, fill=7)
            eng.pic_upload(part, blank)
            eng.pic_upsample_ctbs(part, b_id, u, lc, some)
            got = eng.pic_download(part, pe)
            for c in range(3):
                s = 1 if c else 0
                g, w_, mask = got.visible(c), want.visible(c), np.zeros(got.visible(c).shape, bool)
                for a in some:
                    x0, y0 = (a % cw) * (ctb >> s), (a // cw) * (ctb >> s)
                    mask[y0:y0 + (ctb >> s), x0:x0 + (ctb >> s)] = True
                assert np.array_equal(g[mask], w_[mask]) and (g[~mask] == 7).all(), (case[0], lc, c)
            eng.pic_upsample_ctbs(part, b_id, u, lc, [a for a in range(cw * ch) if a not in some])
            assert md5_planes(eng.pic_download(part, pe)) == gold["expected"][case[0]], (case[0], lc)
            eng.pic_upsample_ctbs(part, b_id, u, lc, [])                     # an empty list is nothing to do
        for i in (b_id, whole, part):
            eng.pic_free(i)
    # the reference's routine is 8-bit only: a 10-bit request is refused, not approximated
    p10 = F.pic_params(416, 240, bit_depth=10)
    a, b = eng.pic_alloc(p10), eng.pic_alloc(p10)
    with pytest.raises(EngineError):
        eng.pic_upsample(a, b, F.upsample_setup(416, 240, 416, 240))
    eng.pic_free(a)
    eng.pic_free(b)


def _random_up_geometries(seed, count):
    """(base layer size, enhancement layer size, scaled reference layer offsets, phase alignment): ratios 1 .. 2, sizes in units of 8"""
    import random
    rng = random.Random(seed)
    for _ in range(count):
        wb, hb = 8 * rng.randint(4, 60), 8 * rng.randint(3, 40)
        r = rng.choice([1.0, 1.5, 2.0, rng.uniform(1.0, 2.0), rng.uniform(1.0, 2.0)])
        we, he = max(wb, int(wb * r) // 8 * 8), max(hb, int(hb * r) // 8 * 8)
        win = tuple(2 * rng.randint(0, 6) if rng.random() < 0.5 else 0 for _ in range(4))
        if we - win[0] - win[1] < wb or he - win[2] - win[3] < hb:
            win = (0, 0, 0, 0)
        yield (wb, hb), (we, he), win, rng.choice([0, 0, 1])


def test_shvc_upsample_random_geometries(eng):
    """oh_pic_upsample over random base / enhancement layer geometries (ratios 1 .. 2, scaled reference layer offsets, phase
    alignment) against the checker — which tests/test_upsample_vs_ref.py holds against the reference's slot on the same sweep"""
    from oracle_lib import OhHostPicC
    n = 0
    for (wb, hb), (we, he), win, pa in _random_up_geometries(4711, 60):
        u = F.upsample_setup(wb, hb, we, he, win, pa)
        pb, pe = F.pic_params(wb, hb), F.pic_params(we, he)
        bl = F.HostPic(pb, rng=np.random.default_rng(n))
        want = F.HostPic(pe, fill=0)

        def as_c(p, hp):
            c_ = OhHostPicC()
            for c, pl in enumerate(hp.planes):
                w, h = F.plane_dims(p, c)
                c_.data[c], c_.stride[c], c_.width[c], c_.height[c] = pl.ctypes.data, pl.strides[0], w, h
            c_.bit_depth = 8
            return c_
        b_c, e_c = as_c(pb, bl), as_c(pe, want)
        assert oracle().oh_or_upsample_frame(C.byref(b_c), C.byref(e_c), C.byref(u)) == 0
        b_id, e_id = eng.pic_alloc(pb), eng.pic_alloc(pe)
        eng.pic_upload(b_id, bl)
        eng.pic_upsample(e_id, b_id, u)
        eng.sync()
        assert_same(want, eng.pic_download(e_id, pe), f"up-sampling {wb}x{hb} -> {we}x{he} offsets {win} phase alignment {pa}")
        eng.pic_free(b_id)
        eng.pic_free(e_id)
        n += 1
    assert n == 60


@pytest.mark.parametrize("seed,count,max_w8,max_h8", [(20261004, 40, 34, 26), (20261005, 10, 160, 90)],
                         ids=["40_small", "10_up_to_1280x720"])
def test_random_configurations(eng, seed, count, max_w8, max_h8):
    """seeded sweep over geometry x bit depth x chroma format x CTB size x tool switches x generator knobs:
    every picture must match the oracle bit for bit (catches interactions the hand-picked cases miss)"""
    rng = np.random.default_rng(seed)
    n_checked = 0
    for it in range(count):
        chroma = int(rng.choice([0, 1, 1, 1, 2, 3]))
        bd = int(rng.choice([8, 8, 10, 10, 12]))
        lc = int(rng.choice([4, 5, 6]))
        w, h = 8 * int(rng.integers(2, max_w8)), 8 * int(rng.integers(2, max_h8))
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
                     ccp_pct=int(rng.choice([0, 50])) if chroma == 3 else 0, bs_from_motion=int(rng.integers(0, 3) == 0))
        rec = F.Recorder(p)
        f = rec.synth(F.synth_params(st, 555000 + it + seed % 1000, **knobs), 2, [0, 1] if st else [])
        prng = np.random.default_rng(it)
        pics = {0: F.HostPic(p, rng=prng), 1: F.HostPic(p, rng=prng), 2: F.HostPic(p, rng=prng)}
        want, got = run_both(eng, p, f, pics)
        assert_same(want, got, f"random configuration {it}: {w}x{h} {bd} bit chroma {chroma} ctb {1 << lc} slice {st} "
                               f"pcm {pcm} bypass {byp} cip {cip} knobs {knobs}")
        n_checked += 1
        rec.close()
    assert n_checked == count


def test_output_window_download(eng):
    """oh_pic_download_window against the reference's output arithmetic restated with numpy slices:
    ff_hevc_output_frame advances plane i by (left >> hshift) samples and (top >> vshift) rows (hevc_refs.c:248-254),
    libOpenHevcGetOutputCpy then copies `height >> vshift` rows of `(width >> hshift) << pixel_shift` bytes with width / height
    = the cropped size (openHevcWrapper.c:353-398, pitches from libOpenHevcGetPictureInfoCpy :245-300)."""
    from openhevc_amd.engine import EngineError
    rng = np.random.default_rng(11)
    for (w, h, bd, cf), (l, r, t, b), pad in [((416, 240, 8, 1), (0, 0, 0, 0), 0), ((416, 240, 8, 1), (8, 16, 2, 6), 0),
                                              ((416, 240, 10, 2), (4, 2, 1, 3), 64), ((192, 128, 12, 3), (3, 5, 7, 9), 0),
                                              ((192, 128, 8, 0), (64, 0, 0, 64), 32), ((1920, 1080, 10, 1), (0, 0, 0, 8), 0)]:
        p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)
        hp = F.HostPic(p, rng=rng)
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        got = eng.pic_download_window(pid, p, l, r, t, b, pad=pad)
        W, H = w - l - r, h - t - b
        for c, pl in enumerate(got):
            hs, vs = (1 if c and cf in (1, 2) else 0), (1 if c and cf == 1 else 0)
            pw = F.plane_dims(p, c)[0]
            want = hp.planes[c][:, :pw][t >> vs:(t >> vs) + (H >> vs), l >> hs:(l >> hs) + (W >> hs)]
            assert pl.shape == want.shape and np.array_equal(pl, want), (w, h, bd, cf, l, r, t, b, c)
        with pytest.raises(EngineError):                    # a window that leaves nothing is refused
            eng.pic_download_window(pid, p, w // 2, w // 2, 0, 0)
        eng.pic_free(pid)


FORCED_CONFIGS = [(416, 240, 8, 1, 6, 0, {}), (416, 240, 10, 1, 6, 2, {"intra_pct": 60}), (200, 136, 10, 3, 5, 0, {"split_pct": 90}),
                  (416, 240, 8, 2, 4, 0, {"split_pct": 10}), (1920, 1080, 10, 1, 6, 0, {})]


def run_forced(**switches):
    """I / B pictures of several formats, with and without large blocks, through an engine created with these switches
    (tests/forced_engine.py)"""
    with forced_engine(**switches) as e:
        for w, h, bd, cf, lc, st, knobs in FORCED_CONFIGS:
            p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf, log2_ctb_size=lc)
            rec = F.Recorder(p)
            f = rec.synth(F.synth_params(st, 77, **knobs), 2, [0, 1])
            rng = np.random.default_rng(5)
            pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
            want, got = run_both(e, p, f, pics)
            assert_same(want, got, f"{w}x{h} {bd}-bit chroma {cf} ctb {lc}")
            rec.close()


@pytest.mark.parametrize("waves,phases", [(2, 2), (4, 2), (8, 2), (4, 4), (8, 4), (8, 8)])
def test_intra_wave_layouts(waves, phases):
    """the intra kernel deals the sub-levels of a CTU to `phases` groups of its waves; the engine picks 2 / 4 / 8 waves per
    launch from the content and 2 phases.  Force every layout over I / B pictures of several formats, with and without large
    blocks."""
    run_forced(OHEVC_INTRA_WAVES=waves, OHEVC_INTRA_PHASES=phases)


@pytest.mark.parametrize("mode", ["dag", "direct"])
def test_intra_pass_forms(mode):
    """The intra pass of a picture runs in one launch — a wave per CTU on the picture in HBM (`direct`: pictures with few intra blocks)
    or a workgroup per CTU staged in LDS (`dag`), CTUs waiting for their neighbours' flags.  The engine chooses per picture;
    OHEVC_INTRA_MODE forces one form for every picture: I and B pictures of several formats through each."""
    run_forced(OHEVC_INTRA_MODE=mode)


_GIVE_UP_SCRIPT = r"""
import sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import numpy as np
from openhevc_amd import frame as F
from openhevc_amd.engine import Engine, EngineError, remap_frame
eng = Engine(0)
p = F.pic_params(1920, 1080, bit_depth=8)
rec = F.Recorder(p)
f = rec.synth(F.synth_params(0, 5), 0, [])
pid = eng.pic_alloc(p)
eng.pic_upload(pid, F.HostPic(p))
eng.frame_submit(remap_frame(f, {{0: pid}}))
try:
    eng.sync()
    print("no error reported")
except EngineError as exc:
    msg = str(exc)
    print("reported:", msg)
    assert "gave up" in msg and "picture" in msg, msg
    eng.sync()                      # reported once: the engine goes on
    print("ok")
eng.close()
"""


@pytest.mark.parametrize("mode", ["dag", "direct"])
def test_intra_wait_that_gives_up_is_reported(mode):
    """A CTU that waits for its neighbours polls a bounded number of times; when it gives up, the kernel latches
    picture and schedule entry in the engine's error word and oh_engine_sync fails with them — never a silently wrong
    picture.  OHEVC_SPIN_LIMIT=1 makes every wait give up at its first unsuccessful poll: a 1080p I picture (hundreds of dependent CTUs)
    cannot get through without one."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, OHEVC_INTRA_MODE=mode, OHEVC_SPIN_LIMIT="1")
    r = subprocess.run([sys.executable, "-c", _GIVE_UP_SCRIPT.format(tests=here, root=os.path.dirname(here))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("res_lds", [0, 1])
def test_intra_residual_staging(res_lds):
    """The staged form (intra_dag_kernel) stages the CTUs' residual spans in LDS in launches the chip holds at once and fetches them
    per block from HBM in the prepare stage in wider ones; OHEVC_INTRA_RES_LDS forces one way.  Both over the same I / B pictures,
    every picture through the staged form."""
    run_forced(OHEVC_INTRA_MODE="dag", OHEVC_INTRA_RES_LDS=res_lds)


@pytest.mark.parametrize("w,h,bd,lc,lcb,seed", [(416, 240, 8, 6, 3, 1), (416, 240, 10, 4, 3, 2), (200, 136, 8, 5, 3, 3), (1920, 1080, 10, 6, 3, 4),
                                                (272, 144, 8, 6, 4, 5), (3840, 2160, 10, 6, 3, 6)])
def test_boundary_strengths_from_motion_field(eng, w, h, bd, lc, lcb, seed):
    """with OhFrame.bs_in the engine derives both BS grids on the GPU (bs_kernel) — they must equal the CPU
    checker's grids (oh_or_bs_derive, itself pinned against the reference's ff_hevc_deblocking_boundary_strengths in
    tests/test_bs_derive.py), and the picture decoded with them must equal the picture decoded with those grids handed over."""
    from bs_inputs import as_struct, make_inputs
    from openhevc_amd.engine import remap_frame
    p = F.pic_params(w, h, bit_depth=bd, log2_ctb_size=lc, log2_min_cb_size=lcb)
    fn = oracle().oh_or_bs_derive
    fn.argtypes, fn.restype = [C.c_void_p] * 4, C.c_int
    rec = F.Recorder(p)
    rng = np.random.default_rng(seed)
    pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
    ids = {k: eng.pic_alloc(p) for k in pics}
    for k, hp in pics.items():
        eng.pic_upload(ids[k], hp)
    for k in range(2):
        maps = make_inputs(p, 100 * seed + k, intra_pct=(10, 35)[k])
        bs_in = as_struct(*maps)
        n = F.bs_size(p)
        want_v, want_h = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        assert fn(C.byref(p), C.byref(bs_in), want_v.ctypes.data, want_h.ctypes.data) == 0
        f = rec.synth(F.synth_params(2, 9000 + seed + k), 2, [0, 1])
        # (a) the grids handed over (= the checker's), (b) derived on the GPU from the maps
        fa = remap_frame(f, ids)
        C.memmove(fa.vertical_bs, want_v.ctypes.data, min(n, fa.bs_size))
        C.memmove(fa.horizontal_bs, want_h.ctypes.data, min(n, fa.bs_size))
        eng.pic_upload(ids[2], pics[2])
        eng.frame_submit(fa)
        eng.sync()
        pic_a = eng.pic_download(ids[2], p)
        fb = remap_frame(f, ids)
        fb.bs_in = C.addressof(bs_in)
        fb.vertical_bs = fb.horizontal_bs = None
        eng.pic_upload(ids[2], pics[2])
        df = eng.frame_upload(fb)
        got_v, got_h = eng.frame_download_bs(df, p)
        assert np.array_equal(got_v, want_v), f"vertical grid: {np.nonzero(got_v != want_v)[0][:8]}"
        assert np.array_equal(got_h, want_h), f"horizontal grid: {np.nonzero(got_h != want_h)[0][:8]}"
        eng.frame_execute(df)
        eng.sync()
        assert_same(pic_a, eng.pic_download(ids[2], p), f"{w}x{h} picture decoded with derived vs handed-over strengths")
        chk = {k_: v_.copy() for k_, v_ in pics.items()}        # and the checker takes the same work list (derives the grids itself)
        fo = remap_frame(f, {0: 0, 1: 1, 2: 2})
        fo.bs_in, fo.vertical_bs, fo.horizontal_bs = C.addressof(bs_in), None, None
        assert oracle().oh_or_frame(C.byref(fo), host_pic_array(chk)) == 0
        assert_same(chk[2], pic_a, f"{w}x{h} checker with bs_in")
        eng.frame_free(df)
        assert {0, 1, 2} <= set(np.unique(got_v)) | set(np.unique(got_h))
        if k == 0:                                          # a block size the picture cannot have is refused on the host
            from openhevc_amd.engine import EngineError
            bad = maps[2].copy()
            bad[0, 0] = 9
            bad_in = as_struct(maps[0], maps[1], bad, maps[3], maps[4])
            fb.bs_in = C.addressof(bad_in)
            with pytest.raises(EngineError):
                eng.frame_upload(fb)
    for v in ids.values():
        eng.pic_free(v)
    rec.close()


@pytest.mark.parametrize("w,h,lc,bd,chroma", [(416, 240, 6, 8, 1), (16, 16, 4, 10, 1), (8, 8, 4, 8, 0), (24, 8, 4, 12, 3), (64, 64, 6, 8, 2)])
def test_empty_and_minimal_work_lists(eng, w, h, lc, bd, chroma):
    """edge cases: a work list with no blocks at all (the picture only passes through the in-loop filters, whose grids are
    all zero), the smallest pictures the format allows (one min coding block; a single partial CTB), and an empty batch"""
    from openhevc_amd.engine import remap_frame
    p = F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc)
    rec = F.Recorder(p)
    lib = F.host()
    refs = (C.c_int32 * F.OH_MAX_REFS)(*([0, 1] + [-1] * (F.OH_MAX_REFS - 2)))
    lib.oh_rec_begin(rec.h, 2, refs, F.OH_MAX_REFS)
    f = lib.oh_rec_finish(rec.h).contents                  # nothing recorded
    assert (f.n_pu, f.n_tu, f.n_intra) == (0, 0, 0)
    rng = np.random.default_rng(w + h)
    pics = {0: F.HostPic(p, rng=rng), 1: F.HostPic(p, rng=rng), 2: F.HostPic(p, rng=rng)}
    want, got = run_both(eng, p, f, pics)
    assert_same(want, got, f"empty work list {w}x{h}")
    assert_same(pics[2], got, "no block, zero strengths, SAO off everywhere: the picture is unchanged")
    for st in (0, 2):                                       # and a full synthetic picture of the same minimal geometry
        g = rec.synth(F.synth_params(st, 31 + st), 2, [0, 1] if st else [])
        want, got = run_both(eng, p, g, pics)
        assert_same(want, got, f"minimal picture {w}x{h} slice type {st}")
    eng.frames_execute([])                                  # an empty batch is a no-op
    eng.sync()
    rec.close()
