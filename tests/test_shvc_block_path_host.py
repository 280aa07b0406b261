"""SHVC up-sampling along the reference's CTB path (its default build, ACTIVE_PU_UPSAMPLING): where its output is defined
(oh_upsample_blocks_defined, host only) and the two-layer writer's option for it (oh_stream_write_opts)."""
import ctypes as C

import pytest

import refdec
import streamgen
from openhevc_amd import frame as F
from openhevc_amd.engine import EngineError, upsample_blocks_defined
from oracle_lib import have_ref

OH_STREAM_SHVC_BLOCK_PATH = 1


def defined(bl, el, lc, win=(0, 0, 0, 0), pa=0):
    return upsample_blocks_defined(F.upsample_setup(*bl, *el, win, pa), *bl, *el, lc)


@pytest.mark.parametrize("lc", [4, 5, 6])
@pytest.mark.parametrize("bl,el", [((2560, 1440), (3840, 2160)), ((5120, 2880), (7680, 4320)), ((1376, 128), (2064, 192))])
def test_x1_5_beyond_2048_is_defined(bl, el, lc):
    assert F.upsample_setup(*bl, *el).idx == F.OH_UP_X1_5
    assert defined(bl, el, lc) == (True, -1)


@pytest.mark.parametrize("bl,el,lc", [((208, 120), (416, 240), 6), ((208, 120), (416, 240), 4), ((176, 96), (264, 144), 5),
                                      ((264, 144), (264, 144), 6), ((200, 112), (328, 200), 5), ((960, 544), (1920, 1088), 6)])
def test_geometries_where_the_reference_paths_agree_are_defined(bl, el, lc):
    """every geometry of test_upsample_vs_ref.py::test_pu_driven_block_path_equals_whole_picture_slot"""
    assert defined(bl, el, lc) == (True, -1)


def test_offsets_and_phase_alignment():
    """the geometries of test_upsample_vs_ref.py::test_reference_paths_disagree_with_offsets_or_phase_alignment (CTB 64).
    Phase alignment alone is defined: the x2 slots ignore the phase, deterministically.  With scaled reference layer offsets
    (8, 8, 8, 8) the driver sizes its window from the CTB position without the offsets (hevc_filter.c:1257-1258) while the
    vertical slot positions by y - top_offset: CTB 6 (first CTB of the second row) reads intermediate rows its call never
    filtered, scratch of an earlier call, so that picture is not defined and is refused."""
    assert defined((208, 120), (416, 240), 6, pa=1) == (True, -1)
    assert defined((200, 112), (416, 240), 6, win=(8, 8, 8, 8)) == (False, 6)


def test_undefined_geometries_are_rejected():
    # a single CTB row: the top edge is emulated, so the bottom one is not (videodsp_template.c:141-151)
    assert defined((64, 32), (128, 64), 6) == (False, 0)
    # vertical ratio above 2: the driver's chroma base-layer height (hevc_filter.c:1252) is larger than the base layer's chroma plane
    assert defined((64, 64), (144, 144), 6)[0] is False
    # test_upsample_vs_ref.py::test_reference_paths_disagree_for_some_generic_ratios: the window estimate is a row short there
    assert defined((240, 120), (416, 200), 5)[0] is False
    assert defined((96, 240), (128, 464), 6)[0] is False


def test_horizontal_ratio_above_2_is_deterministic():
    """64x64 -> 144x128 (x2.25 horizontally, x2 vertically): the short width estimate only decides whether the right edge is
    emulated; every column the slots read lies in the base layer or in the replicated right edge of the same call, and the
    vertical ratio 2 keeps the chroma height of hevc_filter.c:1252 inside the plane.  So the reference's output is defined there
    (the GPU test checks the engine against the reference at this geometry); x2.25 in both directions is not."""
    assert defined((64, 64), (144, 128), 6) == (True, -1)
    assert defined((64, 64), (144, 128), 4) == (True, -1)


def test_scale_above_one_and_bad_arguments():
    assert defined((416, 240), (208, 120), 6) == (False, -1)          # EL smaller than BL
    with pytest.raises(EngineError):
        defined((208, 120), (416, 240), 7)


def write_stream_opts(width, height, seed, opts, **kw):
    """streamgen.write_stream through oh_stream_write_opts"""
    H = streamgen._lib()
    H.oh_stream_write_opts.argtypes = [C.POINTER(streamgen.OhStreamParams), C.c_uint, C.POINTER(streamgen.OhStream)]
    sp = streamgen.OhStreamParams()
    H.oh_stream_defaults(C.byref(sp), width, height, seed)
    for k, v in kw.items():
        assert hasattr(sp, k), k
        setattr(sp, k, v)
    st = streamgen.OhStream()
    rc = H.oh_stream_write_opts(C.byref(sp), opts, C.byref(st))
    if rc:
        raise ValueError(f"oh_stream_write_opts refused the parameters ({rc})")
    data = bytes(C.string_at(st.data, st.size))
    aus = [(st.au_offset[i], st.au_offset[i + 1]) for i in range(st.n_pictures)]
    H.oh_stream_free(C.byref(st))
    return data, aus


def test_writer_option_lifts_the_x1_5_limit():
    kw = dict(n_pictures=2, gop=1, shvc_el_width=2112, shvc_el_height=192)
    with pytest.raises(ValueError):
        streamgen.write_stream(1408, 128, 71, **kw)
    with pytest.raises(ValueError):
        write_stream_opts(1408, 128, 71, 2, **kw)                   # unknown option bit
    with pytest.raises(ValueError):
        write_stream_opts(1408, 128, 71, 0, **kw)                   # opts = 0 is oh_stream_write
    small = dict(n_pictures=2, gop=1, shvc_el_width=144, shvc_el_height=96)
    assert write_stream_opts(96, 64, 71, 0, **small) == streamgen.write_stream(96, 64, 71, **small)
    data, aus = write_stream_opts(1408, 128, 71, OH_STREAM_SHVC_BLOCK_PATH, **kw)
    assert len(aus) == 2


@pytest.mark.skipif(not have_ref(), reason="reference decoder not built")
def test_reference_decodes_both_layers_of_a_wide_x1_5_stream():
    data, _ = write_stream_opts(1408, 128, 71, OH_STREAM_SHVC_BLOCK_PATH, n_pictures=2, gop=1, shvc_el_width=2112, shvc_el_height=192)
    with refdec.captured_stderr() as cap:
        pics = refdec.decode(data)
    assert "rror" not in cap.text.replace("Could not find ref with POC", ""), cap.text[-1500:]
    assert [p[0].shape for p in pics] == [(192, 2112)] * 2
    got = []
    n = refdec.record_layer_work_lists(data, lambda layer, f, cur, poc, il: got.append((layer, il is not None)))
    assert n == [2, 2] and got == [(0, False), (1, True)] * 2
