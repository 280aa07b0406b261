"""The host-only functions of the frame packing service (openhevc_amd/csrc/pics_math.hip: oh_packing_from_sei, oh_packing_view_size,
oh_packing_sample, oh_packing_pack_sample, oh_packing_views) through ctypes against tests/packing_model.py, every refusal included, and
tests/packing_math_check.cpp, which runs them over heap blocks of exactly the sizes they may touch as a stand-alone program built with
AddressSanitizer and UBSan — no GPU, nothing of the sanitizers loaded into Python."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import packing_model as M
from openhevc_amd import annexb as A
from openhevc_amd import engine as E
from openhevc_amd import frame as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_packing_math_under_sanitizers(tmp_path):
    exe = str(tmp_path / "packing_math_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "packing_math_check.cpp"), os.path.join(ROOT, "openhevc_amd", "csrc", "pics_math.hip"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("packing math ok"), r.stdout + r.stderr
    assert len(r.stdout.splitlines()) == 4                               # one line per group, then the verdict


def params(w, h, bd=8, cf=1):
    p = F.pic_params(w, h)
    p.bit_depth, p.chroma_format_idc = bd, cf
    return p


def planes_of(rng, w, h, bd, cf):
    out = []
    for c in range(3 if cf else 1):
        hs, vs = M.shifts(cf, c)
        out.append(rng.integers(0, 1 << bd, (h >> vs, w >> hs)).astype(np.uint8 if bd == 8 else np.uint16))
    return out


def want_view(packing, planes, p, v, c, full):
    """the coded plane c of view v by the model"""
    sbs = packing.arrangement == M.SBS
    g = packing.grid[v][0 if sbs else 1]
    win = M.unpack_plane(planes[c], packing.arrangement, v, flip=packing.flip[v], g=g, quincunx=packing.quincunx, full=full, plane=c,
                         chroma_format_idc=p.chroma_format_idc, bit_depth=p.bit_depth)
    vp = packing.view_size(p, full)
    hs, vs = M.shifts(p.chroma_format_idc, c)
    return M.coded(win, vp.height >> vs, vp.width >> hs)


@pytest.mark.parametrize("arr", [M.SBS, M.TB])
@pytest.mark.parametrize("bd,cf", [(8, 1), (10, 2), (12, 3), (8, 0)])
def test_sample_against_the_model(arr, bd, cf):
    rng = np.random.default_rng(arr * 100 + bd + cf)
    p = params(24, 16, bd, cf)
    planes = planes_of(rng, 24, 16, bd, cf)
    cases = [dict(), dict(flip=(True, False), grid=((5, 3), (14, 9))), dict(flip=(False, True), grid=((8, 0), (0, 8))), dict(quincunx=True),
             dict(quincunx=True, flip=(True, True))]
    for kw in cases:
        pk = E.make_packing(arr, **kw)
        for full in (False, True):
            for v in range(2):
                for c in range(len(planes)):
                    want = want_view(pk, planes, p, v, c, full)
                    got = np.array([[pk.sample(p, planes[c], v, c, x, y, full=full) for x in range(want.shape[1])] for y in range(want.shape[0])])
                    assert np.array_equal(got, want), (kw, full, v, c)


@pytest.mark.parametrize("arr", [M.SBS, M.TB])
def test_pack_sample_against_the_model(arr):
    rng = np.random.default_rng(arr)
    p = params(16, 8, 10, 1)
    for quincunx, flip in itertools.product((False, True), itertools.product((False, True), repeat=2)):
        pk = E.make_packing(arr, quincunx=quincunx, flip=flip)
        for c in range(3):
            hs, vs = M.shifts(1, c)
            pw, ph = 16 >> hs, 8 >> vs
            vw, vh = (pw, ph) if quincunx else (pw // 2, ph) if arr == M.SBS else (pw, ph // 2)
            views = [rng.integers(0, 1024, (vh, vw)).astype(np.uint16) for _ in range(2)]
            want = M.pack_plane(views[0], views[1], arr, flip=flip, quincunx=quincunx)
            got = np.array([[pk.pack_sample(p, views[0], views[1], c, x, y) for x in range(pw)] for y in range(ph)])
            assert np.array_equal(got, want), (quincunx, flip, c)


def test_from_sei_fills_the_descriptor():
    def sei(**kw):
        d = dict(id=0, cancel=False, arrangement_type=3, quincunx_sampling=False, content_interpretation_type=1, grid=((0, 0), (8, 0)))
        d.update(kw)
        return d

    pk = E.packing_from_sei(sei())
    assert (pk.arrangement, pk.quincunx, pk.flip, pk.grid, pk.content_interpretation) == (3, False, (False, False), ((0, 0), (8, 0)), 1)
    assert pk.views() == (0, 1)
    # spatial_flipping_flag with frame0_flipped_flag: frame 0 is the mirrored one; without: frame 1
    assert E.packing_from_sei(sei(spatial_flipping=True, frame0_flipped=True)).flip == (True, False)
    assert E.packing_from_sei(sei(spatial_flipping=True)).flip == (False, True)
    assert E.packing_from_sei(sei(frame0_flipped=True)).flip == (False, False)
    pk = E.packing_from_sei(sei(arrangement_type=4, quincunx_sampling=True, content_interpretation_type=2, grid=((0, 0), (0, 0))))
    assert (pk.arrangement, pk.quincunx, pk.views()) == (4, True, (1, 0))
    assert E.packing_from_sei(sei(content_interpretation_type=0)).views() is None
    assert E.packing_from_sei(sei(content_interpretation_type=3)).views() is None
    # the flags that change no sample are passed over
    assert E.packing_from_sei(sei(current_frame_is_frame0=True, frame0_self_contained=True, frame1_self_contained=True)).flip == (False, False)
    # parsed from bytes: id 0, not cancelled, type 3, cit 1, no flags, grid (0, 0), (8, 0), reserved 0, persistence 1, aspect 0
    bits = "1" + "0" + format(3, "07b") + "0" + format(1, "06b") + "000000" + "0000" "0000" "1000" "0000" + "00000000" + "1" + "0" + "1"
    bits += "0" * (-len(bits) % 8)
    payload = int(bits, 2).to_bytes(len(bits) // 8, "big")
    nal = bytes([39 << 1, 1, 45, len(payload)]) + payload + b"\x80"
    assert b"\x00\x00" not in nal[2:]
    pk = E.packing_from_sei(A.frame_packing(nal))
    assert (pk.arrangement, pk.grid, pk.views()) == (3, ((0, 0), (8, 0)), (0, 1))


@pytest.mark.parametrize("kw,code,word", [
    (dict(arrangement_type=5), E.OH_E_UNSUPPORTED, "temporal interleaving"),
    (dict(arrangement_type=0), E.OH_E_UNSUPPORTED, "does not define"),
    (dict(arrangement_type=2), E.OH_E_UNSUPPORTED, "does not define"),
    (dict(arrangement_type=6), E.OH_E_UNSUPPORTED, "does not define"),
    (dict(arrangement_type=127), E.OH_E_UNSUPPORTED, "does not define"),
    (dict(arrangement_type=3, field_views=True), E.OH_E_UNSUPPORTED, "field_views_flag"),
    (dict(arrangement_type=4, cancel=True), E.OH_E_ARG, ""),
])
def test_from_sei_refusals(kw, code, word):
    d = dict(id=0, cancel=False, quincunx_sampling=False, content_interpretation_type=1)
    d.update(kw)
    with pytest.raises(E.EngineError) as err:
        E.packing_from_sei(d)
    assert err.value.code == code and word in str(err.value)
    with pytest.raises(ValueError):
        E.packing_from_sei(None)


def test_view_size_and_its_refusals():
    p = params(80, 24, 10, 1)
    sbs, tb = E.make_packing("side_by_side"), E.make_packing("top_bottom")
    for pk, full, want in ((sbs, False, (40, 24)), (sbs, True, (80, 24)), (tb, False, (80, 16)), (tb, True, (80, 24))):
        vp = pk.view_size(p, full)
        assert (vp.width, vp.height) == want and (vp.bit_depth, vp.chroma_format_idc, vp.log2_min_cb_size) == (10, 1, p.log2_min_cb_size)
        assert M.view_size(80, 24, pk.arrangement, full)[2:] == want
    # the smallest picture: half of 8 is 4, which rounds up to the full size
    q = params(8, 8)
    assert [(sbs.view_size(q, f).width, sbs.view_size(q, f).height) for f in (False, True)] == [(8, 8), (8, 8)]
    # each half a whole number of chroma samples
    for cf, w, ok in ((1, 8, True), (1, 10, False), (1, 12, True), (3, 10, True), (3, 9, False), (2, 10, False), (0, 10, True)):
        r = params(8, 8, 8, cf)
        r.width = w
        if ok:
            sbs.view_size(r, False)
        else:
            with pytest.raises(E.EngineError) as err:
                sbs.view_size(r, False)
            assert err.value.code == E.OH_E_ARG
    for cf, h, ok in ((1, 12, True), (1, 10, False), (2, 10, True), (3, 9, False)):
        r = params(8, 8, 8, cf)
        r.height = h
        if ok:
            tb.view_size(r, True)
        else:
            with pytest.raises(E.EngineError):
                tb.view_size(r, True)
    for bad in (dict(grid=((16, 0), (0, 0))), dict(grid=((0, 0), (0, -1)))):
        with pytest.raises(E.EngineError) as err:
            E.make_packing(3, **bad).view_size(p)
        assert err.value.code == E.OH_E_ARG
    pk = E.make_packing(3)
    pk.arrangement = 5
    with pytest.raises(E.EngineError):
        pk.view_size(p)
    with pytest.raises(ValueError):
        E.make_packing("frame_sequence")


def test_sample_refusals():
    p = params(16, 8)
    pk = E.make_packing(3)
    a = np.zeros((8, 16), np.uint8)
    assert pk.sample(p, a, 1, 0, 7, 7, full=False) == 0
    for args in ((2, 0, 0, 0), (0, 3, 0, 0), (0, 0, 8, 0), (0, 0, 0, 8), (0, 0, -1, 0)):
        with pytest.raises(E.EngineError) as err:
            pk.sample(p, a, *args, full=False)
        assert err.value.code == E.OH_E_ARG
    with pytest.raises(E.EngineError):
        pk.sample(p, a[:, :8], 0, 0, 0, 0, full=False)       # rows shorter than the packed plane
    with pytest.raises(E.EngineError):
        pk.sample(params(16, 8, 8, 0), a, 0, 1, 0, 0)        # no chroma plane in a 4:0:0 picture
