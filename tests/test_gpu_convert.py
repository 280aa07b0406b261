"""-m gpu: oh_pics_convert / Engine.pics_convert on the MI355X against oh_pic_download_window and the numpy model of
tests/convert_model.py, bit for bit: YUV and RGB layouts over chroma formats, bit depths and windows, batches of more than one launch,
the finished half after SAO, the engine's replay of the recorded stream fixtures, ordering with torch streams and the argument rules."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import convert_model as M                                                   # noqa: E402
import device_room as DR                                                    # noqa: E402
import picture_hash as PH                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

RGB_FORMATS = ("rgb_planar", "rgb", "rgba")
RGB_DTYPES = ("uint8", "uint16", "float16", "float32")
SAMPLE_OF = {"uint8": E.CONV_U8, "uint16": E.CONV_U16, "float16": E.CONV_F16, "float32": E.CONV_F32}


def torch_dtype(name):
    import torch
    return getattr(torch, name)


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def random_pic(p, rng):
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        v[...] = rng.integers(0, 1 << p.bit_depth, v.shape, dtype=v.dtype)
    return hp


def coded(hp, p):
    return [hp.visible(c) for c in range(F.n_planes(p))]


def host(t):
    """a torch tensor as numpy, floats as their bits (exact comparison)"""
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32) if a.dtype == np.float32 else a


def bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32) if a.dtype == np.float32 else a


def upload(eng, p, n, rng):
    pids, hps = [], []
    for _ in range(n):
        hp = random_pic(p, rng)
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        pids.append(pid)
        hps.append(hp)
    return pids, hps


def check_yuv(eng, pids, p, win):
    """PLANAR / NATIVE = the downloaded window; SEMIPLANAR = it interleaved (MSB-aligned above 8 bit); U8 forms = the model"""
    l, r, t, b = win
    got_p = host(eng.pics_convert(pids, "planar", window=win))
    got_s = host(eng.pics_convert(pids, "semiplanar", window=win)) if p.chroma_format_idc else None
    got_p8 = host(eng.pics_convert(pids, "planar", dtype=torch_dtype("uint8"), window=win))
    for i, pid in enumerate(pids):
        planes = eng.pic_download_window(pid, p, l, r, t, b)
        assert np.array_equal(got_p[i].ravel(), np.concatenate([pl.ravel() for pl in planes])), i
        full = coded(eng.pic_download(pid, p), p)
        assert np.array_equal(got_p[i], M.convert(full, p, "planar", E.CONV_NATIVE, win)), i
        assert np.array_equal(got_p8[i], M.convert(full, p, "planar", E.CONV_U8, win)), i
        if got_s is not None:
            y, cb, cr = [pl.astype(np.int64) << (16 - p.bit_depth if p.bit_depth > 8 else 0) for pl in planes]
            want = np.concatenate([y.ravel(), np.stack([cb, cr], -1).ravel()])
            assert np.array_equal(got_s[i].ravel().astype(np.int64), want), i
            assert np.array_equal(host(eng.pics_convert([pid], "semiplanar", dtype=torch_dtype("uint8"), window=win))[0],
                                  M.convert(full, p, "semiplanar", E.CONV_U8, win)), i


YUV_CASES = [(64, 64, 8, 0, (0, 0, 0, 0)), (72, 40, 10, 0, (3, 1, 2, 5)), (416, 240, 8, 1, (2, 4, 0, 2)), (416, 240, 9, 1, (0, 0, 0, 0)),
             (1920, 1088, 10, 1, (0, 0, 0, 8)), (264, 200, 12, 1, (6, 2, 4, 8)), (264, 200, 9, 2, (2, 0, 1, 3)),
             (200, 136, 10, 2, (0, 0, 0, 0)), (200, 136, 12, 3, (1, 2, 3, 0)), (136, 72, 8, 3, (5, 0, 0, 1)), (24, 8, 10, 3, (0, 1, 0, 0)),
             (3840, 2160, 10, 1, (0, 0, 0, 0)), (7680, 4320, 8, 1, (0, 0, 0, 0)),
             # 4:4:4 wider than 2048: an interleaved CbCr row (NV24 / P410) holds twice the luma row's samples
             (2112, 64, 10, 3, (2, 0, 0, 0)), (2056, 32, 8, 3, (0, 0, 0, 0)), (4104, 16, 12, 2, (0, 0, 0, 0)),
             (3840, 2160, 8, 3, (0, 0, 0, 0)), (3840, 2160, 10, 3, (0, 0, 0, 0))]


@pytest.mark.parametrize("w,h,bd,cf,win", YUV_CASES, ids=[f"{c[0]}x{c[1]}_{c[2]}b_cf{c[3]}_win{'_'.join(map(str, c[4]))}" for c in YUV_CASES])
def test_yuv_formats_equal_the_download(w, h, bd, cf, win):
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, cf)
    eng = Engine(0)
    pids, _ = upload(eng, p, 1 if w * h > 4_000_000 else 3, np.random.default_rng(w + h + bd + cf))
    check_yuv(eng, pids, p, win)
    eng.close()


RGB_GEOMS = [(72, 40, 8, 0, (2, 0, 0, 2)), (72, 40, 10, 1, (2, 4, 2, 0)), (136, 72, 9, 1, (0, 0, 0, 0)), (104, 48, 12, 2, (2, 2, 1, 0)),
             (40, 24, 10, 3, (1, 0, 3, 2)), (72, 40, 8, 3, (0, 3, 0, 0))]


@pytest.mark.parametrize("w,h,bd,cf,win", RGB_GEOMS, ids=[f"{c[0]}x{c[1]}_{c[2]}b_cf{c[3]}" for c in RGB_GEOMS])
def test_every_rgb_form_equals_the_model(w, h, bd, cf, win):
    """every layout x sample type x matrix x range x filter; two pictures per call"""
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, cf)
    eng = Engine(0)
    pids, hps = upload(eng, p, 2, np.random.default_rng(bd * 7 + cf))
    for fmt, dt, matrix, fr, chroma in itertools.product(RGB_FORMATS, RGB_DTYPES, (1, 5, 6, 9), (False, True), ("linear", "nearest")):
        got = host(eng.pics_convert(pids, fmt, dtype=torch_dtype(dt), window=win, matrix=matrix, full_range=fr, chroma=chroma))
        for i, hp in enumerate(hps):
            want = bits(M.convert(coded(hp, p), p, fmt, SAMPLE_OF[dt], win, matrix, fr, chroma))
            assert got[i].shape == want.shape and np.array_equal(got[i], want), (fmt, dt, matrix, fr, chroma, i)
    eng.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("w,h,bd,forms", [
    (3840, 2160, 10, [("rgb", "uint8", 1, False, "linear"), ("rgb_planar", "float16", 9, True, "linear"),
                      ("rgba", "float32", 1, False, "nearest")]),
    (7680, 4320, 8, [("rgb", "uint8", 1, False, "linear")]),
    (1920, 1088, 8, [("rgb", "uint8", 1, False, "linear"), ("rgb_planar", "uint16", 5, False, "linear")]),
], ids=["2160p_main10", "4320p_main8", "1080p_main8"])
def test_large_pictures_to_rgb(w, h, bd, forms):
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, 1)
    win = (0, 0, 0, 8) if h == 1088 else (0, 0, 0, 0)
    eng = Engine(0)
    pids, hps = upload(eng, p, 1, np.random.default_rng(w))
    for fmt, dt, matrix, fr, chroma in forms:
        got = host(eng.pics_convert(pids, fmt, dtype=torch_dtype(dt), window=win, matrix=matrix, full_range=fr, chroma=chroma))
        want = bits(M.convert(coded(hps[0], p), p, fmt, SAMPLE_OF[dt], win, matrix, fr, chroma))
        assert np.array_equal(got[0], want), (fmt, dt)
    eng.close()


def test_more_pictures_than_one_launch():
    """150 pictures: three launches of at most OH_CONV_MAX_PICS; each image lands at its own offset"""
    import torch
    from openhevc_amd.engine import Engine
    p = params(48, 32, 10, 1)
    eng = Engine(0)
    n = 2 * E.CONV_MAX_PICS + 22
    pids, hps = upload(eng, p, n, np.random.default_rng(150))
    got = host(eng.pics_convert(pids, "rgb", dtype=torch.float32, window=(2, 0, 0, 2)))
    got_p = host(eng.pics_convert(pids[::-1], "planar"))
    for i in range(n):
        assert np.array_equal(got[i], bits(M.convert(coded(hps[i], p), p, "rgb", E.CONV_F32, (2, 0, 0, 2)))), i
        assert np.array_equal(got_p[n - 1 - i], M.convert(coded(hps[i], p), p, "planar", E.CONV_NATIVE)), i
    eng.close()


def test_conversion_follows_the_finished_half():
    """after a work list with SAO the finished picture lives in half 1: the conversion is of what oh_pic_download returns"""
    import torch
    from openhevc_amd.engine import Engine, remap_frame
    eng = Engine(0)
    rec = F.Recorder(params(416, 240, 8, 1))
    f = rec.synth(F.synth_params(0, 3, sao_pct=90), 0)
    pid = eng.pic_alloc(f.p)
    eng.frame_submit(remap_frame(f, {0: pid}))
    assert eng.pic_final_half(pid) == 1
    hp = eng.pic_download(pid, f.p)
    full = coded(hp, f.p)
    assert np.array_equal(host(eng.pics_convert([pid], "planar"))[0], M.convert(full, f.p, "planar", E.CONV_NATIVE))
    got = host(eng.pics_convert([pid], "rgb", dtype=torch.uint8, window=(0, 0, 0, 2)))[0]
    assert np.array_equal(got, M.convert(full, f.p, "rgb", E.CONV_U8, (0, 0, 0, 2)))
    eng.close()
    rec.close()


# ---- the recorded stream fixtures (tests/golden/streams: work lists recorded inside the reference decoder, MD5s of its output) ----
GOLD = os.path.join(HERE, "golden", "streams")
FIXTURES = [os.path.join(GOLD, n + ".npz") for n in ("ipb_8b", "b_hier_tmvp_idr_10b", "b_422_tools_8b", "i_444_ccp_10b_ctb16")]


def fixture(path):
    z = np.load(path)
    n = int(z["n_pictures"][0])
    frames = []
    for k in range(n):
        pre = f"pic{k}_"
        frames.append(F.FrameFromArrays({key[len(pre):]: z[key] for key in z.files if key.startswith(pre)}))
    return frames, z["md5"].tobytes()


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_stream_fixtures_convert_what_the_reference_decoded(path):
    """replay a fixture on the engine; the downloads match the fixture's MD5s (the reference's output), and the conversions of each
    finished picture equal the model of its download"""
    import torch
    from openhevc_amd.engine import Engine, remap_frame
    frames, want_md5 = fixture(path)
    eng = Engine(0)
    ids, md5 = {}, []
    for ff in frames:
        f = ff.frame
        for i in [f.cur_pic] + [f.ref_pics[k] for k in range(F.OH_MAX_REFS) if f.ref_pics[k] >= 0]:
            if i not in ids:
                ids[i] = eng.pic_alloc(f.p)
        eng.frame_submit(remap_frame(f, ids))
        pid = ids[f.cur_pic]
        rgb = eng.pics_convert([pid], "rgb", dtype=torch.uint8)
        planar = eng.pics_convert([pid], "planar")
        eng.sync()
        hp = eng.pic_download(pid, f.p)
        md5.append(b"".join(PH.host_pic_hash(hp, f.p, 0)[1]))
        full = coded(hp, f.p)
        assert np.array_equal(host(planar)[0], M.convert(full, f.p, "planar", E.CONV_NATIVE)), len(md5)
        assert np.array_equal(host(rgb)[0], M.convert(full, f.p, "rgb", E.CONV_U8)), len(md5)
    eng.close()
    assert b"".join(md5) == want_md5


# ---- ordering with torch ----
def _ordering(stream_of_engine):
    import torch
    from openhevc_amd.engine import Engine, remap_frame
    eng = Engine(0, stream=stream_of_engine)
    rec = F.Recorder(params(416, 240, 8, 1))
    f = rec.synth(F.synth_params(0, 11, sao_pct=50), 0)
    pid = eng.pic_alloc(f.p)
    eng.frame_submit(remap_frame(f, {0: pid}))
    out = eng.pics_convert([pid], "rgb_planar", dtype=torch.float32)     # no sync: ordered on the engine stream
    snap = out.clone()                                                      # read on torch's current stream
    s = float(out.sum(dtype=torch.float64))
    eng.sync()
    full = coded(eng.pic_download(pid, f.p), f.p)
    want = M.convert(full, f.p, "rgb_planar", E.CONV_F32)
    assert np.array_equal(host(snap)[0], bits(want))
    ws = float(np.sum(want, dtype=np.float64))
    assert abs(s - ws) <= 1e-9 * max(1.0, abs(ws))
    eng.close()
    rec.close()


def test_ordering_with_an_engine_stream_of_its_own():
    _ordering(None)


def test_ordering_with_an_engine_on_torchs_stream():
    import torch
    _ordering(torch.cuda.current_stream().cuda_stream)


def test_out_reuse_across_calls():
    import torch
    from openhevc_amd.engine import Engine, EngineError
    p = params(200, 136, 10, 1)
    eng = Engine(0)
    pids, hps = upload(eng, p, 4, np.random.default_rng(77))
    out = torch.empty((2, 136, 200, 4), dtype=torch.uint8, device="cuda:0")
    for k in range(2):
        r = eng.pics_convert(pids[2 * k:2 * k + 2], "rgba", out=out, matrix=9)
        assert r.data_ptr() == out.data_ptr()
        got = host(out)
        for i in range(2):
            assert np.array_equal(got[i], M.convert(coded(hps[2 * k + i], p), p, "rgba", E.CONV_U8, matrix=9)), (k, i)
    with pytest.raises(ValueError):
        eng.pics_convert(pids[:2], "rgb", out=out)                          # wrong shape
    with pytest.raises(ValueError):
        eng.pics_convert(pids[:2], "rgba", out=out.float())                 # wrong dtype
    with pytest.raises(EngineError):
        eng.pics_convert(pids[:1], "rgb", dtype=torch.uint8, matrix=4)
    eng.close()


def test_uint16_yuv_of_an_8bit_picture_is_refused():
    """uint16 asks a YUV format for the stored samples above 8 bit; an 8-bit picture has no such form: OH_E_UNSUPPORTED, not uint8"""
    from openhevc_amd.engine import Engine, EngineError
    eng = Engine(0)
    p8, p10 = params(64, 32, 8, 1), params(64, 32, 10, 1)
    (pid8,), (hp8,) = upload(eng, p8, 1, np.random.default_rng(16))
    (pid10,), (hp10,) = upload(eng, p10, 1, np.random.default_rng(17))
    for fmt in ("planar", "semiplanar"):
        with pytest.raises(EngineError) as ei:
            eng.pics_convert([pid8], fmt, dtype=torch.uint16)
        assert ei.value.code == E.OH_E_UNSUPPORTED
        out = torch.empty((1, 48, 64), dtype=torch.uint16, device="cuda:0")
        with pytest.raises(EngineError) as ei:
            eng.pics_convert([pid8], fmt, dtype=torch.uint16, out=out)
        assert ei.value.code == E.OH_E_UNSUPPORTED
        got = eng.pics_convert([pid10], fmt, dtype=torch.uint16)
        assert got.dtype == torch.uint16
        assert np.array_equal(host(got)[0], M.convert(coded(hp10, p10), p10, fmt, E.CONV_NATIVE))
        assert np.array_equal(host(eng.pics_convert([pid8], fmt))[0], M.convert(coded(hp8, p8), p8, fmt, E.CONV_NATIVE))
    eng.close()


# ---- the argument rules: raw C calls into a guarded device buffer ----
def test_argument_errors_write_nothing():
    import torch
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    p = params(64, 32, 10, 1)
    p8 = params(64, 32, 8, 1)
    pm = params(64, 32, 8, 0)
    pids, _ = upload(eng, p, 2, np.random.default_rng(1))
    other, _ = upload(eng, p8, 1, np.random.default_rng(2))
    mono, _ = upload(eng, pm, 1, np.random.default_rng(3))
    G = 4096
    cv = E.make_convert("rgb", E.CONV_U8)
    ib = E.convert_image_bytes(p, cv)
    buf = torch.full((2 * ib + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()                                                # raw calls: no ordering against torch's stream
    dst = buf.data_ptr() + G

    def call(ids, cv, dst, stride, nbytes):
        return L.oh_pics_convert(eng.h, (C.c_int * max(len(ids), 1))(*ids), len(ids), C.byref(cv), C.c_void_p(dst), stride, nbytes)

    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    assert call(pids, cv, dst, ib, 2 * ib - 1) == arg                       # one byte short
    assert call(pids[:1], cv, dst, ib, ib - 1) == arg
    assert call(pids, cv, dst, ib - 1, 2 * ib) == arg                       # stride below the image
    host_buf = np.zeros(2 * ib, np.uint8)
    assert call(pids, cv, host_buf.ctypes.data, ib, 2 * ib) == arg          # a host pointer
    assert call(pids + other, cv, dst, ib, 3 * ib) == arg                   # mixed params
    assert call([pids[0], 999], cv, dst, ib, 2 * ib) == arg                 # unknown id
    assert call([pids[0], -1], cv, dst, ib, 2 * ib) == arg
    for win in ((1, 0, 0, 0), (0, 0, 0, 1), (64, 0, 0, 0), (0, 0, 16, 16), (-2, 0, 0, 0)):
        assert call(pids, E.make_convert("rgb", E.CONV_U8, win), dst, ib, 2 * ib) == arg, win
    assert call(mono, E.make_convert("semiplanar", E.CONV_NATIVE), dst, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("planar", E.CONV_F32), dst, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("planar", E.CONV_U16), dst, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("rgb", E.CONV_NATIVE), dst, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("rgb", E.CONV_U8, matrix=4), dst, ib, 2 * ib) == uns
    assert call([], cv, dst, ib, 0) == 0                                    # n == 0: nothing to do
    cv16 = E.make_convert("rgb", E.CONV_U16)
    ib16 = E.convert_image_bytes(p, cv16)
    assert call(pids[:1], cv16, dst, ib16 + 1, ib16 + 1) == arg             # stride, dst: multiples of the sample size
    assert call(pids[:1], cv16, dst + 1, ib16, ib16) == arg
    # two 16 x 16 pictures into memory whose allocation ends one byte before the second image does
    small, _ = upload(eng, params(16, 16, 8, 1), 2, np.random.default_rng(4))
    sb = E.convert_image_bytes(params(16, 16, 8, 1), cv)
    short, stride, claim = DR.one_byte_short(L, 2, sb)
    assert call(small, cv, short.data_ptr(), stride, claim) == arg
    eng.sync()
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()) and bool((short == 0xA5).all()), "a refused call wrote into the destination"
    # the same buffer taken exactly: the guards around it stay untouched
    assert call(pids, cv, dst, ib, 2 * ib) == 0
    eng.sync()
    b = buf.cpu().numpy()
    assert np.all(b[:G] == 0xA5) and np.all(b[G + 2 * ib:] == 0xA5)
    eng.close()


def test_unaligned_destinations_and_strides():
    """odd byte offsets and padded image strides: the head / tail stores land exactly, nothing outside an image is written"""
    import torch
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    p = params(136, 40, 10, 1)
    pids, hps = upload(eng, p, 3, np.random.default_rng(9))
    for fmt, dt, win in (("rgb", E.CONV_U8, (2, 0, 0, 0)), ("planar", E.CONV_U8, (0, 2, 0, 0)), ("semiplanar", E.CONV_NATIVE, (2, 2, 0, 0))):
        cv = E.make_convert(fmt, dt, win)
        ib = E.convert_image_bytes(p, cv)
        for off, pad in ((0, 0), (2, 6), (6, 10), (14, 34)):
            if dt == E.CONV_U8:
                off, pad = off + 1, pad + 1
            stride = ib + pad
            buf = torch.full((3 * stride + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()                                        # the raw call below does not order against torch's stream
            rc = eng.L.oh_pics_convert(eng.h, (C.c_int * 3)(*pids), 3, C.byref(cv), C.c_void_p(buf.data_ptr() + off), stride, 3 * stride)
            assert rc == 0, (fmt, off, pad)
            eng.sync()
            b = buf.cpu().numpy()
            assert np.all(b[:off] == 0x5A)
            for i in range(3):
                img = b[off + i * stride:off + i * stride + ib]
                want = M.convert(coded(hps[i], p), p, fmt, dt, win)
                assert np.array_equal(img, want.view(np.uint8).ravel()), (fmt, off, pad, i)
                assert np.all(b[off + i * stride + ib:off + (i + 1) * stride] == 0x5A)
    eng.close()
