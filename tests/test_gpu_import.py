"""-m gpu: oh_pics_import / Engine.pics_import on the MI355X against the numpy model of tests/import_model.py, bit for bit and over the
whole coded planes (oh_pic_download): YUV and RGB layouts over chroma formats, bit depths and windows with margins, the round trip
with oh_pics_convert on the device, images wider than a workgroup segment, more pictures than one launch, unaligned sources, the
other picture services on imported pictures, ordering with torch streams and the argument rules."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import convert_model as CM                                                  # noqa: E402
import device_room as DR                                                    # noqa: E402
import import_model as IM                                                   # noqa: E402
import picture_hash as PH                                                   # noqa: E402
import resize_model as RM                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RGB_FORMATS = ("rgb_planar", "rgb", "rgba")
RGB_DTYPES = ("uint8", "uint16", "float16", "float32")
SAMPLE_OF = {"uint8": E.CONV_U8, "uint16": E.CONV_U16, "float16": E.CONV_F16, "float32": E.CONV_F32}
ZERO = (0, 0, 0, 0)


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def coded(hp, p):
    return [hp.visible(c) for c in range(F.n_planes(p))]


def download(eng, pid, p):
    return coded(eng.pic_download(pid, p), p)


def random_pic(p, rng):
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        v[...] = rng.integers(0, 1 << p.bit_depth, v.shape, dtype=v.dtype)
    return hp


def upload(eng, p, n, rng):
    pids, hps = [], []
    for _ in range(n):
        hp = random_pic(p, rng)
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        pids.append(pid)
        hps.append(hp)
    return pids, hps


def window_size(p, win):
    return p.width - win[0] - win[1], p.height - win[2] - win[3]


def yuv_samples(p, win):
    W, H = window_size(p, win)
    hs, vs = IM.shifts(p.chroma_format_idc)
    return W * H + (2 * (W >> hs) * (H >> vs) if p.chroma_format_idc else 0)


def yuv_images(p, win, n, dtype, hi, rng):
    """n random YUV images of the window as (n, rows, W), values below hi"""
    W, _ = window_size(p, win)
    return rng.integers(0, hi, (n, yuv_samples(p, win) // W, W)).astype(dtype)


def rgb_shape(fmt, W, H):
    return (3, H, W) if fmt == "rgb_planar" else (H, W, 4 if fmt == "rgba" else 3)


def same_planes(got, want, what):
    assert len(got) == len(want), what
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (what, c, np.argwhere(g != w)[:4].tolist())


def check_import(eng, imgs, p, fmt, sample, win, pids, **kw):
    """imgs (numpy, one image per picture) through Engine.pics_import into pids: every coded plane equals the model"""
    ids, w = eng.pics_import(torch.from_numpy(imgs).to(DEV), fmt, out=pids, window=win, **kw)
    assert ids == list(pids) and tuple(w) == tuple(win)
    for i, pid in enumerate(pids):
        assert eng.pic_final_half(pid) == 0
        same_planes(download(eng, pid, p), IM.import_picture(imgs[i], p, fmt, sample, win, **kw), (fmt, sample, win, kw, i))


YUV_CASES = [(72, 40, 10, 0, (3, 1, 2, 5)), (416, 240, 8, 1, (2, 4, 0, 2)), (264, 200, 12, 1, (6, 2, 4, 8)), (264, 200, 9, 2, (2, 0, 1, 3)),
             (200, 136, 12, 3, (1, 2, 3, 0)), (24, 8, 10, 3, (0, 1, 0, 0)), (8, 8, 8, 0, ZERO)]


@pytest.mark.parametrize("w,h,bd,cf,win", YUV_CASES, ids=[f"{c[0]}x{c[1]}_{c[2]}b_cf{c[3]}_win{'_'.join(map(str, c[4]))}" for c in YUV_CASES])
def test_yuv_forms_bit_for_bit(w, h, bd, cf, win):
    """planar and semi-planar, NATIVE and U8, two images per call; the whole coded planes, replicated margins included"""
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, cf)
    rng = np.random.default_rng(w + h + bd + cf)
    eng = Engine(0)
    pids = [eng.pic_alloc(p) for _ in range(2)]
    native = np.uint8 if bd == 8 else np.uint16
    for fmt in ("planar", "semiplanar") if cf else ("planar",):
        # NATIVE: stored samples; the semi-planar form above 8 bit carries them at the MSB end, any 16-bit value is defined
        hi = 1 << (16 if fmt == "semiplanar" and bd > 8 else bd)
        check_import(eng, yuv_images(p, win, 2, native, hi, rng), p, fmt, E.CONV_NATIVE, win, pids)
        check_import(eng, yuv_images(p, win, 2, np.uint8, 256, rng), p, fmt, E.CONV_U8, win, pids)
    eng.close()


def test_planar_samples_above_the_bit_depth_are_clamped():
    from openhevc_amd.engine import Engine
    p = params(72, 40, 10, 1)
    win = (2, 2, 0, 2)
    eng = Engine(0)
    pids = [eng.pic_alloc(p) for _ in range(2)]
    imgs = yuv_images(p, win, 2, np.uint16, 1 << 16, np.random.default_rng(4))
    imgs[0, 0, :4] = [1023, 1024, 65535, 0]
    check_import(eng, imgs, p, "planar", E.CONV_NATIVE, win, pids)
    for pid in pids:
        assert max(int(pl.max()) for pl in download(eng, pid, p)) == 1023
    eng.close()


@pytest.mark.parametrize("w,h,bd,cf,win", [(416, 240, 8, 1, (2, 4, 0, 2)), (264, 200, 12, 1, (6, 2, 4, 8)), (264, 200, 9, 2, (2, 0, 1, 3)),
                                           (200, 136, 10, 3, (1, 2, 3, 0)), (72, 40, 10, 0, (3, 1, 2, 5))])
def test_round_trip_on_the_device(w, h, bd, cf, win):
    """what pics_convert gave, pics_import takes back: no sample of the window differs, and the rest of the picture is the model's"""
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, cf)
    eng = Engine(0)
    pids, hps = upload(eng, p, 2, np.random.default_rng(w + bd))
    for fmt in ("planar", "semiplanar") if cf else ("planar",):
        img = eng.pics_convert(pids, fmt, window=win)
        back = [eng.pic_alloc(p) for _ in pids]
        ids, bw = eng.pics_import(img, fmt, out=back, window=win)
        for cmp in eng.pics_compare(pids, ids, window=bw, ssim=False):
            assert [pl.differing for pl in cmp.plane] == [0, 0, 0]
        for i, hp in enumerate(hps):
            model = IM.replicate(CM.crop(coded(hp, p), cf, win), w, h, cf, win)
            for ht in (0, 1):
                assert eng.pics_hash([ids[i]], ht)[0] == PH.picture_hash(model, bd, ht), (fmt, i, ht)
        for pid in back:
            eng.pic_free(pid)
    eng.close()


def test_fresh_pictures_take_the_image_at_the_top_left():
    from openhevc_amd.engine import Engine, EngineError
    eng = Engine(0)
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (2, 38, 70, 3)).astype(np.uint8)
    ids, win = eng.pics_import(torch.from_numpy(img).to(DEV), "rgb", bit_depth=10, chroma_format_idc=1, matrix=9, full_range=True)
    p = eng._pic_params(ids[0])
    assert (p.width, p.height, p.bit_depth, p.chroma_format_idc) == (72, 40, 10, 1) and win == (0, 2, 0, 2)
    for i, pid in enumerate(ids):
        same_planes(download(eng, pid, p), IM.import_picture(img[i], p, "rgb", E.CONV_U8, win, matrix=9, full_range=True), i)
    yuv = rng.integers(0, 1024, (1, 60, 64)).astype(np.uint16)             # I420 of 64 x 40
    ids2, win2 = eng.pics_import(torch.from_numpy(yuv).to(DEV), "planar", bit_depth=10, chroma_format_idc=1)
    p2 = eng._pic_params(ids2[0])
    assert (p2.width, p2.height) == (64, 40) and win2 == ZERO
    same_planes(download(eng, ids2[0], p2), IM.import_picture(yuv[0], p2, "planar", E.CONV_NATIVE), "fresh planar")
    known = len(eng._params)
    with pytest.raises(EngineError) as ei:                                   # an odd width cannot be a 4:2:0 window: the pictures are freed again
        eng.pics_import(torch.zeros((1, 38, 71, 3), dtype=torch.uint8, device=DEV), "rgb", bit_depth=8, chroma_format_idc=1)
    assert ei.value.code == E.OH_E_ARG and len(eng._params) == known
    with pytest.raises(ValueError):
        eng.pics_import(torch.zeros((1, 38, 70, 3), dtype=torch.uint8, device=DEV), "rgb")
    with pytest.raises(ValueError):                                          # the image is not the window's size
        eng.pics_import(torch.zeros((2, 38, 70, 3), dtype=torch.uint8, device=DEV), "rgb", out=ids, window=ZERO)
    with pytest.raises(ValueError):
        eng.pics_import(torch.zeros((1, 38, 70, 3), dtype=torch.uint8, device=DEV), "rgb", out=ids, window=win)
    eng.close()


RGB_GEOMS = [(72, 40, 8, 0, (2, 0, 0, 2)), (72, 40, 10, 1, (2, 4, 2, 0)), (136, 72, 9, 1, ZERO), (104, 48, 12, 2, (2, 2, 1, 0)),
             (40, 24, 10, 3, (1, 0, 3, 2)), (72, 40, 8, 3, (0, 3, 0, 0))]


def rgb_inputs(eng, p, fmt, dt, win, rng):
    """two images: u8 / u16 random over the full range; floats what pics_convert gives for random pictures, plus a few hand-placed
    values: 0, 1, slightly above 1, negative, NaN (and the infinities)"""
    W, H = window_size(p, win)
    if dt in ("uint8", "uint16"):
        return rng.integers(0, 1 << (8 if dt == "uint8" else 16), (2,) + rgb_shape(fmt, W, H)).astype(dt)
    pids, _ = upload(eng, p, 2, rng)
    t = eng.pics_convert(pids, fmt, dtype=getattr(torch, dt), window=win, matrix=5, full_range=True, chroma="nearest")
    a = t.cpu().numpy().copy()
    for pid in pids:
        eng.pic_free(pid)
    flat = a.reshape(2, -1)
    flat[:, :8] = np.array([0.0, 1.0, 1.0005, -0.25, np.nan, np.inf, -np.inf, 0.5], a.dtype)
    flat[:, -3:] = np.array([np.nan, 2.0, -0.0], a.dtype)
    return a


@pytest.mark.parametrize("w,h,bd,cf,win", RGB_GEOMS, ids=[f"{c[0]}x{c[1]}_{c[2]}b_cf{c[3]}" for c in RGB_GEOMS])
def test_every_rgb_form_equals_the_model(w, h, bd, cf, win):
    """every layout x sample type x matrix x range x filter; two images per call"""
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, cf)
    rng = np.random.default_rng(bd * 7 + cf)
    eng = Engine(0)
    pids = [eng.pic_alloc(p) for _ in range(2)]
    for fmt, dt in itertools.product(RGB_FORMATS, RGB_DTYPES):
        imgs = rgb_inputs(eng, p, fmt, dt, win, rng)
        dev = torch.from_numpy(imgs).to(DEV)
        for matrix, fr, chroma in itertools.product((1, 5, 6, 9), (False, True), ("linear", "nearest")):
            eng.pics_import(dev, fmt, out=pids, window=win, matrix=matrix, full_range=fr, chroma=chroma)
            for i, pid in enumerate(pids):
                want = IM.import_picture(imgs[i], p, fmt, SAMPLE_OF[dt], win, matrix, fr, chroma)
                same_planes(download(eng, pid, p), want, (fmt, dt, matrix, fr, chroma, i))
    eng.close()


SEGMENT_CASES = [
    (4112, 16, 12, 2, ZERO, [("planar", "uint16"), ("semiplanar", "uint8"), ("rgb", "uint16"), ("rgb_planar", "float32")]),
    (2056, 32, 8, 3, ZERO, [("rgb", "uint8"), ("rgba", "uint8"), ("planar", "uint8")]),
    (2112, 64, 10, 3, ZERO, [("semiplanar", "uint16"), ("rgb", "float16")]),
    (4104, 16, 10, 1, (2, 0, 0, 0), [("planar", "uint16"), ("semiplanar", "uint16"), ("rgb", "uint8"), ("rgb_planar", "uint16"),
                                     ("rgba", "float32")]),
]


@pytest.mark.parametrize("w,h,bd,cf,win,forms", SEGMENT_CASES, ids=[f"{c[0]}x{c[1]}_{c[2]}b_cf{c[3]}" for c in SEGMENT_CASES])
def test_images_wider_than_one_segment(w, h, bd, cf, win, forms):
    """several workgroups per row: the filter's halo column and the clamped margins at the seams"""
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, cf)
    rng = np.random.default_rng(w)
    eng = Engine(0)
    pids = [eng.pic_alloc(p) for _ in range(2)]
    W, H = window_size(p, win)
    for fmt, dt in forms:
        if fmt in ("planar", "semiplanar"):
            sample = E.CONV_U8 if dt == "uint8" and bd > 8 else E.CONV_NATIVE
            check_import(eng, yuv_images(p, win, 2, dt, 256 if dt == "uint8" else 1 << (16 if fmt == "semiplanar" else bd), rng), p, fmt,
                         sample, win, pids)
        elif dt in ("uint8", "uint16"):
            imgs = rng.integers(0, 1 << (8 if dt == "uint8" else 16), (2,) + rgb_shape(fmt, W, H)).astype(dt)
            for chroma in ("linear", "nearest"):
                check_import(eng, imgs, p, fmt, SAMPLE_OF[dt], win, pids, matrix=9, chroma=chroma)
        else:
            imgs = rng.random((2,) + rgb_shape(fmt, W, H), dtype=np.float32).astype(dt)
            check_import(eng, imgs, p, fmt, SAMPLE_OF[dt], win, pids, matrix=1, full_range=True)
    eng.close()


def test_more_pictures_than_one_launch():
    from openhevc_amd.engine import Engine
    p = params(64, 64, 10, 1)
    rng = np.random.default_rng(70)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 6
    pids = [eng.pic_alloc(p) for _ in range(n)]
    check_import(eng, yuv_images(p, ZERO, n, np.uint16, 1 << 16, rng), p, "semiplanar", E.CONV_NATIVE, ZERO, pids)
    check_import(eng, rng.integers(0, 256, (n, 64, 64, 3)).astype(np.uint8), p, "rgb", E.CONV_U8, ZERO, pids[::-1])
    eng.close()


def test_unaligned_sources_and_strides():
    """src one sample into a tensor, an image stride above the image size that is no multiple of 16, and an odd width in 4:4:4 (rows of
    a u8 H x W x 3 image start at any byte)"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(9)
    for (w, h, bd, cf, win), fmt, sample, kw in (
            ((136, 40, 10, 3, (1, 2, 0, 0)), "rgb", E.CONV_U8, dict(matrix=5)),
            ((136, 40, 8, 3, (0, 3, 1, 0)), "rgb", E.CONV_U8, dict(full_range=True)),
            ((136, 40, 10, 1, (2, 0, 0, 0)), "planar", E.CONV_U8, {}),
            ((136, 40, 10, 1, (2, 2, 0, 0)), "semiplanar", E.CONV_NATIVE, {}),
            ((136, 40, 12, 2, (2, 0, 3, 0)), "rgb_planar", E.CONV_F32, {})):
        p = params(w, h, bd, cf)
        cv = E.make_convert(fmt, sample, win, kw.get("matrix", 1), kw.get("full_range", False))
        ib = E.convert_image_bytes(p, cv)
        sb = {E.CONV_U8: 1, E.CONV_F32: 4}.get(sample, 2)
        dt = {1: np.uint8, 2: np.uint16, 4: np.float32}[sb]
        pids = [eng.pic_alloc(p) for _ in range(3)]
        for off, pad in ((1, 1), (3, 7), (7, 11), (15, 35)):
            off, pad = off * sb, pad * sb
            stride = ib + pad
            if stride % 16 == 0:
                stride += sb
            host_buf = np.zeros(off + 3 * stride, np.uint8)
            imgs = []
            for i in range(3):
                img = rng.random(ib // sb, dtype=np.float32) if sb == 4 else rng.integers(0, 1 << (8 * sb), ib // sb).astype(dt)
                host_buf[off + i * stride:off + i * stride + ib] = img.view(np.uint8)
                imgs.append(img)
            buf = torch.from_numpy(host_buf).to(DEV)
            torch.cuda.synchronize()                                        # the raw call below does not order against torch's stream
            rc = eng.L.oh_pics_import(eng.h, (C.c_int * 3)(*pids), 3, C.byref(cv), C.c_void_p(buf.data_ptr() + off), stride, 3 * stride)
            assert rc == 0, (fmt, off, pad)
            eng.sync()
            W, H = window_size(p, win)
            for i, pid in enumerate(pids):
                img = imgs[i].reshape(rgb_shape(fmt, W, H)) if fmt.startswith("rgb") else imgs[i]
                same_planes(download(eng, pid, p), IM.import_picture(img, p, fmt, sample, win, **kw), (fmt, off, pad, i))
        for pid in pids:
            eng.pic_free(pid)
    eng.close()


def test_an_imported_picture_is_an_ordinary_finished_picture():
    """import -> resize -> convert equals the models chained; a wrapped picture takes an import like an allocated one"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(21)
    p = params(200, 136, 10, 1)
    win = (2, 6, 4, 0)
    W, H = window_size(p, win)
    img = rng.integers(0, 1 << 16, (2, H, W, 3)).astype(np.uint16)
    half = eng.L.oh_pic_bytes(C.byref(p)) // 2
    mem = torch.zeros(2 * half, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    pids = [eng.pic_alloc(p), eng.pic_wrap(p, mem.data_ptr(), mem.data_ptr() + half, half)]
    ids, iw = eng.pics_import(torch.from_numpy(img).to(DEV), "rgb", out=pids, window=win, matrix=9)
    small, sw = eng.pics_resize(ids, (96, 64), window=iw, filter="bicubic")
    got = eng.pics_convert(small, "rgb_planar", dtype=torch.uint16, window=sw, matrix=9).cpu().numpy()
    dp = eng._pic_params(small[0])
    for i in range(2):
        planes = IM.import_picture(img[i], p, "rgb", E.CONV_U16, win, matrix=9)
        same_planes(download(eng, ids[i], p), planes, ("imported", i))
        res = RM.pad_to(RM.resize(planes, 1, 10, (96, 64), "bicubic", win), 1, (dp.width, dp.height))
        assert np.array_equal(got[i], CM.convert(res, dp, "rgb_planar", E.CONV_U16, sw, matrix=9)), i
    eng.close()


def test_import_into_a_picture_whose_finished_half_was_1():
    from openhevc_amd.engine import Engine, remap_frame
    eng = Engine(0)
    rec = F.Recorder(params(416, 240, 8, 1))
    f = rec.synth(F.synth_params(0, 3, sao_pct=90), 0)
    pid = eng.pic_alloc(f.p)
    eng.frame_submit(remap_frame(f, {0: pid}))
    assert eng.pic_final_half(pid) == 1
    img = np.random.default_rng(2).integers(0, 256, (1, 360, 416)).astype(np.uint8)
    eng.pics_import(torch.from_numpy(img).to(DEV), "semiplanar", out=[pid])  # no sync: ordered behind the passes on the engine stream
    assert eng.L.oh_pic_final_half(eng.h, pid) == 0
    back = eng.pics_convert([pid], "semiplanar").cpu().numpy()
    assert np.array_equal(back, img)
    same_planes(download(eng, pid, f.p), IM.import_picture(img[0], f.p, "semiplanar", E.CONV_NATIVE), "half 0")
    eng.close()
    rec.close()


# ---- ordering with torch ----
def _ordering(stream_of_engine):
    """the image comes out of a torch kernel immediately before the call and is overwritten immediately after it"""
    from openhevc_amd.engine import Engine
    eng = Engine(0, stream=stream_of_engine)
    W, H = 1280, 720
    idx = torch.arange(H * W * 3, dtype=torch.int64, device=DEV)
    img = ((idx * 2654435761) >> 7).remainder(256).to(torch.uint8).reshape(1, H, W, 3)     # queued, not waited for
    ids, win = eng.pics_import(img, "rgb", bit_depth=8, chroma_format_idc=1)
    img.fill_(77)                                                           # torch's stream waits for the engine's read
    del img
    junk = torch.full((H * W * 3,), 99, dtype=torch.uint8, device=DEV)     # the allocator may hand the same memory out again
    eng.sync()
    n = np.arange(H * W * 3, dtype=np.int64)
    want_img = (((n * 2654435761) >> 7) % 256).astype(np.uint8).reshape(H, W, 3)
    p = eng._pic_params(ids[0])
    same_planes(download(eng, ids[0], p), IM.import_picture(want_img, p, "rgb", E.CONV_U8, win), "ordering")
    assert int(junk[0]) == 99
    eng.close()


def test_ordering_with_an_engine_stream_of_its_own():
    _ordering(None)


def test_ordering_with_an_engine_on_torchs_stream():
    _ordering(torch.cuda.current_stream().cuda_stream)


# ---- the argument rules: raw C calls, the destinations' hashes stay ----
def test_argument_errors_write_nothing():
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    p, p8, pm = params(64, 32, 10, 1), params(64, 32, 8, 1), params(64, 32, 8, 0)
    pids, _ = upload(eng, p, 2, np.random.default_rng(1))
    other, _ = upload(eng, p8, 1, np.random.default_rng(2))
    mono, _ = upload(eng, pm, 1, np.random.default_rng(3))
    everything = pids + other + mono
    before = [eng.pics_hash([pid], 0) for pid in everything]
    cv = E.make_convert("rgb", E.CONV_U8)
    cv16 = E.make_convert("rgb", E.CONV_U16)
    ib, ib16 = E.convert_image_bytes(p, cv), E.convert_image_bytes(p, cv16)
    buf = torch.full((4 * ib16 + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    short = torch.full((ib,), 0x5A, dtype=torch.uint8, device=DEV)          # one image where two are asked for
    torch.cuda.synchronize()                                                # raw calls: no ordering against torch's stream
    src = buf.data_ptr()

    def call(ids, cv, src, stride, nbytes):
        arr = None if ids is None else (C.c_int * max(len(ids), 1))(*ids)
        return L.oh_pics_import(eng.h, arr, 2 if ids is None else len(ids), None if cv is None else C.byref(cv),
                                None if src is None else C.c_void_p(src), stride, nbytes)

    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    assert call(pids, None, src, ib, 2 * ib) == arg                         # null arguments
    assert call(None, cv, src, ib, 2 * ib) == arg
    assert call(pids, cv, None, ib, 2 * ib) == arg
    assert L.oh_pics_import(None, (C.c_int * 2)(*pids), 2, C.byref(cv), C.c_void_p(src), ib, 2 * ib) == arg
    assert call([pids[0], 999], cv, src, ib, 2 * ib) == arg                 # unknown pictures
    assert call([pids[0], -1], cv, src, ib, 2 * ib) == arg
    assert call(pids + other, cv, src, ib, 3 * ib) == arg                   # params differ
    assert call([pids[0], pids[1], pids[0]], cv, src, ib, 3 * ib) == arg    # a destination twice
    for win in ((1, 0, 0, 0), (0, 0, 0, 1), (64, 0, 0, 0), (0, 0, 16, 16), (-2, 0, 0, 0)):
        assert call(pids, E.make_convert("rgb", E.CONV_U8, win), src, ib, 2 * ib) == arg, win
    assert call(pids, cv, src, ib - 1, 2 * ib) == arg                       # stride below the image
    assert call(pids, cv16, src, ib16 + 1, 2 * ib16 + 1) == arg             # stride, src: multiples of the sample size
    assert call(pids, cv16, src + 1, ib16, 2 * ib16) == arg
    assert call(pids, cv, src, ib, 2 * ib - 1) == arg                       # images that do not fit src_bytes
    assert call(pids[:1], cv, src, ib, ib - 1) == arg
    assert call(pids, cv, short.data_ptr(), ib, short.numel()) == arg       # a tensor one image too short
    host_buf = np.zeros(2 * ib, np.uint8)
    assert call(pids, cv, host_buf.ctypes.data, ib, 2 * ib) == arg          # a host pointer
    assert call(mono, E.make_convert("semiplanar", E.CONV_NATIVE), src, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("planar", E.CONV_F32), src, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("planar", E.CONV_U16), src, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("rgb", E.CONV_NATIVE), src, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("rgb", E.CONV_U8, matrix=4), src, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("rgb", E.CONV_U8, matrix=0), src, ib, 2 * ib) == uns
    assert call([], cv, src, ib, 0) == 0                                    # n == 0: nothing to do
    # two 16 x 16 pictures from memory whose allocation ends one byte before the second image does
    small, _ = upload(eng, params(16, 16, 8, 1), 2, np.random.default_rng(4))
    before_small = [eng.pics_hash([pid], 0) for pid in small]
    gone, stride, claim = DR.one_byte_short(eng.L, 2, E.convert_image_bytes(params(16, 16, 8, 1), cv))
    assert call(small, cv, gone.data_ptr(), stride, claim) == arg
    eng.sync()
    assert [eng.pics_hash([pid], 0) for pid in small] == before_small
    assert [eng.pics_hash([pid], 0) for pid in everything] == before, "a refused call wrote into a destination"
    # every refusal has the code oh_pics_convert gives for the same combination
    for bad in (E.make_convert("planar", E.CONV_F32), E.make_convert("rgb", E.CONV_NATIVE), E.make_convert("rgb", E.CONV_U8, matrix=4),
                E.make_convert("rgb", E.CONV_U8, (1, 0, 0, 0))):
        ids = (C.c_int * 2)(*pids)
        assert L.oh_pics_import(eng.h, ids, 2, C.byref(bad), C.c_void_p(src), ib16, 4 * ib16) == \
            L.oh_pics_convert(eng.h, ids, 2, C.byref(bad), C.c_void_p(src), ib16, 4 * ib16)
    eng.sync()
    assert bool((buf == 0x5A).all())
    # the same source taken exactly
    assert call(pids, cv, src, ib, 2 * ib) == 0
    eng.sync()
    img = np.full((32, 64, 3), 0x5A, np.uint8)
    for pid in pids:
        same_planes(download(eng, pid, p), IM.import_picture(img, p, "rgb", E.CONV_U8), "exact fit")
    with pytest.raises(ValueError):
        eng.pics_import(short.reshape(1, 32, 64, 3), "rgb", out=pids)       # one image for two pictures
    eng.close()
