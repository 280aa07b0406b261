"""-m gpu: oh_pics_convert_colour / Engine.pics_convert(colour=...) on the MI355X against the numpy model of tests/colour_model.py, bit
for bit: the transfer curves, tone curve and primaries over chroma formats, bit depths, windows, layouts and sample types, segment
boundaries, batches of more than one launch, two calls in flight with different tables, ordering with torch streams and the argument
rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import colour_model as M                                                    # noqa: E402
import device_room as DR                                                    # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

RGB_FORMATS = ("rgb_planar", "rgb", "rgba")
SAMPLE_OF = {"uint8": E.CONV_U8, "uint16": E.CONV_U16, "float16": E.CONV_F16, "float32": E.CONV_F32}
# name -> (OhColour, H.273 matrix of the source, the permitted sample types)
PIPELINES = {
    "pq2020_srgb709": (E.make_colour(16, 9, out="srgb", tone="bt2390", norm="maxrgb", src_peak=1000, dst_peak=100), 9,
                       ("uint8", "uint16", "float16", "float32")),
    "hlg2020_gamma24_709": (E.make_colour(18, 9, out="gamma24", tone="bt2390", norm="luma", src_peak=1000, dst_peak=100), 9,
                            ("uint8", "uint16", "float16", "float32")),
    "srgb709_linear": (E.make_colour(13, 1, out="linear", tone="none", src_peak=100), 1, ("float16", "float32")),
    "pq2020_linear2020": (E.make_colour(16, 9, out="linear", out_primaries=9, tone="none"), 9, ("float16", "float32")),
}
_tables = {}


def tables(name):
    """the tables of a pipeline, computed once"""
    if name not in _tables:
        _tables[name] = E.colour_tables(PIPELINES[name][0])
    return _tables[name]


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def fill(p, how, rng):
    """a picture of uniform random codes over the whole sample range, a luma ramp through every code with neutral chroma, all zero or
    all maximum"""
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


def bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32) if a.dtype == np.float32 else a


def host(t):
    return bits(t.cpu().numpy())


def want(hp, p, fmt, dt, name, win=(0, 0, 0, 0), **kw):
    col, matrix, _ = PIPELINES[name]
    return bits(M.convert(coded(hp, p), p, fmt, SAMPLE_OF[dt], col, win, matrix, tables=tables(name), **kw))


def got(eng, pids, fmt, dt, name, win=(0, 0, 0, 0), **kw):
    col, matrix, _ = PIPELINES[name]
    return eng.pics_convert(pids, fmt, dtype=getattr(torch, dt), window=win, matrix=matrix, colour=col, **kw)


# coded size, bit depth, chroma format, window; the third gives images of 71 x 39 (coded sizes are multiples of the minimum coding block)
GEOMS = [(72, 40, 10, 1, (2, 4, 2, 0)), (104, 48, 12, 2, (2, 2, 1, 0)), (72, 40, 10, 3, (1, 0, 0, 1)), (72, 40, 8, 1, (0, 0, 0, 0))]


@pytest.mark.parametrize("name", list(PIPELINES))
@pytest.mark.parametrize("w,h,bd,cf,win", GEOMS, ids=[f"{c[0]}x{c[1]}_{c[2]}b_cf{c[3]}" for c in GEOMS])
def test_every_form_equals_the_model(w, h, bd, cf, win, name):
    """random, ramp, all-zero and all-maximum pictures in one call; every layout x permitted sample type; limited range (the random codes
    bring super-white and sub-black) with the linear chroma filter, full range with the nearest"""
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, cf)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random", "ramp", "zero", "max"), np.random.default_rng(bd * 7 + cf))
    for fmt in RGB_FORMATS:
        for dt in PIPELINES[name][2]:
            for kw in (dict(full_range=False, chroma="linear"), dict(full_range=True, chroma="nearest")):
                g = host(got(eng, pids, fmt, dt, name, win, **kw))
                for i, hp in enumerate(hps):
                    wnt = want(hp, p, fmt, dt, name, win, **kw)
                    assert g[i].shape == wnt.shape and np.array_equal(g[i], wnt), (fmt, dt, kw, i)
    eng.close()


def test_segment_boundaries_at_every_segment_width():
    """images of 4158 x 4 (coded 4160 x 8, the window's left at 2): their rows cross the 2048-, 1024- and 512-pixel segments of the sample
    types"""
    from openhevc_amd.engine import Engine
    p = params(4160, 8, 10, 1)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random",), np.random.default_rng(4160))
    win = (2, 0, 0, 4)
    for fmt, dt, name in (("rgb", "uint8", "pq2020_srgb709"), ("rgb_planar", "uint16", "pq2020_srgb709"),
                          ("rgba", "float16", "hlg2020_gamma24_709"), ("rgb_planar", "float32", "pq2020_linear2020"),
                          ("rgb", "float32", "srgb709_linear")):
        g = host(got(eng, pids, fmt, dt, name, win))
        assert np.array_equal(g[0], want(hps[0], p, fmt, dt, name, win)), (fmt, dt, name)
    eng.close()


def test_more_pictures_than_one_launch():
    """66 pictures: two launches; each image lands at its own offset"""
    from openhevc_amd.engine import Engine
    p = params(16, 8, 10, 1)
    eng = Engine(0)
    n = E.CONV_MAX_PICS + 2
    pids, hps = upload(eng, p, ("random",) * n, np.random.default_rng(66))
    g = host(got(eng, pids, "rgb", "uint8", "pq2020_srgb709"))
    for i in range(n):
        assert np.array_equal(g[i], want(hps[i], p, "rgb", "uint8", "pq2020_srgb709")), i
    eng.close()


def test_two_calls_in_flight_keep_their_own_tables():
    """two calls with different OhColour into different tensors, no sync between them: the second call's table copy is ordered behind
    the first call's kernel"""
    from openhevc_amd.engine import Engine
    p = params(200, 136, 10, 1)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random", "ramp"), np.random.default_rng(2))
    a = got(eng, pids, "rgb_planar", "uint16", "pq2020_srgb709")
    b = got(eng, pids, "rgb_planar", "uint16", "hlg2020_gamma24_709")
    c = got(eng, pids, "rgb_planar", "uint16", "pq2020_srgb709")
    ga, gb, gc = host(a), host(b), host(c)
    for i, hp in enumerate(hps):
        assert np.array_equal(ga[i], want(hp, p, "rgb_planar", "uint16", "pq2020_srgb709")), i
        assert np.array_equal(gb[i], want(hp, p, "rgb_planar", "uint16", "hlg2020_gamma24_709")), i
    assert np.array_equal(ga, gc)
    eng.close()


def test_out_reuse_and_the_plain_path_beside_it():
    from openhevc_amd.engine import Engine, EngineError
    import convert_model as CM
    p = params(200, 136, 10, 1)
    eng = Engine(0)
    pids, hps = upload(eng, p, ("random",) * 4, np.random.default_rng(77))
    col = PIPELINES["pq2020_srgb709"][0]
    out = torch.empty((2, 136, 200, 4), dtype=torch.uint8, device="cuda:0")
    for k in range(2):
        r = eng.pics_convert(pids[2 * k:2 * k + 2], "rgba", out=out, matrix=9, colour=col)
        assert r.data_ptr() == out.data_ptr()
        g = host(out)
        for i in range(2):
            assert np.array_equal(g[i], want(hps[2 * k + i], p, "rgba", "uint8", "pq2020_srgb709")), (k, i)
    plain = host(eng.pics_convert(pids[:1], "rgba", out=out[:1], matrix=9))     # colour=None: oh_pics_convert as before
    assert np.array_equal(plain[0], CM.convert(coded(hps[0], p), p, "rgba", E.CONV_U8, matrix=9))
    with pytest.raises(ValueError):
        eng.pics_convert(pids[:2], "rgb", out=out, colour=col)                  # wrong shape
    for kw in (dict(fmt="planar"), dict(fmt="rgb", dtype=torch.uint8, colour=PIPELINES["srgb709_linear"][0])):
        kw.setdefault("colour", col)
        with pytest.raises(EngineError) as ei:
            eng.pics_convert(pids[:1], kw.pop("fmt"), **kw)
        assert ei.value.code == E.OH_E_UNSUPPORTED
    eng.close()


def _ordering(stream_of_engine):
    """no sync between the upload's stream work, the conversion and torch's read of it"""
    from openhevc_amd.engine import Engine
    eng = Engine(0, stream=stream_of_engine)
    p = params(416, 240, 10, 1)
    pids, hps = upload(eng, p, ("random",), np.random.default_rng(11))
    out = got(eng, pids, "rgb_planar", "float32", "pq2020_linear2020")
    snap = out.clone()                                                      # read on torch's current stream
    s = float(out.sum(dtype=torch.float64))
    eng.sync()
    wnt = M.convert(coded(hps[0], p), p, "rgb_planar", E.CONV_F32, PIPELINES["pq2020_linear2020"][0], matrix=9)
    assert np.array_equal(host(snap)[0], bits(wnt))
    ws = float(np.sum(wnt, dtype=np.float64))
    assert abs(s - ws) <= 1e-9 * max(1.0, abs(ws))
    eng.close()


def test_ordering_with_an_engine_stream_of_its_own():
    _ordering(None)


def test_ordering_with_an_engine_on_torchs_stream():
    _ordering(torch.cuda.current_stream().cuda_stream)


def test_argument_errors_write_nothing():
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    p = params(64, 32, 10, 1)
    pids, hps = upload(eng, p, ("random", "random"), np.random.default_rng(1))
    other, _ = upload(eng, params(64, 32, 8, 1), ("random",), np.random.default_rng(2))
    G = 4096
    cv = E.make_convert("rgb", E.CONV_U8, matrix=9)
    ok = PIPELINES["pq2020_srgb709"][0]
    ib = E.convert_image_bytes(p, cv)
    buf = torch.full((2 * ib + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()                                                # raw calls: no ordering against torch's stream
    dst = buf.data_ptr() + G

    def call(ids, cv, col, dst, stride, nbytes):
        return L.oh_pics_convert_colour(eng.h, (C.c_int * max(len(ids), 1))(*ids), len(ids), C.byref(cv),
                                        C.byref(col) if col is not None else None, C.c_void_p(dst), stride, nbytes)

    def changed(**kw):
        col = E.make_colour(16, 9, src_peak=1000, dst_peak=100)
        for k, v in kw.items():
            setattr(col, k, v)
        return col

    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    assert call(pids, cv, None, dst, ib, 2 * ib) == arg
    assert call([], cv, None, dst, ib, 0) == arg
    for kw in (dict(out_transfer=3), dict(tone=-1), dict(norm=2), dict(src_peak=0.0), dict(dst_peak=float("nan")), dict(white=float("inf")),
               dict(white=-203.0)):
        assert call(pids, cv, changed(**kw), dst, ib, 2 * ib) == arg, kw
    for kw in (dict(in_transfer=2), dict(in_primaries=5), dict(out_primaries=22), dict(in_transfer=18), dict(in_transfer=18, norm=1, src_peak=300.0),
               dict(dst_peak=1000.0), dict(out_transfer=E.COL_OUT["linear"])):
        assert call(pids, cv, changed(**kw), dst, ib, 2 * ib) == uns, kw
    assert call(pids, E.make_convert("rgb", E.CONV_U16, matrix=9), changed(out_transfer=E.COL_OUT["linear"]), dst, 2 * ib, 4 * ib) == uns
    assert call(pids, E.make_convert("planar", E.CONV_NATIVE), ok, dst, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("semiplanar", E.CONV_U8), ok, dst, ib, 2 * ib) == uns
    assert call(pids, E.make_convert("rgb", E.CONV_U8, matrix=4), ok, dst, ib, 2 * ib) == uns
    # what oh_pics_convert refuses
    assert call(pids, cv, ok, dst, ib, 2 * ib - 1) == arg                   # one byte short
    assert call(pids, cv, ok, dst, ib - 1, 2 * ib) == arg                   # stride below the image
    host_buf = np.zeros(2 * ib, np.uint8)
    assert call(pids, cv, ok, host_buf.ctypes.data, ib, 2 * ib) == arg      # a host pointer
    assert call(pids + other, cv, ok, dst, ib, 3 * ib) == arg               # mixed params
    assert call([pids[0], 999], cv, ok, dst, ib, 2 * ib) == arg             # unknown id
    assert call(pids, E.make_convert("rgb", E.CONV_U8, (1, 0, 0, 0), matrix=9), ok, dst, ib, 2 * ib) == arg
    assert call([], cv, ok, dst, ib, 0) == 0                                # n == 0: nothing to do
    cv16 = E.make_convert("rgb", E.CONV_U16, matrix=9)
    assert call(pids[:1], cv16, ok, dst, 2 * ib + 1, 2 * ib + 1) == arg     # stride, dst: multiples of the sample size
    assert call(pids[:1], cv16, ok, dst + 1, 2 * ib, 2 * ib) == arg
    # two 16 x 16 pictures into memory whose allocation ends one byte before the second image does
    small, _ = upload(eng, params(16, 16, 8, 1), ("random", "random"), np.random.default_rng(4))
    sb = E.convert_image_bytes(params(16, 16, 8, 1), cv)
    short, stride, claim = DR.one_byte_short(L, 2, sb)
    assert call(small, cv, ok, short.data_ptr(), stride, claim) == arg
    eng.sync()
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()) and bool((short == 0xA5).all()), "a refused call wrote into the destination"
    # the same buffer taken exactly: the guards around it stay untouched
    assert call(pids, cv, ok, dst, ib, 2 * ib) == 0
    eng.sync()
    b = buf.cpu().numpy()
    assert np.all(b[:G] == 0xA5) and np.all(b[G + 2 * ib:] == 0xA5)
    for i in range(2):
        assert np.array_equal(b[G + i * ib:G + (i + 1) * ib], want(hps[i], p, "rgb", "uint8", "pq2020_srgb709").ravel()), i
    eng.close()
