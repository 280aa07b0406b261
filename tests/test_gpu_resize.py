"""-m gpu: oh_pics_resize / Engine.pics_resize on the MI355X against the numpy model of tests/resize_model.py applied to what
oh_pic_download returns for the sources, bit for bit: chroma formats, bit depths, both filters, windows, shrinking / enlarging / mixed /
equal sizes, images smaller than their destination pictures (the replicated padding), more pictures than one launch set, reuse of
destinations, composition with the hashes / the conversion / the window download, the finished half of replayed stream fixtures, and
the argument rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import convert_model as CM                                                  # noqa: E402
import picture_hash as PH                                                   # noqa: E402
import resize_model as M                                                    # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu


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


def upload(eng, p, n, rng):
    pids = []
    for _ in range(n):
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, random_pic(p, rng))
        pids.append(pid)
    return pids


def want_coded(eng, pid, p, dp, size, filt, win):
    """the model on the downloaded source: the destination's coded planes"""
    src = coded(eng.pic_download(pid, p), p)
    return M.pad_to(M.resize(src, p.chroma_format_idc, p.bit_depth, size, filt, win), p.chroma_format_idc, (dp.width, dp.height))


def check(eng, pids, p, size, filt, win=(0, 0, 0, 0), out=None):
    dst, dwin = eng.pics_resize(pids, size, window=win, filter=filt, out=out)
    dp = eng._pic_params(dst[0])
    assert dwin == (0, dp.width - size[0], 0, dp.height - size[1])
    for s, d in zip(pids, dst):
        assert eng.pic_final_half(d) == 0
        got = coded(eng.pic_download(d, dp), dp)
        want = want_coded(eng, s, p, dp, size, filt, win)
        for c, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(g, w), (size, filt, win, s, c, np.argwhere(g != w)[:4].tolist())
    return dst, dwin


def case_id(c):
    return "_".join(str(v) if not isinstance(v, tuple) else "x".join(map(str, v)) for v in c)


# (source w, h, bit depth, chroma format, window, [sizes]): shrinking, enlarging, mixed, equal, not multiples of 8
GEOMS = [
    (64, 48, 8, 0, (0, 0, 0, 0), [(32, 24), (64, 48), (101, 37), (19, 131)]),
    (72, 40, 10, 0, (3, 1, 2, 5), [(68, 33), (25, 80), (299, 299)]),
    (416, 240, 8, 1, (0, 0, 0, 0), [(224, 224), (150, 86), (416, 240), (832, 120)]),
    (416, 240, 10, 1, (2, 4, 0, 2), [(410, 238), (150, 86), (64, 480)]),
    (264, 200, 9, 1, (0, 0, 0, 0), [(132, 100), (300, 298)]),
    (264, 200, 12, 1, (6, 2, 4, 8), [(112, 112), (256, 188)]),
    (264, 200, 8, 2, (2, 0, 1, 3), [(150, 87), (262, 196), (524, 51)]),
    (200, 136, 10, 2, (0, 0, 0, 0), [(298, 299), (50, 34)]),
    (200, 136, 12, 3, (1, 2, 3, 0), [(299, 299), (197, 133), (33, 207)]),
    (136, 72, 8, 3, (5, 0, 0, 1), [(131, 71), (67, 145)]),
    (136, 72, 9, 3, (0, 0, 0, 0), [(17, 9)]),
    (2048, 16, 8, 0, (0, 0, 0, 0), [(16, 16), (32, 128)]),                  # 128:1 and 1:8 on one picture
]


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("w,h,bd,cf,win,sizes", GEOMS, ids=[case_id(c[:5]) for c in GEOMS])
def test_resize_equals_the_model(w, h, bd, cf, win, sizes, filt):
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, cf)
    eng = Engine(0)
    pids = upload(eng, p, 2, np.random.default_rng(w + h + bd + cf))
    for size in sizes:
        check(eng, pids, p, size, filt, win)
    eng.close()


LARGE = [(3840, 2160, 10, (224, 224), "bilinear"), (3840, 2160, 10, (224, 224), "bicubic"), (3840, 2160, 8, (1920, 1080), "bilinear"),
         (3840, 2160, 10, (1920, 1080), "bicubic"), (7680, 4320, 8, (224, 224), "bicubic"), (7680, 4320, 10, (224, 224), "bilinear"),
         (416, 240, 10, (3328, 1920), "bicubic"), (416, 240, 8, (3328, 1920), "bilinear")]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("w,h,bd,size,filt", LARGE, ids=[case_id(c) for c in LARGE])
def test_large_pictures(w, h, bd, size, filt):
    from openhevc_amd.engine import Engine
    p = params(w, h, bd, 1)
    eng = Engine(0)
    pids = upload(eng, p, 1, np.random.default_rng(w + bd))
    check(eng, pids, p, size, filt)
    eng.close()


def test_more_pictures_than_one_launch_set_and_reused_destinations():
    """150 pictures: three launch sets of at most OH_RESIZE_MAX_PICS; then the same destinations take other sources"""
    from openhevc_amd.engine import Engine
    p = params(48, 32, 10, 1)
    eng = Engine(0)
    n = 2 * E.RESIZE_MAX_PICS + 22
    pids = upload(eng, p, n, np.random.default_rng(150))
    dst, _ = check(eng, pids, p, (30, 20), "bicubic", (2, 0, 0, 2))
    dst2, _ = check(eng, pids[::-1], p, (26, 24), "bilinear", out=dst)
    assert dst2 == dst
    eng.close()


def test_composition_with_hashes_conversion_and_window_download():
    import torch
    from openhevc_amd.engine import Engine
    p = params(200, 136, 10, 1)
    eng = Engine(0)
    pids = upload(eng, p, 3, np.random.default_rng(5))
    size, filt, win = (150, 86), "bicubic", (4, 0, 2, 0)
    dst, dwin = eng.pics_resize(pids, size, window=win, filter=filt)
    dp = eng._pic_params(dst[0])
    assert (dp.width, dp.height) == (152, 88) and dwin == (0, 2, 0, 2)
    rgb = eng.pics_convert(dst, "rgb_planar", dtype=torch.float16, window=dwin).cpu().numpy().view(np.uint16)
    hashes = [eng.pics_hash(dst, t) for t in range(3)]
    for i, (s, d) in enumerate(zip(pids, dst)):
        want = want_coded(eng, s, p, dp, size, filt, win)
        hp = F.HostPic(dp)
        for c in range(3):
            hp.visible(c)[...] = want[c]
        for t in range(3):
            assert hashes[t][i] == PH.host_pic_hash(hp, dp, t), (i, t)
        assert np.array_equal(rgb[i], CM.convert(want, dp, "rgb_planar", E.CONV_F16, dwin).view(np.uint16)), i
        image = eng.pic_download_window(d, dp, *dwin)
        for c in range(3):
            hs, vs = M.shifts(1, c)
            assert np.array_equal(image[c], want[c][:size[1] >> vs, :size[0] >> hs]), (i, c)
    eng.close()


GOLD = os.path.join(HERE, "golden", "streams")
FIXTURES = [os.path.join(GOLD, n + ".npz") for n in ("ipb_8b", "b_422_tools_8b", "i_444_ccp_10b_ctb16")]


def fixture(path):
    z = np.load(path)
    frames = []
    for k in range(int(z["n_pictures"][0])):
        pre = f"pic{k}_"
        frames.append(F.FrameFromArrays({key[len(pre):]: z[key] for key in z.files if key.startswith(pre)}))
    return frames


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_stream_fixtures_resize_the_finished_half(path):
    """replay a recorded stream on the engine and resize every picture behind the work list that finished it, without a sync in
    between; afterwards the images equal the model on the downloaded pictures and the sources are what they were"""
    from openhevc_amd.engine import Engine, remap_frame
    frames = fixture(path)
    eng = Engine(0)
    ids, jobs = {}, []
    for k, ff in enumerate(frames):
        f = ff.frame
        for i in [f.cur_pic] + [f.ref_pics[j] for j in range(F.OH_MAX_REFS) if f.ref_pics[j] >= 0]:
            if i not in ids:
                ids[i] = eng.pic_alloc(f.p)
        eng.frame_submit(remap_frame(f, ids))
        pid = ids[f.cur_pic]
        size = (f.p.width // 2 + 2 * (k % 3), f.p.height + 8) if k % 2 else (100, 60)
        filt = "bicubic" if k % 2 else "bilinear"
        dst, _ = eng.pics_resize([pid], size, filter=filt)
        md5 = eng.pics_md5([pid])[0]
        jobs.append((pid, dst[0], size, filt, md5, F.OhPicParams.from_buffer_copy(f.p), eng.pic_final_half(pid)))
        # the picture is overwritten when its id comes round again: check before that
        pid_, d, size, filt, md5, p, half = jobs[-1]
        dp = eng._pic_params(d)
        got = coded(eng.pic_download(d, dp), dp)
        want = want_coded(eng, pid_, p, dp, size, filt, (0, 0, 0, 0))
        for c in range(len(want)):
            assert np.array_equal(got[c], want[c]), (k, c)
        assert eng.pics_md5([pid_])[0] == md5 and eng.pic_final_half(pid_) == half, k
        eng.pic_free(d)
    eng.close()


def test_resize_follows_the_finished_half():
    """after a work list with SAO the finished picture lives in half 1: the resize, enqueued without a sync, reads that half"""
    from openhevc_amd.engine import Engine, remap_frame
    eng = Engine(0)
    rec = F.Recorder(params(416, 240, 8, 1))
    f = rec.synth(F.synth_params(0, 3, sao_pct=90), 0)
    pid = eng.pic_alloc(f.p)
    eng.frame_submit(remap_frame(f, {0: pid}))
    dst, _ = eng.pics_resize([pid], (224, 224), filter="bicubic")
    assert eng.pic_final_half(pid) == 1 and eng.pic_final_half(dst[0]) == 0
    before = eng.pics_md5([pid])[0]
    check(eng, [pid], f.p, (224, 224), "bicubic", out=dst)
    dp = eng._pic_params(dst[0])
    got = coded(eng.pic_download(dst[0], dp), dp)
    want = want_coded(eng, pid, f.p, dp, (224, 224), "bicubic", (0, 0, 0, 0))
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert eng.pics_md5([pid])[0] == before and eng.pic_final_half(pid) == 1
    eng.close()
    rec.close()


def test_argument_errors_write_nothing():
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    p = params(64, 32, 10, 1)
    rng = np.random.default_rng(1)
    src = upload(eng, p, 2, rng)
    dst = upload(eng, params(40, 24, 10, 1), 2, rng)
    other_src = upload(eng, params(64, 32, 8, 1), 1, rng)                  # other params among the sources
    other_dst = upload(eng, params(48, 24, 10, 1), 1, rng)                 # other params among the destinations
    dst8 = upload(eng, params(40, 24, 8, 1), 2, rng)                       # another bit depth
    dst444 = upload(eng, params(40, 24, 10, 3), 2, rng)                    # another chroma format
    wide = upload(eng, params(2080, 16, 10, 1), 2, rng)
    guarded = dst + other_dst + dst8 + dst444
    before = {d: eng.pics_md5([d])[0] for d in guarded}

    def call(s, d, size=(32, 16), win=(0, 0, 0, 0), filt=0, n=None):
        rs = E.OhResize(filt, E.OhWindow(*win), size[0], size[1])
        n = len(s) if n is None else n
        return L.oh_pics_resize(eng.h, (C.c_int * max(len(s), 1))(*s), (C.c_int * max(len(d), 1))(*d), n, C.byref(rs))

    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    assert call([src[0], 999], dst) == arg                                  # unknown pictures
    assert call(src, [dst[0], -1]) == arg
    assert call([src[0]] + other_src, dst) == arg                           # params differ among the sources
    assert call(src, [dst[0]] + other_dst) == arg                           # ... among the destinations
    assert call(src, [dst[0], dst[0]]) == arg                               # a destination twice
    assert call([src[0], dst[1]], [dst[0], src[0]]) == arg                  # both source and destination
    for win in ((1, 0, 0, 0), (0, 0, 0, 1), (64, 0, 0, 0), (0, 0, 16, 16), (-2, 0, 0, 0)):
        assert call(src, dst, win=win) == arg, win
    for size in ((0, 16), (32, 0), (-2, 16), (42, 16), (32, 26), (31, 16), (32, 15)):
        assert call(src, dst, size=size) == arg, size
    assert call(src, dst, filt=2) == arg and call(src, dst, filt=-1) == arg
    assert L.oh_pics_resize(eng.h, None, None, 2, C.byref(E.OhResize(0, E.OhWindow(0, 0, 0, 0), 32, 16))) == arg
    assert L.oh_pics_resize(eng.h, (C.c_int * 2)(*src), (C.c_int * 2)(*dst), 2, None) == arg
    assert call(src, dst, n=-1) == arg
    assert call(src, dst8) == uns
    assert call(src, dst444) == uns
    assert call(wide, dst, size=(16, 16)) == uns                            # 130:1
    assert call(src, dst, size=(40, 16), win=(0, 62, 0, 0)) == uns          # 1:20 (2 -> 40 luma columns)
    assert call([], [], n=0) == 0
    eng.sync()
    for d in guarded:
        assert eng.pics_md5([d])[0] == before[d], d
    assert call(src, dst) == 0                                              # and the same call with nothing wrong
    eng.sync()
    eng.close()
