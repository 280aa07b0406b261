"""-m gpu: oh_pics_compose / Engine.pics_compose on the MI355X against the numpy model of tests/compose_model.py, every coded plane bit
for bit: chroma formats and bit depths, clipping, the seams of the kernel's 16-byte granules and of its tiles, the fill, the finished
half, batches of more than one launch set, alpha planes with any strides, calls back to back, pictures that oh_pics_import and
oh_pics_resize made, the ordering with torch, and the argument rules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch                                                                # noqa: F401  before the engine library: one HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import compose_model as PM                                                  # noqa: E402
import convert_model as CM                                                  # noqa: E402
import import_model as IM                                                   # noqa: E402
import picture_hash as PH                                                   # noqa: E402
from openhevc_amd import engine as E                                        # noqa: E402
from openhevc_amd import frame as F                                         # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def random_pic(p, rng):
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        v[...] = rng.integers(0, 1 << p.bit_depth, v.shape, dtype=v.dtype)
    return hp


def up(eng, p, hp):
    """(id, HostPic) of an uploaded picture"""
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, hp)
    return pid, hp


def new(eng, p, rng):
    return up(eng, p, random_pic(p, rng))


def coded(hp):
    return [hp.visible(c) for c in range(len(hp.planes))]


def dev_alpha(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


def random_alpha(rng, *shape):
    """0 .. 255 with 0 and 255 in it"""
    a = rng.integers(0, 256, shape).astype(np.uint8)
    flat = a.reshape(-1)
    flat[0], flat[-1] = 0, 255
    flat[rng.integers(0, flat.size, max(flat.size // 8, 1))] = 255
    flat[rng.integers(0, flat.size, max(flat.size // 8, 1))] = 0
    return a


def model(p, dst, specs, fill=None):
    """per destination the coded planes the call leaves.  dst: [(id, HostPic)]; specs: dicts with "src", one (id, HostPic) for all
    destinations or a list of one per destination, "rect", "at", "opacity", and "alpha", an (h, w) or (n, h, w) array"""
    want = []
    for i, (_, hp) in enumerate(dst):
        ml = []
        for s in specs:
            src = s["src"][i] if isinstance(s["src"], list) else s["src"]
            a = s.get("alpha")
            if a is not None and a.ndim == 3:
                a = a[i]
            ml.append({"src": coded(src[1]), "rect": s.get("rect"), "at": s.get("at", (0, 0)), "opacity": s.get("opacity", 256), "alpha": a})
        want.append(PM.compose(coded(hp), p, ml, fill))
    return want


def layers_of(specs):
    out = []
    for s in specs:
        src = [q[0] for q in s["src"]] if isinstance(s["src"], list) else s["src"][0]
        al = s.get("alpha_t")
        if al is None and s.get("alpha") is not None:
            al = dev_alpha(s["alpha"])
        out.append(E.Layer(src, s.get("rect"), s.get("at", (0, 0)), s.get("opacity", 256), al))
    return out


def verify(eng, p, dst, want, what=None, hashes=False):
    """the destinations on the device equal `want`; their HostPics then hold it too, so that calls chain"""
    for i, (pid, hp) in enumerate(dst):
        got = eng.pic_download(pid, p)
        for c in range(F.n_planes(p)):
            assert np.array_equal(got.visible(c), want[i][c]), (what, i, c, np.argwhere(got.visible(c) != want[i][c])[:4])
            hp.visible(c)[...] = want[i][c]
        if hashes:
            assert eng.pics_hash([pid], 2)[0] == PH.picture_hash(coded(hp), p.bit_depth, 2), (what, i)


def check(eng, p, dst, specs, fill=None, what=None, hashes=False):
    """one call against the model"""
    want = model(p, dst, specs, fill)
    ids = [d[0] for d in dst]
    assert eng.pics_compose(ids, layers_of(specs), fill=fill) == ids
    verify(eng, p, dst, want, what, hashes)
    return want


FORMATS = [(8, 1), (10, 1), (10, 2), (12, 3), (8, 0)]                       # bit depth, chroma_format_idc


@pytest.mark.parametrize("bd,cf", FORMATS, ids=[f"{b}b_cf{c}" for b, c in FORMATS])
def test_formats_equal_the_model(bd, cf):
    """a 96 x 40 destination, sources of 64 x 32 and 96 x 40: an opaque layer, a layer of opacity 128 and a layer with a random alpha
    plane, each alone and the three, which overlap, in one call; the same three in another order give another picture"""
    from openhevc_amd.engine import Engine
    p, ps = params(96, 40, bd, cf), params(64, 32, bd, cf)
    rng = np.random.default_rng(bd * 5 + cf)
    eng = Engine(0)
    small, big = new(eng, ps, rng), new(eng, p, rng)
    opaque = {"src": small, "at": (8, 4)}
    half = {"src": big, "rect": (16, 8, 48, 24), "at": (40, 12), "opacity": 128}
    alpha = {"src": small, "at": (24, 6), "alpha": random_alpha(rng, 32, 64), "opacity": 256}
    base = random_pic(p, rng)
    for k, spec in enumerate((opaque, half, alpha)):
        check(eng, p, [up(eng, p, base.copy())], [spec], what=("alone", k), hashes=True)
    d1, d2 = up(eng, p, base.copy()), up(eng, p, base.copy())
    w1 = check(eng, p, [d1], [opaque, half, alpha], what="three")
    w2 = check(eng, p, [d2], [alpha, half, opaque], what="three, other order")
    assert any(not np.array_equal(x, y) for x, y in zip(w1[0], w2[0]))
    assert all(np.array_equal(x[30:, :4], b[30:, :4]) for x, b in zip(w1[0][:1], coded(base)[:1]))   # outside every layer: untouched
    eng.close()


@pytest.mark.parametrize("bd,cf", [(10, 1), (8, 3)], ids=["10b_cf1", "8b_cf3"])
def test_clipping(bd, cf):
    """negative dx, dy beyond the bottom, both at once with an alpha plane (its origin moves with the rectangle), a layer wholly
    outside, the smallest rectangle and a rectangle in the source's bottom-right corner"""
    from openhevc_amd.engine import Engine
    p, ps = params(96, 40, bd, cf), params(64, 32, bd, cf)
    rng = np.random.default_rng(bd + cf)
    eng = Engine(0)
    src, dst = new(eng, ps, rng), new(eng, p, rng)
    sw, sh = (2, 2) if cf == 1 else (1, 1)
    before = [c.copy() for c in coded(dst[1])]
    check(eng, p, [dst], [{"src": src, "at": (-20, 4)}], what="left")
    check(eng, p, [dst], [{"src": src, "at": (50, 30), "opacity": 77}], what="bottom and right")
    check(eng, p, [dst], [{"src": src, "at": (-30, -10), "alpha": random_alpha(rng, 32, 64)},
                          {"src": src, "at": (70, 22), "alpha": random_alpha(rng, 32, 64), "opacity": 201}], what="corners with alpha")
    now = [c.copy() for c in coded(dst[1])]
    for at in ((96, 0), (0, 40), (-64, 0), (0, -32), (4000, -4000), (2 ** 31 - 2, 0), (0, -2 ** 31), (-2 ** 31, 2 ** 31 - 2)):
        check(eng, p, [dst], [{"src": src, "at": at}], what=("outside", at))
    assert all(np.array_equal(x, y) for x, y in zip(now, coded(dst[1]))) and any(not np.array_equal(x, y) for x, y in zip(before, now))
    check(eng, p, [dst], [{"src": src, "rect": (10 * sw, 3 * sh, sw, sh), "at": (46 * sw // 2 * 2, 18)}], what="smallest")
    check(eng, p, [dst], [{"src": src, "rect": (64 - sw, 32 - sh, sw, sh), "at": (96 - sw, 40 - sh), "alpha": random_alpha(rng, sh, sw)},
                          {"src": src, "rect": (64 - 16, 32 - 8, 16, 8), "at": (2, 2)}], what="bottom-right corner of the source")
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_granule_seams(bd):
    """4:2:0, where a luma granule of 16 bytes is 16 / 8 samples and a chroma granule covers twice as many luma columns: layers that
    start and end at every position relative to the granules, opaque (the destination is not read where a granule is covered), with
    opacity and with alpha"""
    from openhevc_amd.engine import Engine
    p, ps = params(64, 24, bd, 1), params(64, 16, bd, 1)
    rng = np.random.default_rng(bd)
    eng = Engine(0)
    src, dst = new(eng, ps, rng), new(eng, p, rng)
    for dx in (2, 6, 14, 18, 30):
        for w in (2, 14, 16, 18, 34):
            a = random_alpha(rng, 8, w)
            check(eng, p, [dst], [{"src": src, "rect": (w % 8 * 2, 0, w, 8), "at": (dx, 0)},
                                  {"src": src, "rect": (6, 8, w, 8), "at": (dx, 8), "alpha": a},
                                  {"src": src, "rect": (0, 4, w, 8), "at": (dx, 16), "opacity": 100}], what=(dx, w))
    eng.close()


@pytest.mark.parametrize("bd", (8, 10))
def test_tile_seams(bd):
    """a 4:4:4 destination one granule wider and one row taller than the kernel's tile, rounded up to a coded size: layers across the
    tile's right and lower seam at odd positions, and a whole-picture layer over all tiles"""
    from openhevc_amd.engine import Engine
    gs = 16 if bd == 8 else 8                                               # samples of a granule
    tw, th = E.CPS_TW * gs, E.CPS_TH
    w, h = tw + gs, (th + 1 + 7) // 8 * 8
    assert w % 8 == 0 and h > th
    p, ps = params(w, h, bd, 3), params(40, 8, bd, 3)
    rng = np.random.default_rng(40 + bd)
    eng = Engine(0)
    src, whole, dst = new(eng, ps, rng), new(eng, p, rng), new(eng, p, rng)
    check(eng, p, [dst], [{"src": src, "rect": (1, 0, 7, 5), "at": (tw - 3, th - 2), "alpha": random_alpha(rng, 5, 7)},
                          {"src": src, "rect": (3, 1, 37, 7), "at": (tw - 19, 1), "opacity": 255},
                          {"src": src, "rect": (0, 0, 11, 3), "at": (w - 11, h - 3)}], what="seams")
    check(eng, p, [dst], [{"src": whole, "opacity": 130, "alpha": random_alpha(rng, h, w)}], what="whole with alpha")
    check(eng, p, [dst], [{"src": whole}], what="whole, a copy")
    assert all(np.array_equal(x, y) for x, y in zip(coded(dst[1]), coded(whole[1])))
    eng.close()


@pytest.mark.parametrize("bd,cf", [(8, 1), (10, 1), (12, 3), (8, 0)], ids=["8b_cf1", "10b_cf1", "12b_cf3", "8b_cf0"])
def test_fill(bd, cf):
    """the fill alone over random samples (nothing of them survives), with layers, and the values 0 and the maximum code"""
    from openhevc_amd.engine import Engine
    p, ps = params(72, 40, bd, cf), params(32, 16, bd, cf)
    top = (1 << bd) - 1
    rng = np.random.default_rng(bd + 3 * cf)
    eng = Engine(0)
    src, dst = new(eng, ps, rng), new(eng, p, rng)
    want = check(eng, p, [dst], [], fill=(16 << (bd - 8), 1 << (bd - 1), 1 << (bd - 1)), what="black", hashes=True)
    assert all((pl == (16 << (bd - 8) if c == 0 else 1 << (bd - 1))).all() for c, pl in enumerate(want[0]))
    check(eng, p, [dst], [{"src": src, "at": (20, 12)}, {"src": src, "at": (40, 20), "alpha": random_alpha(rng, 16, 32), "opacity": 250},
                          {"src": src, "at": (-8, 30), "opacity": 128}], fill=(top, 0, top), what="fill and layers")
    check(eng, p, [dst], [], fill=(0, 0, 0), what="zero")
    want = check(eng, p, [dst], [], fill=(top, top, top), what="maximum")
    assert all((pl == top).all() for pl in want[0])
    if cf == 0:                                                             # fill[1..2] of a 4:0:0 picture are not read
        ids = [dst[0]]
        assert eng.pics_compose(ids, [], fill=(7, -1, 1 << 20)) == ids
        verify(eng, p, [dst], model(p, [dst], [], (7,)), "4:0:0")
    eng.close()


def test_the_finished_half_is_composed():
    """an uploaded picture whose finished half is then declared to be half 1: the fill goes there, the half stays the finished one,
    and the upload in half 0 is untouched"""
    from openhevc_amd.engine import Engine
    p = params(64, 32, 10, 1)
    rng = np.random.default_rng(9)
    eng = Engine(0)
    pid, hp = new(eng, p, rng)
    eng.pic_set_final_half(pid, 1)
    eng.pics_compose([pid], [], fill=(100, 200, 300))
    assert eng.pic_final_half(pid) == 1
    got = eng.pic_download(pid, p)
    assert all((got.visible(c) == v).all() for c, v in enumerate((100, 200, 300)))
    eng.pic_set_final_half(pid, 0)
    got = eng.pic_download(pid, p)
    assert all(np.array_equal(got.visible(c), hp.visible(c)) for c in range(3))
    # and a source is read from its finished half: the filled one
    eng.pic_set_final_half(pid, 1)
    dst = new(eng, p, rng)
    flat = F.HostPic(p)
    for c, v in enumerate((100, 200, 300)):
        flat.visible(c)[...] = v
    want = model(p, [dst], [{"src": (pid, flat), "rect": (0, 0, 32, 16), "at": (8, 8), "opacity": 128}])
    eng.pics_compose([dst[0]], [E.Layer(pid, (0, 0, 32, 16), (8, 8), 128)])
    verify(eng, p, [dst], want, "source half")
    eng.close()


def test_batches():
    """three destinations with a source each, a logo shared by all and an alpha plane each; 65 destinations of 16 x 16 — two launch
    sets — with a source each; sixteen layers as a 4 x 4 contact sheet"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(65)
    eng = Engine(0)
    p, pl = params(96, 40, 10, 1), params(32, 16, 10, 1)
    dst = [new(eng, p, rng) for _ in range(3)]
    srcs, logo = [new(eng, p, rng) for _ in range(3)], new(eng, pl, rng)
    check(eng, p, dst, [{"src": srcs, "rect": (8, 8, 64, 24), "at": (16, 4), "opacity": 192},
                        {"src": logo, "at": (60, 20), "alpha": random_alpha(rng, 3, 16, 32)}], what="three")
    p = params(16, 16, 8, 1)
    n = E.CONV_MAX_PICS + 1
    dst, srcs = [new(eng, p, rng) for _ in range(n)], [new(eng, p, rng) for _ in range(n)]
    check(eng, p, dst, [{"src": srcs, "rect": (2, 2, 12, 10), "at": (4, 2), "alpha": random_alpha(rng, 10, 12)},
                        {"src": srcs[::-1], "rect": (0, 0, 8, 8), "at": (8, 8), "opacity": 64}], what="two launch sets")
    p, pt = params(64, 32, 8, 1), params(16, 8, 8, 1)
    tiles = [new(eng, pt, rng) for _ in range(16)]
    dst = [new(eng, p, rng)]
    assert len(tiles) == E.COMPOSE_MAX_LAYERS
    want = check(eng, p, dst, [{"src": t, "at": (16 * (k % 4), 8 * (k // 4))} for k, t in enumerate(tiles)], what="contact sheet")
    for k, t in enumerate(tiles):
        assert np.array_equal(want[0][0][8 * (k // 4):8 * (k // 4) + 8, 16 * (k % 4):16 * (k % 4) + 16], t[1].visible(0))
    eng.close()


def test_alpha_addressing():
    """the [..., 3] view of an (h, w, 4) tensor (pixel stride 4), rows inside a wider tensor (a row stride larger than the row), an odd
    base address, and a stride of 0 along an axis, on 8 and 10 bit"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(4)
    eng = Engine(0)
    for bd in (8, 10):
        p, ps = params(96, 40, bd, 1), params(64, 32, bd, 1)
        src, dst = new(eng, ps, rng), [new(eng, p, rng) for _ in range(2)]
        rgba = torch.from_numpy(rng.integers(0, 256, (32, 64, 4)).astype(np.uint8)).to(DEV)
        v = rgba[..., 3]
        assert v.stride() == (256, 4)
        check(eng, p, dst, [{"src": src, "at": (16, 4), "alpha": v.cpu().numpy(), "alpha_t": v}], what="pixel stride 4")
        rgba2 = torch.from_numpy(rng.integers(0, 256, (2, 32, 64, 4)).astype(np.uint8)).to(DEV)
        v = rgba2[..., 3]
        check(eng, p, dst, [{"src": src, "at": (-6, 12), "alpha": v.cpu().numpy(), "alpha_t": v, "opacity": 199}], what="per destination, stride 4")
        wide = torch.from_numpy(rng.integers(0, 256, (40, 100)).astype(np.uint8)).to(DEV)
        v = wide[5:37, 21:85]
        assert v.stride() == (100, 1) and v.data_ptr() % 2 == 1
        check(eng, p, dst, [{"src": src, "at": (30, 8), "alpha": v.cpu().numpy(), "alpha_t": v}], what="row stride, odd base")
        flat = torch.from_numpy(rng.integers(0, 256, (1 + 24 * 50,)).astype(np.uint8)).to(DEV)
        v = flat[1:].view(24, 50)[:, :48]
        assert v.data_ptr() % 2 == 1
        check(eng, p, dst, [{"src": src, "rect": (8, 4, 48, 24), "at": (40, 10), "alpha": v.cpu().numpy(), "alpha_t": v}], what="odd base")
        row = torch.from_numpy(rng.integers(0, 256, (64,)).astype(np.uint8)).to(DEV)
        v = row.expand(32, 64)
        assert v.stride() == (0, 1)
        check(eng, p, dst, [{"src": src, "at": (2, 2), "alpha": v.cpu().numpy(), "alpha_t": v}], what="row stride 0")
    eng.close()


def test_calls_back_to_back():
    """a call of one layer and at once a call of sixteen layers on forty destinations, whose table is larger (the scratch grows between
    them), with no wait between; then the same call twice"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(16)
    eng = Engine(0)
    p, ps = params(64, 32, 10, 1), params(32, 16, 10, 1)
    first, many = [new(eng, p, rng)], [new(eng, p, rng) for _ in range(40)]
    srcs = [[new(eng, ps, rng) for _ in range(40)] for _ in range(2)]
    one = [{"src": srcs[0][0], "at": (10, 6), "opacity": 128}]
    a = random_alpha(rng, 40, 16, 32)
    sixteen = [{"src": srcs[k % 2] if k % 3 else srcs[k % 2][5], "at": (4 * k - 8, 2 * k - 4), "opacity": 96 + 10 * k,
                "alpha": a if k % 4 == 1 else None} for k in range(16)]
    w_one, w_many = model(p, first, one), model(p, many, sixteen)
    eng.pics_compose([first[0][0]], layers_of(one))
    eng.pics_compose([d[0] for d in many], layers_of(sixteen))
    verify(eng, p, first, w_one, "one layer")
    verify(eng, p, many, w_many, "sixteen layers")
    w1 = model(p, first, one)                                               # on what the first call left
    for d, w in zip(first, w1):
        for c in range(3):
            d[1].visible(c)[...] = w[c]
    w2 = model(p, first, one)
    lay = layers_of(one)
    eng.pics_compose([first[0][0]], lay)
    eng.pics_compose([first[0][0]], lay)
    verify(eng, p, first, w2, "the same call twice")
    assert any(not np.array_equal(x, y) for x, y in zip(w1[0], w2[0]))
    eng.close()


def test_with_import_resize_and_convert():
    """an RGBA overlay: oh_pics_import makes the picture, its [..., 3] view is the alpha plane, oh_pics_convert of the composed
    destination equals the models chained; a resized picture on a filled canvas at an offset (letterbox)"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(33)
    eng = Engine(0)
    p, po = params(96, 48, 10, 1), params(48, 24, 10, 1)
    rgba = rng.integers(0, 256, (1, 24, 48, 4)).astype(np.uint8)
    t = torch.from_numpy(rgba).to(DEV)
    ov, win = eng.pics_import(t, "rgba", bit_depth=10, chroma_format_idc=1, matrix=1)
    assert win == (0, 0, 0, 0)
    dst = new(eng, p, rng)
    eng.pics_compose([dst[0]], [E.Layer(ov[0], None, (30, 14), 256, t[0, :, :, 3])])
    got = eng.pics_convert([dst[0]], "rgb", dtype=torch.uint8, matrix=1).cpu().numpy()[0]
    ov_planes = IM.import_picture(rgba[0], po, "rgba", E.CONV_U8, matrix=1)
    want = PM.compose(coded(dst[1]), p, [{"src": ov_planes, "at": (30, 14), "alpha": rgba[0, :, :, 3]}])
    verify(eng, p, [dst], [want], "overlay")
    assert np.array_equal(got, CM.convert(want, p, "rgb", E.CONV_U8, matrix=1))
    # letterbox: 96 x 48 resized to 64 x 32 in the middle of a black 96 x 48 canvas
    pic = new(eng, p, rng)
    small, swin = eng.pics_resize([pic[0]], (64, 32))
    sp = eng._pic_params(small[0])
    assert (sp.width, sp.height) == (64, 32) and swin == (0, 0, 0, 0)
    canvas = new(eng, p, rng)
    eng.pics_compose([canvas[0]], [E.Layer(small[0], None, (16, 8))], fill=(64, 512, 512))
    res = eng.pic_download(small[0], sp)
    want = PM.compose(coded(canvas[1]), p, [{"src": coded(res), "at": (16, 8)}], (64, 512, 512))
    verify(eng, p, [canvas], [want], "letterbox")
    assert (want[0][:8] == 64).all() and (want[1][:, :8] == 512).all() and not (want[0][8:40, 16:80] == 64).all()
    eng.close()


def test_ordering_with_torch():
    """the alpha plane comes out of a torch kernel on torch's current stream immediately before the call and is overwritten immediately
    after it, twenty times, with no host wait in between: every result is right"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(20)
    eng = Engine(0)
    p = params(256, 128, 8, 1)
    src = new(eng, p, rng)
    dst = [new(eng, p, rng) for _ in range(20)]
    idx = torch.arange(128 * 256, dtype=torch.int64, device=DEV)
    n = np.arange(128 * 256, dtype=np.int64)
    alphas = []
    for k in range(20):
        a = ((idx * (2654435761 + 2 * k)) >> 9).remainder(256).to(torch.uint8).reshape(128, 256)     # queued, not waited for
        eng.pics_compose([dst[k][0]], [E.Layer(src[0], None, (0, 0), 256 - k, a)])
        a.fill_(k)                                                          # torch's stream waits for the engine's read
        del a
        alphas.append((((n * (2654435761 + 2 * k)) >> 9) % 256).astype(np.uint8).reshape(128, 256))
    junk = torch.full((128 * 256,), 99, dtype=torch.uint8, device=DEV)
    for k in range(20):
        want = PM.compose(coded(dst[k][1]), p, [{"src": coded(src[1]), "opacity": 256 - k, "alpha": alphas[k]}])
        verify(eng, p, [dst[k]], [want], ("ordering", k))
    assert int(junk[0]) == 99
    eng.close()


def test_argument_errors_write_nothing():
    """every OH_E_ARG and OH_E_UNSUPPORTED case of ohevc_hip.h through the raw C call: refused on the host, the destinations' hashes
    stay; n == 0 and n_layers == 0 are fine and write nothing either"""
    from openhevc_amd.engine import Engine
    eng = Engine(0)
    L = eng.L
    rng = np.random.default_rng(1)
    p, ps = params(64, 32, 10, 1), params(32, 16, 10, 1)
    dst = [new(eng, p, rng)[0] for _ in range(2)]
    src = [new(eng, ps, rng)[0] for _ in range(2)]
    p8, p444, pbig = params(32, 16, 8, 1), params(32, 16, 10, 3), params(72, 40, 10, 1)
    s8, s444, sbig, dbig = new(eng, p8, rng)[0], new(eng, p444, rng)[0], new(eng, pbig, rng)[0], new(eng, pbig, rng)[0]
    alpha = torch.full((2, 16, 32), 200, dtype=torch.uint8, device=DEV)
    host_alpha = np.zeros((2, 16, 32), np.uint8)
    torch.cuda.synchronize()                                                # raw calls: no ordering against torch's stream

    def hashes():
        return [eng.pics_hash([pid], 0) for pid in dst + [dbig]]

    before = hashes()
    keep = []

    def ids(v):
        a = (C.c_int32 * max(len(v), 1))(*v)
        keep.append(a)
        return a

    def layer(src_ids=src, rect=(0, 0, 32, 16), at=(0, 0), opacity=256, alpha_ptr=None, strides=(1, 32, 512)):
        o = E.OhLayer()
        o.src_ids = C.cast(ids(src_ids), C.POINTER(C.c_int32)) if src_ids is not None else None
        o.sx, o.sy, o.w, o.h = rect
        o.dx, o.dy = at
        o.opacity = opacity
        o.alpha = alpha_ptr
        o.alpha_pixel_stride, o.alpha_row_stride, o.alpha_image_stride = strides
        return o

    def call(layers, d=dst, flags=0, fill=(0, 0, 0), n=None, n_layers=None, null_layers=False, cp_null=False):
        arr = (E.OhLayer * max(len(layers), 1))(*layers)
        cp = E.OhCompose(flags, (C.c_int32 * 3)(*fill), len(layers) if n_layers is None else n_layers, None if null_layers else arr)
        return L.oh_pics_compose(eng.h, ids(d) if d is not None else None, len(d or []) if n is None else n, None if cp_null else C.byref(cp))

    arg, uns = E.OH_E_ARG, E.OH_E_UNSUPPORTED
    ok = layer()
    assert L.oh_pics_compose(None, ids(dst), 2, C.byref(E.OhCompose())) == arg                  # null e, cp, id arrays
    assert call([ok], cp_null=True) == arg and call([ok], d=None, n=2) == arg and call([layer(src_ids=None)]) == arg
    assert call([ok], n=-1) == arg
    assert call([ok], n_layers=17) == arg and call([ok], n_layers=-1) == arg and call([ok], null_layers=True) == arg
    assert call([ok], d=[dst[0], 999]) == arg and call([layer(src_ids=[src[0], 999])]) == arg     # unknown pictures
    assert call([ok], d=[dst[0], dbig]) == arg and call([layer(src_ids=[src[0], sbig])]) == arg   # params differ
    assert call([ok], d=[dst[0], dst[0]]) == arg                                                # a destination twice
    assert call([layer(src_ids=[src[0], dst[0]])]) == arg and call([layer(src_ids=[dst[1], src[1]])]) == arg      # destination and source
    for rect in ((0, 0, 0, 16), (0, 0, 32, 0), (0, 0, -2, 16), (2, 0, 32, 16), (0, 2, 32, 16), (-2, 0, 8, 8), (0, -2, 8, 8), (0, 0, 34, 16),
                 (0, 0, 32, 18), (1, 0, 8, 8), (0, 1, 8, 8), (0, 0, 7, 8), (0, 0, 8, 7)):
        assert call([ok, layer(rect=rect)]) == arg, rect                                        # empty, outside the source, misaligned
    for at in ((1, 0), (0, 1), (-3, 0), (0, 31)):
        assert call([layer(at=at)]) == arg, at
    for op in (-1, 257, 1 << 20):
        assert call([layer(opacity=op)]) == arg, op
    for flags in (2, 3, -1, 1 << 30):
        assert call([ok], flags=flags) == arg, flags
    for fill in ((1024, 0, 0), (0, -1, 0), (0, 0, 4096)):
        assert call([ok], flags=E.COMPOSE_FILL, fill=fill) == arg, fill
    ap = alpha.data_ptr()
    assert call([layer(alpha_ptr=host_alpha.ctypes.data)]) == arg                               # not device memory
    assert call([layer(alpha_ptr=ap, strides=(-1, 32, 512))]) == arg and call([layer(alpha_ptr=ap, strides=(1, -32, 512))]) == arg
    # strides that leave every allocation of the device: the second image, row 15, pixel 31 lie behind the end of alpha's
    assert call([layer(alpha_ptr=ap, strides=(1, 32, 1 << 40))]) == arg
    assert call([layer(alpha_ptr=ap, strides=(1, 1 << 38, 0))]) == arg
    assert call([layer(alpha_ptr=ap, strides=(1 << 38, 32, 512))]) == arg
    assert call([layer(alpha_ptr=ap, strides=((1 << 63) - 1, (1 << 63) - 1, (1 << 63) - 1))]) == arg
    assert call([layer(src_ids=[s8, s8])]) == uns and call([layer(src_ids=[s444, s444])]) == uns  # another bit depth, another chroma format
    eng.sync()
    assert hashes() == before, "a refused call wrote into a picture"
    assert call([], d=[], n=0) == 0 and call([ok], d=None, n=0) == 0                            # n == 0
    assert call([]) == 0 and call([], null_layers=True) == 0                                    # no layers, no fill: nothing to do
    assert call([layer(at=(64, 0)), layer(at=(-32, -16))]) == 0                                 # wholly outside
    eng.sync()
    assert hashes() == before
    assert call([layer(alpha_ptr=ap), layer(at=(16, 8), alpha_ptr=ap + 512, strides=(1, 32, 0))]) == 0      # the tensor taken exactly
    eng.sync()
    after = hashes()
    assert after[0] != before[0] and after[1] != before[1] and after[2] == before[2]
    eng.close()
