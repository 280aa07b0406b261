"""oh_pic_upsample_blocks on the MI355X against the reference's own CTB up-sampling path (its default build: ff_upsample_block,
hevc_filter.c:1370-1426, run CTB by CTB by ref_up_blocks from oracle/_ref), and two-layer streams decoded with it end to end."""
import ctypes as C
import random

import numpy as np
import pytest

from openhevc_amd import frame as F
from openhevc_amd.engine import Engine, EngineError, remap_frame, upsample_blocks_defined
from oracle_lib import have_ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_ref(), reason="reference kernels not built (oracle/_ref)")]

OH_E_UNSUPPORTED = -4


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def ref_blocks(u, bl, bl_size, el_size, lc):
    from test_upsample_vs_ref import run_block_path
    return run_block_path(u, bl, bl_size, el_size, lc)


def engine_blocks(eng, u, bl, bl_size, el_size, lc, ctbs=None, fill=0):
    pb, pe = F.pic_params(*bl_size), F.pic_params(*el_size)
    b_id, e_id = eng.pic_alloc(pb), eng.pic_alloc(pe)
    try:
        eng.pic_upload(b_id, bl)
        eng.pic_upload(e_id, F.HostPic(pe, fill=fill))
        eng.pic_upsample_blocks(e_id, b_id, u, lc, ctbs)
        return eng.pic_download(e_id, pe)
    finally:
        eng.pic_free(b_id)
        eng.pic_free(e_id)


@pytest.mark.parametrize("lc", [5, 6])
def test_x1_5_beyond_2048_columns(eng, lc):
    """the x1.5 block slots position by exact thirds: from EL column 2048 on they pick other luma phases than the whole-picture
    slot; oh_pic_upsample_blocks is the block path bit for bit, oh_pic_upsample is not"""
    bl_size, el_size = (1376, 128), (2064, 192)
    u = F.upsample_setup(*bl_size, *el_size)
    assert u.idx == F.OH_UP_X1_5
    bl = F.HostPic(F.pic_params(*bl_size), rng=np.random.default_rng(11))
    want = ref_blocks(u, bl, bl_size, el_size, lc)
    got = engine_blocks(eng, u, bl, bl_size, el_size, lc)
    for c in range(3):
        assert np.array_equal(want.visible(c), got.visible(c)), c
    pb, pe = F.pic_params(*bl_size), F.pic_params(*el_size)
    b_id, e_id = eng.pic_alloc(pb), eng.pic_alloc(pe)
    eng.pic_upload(b_id, bl)
    eng.pic_upsample(e_id, b_id, u)
    whole = eng.pic_download(e_id, pe)
    eng.pic_free(b_id)
    eng.pic_free(e_id)
    xs = np.unique(np.nonzero(whole.visible(0) != want.visible(0))[1])
    assert len(xs) and xs.min() == 2048


def sweep_geometries(seed=7, count=120):
    """ratios 1, 1.5, 2 and generic ones in between, even offsets up to 12, phase alignment 0 / 1, CTBs of 16 .. 64"""
    rng = random.Random(seed)
    for _ in range(count):
        wb, hb = 8 * rng.randint(4, 60), 8 * rng.randint(3, 40)
        r = rng.choice([1.0, 1.5, 2.0, rng.uniform(1.0, 2.0), rng.uniform(1.0, 2.0)])
        we, he = max(wb, int(wb * r) // 8 * 8), max(hb, int(hb * r) // 8 * 8)
        if r == 1.5:
            wb, hb = wb // 16 * 16, hb // 16 * 16
            we, he = wb * 3 // 2, hb * 3 // 2
        win = tuple(2 * rng.randint(0, 6) if rng.random() < 0.5 else 0 for _ in range(4)) if rng.random() < 0.5 else (0, 0, 0, 0)
        if we - win[0] - win[1] < wb or he - win[2] - win[3] < hb:
            win = (0, 0, 0, 0)
        pa, lc = rng.choice([0, 0, 1]), rng.choice([4, 5, 6])
        yield (wb, hb), (we, he), win, pa, lc


def test_seeded_sweep_against_the_reference_block_path(eng):
    extra = [((64, 64), (144, 128), (0, 0, 0, 0), 0, 6), ((208, 120), (416, 240), (0, 0, 0, 0), 1, 6),
             ((200, 112), (416, 240), (8, 8, 8, 8), 0, 6), ((64, 32), (128, 64), (0, 0, 0, 0), 0, 6)]
    n = accepted = with_offsets = 0
    for it, (bl_size, el_size, win, pa, lc) in enumerate(list(sweep_geometries()) + extra):
        u = F.upsample_setup(*bl_size, *el_size, win, pa)
        ok, _ = upsample_blocks_defined(u, *bl_size, *el_size, lc)
        bl = F.HostPic(F.pic_params(*bl_size), rng=np.random.default_rng(500 + it))
        n += 1
        if not ok:
            with pytest.raises(EngineError, match=f"\\({OH_E_UNSUPPORTED}\\).*CTB"):
                engine_blocks(eng, u, bl, bl_size, el_size, lc)
            continue
        accepted += 1
        with_offsets += win != (0, 0, 0, 0) or pa != 0
        want = ref_blocks(u, bl, bl_size, el_size, lc)
        got = engine_blocks(eng, u, bl, bl_size, el_size, lc)
        for c in range(3):
            assert np.array_equal(want.visible(c), got.visible(c)), (bl_size, el_size, win, pa, lc, c)
    print(f"{n} geometries, {accepted} defined ({with_offsets} of them with offsets or phase alignment)")
    assert n >= 80 and accepted >= 60


@pytest.mark.parametrize("bl_size,el_size,lc", [((176, 96), (264, 144), 4), ((208, 120), (416, 240), 5), ((200, 112), (328, 200), 5)])
def test_partial_ctb_list_leaves_the_rest(eng, bl_size, el_size, lc):
    u = F.upsample_setup(*bl_size, *el_size)
    bl = F.HostPic(F.pic_params(*bl_size), rng=np.random.default_rng(3))
    want = ref_blocks(u, bl, bl_size, el_size, lc)
    ctb = 1 << lc
    cw, ch = -(-el_size[0] // ctb), -(-el_size[1] // ctb)
    some = sorted(np.random.default_rng(lc).choice(cw * ch, size=max(1, cw * ch // 3), replace=False).tolist())
    got = engine_blocks(eng, u, bl, bl_size, el_size, lc, some, fill=7)
    for c in range(3):
        s = 1 if c else 0
        mask = np.zeros(got.visible(c).shape, bool)
        for a in some:
            x0, y0 = (a % cw) * (ctb >> s), (a // cw) * (ctb >> s)
            mask[y0:y0 + (ctb >> s), x0:x0 + (ctb >> s)] = True
        assert np.array_equal(got.visible(c)[mask], want.visible(c)[mask]) and (got.visible(c)[~mask] == 7).all(), c


def test_refusals(eng):
    pb, pe = F.pic_params(208, 120), F.pic_params(416, 240)
    b_id, e_id = eng.pic_alloc(pb), eng.pic_alloc(pe)
    u = F.upsample_setup(208, 120, 416, 240)
    with pytest.raises(EngineError, match=f"\\({OH_E_UNSUPPORTED}\\)"):
        eng.pic_upsample_blocks(e_id, b_id, u, 6, el_conf_win=(0, 8, 0, 0))
    eng.pic_upsample_blocks(e_id, b_id, u, 6, [], el_conf_win=(0, 0, 0, 0))          # an empty list is nothing to do
    eng.pic_free(b_id)
    eng.pic_free(e_id)


def decode_two_layers(eng, data, block_path):
    """both layers' work lists from the hooked reference decoder; the inter-layer reference made by oh_pic_upsample_blocks (or
    oh_pic_upsample) from the base layer's picture; the enhancement layer's pictures in decode order"""
    import refdec
    ids, out = ({}, {}), []

    def on_picture(layer, f, cur, poc, il):
        mine = ids[layer]
        for i in [cur] + [f.ref_pics[k] for k in range(F.OH_MAX_REFS) if f.ref_pics[k] >= 0]:
            if i not in mine:
                mine[i] = eng.pic_alloc(f.p)
        if il is not None:
            slot, bl_id, up = il
            if block_path:
                eng.pic_upsample_blocks(mine[f.ref_pics[slot]], ids[0][bl_id], up, f.p.log2_ctb_size)
            else:
                eng.pic_upsample(mine[f.ref_pics[slot]], ids[0][bl_id], up)
        eng.frame_submit(remap_frame(f, mine))
        if layer == 1:
            out.append(eng.pic_download(mine[cur], f.p))
    try:
        n = refdec.record_layer_work_lists(data, on_picture)
    finally:
        for m in ids:
            for v in m.values():
                eng.pic_free(v)
    return n, out


@pytest.mark.parametrize("bl_size,el_size,n_pics", [((1408, 128), (2112, 192), 3), ((2560, 1440), (3840, 2160), 2)], ids=["2112x192", "3840x2160"])
def test_two_layer_streams_end_to_end(eng, bl_size, el_size, n_pics):
    import refdec
    from test_shvc_block_path_host import OH_STREAM_SHVC_BLOCK_PATH, write_stream_opts
    data, _ = write_stream_opts(*bl_size, 81, OH_STREAM_SHVC_BLOCK_PATH, n_pictures=n_pics, gop=1,
                                shvc_el_width=el_size[0], shvc_el_height=el_size[1])
    with refdec.captured_stderr():
        want = refdec.decode(data)
        n, got = decode_two_layers(eng, data, True)
    assert n == [n_pics, n_pics] and len(want) == len(got) == n_pics
    for k in range(n_pics):
        for c in range(3):
            assert np.array_equal(want[k][c], got[k].visible(c)), (k, c)
    if el_size[0] == 2112:                                  # the whole-picture slot is not what the reference decodes here
        with refdec.captured_stderr():
            _, whole = decode_two_layers(eng, data, False)
        assert any(not np.array_equal(want[k][0], whole[k].visible(0)) for k in range(n_pics))
