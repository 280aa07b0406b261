"""-m gpu: CRC and checksum picture hashes (H.265 Annex D, decoded-picture-hash SEI hash_type 1 and 2) computed on the MI355X by
oh_pics_hash against the host models of tests/picture_hash.py, on synthetic pictures, on the engine's replay of the recorded stream
fixtures, and end to end against SEIs written into streams (where the hooked reference front end in oracle/_ref travelled)."""
import glob
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import picture_hash as PH                                                   # noqa: E402
from openhevc_amd import frame as F                                          # noqa: E402

pytestmark = pytest.mark.gpu

GEOMETRIES = [(64, 64, 8, 1), (416, 240, 8, 1), (416, 240, 10, 1), (200, 136, 10, 3), (264, 200, 8, 2), (72, 40, 8, 0),
              (1920, 1080, 10, 1), (8, 8, 8, 1), (24, 8, 8, 1), (3840, 2160, 10, 1), (7680, 4320, 8, 1)]
COMPANIONS = [(72, 40, 8, 0), (200, 136, 12, 2), (24, 8, 10, 3)]           # other depths / formats in the same call


def params(w, h, bd, cf):
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=cf)


def random_pic(p, rng):
    hp = F.HostPic(p)
    for c in range(F.n_planes(p)):
        v = hp.visible(c)
        v[...] = rng.integers(0, 1 << p.bit_depth, v.shape, dtype=v.dtype)
    return hp


def md5_shape(digests):
    return [(0, list(d)) for d in digests]


@pytest.mark.parametrize("w,h,bd,cf", GEOMETRIES, ids=[f"{g[0]}x{g[1]}_{g[2]}b_cf{g[3]}" for g in GEOMETRIES])
def test_crc_and_checksum_on_the_gpu_equal_the_host_model(w, h, bd, cf):
    """several pictures per call, mixed bit depths and chroma formats; type 0 is oh_pics_md5; planes a monochrome picture lacks are 0"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(w * 131 + h * 7 + bd + cf)
    eng = Engine(0)
    shapes = [params(w, h, bd, cf)] * 2 + [params(*g) for g in COMPANIONS]
    pids, hps = [], []
    for p in shapes:
        hp = random_pic(p, rng)
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        pids.append(pid)
        hps.append(hp)
    for t in (1, 2):
        got = eng.pics_hash(pids, t)
        want = [PH.host_pic_hash(hp, p, t) for hp, p in zip(hps, shapes)]
        assert got == want, t
    assert eng.pics_hash(pids, 0) == md5_shape(eng.pics_md5(pids))
    assert eng.pics_hash(pids, 0) == [PH.host_pic_hash(hp, p, 0) for hp, p in zip(hps, shapes)]
    mono = [k for k, p in enumerate(shapes) if p.chroma_format_idc == 0]
    for t in (1, 2):
        got = eng.pics_hash([pids[k] for k in mono], t)
        assert all(v[1][1] == 0 and v[1][2] == 0 for v in got)
    eng.close()


def test_hash_follows_the_finished_half():
    """after a work list with SAO the finished picture lives in the other half of the allocation: the hash is of what oh_pic_download returns"""
    from openhevc_amd.engine import Engine, remap_frame
    eng = Engine(0)
    rec = F.Recorder(params(416, 240, 8, 1))
    f = rec.synth(F.synth_params(0, 3, sao_pct=90), 0)
    pid = eng.pic_alloc(f.p)
    eng.frame_submit(remap_frame(f, {0: pid}))
    assert eng.pic_final_half(pid) == 1
    hp = eng.pic_download(pid, f.p)
    for t in (0, 1, 2):
        assert eng.pics_hash([pid], t) == [PH.host_pic_hash(hp, f.p, t)], t
    eng.close()
    rec.close()


def test_arguments():
    from openhevc_amd.engine import Engine, EngineError
    eng = Engine(0)
    p = params(64, 64, 8, 1)
    pid = eng.pic_alloc(p)
    eng.pic_upload(pid, F.HostPic(p))
    for t in (0, 1, 2):
        assert eng.pics_hash([], t) == []
    with pytest.raises(EngineError):
        eng.pics_hash([pid + 1000], 1)
    with pytest.raises(EngineError):
        eng.pics_hash([pid], 3)
    with pytest.raises(EngineError):
        eng.pics_hash([pid], -1)
    assert eng.pics_hash([pid], 2) == [PH.host_pic_hash(F.HostPic(p), p, 2)]         # the engine is still usable
    eng.close()


@pytest.mark.timeout(900)
def test_batch_of_32_uhd_main10_pictures():
    """the call tools/hash_rate.py times: 32 pictures of 3840x2160 Main 10 4:2:0 (796 MB) in one oh_pics_hash per type"""
    from openhevc_amd.engine import Engine
    rng = np.random.default_rng(32)
    p = params(3840, 2160, 10, 1)
    base = random_pic(p, rng)
    eng = Engine(0)
    pids, want = [], {1: [], 2: []}
    for k in range(32):
        hp = F.HostPic(p)
        for c in range(3):
            hp.visible(c)[...] = (base.visible(c) + k * 37) & 1023        # a different picture each, cheaply
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        pids.append(pid)
        for t in (1, 2):
            want[t].append(PH.host_pic_hash(hp, p, t))
    for t in (1, 2):
        assert eng.pics_hash(pids, t) == want[t], t
    eng.close()


# ---- the recorded stream fixtures (tests/golden/streams: work lists recorded inside the reference decoder, MD5s of its output) ----
GOLD = os.path.join(HERE, "golden", "streams")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "*.npz")))


def fixture(path):
    z = np.load(path)
    n = int(z["n_pictures"][0])
    frames = []
    for k in range(n):
        pre = f"pic{k}_"
        frames.append(F.FrameFromArrays({key[len(pre):]: z[key] for key in z.files if key.startswith(pre)}))
    return frames, z["md5"].tobytes()


def fixture_stream(path):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_stream_golden as M
    import streamgen
    case = [c for c in M.STREAM_CASES if c[0] == os.path.basename(path)[:-4]][0]
    return streamgen.write_stream(case[1], case[2], case[3], **case[4])


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_stream_fixtures_hash_on_the_gpu(path):
    """replay each fixture on the engine (as test_engine_reproduces_reference_output): GPU MD5 = the fixture's digests, GPU CRC and
    checksum = the host model of the downloaded picture; SEIs written from those values read back equal; a flipped value mismatches in
    exactly its plane"""
    from openhevc_amd.engine import Engine, remap_frame
    frames, want_md5 = fixture(path)
    eng = Engine(0)
    ids, got = {}, {0: [], 1: [], 2: []}
    for ff in frames:
        f = ff.frame
        for i in [f.cur_pic] + [f.ref_pics[k] for k in range(F.OH_MAX_REFS) if f.ref_pics[k] >= 0]:
            if i not in ids:
                ids[i] = eng.pic_alloc(f.p)
        eng.frame_submit(remap_frame(f, ids))
        eng.sync()
        hp = eng.pic_download(ids[f.cur_pic], f.p)
        for t in (0, 1, 2):
            h = eng.pics_hash([ids[f.cur_pic]], t)[0]
            if t:
                assert h == PH.host_pic_hash(hp, f.p, t), (len(got[t]), t)
            got[t].append(h)
    eng.close()
    assert b"".join(b"".join(v) for _, v in got[0]) == want_md5
    data, aus = fixture_stream(path)
    assert len(aus) == len(frames)
    for t in (1, 2):
        vals = [v for _, v in got[t]]
        with_sei, aus2 = PH.add_hash(data, aus, t, vals)
        assert PH.sei_hashes(with_sei, aus2) == got[t]
        k, c = len(vals) // 2, len(vals) % 3
        wrong = [list(v) for v in vals]
        wrong[k][c] ^= 1
        bad, aus3 = PH.add_hash(data, aus, t, wrong)
        read = PH.sei_hashes(bad, aus3)
        diff = [(i, j) for i in range(len(vals)) for j in range(3) if read[i][1][j] != got[t][i][1][j]]
        assert diff == [(k, c)]


# ---- end to end: streams with CRC / checksum SEIs -> hooked reference front end -> work lists -> engine -> oh_pics_hash vs the SEI ----
HOOKED_LIB = os.path.join(ROOT, "oracle", "_ref", "libopenhevc_hooked.so")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libopenhevc_ref.so")
need_front_end = pytest.mark.skipif(not (os.path.exists(HOOKED_LIB) and os.path.exists(REF_LIB)),
                                    reason="the hooked reference front end (oracle/_ref) is not built here")

STREAMS = [
    ("main8_lowdelay", 416, 240, 11, dict(n_pictures=6, gop=2)),
    ("main10_tools", 416, 240, 12, dict(n_pictures=5, gop=2, bit_depth=10, amp=1, pcm=1, transform_skip=1, weighted_pred=1)),
    ("rext422_10b", 264, 200, 20, dict(n_pictures=4, gop=2, chroma_format_idc=2, bit_depth=10, log2_ctb_size=4, log2_max_tb_size=4, sao_pct=90)),
    ("hier_b_reordered", 416, 240, 18, dict(n_pictures=7, gop=3, tmvp=1, n_refs=3)),
]


@need_front_end
@pytest.mark.parametrize("case", STREAMS, ids=[c[0] for c in STREAMS])
def test_engine_pictures_match_crc_and_checksum_seis(case):
    import refdec
    import streamgen
    from openhevc_amd.engine import Engine, remap_frame
    name, w, h, seed, kw = case
    data, aus = streamgen.write_stream(w, h, seed, **kw)
    pics = refdec.decode(data)                                # output order
    n = kw["n_pictures"]
    rank = streamgen.output_rank(n, kw.get("gop", 2), kw.get("idr_period", 0))
    bd = kw.get("bit_depth", 8)
    for t in (1, 2):
        vals = [PH.picture_hash(pics[rank[k]], bd, t)[1] for k in range(n)]   # the SEI of an access unit describes ITS picture
        with_sei, aus2 = PH.add_hash(data, aus, t, vals)
        seis = PH.sei_hashes(with_sei, aus2)
        eng = Engine(0)
        ids, got = {}, []

        def on_picture(f, cur, poc):
            for i in [cur] + [f.ref_pics[k] for k in range(F.OH_MAX_REFS) if f.ref_pics[k] >= 0]:
                if i not in ids:
                    ids[i] = eng.pic_alloc(f.p)
            eng.frame_submit(remap_frame(f, ids))
            got.append(eng.pics_hash([ids[cur]], t)[0])
        assert refdec.record_work_lists(with_sei, on_picture) == n
        eng.close()
        assert got == seis, (name, t)
        assert all(s is not None and s[0] == t for s in seis)
